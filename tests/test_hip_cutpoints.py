"""GPU: cut points, bridges and fragmentation of posterior samples and of given networks on the device (vmr_sample_cutpoints,
vmr_network_cutpoints), held to the restatement (tests/cutpoints_util.py) of the samples `CaviEngine.sample` returns for the same
seeds.  Everything is an integer: every comparison is `==`.  Both modes everywhere.  Both data layouts, the general kernels, a
coordinate-list handle; the word boundaries with graphs that are not trivial; designed graphs with closed forms; the wider launch
shapes; several chunks, two runs; the node bound; every optional output on its own, the argument errors, and the model's method."""
import warnings

import numpy as np
import pytest

from tests.cutpoints_util import (CUT_KEYS, CUT_VALUES, MODES, SUMMARY, all_designed, cutpoints_np, designed_closed_forms, graph,
                                  reduce_values)
from tests.golden_util import case_config, load_case
from tests.test_hip_betweenness import _stateless
from tests.test_hip_centrality import _coo_engine_with_rho, _engine_with_rho, _medium_case
from tests.test_hip_netstats import _engine_for, _golden_state
from vimure_amd.engine import CutpointArgumentError, EngineError

pytestmark = pytest.mark.gpu

ALL_KEYS = CUT_KEYS + CUT_VALUES
REDUCED = tuple(k for k in CUT_KEYS if k != "connected_pairs")


def _assert_equal_cut(got, want, keys=ALL_KEYS):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, got[k].dtype, want[k].dtype, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), k


def _check_mode(eng, Ys, seed, mode, top_k=3, n_trials=1):
    """`sample_cutpoints` against the restatement of the samples Ys of the same seeds -- the values and, from them, the summary and
    all seven per-node reductions -- and `network_cutpoints` of the same samples; returns the restatement."""
    S = len(Ys)
    want = cutpoints_np(Ys, mode, top_k)
    got = eng.sample_cutpoints(seed, S, mode=mode, top_k=top_k, n_trials=n_trials, values=True)
    assert sorted(got) == sorted(ALL_KEYS)
    _assert_equal_cut(got, want)
    _assert_equal_cut(got, reduce_values(got["pairs_cut"], got["branches"], got["bridges"], top_k), keys=REDUCED)
    net = eng.network_cutpoints(Ys, mode=MODES.index(mode), summary=True)
    assert sorted(net) == sorted(CUT_VALUES + SUMMARY)
    _assert_equal_cut(net, got, keys=CUT_VALUES + SUMMARY)
    return want


def _check(eng, seed, S, trials=(1,), top_k=3):
    for n_trials in trials:
        Ys = np.asarray([eng.sample(seed + s, n_trials) for s in range(S)])
        for m in MODES:
            _check_mode(eng, Ys, seed, m, top_k, n_trials)


@pytest.mark.parametrize("case", ["A_ones_mut", "B_random_mask_K3", "D_self_mask", "E_undirected"])
def test_values_against_the_restatement(case, vmr_format):
    d = load_case(case)
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        assert eng.data_format()[0] == vmr_format
        _check(eng, 11, 8, trials=(1, 3))
    finally:
        eng.close()


@pytest.mark.parametrize("case", ["L_default_K12", "M_K16_nomut"])
def test_values_against_the_restatement_general_kernels(case):
    d = load_case(case)
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    assert K > 8
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        _check(eng, 5, 8, trials=(1, 3))
    finally:
        eng.close()


def test_values_against_the_restatement_coo_handle():
    d = load_case("D_self_mask")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d), coo=True)
    try:
        _check(eng, 3, 8, trials=(1, 3))
    finally:
        eng.close()


def _tie_rho(L, N, K, mode):
    """rho [L, N, N, K] with the same mass on a tie everywhere: 1.5 / N for "union"; sqrt(2 / N) for "mutual" -- the two
    directions are drawn independently, so the reciprocated network then has about 2 ties per node (at 1.5 / N it would be empty)."""
    p = 1.5 / N if mode == "union" else np.sqrt(2.0 / N)
    rho = np.empty((L, N, N, K))
    rho[..., 0] = 1.0 - p
    rho[..., 1:] = p / (K - 1)
    return rho


def _assert_not_trivial(want, Ys, mode):
    """From the restatement, not from the device: in every layer, over the samples, at least 4 cut points in some sample, a node
    with 3 or more branches, a non-cut node that has a tie, at least one bridge, two cut points with different pairs_cut."""
    S, L = want["n_cut"].shape
    for l in range(L):
        b, p = want["branches"][:, l].astype(np.int64), want["pairs_cut"][:, l].astype(np.int64)
        assert want["n_cut"][:, l].max() >= 4, (mode, l, want["n_cut"][:, l])
        assert b.max() >= 3, (mode, l, b.max())
        assert any(((b[s] == 1) & graph(Ys[s, l], mode).any(axis=1)).any() for s in range(S)), (mode, l)
        assert want["n_bridges"][:, l].max() >= 1, (mode, l)
        assert any(np.unique(p[s][b[s] >= 2]).size >= 2 for s in range(S)), (mode, l)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N", [5, 63, 64, 65, 129])
def test_word_boundaries(N, mode):
    """L = 2, K = 3, S = 8 and W = ceil(N / 64) = 1, 1, 1, 2, 3 words per bit row and as many blocks of 64 removal experiments, at
    the density where a random graph is full of cut points and bridges."""
    L, K, S, seed = 2, 3, 8, 7
    eng = _engine_with_rho(_tie_rho(L, N, K, mode), 100 + N)
    try:
        Ys = np.asarray([eng.sample(seed + s) for s in range(S)])
        assert Ys[:, :, np.arange(N), np.arange(N)].any()             # clearing the diagonal is exercised
        want = _check_mode(eng, Ys, seed, mode)
        if N >= 63:
            _assert_not_trivial(want, Ys, mode)
    finally:
        eng.close()


def test_designed_graphs():
    """One-hot rho, N = 129, L = 8, K = 2: every sample is the design whatever the seed.  device == closed forms == restatement,
    by the sampled call and by `network_cutpoints`, on a handle with a state and on one without."""
    Y = all_designed()
    rho = np.stack([1.0 - Y, Y], axis=-1).astype(np.float64)
    eng = _engine_with_rho(rho, 3)
    bare = _stateless(8, 129)
    try:
        assert np.array_equal(eng.sample(40), Y)
        for m in MODES:
            closed = designed_closed_forms(m)
            want = cutpoints_np([Y, Y], m, top_k=5)
            got = eng.sample_cutpoints(40, 2, mode=m, top_k=5, values=True)
            _assert_equal_cut(got, want)
            for e in (eng, bare):
                net = e.network_cutpoints(Y, mode=m, summary=True)
                for k in CUT_VALUES:
                    assert np.array_equal(net[k], closed[k]), (m, k)
                    assert np.array_equal(got[k][0], net[k]) and np.array_equal(got[k][1], net[k]), (m, k)
                for k in SUMMARY:
                    assert np.array_equal(net[k], closed[k]) and np.array_equal(got[k], [closed[k]] * 2), (m, k)
            many = bare.network_cutpoints(np.stack([Y, Y[::-1], Y]), mode=m)
            for k in CUT_VALUES:
                assert np.array_equal(many[k][0], closed[k]) and np.array_equal(many[k][1], closed[k][::-1]) and np.array_equal(many[k][2], closed[k])
    finally:
        eng.close()
        bare.close()


def test_wider_launch_shape_five_words():
    """N = 300, L = 2, K = 3, S = 2: five words per bit row -- G = 4 lanes to a row with a second trip of the word stride -- two
    nodes per thread, five blocks of removal experiments; both modes at their densities."""
    N, L, K, S, seed = 300, 2, 3, 2, 21
    for m in MODES:
        eng = _engine_with_rho(_tie_rho(L, N, K, m), 300, M=2)
        try:
            Ys = np.asarray([eng.sample(seed + s) for s in range(S)])
            want = _check_mode(eng, Ys, seed, m, top_k=10)
            assert want["n_cut"].min() >= 4 and want["n_bridges"].min() >= 1 and want["branches"].max() >= 3, m
        finally:
            eng.close()


def test_wider_launch_shape_eighteen_words():
    """N = 1100, L = 1, K = 2, S = 2 on a coordinate-list handle: 18 words per bit row -- G = 16 lanes with a second trip -- five
    nodes per thread, 18 blocks of removal experiments; both modes at their densities."""
    N, S, seed = 1100, 2, 5
    for m in MODES:
        eng = _coo_engine_with_rho(_tie_rho(1, N, 2, m))
        try:
            Ys = np.asarray([eng.sample(seed + s) for s in range(S)])
            want = _check_mode(eng, Ys, seed, m, top_k=20)
            assert want["n_cut"].min() >= 20 and want["branches"].max() >= 3, m
        finally:
            eng.close()


def test_medium_case_chunks_and_reruns(monkeypatch):
    """L = 2, N = 300, K = 3 on report lists, S = 16: one chunk against chunks of 5 samples (16 = 5 + 5 + 5 + 1) and against a
    second run, every array identical; the first samples against the restatement; `sample_stats`, `sample_connectivity` and
    `sample_cores` of the same engine are what they were before the calls."""
    X, st = _medium_case()
    seed, S = 1000, 16
    monkeypatch.setenv("VMR_FORMAT", "sparse")
    monkeypatch.delenv("VMR_NETSTATS_CHUNK", raising=False)

    def others(eng):
        out = dict(eng.sample_stats(seed, S, degrees=True), **eng.sample_connectivity(seed, S, nodes=True))
        out.update({"cores_" + k: v for k, v in eng.sample_cores(seed, S, values=True).items()})
        return out

    eng = _engine_for(X, None, 3, True, st)
    try:
        before = others(eng)
        one = {m: eng.sample_cutpoints(seed, S, mode=m, top_k=10, values=True) for m in MODES}
        again = {m: eng.sample_cutpoints(seed, S, mode=m, top_k=10, values=True) for m in MODES}
        after = others(eng)
        Ys = np.asarray([eng.sample(seed + s) for s in range(2)])
    finally:
        eng.close()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    for m in MODES:
        _assert_equal_cut(again[m], one[m])
        want = cutpoints_np(Ys, m)
        for k in CUT_VALUES + SUMMARY:
            assert np.array_equal(one[m][k][:2], want[k]), (m, k)
        _assert_equal_cut(one[m], reduce_values(one[m]["pairs_cut"], one[m]["branches"], one[m]["bridges"], 10), keys=REDUCED)
    monkeypatch.setenv("VMR_NETSTATS_CHUNK", "5")
    eng = _engine_for(X, None, 3, True, st)
    try:
        many = {m: eng.sample_cutpoints(seed, S, mode=m, top_k=10, values=True) for m in MODES}
        again = {m: eng.sample_cutpoints(seed, S, mode=m, top_k=10, values=True) for m in MODES}
    finally:
        eng.close()
    for m in MODES:
        _assert_equal_cut(many[m], one[m])
        _assert_equal_cut(again[m], one[m])


def test_the_node_bound():
    """N = CUT_NMAX = 2048: L = 1, K = 2, S = 2, rho_1 = 3 / N on a coordinate-list handle with no dense array anywhere -- 32 words
    per bit row, threads own eight nodes, 48 KiB of LDS, 32 blocks of removal experiments -- in "union" against the restatement."""
    from vimure_amd import _lib
    N, S = _lib.CUT_NMAX, 2
    assert N == 2048
    rho = np.empty((1, N, N, 2))
    rho[..., 1] = 3.0 / N
    rho[..., 0] = 1.0 - 3.0 / N
    eng = _coo_engine_with_rho(rho)
    try:
        Ys = np.asarray([eng.sample(5 + s) for s in range(S)])
        assert Ys[:, 0, N - 1].any() and Ys[:, 0, :, N - 1].any()      # the last node has ties both ways
        want = _check_mode(eng, Ys, 5, "union", top_k=N)
        assert want["n_cut"].min() >= 20 and want["branches"].max() >= 3
        assert np.array_equal(want["node_top"], np.full((1, N), S))     # top_k = N: every node, every sample
    finally:
        eng.close()


def test_more_nodes_than_the_bound_are_refused():
    """A coordinate-list handle of VMR_CUT_NMAX + 1 nodes and no state: both calls refuse it for its N, not for its state."""
    from vimure_amd import _lib
    N = _lib.CUT_NMAX + 1
    eng = _stateless(1, N)
    try:
        with pytest.raises(CutpointArgumentError, match="vmr_sample_cutpoints.*N <= %d" % _lib.CUT_NMAX):
            eng.sample_cutpoints(1, 2)
        with pytest.raises(CutpointArgumentError, match="vmr_network_cutpoints.*N <= %d" % _lib.CUT_NMAX):
            eng.network_cutpoints(np.zeros((1, N, N), np.uint8))
        ns = np.zeros((1, N))
        assert eng.lib.vmr_sample_cutpoints(eng._h, 1, 2, 1, 0, 1, ns.ctypes.data, *[None] * 10) == _lib.VMR_EINVAL
        err = eng.lib.vmr_last_error(eng._h)
        assert b"N <= 2048" in err and b"LDS" in err
    finally:
        eng.close()


def test_optional_outputs():
    """node_sum alone, node_sum with each other output alone (the raw call, the others NULL), and values=False against
    values=True."""
    from vimure_amd import _lib
    d = load_case("B_random_mask_K3")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        S, top_k = 4, 3
        for md, m in enumerate(MODES):
            full = eng.sample_cutpoints(9, S, mode=m, top_k=top_k, values=True)
            plain = eng.sample_cutpoints(9, S, mode=m, top_k=top_k)
            assert sorted(plain) == sorted(CUT_KEYS)
            _assert_equal_cut(plain, full, keys=CUT_KEYS)
            L, N = eng.L, eng.N
            outs = [("node_sumsq", np.full((L, N), -1.0)), ("node_rank_sum", np.full((L, N), 7, np.uint64)),
                    ("node_top", np.full((L, N), 7, np.uint32)), ("node_cut", np.full((L, N), 7, np.uint32)),
                    ("node_branch_sum", np.full((L, N), 7, np.uint64)), ("node_bridge_sum", np.full((L, N), 7, np.uint64)),
                    ("summary", np.full((S, L, 4), 7, np.uint32)), ("pairs_cut", np.full((S, L, N), 7, np.uint32)),
                    ("branches", np.full((S, L, N), 7, np.uint16)), ("bridges", np.full((S, L, N), 7, np.uint16))]
            for pick in [None] + list(range(len(outs))):
                ns = np.full((L, N), -1.0)
                ptrs = [a.ctypes.data if i == pick else None for i, (_, a) in enumerate(outs)]
                assert eng.lib.vmr_sample_cutpoints(eng._h, 9, S, 1, md, top_k, ns.ctypes.data, *ptrs) == _lib.VMR_OK
                assert np.array_equal(ns, full["node_sum"]), pick
                if pick is not None:
                    name, arr = outs[pick]
                    if name == "summary":
                        for q, k in enumerate(SUMMARY):
                            assert np.array_equal(arr[..., q], full[k]), k
                    else:
                        assert np.array_equal(arr.astype(full[name].dtype), full[name]), name
    finally:
        eng.close()


def test_argument_errors_on_a_live_handle():
    from vimure_amd import _lib
    d = load_case("A_ones_mut")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, None)
    try:
        L, N = eng.L, eng.N
        ns, vals, Y = np.zeros((L, N)), np.full((1, L, N), 9, np.uint32), np.zeros((1, L, N, N), np.uint8)
        nul = [None] * 10

        def raw(S=2, n_trials=1, md=0, top_k=1, nsp=ns.ctypes.data):
            return eng.lib.vmr_sample_cutpoints(eng._h, 1, S, n_trials, md, top_k, nsp, *nul)

        def raw_net(Yp=Y.ctypes.data, n=1, md=0, out=vals.ctypes.data):
            return eng.lib.vmr_network_cutpoints(eng._h, Yp, n, md, out, None, None, None)

        bad = ((raw, {"S": 0}, b"n_samples"), (raw, {"n_trials": 0}, b"n_trials"), (raw, {"md": 2}, b"mode"), (raw, {"md": -1}, b"mode"),
               (raw, {"top_k": 0}, b"top_k"), (raw, {"top_k": N + 1}, b"top_k"), (raw, {"nsp": None}, b"node_sum"),
               (raw_net, {"n": 0}, b"n must"), (raw_net, {"md": 2}, b"mode"), (raw_net, {"md": -1}, b"mode"),
               (raw_net, {"Yp": None}, b"Y is NULL"), (raw_net, {"out": None}, b"pairs_cut is NULL"))
        # before vmr_set_state: the state is what is missing, unless an argument is refused first; the networks' call needs none
        with pytest.raises(EngineError, match="vmr_set_state") as ei:
            eng.sample_cutpoints(1, 2)
        assert not isinstance(ei.value, CutpointArgumentError)
        assert raw() == _lib.VMR_ESTATE and raw_net() == _lib.VMR_OK and not vals.any()
        for fn, kw, word in bad:
            assert fn(**kw) == _lib.VMR_EINVAL, kw
            err = eng.lib.vmr_last_error(eng._h)
            assert word in err and (b"vmr_sample_cutpoints" if fn is raw else b"vmr_network_cutpoints") in err, (kw, err)
        eng.set_state(*_golden_state(d))
        for fn, kw, word in bad:
            assert fn(**kw) == _lib.VMR_EINVAL and word in eng.lib.vmr_last_error(eng._h), (kw, word)
        for kw, word in (({"n_samples": 0}, "n_samples"), ({"n_trials": 0}, "n_trials"), ({"top_k": 0}, "top_k"), ({"top_k": N + 1}, "top_k"),
                         ({"mode": "total"}, "mode"), ({"mode": 2}, "mode"), ({"mode": -1}, "mode")):
            args = dict(seed=1, n_samples=2)
            args.update(kw)
            with pytest.raises(CutpointArgumentError, match=word):
                eng.sample_cutpoints(**args)
        with pytest.raises(CutpointArgumentError, match="mode"):
            eng.network_cutpoints(Y[0], mode="both")
        with pytest.raises(CutpointArgumentError, match="shape"):
            eng.network_cutpoints(np.zeros((L, N, N + 1), np.uint8))
        # the ends of every range are accepted, and the handle still works
        got = eng.sample_cutpoints(1, 2, mode=1, top_k=N)
        assert got["node_sum"].shape == (L, N) and np.array_equal(got["node_top"], np.full((L, N), 2))
        got = eng.sample_cutpoints(1, 1, mode=0, top_k=1, n_trials=1)
        assert got["n_cut"].shape == (1, L)
        Ys = np.asarray([eng.sample(1)])
        _assert_equal_cut(got, cutpoints_np(Ys, "union", 1), keys=CUT_KEYS)
    finally:
        eng.close()


def test_model_posterior_cutpoints():
    from vimure_amd import CutpointStats, VimureModel
    from vimure_amd.synthetic import standard_sbm
    net = standard_sbm(N=60, M=8, L=1, K=2, avg_degree=6.0, eta=0.4, seed=4)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = VimureModel(mutuality=True)
        m.fit(net.X, K=2, seed=1, max_iter=30, num_realisations=1, keep_engine=True)
    try:
        S, sd = 8, 321
        stats0 = m.posterior_network_stats(n_samples=S, seed=sd)
        conn0 = m.posterior_connectivity(n_samples=S, seed=sd)
        Yinf = m.get_inferred_model()
        Ys = np.asarray([m.sample_inferred_model(N=1, seed=sd + s, device=True)[0] for s in range(S)])
        for mode in MODES:
            res = m.posterior_cutpoints(mode=mode, n_samples=S, seed=sd, top_k=5, values=True)
            assert isinstance(res, CutpointStats) and res.mode == mode
            assert m._rho_f is None                                           # rho has not crossed PCIe
            inf = m._engine.network_cutpoints(Yinf, mode=mode)
            winf = cutpoints_np([Yinf], mode)
            for k in CUT_VALUES:
                assert res.inferred[k].shape == (m.L, m.N) and np.array_equal(res.inferred[k], inf[k]), (mode, k)
                assert np.array_equal(res.inferred[k], winf[k][0]), (mode, k)
            want = cutpoints_np(Ys, mode, 5)
            for k in CUT_VALUES:
                assert getattr(res, k).shape == (S, m.L, m.N) and np.array_equal(getattr(res, k), want[k]), (mode, k)
            for k in CUT_KEYS:
                assert np.array_equal(getattr(res, k), want[k]), (mode, k)
            for name in ("cut_prob", "mean", "sd", "expected_rank", "top_prob", "mean_branches", "mean_bridges"):
                assert getattr(res, name).shape == (m.L, m.N), name
            for name in SUMMARY:
                assert getattr(res, name).shape == (S, m.L), name
            for p in (res.cut_prob, res.top_prob, res.fragmentation()):
                assert (p >= 0).all() and (p <= 1).all()
            assert np.array_equal(res.mean, want["node_sum"] / S) and np.array_equal(res.cut_prob, want["node_cut"] / S)
            assert res.top(5).shape == (5,) and res.key_players().shape == (m.L, m.N)
            assert len(res.frame()) == m.L * m.N and len(res.summary()) == 4 * m.L
            assert res.quantiles()["n_cut"].shape == (3, m.L)
        plain = m.posterior_cutpoints(n_samples=S, seed=sd)
        assert plain.pairs_cut is None and plain.values is None and plain.top_k == 10
        assert np.array_equal(plain.node_cut, m._engine.sample_cutpoints(sd, S)["node_cut"])
        stats1 = m.posterior_network_stats(n_samples=S, seed=sd)
        conn1 = m.posterior_connectivity(n_samples=S, seed=sd)
        for k in ("edges", "mutual"):
            assert np.array_equal(getattr(stats0, k), getattr(stats1, k)), k
        for k in ("components_w", "giant_w", "reach_pairs", "dist_sum"):
            assert np.array_equal(getattr(conn0, k), getattr(conn1, k)), k
    finally:
        m.close()
