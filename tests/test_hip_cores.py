"""GPU: the k-core decomposition of posterior samples and of given networks on the device (vmr_sample_cores, vmr_network_cores),
held to the NumPy restatement (tests/cores_util.py) of the samples `CaviEngine.sample` returns for the same seeds.  Coreness is an
integer: every comparison is `==`.  Designed networks at every word boundary, a deep peel, k jumping over empty shells, the node
bound; both data layouts, the general kernels (K = 12), a coordinate-list handle; several chunks, two runs, every optional output
on its own, the argument errors, and the model's method."""
import warnings

import numpy as np
import pytest

from tests.cores_util import (CORE_KEYS, MODES, adjacency, core_peel, cores_np, mixed_design, mixed_design_cores, path, random_planted,
                              reduce_values)
from tests.golden_util import case_config, load_case
from tests.test_hip_betweenness import _stateless
from tests.test_hip_centrality import _engine_with_rho, _medium_case
from tests.test_hip_netstats import _engine_for, _golden_state

pytestmark = pytest.mark.gpu

ALL_KEYS = CORE_KEYS + ("values",)
SUMMARY = ("degeneracy", "main_core_size", "core_sum", "kcore_size")


def _assert_equal_cores(got, want, keys=ALL_KEYS):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), k


def _check(eng, seed, S, trials=(1,), k_min=2, top_k=3):
    """`sample_cores` against the restatement on the samples of the same seeds -- the values and, from them, the summary and all
    six per-node reductions -- and `network_cores` of the same samples; returns {mode: result}."""
    res = {}
    for n_trials in trials:
        Ys = np.asarray([eng.sample(seed + s, n_trials) for s in range(S)])
        for m in MODES:
            want = cores_np(Ys, m, k_min, top_k)
            got = eng.sample_cores(seed, S, mode=m, k_min=k_min, top_k=top_k, n_trials=n_trials, values=True)
            assert sorted(got) == sorted(ALL_KEYS)
            _assert_equal_cores(got, want)
            _assert_equal_cores(got, reduce_values(got["values"], k_min, top_k), keys=CORE_KEYS)
            vals, sm = eng.network_cores(Ys, mode=m, k_min=k_min, summary=True)
            assert np.array_equal(vals, got["values"]), m
            for k in SUMMARY:
                assert np.array_equal(sm[k], got[k]), (m, k)
            res[m] = got
    return res


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


def test_values_against_the_restatement_general_kernels():
    d = load_case("L_default_K12")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    assert K > 8
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        _check(eng, 5, 8)
    finally:
        eng.close()


def test_values_against_the_restatement_coo_handle():
    d = load_case("D_self_mask")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d), coo=True)
    try:
        _check(eng, 3, 8)
    finally:
        eng.close()


def _check_networks(N, Ys, k_min=1):
    """`network_cores` of the networks Ys [n][N, N] (L = 1) on a handle with no state, every mode, values and summary."""
    Y4 = np.asarray(Ys)[:, None]
    eng = _stateless(1, N)
    try:
        for m in MODES:
            want = cores_np(Y4, m, k_min, 1)
            vals, sm = eng.network_cores(Y4, mode=m, k_min=k_min, summary=True)
            assert vals.dtype == np.uint16 and vals.shape == (len(Y4), 1, N)
            assert np.array_equal(vals, want["values"]), (N, m)
            for k in SUMMARY:
                assert sm[k].dtype == np.int64 and np.array_equal(sm[k], want[k]), (N, m, k)
            assert np.array_equal(eng.network_cores(Y4[0], mode=MODES.index(m)), want["values"][0])      # one network, no summary
    finally:
        eng.close()


@pytest.mark.parametrize("N", [63, 64, 65, 129, 257])
def test_word_boundaries(N):
    """W = ceil(N / 64) = 1, 1, 2, 3, 5 words per bit row, a thread owns one or two nodes: random digraphs with 2 and with N / 4
    ties per node, random diagonal entries, a planted clique that holds the last node.  These are the boundaries of the first
    five words only: one to four lanes per row.  8 and 16 lanes, a second trip of the word stride behind them and three to five
    nodes per thread are held in tests/test_hip_graph_shapes.py."""
    sparse, dense = random_planted(N, 2.0, 6, N), random_planted(N, N / 4.0, 3, 2 * N)
    assert sparse.diagonal().any() and dense.diagonal().any()
    assert core_peel(adjacency(dense), "union")[0].max() >= N // 4 and core_peel(adjacency(sparse), "union")[0][N - 1] == 5
    _check_networks(N, [sparse, dense], k_min=3)


def test_deep_peel_and_jumps():
    """N = 300.  The path of 300: one jump, then 150 rounds that remove two nodes each.  The 40-clique beside a path, a mutual
    pair and isolated nodes: k jumps 0 -> 1 -> 39 (78 for total), the pair's nodes leave in the same round, a mutual neighbour
    loses 2 under total; the closed forms are met."""
    N = 300
    assert core_peel(adjacency(path(N)), "union")[1] == 151
    _check_networks(N, [path(N), mixed_design(N), path(N).T, np.zeros((N, N), np.uint8)])
    eng = _stateless(1, N)
    try:
        closed = mixed_design_cores(N)
        for m in MODES:
            vals, sm = eng.network_cores(mixed_design(N)[None], mode=m, k_min=2, summary=True)
            assert np.array_equal(vals[0], closed[m]), m
            assert sm["degeneracy"][0] == closed[m].max() and sm["main_core_size"][0] == 40 and sm["core_sum"][0] == closed[m].sum()
            assert sm["kcore_size"][0] == (42 if m == "total" else 40)
        assert np.array_equal(eng.network_cores(path(N)[None] * 7, "union")[0], np.ones(N))             # entries > 0 are ties
        assert not eng.network_cores(path(N)[None], "in").any() and not eng.network_cores(path(N)[None], "out").any()
    finally:
        eng.close()


def test_one_hot_rho_draws_the_design():
    """A one-hot rho: every sample is the design whatever the seed, and `sample_cores` equals `network_cores`."""
    N, S = 300, 3
    Y = np.stack([mixed_design(N), path(N)])
    rho = np.stack([1.0 - (Y > 0), Y > 0], axis=-1).astype(np.float64)
    eng = _engine_with_rho(rho, 3)
    try:
        assert np.array_equal(eng.sample(40) > 0, Y > 0)
        for m in MODES:
            got = eng.sample_cores(40, S, mode=m, k_min=1, top_k=40, values=True)
            net = eng.network_cores(Y, mode=m)
            assert np.array_equal(net[0], mixed_design_cores(N)[m])
            for s in range(S):
                assert np.array_equal(got["values"][s], net), (m, s)
            _assert_equal_cores(got, cores_np([Y] * S, m, 1, 40))
            assert np.array_equal(got["node_top"][0, :40], np.full(40, S)) and not got["node_top"][0, 40:].any()
    finally:
        eng.close()


def test_medium_case_chunks_and_reruns(monkeypatch):
    """L = 2, N = 300, K = 3 on report lists, S = 12: one chunk against chunks of 5 samples (12 = 5 + 5 + 2) and against a second
    run, every array identical; the first samples against the restatement."""
    X, st = _medium_case()
    seed, S = 1000, 12
    monkeypatch.setenv("VMR_FORMAT", "sparse")
    monkeypatch.delenv("VMR_NETSTATS_CHUNK", raising=False)
    eng = _engine_for(X, None, 3, True, st)
    try:
        one = {m: eng.sample_cores(seed, S, mode=m, k_min=60, top_k=10, values=True) for m in MODES}
        again = {m: eng.sample_cores(seed, S, mode=m, k_min=60, top_k=10, values=True) for m in MODES}
        Ys = np.asarray([eng.sample(seed + s) for s in range(2)])
    finally:
        eng.close()
    for m in MODES:
        _assert_equal_cores(again[m], one[m])
        assert np.array_equal(one[m]["values"][:2], cores_np(Ys, m)["values"]), m
        _assert_equal_cores(one[m], reduce_values(one[m]["values"], 60, 10), keys=CORE_KEYS)
    assert one["union"]["degeneracy"].min() >= 2
    monkeypatch.setenv("VMR_NETSTATS_CHUNK", "5")
    eng = _engine_for(X, None, 3, True, st)
    try:
        many = {m: eng.sample_cores(seed, S, mode=m, k_min=60, top_k=10, values=True) for m in MODES}
        again = {m: eng.sample_cores(seed, S, mode=m, k_min=60, top_k=10, values=True) for m in MODES}
    finally:
        eng.close()
    for m in MODES:
        _assert_equal_cores(many[m], one[m])
        _assert_equal_cores(again[m], one[m])


def test_networks_across_chunk_boundaries(monkeypatch):
    """The upload loop `network_betweenness` and `network_cores` share, on a handle with no state: L = 2, N = 65 (two words per
    bit row), seven random networks with diagonal entries, in one chunk and in chunks of 3 + 3 + 1 on a fresh handle (the switch is
    read once per handle).  Every array is the same bytes in both runs; the coreness and its summary equal the restatement, the
    betweenness is held to its restatement by the bound tests/test_hip_betweenness.py derives (the blocks' sums associate
    differently from NumPy's)."""
    from tests.betweenness_util import DIRECTIONS, betweenness_np
    from tests.test_hip_betweenness import _assert_values
    L, N, n = 2, 65, 7
    rng = np.random.RandomState(65)
    Y = (rng.random_sample((n, L, N, N)) < 3.0 / N).astype(np.uint8) * rng.randint(1, 4, (n, L, N, N)).astype(np.uint8)
    Y[:, :, np.arange(0, N, 3), np.arange(0, N, 3)] = 1
    Y[:, :, N - 1, 0], Y[:, :, 1, N - 1] = 1, 2
    assert Y[..., N - 1].any(axis=-1).all() and Y[..., N - 1, :].any(axis=-1).all()      # the second word's node has ties both ways

    def run():
        eng = _stateless(L, N)
        try:
            out = {("btw", d): eng.network_betweenness(Y, direction=d) for d in DIRECTIONS}
            for m in MODES:
                vals, sm = eng.network_cores(Y, mode=m, k_min=2, summary=True)
                out[("cores", m)] = vals
                out.update({("cores", m, k): sm[k] for k in SUMMARY})
            return out
        finally:
            eng.close()

    monkeypatch.delenv("VMR_NETSTATS_CHUNK", raising=False)
    one = run()
    monkeypatch.setenv("VMR_NETSTATS_CHUNK", "3")
    many = run()
    assert len(one) == len(many) == 2 + 4 * 5
    for k in one:
        assert one[k].dtype == many[k].dtype and one[k].shape == many[k].shape and one[k].tobytes() == many[k].tobytes(), k
    for d in DIRECTIONS:
        assert one[("btw", d)].shape == (n, L, N) and one[("btw", d)].dtype == np.float64
        assert (one[("btw", d)] > 0).any(axis=-1).all()
        _assert_values(one[("btw", d)], betweenness_np(Y, d)["values"], N, "chunked networks " + d)
    for m in MODES:
        want = cores_np(Y, m, 2, 1)
        assert one[("cores", m)].dtype == np.uint16 and np.array_equal(one[("cores", m)], want["values"]), m
        for k in SUMMARY:
            assert one[("cores", m, k)].dtype == np.int64 and np.array_equal(one[("cores", m, k)], want[k]), (m, k)


def test_the_node_bound():
    """N = CORE_NMAX: one network, 3 ties per node and a planted 64-clique that holds node N - 1 -- 32 words per bit row, threads
    own eight nodes -- against the restatement, every mode."""
    from vimure_amd import _lib
    N = _lib.CORE_NMAX
    Y = random_planted(N, 3.0, 64, 8)
    assert core_peel(adjacency(Y), "union")[0].max() == 63
    _check_networks(N, [Y], k_min=4)


def test_more_nodes_than_the_bound_are_refused():
    """A coordinate-list handle of VMR_CORE_NMAX + 1 nodes and no state: both calls refuse it for its N, not for its state."""
    from vimure_amd import _lib
    from vimure_amd.engine import CoresArgumentError
    N = _lib.CORE_NMAX + 1
    eng = _stateless(1, N)
    try:
        with pytest.raises(CoresArgumentError, match="vmr_sample_cores.*N <= %d" % _lib.CORE_NMAX):
            eng.sample_cores(1, 2)
        with pytest.raises(CoresArgumentError, match="vmr_network_cores.*N <= %d" % _lib.CORE_NMAX):
            eng.network_cores(np.zeros((1, N, N), np.uint8))
        ns = np.zeros((1, N))
        assert eng.lib.vmr_sample_cores(eng._h, 1, 2, 1, 0, 0, 1, ns.ctypes.data, *[None] * 7) == _lib.VMR_EINVAL
        assert b"N <= %d" % _lib.CORE_NMAX in eng.lib.vmr_last_error(eng._h) and b"LDS" in eng.lib.vmr_last_error(eng._h)
    finally:
        eng.close()


def test_optional_outputs():
    """node_sum alone, and node_sum with each other output alone (the raw call, the others NULL)."""
    from vimure_amd import _lib
    d = load_case("B_random_mask_K3")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        S, top_k, k_min = 4, 3, 2
        full = eng.sample_cores(9, S, mode="total", k_min=k_min, top_k=top_k, values=True)
        plain = eng.sample_cores(9, S, mode="total", k_min=k_min, top_k=top_k)
        assert sorted(plain) == sorted(CORE_KEYS)
        _assert_equal_cores(plain, full, keys=CORE_KEYS)
        L, N = eng.L, eng.N
        outs = [("node_sumsq", np.full((L, N), -1.0)), ("node_rank_sum", np.full((L, N), 7, np.uint64)),
                ("node_top", np.full((L, N), 7, np.uint32)), ("node_main", np.full((L, N), 7, np.uint32)),
                ("node_atleast", np.full((L, N), 7, np.uint32)), ("summary", np.full((S, L, 4), 7, np.uint32)),
                ("values", np.full((S, L, N), 7, np.uint16))]
        for pick in [None] + list(range(len(outs))):
            ns = np.full((L, N), -1.0)
            ptrs = [a.ctypes.data if i == pick else None for i, (_, a) in enumerate(outs)]
            assert eng.lib.vmr_sample_cores(eng._h, 9, S, 1, 1, k_min, top_k, ns.ctypes.data, *ptrs) == _lib.VMR_OK
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
    from vimure_amd.engine import CoresArgumentError, EngineError
    d = load_case("A_ones_mut")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, None)
    try:
        L, N = eng.L, eng.N
        ns, vals, Y = np.zeros((L, N)), np.full((1, L, N), 9, np.uint16), np.zeros((1, L, N, N), np.uint8)
        nul = [None] * 7

        def raw(S=2, n_trials=1, md=0, k_min=0, top_k=1, nsp=ns.ctypes.data):
            return eng.lib.vmr_sample_cores(eng._h, 1, S, n_trials, md, k_min, top_k, nsp, *nul)

        def raw_net(Yp=Y.ctypes.data, n=1, md=0, k_min=0, out=vals.ctypes.data):
            return eng.lib.vmr_network_cores(eng._h, Yp, n, md, k_min, out, None)

        bad = ((raw, {"S": 0}, b"n_samples"), (raw, {"n_trials": 0}, b"n_trials"), (raw, {"md": 4}, b"mode"), (raw, {"md": -1}, b"mode"),
               (raw, {"k_min": -1}, b"k_min"), (raw, {"k_min": 2 * N - 1}, b"k_min"), (raw, {"top_k": 0}, b"top_k"),
               (raw, {"top_k": N + 1}, b"top_k"), (raw, {"nsp": None}, b"node_sum"),
               (raw_net, {"n": 0}, b"n must"), (raw_net, {"md": 4}, b"mode"), (raw_net, {"k_min": 2 * N - 1}, b"k_min"),
               (raw_net, {"Yp": None}, b"Y is NULL"), (raw_net, {"out": None}, b"values is NULL"))
        # before vmr_set_state: the state is what is missing, unless an argument is refused first; the networks' call needs none
        with pytest.raises(EngineError, match="vmr_set_state") as ei:
            eng.sample_cores(1, 2)
        assert not isinstance(ei.value, CoresArgumentError)
        assert raw() == _lib.VMR_ESTATE and raw_net() == _lib.VMR_OK and not vals.any()
        for fn, kw, word in bad:
            assert fn(**kw) == _lib.VMR_EINVAL, kw
            err = eng.lib.vmr_last_error(eng._h)
            assert word in err and (b"vmr_sample_cores" if fn is raw else b"vmr_network_cores") in err, (kw, err)
        eng.set_state(*_golden_state(d))
        for fn, kw, word in bad:
            assert fn(**kw) == _lib.VMR_EINVAL and word in eng.lib.vmr_last_error(eng._h), (kw, word)
        for kw, word in (({"n_samples": 0}, "n_samples"), ({"n_trials": 0}, "n_trials"), ({"top_k": 0}, "top_k"), ({"top_k": N + 1}, "top_k"),
                         ({"k_min": -1}, "k_min"), ({"k_min": 2 * N - 1}, "k_min"), ({"mode": "directed"}, "mode"), ({"mode": 4}, "mode"),
                         ({"mode": -1}, "mode")):
            args = dict(seed=1, n_samples=2)
            args.update(kw)
            with pytest.raises(CoresArgumentError, match=word):
                eng.sample_cores(**args)
        with pytest.raises(CoresArgumentError, match="mode"):
            eng.network_cores(Y[0], mode="both")
        with pytest.raises(CoresArgumentError, match="shape"):
            eng.network_cores(np.zeros((L, N, N + 1), np.uint8))
        # the ends of every range are accepted, and the handle still works
        got = eng.sample_cores(1, 2, mode=3, k_min=2 * (N - 1), top_k=N)
        assert got["node_sum"].shape == (L, N) and not got["node_atleast"].any() and np.array_equal(got["node_top"], np.full((L, N), 2))
        got = eng.sample_cores(1, 1, mode=0, k_min=0, top_k=1)
        assert got["degeneracy"].shape == (1, L) and np.array_equal(got["kcore_size"], np.full((1, L), N))
    finally:
        eng.close()


def test_model_posterior_cores():
    from vimure_amd import VimureModel
    from vimure_amd.synthetic import standard_sbm
    net = standard_sbm(N=60, M=8, L=1, K=2, avg_degree=6.0, eta=0.4, seed=4)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = VimureModel(mutuality=True)
        m.fit(net.X, K=2, seed=1, max_iter=30, num_realisations=1, keep_engine=True)
    try:
        S, sd = 8, 321
        res = m.posterior_cores(mode="union", n_samples=S, seed=sd, top_k=5, values=True)
        assert m._rho_f is None                                           # rho has not crossed PCIe
        Yinf = m.get_inferred_model()
        inf = cores_np([Yinf], "union")["values"][0]
        assert inf.max() >= 2
        assert res.inferred.shape == (m.L, m.N) and np.array_equal(res.inferred, inf)
        assert np.array_equal(res.inferred, m._engine.network_cores(Yinf))
        assert res.k_min == inf.max(axis=1).min() and res.mode == "union"
        Ys = np.asarray([m.sample_inferred_model(N=1, seed=sd + s, device=True)[0] for s in range(S)])
        want = cores_np(Ys, "union", res.k_min, 5)
        assert res.values.shape == (S, m.L, m.N) and np.array_equal(res.values, want["values"])
        for k in CORE_KEYS:
            assert np.array_equal(getattr(res, k), want[k]), k
        for name in ("mean", "sd", "expected_rank", "top_prob", "main_core_prob", "kcore_prob"):
            assert getattr(res, name).shape == (m.L, m.N), name
        for name in ("degeneracy", "main_core_size", "kcore_size"):
            assert getattr(res, name).shape == (S, m.L), name
        for p in (res.top_prob, res.main_core_prob, res.kcore_prob):
            assert (p >= 0).all() and (p <= 1).all()
        assert res.main_core_prob.max() > 0 and np.array_equal(res.mean, want["node_sum"] / S)
        assert res.top(5).shape == (5,) and res.core_members().shape == (m.L, m.N)
        assert len(res.frame()) == m.L * m.N and len(res.summary()) == 4 * m.L
        tot = m.posterior_cores(mode="total", k=3, n_samples=S, seed=sd)
        assert tot.values is None and tot.k_min == 3
        assert np.array_equal(tot.node_atleast, m._engine.sample_cores(sd, S, mode="total", k_min=3)["node_atleast"])
    finally:
        m.close()
