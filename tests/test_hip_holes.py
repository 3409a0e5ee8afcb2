"""GPU: Burt's structural holes of posterior samples and of given networks on the device (vmr_sample_structural_holes,
vmr_network_structural_holes), held to the NumPy restatement (tests/holes_util.py) of the samples `CaviEngine.sample` returns for
the same seeds.  Degree, strength, redundancy and the effective size -- one division of two exact integers -- are compared with
`==`.  The constraint is compared within `constraint_bound(N)` = 8 N 2^-53 relative, whose count of the rounded operations on both
sides is in that function's docstring.  The accumulators, ranks and summaries are held to `reduce_values` of the device's own
values: integers, sums and sums of squares `==`; the summary's two sums within N 2^-53 relative of `math.fsum` (N - 1 additions of
non-negative terms).  Both data layouts, the general kernels (K = 12), a coordinate-list handle; every word boundary and launch
shape; closed forms; several chunks, two runs, every optional output on its own, the argument errors, and the model's method."""
import warnings

import numpy as np
import pytest

from tests.golden_util import case_config, load_case
from tests.holes_util import (ACC_KEYS, MODES, SHAPE_NS, SUM_KEYS, U, VALUE_KEYS, clique_constraint, constraint_bound, designs, holes_loops,
                              holes_np, planted, reduce_values)
from tests.test_hip_betweenness import _stateless
from tests.test_hip_centrality import _engine_with_rho, _medium_case
from tests.test_hip_netstats import _engine_for, _golden_state

pytestmark = pytest.mark.gpu

ALL_KEYS = ACC_KEYS + SUM_KEYS + VALUE_KEYS
INT_VALUES = ("degree", "strength", "redundancy")


def _assert_values(got, want, N, what):
    """The per-network values of the device against the restatement's: integers and effective size `==` (NaN where undefined on
    both sides), the constraint within the bound."""
    for k in INT_VALUES:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)
    undefined = want["degree"] == 0
    assert np.array_equal(np.isnan(got["effective_size"]), undefined) and np.array_equal(np.isnan(got["constraint"]), undefined), what
    assert np.array_equal(got["effective_size"], want["effective_size"], equal_nan=True), what
    g, w = got["constraint"][~undefined], want["constraint"][~undefined]
    assert (np.abs(g - w) <= constraint_bound(N) * w).all(), (what, float(np.max(np.abs(g - w) / w, initial=0.0)) / U)


def _assert_reduction(got, top_k, N, what):
    """The accumulators, the ranks behind them and the summary against `reduce_values` of the device's own values."""
    want = reduce_values(got["degree"], got["effective_size"], got["constraint"], top_k)
    for k in ACC_KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)
    for k in SUM_KEYS:
        assert got[k].shape == want[k].shape and (np.abs(got[k] - want[k]) <= N * U * want[k]).all(), (what, k)


def _assert_bytes(a, b, keys, what=""):
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k)


def _check(eng, seed, S, trials=(1,), top_k=3):
    """`sample_structural_holes` against the restatement of the samples of the same seeds and against `reduce_values` of its own
    values, and `network_structural_holes` of the same samples byte for byte; returns {mode: result}."""
    res = {}
    for n_trials in trials:
        Ys = np.asarray([eng.sample(seed + s, n_trials) for s in range(S)])
        for m in MODES:
            got = eng.sample_structural_holes(seed, S, n_trials=n_trials, mode=m, top_k=top_k, values=True)
            assert sorted(got) == sorted(ALL_KEYS)
            _assert_values(got, holes_np(Ys, m, top_k), eng.N, (m, n_trials))
            _assert_reduction(got, top_k, eng.N, (m, n_trials))
            net = eng.network_structural_holes(Ys, mode=m, summary=True)
            _assert_bytes(net, got, VALUE_KEYS + SUM_KEYS + ("n_defined",), (m, n_trials))
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


def _check_networks(N, Ys):
    """`network_structural_holes` of the networks Ys [n][N, N] (L = 1) on a handle with no state, both modes, values and summary;
    returns {mode: result}."""
    Y4 = np.asarray(Ys)[:, None]
    eng = _stateless(1, N)
    res = {}
    try:
        for m in MODES:
            want = holes_np(Y4, m)
            got = eng.network_structural_holes(Y4, mode=m, summary=True)
            assert sorted(got) == sorted(VALUE_KEYS + SUM_KEYS + ("n_defined",))
            assert got["effective_size"].shape == (len(Y4), 1, N) and got["n_defined"].shape == (len(Y4), 1)
            _assert_values(got, want, N, (N, m))
            assert np.array_equal(got["n_defined"], want["n_defined"])
            for k in SUM_KEYS:
                own = reduce_values(got["degree"], got["effective_size"], got["constraint"], 1)[k]
                assert (np.abs(got[k] - own) <= N * U * own).all(), (N, m, k)
            one = eng.network_structural_holes(Y4[0], mode=MODES.index(m))          # one network, no summary
            assert sorted(one) == sorted(VALUE_KEYS)
            _assert_bytes(one, {k: got[k][0] for k in VALUE_KEYS}, VALUE_KEYS, (N, m))
            res[m] = got
    finally:
        eng.close()
    return res


@pytest.mark.parametrize("N", [63, 64, 65, 129, 257])
def test_word_boundaries(N):
    """W = ceil(N / 64) = 1, 1, 2, 3, 5 words per bit row, one to four lanes per neighbour, one or two rank tiles: a network with 2
    ties per node, which has isolates and nodes with in-ties only, and one with N / 4; both with random diagonal entries, entries >
    1, forced mutual ties and a planted clique that holds node N - 1."""
    assert N in SHAPE_NS
    sparse, dense = planted(N, 2.0, 6, N), planted(N, N / 4.0, 3, 2 * N)
    for Y in (sparse, dense):
        A = (Y > 0) & ~np.eye(N, dtype=bool)
        assert Y.diagonal().any() and Y.max() > 1 and (A & A.T).any() and A[N - 1].sum() >= 2
    A = (sparse > 0) & ~np.eye(N, dtype=bool)
    assert (~A.any(axis=1) & ~A.any(axis=0)).any() and (~A.any(axis=1) & A.any(axis=0)).any()          # isolates; in-ties only
    _check_networks(N, [sparse, dense])


@pytest.mark.parametrize("N", [513, 1024, 1025, 2048, 2049, 4097])
def test_launch_shapes(N):
    """One sparse network each, about 3 ties per node and a planted 16-clique on the last nodes: G = 8 .. 64 lanes per neighbour,
    row i in registers or not, one to three list blocks, a second trip of the word stride, up to 17 rank tiles (`SHAPE_NS`)."""
    assert N in SHAPE_NS
    Y = planted(N, 3.0, 16, N, last=False)
    res = _check_networks(N, [Y])
    for m in MODES:
        assert np.array_equal(res[m]["effective_size"][0, 0, N - 16:] >= 1.0, np.ones(16, bool)) and res[m]["degree"][0, 0, N - 1] >= 15


def test_closed_forms():
    """The designed networks at N = 300, both modes.  Met exactly where they are dyadic rationals: the centre of a star with 256
    leaves (ES = 256, c = 1 / 256), its leaves (1, 1), the path (ends 1, 1; inside 2, 1 / 2), the effective size of a clique's
    node (1).  The clique's constraint, the clique beside a star and the mutual pair with asymmetric spokes are met to the bound,
    against exact rationals.  An all-zero network: every node undefined, #defined = 0, and in the sampled call's ranks 0."""
    from fractions import Fraction
    N = 300
    D = designs(N)
    names = list(D)
    res = _check_networks(N, [D[k] for k in names])
    for m in MODES:
        es, con, nd = res[m]["effective_size"][:, 0], res[m]["constraint"][:, 0], res[m]["n_defined"][:, 0]
        for name in ("star", "mutual star"):
            q = names.index(name)
            assert es[q, 0] == 256.0 and con[q, 0] == 1.0 / 256 and nd[q] == 257
            assert np.array_equal(es[q, 1:257], np.ones(256)) and np.array_equal(con[q, 1:257], np.ones(256)) and np.isnan(es[q, 257:]).all()
            assert res[m]["effective_size_sum"][q, 0] == 512.0 and res[m]["constraint_sum"][q, 0] == 256.0 + 1.0 / 256
        q = names.index("path")
        assert np.array_equal(es[q], np.r_[1.0, np.full(N - 2, 2.0), 1.0]) and np.array_equal(con[q], np.r_[1.0, np.full(N - 2, 0.5), 1.0])
        q = names.index("clique")
        want = clique_constraint(17)
        assert np.array_equal(es[q, N - 17:], np.ones(17)) and nd[q] == 17
        assert all(abs(Fraction(x) - want) <= Fraction(constraint_bound(N)) * want for x in con[q, N - 17:])
        for name in ("clique and star", "pair and spokes"):
            q = names.index(name)
            dl, sl, Rl, ESl, cl = holes_loops(D[name], m)
            for i in range(N):
                if dl[i]:
                    assert es[q, i] == float(ESl[i]) and abs(Fraction(con[q, i]) - cl[i]) <= Fraction(constraint_bound(N)) * cl[i], (name, m, i)
        q = names.index("empty")
        assert nd[q] == 0 and np.isnan(es[q]).all() and np.isnan(con[q]).all() and not res[m]["degree"][q].any()
        assert res[m]["effective_size_sum"][q, 0] == 0.0 and res[m]["constraint_sum"][q, 0] == 0.0
    # node 0 of the clique beside a star bridges them: the least constrained node and the largest effective size of its network
    q = names.index("clique and star")
    assert np.nanargmin(res["union"]["constraint"][q, 0]) == 0 and np.nanargmax(res["union"]["effective_size"][q, 0]) == 0


def test_one_hot_rho_draws_the_design():
    """A one-hot rho: every sample is the design whatever the seed, the sampled call equals the networks' call byte for byte, and
    node_defined is S or 0.  The second layer is empty: every rank there is 0 = #defined, and every node enters the top."""
    N, S = 300, 3
    D = designs(N)
    Y = np.stack([D["pair and spokes"] | D["clique"], D["empty"]])
    rho = np.stack([1.0 - (Y > 0), Y > 0], axis=-1).astype(np.float64)
    eng = _engine_with_rho(rho, 3)
    try:
        assert np.array_equal(eng.sample(40) > 0, Y > 0)
        for m in MODES:
            got = eng.sample_structural_holes(40, S, mode=m, top_k=2, values=True)
            net = eng.network_structural_holes(Y, mode=m, summary=True)
            for s in range(S):
                _assert_bytes({k: got[k][s] for k in VALUE_KEYS + SUM_KEYS + ("n_defined",)}, net, VALUE_KEYS + SUM_KEYS + ("n_defined",), (m, s))
            _assert_values(got, holes_np([Y] * S, m, 2), N, m)
            _assert_reduction(got, 2, N, m)
            assert np.array_equal(got["node_defined"], np.where(net["degree"] > 0, S, 0))
            assert not got["node_rank_sum"][:, 1].any() and np.array_equal(got["node_top"][:, 1], np.full((2, N), S))
            assert not got["node_sum"][:, 1].any() and not got["n_defined"][:, 1].any()
    finally:
        eng.close()


def test_medium_case_chunks_and_reruns(monkeypatch):
    """L = 2, N = 300, K = 3 on report lists, S = 12: one chunk against chunks of 5 samples (12 = 5 + 5 + 2) on a fresh handle, and
    each against a second run: every array is the same bytes, the constraint included; the first samples against the
    restatement."""
    X, st = _medium_case()
    seed, S = 1000, 12
    monkeypatch.setenv("VMR_FORMAT", "sparse")
    monkeypatch.delenv("VMR_NETSTATS_CHUNK", raising=False)
    eng = _engine_for(X, None, 3, True, st)
    try:
        one = {m: eng.sample_structural_holes(seed, S, mode=m, top_k=10, values=True) for m in MODES}
        again = {m: eng.sample_structural_holes(seed, S, mode=m, top_k=10, values=True) for m in MODES}
        Ys = np.asarray([eng.sample(seed + s) for s in range(2)])
    finally:
        eng.close()
    for m in MODES:
        _assert_bytes(again[m], one[m], ALL_KEYS, m)
        _assert_values({k: one[m][k][:2] for k in VALUE_KEYS}, holes_np(Ys, m), 300, m)
        _assert_reduction(one[m], 10, 300, m)
    monkeypatch.setenv("VMR_NETSTATS_CHUNK", "5")
    eng = _engine_for(X, None, 3, True, st)
    try:
        many = {m: eng.sample_structural_holes(seed, S, mode=m, top_k=10, values=True) for m in MODES}
        again = {m: eng.sample_structural_holes(seed, S, mode=m, top_k=10, values=True) for m in MODES}
    finally:
        eng.close()
    for m in MODES:
        _assert_bytes(many[m], one[m], ALL_KEYS, m)
        _assert_bytes(again[m], one[m], ALL_KEYS, m)


def test_networks_across_chunk_boundaries(monkeypatch):
    """The upload loop on a handle with no state: L = 2, N = 65, seven random networks with diagonal entries, in one chunk and in
    chunks of 3 + 3 + 1 on a fresh handle (the switch is read once per handle): the same bytes, and the restatement's values."""
    L, N, n = 2, 65, 7
    Y = np.stack([planted(N, 3.0, 4, 100 + q) for q in range(n * L)]).reshape(n, L, N, N)
    keys = VALUE_KEYS + SUM_KEYS + ("n_defined",)

    def run():
        eng = _stateless(L, N)
        try:
            return {m: eng.network_structural_holes(Y, mode=m, summary=True) for m in MODES}
        finally:
            eng.close()

    monkeypatch.delenv("VMR_NETSTATS_CHUNK", raising=False)
    one = run()
    monkeypatch.setenv("VMR_NETSTATS_CHUNK", "3")
    many = run()
    for m in MODES:
        _assert_bytes(many[m], one[m], keys, m)
        assert one[m]["constraint"].shape == (n, L, N) and one[m]["n_defined"].shape == (n, L)
        _assert_values(one[m], holes_np(Y, m), N, m)


def test_optional_outputs():
    """node_sum alone, and node_sum with each other output alone (the raw call, the others NULL): node_sum is unchanged by the
    others, and every output equals the full call's."""
    from vimure_amd import _lib
    d = load_case("B_random_mask_K3")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        S, top_k = 4, 3
        full = eng.sample_structural_holes(9, S, mode="weighted", top_k=top_k, values=True)
        plain = eng.sample_structural_holes(9, S, mode="weighted", top_k=top_k)
        assert sorted(plain) == sorted(ACC_KEYS + SUM_KEYS)
        _assert_bytes(plain, full, ACC_KEYS + SUM_KEYS)
        L, N = eng.L, eng.N
        undefined = full["degree"] == 0
        outs = [("node_sumsq", np.full((2, L, N), -1.0)), ("node_rank_sum", np.full((2, L, N), 7, np.uint64)),
                ("node_top", np.full((2, L, N), 7, np.uint32)), ("node_defined", np.full((L, N), 7, np.uint32)),
                ("summary", np.full((S, L, 3), -1.0)), ("degree", np.full((S, L, N), 7, np.int32)), ("strength", np.full((S, L, N), 7, np.int32)),
                ("redundancy", np.full((S, L, N), 7, np.uint64)), ("effective_size", np.full((S, L, N), -1.0)),
                ("constraint", np.full((S, L, N), -1.0))]
        for pick in [None] + list(range(len(outs))):
            ns = np.full((2, L, N), -1.0)
            ptrs = [a.ctypes.data if i == pick else None for i, (_, a) in enumerate(outs)]
            assert eng.lib.vmr_sample_structural_holes(eng._h, 9, S, 1, 1, top_k, ns.ctypes.data, *ptrs) == _lib.VMR_OK
            assert ns.tobytes() == full["node_sum"].tobytes(), pick
            if pick is None:
                continue
            name, arr = outs[pick]
            if name == "summary":
                for q, k in enumerate(_lib.SH_SUMMARY):
                    assert arr[..., q].tobytes() == full[k].tobytes(), k
            elif name in ("effective_size", "constraint"):
                assert not arr[undefined].any()                                           # the C ABI stores 0.0 where undefined
                assert np.array_equal(arr[~undefined], full[name][~undefined]), name
            else:
                assert np.array_equal(arr.astype(full[name].dtype), full[name]), name
    finally:
        eng.close()


def test_argument_errors_on_a_live_handle():
    from vimure_amd import _lib
    from vimure_amd.engine import EngineError, StructuralHolesArgumentError
    d = load_case("A_ones_mut")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, None)
    try:
        L, N = eng.L, eng.N
        ns, Y = np.zeros((2, L, N)), np.zeros((1, L, N, N), np.uint8)
        es, con = np.full((1, L, N), 9.0), np.full((1, L, N), 9.0)
        nul = [None] * 10

        def raw(S=2, n_trials=1, md=0, top_k=1, nsp=ns.ctypes.data):
            return eng.lib.vmr_sample_structural_holes(eng._h, 1, S, n_trials, md, top_k, nsp, *nul)

        def raw_net(Yp=Y.ctypes.data, n=1, md=0, esp=es.ctypes.data, conp=con.ctypes.data):
            return eng.lib.vmr_network_structural_holes(eng._h, Yp, n, md, esp, conp, None, None, None, None)

        bad = ((raw, {"S": 0}, b"n_samples"), (raw, {"n_trials": 0}, b"n_trials"), (raw, {"md": 2}, b"mode"), (raw, {"md": -1}, b"mode"),
               (raw, {"top_k": 0}, b"top_k"), (raw, {"top_k": N + 1}, b"top_k"), (raw, {"nsp": None}, b"node_sum"),
               (raw_net, {"n": 0}, b"n must"), (raw_net, {"md": 2}, b"mode"), (raw_net, {"md": -1}, b"mode"), (raw_net, {"Yp": None}, b"Y is NULL"),
               (raw_net, {"esp": None}, b"effective_size is NULL"), (raw_net, {"conp": None}, b"constraint is NULL"))
        # before vmr_set_state: the state is what is missing, unless an argument is refused first; the networks' call needs none
        with pytest.raises(EngineError, match="vmr_set_state") as ei:
            eng.sample_structural_holes(1, 2)
        assert not isinstance(ei.value, StructuralHolesArgumentError)
        assert raw() == _lib.VMR_ESTATE and raw_net() == _lib.VMR_OK and not es.any() and not con.any()
        for fn, kw, word in bad:
            assert fn(**kw) == _lib.VMR_EINVAL, kw
            err = eng.lib.vmr_last_error(eng._h)
            assert word in err and (b"vmr_sample_structural_holes" if fn is raw else b"vmr_network_structural_holes") in err, (kw, err)
        eng.set_state(*_golden_state(d))
        for fn, kw, word in bad:
            assert fn(**kw) == _lib.VMR_EINVAL and word in eng.lib.vmr_last_error(eng._h), (kw, word)
        for kw, word in (({"n_samples": 0}, "n_samples"), ({"n_trials": 0}, "n_trials"), ({"top_k": 0}, "top_k"), ({"top_k": N + 1}, "top_k"),
                         ({"mode": "mutual"}, "mode"), ({"mode": 2}, "mode"), ({"mode": -1}, "mode")):
            args = dict(seed=1, n_samples=2)
            args.update(kw)
            with pytest.raises(StructuralHolesArgumentError, match=word):
                eng.sample_structural_holes(**args)
        with pytest.raises(StructuralHolesArgumentError, match="mode"):
            eng.network_structural_holes(Y[0], mode="both")
        with pytest.raises(StructuralHolesArgumentError, match="shape"):
            eng.network_structural_holes(np.zeros((L, N, N + 1), np.uint8))
        # the ends of every range are accepted, and the handle still works
        got = eng.sample_structural_holes(1, 2, mode=1, top_k=N)
        assert got["node_sum"].shape == (2, L, N) and np.array_equal(got["node_top"], np.full((2, L, N), 2))
        got = eng.sample_structural_holes(1, 1, mode=0, top_k=1, n_trials=1)
        assert got["n_defined"].shape == (1, L) and (got["node_top"].sum(axis=2) >= 1).all()
    finally:
        eng.close()


def test_model_posterior_structural_holes():
    from vimure_amd import VimureModel
    from vimure_amd.synthetic import standard_sbm
    net = standard_sbm(N=60, M=8, L=1, K=2, avg_degree=6.0, eta=0.4, seed=4)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = VimureModel(mutuality=True)
        m.fit(net.X, K=2, seed=1, max_iter=30, num_realisations=1, keep_engine=True)
    try:
        S, sd = 8, 321
        res = m.posterior_structural_holes(mode="weighted", n_samples=S, seed=sd, top_k=5, values=True)
        assert m._rho_f is None                                           # rho has not crossed PCIe
        Yinf = m.get_inferred_model()
        inf = holes_np([Yinf], "weighted")
        assert sorted(res.inferred) == sorted(VALUE_KEYS) and res.inferred["constraint"].shape == (m.L, m.N)
        _assert_values({k: res.inferred[k][None] for k in VALUE_KEYS}, inf, m.N, "inferred")
        _assert_bytes(res.inferred, m._engine.network_structural_holes(Yinf, mode="weighted"), VALUE_KEYS)
        Ys = np.asarray([m.sample_inferred_model(N=1, seed=sd + s, device=True)[0] for s in range(S)])
        want = holes_np(Ys, "weighted", 5)
        got = {"degree": res.degree, "strength": res.strength, "redundancy": res.redundancy, "effective_size": res.effective_size.values,
               "constraint": res.constraint.values}
        _assert_values(got, want, m.N, "samples")
        own = reduce_values(res.degree, res.effective_size.values, res.constraint.values, 5)
        assert res.mode == "weighted" and res.top_k == 5 and np.array_equal(res.node_defined, own["node_defined"])
        for q, view in enumerate((res.effective_size, res.constraint)):
            for name in ("mean", "sd", "expected_rank", "top_prob", "defined_prob"):
                assert getattr(view, name).shape == (m.L, m.N), name
            assert view.values.shape == (S, m.L, m.N) and np.array_equal(view.node_sum, own["node_sum"][q])
            some = res.node_defined > 0
            assert np.array_equal(view.mean[some], own["node_sum"][q][some] / res.node_defined[some]) and np.isnan(view.mean[~some]).all()
            assert (view.top_prob >= 0).all() and (view.top_prob <= 1).all() and np.array_equal(view.expected_rank, own["node_rank_sum"][q] / S)
        assert res.n_defined.shape == (S, m.L) and np.array_equal(res.n_defined, own["n_defined"]) and res.n_defined.min() >= 2
        assert res.efficiency().shape == (S, m.L, m.N) and res.brokers(5).shape == (5,) and res.constraint.top(3, 0).shape == (3,)
        assert len(res.frame()) == m.L * m.N and len(res.effective_size.frame()) == m.L * m.N and len(res.summary()) == 3 * m.L
        un = m.posterior_structural_holes(n_samples=S, seed=sd)
        assert un.mode == "union" and un.effective_size.values is None and un.efficiency() is None
        assert np.array_equal(un.constraint.node_sum, m._engine.sample_structural_holes(sd, S)["node_sum"][1])
    finally:
        m.close()
