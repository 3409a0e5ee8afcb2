"""GPU: betweenness centrality of posterior samples and of given networks on the device (vmr_sample_betweenness,
vmr_network_betweenness), held to the NumPy restatement (tests/betweenness_util.py) of the samples `CaviEngine.sample` returns for
the same seeds: both data layouts, the general kernels (K = 12, 16), a coordinate-list handle, every word boundary, designed
graphs with closed forms bit for bit, the node bound.  Several chunks, two runs, every optional output on its own, the argument
errors, and the model's method.

The tolerance of a value is derived, not measured.  All terms are non-negative.  Per source a delta collects, per term of its sum,
at most one rounding each for 1 + delta, the quotient by sigma and the add, and one for the product with sigma per node -- the
device sums sigma[w] * sum_v (1 + delta[v]) / sigma[v], the restatement the same, and a sum of n non-negative terms is within
(n - 1) roundings of its value in any order -- over levels whose widths sum to N: no more than 4 N roundings; the sum over the
sources adds N more.  So each side is within 5 N 2^-53 relative, and |got - want| <= 10 N 2^-53 want.  (sigma itself is exact:
`betweenness_np(exact_sigma=True)` asserts sigma <= 2^53.)"""
import math
import warnings

import numpy as np
import pytest

from tests.betweenness_util import (BTW_KEYS, DIRECTIONS, EPS, betweenness_np, brandes_levels, diamond_chain, diamond_closed_form,
                                    reduce_values, search_graph, sigma_ok)
from tests.connectivity_util import designed_graphs
from tests.golden_util import case_config, load_case
from tests.test_hip_centrality import _coo_engine_with_rho, _engine_with_rho, _medium_case
from tests.test_hip_netstats import _engine_for, _golden_state

pytestmark = pytest.mark.gpu

ALL_KEYS = BTW_KEYS + ("values",)
OWN_KEYS = ("node_sum", "node_sumsq", "node_rank_sum", "node_top", "max")


def _assert_equal_btw(got, want, keys=ALL_KEYS):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), k


def _assert_values(got, want, N, what=""):
    """|got - want| <= 10 N 2^-53 want (the module's derivation); prints the largest observed ratio to that bound."""
    assert got.shape == want.shape and np.isfinite(got).all()
    err = np.abs(got - want)
    bound = 10 * N * EPS * want
    pos = want > 0
    ratio = (err[pos] / bound[pos]).max() if pos.any() else 0.0
    print("%s: largest |got - want| / (10 N 2^-53 want) = %.3g over %d values" % (what, ratio, int(pos.sum())))
    assert np.all(err <= bound), what


def _assert_own_reductions(got, top_k, N):
    """Every reduction against the restatement's reduction of the DEVICE's values: bit for bit, but for the sample's total,
    whose tree differs: N 2^-53 relative."""
    own = reduce_values(got["values"], top_k)
    _assert_equal_btw(got, own, keys=OWN_KEYS)
    assert np.all(np.abs(got["total"] - own["total"]) <= N * EPS * own["total"])


def _assert_path_length_identity(eng, got, seed, S, n_trials=1):
    """DIRECTED: sum_v b(v) is the number of inner nodes of one shortest path per reachable ordered pair, sum (d(s, t) - 1) =
    dist_sum - reach_pairs of `sample_connectivity` (reach_pairs leaves s = t out: include/vimure_hip.h) -- an integer from
    another kernel, no tolerance to choose."""
    conn = eng.sample_connectivity(seed, S, n_trials=n_trials, hist=False)
    want = conn["dist_sum"] - conn["reach_pairs"]
    assert np.array_equal(np.rint(got["total"]).astype(np.int64), want)
    for s in range(S):
        for l in range(eng.L):
            tot = math.fsum(got["values"][s, l].tolist())
            assert abs(tot - int(want[s, l])) <= eng.N * EPS * int(want[s, l]), (s, l, tot, int(want[s, l]))


def _check(eng, seed, S, trials=(1,), top_k=3):
    """`sample_betweenness` against the restatement on the samples of the same seeds, the reductions against the device's own
    values, the path-length identity, and `network_betweenness` of the same samples bit for bit; returns {direction: result}."""
    res = {}
    for n_trials in trials:
        Ys = np.asarray([eng.sample(seed + s, n_trials) for s in range(S)])
        for d in DIRECTIONS:
            want = betweenness_np(Ys, d, top_k, exact_sigma=True)
            got = eng.sample_betweenness(seed, S, direction=d, top_k=top_k, n_trials=n_trials, values=True)
            assert sorted(got) == sorted(ALL_KEYS)
            for k in ALL_KEYS:
                assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
            _assert_values(got["values"], want["values"], eng.N, "direction %s n_trials %d" % (d, n_trials))
            _assert_own_reductions(got, top_k, eng.N)
            if d == "directed":
                _assert_path_length_identity(eng, got, seed, S, n_trials)
            assert np.array_equal(eng.network_betweenness(Ys, direction=d), got["values"]), d
            res[d] = got
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


@pytest.mark.parametrize("case", ["L_default_K12", "M_K16_nomut"])
def test_values_against_the_restatement_general_kernels(case):
    d = load_case(case)
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


@pytest.mark.parametrize("N", [5, 63, 64, 65, 129])
def test_word_boundaries(N):
    """L = 2, K = 3 and W = ceil(N / 64) = 1, 1, 1, 2, 3 words per bit row; rho puts 1 - 3 / N on "no tie" and splits the rest:
    above the percolation threshold, where shortest paths are long and many pairs have several.  These are the boundaries of the
    first three words only: one or two lanes per row, one node per thread.  The wider shapes -- 8 and 16 lanes, a second trip of
    the word stride behind them, three to five nodes per thread on the rungs 4 and 8 -- are held in
    tests/test_hip_graph_shapes.py."""
    L, K, S = 2, 3, 8
    rho = np.empty((L, N, N, K))
    rho[..., 0] = 1.0 - 3.0 / N
    rho[..., 1:] = 1.5 / N
    eng = _engine_with_rho(rho, 100 + N)
    try:
        Ys = np.asarray([eng.sample(7 + s) for s in range(S)])
        assert Ys[:, :, np.arange(N), np.arange(N)].any()             # clearing the diagonal is exercised
        res = _check(eng, 7, S)
        if N >= 63:                                                    # path counting is exercised in every sample and layer
            for s in range(S):
                for l in range(L):
                    assert (res["directed"]["values"][s, l] > 0).sum() >= 16, (s, l)
                    assert sigma_ok(search_graph(Ys[s, l], "directed"))[0] >= 2, (s, l)
    finally:
        eng.close()


def _stateless(L, N, M=2):
    """A coordinate-list handle with a handful of reports and NO state."""
    from vimure_amd import CaviEngine
    subs = tuple(np.array(a, np.int64) for a in ([0, 0, 0], [0, 1, N - 1], [1, N - 1, 0], [0, 1, 0]))
    return CaviEngine.from_coo(subs, np.array([1, 2, 1], np.int64), (L, N, N, M), K=2)


def test_designed_graphs_bit_for_bit():
    """`network_betweenness` on a handle with no state.  N = 129, L = 4: the directed path (b = i (N - 1 - i)), the directed
    cycle ((N - 1)(N - 2) / 2), two cycles of 64 beside a node with only a self-loop, the empty graph; several networks in one
    call.  Then a chain of 70 diamonds, N = 211: sigma reaches 2^70 -- a sigma kept in 32 or 64 bits fails -- every quantity is
    dyadic and the closed form is met exactly."""
    Y = designed_graphs()
    N = Y.shape[1]
    i = np.arange(N)
    closed = np.zeros((4, N))
    closed[0] = i * (N - 1.0 - i)
    closed[1] = (N - 1) * (N - 2) / 2.0
    closed[2, :128] = 63 * 62 / 2.0
    eng = _stateless(4, N)
    try:
        got = eng.network_betweenness(Y)
        assert got.shape == (4, N) and got.dtype == np.float64 and np.array_equal(got, closed)
        assert np.array_equal(got, betweenness_np([Y], "directed")["values"][0])
        three = eng.network_betweenness(np.stack([Y, Y[::-1], Y]), direction=0)
        assert np.array_equal(three, np.stack([closed, closed[::-1], closed]))
        assert np.array_equal(eng.network_betweenness(np.swapaxes(Y, 1, 2)), closed)      # reversing the graph leaves b unchanged
        assert np.array_equal(eng.network_betweenness(Y, "union"), betweenness_np([Y], "union")["values"][0])
        assert np.array_equal(eng.network_betweenness(Y * 7, "union")[1], np.full(N, 64 * 63 / 2.0))   # entries > 0 are ties
    finally:
        eng.close()
    Yd = diamond_chain()
    D, sigma, _ = brandes_levels(search_graph(Yd, "directed"))
    assert sigma.max() == 2.0 ** 70 and D.max() == 140
    closed = diamond_closed_form()
    assert (closed[1], closed[3], closed[4]) == (104.0, 621.0, 410.0)
    eng = _stateless(1, 211)
    try:
        assert np.array_equal(eng.network_betweenness(Yd[None])[0], closed)
    finally:
        eng.close()


def test_medium_case_chunks_and_reruns(monkeypatch):
    """L = 2, N = 300, K = 3 on report lists: threads own two nodes, five words per bit row, 19 source blocks.  S = 16 in one
    chunk against chunks of 5 samples (16 = 5 + 5 + 5 + 1) and against a second run, bit for bit, the per-node sums over the
    samples included; the first samples against the restatement; `sample_stats` and `sample_connectivity` of the same engine are
    what they were before the calls."""
    X, st = _medium_case()
    seed, S = 1000, 16
    monkeypatch.setenv("VMR_FORMAT", "sparse")
    monkeypatch.delenv("VMR_NETSTATS_CHUNK", raising=False)
    eng = _engine_for(X, None, 3, True, st)
    try:
        assert eng.data_format()[0] == "sparse"
        before = dict(eng.sample_stats(seed, S, degrees=True), **eng.sample_connectivity(seed, S, nodes=True))
        one = {d: eng.sample_betweenness(seed, S, direction=d, top_k=10, values=True) for d in DIRECTIONS}
        again = {d: eng.sample_betweenness(seed, S, direction=d, top_k=10, values=True) for d in DIRECTIONS}
        after = dict(eng.sample_stats(seed, S, degrees=True), **eng.sample_connectivity(seed, S, nodes=True))
        Ys = np.asarray([eng.sample(seed + s) for s in range(2)])
    finally:
        eng.close()
    for d in DIRECTIONS:
        _assert_equal_btw(again[d], one[d])
        assert (one[d]["node_sum"] > 0).all() and (one[d]["node_sumsq"] > 0).all()
        _assert_values(one[d]["values"][:2], betweenness_np(Ys, d)["values"], 300, "medium " + d)
        _assert_own_reductions(one[d], 10, 300)
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    monkeypatch.setenv("VMR_NETSTATS_CHUNK", "5")
    eng = _engine_for(X, None, 3, True, st)
    try:
        many = {d: eng.sample_betweenness(seed, S, direction=d, top_k=10, values=True) for d in DIRECTIONS}
    finally:
        eng.close()
    for d in DIRECTIONS:
        _assert_equal_btw(many[d], one[d])


def test_the_node_bound():
    """N = BTW_NMAX: L = 1, K = 2, S = 1, rho_1 = 3 / N on a coordinate-list handle -- 32 words per bit row, threads own eight
    nodes, 128 source blocks -- against the restatement."""
    from vimure_amd import _lib
    N = _lib.BTW_NMAX
    rho = np.empty((1, N, N, 2))
    rho[..., 1] = 3.0 / N
    rho[..., 0] = 1.0 - 3.0 / N
    eng = _coo_engine_with_rho(rho)
    try:
        Ys = np.asarray([eng.sample(5)])
        assert Ys[0, 0, N - 1].any() and Ys[0, 0, :, N - 1].any()      # the last node has ties both ways
        for d in DIRECTIONS:
            want = betweenness_np(Ys, d, top_k=N, exact_sigma=True)
            got = eng.sample_betweenness(5, 1, direction=d, top_k=N, values=True)
            _assert_values(got["values"], want["values"], N, "node bound " + d)
            _assert_own_reductions(got, N, N)
            assert np.array_equal(got["node_top"], np.ones((1, N)))        # top_k = N: every node
        _assert_path_length_identity(eng, eng.sample_betweenness(5, 1, values=True), 5, 1)
    finally:
        eng.close()


def test_more_nodes_than_the_bound_are_refused():
    """A coordinate-list handle of VMR_BTW_NMAX + 1 nodes and no state: both calls refuse it for its N, not for its state."""
    from vimure_amd import _lib
    from vimure_amd.engine import BetweennessArgumentError
    N = _lib.BTW_NMAX + 1
    eng = _stateless(1, N)
    try:
        with pytest.raises(BetweennessArgumentError, match=str(_lib.BTW_NMAX)):
            eng.sample_betweenness(1, 2)
        with pytest.raises(BetweennessArgumentError, match=str(_lib.BTW_NMAX)):
            eng.network_betweenness(np.zeros((1, N, N), np.uint8))
        ns = np.zeros((1, N))
        assert eng.lib.vmr_sample_betweenness(eng._h, 1, 2, 1, 0, 1, ns.ctypes.data, *[None] * 5) == _lib.VMR_EINVAL
        assert b"N <= %d" % _lib.BTW_NMAX in eng.lib.vmr_last_error(eng._h) and b"LDS" in eng.lib.vmr_last_error(eng._h)
    finally:
        eng.close()


def test_optional_outputs():
    """node_sum alone, and node_sum with each other output alone (the raw call, the others NULL)."""
    from vimure_amd import _lib
    d = load_case("B_random_mask_K3")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        S, top_k = 4, 3
        full = eng.sample_betweenness(9, S, direction="union", top_k=top_k, values=True)
        plain = eng.sample_betweenness(9, S, direction="union", top_k=top_k)
        assert sorted(plain) == sorted(BTW_KEYS)
        _assert_equal_btw(plain, full, keys=BTW_KEYS)
        L, N = eng.L, eng.N
        outs = [("node_sumsq", np.full((L, N), -1.0)), ("node_rank_sum", np.full((L, N), 7, np.uint64)),
                ("node_top", np.full((L, N), 7, np.uint32)), ("summary", np.full((S, L, 2), -1.0)), ("values", np.full((S, L, N), -1.0))]
        for pick in [None] + list(range(len(outs))):
            ns = np.full((L, N), -1.0)
            ptrs = [a.ctypes.data if i == pick else None for i, (_, a) in enumerate(outs)]
            assert eng.lib.vmr_sample_betweenness(eng._h, 9, S, 1, 1, top_k, ns.ctypes.data, *ptrs) == _lib.VMR_OK
            assert np.array_equal(ns, full["node_sum"]), pick
            if pick is not None:
                name, arr = outs[pick]
                if name == "summary":
                    assert np.array_equal(arr[..., 0], full["total"]) and np.array_equal(arr[..., 1], full["max"])
                else:
                    assert np.array_equal(arr.astype(full[name].dtype), full[name]), name
    finally:
        eng.close()


def test_argument_errors_on_a_live_handle():
    from vimure_amd import _lib
    from vimure_amd.engine import BetweennessArgumentError, EngineError
    d = load_case("A_ones_mut")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, None)
    try:
        L, N = eng.L, eng.N
        ns, vals, Y = np.zeros((L, N)), np.zeros((1, L, N)), np.zeros((1, L, N, N), np.uint8)
        nul = [None] * 5

        def raw(S=2, n_trials=1, d=0, top_k=1, nsp=ns.ctypes.data):
            return eng.lib.vmr_sample_betweenness(eng._h, 1, S, n_trials, d, top_k, nsp, *nul)

        def raw_net(Yp=Y.ctypes.data, n=1, d=0, out=vals.ctypes.data):
            return eng.lib.vmr_network_betweenness(eng._h, Yp, n, d, out)

        bad = ((raw, {"S": 0}, b"n_samples"), (raw, {"n_trials": 0}, b"n_trials"), (raw, {"d": 2}, b"direction"), (raw, {"d": -1}, b"direction"),
               (raw, {"top_k": 0}, b"top_k"), (raw, {"top_k": N + 1}, b"top_k"), (raw, {"nsp": None}, b"node_sum"),
               (raw_net, {"n": 0}, b"n must"), (raw_net, {"d": 2}, b"direction"), (raw_net, {"Yp": None}, b"Y is NULL"),
               (raw_net, {"out": None}, b"values is NULL"))
        # before vmr_set_state: the state is what is missing, unless an argument is refused first; the networks' call needs none
        with pytest.raises(EngineError, match="vmr_set_state") as ei:
            eng.sample_betweenness(1, 2)
        assert not isinstance(ei.value, BetweennessArgumentError)
        assert raw() == _lib.VMR_ESTATE and raw_net() == _lib.VMR_OK and not vals.any()
        for fn, kw, word in bad:
            assert fn(**kw) == _lib.VMR_EINVAL and word in eng.lib.vmr_last_error(eng._h), (kw, word)
        eng.set_state(*_golden_state(d))
        for fn, kw, word in bad:
            assert fn(**kw) == _lib.VMR_EINVAL and word in eng.lib.vmr_last_error(eng._h), (kw, word)
        for kw, word in (({"n_samples": 0}, "n_samples"), ({"n_trials": 0}, "n_trials"), ({"top_k": 0}, "top_k"), ({"top_k": N + 1}, "top_k"),
                         ({"direction": "out"}, "direction"), ({"direction": 2}, "direction"), ({"direction": -1}, "direction")):
            args = dict(seed=1, n_samples=2)
            args.update(kw)
            with pytest.raises(BetweennessArgumentError, match=word):
                eng.sample_betweenness(**args)
        with pytest.raises(BetweennessArgumentError, match="direction"):
            eng.network_betweenness(Y[0], direction="in")
        with pytest.raises(BetweennessArgumentError, match="shape"):
            eng.network_betweenness(np.zeros((L, N, N + 1), np.uint8))
        # the ends of every range are accepted, and the handle still works
        got = eng.sample_betweenness(1, 2, direction=1, top_k=N)
        assert got["node_sum"].shape == (L, N) and np.isfinite(got["node_sum"]).all()
        assert eng.sample_betweenness(1, 1, top_k=1)["total"].shape == (1, L)
    finally:
        eng.close()


def test_model_posterior_betweenness():
    from vimure_amd import VimureModel
    from vimure_amd.synthetic import standard_sbm
    net = standard_sbm(N=60, M=8, L=1, K=2, avg_degree=6.0, eta=0.4, seed=4)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = VimureModel(mutuality=True)
        m.fit(net.X, K=2, seed=1, max_iter=30, num_realisations=1, keep_engine=True)
    try:
        S, sd = 8, 321
        base = m.posterior_network_stats(n_samples=S, seed=sd)
        res = m.posterior_betweenness(direction="directed", n_samples=S, seed=sd, top_k=5, values=True)
        assert m._rho_f is None                                           # rho has not crossed PCIe
        Ys = np.asarray([m.sample_inferred_model(N=1, seed=sd + s, device=True)[0] for s in range(S)])
        want = betweenness_np(Ys, "directed", top_k=5)
        assert want["values"].max() > 0
        _assert_values(res.values, want["values"], m.N, "model")
        own = reduce_values(res.values, 5)
        for k in OWN_KEYS:
            assert np.array_equal(getattr(res, k), own[k]), k
        assert np.array_equal(res.mean, own["node_sum"] / S) and np.array_equal(res.expected_rank, own["node_rank_sum"] / S)
        assert (res.top_prob >= 0).all() and (res.top_prob <= 1).all() and res.top_prob.sum() >= 5
        assert (res.sd >= 0).all() and res.sd.max() > 0
        Yinf = m.get_inferred_model()
        assert m._rho_f is None
        inf = betweenness_np([Yinf], "directed")["values"][0]
        assert inf.max() > 0
        _assert_values(res.inferred, inf, m.N, "inferred")
        assert np.array_equal(res.inferred, m._engine.network_betweenness(Yinf))
        assert np.array_equal(res.normalized()["mean"], res.mean / ((m.N - 1) * (m.N - 2)))
        assert res.top(5).shape == (5,) and len(res.frame()) == m.L * m.N and len(res.summary()) == 2 * m.L
        uni = m.posterior_betweenness(direction="union", n_samples=S, seed=sd)
        assert uni.values is None and uni.scale == (m.N - 1) * (m.N - 2) / 2.0
        assert np.array_equal(uni.node_sum, m._engine.sample_betweenness(sd, S, direction="union")["node_sum"])
        base2 = m.posterior_network_stats(n_samples=S, seed=sd)             # the dyad read-out is what it was
        for k, v in base.statistics().items():
            assert np.array_equal(v, base2.statistics()[k], equal_nan=True), k
    finally:
        m.close()
