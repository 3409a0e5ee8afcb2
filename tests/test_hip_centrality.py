"""GPU: diffusion centrality of posterior samples and of the posterior mean network on the device (vmr_sample_centrality,
vmr_mean_centrality).  With q a negative power of two every number is exactly representable (tests/centrality_util.exact_ok
asserts it), so every output is held bit for bit to the NumPy restatement of the samples `CaviEngine.sample` returns for the same
seeds: both data layouts, the general kernels (K = 12, 16), a coordinate-list handle, every word boundary at the percolation
threshold, designed graphs with closed forms, the node bound.  With a general q the values are held to the restatement within
the rounding of both sides and every reduction to the restatement's reduction of the device's own values.  Several chunks, two
runs, every optional output on its own, the argument errors, and the model's method against `sample_inferred_model`."""
import functools
import warnings

import numpy as np
import pytest

from tests.centrality_util import (CENT_KEYS, DIRECTIONS, EPS, adjacency, centrality_np, designed_closed_forms, exact_ok,
                                   mean_centrality_np, reduce_values)
from tests.connectivity_util import designed_graphs
from tests.golden_util import case_config, load_case
from tests.test_hip_netstats import _engine_for, _golden_state, _medium, _random_state

pytestmark = pytest.mark.gpu

ALL_KEYS = CENT_KEYS + ("values",)
Q2 = (0.5, 0.25)        # one passing probability per layer, so that a mis-indexed q shows


def _assert_equal_cent(got, want, keys=ALL_KEYS):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), k


def _check_exact(eng, seed, S, trials=(1, 3), Ts=(1, 8), top_k=3):
    """`sample_centrality` against the restatement on the samples of the same seeds, bit for bit, after `exact_ok` on every
    sample; returns the last reference of direction "out"."""
    q = np.array(Q2[:eng.L]) if eng.L <= 2 else np.full(eng.L, 0.5)
    ref = None
    for n_trials in trials:
        Ys = np.asarray([eng.sample(seed + s, n_trials) for s in range(S)])
        for T in Ts:
            for d in DIRECTIONS:
                for s in range(S):
                    for l in range(eng.L):
                        exact_ok(adjacency(Ys[s, l], d), q[l], T)
                want = centrality_np(Ys, q, T, d, top_k)
                got = eng.sample_centrality(seed, S, q, T, direction=d, top_k=top_k, n_trials=n_trials, values=True)
                assert sorted(got) == sorted(ALL_KEYS)
                _assert_equal_cent(got, want)
                if d == "out":
                    ref = want
    return ref


@pytest.mark.parametrize("case", ["A_ones_mut", "B_random_mask_K3", "D_self_mask", "E_undirected"])
def test_outputs_equal_numpy_on_the_samples(case, vmr_format):
    d = load_case(case)
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        assert eng.data_format()[0] == vmr_format
        _check_exact(eng, 11, 8)
    finally:
        eng.close()


@pytest.mark.parametrize("case", ["L_default_K12", "M_K16_nomut"])
def test_outputs_equal_numpy_general_kernels(case):
    d = load_case(case)
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    assert K > 8
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        _check_exact(eng, 5, 8)
    finally:
        eng.close()


def test_outputs_equal_numpy_coo_handle():
    d = load_case("D_self_mask")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d), coo=True)
    try:
        _check_exact(eng, 3, 8)
    finally:
        eng.close()


def _engine_with_rho(rho, seed, M=4):
    """An engine on random reports whose state holds the given rho [L, N, N, K]."""
    L, N, _, K = rho.shape
    g = np.random.RandomState(seed)
    X = (g.rand(L, N, N, M) < 0.1).astype(np.uint8)
    st = _random_state(g, L, N, M, K)
    return _engine_for(X, None, K, True, st[:6] + (rho,))


def _coo_engine_with_rho(rho, M=2):
    """A coordinate-list engine with a handful of reports whose state holds the given rho: no dense [L, N, N, M] anywhere."""
    from vimure_amd import CaviEngine
    L, N, _, K = rho.shape
    subs = tuple(np.array(a, np.int64) for a in ([0, 0, 0], [0, 5, N - 1], [1, N - 1, 0], [0, 1, 0]))
    eng = CaviEngine.from_coo(subs, np.array([1, 2, 1], np.int64), (L, N, N, M), K=K)
    eng.set_priors(0.1 * np.ones((L, M)), 0.1 * np.ones((L, M)), 10.0 * np.ones((L, K)), 10.0 * np.ones((L, K)), 0.5, 1.0)
    eng.set_state(np.ones((L, M)), np.ones((L, M)), np.ones((L, K)), np.ones((L, K)), 3.0, 2.5, rho)
    return eng


@pytest.mark.parametrize("N", [5, 63, 64, 65, 129])
def test_word_boundaries(N):
    """L = 2, K = 3 and W = ceil(N / 64) = 1, 1, 1, 2, 3 words per bit row; rho puts 1 - 1.5 / N on "no tie" and splits the rest:
    the percolation threshold, where few nodes have distinct walk counts and many tie.  These are the boundaries of the first
    three words only: one or two lanes per row, one node per thread.  The wider shapes -- 8 and 16 lanes, a second trip of the word
    stride behind them, three to five nodes per thread on the rungs 4 and 8 -- are held in tests/test_hip_graph_shapes.py."""
    L, K, S = 2, 3, 8
    rho = np.empty((L, N, N, K))
    rho[..., 0] = 1.0 - 1.5 / N
    rho[..., 1:] = 0.75 / N
    eng = _engine_with_rho(rho, 100 + N)
    try:
        Ys = np.asarray([eng.sample(7 + s) for s in range(S)])
        assert Ys[:, :, np.arange(N), np.arange(N)].any()             # clearing the diagonal is exercised
        want = _check_exact(eng, 7, S, trials=(1,))
        if N >= 63:                                                    # the comparison cannot pass on trivial graphs
            for s in range(S):
                for l in range(L):
                    distinct = np.unique(want["values"][s, l]).size
                    assert 8 <= distinct < N, (s, l, distinct)           # at least 8 distinct values, and tied ranks
    finally:
        eng.close()


def test_designed_graphs():
    """One-hot rho, N = 129, L = 4, K = 2: every sample is the design whatever the seed -- the directed path, the directed cycle,
    two cycles beside a node with a self-loop, the empty graph.  The mean network is the design too: P is 0 / 1."""
    Y = designed_graphs()
    rho = np.stack([1.0 - Y, Y], axis=-1).astype(np.float64)
    q, T = 0.5, 16
    closed = designed_closed_forms(q, T)
    eng = _engine_with_rho(rho, 3)
    try:
        assert np.array_equal(eng.sample(40), Y)
        for l in range(4):
            assert np.array_equal(exact_ok(adjacency(Y[l], "out"), q, T), closed[l])
        want = centrality_np([Y, Y], q, T, "out", top_k=5)
        got = eng.sample_centrality(40, 2, q, T, direction="out", top_k=5, values=True)
        assert np.array_equal(got["values"][0], closed) and np.array_equal(got["values"][1], closed)
        _assert_equal_cent(got, want)
        for d in DIRECTIONS:
            for l in range(4):
                exact_ok(adjacency(Y[l], d), q, T)
            c = eng.sample_centrality(40, 1, q, T, direction=d, values=True)["values"][0]
            assert np.array_equal(c, centrality_np([Y], q, T, d)["values"][0]), d
            assert np.array_equal(eng.mean_centrality(q, T, direction=d), c), d
    finally:
        eng.close()


@functools.lru_cache(maxsize=1)
def _medium_case():
    g = np.random.RandomState(21)
    return _medium(g)


def test_medium_case_chunks_and_reruns(monkeypatch):
    """L = 2, N = 300, K = 3 on report lists: threads own two nodes, five words per bit row.  S = 16 in one chunk against chunks
    of 5 samples (16 = 5 + 5 + 5 + 1) and against a second run, bit for bit, the per-node sums over the samples included;
    `sample_stats` and `sample_connectivity` of the same engine are what they were before the call."""
    X, st = _medium_case()
    seed, S, q, T = 1000, 16, 0.3, 8
    monkeypatch.setenv("VMR_FORMAT", "sparse")
    monkeypatch.delenv("VMR_NETSTATS_CHUNK", raising=False)
    eng = _engine_for(X, None, 3, True, st)
    try:
        assert eng.data_format()[0] == "sparse"
        before = dict(eng.sample_stats(seed, S, degrees=True), **eng.sample_connectivity(seed, S, nodes=True))
        one = {d: eng.sample_centrality(seed, S, q, T, direction=d, top_k=10, values=True) for d in DIRECTIONS}
        again = {d: eng.sample_centrality(seed, S, q, T, direction=d, top_k=10, values=True) for d in DIRECTIONS}
        after = dict(eng.sample_stats(seed, S, degrees=True), **eng.sample_connectivity(seed, S, nodes=True))
    finally:
        eng.close()
    for d in DIRECTIONS:
        _assert_equal_cent(again[d], one[d])
        assert (one[d]["node_sum"] > 0).all() and (one[d]["node_sumsq"] > 0).all()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    monkeypatch.setenv("VMR_NETSTATS_CHUNK", "5")
    eng = _engine_for(X, None, 3, True, st)
    try:
        many = {d: eng.sample_centrality(seed, S, q, T, direction=d, top_k=10, values=True) for d in DIRECTIONS}
    finally:
        eng.close()
    for d in DIRECTIONS:
        _assert_equal_cent(many[d], one[d])


def _check_general(eng, Ys, seed, q, T, top_k):
    """A general q: the values within the rounding of both sides -- all terms are non-negative and each side makes at most N + 1
    roundings per step: relative 2 T (N + 1) 2^-53 -- and every reduction equal to the restatement's reduction of the DEVICE's
    values, but for the sample's total, whose tree differs: N 2^-53 relative."""
    S, L, N, _ = Ys.shape
    for d in DIRECTIONS:
        want = centrality_np(Ys, q, T, d, top_k)
        got = eng.sample_centrality(seed, S, q, T, direction=d, top_k=top_k, values=True)
        assert (want["values"] > 0).any() and np.isfinite(want["values"]).all()
        err = np.abs(got["values"] - want["values"])
        print("direction %s T %d: largest relative error %.3g, bound %.3g"
              % (d, T, (err / np.maximum(want["values"], 1e-300)).max(), 2 * T * (N + 1) * EPS))
        assert np.all(err <= 2 * T * (N + 1) * EPS * want["values"]), d
        own = reduce_values(got["values"], top_k)
        _assert_equal_cent(got, own, keys=("node_sum", "node_sumsq", "node_rank_sum", "node_top", "max"))
        assert np.all(np.abs(got["total"] - own["total"]) <= N * EPS * own["total"]), d


def test_general_q_and_the_mean_network(monkeypatch):
    """The medium case with q = 0.3, T = 8, and with T = CENT_TMAX at q = 1 / (mean degree), a scalar and per layer; then
    `mean_centrality` of the same engine against NumPy on the rho of `get_state`: relative 4 T (N + 1) 2^-53, one more rounding
    per term for the product."""
    from vimure_amd import _lib
    X, st = _medium_case()
    seed, S = 1000, 4
    monkeypatch.delenv("VMR_NETSTATS_CHUNK", raising=False)
    eng = _engine_for(X, None, 3, True, st)
    try:
        N = eng.N
        Ys = np.asarray([eng.sample(seed + s) for s in range(S)])
        _check_general(eng, Ys, seed, 0.3, 8, 10)
        deg = np.asarray([[adjacency(Ys[s, l], "out").sum() / N for l in range(eng.L)] for s in range(S)]).mean(axis=0)
        assert (deg > 1).all()
        _check_general(eng, Ys, seed, 1.0 / deg, _lib.CENT_TMAX, 10)
        rho = eng.get_state()["rho"]
        for d in DIRECTIONS:
            for q, T in ((0.3, 8), (np.array([0.01, 0.02]), 5), (1.0 / deg, 3)):
                want = mean_centrality_np(rho, q, T, d)
                got = eng.mean_centrality(q, T, direction=d)
                assert got.shape == (eng.L, N) and (want > 0).all()
                assert np.all(np.abs(got - want) <= 4 * T * (N + 1) * EPS * want), (d, T)
            assert np.array_equal(eng.mean_centrality(0.3, 8, direction=d), eng.mean_centrality(0.3, 8, direction=d))
    finally:
        eng.close()


@pytest.mark.parametrize("case", ["B_random_mask_K3", "L_default_K12"])
def test_mean_centrality_golden(case):
    d = load_case(case)
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        rho = eng.get_state()["rho"]
        q = np.array(Q2[:eng.L])
        for dr in DIRECTIONS:
            for T in (1, 2, 7):
                want = mean_centrality_np(rho, q, T, dr)
                got = eng.mean_centrality(q, T, direction=dr)
                assert np.all(np.abs(got - want) <= 4 * T * (eng.N + 1) * EPS * want) and (want > 0).any(), (dr, T)
    finally:
        eng.close()


def test_mean_centrality_has_no_node_bound():
    """N = 2100 > CENT_NMAX, L = 1, T = 2: the mean network's call runs, the sampled one is refused for N."""
    from vimure_amd import _lib
    from vimure_amd.engine import CentralityArgumentError
    N, T = 2100, 2
    assert N > _lib.CENT_NMAX
    g = np.random.RandomState(4)
    rho = np.empty((1, N, N, 2))
    rho[..., 1] = g.rand(N, N) * (4.0 / N)
    rho[..., 0] = 1.0 - rho[..., 1]
    eng = _coo_engine_with_rho(rho)
    try:
        for d in DIRECTIONS:
            want = mean_centrality_np(rho, 0.5, T, d)
            got = eng.mean_centrality(0.5, T, direction=d)
            assert (want > 0).all() and np.all(np.abs(got - want) <= 4 * T * (N + 1) * EPS * want), d
        with pytest.raises(CentralityArgumentError, match=str(_lib.CENT_NMAX)):
            eng.sample_centrality(1, 2, 0.5, T)
    finally:
        eng.close()


def test_the_node_bound():
    """N = CENT_NMAX: L = 1, K = 2, S = 2, T = 4, rho_1 = 3 / N -- 32 words per bit row, threads own eight nodes, 32 KiB of LDS --
    exact with q = 1/2."""
    from vimure_amd import _lib
    N, S, T, q = _lib.CENT_NMAX, 2, 4, 0.5
    rho = np.empty((1, N, N, 2))
    rho[..., 1] = 3.0 / N
    rho[..., 0] = 1.0 - 3.0 / N
    eng = _coo_engine_with_rho(rho)
    try:
        Ys = np.asarray([eng.sample(5 + s) for s in range(S)])
        assert Ys[:, 0, N - 1].any() and Ys[:, 0, :, N - 1].any()      # the last node has ties both ways
        for d in DIRECTIONS:
            for s in range(S):
                exact_ok(adjacency(Ys[s, 0], d), q, T)
            want = centrality_np(Ys, q, T, d, top_k=N)
            got = eng.sample_centrality(5, S, q, T, direction=d, top_k=N, values=True)
            _assert_equal_cent(got, want)
            assert np.array_equal(got["node_top"], np.full((1, N), S))     # top_k = N: every node, every sample
    finally:
        eng.close()


def test_more_nodes_than_the_bound_are_refused():
    """A coordinate-list handle of VMR_CENT_NMAX + 1 nodes with a handful of entries and no state: refused for its N, not for
    its state."""
    from vimure_amd import CaviEngine, _lib
    from vimure_amd.engine import CentralityArgumentError
    N = _lib.CENT_NMAX + 1
    subs = tuple(np.array(a, np.int64) for a in ([0, 0, 0], [0, 5, N - 1], [1, N - 1, 0], [0, 1, 0]))
    eng = CaviEngine.from_coo(subs, np.array([1, 2, 1], np.int64), (1, N, N, 2), K=2)
    try:
        with pytest.raises(CentralityArgumentError, match=str(_lib.CENT_NMAX)):
            eng.sample_centrality(1, 2, 0.5, 3)
        q, ns = np.full(1, 0.5), np.zeros((1, N))
        assert eng.lib.vmr_sample_centrality(eng._h, 1, 2, 1, q.ctypes.data, 3, 0, 1, ns.ctypes.data, *[None] * 5) == _lib.VMR_EINVAL
        assert b"N <= %d" % _lib.CENT_NMAX in eng.lib.vmr_last_error(eng._h) and b"LDS" in eng.lib.vmr_last_error(eng._h)
    finally:
        eng.close()


def test_optional_outputs():
    """node_sum alone, and node_sum with each other output alone (the raw call, the others NULL)."""
    from vimure_amd import _lib
    d = load_case("B_random_mask_K3")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        S, T, top_k = 4, 5, 3
        q = np.array(Q2)
        full = eng.sample_centrality(9, S, q, T, direction="union", top_k=top_k, values=True)
        plain = eng.sample_centrality(9, S, q, T, direction="union", top_k=top_k)
        assert sorted(plain) == sorted(CENT_KEYS)
        _assert_equal_cent(plain, full, keys=CENT_KEYS)
        L, N = eng.L, eng.N
        outs = [("node_sumsq", np.full((L, N), -1.0)), ("node_rank_sum", np.full((L, N), 7, np.uint64)),
                ("node_top", np.full((L, N), 7, np.uint32)), ("summary", np.full((S, L, 2), -1.0)), ("values", np.full((S, L, N), -1.0))]
        for pick in [None] + list(range(len(outs))):
            ns = np.full((L, N), -1.0)
            ptrs = [a.ctypes.data if i == pick else None for i, (_, a) in enumerate(outs)]
            assert eng.lib.vmr_sample_centrality(eng._h, 9, S, 1, q.ctypes.data, T, 2, top_k, ns.ctypes.data, *ptrs) == _lib.VMR_OK
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
    from vimure_amd.engine import CentralityArgumentError, EngineError
    d = load_case("A_ones_mut")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, None)
    try:
        L, N = eng.L, eng.N
        q, ns, mc = np.full(L, 0.5), np.zeros((L, N)), np.zeros((L, N))
        nul = [None] * 5

        def raw(S=2, n_trials=1, qp=q.ctypes.data, T=3, d=0, top_k=1, nsp=ns.ctypes.data):
            return eng.lib.vmr_sample_centrality(eng._h, 1, S, n_trials, qp, T, d, top_k, nsp, *nul)

        def raw_mean(qp=q.ctypes.data, T=3, d=0, out=mc.ctypes.data):
            return eng.lib.vmr_mean_centrality(eng._h, qp, T, d, out)

        # before vmr_set_state: the state is what is missing, unless an argument is refused first
        with pytest.raises(EngineError, match="vmr_set_state") as ei:
            eng.sample_centrality(1, 2, 0.5, 3)
        assert not isinstance(ei.value, CentralityArgumentError)
        with pytest.raises(EngineError, match="vmr_set_state") as ei:
            eng.mean_centrality(0.5, 3)
        assert not isinstance(ei.value, CentralityArgumentError)
        assert raw() == _lib.VMR_ESTATE and raw_mean() == _lib.VMR_ESTATE
        assert raw(T=0) == _lib.VMR_EINVAL and raw_mean(d=3) == _lib.VMR_EINVAL      # whatever the handle's state
        eng.set_state(*_golden_state(d))
        bad_q = [np.full(L, np.nan), np.full(L, np.inf), np.full(L, -0.25), np.full(L, 1.5)]
        for kw, word in (({"n_samples": 0}, "n_samples"), ({"n_trials": 0}, "n_trials"), ({"T": 0}, "T must"),
                         ({"T": _lib.CENT_TMAX + 1}, "T must"), ({"top_k": 0}, "top_k"), ({"top_k": N + 1}, "top_k"),
                         ({"direction": "both"}, "direction"), ({"direction": 3}, "direction"), ({"direction": -1}, "direction"),
                         ({"q": np.zeros(L + 1)}, "q must")) + tuple(({"q": b}, r"q\[0\]") for b in bad_q):
            args = dict(seed=1, n_samples=2, q=0.5, T=3)
            args.update(kw)
            with pytest.raises(CentralityArgumentError, match=word):
                eng.sample_centrality(**args)
            margs = {k: args[k] for k in ("q", "T", "direction") if k in args}
            if any(k in kw for k in ("q", "T", "direction")):
                with pytest.raises(CentralityArgumentError, match=word):
                    eng.mean_centrality(**margs)
        for fn, kw, word in ((raw, {"S": 0}, b"n_samples"), (raw, {"n_trials": 0}, b"n_trials"), (raw, {"T": 0}, b"T must"),
                             (raw, {"T": _lib.CENT_TMAX + 1}, b"T must"), (raw, {"d": 3}, b"direction"), (raw, {"d": -1}, b"direction"),
                             (raw, {"top_k": 0}, b"top_k"), (raw, {"top_k": N + 1}, b"top_k"), (raw, {"qp": None}, b"q is NULL"),
                             (raw, {"nsp": None}, b"node_sum"), (raw_mean, {"T": 65}, b"T must"), (raw_mean, {"d": 7}, b"direction"),
                             (raw_mean, {"qp": None}, b"q is NULL"), (raw_mean, {"out": None}, b"out is NULL")):
            assert fn(**kw) == _lib.VMR_EINVAL and word in eng.lib.vmr_last_error(eng._h), (kw, word)
        for b in bad_q:
            assert raw(qp=b.ctypes.data) == _lib.VMR_EINVAL and b"q[0]" in eng.lib.vmr_last_error(eng._h)
            assert raw_mean(qp=b.ctypes.data) == _lib.VMR_EINVAL and b"q[0]" in eng.lib.vmr_last_error(eng._h)
        # the ends of every range are accepted, and the handle still works
        got = eng.sample_centrality(1, 2, np.r_[1.0, np.zeros(L - 1)], _lib.CENT_TMAX, direction=2, top_k=N)
        assert got["node_sum"].shape == (L, N) and np.isfinite(got["node_sum"]).all()
        assert not eng.sample_centrality(1, 2, 0.0, 1, top_k=1)["node_sum"].any()
        assert eng.mean_centrality(1.0, _lib.CENT_TMAX, direction="in").shape == (L, N)
    finally:
        eng.close()


def test_model_posterior_centrality():
    from vimure_amd import VimureModel
    from vimure_amd.centrality import default_q
    from vimure_amd.synthetic import standard_sbm
    net = standard_sbm(N=60, M=8, L=1, K=2, avg_degree=6.0, eta=0.4, seed=4)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = VimureModel(mutuality=True)
        m.fit(net.X, K=2, seed=1, max_iter=30, num_realisations=1, keep_engine=True)
    try:
        S, sd = 8, 321
        base = m.posterior_network_stats(n_samples=S, seed=sd)
        conn = m.posterior_connectivity(n_samples=S, seed=sd)
        res = m.posterior_centrality(q=0.25, T=6, direction="out", n_samples=S, seed=sd, top_k=5, values=True)
        assert m._rho_f is None                                           # rho has not crossed PCIe
        Ys = np.asarray([m.sample_inferred_model(N=1, seed=sd + s, device=True)[0] for s in range(S)])
        for s in range(S):
            exact_ok(adjacency(Ys[s, 0], "out"), 0.25, 6)
        want = centrality_np(Ys, 0.25, 6, "out", top_k=5)
        assert want["values"].max() > 0
        for k in ALL_KEYS:
            assert np.array_equal(getattr(res, k), want[k]), k
        assert np.array_equal(res.mean, want["node_sum"] / S) and np.array_equal(res.expected_rank, want["node_rank_sum"] / S)
        assert (res.top_prob >= 0).all() and (res.top_prob <= 1).all() and res.top_prob.sum() >= 5
        assert (res.sd >= 0).all() and res.sd.max() > 0
        assert np.array_equal(res.plug_in, m._engine.mean_centrality(0.25, 6, direction="out"))
        assert res.top(5).shape == (5,) and len(res.frame()) == m.L * m.N and len(res.summary()) == 2 * m.L
        # q None: the reciprocal of the expected mean degree, per layer
        auto = m.posterior_centrality(T=3, direction="union", n_samples=S, seed=sd)
        q = default_q(m.N, m._engine.expected_stats()["edges"])
        assert np.array_equal(auto.q, q) and (q > 0).all() and (q < 1).all() and auto.values is None
        assert np.array_equal(auto.node_sum, m._engine.sample_centrality(sd, S, q, 3, direction="union")["node_sum"])
        assert np.array_equal(auto.plug_in, m._engine.mean_centrality(q, 3, direction="union"))
        # the dyad and the connectivity read-outs are what they were
        base2 = m.posterior_network_stats(n_samples=S, seed=sd)
        conn2 = m.posterior_connectivity(n_samples=S, seed=sd)
        for k, v in base.statistics().items():
            assert np.array_equal(v, base2.statistics()[k], equal_nan=True), k
        for k, v in conn.statistics().items():
            assert np.array_equal(v, conn2.statistics()[k], equal_nan=True), k
    finally:
        m.close()
