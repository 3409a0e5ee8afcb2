"""GPU: cascades on posterior samples and on given networks (vmr_sample_outreach, vmr_sample_seed_outreach, vmr_network_outreach,
vmr_network_seed_outreach), held to the NumPy restatement (tests/cascade_util.py) on the samples `CaviEngine.sample` returns for
the same seeds.  The live ties are a counter-based draw and everything after them is an integer: every comparison is `==` on
arrays of the documented dtype and shape.  Both data layouts, the general kernels (K = 12), a coordinate-list handle; the merged
connectivity unit as a cross-check; every word boundary and the node bound; depth and the period cut; seed sets; several chunks,
two runs; the argument errors; the model's method."""
import warnings

import numpy as np
import pytest

from tests.cascade_util import (DIRECTIONS, NODE_KEYS, NPER, adjacency, outreach_np, outreach_values, path, path_outreach, random_digraph,
                                reduce_values, seed_outreach_np, set_words, star, star_outreach, two_cliques, two_cliques_outreach)
from tests.golden_util import case_config, load_case
from tests.test_hip_betweenness import _stateless
from tests.test_hip_centrality import _medium_case
from tests.test_hip_netstats import _engine_for, _golden_state

pytestmark = pytest.mark.gpu

ALL_KEYS = NODE_KEYS + ("values",)
SET_KEYS = ("values", "curve", "node_hits")


def _assert_equal(got, want, keys=ALL_KEYS, what=None):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, what, got[k].dtype, want[k].dtype)
        assert np.array_equal(got[k], want[k]), (k, what)


def _layer_q(L):
    """A different passing probability per layer, strictly inside (0, 1)."""
    return 0.35 + 0.4 * np.arange(L) / max(L, 1)


def _check(eng, seed, S, trials=(1,), Ts=(1, 3, 64), K=3, top_k=3):
    """`sample_outreach` with every output against the restatement on the samples of the same seeds, the reductions recomputed
    from the values, and `network_outreach` of the same samples."""
    q, cs = _layer_q(eng.L), seed + 1000
    for n_trials in trials:
        Ys = np.asarray([eng.sample(seed + s, n_trials) for s in range(S)])
        for d in DIRECTIONS:
            for T in Ts:
                what = (n_trials, d, T)
                want = outreach_np(Ys, cs, K, q, T, d, top_k)
                got = eng.sample_outreach(seed, S, q, T=T, direction=d, n_cascades=K, cascade_seed=cs, top_k=top_k, n_trials=n_trials, values=True)
                assert sorted(got) == sorted(ALL_KEYS)
                assert got["values"].dtype == np.uint32 and got["values"].shape == (S, eng.L, eng.N)
                _assert_equal(got, want, what=what)
                _assert_equal(got, reduce_values(got["values"], K, top_k), keys=NODE_KEYS, what=what)
                vals, sm = eng.network_outreach(Ys, q, T=T, direction=DIRECTIONS.index(d), n_cascades=K, cascade_seed=cs, summary=True)
                assert vals.dtype == np.uint32 and np.array_equal(vals, got["values"]), what
                assert np.array_equal(sm["total"], got["total"]) and np.array_equal(sm["max"], got["max"]), what
        assert want["values"].any()


@pytest.mark.parametrize("case", ["A_ones_mut", "B_random_mask_K3", "D_self_mask", "E_undirected"])
def test_outreach_against_the_restatement(case, vmr_format):
    d = load_case(case)
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        assert eng.data_format()[0] == vmr_format
        _check(eng, 11, 8, trials=(1, 3))
    finally:
        eng.close()


def test_outreach_against_the_restatement_general_kernels():
    d = load_case("L_default_K12")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    assert K > 8
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        _check(eng, 5, 8)
    finally:
        eng.close()


def test_outreach_against_the_restatement_coo_handle():
    d = load_case("D_self_mask")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d), coo=True)
    try:
        _check(eng, 3, 8)
    finally:
        eng.close()


def test_cross_checks_against_merged_units():
    """On one engine and the same seeds.  q = 1, T = N, one cascade: the outreach is `sample_connectivity`'s node_reach_out, "in"
    its node_reach_in.  q = 1, T = 1: the out-degrees of the samples, diagonal cleared.  q = 0: zeros."""
    d = load_case("B_random_mask_K3")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        S, sd, N = 8, 21, eng.N
        conn = eng.sample_connectivity(sd, S, nodes=True)
        out = eng.sample_outreach(sd, S, 1.0, T=N, direction="out", n_cascades=1, cascade_seed=5, values=True)["values"]
        inn = eng.sample_outreach(sd, S, 1.0, T=N, direction="in", n_cascades=1, cascade_seed=5, values=True)["values"]
        assert conn["node_reach_out"].any() and (conn["node_reach_out"] != conn["node_reach_in"]).any()
        assert np.array_equal(out, conn["node_reach_out"].astype(np.uint32)) and np.array_equal(inn, conn["node_reach_in"].astype(np.uint32))
        A = adjacency(np.asarray([eng.sample(sd + s) for s in range(S)]))
        one = eng.sample_outreach(sd, S, 1.0, T=1, direction="out", n_cascades=1, values=True)
        assert np.array_equal(one["values"], A.sum(axis=-1).astype(np.uint32))
        assert np.array_equal(eng.sample_outreach(sd, S, 1.0, T=1, direction="in", n_cascades=4, values=True)["values"],
                              4 * A.sum(axis=-2).astype(np.uint32))
        for dr in DIRECTIONS:
            zero = eng.sample_outreach(sd, S, 0.0, T=5, direction=dr, n_cascades=2, values=True)
            assert not zero["values"].any() and not zero["node_sum"].any() and not zero["node_rank_sum"].any()
            assert np.array_equal(zero["node_top"], np.full((eng.L, N), S))                # everybody ties at rank 0
    finally:
        eng.close()


def _sets_for(N, rng):
    """Five seed sets on N nodes: a single node, the last node with a random handful (overlapping the others), the empty set,
    every third node, the first node again beside the last."""
    return [[1], sorted(set([N - 1] + list(rng.randint(0, N, 5)))), [], list(range(0, N, 3)), [1, N - 1]]


def _check_networks(N, Ys, q, Ts, K=2, cs=40):
    """`network_outreach` and `network_seed_outreach` of the networks Ys [n][N, N] (L = 1) on a handle with no state against the
    restatement, every direction."""
    Y4 = np.asarray(Ys)[:, None]
    sets = _sets_for(N, np.random.RandomState(N))
    eng = _stateless(1, N)
    try:
        for d in DIRECTIONS:
            for T in Ts:
                want = outreach_values(Y4, cs, K, q, T, d)
                vals, sm = eng.network_outreach(Y4, q, T=T, direction=d, n_cascades=K, cascade_seed=cs, summary=True)
                assert vals.dtype == np.uint32 and vals.shape == (len(Y4), 1, N)
                assert np.array_equal(vals, want), (N, d, T)
                red = reduce_values(want, K, 1)
                assert sm["total"].dtype == np.int64 and np.array_equal(sm["total"], red["total"]) and np.array_equal(sm["max"], red["max"])
                assert np.array_equal(eng.network_outreach(Y4[0], q, T=T, direction=d, n_cascades=K, cascade_seed=cs), want[0])
                got = eng.network_seed_outreach(Y4, sets, q, T=T, direction=d, n_cascades=K, cascade_seed=cs, node_hits=True)
                _assert_equal(got, seed_outreach_np(Y4, cs, K, q, T, d, sets), keys=SET_KEYS, what=(N, d, T))
                assert np.array_equal(got["values"][..., 0], want[..., 1])                  # the set {1} is node 1's own outreach
        assert want.any()
    finally:
        eng.close()


@pytest.mark.parametrize("N", [63, 64, 65, 129, 257])
def test_word_boundaries(N):
    """W = ceil(N / 64) = 1, 1, 2, 3, 5 words per bit row, one to four lanes per row: a sparse random digraph (2 ties per node)
    and a dense one (N / 4), random diagonal entries, 0 < q < 1."""
    sparse, dense = random_digraph(N, 2.0, N), random_digraph(N, N / 4.0, 2 * N)
    sparse[N - 1, 0], sparse[1, N - 1] = 1, 2                                             # the last word's node has ties both ways
    assert sparse.diagonal().any() and dense.diagonal().any()
    _check_networks(N, [sparse, dense], 0.45, (1, 5))


@pytest.mark.parametrize("N", [513, 1024, 1025])
def test_wide_rows(N):
    """W = 9, 16, 17: 8 and 16 lanes per row, a second trip of the word stride, three to five nodes per thread."""
    Y = random_digraph(N, 2.0, N)
    Y[N - 1, 0], Y[1, N - 1] = 1, 2
    _check_networks(N, [Y], 0.7, (4,))


def test_the_node_bound():
    """N = CASC_NMAX = 2048, L = 2: 32 words per bit row, 48 KiB of LDS, threads own eight nodes.  q = 1 designs with closed
    forms: the path (2047 periods deep) and the star."""
    from vimure_amd import _lib
    N = _lib.CASC_NMAX
    Y = np.stack([path(N), star(N)])
    eng = _stateless(2, N)
    try:
        for d in DIRECTIONS:
            for T in (3, 65535):
                vals, sm = eng.network_outreach(Y, 1.0, T=T, direction=d, n_cascades=2, cascade_seed=9, summary=True)
                want = 2 * np.stack([path_outreach(N, T, d), star_outreach(N, T, d)])
                assert vals.dtype == np.uint32 and np.array_equal(vals, want.astype(np.uint32)), (d, T)
                assert np.array_equal(sm["total"], want.sum(axis=1) % 2 ** 32) and np.array_equal(sm["max"], want.max(axis=1))
        sets = [[0], [N - 1], list(range(N)), [], [5, 1000]]
        got = eng.network_seed_outreach(Y, sets, 1.0, T=65535, direction="out", n_cascades=1, node_hits=True)
        assert np.array_equal(got["values"], np.array([[N - 1, 0, 0, 0, N - 7], [N - 1, 0, 0, 0, 0]], np.uint32))
        assert np.array_equal(got["curve"].sum(axis=-1), got["values"].astype(np.int64))
        assert np.array_equal(got["curve"][0, 0], np.r_[np.ones(NPER - 1, np.int64), N - 1 - (NPER - 1)])
        assert np.array_equal(got["curve"][1, 0], np.r_[N - 1, np.zeros(NPER - 1, np.int64)])
        assert np.array_equal(got["node_hits"][0, 4], (np.arange(N) >= 5).astype(np.int64)) and got["node_hits"][:, 0].all()
        assert np.array_equal(got["node_hits"][1, 4], np.isin(np.arange(N), [5, 1000]).astype(np.int64))
    finally:
        eng.close()


def test_more_nodes_than_the_bound_are_refused():
    """A coordinate-list handle of VMR_CASC_NMAX + 1 nodes and no state: every call refuses it for its N, not for its state."""
    from vimure_amd import _lib
    from vimure_amd.engine import CascadeArgumentError
    N = _lib.CASC_NMAX + 1
    eng = _stateless(1, N)
    try:
        Y = np.zeros((1, N, N), np.uint8)
        for name, call in (("vmr_sample_outreach", lambda: eng.sample_outreach(1, 2, 0.5)),
                           ("vmr_sample_seed_outreach", lambda: eng.sample_seed_outreach(1, 2, [[0]], 0.5)),
                           ("vmr_network_outreach", lambda: eng.network_outreach(Y, 0.5)),
                           ("vmr_network_seed_outreach", lambda: eng.network_seed_outreach(Y, [[0]], 0.5))):
            with pytest.raises(CascadeArgumentError, match=name + ".*N <= %d" % _lib.CASC_NMAX):
                call()
            assert b"LDS" in eng.lib.vmr_last_error(eng._h)
    finally:
        eng.close()


def test_depth_and_the_period_cut():
    """The path of 300 at q = 1: T = 7, 64, 299 and 65535 against the closed form and the restatement; the seed set {0} fills
    one bin per period, the last bin collects every period >= 64 and the bins sum to the outreach; beside it the two cliques
    joined by a bridge, a mutual pair and isolated nodes."""
    N = 300
    Y = np.stack([path(N), two_cliques(N)])
    sets = [[0], [150, 299], [19], []]
    eng = _stateless(2, N)
    try:
        for T in (7, 64, 299, 65535):
            for d in DIRECTIONS:
                vals = eng.network_outreach(Y, 1.0, T=T, direction=d, n_cascades=1)
                assert np.array_equal(vals[0], path_outreach(N, T, d).astype(np.uint32)), (T, d)
                assert np.array_equal(vals[1], two_cliques_outreach(N, T, d).astype(np.uint32)), (T, d)
            got = eng.network_seed_outreach(Y[None], sets, 1.0, T=T, direction="out", n_cascades=3, cascade_seed=T, node_hits=True)
            _assert_equal(got, seed_outreach_np(Y[None], T, 3, 1.0, T, "out", sets), keys=SET_KEYS, what=T)
            reach = min(T, N - 1)
            assert got["values"][0, 0, 0] == 3 * reach and np.array_equal(got["curve"].sum(axis=-1), got["values"][0].astype(np.int64))
            assert np.array_equal(got["curve"][0, 0, :NPER - 1], 3 * (np.arange(1, NPER) <= reach))
            assert got["curve"][0, 0, NPER - 1] == 3 * max(reach - (NPER - 1), 0)
            assert got["values"][0, 1, 2] == 3 * (19 + 1 + 19)         # the bridge's tail: its clique, the head, the head's clique
    finally:
        eng.close()


def test_seed_sets():
    """64 sets on a sampled handle -- one empty, one holding every node, overlapping ones, a node in several sets -- and n_sets =
    1, against the restatement, curve and node_hits included; the singleton {v} gives `sample_outreach`'s value of v for the same
    seeds (the two closures agree); a seed bit at n_sets is refused."""
    from vimure_amd.engine import CascadeArgumentError
    d = load_case("B_random_mask_K3")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        S, sd, cs, N, L = 6, 31, 77, eng.N, eng.L
        q = _layer_q(L)
        rng = np.random.RandomState(3)
        sets = [[], list(range(N)), [0], [0, 1], [0, N - 1]] + [sorted(set(rng.randint(0, N, 1 + b % 7))) for b in range(59)]
        assert len(sets) == 64 and sum(0 in s for s in sets) >= 4
        Ys = np.asarray([eng.sample(sd + s) for s in range(S)])
        for dr in DIRECTIONS:
            got = eng.sample_seed_outreach(sd, S, sets, q, T=3, direction=dr, n_cascades=3, cascade_seed=cs, node_hits=True)
            assert got["values"].shape == (S, L, 64) and got["curve"].shape == (L, 64, NPER) and got["node_hits"].shape == (L, 64, N)
            _assert_equal(got, seed_outreach_np(Ys, cs, 3, q, 3, dr, sets), keys=SET_KEYS, what=dr)
            assert not got["values"][..., 0].any() and not got["values"][..., 1].any() and got["values"].any()
            assert np.array_equal(got["node_hits"][:, 1], np.full((L, N), 3 * S)) and not got["node_hits"][:, 0].any()
            net = eng.network_seed_outreach(Ys, sets, q, T=3, direction=dr, n_cascades=3, cascade_seed=cs, node_hits=True)
            _assert_equal(net, got, keys=SET_KEYS, what=dr)
            # singletons, 64 nodes at a time, against the every-node closure
            every = eng.sample_outreach(sd, S, q, T=3, direction=dr, n_cascades=3, cascade_seed=cs, values=True)["values"]
            for v0 in range(0, N, 64):
                nodes = list(range(v0, min(v0 + 64, N)))
                single = eng.sample_seed_outreach(sd, S, [[v] for v in nodes], q, T=3, direction=dr, n_cascades=3, cascade_seed=cs, curve=False)
                assert sorted(single) == ["values"] and np.array_equal(single["values"], every[..., nodes]), (dr, v0)
        one = eng.sample_seed_outreach(sd, S, [[2, 3]], q, T=2, n_cascades=2, cascade_seed=cs, node_hits=True)
        assert one["values"].shape == (S, L, 1)
        _assert_equal(one, seed_outreach_np(Ys, cs, 2, q, 2, "out", [[2, 3]]), keys=SET_KEYS)
        words = set_words([[0], [1, 2]], N)
        assert np.array_equal(eng.seed_words([[0], [1, 2]])[0], words)
        ok = eng.sample_seed_outreach(sd, 2, words, q, n_sets=2, curve=False)
        assert ok["values"].shape == (2, L, 2)
        with pytest.raises(CascadeArgumentError, match=r"vmr_sample_seed_outreach: seed_words\[1\].*n_sets = 1"):
            eng.sample_seed_outreach(sd, 2, words, q, n_sets=1)
        with pytest.raises(CascadeArgumentError, match=r"vmr_network_seed_outreach: seed_words\[1\].*n_sets = 1"):
            eng.network_seed_outreach(Ys, words, q, n_sets=1)
        with pytest.raises(CascadeArgumentError, match="seed set 0 names a node"):
            eng.sample_seed_outreach(sd, 2, [[N]], q)
        with pytest.raises(CascadeArgumentError, match="between 1 and 64"):
            eng.sample_seed_outreach(sd, 2, [[0]] * 65, q)
    finally:
        eng.close()


def test_chunks_and_reruns(monkeypatch):
    """L = 2, N = 300, K = 3 on report lists, 8 samples: one chunk against chunks of 3 samples (8 = 3 + 3 + 2; the key of a
    sample is its global index) and against a second run, every array identical; the networks' upload loop the same way."""
    X, st = _medium_case()
    seed, S, cs, q = 1000, 8, 123, [0.01, 0.02]     # (about 200 ties per node: a q at which nothing saturates)
    sets = [[0, 5], [299], list(range(0, 300, 7))]

    def run():
        eng = _engine_for(X, None, 3, True, st)
        try:
            out = {}
            for _ in range(2):
                res = {d: eng.sample_outreach(seed, S, q, T=2, direction=d, n_cascades=2, cascade_seed=cs, values=True) for d in DIRECTIONS}
                res["sets"] = eng.sample_seed_outreach(seed, S, sets, q, T=2, n_cascades=2, cascade_seed=cs, node_hits=True)
                Ys = np.asarray([eng.sample(seed + s) for s in range(S)])
                vals, sm = eng.network_outreach(Ys, q, T=2, n_cascades=2, cascade_seed=cs, summary=True)
                res["net"] = dict(sm, values=vals)
                res["netsets"] = eng.network_seed_outreach(Ys, sets, q, T=2, n_cascades=2, cascade_seed=cs, node_hits=True)
                if out:
                    for k in res:
                        _assert_equal(res[k], out[k], keys=sorted(out[k]), what=("rerun", k))
                out = res
            return out, Ys
        finally:
            eng.close()

    monkeypatch.setenv("VMR_FORMAT", "sparse")
    monkeypatch.delenv("VMR_NETSTATS_CHUNK", raising=False)
    one, Ys = run()
    monkeypatch.setenv("VMR_NETSTATS_CHUNK", "3")
    many, _ = run()
    for k in one:
        _assert_equal(many[k], one[k], keys=sorted(one[k]), what=("chunks", k))
    assert np.array_equal(one["out"]["values"], one["net"]["values"]) and np.array_equal(one["out"]["total"], one["net"]["total"])
    _assert_equal(one["sets"], one["netsets"], keys=SET_KEYS)
    assert np.array_equal(one["out"]["values"][:2], outreach_values(Ys[:2], cs, 2, q, 2, "out"))
    _assert_equal(one["union"], reduce_values(one["union"]["values"], 2, 10), keys=NODE_KEYS)
    assert (one["out"]["values"][:3] != one["out"]["values"][3:6]).any()


def test_optional_outputs():
    """node_sum alone, and node_sum with each other output alone (the raw call, the others NULL)."""
    from vimure_amd import _lib
    d = load_case("B_random_mask_K3")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        S, top_k, L, N = 4, 3, eng.L, eng.N
        q = np.ascontiguousarray(_layer_q(L))
        full = eng.sample_outreach(9, S, q, T=3, direction="union", n_cascades=2, cascade_seed=4, top_k=top_k, values=True)
        plain = eng.sample_outreach(9, S, q, T=3, direction="union", n_cascades=2, cascade_seed=4, top_k=top_k)
        assert sorted(plain) == sorted(NODE_KEYS)
        _assert_equal(plain, full, keys=NODE_KEYS)
        outs = [("node_sumsq", np.full((L, N), -1.0)), ("node_rank_sum", np.full((L, N), 7, np.uint64)),
                ("node_top", np.full((L, N), 7, np.uint32)), ("summary", np.full((S, L, 2), 7, np.uint32)),
                ("values", np.full((S, L, N), 7, np.uint32))]
        for pick in [None] + list(range(len(outs))):
            ns = np.full((L, N), -1.0)
            ptrs = [a.ctypes.data if i == pick else None for i, (_, a) in enumerate(outs)]
            assert eng.lib.vmr_sample_outreach(eng._h, 9, S, 1, 4, 2, q.ctypes.data, 3, 2, top_k, ns.ctypes.data, *ptrs) == _lib.VMR_OK
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
    from vimure_amd.engine import CascadeArgumentError, EngineError
    d = load_case("A_ones_mut")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, None)
    try:
        L, N = eng.L, eng.N
        ns, Y = np.zeros((L, N)), np.zeros((1, L, N, N), np.uint8)
        q, nan, big, neg = np.full(L, 0.5), np.full(L, 0.5), np.full(L, 0.5), np.full(L, 0.5)
        nan[L - 1], big[L - 1], neg[0] = np.nan, 1.5, -0.1
        inf = np.full(L, np.inf)
        words, high = np.zeros(N, np.uint64), np.zeros(N, np.uint64)
        words[0], high[N - 1] = 1, 2
        vn, vs = np.full((1, L, N), 9, np.uint32), np.full((2, L, 1), 9, np.uint32)
        lib, h = eng.lib, eng._h

        def nodes(S=2, n_trials=1, K=2, qp=q, T=3, dr=0, top_k=1, nsp=ns.ctypes.data):
            return lib.vmr_sample_outreach(h, 1, S, n_trials, 7, K, None if qp is None else qp.ctypes.data, T, dr, top_k, nsp, *[None] * 5)

        def sets(S=2, n_trials=1, K=2, qp=q, T=3, dr=0, w=words, n_sets=1, out=vs.ctypes.data):
            return lib.vmr_sample_seed_outreach(h, 1, S, n_trials, 7, K, None if qp is None else qp.ctypes.data, T, dr,
                                                None if w is None else w.ctypes.data, n_sets, out, None, None)

        def net(Yp=Y.ctypes.data, n=1, K=2, qp=q, T=3, dr=0, out=vn.ctypes.data):
            return lib.vmr_network_outreach(h, Yp, n, 7, K, None if qp is None else qp.ctypes.data, T, dr, out, None)

        def netsets(Yp=Y.ctypes.data, n=1, K=2, qp=q, T=3, dr=0, w=words, n_sets=1, out=vs.ctypes.data):
            return lib.vmr_network_seed_outreach(h, Yp, n, 7, K, None if qp is None else qp.ctypes.data, T, dr,
                                                 None if w is None else w.ctypes.data, n_sets, out, None, None)

        names = {nodes: b"vmr_sample_outreach", sets: b"vmr_sample_seed_outreach", net: b"vmr_network_outreach",
                 netsets: b"vmr_network_seed_outreach"}
        shared = [({"K": 0}, b"n_cascades"), ({"K": _lib.CASC_KMAX + 1}, b"n_cascades"), ({"T": 0}, b"T must"),
                  ({"T": _lib.CASC_TMAX + 1}, b"T must"), ({"dr": 3}, b"direction"), ({"dr": -1}, b"direction"), ({"qp": None}, b"q is NULL"),
                  ({"qp": nan}, b"q[%d]" % (L - 1)), ({"qp": big}, b"q[%d]" % (L - 1)), ({"qp": neg}, b"q[0]"), ({"qp": inf}, b"q[0]")]
        bad = [(fn, kw, word) for fn in names for kw, word in shared]
        bad += [(fn, kw, word) for fn in (nodes, sets) for kw, word in (({"S": 0}, b"n_samples"), ({"n_trials": 0}, b"n_trials"))]
        bad += [(fn, kw, word) for fn in (net, netsets) for kw, word in (({"n": 0}, b"n must"), ({"Yp": None}, b"Y is NULL"))]
        bad += [(fn, kw, word) for fn in (sets, netsets) for kw, word in (({"n_sets": 0}, b"n_sets"), ({"n_sets": 65}, b"n_sets"),
                                                                           ({"w": None}, b"seed_words is NULL"),
                                                                           ({"w": high}, b"seed_words[%d]" % (N - 1)),
                                                                           ({"out": None}, b"values is NULL"))]
        bad += [(nodes, {"top_k": 0}, b"top_k"), (nodes, {"top_k": N + 1}, b"top_k"), (nodes, {"nsp": None}, b"node_sum"),
                (net, {"out": None}, b"values is NULL")]

        def check_bad():
            for fn, kw, word in bad:
                assert fn(**kw) == _lib.VMR_EINVAL, (names[fn], kw)
                err = lib.vmr_last_error(h)
                assert word in err and names[fn] + b":" in err, (names[fn], kw, err)

        # before vmr_set_state: the state is what is missing, unless an argument is refused first; the networks' calls need none
        for call in (lambda: eng.sample_outreach(1, 2, 0.5), lambda: eng.sample_seed_outreach(1, 2, [[0]], 0.5)):
            with pytest.raises(EngineError, match="vmr_set_state") as ei:
                call()
            assert not isinstance(ei.value, CascadeArgumentError)
        assert nodes() == _lib.VMR_ESTATE and sets() == _lib.VMR_ESTATE
        assert net() == _lib.VMR_OK and not vn.any() and netsets() == _lib.VMR_OK and not vs[:1].any()
        check_bad()
        eng.set_state(*_golden_state(d))
        check_bad()
        for kw, word in (({"n_samples": 0}, "n_samples"), ({"n_trials": 0}, "n_trials"), ({"top_k": 0}, "top_k"), ({"top_k": N + 1}, "top_k"),
                         ({"T": 0}, "T must"), ({"n_cascades": 0}, "n_cascades"), ({"direction": "both"}, "direction"), ({"direction": 3}, "direction"),
                         ({"q": 1.5}, "q"), ({"q": np.full(L + 1, 0.5)}, "q must"), ({"q": "x"}, "q must")):
            args = dict(seed=1, n_samples=2, q=0.5)
            args.update(kw)
            with pytest.raises(CascadeArgumentError, match=word):
                eng.sample_outreach(**args)
        with pytest.raises(CascadeArgumentError, match="direction"):
            eng.network_outreach(Y[0], 0.5, direction="directed")
        with pytest.raises(CascadeArgumentError, match="shape"):
            eng.network_outreach(np.zeros((L, N, N + 1), np.uint8), 0.5)
        # the ends of every range are accepted, and the handle still works
        got = eng.sample_outreach(1, 1, 1.0, T=_lib.CASC_TMAX, direction=2, n_cascades=1, top_k=N)
        assert got["node_sum"].shape == (L, N) and np.array_equal(got["node_top"], np.full((L, N), 1))
        assert eng.sample_seed_outreach(1, 1, [[0]] * 64, 0.0, T=1, n_cascades=1)["values"].shape == (1, L, 64)
    finally:
        eng.close()


def test_model_posterior_cascades():
    import pandas as pd
    from vimure_amd import CascadeStats, SeedOutreach, VimureModel
    from vimure_amd.centrality import default_q
    from vimure_amd.synthetic import standard_sbm
    net = standard_sbm(N=60, M=8, L=1, K=2, avg_degree=6.0, eta=0.4, seed=4)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = VimureModel(mutuality=True)
        m.fit(net.X, K=2, seed=1, max_iter=30, num_realisations=1, keep_engine=True)
    try:
        S, sd, Kc = 8, 321, 4
        res = m.posterior_cascades(T=3, n_cascades=Kc, n_samples=S, seed=sd, top_k=5, values=True)
        assert isinstance(res, CascadeStats) and m._rho_f is None                  # rho has not crossed PCIe
        q = default_q(m.N, m._engine.expected_stats()["edges"])
        assert np.array_equal(res.q, q) and (q > 0).all() and res.cascade_seed == sd
        Ys = np.asarray([m.sample_inferred_model(N=1, seed=sd + s, device=True)[0] for s in range(S)])
        want = outreach_np(Ys, sd, Kc, q, 3, "out", 5)
        assert res.values.dtype == np.uint32 and np.array_equal(res.values, want["values"]) and want["values"].any()
        for k in NODE_KEYS:
            assert np.array_equal(getattr(res, k), want[k]), k
        assert np.array_equal(res.mean, want["node_sum"] / S)
        Yinf = m.get_inferred_model()
        inf = m._engine.network_outreach(Yinf, q, T=3, n_cascades=Kc, cascade_seed=sd)
        assert res.inferred.shape == (m.L, m.N) and np.array_equal(res.inferred, inf) and inf.any()
        assert np.array_equal(res.inferred, outreach_values(np.asarray(Yinf)[None], sd, Kc, q, 3, "out")[0])
        for name in ("mean", "sd", "expected_rank", "top_prob", "inferred_score"):
            assert getattr(res, name).shape == (m.L, m.N), name
        assert res.top(5).shape == (5,) and len(res.frame()) == m.L * m.N and len(res.summary()) == 2 * m.L
        tmp = m.posterior_cascades(T=3, n_cascades=Kc, n_samples=S, seed=sd, top_k=5, X=net.X)     # a temporary engine
        assert tmp.values is None
        for k in NODE_KEYS:
            assert np.array_equal(getattr(tmp, k), want[k]), k
        assert np.array_equal(tmp.inferred, inf)
        # seed sets by index, then by node name
        seeds = {"pair": [3, 17], "one": [40], "none": []}
        got = m.posterior_cascades(q=0.5, T=2, direction="union", seeds=seeds, n_cascades=Kc, n_samples=S, seed=sd, cascade_seed=9)
        assert isinstance(got, SeedOutreach) and got.labels == ["pair", "one", "none"] and got.sets == [[3, 17], [40], []]
        eng = m._engine.sample_seed_outreach(sd, S, [[3, 17], [40], []], 0.5, T=2, direction="union", n_cascades=Kc, cascade_seed=9,
                                             node_hits=True)
        assert np.array_equal(got.values, eng["values"]) and np.array_equal(got.curve_counts, eng["curve"])
        assert np.array_equal(got.node_hits, eng["node_hits"]) and got.values.any()
        assert np.array_equal(got.mean, eng["values"].astype(np.float64).mean(axis=0) / Kc) and got.sd.shape == (m.L, 3)
        assert got.quantiles().shape == (3, m.L, 3) and got.curve().shape == (m.L, 3, NPER) and np.isnan(got.curve()[0, 2]).all()
        assert np.nanmax(got.curve()[..., -1]) == 1.0 and (got.reach_prob()[0, 0, [3, 17]] == 1.0).all()
        assert len(got.frame()) == 3 * m.L and len(got.summary()) == 3 * m.L
        m.nodeNames = pd.DataFrame({"id": np.arange(m.N), "name": ["hh%d" % i for i in range(m.N)]})
        named = m.posterior_cascades(q=0.5, T=2, direction="union", seeds={"pair": ["hh3", "hh17"], "one": ["hh40"], "none": []},
                                     n_cascades=Kc, n_samples=S, seed=sd, cascade_seed=9, X=net.X)
        assert named.sets == got.sets and np.array_equal(named.values, got.values) and np.array_equal(named.node_hits, got.node_hits)
        with pytest.raises(ValueError, match="not a node"):
            m.posterior_cascades(seeds={"x": ["nobody"]}, n_samples=2)
    finally:
        m.close()
