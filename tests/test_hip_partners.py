"""GPU: the shared partners of posterior samples and of given networks on the device (vmr_sample_shared_partners,
vmr_network_shared_partners), held to the definition `tests/partners_util.partners_np` on the samples `CaviEngine.sample` returns
for the same seeds.  Everything is exact integer arithmetic: every comparison is `==`.  Golden cases in both data layouts, the
general kernels (K = 12), a coordinate-list handle; every word boundary; closed forms; a one-hot rho; several chunks and two runs;
every class of the kernels' launch shape (tests/partners_util.SHAPE_NS names what each N is for); listed pairs; the argument
errors; the model's method."""
import functools
import warnings

import numpy as np
import pytest

from tests.census_util import boundary_graph, reversed_nodes
from tests.golden_util import case_config, load_case
from tests.graph_shapes_util import design, design_large, one_hot_rho
from tests.partners_util import MAX_BINS, MODES, book, closed_forms, fold, partners_np, transposed_ends
from tests.test_hip_betweenness import _stateless
from tests.test_hip_census import _design_engine
from tests.test_hip_centrality import _engine_with_rho, _medium_case
from tests.test_hip_netstats import _engine_for, _golden_state

pytestmark = pytest.mark.gpu

PER_SAMPLE = ("hist", "totals", "node_ties", "node_supported")
PAIR_SUMS = ("pair_present", "pair_supported", "pair_partners")


def _assert_counts(got, want, what="", pair_sums=False, net=False, nodes=True):
    """The dict of an engine call against the dict of `partners_np` (its leading axis dropped by the caller where the call's is)."""
    keys = [k for k in PER_SAMPLE if nodes or not k.startswith("node")] + (list(PAIR_SUMS) if pair_sums else [])
    for k in keys:
        w = want[k]
        assert got[k].dtype == (np.int32 if k.startswith("node") else np.int64) and got[k].shape == w.shape, (what, k, got[k].shape, w.shape)
        assert np.array_equal(got[k], w), (what, k, np.argwhere(got[k] != w)[:5].tolist())
    if net:
        assert got["pair_partners"].dtype == np.int32 and np.array_equal(got["pair_partners"], want["pair_partners_net"]), (what, "pairs of the networks")
    assert set(got) == set(keys) | ({"pair_partners"} if net else set()), what


def _first(d, q=0):
    """Entry q along the leading axis of the per-sample (per-network) arrays of a result or a reference."""
    return {k: v[q] for k, v in d.items() if k in PER_SAMPLE or k == "pair_partners_net"}


def _some_pairs(Ys, n=40, seed=0):
    """Pairs (layer, i, j) for the networks Ys [S, L, N, N]: ties of the first network in both orders, its first tie twice, the
    last node, and random pairs, most of them untied."""
    Ys = np.asarray(Ys)
    L, N = Ys.shape[1:3]
    g = np.random.RandomState(seed)
    T = np.argwhere((Ys[0] > 0) & ~np.eye(N, dtype=bool)[None])
    tied = T[g.permutation(len(T))[:n // 2]]
    rnd = np.stack([g.randint(0, L, n), g.randint(0, N, n), g.randint(0, N, n)], axis=1)
    rnd = rnd[rnd[:, 1] != rnd[:, 2]]
    p = np.concatenate([tied, tied[:, [0, 2, 1]], tied[:1], rnd, [[L - 1, N - 1, 0], [0, 1, N - 1]]])
    return np.ascontiguousarray(p, dtype=np.int32)


def _check(eng, seed, S, trials=(1,), n_bins=64):
    """`sample_shared_partners` in every mode, with nodes and a pair list, against `partners_np` of the samples of the same seeds;
    `network_shared_partners` of those samples; the pair accumulators against the per-sample reference, summed."""
    for n_trials in trials:
        Ys = np.asarray([eng.sample(seed + s, n_trials) for s in range(S)])
        pairs = _some_pairs(Ys, seed=seed)
        for mode in MODES:
            want = partners_np(Ys, mode, n_bins, pairs)
            what = (mode, "n_trials %d" % n_trials)
            got = eng.sample_shared_partners(seed, S, n_trials=n_trials, mode=mode, n_bins=n_bins, nodes=True, pairs=pairs)
            _assert_counts(got, want, what, pair_sums=True)
            assert np.array_equal(want["pair_present"], (want["pair_partners_net"] >= 0).sum(axis=0))
            _assert_counts(eng.network_shared_partners(Ys, mode=mode, n_bins=n_bins, nodes=True, pairs=pairs), want, what + ("networks",), net=True)
            one = eng.network_shared_partners(Ys[0], mode=mode, n_bins=n_bins)
            _assert_counts(one, _first(want), what + ("one network",), nodes=False)
        assert want["totals"][..., 0].all()


@pytest.mark.parametrize("case", ["A_ones_mut", "B_random_mask_K3", "D_self_mask", "E_undirected"])
def test_golden_cases(case, vmr_format):
    d = load_case(case)
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        assert eng.data_format()[0] == vmr_format
        _check(eng, 11, 8, trials=(1, 3))
    finally:
        eng.close()


def test_general_kernels():
    d = load_case("L_default_K12")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    assert K > 8
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        _check(eng, 5, 8, trials=(1, 3))
    finally:
        eng.close()


def test_coo_handle():
    d = load_case("D_self_mask")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d), coo=True)
    try:
        _check(eng, 3, 8, trials=(1, 3))
    finally:
        eng.close()


@pytest.mark.parametrize("N", [63, 64, 65, 129, 257])
def test_word_boundaries(N):
    """W = 1, 1, 2, 3 and 5 words per bit row on 1, 1, 2, 2 and 4 lanes, on a handle with no state: random digraphs with 2 and with
    N / 4 ties per node, a drawn diagonal, entries up to 3, node N - 1 tied both ways; the book, whose spine has bits in the first
    and in the last word; all of them transposed.  Union and mutual do not see the transposition; path mode of the transpose is
    path mode with the ends of every tie swapped."""
    sparse, dense, bk = boundary_graph(N, 2.0, N), boundary_graph(N, N / 4.0, 2 * N), book(N)
    assert sparse.diagonal().any() and dense.diagonal().any() and sparse.max() == 3
    Y = np.stack([sparse, dense, bk])[:, None]
    Yt = np.ascontiguousarray(Y.transpose(0, 1, 3, 2))
    pairs = _some_pairs(Y[1:2], seed=N)
    eng = _stateless(1, N)
    try:
        for mode in MODES:
            want = partners_np(Y, mode, 512, pairs)
            assert want["totals"][1, 0, 3] >= 1 and want["totals"][2, 0, 3] == N - 2 and not want["hist"][..., -1].any()
            _assert_counts(eng.network_shared_partners(Y, mode=mode, n_bins=512, nodes=True, pairs=pairs), want, (N, mode), net=True)
            got = eng.network_shared_partners(Yt, mode=mode, n_bins=512, nodes=True, pairs=pairs if mode != "path" else transposed_ends(pairs))
            _assert_counts(got, want, (N, mode, "transposed"), net=True)
    finally:
        eng.close()


def test_closed_forms():
    """N = 300 through the network call: empty, complete, the path, the stars, one 3-cycle, one transitive triple, the book; a
    path of sevens and a diagonal of sevens count as ties and as nothing."""
    N = 300
    cases = closed_forms(N)
    cases["path of sevens"] = (7 * cases["path"][0], cases["path"][1])
    cases["complete with a diagonal of sevens"] = (np.full((N, N), 7, np.uint8), cases["complete"][1])
    Y = np.stack([y for y, _ in cases.values()])[:, None]
    eng = _stateless(1, N)
    try:
        for mode in MODES:
            got = eng.network_shared_partners(Y, mode=mode, n_bins=512, nodes=True)
            _assert_counts(got, partners_np(Y, mode, 512), mode)
            for q, (name, (_, want)) in enumerate(cases.items()):
                assert tuple(got["totals"][q, 0]) == want[mode], (name, mode)
            c = list(cases).index("complete")
            assert got["hist"][c, 0, N - 2] == want_ties(N, mode) and (got["node_supported"][c, 0] == (N - 1) * (2 if mode == "path" else 1)).all()
    finally:
        eng.close()


def want_ties(N, mode):
    return N * (N - 1) // (1 if mode == "path" else 2)


def test_one_hot_rho_draws_the_design():
    """A one-hot rho: every sample is the design whatever the seed, and the sampled call equals the network call."""
    N, S = 300, 3
    Y = np.stack([boundary_graph(N, 6.0, 1), boundary_graph(N, 40.0, 2), book(N)])
    pairs = _some_pairs(Y[None], seed=9)
    eng = _engine_with_rho(one_hot_rho(Y), 3)
    try:
        assert np.array_equal(eng.sample(40) > 0, Y > 0)
        for mode in MODES:
            net = eng.network_shared_partners(Y, mode=mode, n_bins=512, nodes=True, pairs=pairs)
            want = partners_np(Y[None], mode, 512, pairs)
            _assert_counts(net, _first(want), mode, net=True)
            for seed in (40, 41, 2 ** 63):
                got = eng.sample_shared_partners(seed, S, mode=mode, n_bins=512, nodes=True, pairs=pairs)
                for k in PER_SAMPLE:
                    for s in range(S):
                        assert np.array_equal(got[k][s], net[k]), (mode, seed, s, k)
                tie = net["pair_partners"] >= 0
                assert np.array_equal(got["pair_present"], S * tie) and np.array_equal(got["pair_supported"], S * (net["pair_partners"] > 0))
                assert np.array_equal(got["pair_partners"], S * np.where(tie, net["pair_partners"], 0).astype(np.int64))
    finally:
        eng.close()


def _bytes(res):
    return b"".join(np.ascontiguousarray(res[k]).tobytes() for k in sorted(res))


def test_medium_case_chunks_and_reruns(monkeypatch):
    """L = 2, N = 300, K = 3 on report lists, S = 12: one chunk against chunks of 5 samples (12 = 5 + 5 + 2) on a fresh handle and
    against a second run, byte for byte, the pair accumulators -- which live across the chunks -- included; the first samples
    against the definition."""
    X, st = _medium_case()
    seed, S = 1000, 12
    monkeypatch.setenv("VMR_FORMAT", "sparse")
    monkeypatch.delenv("VMR_NETSTATS_CHUNK", raising=False)
    eng = _engine_for(X, None, 3, True, st)
    try:
        Ys = np.asarray([eng.sample(seed + s) for s in range(S)])
        pairs = _some_pairs(Ys, seed=3)
        one = {m: eng.sample_shared_partners(seed, S, mode=m, nodes=True, pairs=pairs) for m in MODES}
        again = {m: eng.sample_shared_partners(seed, S, mode=m, nodes=True, pairs=pairs) for m in MODES}
    finally:
        eng.close()
    for m in MODES:
        assert _bytes(one[m]) == _bytes(again[m]), m
        _assert_counts(one[m], partners_np(Ys, m, 64, pairs), m, pair_sums=True)
        assert m == "mutual" or (one[m]["pair_present"].max() > 1 and one[m]["totals"][..., 0].all())
    monkeypatch.setenv("VMR_NETSTATS_CHUNK", "5")
    eng = _engine_for(X, None, 3, True, st)
    try:
        for m in MODES:
            many = eng.sample_shared_partners(seed, S, mode=m, nodes=True, pairs=pairs)
            assert _bytes(many) == _bytes(one[m]), m
            assert _bytes(eng.sample_shared_partners(seed, S, mode=m, nodes=True, pairs=pairs)) == _bytes(one[m]), m
    finally:
        eng.close()


def test_networks_across_chunk_boundaries(monkeypatch):
    """The upload loop on a handle with no state: L = 2, N = 65, seven random networks with diagonal entries, in one chunk and in
    chunks of 3 + 3 + 1 on a fresh handle (the switch is read once per handle): the same bytes, equal to the definition."""
    L, N, n = 2, 65, 7
    rng = np.random.RandomState(65)
    Y = (rng.random_sample((n, L, N, N)) < 6.0 / N).astype(np.uint8) * rng.randint(1, 4, (n, L, N, N)).astype(np.uint8)
    Y[:, :, np.arange(0, N, 3), np.arange(0, N, 3)] = 1
    Y[:, :, N - 1, 0], Y[:, :, 1, N - 1] = 1, 2
    pairs = _some_pairs(Y, seed=1)

    def run(mode):
        eng = _stateless(L, N)
        try:
            return eng.network_shared_partners(Y, mode=mode, n_bins=16, nodes=True, pairs=pairs)
        finally:
            eng.close()

    for mode in MODES:
        monkeypatch.delenv("VMR_NETSTATS_CHUNK", raising=False)
        one = run(mode)
        monkeypatch.setenv("VMR_NETSTATS_CHUNK", "3")
        many = run(mode)
        assert _bytes(one) == _bytes(many), mode
        _assert_counts(one, partners_np(Y, mode, 16, pairs), mode, net=True)


# ------------------------------------------------------------------------------------------ launch shapes
def _frozen(d):
    for v in d.values():
        v.flags.writeable = False
    return d


@functools.lru_cache(maxsize=None)
def _design_partners(N, mode):
    """`partners_np` of `design(N)` (layers 0 and 3 at N = 2048) with 512 bins, computed once."""
    Y = design(N)[[0, 3]] if N == 2048 else design(N)
    return _frozen(partners_np(Y[None], mode, 512))


def _reversed_want(want, n_bins):
    """The reference of a design as that of the design with its nodes reversed: the same histogram, the node arrays reversed."""
    return {"hist": fold(want["hist"], n_bins), "totals": want["totals"], "node_ties": want["node_ties"][..., ::-1],
            "node_supported": want["node_supported"][..., ::-1]}


@pytest.mark.parametrize("N", [513, 1024, 1025, 2048])
def test_launch_shapes(N, monkeypatch):
    """`design(N)`: 8 and 16 lanes per neighbour with a second trip of the word stride at 513 and 1025, row i in a register at
    1024 (four layers) and at 2048 (32 words; the sparse and the hub layer).  Two samples in two chunks with 512 bins -- the
    designs' largest count is 254 (the dense layer at 1024, union): the last bin is empty, the histogram unpooled -- and with 64,
    where the dense layer pools; then through the network call the design as it is (entries above 1, the diagonal), with its nodes
    reversed -- the hub as node 0 lists everybody, which as the last node it does not in union and mutual mode -- and transposed."""
    Y = design(N)[[0, 3]] if N == 2048 else design(N)
    Yr, Yt = reversed_nodes(Y), np.ascontiguousarray(Y.transpose(0, 2, 1))
    eng = _design_engine(Y, monkeypatch)
    try:
        for mode in MODES:
            want = _design_partners(N, mode)
            assert not want["hist"][..., -1].any() and want["totals"][..., 3].max() <= 254
            if N == 1024 and mode == "union":
                assert want["totals"][0, 2, 3] == 254
            two = {k: np.repeat(want[k], 2, axis=0) for k in PER_SAMPLE}
            _assert_counts(eng.sample_shared_partners(40, 2, mode=mode, n_bins=512, nodes=True), two, (N, mode))
            two["hist"] = fold(two["hist"], 64)
            assert N == 2048 or mode != "union" or two["hist"][0, 2, -1] > 0
            _assert_counts(eng.sample_shared_partners(40, 2, mode=mode, n_bins=64, nodes=True), two, (N, mode, "pooled"))
            net = eng.network_shared_partners(np.stack([Y, Yr, Yt]), mode=mode, n_bins=512, nodes=True)
            one = _first(want)
            _assert_counts(_first(net), one, (N, mode, "network"))
            _assert_counts(_first(net, 1), _reversed_want(one, 512), (N, mode, "reversed"))
            # union and mutual do not see a transposition; in path mode the ties of the transpose are the ties with their ends
            # swapped, each with the same partners: the same histogram, and a node is an end of the same ties
            _assert_counts(_first(net, 2), one, (N, mode, "transposed"))
    finally:
        eng.close()


@pytest.mark.parametrize("N", [2049, 4097])
def test_beyond_one_list_block(N, monkeypatch):
    """`design_large(N)` with its nodes reversed, one layer, one sample: the hub is node 0 and lists everybody -- at 2049 two list
    blocks, 33 words on 32 lanes; at 4097 three, 65 words on 64 lanes in two trips; the largest count is 19.  The design as it is
    through the network call, and the book, whose spine has N - 2 partners: 2047 and 4095 land in the last of 1024 bins, and the
    totals hold the maximum and the sum unpooled."""
    Y = design_large(N)
    R = reversed_nodes(Y)
    bk = book(N)[None]
    eng = _design_engine(R, monkeypatch)
    try:
        for mode in MODES:
            want = partners_np(Y[None], mode, MAX_BINS)
            assert mode != "union" or want["totals"][0, 0, 3] == 19
            rev = _reversed_want(_first(want), 64)
            _assert_counts(_first(eng.sample_shared_partners(40, 1, mode=mode, n_bins=64, nodes=True)), rev, (N, mode))
            net = eng.network_shared_partners(np.stack([Y, bk]), mode=mode, n_bins=MAX_BINS, nodes=True, pairs=[(0, N - 1, 0), (0, 0, N - 1), (0, 5, 0)])
            _assert_counts(_first(net), _first(want), (N, mode, "network"))
            wb = partners_np(bk[None], mode, MAX_BINS, [(0, N - 1, 0), (0, 0, N - 1), (0, 5, 0)])
            _assert_counts(_first(net, 1), {k: wb[k][0] for k in PER_SAMPLE}, (N, mode, "book"))
            assert net["pair_partners"][1].tolist() == [N - 2, N - 2, 1] == wb["pair_partners_net"][0].tolist()
            ties = (2 if mode == "path" else 1) * (2 * N - 3)
            assert net["totals"][1, 0].tolist() == [ties, ties, (2 if mode == "path" else 1) * 3 * (N - 2), N - 2]
            spine = 2 if mode == "path" else 1
            assert net["hist"][1, 0, min(N - 2, MAX_BINS - 1)] == spine and (N < 4097 or net["hist"][1, 0, -1] == spine)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------ pairs, arguments, the model
def test_pairs():
    """Both orders of a tie, a duplicate row (the two rows get equal results), an untied pair (0 present; -1 from the network
    call) and the last node, on the golden case A in every mode."""
    d = load_case("A_ones_mut")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        S, N = 8, eng.N
        Ys = np.asarray([eng.sample(21 + s) for s in range(S)])
        A = (Ys > 0) & ~np.eye(N, dtype=bool)
        At = A.transpose(0, 1, 3, 2)
        oneway = np.argwhere((A & ~At).any(axis=0))                                           # i -> j without j -> i in some sample
        never = np.argwhere(~(A | At).any(axis=0) & ~np.eye(N, dtype=bool)[None])            # untied in every sample
        last = np.argwhere(A[:, :, N - 1, :].any(axis=0))
        assert len(oneway) and len(never) and len(last)
        (l, i, j), (ln, un, vn), (ll, jl) = oneway[0], never[0], last[0]
        pairs = np.array([[l, i, j], [l, j, i], [l, i, j], [ln, un, vn], [ll, N - 1, jl], [ll, jl, N - 1]], np.int32)
        for mode in MODES:
            want = partners_np(Ys, mode, 64, pairs)
            got = eng.sample_shared_partners(21, S, mode=mode, pairs=pairs)
            _assert_counts(got, want, mode, pair_sums=True, nodes=False)
            net = eng.network_shared_partners(Ys, mode=mode, pairs=pairs)
            _assert_counts(net, want, mode, net=True, nodes=False)
            pres = got["pair_present"]
            assert pres[3] == 0 and (net["pair_partners"][:, 3] == -1).all()                   # the untied pair
            if mode == "path":                                                                 # the two orders are two ties
                assert not np.array_equal(net["pair_partners"][:, 0] >= 0, net["pair_partners"][:, 1] >= 0)
            else:                                                                              # .. and one tie
                assert pres[0] == pres[1] and np.array_equal(net["pair_partners"][:, 0], net["pair_partners"][:, 1])
                assert pres[4] == pres[5]
            assert mode == "mutual" or (pres[0] > 0 and pres[4] + pres[5] > 0)
            for k in PAIR_SUMS:
                assert got[k][0] == got[k][2], (mode, k)                                       # the duplicate row
            assert np.array_equal(net["pair_partners"][:, 0], net["pair_partners"][:, 2])
    finally:
        eng.close()


def test_argument_errors_on_a_live_handle():
    from vimure_amd import _lib
    from vimure_amd.engine import EngineError, PartnersArgumentError
    d = load_case("A_ones_mut")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, None)
    try:
        L, N = eng.L, eng.N
        B = 8
        hs, ts = np.full((2, L, B), 9, np.uint64), np.full((2, L, 4), 9, np.uint64)
        hn, tn, Y = np.full((1, L, B), 9, np.uint64), np.full((1, L, 4), 9, np.uint64), np.zeros((1, L, N, N), np.uint8)
        Y[0, :, 0, 1] = 1
        good = np.array([[0, 0, 1], [L - 1, N - 1, 0]], np.int32)
        acc = [np.zeros(2, np.uint32), np.zeros(2, np.uint32), np.zeros(2, np.uint64)]
        netp = np.zeros((1, 2), np.int32)

        def raw(S=2, n_trials=1, mode=0, n_bins=B, hist=hs.ctypes.data, totals=ts.ctypes.data, pairs=None, n_pairs=0, out=True):
            a = [x.ctypes.data if out else None for x in acc]
            return eng.lib.vmr_sample_shared_partners(eng._h, 1, S, n_trials, mode, n_bins, hist, totals, None, None, pairs, n_pairs, *a)

        def raw_net(Yp=Y.ctypes.data, n=1, mode=0, n_bins=B, hist=hn.ctypes.data, totals=tn.ctypes.data, pairs=None, n_pairs=0, out=True):
            return eng.lib.vmr_network_shared_partners(eng._h, Yp, n, mode, n_bins, hist, totals, None, None, pairs, n_pairs,
                                                       netp.ctypes.data if out else None)

        def bad_pair(row):
            p = np.array([[0, 0, 1], row], np.int32)
            return {"pairs": p.ctypes.data, "n_pairs": 2, "_keep": p}

        shared = [({"mode": -1}, b"mode"), ({"mode": 3}, b"mode"), ({"n_bins": 1}, b"n_bins"), ({"n_bins": 1025}, b"n_bins"), ({"hist": None}, b"hist is NULL"),
                  ({"totals": None}, b"totals is NULL"), ({"n_pairs": -1}, b"n_pairs"), ({"n_pairs": 2}, b"pairs is NULL"),
                  ({"pairs": good.ctypes.data, "n_pairs": 2, "out": False}, b"pair_"), (bad_pair([L, 0, 1]), b"pairs[1]"),
                  (bad_pair([-1, 0, 1]), b"pairs[1]"), (bad_pair([0, N, 1]), b"pairs[1]"), (bad_pair([0, 0, -1]), b"pairs[1]"),
                  (bad_pair([0, 3, 3]), b"pairs[1]")]
        bad = [(raw, kw, word) for kw, word in [({"S": 0}, b"n_samples"), ({"S": -3}, b"n_samples"), ({"n_trials": 0}, b"n_trials")] + shared]
        bad += [(raw_net, kw, word) for kw, word in [({"n": 0}, b"n must"), ({"Yp": None}, b"Y is NULL")] + shared]

        def refused():
            for fn, kw, word in bad:
                kw = {k: v for k, v in kw.items() if k != "_keep"}
                assert fn(**kw) == _lib.VMR_EINVAL, kw
                err = eng.lib.vmr_last_error(eng._h)
                assert word in err and (b"vmr_sample_shared_partners" if fn is raw else b"vmr_network_shared_partners") in err, (kw, err)

        # before vmr_set_state: the state is what is missing, unless an argument is refused first; the networks' call needs none
        with pytest.raises(EngineError, match="vmr_set_state") as ei:
            eng.sample_shared_partners(1, 2)
        assert not isinstance(ei.value, PartnersArgumentError)
        assert raw() == _lib.VMR_ESTATE and (hs == 9).all() and (ts == 9).all()
        assert raw_net(pairs=good.ctypes.data, n_pairs=2) == _lib.VMR_OK
        assert tn[0].tolist() == [[1, 0, 0, 0]] * L and hn[0, :, 0].tolist() == [1] * L and not hn[0, :, 1:].any() and netp.tolist() == [[0, -1]]
        refused()
        a3 = [x.ctypes.data for x in acc]
        assert eng.lib.vmr_sample_shared_partners(None, 1, 2, 1, 0, B, hs.ctypes.data, ts.ctypes.data, None, None, None, 0, *a3) == _lib.VMR_EINVAL
        assert eng.lib.vmr_network_shared_partners(None, Y.ctypes.data, 1, 0, B, hn.ctypes.data, tn.ctypes.data, None, None, None, 0, None) == _lib.VMR_EINVAL
        eng.set_state(*_golden_state(d))
        refused()
        for kw, word in (({"n_samples": 0}, "n_samples"), ({"n_trials": 0}, "n_trials"), ({"mode": "either"}, "mode"), ({"n_bins": 1}, "n_bins"),
                         ({"n_bins": 1025}, "n_bins"), ({"pairs": [[0, 2, 2]]}, "pairs"), ({"pairs": [[0, 1]]}, "shape"), ({"pairs": [[0, 0, N]]}, "pairs")):
            args = dict(seed=1, n_samples=2)
            args.update(kw)
            with pytest.raises(PartnersArgumentError, match=word):
                eng.sample_shared_partners(**args)
        with pytest.raises(PartnersArgumentError, match="shape"):
            eng.network_shared_partners(np.zeros((L, N, N + 1), np.uint8))
        with pytest.raises(PartnersArgumentError, match="n must"):
            eng.network_shared_partners(np.zeros((0, L, N, N), np.uint8))
        with pytest.raises(PartnersArgumentError, match="mode"):
            eng.network_shared_partners(Y, mode="cyclic")
        # the handle still works
        assert raw() == _lib.VMR_OK
        want = partners_np([eng.sample(1), eng.sample(2)], "union", B)
        assert np.array_equal(hs.astype(np.int64), want["hist"]) and np.array_equal(ts.astype(np.int64), want["totals"])
    finally:
        eng.close()


def test_fewer_than_three_nodes():
    """N = 2: a legal handle; a tie is counted and has no partner, whatever the mode."""
    Y = np.array([[[[1, 1], [1, 0]]], [[[0, 0], [3, 0]]], [[[5, 0], [0, 0]]]], np.uint8)
    eng = _stateless(1, 2)
    try:
        for mode in MODES:
            got = eng.network_shared_partners(Y, mode=mode, n_bins=2, nodes=True, pairs=[(0, 0, 1), (0, 1, 0)])
            _assert_counts(got, partners_np(Y, mode, 2, [(0, 0, 1), (0, 1, 0)]), mode, net=True)
            assert not got["totals"][..., 1:].any() and not got["hist"][..., 1:].any() and not got["node_supported"].any()
            assert got["pair_partners"].max() == 0 and got["totals"][:, 0, 0].tolist() == {"union": [1, 1, 0], "mutual": [1, 0, 0], "path": [2, 1, 0]}[mode]
    finally:
        eng.close()


def test_model_posterior_shared_partners():
    from vimure_amd import VimureModel
    from vimure_amd.synthetic import standard_sbm
    net = standard_sbm(N=60, M=8, L=1, K=2, avg_degree=6.0, eta=0.4, seed=4)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = VimureModel(mutuality=True)
        m.fit(net.X, K=2, seed=1, max_iter=30, num_realisations=1, keep_engine=True)
    try:
        S, sd = 8, 321
        Ys = None
        for mode in MODES:
            res = m.posterior_shared_partners(mode=mode, n_samples=S, seed=sd, nodes=True)
            assert m._rho_f is None                                           # rho has not crossed PCIe
            if Ys is None:
                Ys = np.asarray([m.sample_inferred_model(N=1, seed=sd + s, device=True)[0] for s in range(S)])
            point = np.asarray(m.get_inferred_model())
            A = (point > 0) & ~np.eye(m.N, dtype=bool)
            At = A.transpose(0, 2, 1)
            T = A if mode == "path" else np.triu(A & At if mode == "mutual" else A | At, 1)
            pairs = np.argwhere(T)
            assert np.array_equal(res.pairs, pairs) and (mode == "mutual" or len(pairs))
            want = partners_np(Ys, mode, 64, pairs)
            assert mode == "mutual" or want["totals"][..., 2].any()
            for k in PER_SAMPLE:
                assert np.array_equal(getattr(res, k), want[k]), (mode, k)
            for k in PAIR_SUMS:
                assert np.array_equal(getattr(res, k), want[k]), (mode, k)
            inf = partners_np(point[None], mode, 64, pairs)
            for k in PER_SAMPLE:
                assert np.array_equal(res.inferred[k], inf[k][0]), (mode, k)
            assert np.array_equal(res.inferred_partners, inf["pair_partners_net"][0]) and (res.inferred_partners >= 0).all()
            assert (res.S, res.L, res.N, res.seed, res.n_trials, res.mode) == (S, m.L, m.N, sd, 1, mode)
            assert res.support().shape == (S, m.L) and res.node_support().shape == (m.L, m.N)
            assert len(res.frame()) == m.L * 64 and "inferred" in res.frame().columns and len(res.summary()) == 7 * m.L
            tf = res.ties_frame()
            assert len(tf) == len(pairs) and list(tf.columns) == ["layer", "i", "j", "p_present", "p_supported", "mean_partners", "inferred_partners"]
            assert len(res.bridges(0.5)) <= len(tf)
        none = m.posterior_shared_partners(n_samples=2, seed=sd, n_trials=3, ties=None)
        want = partners_np([m.sample_inferred_model(N=3, seed=sd + s, device=True)[0] for s in range(2)], "union", 64)
        assert none.pairs is None and np.array_equal(none.hist, want["hist"]) and np.array_equal(none.totals, want["totals"])
        some = m.posterior_shared_partners(n_samples=2, seed=sd, ties=[[0, 1, 2], [0, 59, 0]])
        assert len(some.ties_frame()) == 2
    finally:
        m.close()
