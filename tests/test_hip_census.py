"""GPU: the triad census of posterior samples and of given networks on the device (vmr_sample_triad_census,
vmr_network_triad_census), held to the restatements of tests/census_util.py on the samples `CaviEngine.sample` returns for the same
seeds.  The census is exact integer arithmetic: every comparison is `==`.  Golden cases in both data layouts, the general kernels
(K = 12), a coordinate-list handle; every word boundary; closed forms; a one-hot rho; several chunks and two runs; every class of
the kernel's launch shape (tests/census_util.SHAPE_NS names what each N is for); the argument errors; the model's method."""
import functools
import warnings
from math import comb

import numpy as np
import pytest

from tests.census_util import (CLASS_NAMES, boundary_graph, census_fast, census_np, class_ladder, complete, empty, ladder_census, path,
                               reversed_nodes, star, three_cycle)
from tests.golden_util import case_config, load_case
from tests.graph_shapes_util import design, design_large, one_hot_rho
from tests.test_hip_betweenness import _stateless
from tests.test_hip_centrality import _coo_engine_with_rho, _engine_with_rho, _medium_case
from tests.test_hip_netstats import _engine_for, _golden_state

pytestmark = pytest.mark.gpu

SWAP_DU = [0, 1, 2, 4, 3, 5, 7, 6, 8, 9, 10, 12, 11, 13, 14, 15]      # the census of the transposed network: D and U change places


def _assert_census(got, want, what=""):
    assert got.dtype == np.int64 and got.shape == want.shape, what
    assert np.array_equal(got, want), (what, (got - want).tolist())


def _check(eng, seed, S, trials=(1,)):
    """`sample_triad_census` against `census_np` of the samples of the same seeds, and `network_triad_census` of those samples."""
    for n_trials in trials:
        Ys = np.asarray([eng.sample(seed + s, n_trials) for s in range(S)])
        want = census_np(Ys)
        assert (want.sum(axis=-1) == comb(eng.N, 3)).all()
        got = eng.sample_triad_census(seed, S, n_trials=n_trials)
        _assert_census(got, want, "n_trials %d" % n_trials)
        _assert_census(eng.network_triad_census(Ys), want, "networks, n_trials %d" % n_trials)
        _assert_census(eng.network_triad_census(Ys[0]), want[0], "one network")
    return want


@pytest.mark.parametrize("case", ["A_ones_mut", "B_random_mask_K3", "D_self_mask", "E_undirected"])
def test_golden_cases(case, vmr_format):
    d = load_case(case)
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        assert eng.data_format()[0] == vmr_format
        _check(eng, 11, 8, trials=(1, 3))
        if case == "E_undirected":
            # The engine draws every ordered pair on its own: a sample of the undirected case is not symmetric (asserted), and
            # its census holds asymmetric classes.  Symmetrised, every tie is mutual: 003, 102, 201 and 300 only.
            Ys = np.asarray([eng.sample(11 + s) for s in range(8)])
            assert (Ys != Ys.transpose(0, 1, 3, 2)).any()
            got = eng.network_triad_census(np.maximum(Ys, Ys.transpose(0, 1, 3, 2)))
            _assert_census(got, census_np(np.maximum(Ys, Ys.transpose(0, 1, 3, 2))), "symmetrised")
            sym = [CLASS_NAMES.index(k) for k in ("003", "102", "201", "300")]
            assert not np.delete(got, sym, axis=-1).any() and got[..., sym[1:]].all()
    finally:
        eng.close()


def test_general_kernels():
    d = load_case("L_default_K12")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    assert K > 8
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        _check(eng, 5, 8)
    finally:
        eng.close()


def test_coo_handle():
    d = load_case("D_self_mask")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d), coo=True)
    try:
        _check(eng, 3, 8)
    finally:
        eng.close()


@pytest.mark.parametrize("N", [63, 64, 65, 129, 257])
def test_word_boundaries(N):
    """W = 1, 1, 2, 3 and 5 words per bit row on 1, 1, 2, 2 and 4 lanes, on a handle with no state: random digraphs with 2 and with
    N / 4 ties per node, a drawn diagonal, entries up to 3, node N - 1 tied both ways; the class ladder; all of them transposed."""
    sparse, dense, ladder = boundary_graph(N, 2.0, N), boundary_graph(N, N / 4.0, 2 * N), class_ladder(N)
    assert sparse.diagonal().any() and dense.diagonal().any() and sparse.max() == 3
    Y = np.stack([sparse, dense, ladder, sparse.T, dense.T, ladder.T])[:, None]
    want = census_np(Y[:3]) if N <= 129 else census_fast(Y[:3])
    assert np.array_equal(want[2, 0], ladder_census(N)) and want[1, 0].all()
    eng = _stateless(1, N)
    try:
        got = eng.network_triad_census(Y)
        _assert_census(got[:3], want, N)
        _assert_census(got[3:], want[..., SWAP_DU], (N, "transposed"))
    finally:
        eng.close()


def test_closed_forms():
    """N = 300 through the network call: empty, complete, the path, the out-, in- and mutual star, one 3-cycle, the full class
    ladder (N = 420 has room for it: on its own handle), and entries of 7 counted as ties."""
    N = 300
    cases = {"empty": empty(N), "complete": complete(N), "path": path(N), "out-star": star(N, "out"), "in-star": star(N, "in", N - 1),
             "mutual star": star(N, "mutual", N // 2), "3-cycle": three_cycle(N)}
    cases["path of sevens"] = (7 * path(N)[0], path(N)[1])
    cases["complete with a diagonal of sevens"] = (np.full((N, N), 7, np.uint8), complete(N)[1])
    eng = _stateless(1, N)
    try:
        got = eng.network_triad_census(np.stack([Y for Y, _ in cases.values()])[:, None])
        for q, (name, (_, want)) in enumerate(cases.items()):
            assert want.sum() == comb(N, 3)
            _assert_census(got[q, 0], want, name)
    finally:
        eng.close()
    eng = _stateless(1, 420)
    try:
        want = ladder_census(420)
        assert np.array_equal(want[3:], np.arange(4, 17))
        _assert_census(eng.network_triad_census(class_ladder(420)[None]), want[None], "ladder")
    finally:
        eng.close()


def test_one_hot_rho_draws_the_design():
    """A one-hot rho: every sample is the design whatever the seed, and the sampled call equals the network call."""
    N, S = 300, 3
    Y = np.stack([boundary_graph(N, 6.0, 1), path(N)[0], star(N, "out", 77)[0]])
    eng = _engine_with_rho(one_hot_rho(Y), 3)
    try:
        assert np.array_equal(eng.sample(40) > 0, Y > 0)
        net = eng.network_triad_census(Y)
        _assert_census(net, census_fast(Y[None])[0])
        assert np.array_equal(net[1], path(N)[1]) and np.array_equal(net[2], star(N, "out")[1])
        for seed in (40, 41, 2 ** 63):
            got = eng.sample_triad_census(seed, S)
            for s in range(S):
                _assert_census(got[s], net, (seed, s))
    finally:
        eng.close()


def test_medium_case_chunks_and_reruns(monkeypatch):
    """L = 2, N = 300, K = 3 on report lists, S = 12: one chunk against chunks of 5 samples (12 = 5 + 5 + 2) on a fresh handle and
    against a second run, byte for byte; the first samples against the restatement."""
    X, st = _medium_case()
    seed, S = 1000, 12
    monkeypatch.setenv("VMR_FORMAT", "sparse")
    monkeypatch.delenv("VMR_NETSTATS_CHUNK", raising=False)
    eng = _engine_for(X, None, 3, True, st)
    try:
        one = eng.sample_triad_census(seed, S)
        again = eng.sample_triad_census(seed, S)
        Ys = np.asarray([eng.sample(seed + s) for s in range(2)])
    finally:
        eng.close()
    assert one.shape == (S, 2, 16) and one.tobytes() == again.tobytes()
    _assert_census(one[:2], census_fast(Ys))
    assert (one.sum(axis=-1) == comb(300, 3)).all() and (one[..., 3:].sum(axis=-1) > 0).all()
    monkeypatch.setenv("VMR_NETSTATS_CHUNK", "5")
    eng = _engine_for(X, None, 3, True, st)
    try:
        many = eng.sample_triad_census(seed, S)
        again = eng.sample_triad_census(seed, S)
    finally:
        eng.close()
    assert many.tobytes() == one.tobytes() and again.tobytes() == one.tobytes()


def test_networks_across_chunk_boundaries(monkeypatch):
    """The upload loop on a handle with no state: L = 2, N = 65, seven random networks with diagonal entries, in one chunk and in
    chunks of 3 + 3 + 1 on a fresh handle (the switch is read once per handle): the same bytes, equal to the restatement."""
    L, N, n = 2, 65, 7
    rng = np.random.RandomState(65)
    Y = (rng.random_sample((n, L, N, N)) < 3.0 / N).astype(np.uint8) * rng.randint(1, 4, (n, L, N, N)).astype(np.uint8)
    Y[:, :, np.arange(0, N, 3), np.arange(0, N, 3)] = 1
    Y[:, :, N - 1, 0], Y[:, :, 1, N - 1] = 1, 2

    def run():
        eng = _stateless(L, N)
        try:
            return eng.network_triad_census(Y)
        finally:
            eng.close()

    monkeypatch.delenv("VMR_NETSTATS_CHUNK", raising=False)
    one = run()
    monkeypatch.setenv("VMR_NETSTATS_CHUNK", "3")
    many = run()
    assert one.tobytes() == many.tobytes()
    _assert_census(one, census_np(Y))


# ------------------------------------------------------------------------------------------ launch shapes
@functools.lru_cache(maxsize=None)
def _design_census(N):
    """The census of `design(N)` (layers 0 and 3 at N = 2048) by `census_fast`, computed once."""
    Y = design(N)[[0, 3]] if N == 2048 else design(N)
    c = census_fast(Y[None])[0]
    c.flags.writeable = False
    return c


def _design_engine(Y, monkeypatch):
    """A coordinate-list handle whose every sample is (Y > 0), with one sample to a chunk."""
    monkeypatch.setenv("VMR_NETSTATS_CHUNK", "1")
    eng = _coo_engine_with_rho(one_hot_rho(Y))
    try:
        assert np.array_equal(eng.sample(40) > 0, Y > 0)
    except BaseException:
        eng.close()
        raise
    return eng


@pytest.mark.parametrize("N", [513, 1024, 1025, 2048])
def test_launch_shapes(N, monkeypatch):
    """`design(N)`: 8 and 16 lanes per neighbour with a second trip of the word stride at 513 and 1025, row i in registers at
    1024 (four layers) and at 2048 (32 words; the sparse and the hub layer).  Two samples in two chunks; then through the network
    call the design as it is (entries above 1, the diagonal), with its nodes reversed -- the hub as node 0 lists everybody, which
    as the last node it does not: a relabelling, the same census -- and transposed: D and U change places."""
    Y = design(N)[[0, 3]] if N == 2048 else design(N)
    want = _design_census(N)
    eng = _design_engine(Y, monkeypatch)
    try:
        got = eng.sample_triad_census(40, 2)
        _assert_census(got, np.stack([want, want]), N)
        net = eng.network_triad_census(np.stack([Y, reversed_nodes(Y), Y.transpose(0, 2, 1)]))
        _assert_census(net, np.stack([want, want, want[:, SWAP_DU]]), (N, "networks"))
    finally:
        eng.close()


@pytest.mark.parametrize("N", [2049, 4097])
def test_beyond_one_list_block(N, monkeypatch):
    """`design_large(N)` with its nodes reversed, one layer, one sample: the hub is node 0 and lists everybody -- at 2049 two
    list blocks (2047 entries and one), 33 words on 32 lanes; at 4097 three (2047, exactly CEN_LIST = 2048, and one), 65 words on 64
    lanes in two trips, and totals beyond 2^32.  The design as it is through the network call."""
    Y = design_large(N)
    want = census_fast(Y[None])[0]
    assert want.sum() == comb(N, 3) and (N < 4097 or want[0, 0] > 2 ** 32)
    R = reversed_nodes(Y)
    eng = _design_engine(R, monkeypatch)
    try:
        _assert_census(eng.sample_triad_census(40, 1), want[None], N)
        _assert_census(eng.network_triad_census(Y), want, (N, "network"))
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------ arguments, the model
def test_argument_errors_on_a_live_handle():
    from vimure_amd import _lib
    from vimure_amd.engine import CensusArgumentError, EngineError
    d = load_case("A_ones_mut")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, None)
    try:
        L, N = eng.L, eng.N
        cs, cn, Y = np.full((2, L, 16), 9, np.uint64), np.full((1, L, 16), 9, np.uint64), np.zeros((1, L, N, N), np.uint8)

        def raw(S=2, n_trials=1, out=cs.ctypes.data):
            return eng.lib.vmr_sample_triad_census(eng._h, 1, S, n_trials, out)

        def raw_net(Yp=Y.ctypes.data, n=1, out=cn.ctypes.data):
            return eng.lib.vmr_network_triad_census(eng._h, Yp, n, out)

        bad = ((raw, {"S": 0}, b"n_samples"), (raw, {"S": -3}, b"n_samples"), (raw, {"n_trials": 0}, b"n_trials"), (raw, {"out": None}, b"counts is NULL"),
               (raw_net, {"n": 0}, b"n must"), (raw_net, {"Yp": None}, b"Y is NULL"), (raw_net, {"out": None}, b"counts is NULL"))
        # before vmr_set_state: the state is what is missing, unless an argument is refused first; the networks' call needs none
        with pytest.raises(EngineError, match="vmr_set_state") as ei:
            eng.sample_triad_census(1, 2)
        assert not isinstance(ei.value, CensusArgumentError)
        assert raw() == _lib.VMR_ESTATE and (cs == 9).all()
        assert raw_net() == _lib.VMR_OK and cn[0, :, 0].tolist() == [comb(N, 3)] * L and not cn[0, :, 1:].any()
        for fn, kw, word in bad:
            assert fn(**kw) == _lib.VMR_EINVAL, kw
            err = eng.lib.vmr_last_error(eng._h)
            assert word in err and (b"vmr_sample_triad_census" if fn is raw else b"vmr_network_triad_census") in err, (kw, err)
        assert eng.lib.vmr_sample_triad_census(None, 1, 2, 1, cs.ctypes.data) == _lib.VMR_EINVAL
        assert eng.lib.vmr_network_triad_census(None, Y.ctypes.data, 1, cn.ctypes.data) == _lib.VMR_EINVAL
        eng.set_state(*_golden_state(d))
        for fn, kw, word in bad:
            assert fn(**kw) == _lib.VMR_EINVAL and word in eng.lib.vmr_last_error(eng._h), (kw, word)
        for kw, word in (({"n_samples": 0}, "n_samples"), ({"n_trials": 0}, "n_trials")):
            args = dict(seed=1, n_samples=2)
            args.update(kw)
            with pytest.raises(CensusArgumentError, match=word):
                eng.sample_triad_census(**args)
        with pytest.raises(CensusArgumentError, match="shape"):
            eng.network_triad_census(np.zeros((L, N, N + 1), np.uint8))
        with pytest.raises(CensusArgumentError, match="n must"):
            eng.network_triad_census(np.zeros((0, L, N, N), np.uint8))
        # the handle still works
        assert raw() == _lib.VMR_OK
        _assert_census(cs.astype(np.int64), census_np([eng.sample(1), eng.sample(2)]))
    finally:
        eng.close()


def test_fewer_than_three_nodes():
    """N = 2: a legal handle, no triple: all zeros from both calls, whatever the ties."""
    eng = _stateless(1, 2)
    try:
        got = eng.network_triad_census(np.array([[[[1, 1], [1, 0]]], [[[0, 0], [3, 0]]]], np.uint8))
        assert got.shape == (2, 1, 16) and not got.any()
    finally:
        eng.close()


def test_model_posterior_triad_census():
    from vimure_amd import VimureModel
    from vimure_amd.synthetic import standard_sbm
    net = standard_sbm(N=60, M=8, L=1, K=2, avg_degree=6.0, eta=0.4, seed=4)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = VimureModel(mutuality=True)
        m.fit(net.X, K=2, seed=1, max_iter=30, num_realisations=1, keep_engine=True)
    try:
        S, sd = 8, 321
        res = m.posterior_triad_census(n_samples=S, seed=sd)
        assert m._rho_f is None                                           # rho has not crossed PCIe
        Ys = np.asarray([m.sample_inferred_model(N=1, seed=sd + s, device=True)[0] for s in range(S)])
        want = census_np(Ys)
        assert want[..., 3:].any()
        _assert_census(res.counts, want)
        _assert_census(res.inferred, census_np([m.get_inferred_model()])[0])
        assert (res.S, res.L, res.N, res.seed, res.n_trials) == (S, m.L, m.N, sd, 1)
        assert res.mean.shape == (m.L, 16) and res.expected_under_man().shape == (S, m.L, 16)
        assert res.transitive_share().shape == (S, m.L) and set(res.dyads()) == {"mutual", "asymmetric", "null"}
        assert len(res.frame()) == m.L * 16 and "inferred" in res.frame().columns and len(res.summary()) == 20 * m.L
        _assert_census(m.posterior_triad_census(n_samples=2, seed=sd, n_trials=3).counts,
                       census_np([m.sample_inferred_model(N=3, seed=sd + s, device=True)[0] for s in range(2)]))
    finally:
        m.close()
