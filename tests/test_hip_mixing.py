"""GPU: mixing by node attribute and overlap between layers of posterior samples, and their expectations, on the device
(vmr_sample_mixing, vmr_expected_mixing).  Every count is held, integer for integer, to the NumPy restatement
(tests/mixing_util.py) of the samples `CaviEngine.sample` returns for the same seeds: both data layouts, the general kernels
(K = 12, 16), a coordinate-list handle, every tile boundary, 1 to 64 groups, 1 to 3 layers, several chunks; the expectations to
NumPy on the rho read back and to `expected_stats`; sampling to its expectation; the model's method to `sample_inferred_model`."""
import warnings

import numpy as np
import pytest

from tests.golden_util import case_config, load_case
from tests.mixing_util import (MIX_KEYS, SAMPLING_CASE, check_sampling_against_expectation, expected_mixing_np, mixing_np,
                               sampling_case_inputs)
from tests.test_hip_netstats import _engine_for, _golden_state, _random_state

pytestmark = pytest.mark.gpu


def _assert_equal_tables(got, want, keys=MIX_KEYS):
    assert sorted(got) == sorted(keys)
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), k


def _mod_groups(N, C, leave_out_first=True):
    g = (np.arange(N) % C).astype(np.int32)
    if leave_out_first:
        g[0] = -1
    return g


def _check_exact(eng, seed, S, groups, C, trials=(1, 3), skips=(True,)):
    """`sample_mixing` against NumPy on the samples of the same seeds; returns the last reference."""
    want = None
    for n_trials in trials:
        Ys = [eng.sample(seed + s, n_trials) for s in range(S)]
        for skip in skips:
            want = mixing_np(Ys, groups, C, skip)
            _assert_equal_tables(eng.sample_mixing(seed, S, groups=groups, C=C, n_trials=n_trials, skip_diagonal=skip), want)
    return want


@pytest.mark.parametrize("case", ["A_ones_mut", "B_random_mask_K3", "D_self_mask", "E_undirected"])
def test_counts_equal_numpy_on_the_samples(case, vmr_format):
    d = load_case(case)
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        assert eng.data_format()[0] == vmr_format
        want = _check_exact(eng, 11, 8, _mod_groups(eng.N, 3), 3)
        assert want["mix"].sum() > 0
    finally:
        eng.close()


@pytest.mark.parametrize("case", ["L_default_K12", "M_K16_nomut"])
def test_counts_equal_numpy_general_kernels(case):
    d = load_case(case)
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    assert K > 8
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        _check_exact(eng, 5, 8, _mod_groups(eng.N, 3), 3)
    finally:
        eng.close()


def test_counts_equal_numpy_coo_handle():
    d = load_case("D_self_mask")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d), coo=True)
    try:
        _check_exact(eng, 3, 8, _mod_groups(eng.N, 3), 3)
    finally:
        eng.close()


def _random_engine(N, seed, L=2, M=4, K=3):
    g = np.random.RandomState(seed)
    X = (g.rand(L, N, N, M) < 0.1).astype(np.uint8)
    return _engine_for(X, None, K, True, _random_state(g, L, N, M, K, sparse_p=True))


@pytest.mark.parametrize("N", [5, 63, 64, 65, 129])
def test_tile_and_word_boundaries(N):
    """L = 2, K = 3 and 1, 1, 1, 2, 3 strips of 64 rows; C = 1 (one bin takes every edge), 2, 7 and 64 groups -- at N = 129 groups
    of 2 or 3 nodes and one round of the walk per layer, at N = 5 mostly empty groups -- with and without the diagonal."""
    eng = _random_engine(N, 100 + N)
    try:
        S, seed = 4, 7
        Ys = np.asarray([eng.sample(seed + s) for s in range(S)])
        assert all(Ys[:, l, np.arange(N), np.arange(N)].any() for l in range(2))   # leaving the diagonal out is exercised
        for C in (1, 2, 7, 64):
            groups = _mod_groups(N, C)
            for skip in (True, False):
                want = mixing_np(Ys, groups, C, skip)
                assert want["mix"].sum() > 0 and want["mutual"].sum() > 0 and want["overlap"][:, 0, 1].sum() > 0   # not a comparison of zeros
                _assert_equal_tables(eng.sample_mixing(seed, S, groups=groups, C=C, skip_diagonal=skip), want)
            kept, left = mixing_np(Ys, groups, C, False), mixing_np(Ys, groups, C, True)
            assert kept["mix"].sum() > left["mix"].sum() or N == 5
    finally:
        eng.close()


def _correlated_engine(L, N=70, M=4, K=3, seed=77):
    """Layers whose rho share a common part: their samples overlap."""
    g = np.random.RandomState(seed)
    X = (g.rand(L, N, N, M) < 0.1).astype(np.uint8)
    st = list(_random_state(g, L, N, M, K, sparse_p=True))
    rho = st[-1]
    strong = g.rand(N, N) < 0.15
    rho[:, strong, 0] *= 0.02
    st[-1] = rho / rho.sum(-1, keepdims=True)
    return _engine_for(X, None, K, True, tuple(st))


@pytest.mark.parametrize("L", [1, 3])
def test_layers_overlap_only_and_mix_only(L):
    eng = _correlated_engine(L)
    try:
        S, seed, C = 6, 31, 4
        N = eng.N
        groups = _mod_groups(N, C)
        Ys = [eng.sample(seed + s) for s in range(S)]
        want = mixing_np(Ys, groups, C, True)
        _assert_equal_tables(eng.sample_mixing(seed, S, groups=groups, C=C), want)
        edges = np.asarray([[(Ys[s][l] > 0).sum() - (np.diag(Ys[s][l]) > 0).sum() for l in range(L)] for s in range(S)])
        assert np.array_equal(np.diagonal(want["overlap"], axis1=1, axis2=2), edges)
        if L > 1:
            off = want["overlap"][:, ~np.eye(L, dtype=bool)]
            assert (off > 0).all() and (off > 0.2 * edges.min()).all()      # correlated layers: a real overlap
        # the overlap alone: group NULL, C = 0
        _assert_equal_tables(eng.sample_mixing(seed, S), want, keys=("overlap",))
        ov = np.zeros((S, L, L), np.uint64)
        assert eng.lib.vmr_sample_mixing(eng._h, seed, S, 1, None, 0, 1, None, None, ov.ctypes.data) == 0
        assert np.array_equal(ov.astype(np.int64), want["overlap"])
        # the groups alone, and mix alone (no transposed tile is staged then)
        _assert_equal_tables(eng.sample_mixing(seed, S, groups=groups, C=C, overlap=False), want, keys=("mix", "mutual"))
        mix = np.zeros((S, L, C, C), np.uint64)
        assert eng.lib.vmr_sample_mixing(eng._h, seed, S, 1, groups.ctypes.data, C, 1, mix.ctypes.data, None, None) == 0
        assert np.array_equal(mix.astype(np.int64), want["mix"])
        mut = np.zeros((S, L, C, C), np.uint64)
        assert eng.lib.vmr_sample_mixing(eng._h, seed, S, 1, groups.ctypes.data, C, 1, None, mut.ctypes.data, None) == 0
        assert np.array_equal(mut.astype(np.int64), want["mutual"])
    finally:
        eng.close()


def test_medium_case_several_chunks(monkeypatch):
    """L = 2, N = 300, K = 3 on report lists (a non-trivial perm), five strips (the last one partial), S = 16: one chunk against
    chunks of 5 samples (16 = 5 + 5 + 5 + 1), both against NumPy; `sample_stats` of the same engine is what it was before."""
    from tests.test_hip_netstats import _medium
    g = np.random.RandomState(21)
    X, st = _medium(g)
    seed, S, C = 1000, 16, 5
    groups = _mod_groups(300, C)
    monkeypatch.setenv("VMR_FORMAT", "sparse")
    monkeypatch.delenv("VMR_NETSTATS_CHUNK", raising=False)
    eng = _engine_for(X, None, 3, True, st)
    try:
        assert eng.data_format()[0] == "sparse"
        before = eng.sample_stats(seed, S, degrees=True)
        one = eng.sample_mixing(seed, S, groups=groups, C=C)
        after = eng.sample_stats(seed, S, degrees=True)
        want = mixing_np([eng.sample(seed + s) for s in range(S)], groups, C, True)
    finally:
        eng.close()
    _assert_equal_tables(one, want)
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    monkeypatch.setenv("VMR_NETSTATS_CHUNK", "5")
    eng = _engine_for(X, None, 3, True, st)
    try:
        many = eng.sample_mixing(seed, S, groups=groups, C=C)
    finally:
        eng.close()
    _assert_equal_tables(many, one)


def test_invariants_against_sample_stats():
    eng = _random_engine(129, 229)
    try:
        S, seed, C = 8, 55, 7
        groups = _mod_groups(129, C, leave_out_first=False)
        got = eng.sample_mixing(seed, S, groups=groups, C=C, skip_diagonal=False)
        st = eng.sample_stats(seed, S)
        assert st["mutual"].min() > 0
        assert np.array_equal(got["mix"].sum(axis=(2, 3)), st["edges"])
        assert np.array_equal(got["mutual"].sum(axis=(2, 3)), st["mutual"])
        assert np.array_equal(np.diagonal(got["overlap"], axis1=1, axis2=2), st["edges"])
        assert np.array_equal(got["mutual"], got["mutual"].transpose(0, 1, 3, 2))
        assert np.array_equal(got["overlap"], got["overlap"].transpose(0, 2, 1))
    finally:
        eng.close()


def _check_expected(eng, N, C=3):
    groups = _mod_groups(N, C)
    rho = eng.get_state()["rho"]
    # every term of every sum is non-negative: any summation order of n terms is within (n + 2) 2^-53 relative (the + 2: the
    # product inside a term); one such bound for the device and one for NumPy
    rtol = 2 * (N * N + 2) * 2.0 ** -53
    n = np.bincount(groups[groups >= 0], minlength=C)
    for skip in (True, False):
        pairs = np.outer(n, n) - (np.diag(n) if skip else 0)
        got, again = eng.expected_mixing(groups=groups, C=C, skip_diagonal=skip), eng.expected_mixing(groups=groups, C=C, skip_diagonal=skip)
        want = expected_mixing_np(rho, groups, C, skip)
        for k in MIX_KEYS:
            assert got[k].shape == want[k].shape and got[k].dtype == np.float64, k
            assert np.array_equal(got[k].view(np.uint64), again[k].view(np.uint64)), k
            pos = want[k] > 0
            assert np.array_equal(pos, np.broadcast_to(pairs > 0 if k != "overlap" else True, pos.shape)), k   # the bins that hold a tie
            print(k, skip, np.max(np.abs(got[k][pos] - want[k][pos]) / want[k][pos]), rtol)
            np.testing.assert_allclose(got[k][pos], want[k][pos], rtol=rtol, atol=0, err_msg=k)
            assert (got[k][~pos] == 0.0).all(), k                                   # empty bins are exact zeros
        assert np.array_equal(got["overlap"], got["overlap"].T)
    # all nodes labelled, the diagonal kept: the totals are those of expected_stats
    allg = _mod_groups(N, C, leave_out_first=False)
    got, st = eng.expected_mixing(groups=allg, C=C, skip_diagonal=False), eng.expected_stats()
    np.testing.assert_allclose(got["mix"].sum(axis=(1, 2)), st["edges"], rtol=rtol, atol=0)
    np.testing.assert_allclose(got["mutual"].sum(axis=(1, 2)), st["mutual"], rtol=rtol, atol=0)
    np.testing.assert_allclose(np.diagonal(got["overlap"]), st["edges"], rtol=rtol, atol=0)
    # an empty group is an exact zero, and so is everything about a node that is left out
    wide = eng.expected_mixing(groups=allg, C=C + 2, skip_diagonal=False)
    assert (wide["mix"][:, C:, :] == 0.0).all() and (wide["mutual"][:, :, C:] == 0.0).all()
    assert np.array_equal(wide["mix"][:, :C, :C].view(np.uint64), got["mix"].view(np.uint64))
    only = eng.expected_mixing(skip_diagonal=False)
    assert sorted(only) == ["overlap"] and np.array_equal(only["overlap"].view(np.uint64), got["overlap"].view(np.uint64))


@pytest.mark.parametrize("N", [5, 65, 129])
def test_expected_mixing_against_numpy(N):
    eng = _random_engine(N, 200 + N)
    try:
        _check_expected(eng, N)
    finally:
        eng.close()


def test_expected_mixing_on_golden_state():
    d = load_case("B_random_mask_K3")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, _golden_state(d))
    try:
        _check_expected(eng, d["X"].shape[1])
    finally:
        eng.close()


def test_sampling_agrees_with_expectation():
    """N = 129, C = 3, S = 256: for every bin whose expectation is at least 20 the mean over the samples lies within 5 standard
    errors of the expectation, the standard error that of the NumPy counts of the same samples
    (tests/test_mixing_host.py::test_sampling_case_holds_on_the_host_reference holds the same seeds to it without a GPU)."""
    c = SAMPLING_CASE
    X, st, groups = sampling_case_inputs()
    eng = _engine_for(X, None, c["K"], True, st)
    try:
        got = eng.sample_mixing(c["seed"], c["S"], groups=groups, C=c["C"])
        exp = eng.expected_mixing(groups=groups, C=c["C"])
        ref = mixing_np([eng.sample(c["seed"] + s) for s in range(c["S"])], groups, c["C"], True)
    finally:
        eng.close()
    assert check_sampling_against_expectation(got, exp, ref) == 2 * c["L"] * c["C"] ** 2 + c["L"] ** 2


def test_argument_errors_on_a_live_handle():
    from vimure_amd import _lib
    from vimure_amd.engine import EngineError, MixingArgumentError
    d = load_case("A_ones_mut")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    eng = _engine_for(d["X"], d["R"], K, mut, None)
    try:
        N, L, C = eng.N, eng.L, 3
        groups = _mod_groups(N, C)
        with pytest.raises(EngineError, match="vmr_set_state") as ei:
            eng.sample_mixing(1, 2, groups=groups, C=C)
        assert not isinstance(ei.value, MixingArgumentError)
        with pytest.raises(EngineError, match="vmr_set_state"):
            eng.expected_mixing(groups=groups, C=C)
        mix, ov = np.zeros((2, L, C, C), np.uint64), np.zeros((2, L, L), np.uint64)
        emix, eov = np.zeros((L, C, C)), np.zeros((L, L))
        gp = groups.ctypes.data
        assert eng.lib.vmr_sample_mixing(eng._h, 1, 2, 1, gp, C, 1, mix.ctypes.data, None, ov.ctypes.data) == _lib.VMR_ESTATE
        assert eng.lib.vmr_expected_mixing(eng._h, gp, C, 1, emix.ctypes.data, None, eov.ctypes.data) == _lib.VMR_ESTATE
        eng.set_state(*_golden_state(d))

        def refused(word, sample_args, expected_args=None):
            assert eng.lib.vmr_sample_mixing(eng._h, *sample_args) == _lib.VMR_EINVAL
            assert word in eng.lib.vmr_last_error(eng._h), eng.lib.vmr_last_error(eng._h)
            if expected_args is not None:
                assert eng.lib.vmr_expected_mixing(eng._h, *expected_args) == _lib.VMR_EINVAL
                assert word in eng.lib.vmr_last_error(eng._h), eng.lib.vmr_last_error(eng._h)

        for bad_c in (0, -1, 65):
            refused(b"C = %d" % bad_c, (1, 2, 1, gp, bad_c, 1, mix.ctypes.data, None, None), (gp, bad_c, 1, emix.ctypes.data, None, None))
        refused(b"group", (1, 2, 1, None, C, 1, mix.ctypes.data, None, None), (None, C, 1, None, emix.ctypes.data, None))
        for bad_label in (C, -2):
            bad = groups.copy()
            bad[N - 1] = bad_label
            refused(b"group[%d]" % (N - 1), (1, 2, 1, bad.ctypes.data, C, 1, mix.ctypes.data, None, None),
                    (bad.ctypes.data, C, 1, emix.ctypes.data, None, None))
        refused(b"n_samples", (1, 0, 1, gp, C, 1, mix.ctypes.data, None, None))
        refused(b"n_trials", (1, 2, 0, gp, C, 1, mix.ctypes.data, None, None))
        refused(b"mix, mutual and overlap", (1, 2, 1, gp, C, 1, None, None, None), (gp, C, 1, None, None, None))
        with pytest.raises(MixingArgumentError, match="n_samples"):
            eng.sample_mixing(1, 0)
        with pytest.raises(MixingArgumentError, match="n_trials"):
            eng.sample_mixing(1, 2, n_trials=0)
        with pytest.raises(MixingArgumentError, match="C = 65"):
            eng.sample_mixing(1, 2, groups=groups, C=65)
        with pytest.raises(MixingArgumentError, match="C = 65"):
            eng.expected_mixing(groups=groups, C=65)
        with pytest.raises(MixingArgumentError, match="outside"):
            eng.sample_mixing(1, 2, groups=groups, C=2)
        with pytest.raises(ValueError, match="integer codes"):
            eng.sample_mixing(1, 2, groups=groups[:-1])
        got = eng.sample_mixing(1, 2, groups=groups, C=C)                           # the handle still works
        assert got["mix"].shape == (2, L, C, C) and got["overlap"].shape == (2, L, L)
        assert eng.expected_mixing(groups=groups, C=C)["mix"].shape == (L, C, C)
    finally:
        eng.close()


def test_more_than_32_layers_refuse_the_overlap():
    """L = 33 > VMR_MIX_LMAX: the overlap is refused with a message that names it; without it the arguments pass (the handle has
    no state yet, which is what the call then reports)."""
    from vimure_amd import _lib
    from vimure_amd.engine import EngineError, MixingArgumentError
    L, N, M, K, C = 33, 6, 3, 2, 2
    g = np.random.RandomState(8)
    X = (g.rand(L, N, N, M) < 0.2).astype(np.uint8)
    eng = _engine_for(X, None, K, True, None)
    try:
        assert L > _lib.MIX_LMAX
        groups = _mod_groups(N, C)
        with pytest.raises(MixingArgumentError, match="overlap"):
            eng.sample_mixing(3, 2, groups=groups, C=C)
        with pytest.raises(MixingArgumentError, match="overlap"):
            eng.expected_mixing()
        with pytest.raises(EngineError, match="vmr_set_state") as ei:
            eng.sample_mixing(3, 2, groups=groups, C=C, overlap=False)
        assert not isinstance(ei.value, MixingArgumentError)
    finally:
        eng.close()


def test_model_posterior_mixing():
    from vimure_amd import VimureModel
    from vimure_amd.mixing import MixingStats
    from vimure_amd.synthetic import standard_sbm
    N, L = 60, 2
    net = standard_sbm(N=N, M=8, L=L, K=2, avg_degree=6.0, eta=0.4, seed=4)
    labels = getattr(net, "communities", None)
    if labels is None:
        labels = np.arange(N) % 2
    groups = ["even" if c == 0 else "odd" for c in labels]
    groups[7] = None
    codes = np.array([-1 if v is None else ("even", "odd").index(v) for v in groups], np.int32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = VimureModel(mutuality=True)
        m.fit(net.X, K=2, seed=1, max_iter=30, num_realisations=1, keep_engine=True)
    try:
        S, sd = 8, 321
        before = m.posterior_network_stats(n_samples=S, seed=sd)
        res = m.posterior_mixing(groups, n_samples=S, seed=sd)
        assert isinstance(res, MixingStats) and m._rho_f is None                 # rho has not crossed PCIe
        assert list(res.labels) == ["even", "odd"] and np.array_equal(res.codes, codes)
        assert np.array_equal(res.group_sizes, np.bincount(codes[codes >= 0], minlength=2))
        Ys = [m.sample_inferred_model(N=1, seed=sd + s, device=True)[0] for s in range(S)]
        want = mixing_np(Ys, codes, 2, True)
        assert want["mix"].min() > 0
        for k in MIX_KEYS:
            assert np.array_equal(getattr(res, k), want[k]), k
        exp = m._engine.expected_mixing(groups=codes, C=2)
        for k in MIX_KEYS:
            assert np.array_equal(res.expected[k], exp[k]), k
        assert res.expected["assortativity"].shape == (L,) and res.assortativity.shape == (S, L)
        assert len(res.summary()) == L * len(res.statistics())
        assert len(res.frame()) == L * 4 and "expected" in res.frame().columns
        dflt = m.posterior_mixing(n_samples=2)                                    # no groups: the overlap only; seed None: the fit's
        assert dflt.mix is None and np.array_equal(
            dflt.overlap, mixing_np([m.sample_inferred_model(N=1, seed=m.seed + s, device=True)[0] for s in range(2)], None, 0, True)["overlap"])
        by_name = m.posterior_mixing({i: g for i, g in enumerate(groups) if g is not None}, n_samples=S, seed=sd)
        assert np.array_equal(by_name.mix, res.mix)
        with pytest.raises(ValueError, match="not a node"):
            m.posterior_mixing({N + 5: "even"}, n_samples=2)
        res2 = m.posterior_mixing(groups, n_samples=S, seed=sd, X=net.X)          # a temporary engine
        for k in MIX_KEYS:
            assert np.array_equal(getattr(res2, k), want[k]), k
        after = m.posterior_network_stats(n_samples=S, seed=sd)
        for k in ("edges", "weight", "mutual"):
            assert np.array_equal(getattr(before, k), getattr(after, k)), k
        for k in before.expected:
            assert np.array_equal(before.expected[k], after.expected[k]), k
    finally:
        m.close()
