"""GPU: the device random draws held, element by element with no tolerance, to the independent NumPy restatement of
tests/draws_ref.py: vmr_sample, vmr_generate_x, vmr_generate_y and vmr_ppc_replicates -- that is philox4x32_10
(csrc/vmr_internal.h), draw_tie (csrc/sample_draw.h) and Rng / poisson_draw / pair_draw (csrc/report_draw.h).  The cases are
built in tests/test_draws_ref_host.py, which asserts on the CPU that none of them holds a draw a last-ulp difference of
exp / log / lgamma or an FMA contraction could flip (draws_ref.MARGIN); every comparison here is np.array_equal.

rho goes on the handle through set_state and the reference is fed what get_state returns.

vmr_sample_stats is tied exactly to CaviEngine.sample by tests/test_hip_netstats.py and so is covered through vmr_sample.

Launch shapes: k_sample runs min(4096, ties / 256) workgroups of 256 threads, so its grid-stride loop takes a second trip
above 1 048 576 ties (test_sample_second_trip_of_the_grid_stride_loop, 1 060 900 ties); k_gen_x runs min(2^20, L N^2) workgroups
(the `second_trip` case, 1 060 900 ties); k_sample_gen runs min(4096, ties / 64) workgroups of 64 threads: a second trip, on
which a thread uses its LDS count column again, above 262 144 ties (test_sample_gen_second_trip, 270 400 ties of K = 9).

Not reachable at these shapes: the high counter word (a tie or pair index >= 2^32), and more than 8192 reporters (the
replicate kernels' wide path would need a rho of 1 GB)."""
import numpy as np
import pytest

from tests import draws_ref as dr
from tests import test_draws_ref_host as cases

pytestmark = pytest.mark.gpu

PRI = (0.1, 0.1, 10.0, 10.0, 0.5, 1.0)


def _engine(X, R, K, rho, coo=False):
    from vimure_amd import CaviEngine
    if coo:
        xs = np.nonzero(X)
        eng = CaviEngine.from_coo(xs, X[xs], X.shape, R=None if R is None else np.nonzero(R), K=K)
    else:
        eng = CaviEngine(X, R, K=K)
    try:
        eng.set_priors(*PRI)
        eng.set_state(*cases.engine_state(X.shape[0], X.shape[3], K, rho))
    except Exception:
        eng.close()
        raise
    return eng


def _rho_back(eng, rho):
    """The handle's rho as get_state returns it -- what the reference is fed.  (set_state stores rho as it is.)"""
    back = eng.get_state()["rho"]
    assert np.array_equal(back, rho)
    return back


# ---------------------------------------------------------------------------------------------- vmr_sample
def _assert_samples(eng, K, rho):
    _rho_back(eng, rho)                                          # (equal bits: the cached reference of the case is the reference of it)
    n = 0
    for n_trials in cases.SAMPLE_TRIALS:
        for seed in cases.SAMPLE_SEEDS:
            want = cases.sample_want(K, n_trials, seed)
            got = eng.sample(seed, n_trials)
            assert got.dtype == np.uint8 and got.shape == want.shape
            bad = np.flatnonzero(got.ravel() != want.ravel())
            assert np.array_equal(got, want), (K, n_trials, seed, bad[:10], got.ravel()[bad[:10]], want.ravel()[bad[:10]])
            n += got.size
    return n


@pytest.mark.parametrize("K", cases.SAMPLE_KS_REG + cases.SAMPLE_KS_GEN)
def test_sample_equals_the_reference(K):
    """L = 3, N = 23; K <= 8: k_sample, trial counts in registers; K > 8: k_sample_gen, counts in LDS.  n_trials 1, 2, 3, 7 (odd
    counts take half of the last Philox call), three seeds (low word, high key word, all ones).  The rows: random, one-hot, zeros
    in the middle, sums of 1 - 1e-12, the boundary rows u = rho_0 / u just below rho_0, mode ties (tests/test_draws_ref_host.py
    holds the hand-made rows to the contract on the host)."""
    rho, marks = cases.sample_case(K)
    L, N = rho.shape[:2]
    eng = _engine(cases.engine_data(L, N, 5), None, K, rho)
    try:
        if K > 8:
            assert eng.sweep_shape()[1] == 0                     # (the general kernels: no LDS levels)
        _assert_samples(eng, K, rho)
        y = eng.sample(cases.CRAFT_SEED, 1).ravel()              # the boundary at the bit, spelled out
        assert np.all(y[marks["at"]] == 1) and np.all(y[marks["above"]] == 0)
        if K >= 3:
            assert np.all(y[marks["last_at"]] == K - 1) and np.all(y[marks["last_above"]] == K - 2)
            assert np.all(eng.sample(cases.CRAFT_SEED, 2).ravel()[marks["mode"]] == 1)      # two categories tie: the first maximum
    finally:
        eng.close()


@pytest.mark.parametrize("K", [2, 3])
def test_sample_on_both_layouts(K, vmr_format):
    """Dense tiles, and report lists: rho stored by sorted position, the sample written back through perm."""
    rho, _ = cases.sample_case(K)
    L, N = rho.shape[:2]
    eng = _engine(cases.engine_data(L, N, 5), None, K, rho)
    try:
        assert eng.data_format()[0] == vmr_format
        _assert_samples(eng, K, rho)
    finally:
        eng.close()


@pytest.mark.parametrize("K", [2, 3])
def test_sample_on_a_from_coo_handle(K):
    rho, _ = cases.sample_case(K)
    L, N = rho.shape[:2]
    eng = _engine(cases.engine_data(L, N, 5), None, K, rho, coo=True)
    try:
        assert eng.data_format()[0] == "sparse"
        _assert_samples(eng, K, rho)
    finally:
        eng.close()


def test_sample_second_trip_of_the_grid_stride_loop():
    rho = cases.sample_big_case()
    L, N, _, K = rho.shape
    assert L * N * N > 4096 * 256
    X = np.zeros((L, N, N, 2), np.uint8)
    X[0, np.arange(0, N, 7), np.arange(3, N + 3, 7) % N, 1] = 1
    eng = _engine(X, None, K, rho)
    try:
        _rho_back(eng, rho)
        for n_trials, seed in ((1, 7), (3, 2 ** 32 + 5)):
            assert np.array_equal(eng.sample(seed, n_trials), cases.sample_big_want(n_trials, seed))
    finally:
        eng.close()


def test_sample_gen_second_trip():
    rho = cases.sample_gen_big_case()
    L, N, _, K = rho.shape
    assert L * N * N > 4096 * 64 and K > 8
    X = np.zeros((L, N, N, 2), np.uint8)
    X[0, np.arange(0, N, 7), np.arange(3, N + 3, 7) % N, 1] = 1
    eng = _engine(X, None, K, rho)
    try:
        _rho_back(eng, rho)
        for n_trials, seed in ((1, 7), (3, 2 ** 32 + 5)):
            assert np.array_equal(eng.sample(seed, n_trials), cases.sample_gen_big_want(n_trials, seed))
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- vmr_generate_x
@pytest.mark.parametrize("name", cases.GENERATE_X_CASES)
def test_generate_x_equals_the_reference(name):
    """vmr_generate_x through synthetic.device_build_x against np.minimum(generate_x_ref, 255): the base cases (both Poisson
    branches and both sides of rate < 30 on one tie row, eta 0, 0.3, 0.9), M = 300 (the reporter stride), counts above 255 (the
    clamp), the self-reporter scope, lambda from Y with and without lambda_diff, and 1 060 900 ties (k_gen_x's second trip)."""
    import torch
    from vimure_amd.synthetic import device_build_x
    c = cases.generate_x_case(name)
    want, lo = cases.generate_x_want(name)
    assert lo >= dr.MARGIN
    dev = torch.device("cuda", 0)
    kw = dict(flag_self_reporter=c["self_reporter"])
    if c["Y"] is not None:
        kw.update(Y=torch.as_tensor(c["Y"], device=dev), lambda_diff=c["lambda_diff"])
    else:
        kw.update(lam=torch.as_tensor(c["lam"], device=dev))
    X = device_build_x(None, c["theta"], c["eta"], c["seed"], **kw)
    torch.cuda.synchronize(dev)
    got = X.cpu().numpy()
    assert got.dtype == np.uint8 and got.shape == want.shape
    if name == "clamp":
        assert want.max() > 255 and got.max() == 255
    bad = np.argwhere(got != np.minimum(want, 255))
    assert np.array_equal(got, np.minimum(want, 255)), (name, len(bad), bad[:5], [(int(got[tuple(b)]), int(want[tuple(b)])) for b in bad[:5]])


# ---------------------------------------------------------------------------------------------- vmr_generate_y
@pytest.mark.parametrize("K", cases.GENERATE_Y_KS)
def test_generate_y_equals_the_reference(K):
    """L = 2, N = 37, C = 3, w of 0, 0.02, 0.8, 5 (inversion) and 45 (PTRS); K = 2 and 4 clip at K - 1, K = 64 lets the PTRS
    draws through."""
    from vimure_amd.synthetic import device_sbm_y
    c = cases.generate_y_case()
    for seed in cases.GENERATE_Y_SEEDS:
        want, lo = cases.generate_y_want(K, seed)
        assert lo >= dr.MARGIN
        Y, _ = device_sbm_y(c["L"], c["N"], K, c["C"], c["w"], c["grp"], seed, "cuda:0")
        got = Y.cpu().numpy()
        assert got.dtype == np.uint8 and np.array_equal(got, want), (K, seed, np.argwhere(got != want)[:5])


# ---------------------------------------------------------------------------------------------- vmr_ppc_replicates
def _assert_ppc(name, n_trials, fmt=None):
    c = cases.ppc_case(name)
    counts_w, by_rep_w, lo, top = cases.ppc_want(name, n_trials)
    assert lo >= dr.MARGIN
    eng = _engine(c["X"], c["R"], c["K"], c["rho"], coo=c["coo"])
    try:
        if fmt is not None:
            assert eng.data_format()[0] == fmt
        if c["coo"]:
            assert eng.mask_format()[0] == "lists"
        _rho_back(eng, c["rho"])
        counts, by_rep = eng.ppc_replicates(c["theta"], c["lam"], c["eta"], cases.PPC_SEED_Y, cases.PPC_SEED_X, n_trials=n_trials, by_reporter=True)
    finally:
        eng.close()
    assert np.array_equal(counts, counts_w), (name, n_trials, counts, counts_w)
    assert np.array_equal(by_rep, by_rep_w)
    return top


@pytest.mark.parametrize("name,n_trials", cases.PPC_RUNS)
def test_ppc_replicates_equal_the_reference(name, n_trials):
    """L = 2, N = 23, M = 70, 3 replicates, a Bernoulli(0.3) mask with rows forced empty and full, K = 2, 3 (k_ns_draw with the
    row in registers) and 12 (counts in LDS); a from_coo self-reporter handle (mask lists); `high`: replicate counts above 255,
    inside the support of R, which the composition of vmr_sample and vmr_generate_x clamps and cannot hold: total and sumsq show whether anything
    clamps."""
    top = _assert_ppc(name, n_trials)
    if name == "high":
        assert top > 255


def test_ppc_replicates_on_both_layouts(vmr_format):
    _assert_ppc("K2", 3, fmt=vmr_format)


def test_ppc_replicates_in_chunks(monkeypatch):
    """3 replicates as 2 + 1 (VMR_NETSTATS_CHUNK, read when the handle is created)."""
    monkeypatch.setenv("VMR_NETSTATS_CHUNK", "2")
    _assert_ppc("K2", 1)
    _assert_ppc("high", 1)
