"""Host side of the reporter table (no GPU): `reporters.reporter_table_np` against brute-force loops over three masks, its
identities, the derived columns and NaN rules of `ReporterTable`, the stated fixed point, and the C-ABI entry."""
import numpy as np
import pytest

from tests.reporter_table_util import assert_counts_equal, assert_sums_close, brute_table, self_reporter_table


def _small(seed, M=4, N=6, K=3):
    g = np.random.RandomState(seed)
    X = ((g.rand(1, N, N, M) < 0.35) * g.randint(1, 4, (1, N, N, M))).astype(np.uint8)
    X[0, 1, 2, 0], X[0, 2, 1, 0], X[0, 3, 3, 1] = 2, 1, 3           # a reciprocated pair, a report on the diagonal
    rho = g.rand(1, N, N, K)
    rho[..., 0] *= 2.0
    rho = rho / rho.sum(-1, keepdims=True)
    rho[0, 0, 1] = np.r_[1.0, np.zeros(K - 1)]                       # prob exactly 0
    rho[0, 0, 2] = np.r_[0.0, 1.0, np.zeros(K - 2)]                  # prob exactly 1
    rho[0, 0, 3] = np.r_[0.5, 0.5, np.zeros(K - 2)]                  # rho_1 at the threshold
    gt, gl = g.gamma(2.0, 1.0, (1, M)) + 0.1, g.gamma(2.0, 1.0, (1, K)) + 0.1
    return g, X, rho, gt, gl, 0.7


def _masks(g, X):
    R = (g.rand(*X.shape) < 0.5).astype(np.uint8)
    R[0, 4] = 0                                                      # empty rows
    R[0, :, :, 3] = 0                                                # a reporter with no scope at all
    return {"none": None, "random": R}


@pytest.mark.parametrize("mask", ["none", "random", "self"])
@pytest.mark.parametrize("mutuality", [True, False])
def test_numpy_restatement_against_loops(mask, mutuality):
    from vimure_amd.reporters import reporter_table_np
    from vimure_amd.synthetic import self_reporter_mask
    if mask == "self":
        g, X, rho, gt, gl, gn = _small(5, M=6)
        R = np.asarray(self_reporter_mask(1, 6, 6)).astype(np.uint8)
    else:
        g, X, rho, gt, gl, gn = _small(4)
        R = _masks(g, X)[mask]
    for method, thr in (("rho_max", None), ("threshold", 0.5)):
        got = reporter_table_np(X, R, rho, gt, gl, gn, mutuality, method, thr)
        want = brute_table(X, R, rho, gt, gl, gn, mutuality, method, thr)
        assert_counts_equal(got, want)
        assert_sums_close(got, want, want["counts"][..., 0], rho.shape[-1])
        c, s = got["counts"], got["sums"]
        assert np.array_equal(c[..., 1] + c[..., 6], (X > 0).sum(axis=(1, 2)))
        assert (c[..., 4] <= np.minimum(c[..., 1], c[..., 3])).all()
        assert (s[..., 1] <= s[..., 0]).all()
        if R is None:
            assert (c[..., 6] == 0).all() and (c[..., 0] == 36).all()
        if mask == "random":
            assert c[0, 3, 0] == 0 and c[..., 6].sum() > 0
        assert c[..., 5].sum() > 0 or mask != "none"
    if mask == "self":
        xs = np.nonzero(X[0])
        sp = self_reporter_table(6, xs, X[0][xs], rho[0], gt[0], gl[0], gn, mutuality)
        want = reporter_table_np(X, R, rho, gt, gl, gn, mutuality)
        assert_counts_equal(sp, want)
        assert_sums_close(sp, want, want["counts"][..., 0], rho.shape[-1])


def test_restatement_refuses_bad_arguments():
    from vimure_amd.reporters import reporter_table_np
    g, X, rho, gt, gl, gn = _small(4)
    with pytest.raises(ValueError):
        reporter_table_np(X, None, rho, gt, gl, gn, True, "rho_mean")
    with pytest.raises(ValueError):
        reporter_table_np(X, None, rho, gt, gl, gn, True, "threshold")          # no threshold
    with pytest.raises(ValueError):
        reporter_table_np(X, X[:, :3], rho, gt, gl, gn, True)
    with pytest.raises(ValueError):
        reporter_table_np(X, None, rho[:, :3], gt, gl, gn, True)
    bad = rho.copy()
    bad[0, 2, 2] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        reporter_table_np(X, None, bad, gt, gl, gn, True)


def test_reporter_table_columns_and_nan_rules():
    from vimure_amd.reporters import COUNT_NAMES, SUM_NAMES, ReporterTable
    counts = np.array([[[10, 4, 9, 5, 3, 2, 1], [10, 0, 0, 0, 0, 0, 0]], [[7, 2, 2, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 3]]], np.int64)
    sums = np.array([[[4.5, 2.5, 6.0], [4.5, 0.0, 0.0]], [[0.25, 0.125, 4.0], [0.0, 0.0, 0.0]]])
    t = ReporterTable({"counts": counts, "sums": sums}, theta=np.full((2, 2), 0.5), theta_mean=np.full((2, 2), 0.6),
                      theta_interval=np.zeros((2, 2, 2)))
    for c, n in enumerate(COUNT_NAMES):
        assert np.array_equal(getattr(t, n), counts[..., c])
    for c, n in enumerate(SUM_NAMES):
        assert np.array_equal(getattr(t, n), sums[..., c])
    assert np.array_equal(t.false_reports, [[1, 0], [2, 0]]) and np.array_equal(t.omissions, [[2, 0], [0, 0]])
    assert t.precision[0, 0] == 0.75 and t.recall[0, 0] == 0.6 and t.residual[0, 0] == 3.0 and t.ratio[0, 0] == 1.5
    assert np.isnan(t.precision[0, 1]) and np.isnan(t.recall[0, 1]) and np.isnan(t.ratio[0, 1])      # zero denominators
    assert t.precision[1, 0] == 0.0 and np.isnan(t.recall[1, 0]) and t.ratio[1, 0] == 0.5
    assert np.isnan(t.precision[1, 1]) and t.residual[1, 1] == 0.0
    f = t.frame()
    assert len(f) == 4 and list(f["layer"]) == [0, 0, 1, 1] and list(f["reporter"]) == [0, 1, 0, 1]
    for n in COUNT_NAMES + SUM_NAMES + ("false_reports", "omissions", "precision", "recall", "residual", "ratio", "theta", "theta_mean",
                                        "theta_lo", "theta_hi"):
        assert n in f.columns, n
    assert f["hits"].tolist() == [3, 0, 0, 0] and f["n_out"].tolist() == [1, 0, 0, 3]
    one = ReporterTable({"counts": counts[1:], "sums": sums[1:]}, layers=[1])
    assert one.frame()["layer"].tolist() == [1, 1] and "theta" not in one.frame().columns
    with pytest.raises(AttributeError):
        t.no_such_column
    with pytest.raises(ValueError):
        ReporterTable({"counts": counts[..., :6], "sums": sums})


def test_sum_quanta_restate_the_header():
    from vimure_amd.reporters import sum_quanta
    gt, gl = np.array([[0.5, 2.0]]), np.array([[0.01, 3.0]])
    q = sum_quanta(70, gt, gl, 0.75, 1000.0)            # b = 13 (4900 <= 8192), e_l = 2 (3 < 4), e_x = 10 (1001 < 1024)
    assert q.shape == (1, 2, 3)
    assert (q[..., 0] == 2.0 ** -48).all() and (q[..., 1] == 2.0 ** -48).all()
    assert np.array_equal(q[0, :, 2], gt[0] * 2.0 ** -46 + 0.75 * 2.0 ** -51)
    assert np.array_equal(sum_quanta(70, gt, gl, 0.75, 1000.0, mutuality=False)[0, :, 2], gt[0] * 2.0 ** -46)
    assert sum_quanta(64, gt, gl, 0.0, 1023.0)[0, 0, 0] == 2.0 ** -49          # N^2 = 2^12 exactly


def test_abi_entry_refuses_a_null_handle():
    from vimure_amd import _lib
    lib = _lib.load()
    assert "vmr_reporter_table" in _lib.SIGNATURES and hasattr(lib, "vmr_reporter_table")
    out = np.zeros((1, 2, _lib.RT_NCOUNT), np.uint64)
    assert lib.vmr_reporter_table(None, _lib.READ_RHO_MAX, 0.0, -1, out.ctypes.data, None) == -1
    assert lib.vmr_reporter_table(None, _lib.READ_RHO_MAX, 0.0, -1, None, None) == -1
    assert not out.any()
    from vimure_amd.engine import EngineError, ReporterTableArgumentError
    from vimure_amd.reporters import COUNT_NAMES, SUM_NAMES
    assert issubclass(ReporterTableArgumentError, EngineError) and issubclass(ReporterTableArgumentError, ValueError)
    assert list(COUNT_NAMES) == _lib.RT_COUNT_NAMES and list(SUM_NAMES) == _lib.RT_SUM_NAMES
