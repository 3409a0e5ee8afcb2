"""GPU: the reporter table on the device (vmr_reporter_table).  The seven counts are held exactly to the NumPy restatement
(vimure_amd/reporters.py) fed with the rho given to `set_state` and the engine's own `get_geometric`; the three sums within
(n K + 16) 2^-52 want + n q, n the reporter's n_scope and q the fixed-point quantum include/vimure_hip.h states
(`reporters.sum_quanta`) -- derived, not measured.  Over both data layouts, no mask, a random mask crossing a 64-bit word with
empty and all-ones rows, a coordinate-list handle with a self-reporter mask (mask lists), K = 2, 3 and the general kernels, both
read-out methods, mutuality on and off; against the merged entry points on the same handle; bit-identical from run to run and
after a restore; a reporter set beyond the LDS bins; the refusals; and through `VimureModel`."""
import warnings

import numpy as np
import pytest

from tests.golden_util import case_config, load_case
from tests.reporter_table_util import assert_counts_equal, assert_sums_close, self_reporter_table

pytestmark = pytest.mark.gpu

PRI = (0.1, 0.1, 10.0, 10.0, 0.5, 1.0)
L, N = 2, 70                  # N: no multiple of 64; 4900 ties: 20 workgroups per layer in the tie pass
METHODS = (("rho_max", 0.0), ("threshold", 0.5))

_CASES = {}


def _case(K, M):
    """X sparse counts with reciprocated reports and reports on the diagonal; rho random and normalised, with rows planted whose
    prob is exactly 0, exactly 1, and whose rho_1 is exactly the threshold 0.5."""
    key = (K, M)
    if key not in _CASES:
        g = np.random.RandomState(70 + K + M)
        X = ((g.rand(L, N, N, M) < 0.05) * g.randint(1, 4, (L, N, N, M))).astype(np.uint8)
        X[:, 5, 9, :3], X[:, 9, 5, :3] = 2, 1                        # reciprocated
        X[0, 11, 11, 1], X[1, 30, 30, M - 1] = 3, 1                  # on the diagonal
        rho = g.rand(L, N, N, K)
        rho[..., 0] *= 6.0
        rho = rho / rho.sum(-1, keepdims=True)
        for q, s in enumerate((0.0, 1.0, 0.5)):
            row = np.zeros(K)
            row[0], row[1] = 1.0 - s, s
            rho[:, 3 + q, ::7] = row
            rho[1, 40:44, 5 + q] = row
        rho = np.ascontiguousarray(rho)
        gs, gr = g.gamma(2.0, 1.0, (L, M)) + 0.1, g.gamma(2.0, 1.0, (L, M)) + 0.1
        ps, pr = g.gamma(5.0, 1.0, (L, K)) + 0.1, g.gamma(2.0, 1.0, (L, K)) + 0.1
        R = (g.rand(L, N, N, M) < 0.5).astype(np.uint8)             # density 0.5, M = 70: two mask words
        R[:, 7] = 0                                                  # empty rows
        R[:, 8], R[0, :, 20] = 1, 1                                  # rows made all ones
        _CASES[key] = dict(X=X, R=R, rho=rho, st=(gs, gr, ps, pr, 3.0, 2.5, rho))
    return _CASES[key]


def _engine(X, R, K, st, mut=True, coo=False):
    from vimure_amd import CaviEngine
    if coo:
        xs = np.nonzero(X)
        eng = CaviEngine.from_coo(xs, X[xs], X.shape, R=None if R is None else np.nonzero(R), K=K, mutuality=mut)
    else:
        eng = CaviEngine(X, R, K=K, mutuality=mut)
    eng.set_priors(*PRI)
    if st is not None:
        eng.set_state(*st)
    return eng


def _quanta(eng, X):
    from vimure_amd.reporters import sum_quanta
    gt, gl, gn, _ = eng.get_geometric()
    return sum_quanta(eng.N, gt, gl, gn, float(np.asarray(X, dtype=np.int64).sum()), eng.mutuality)


def _check(eng, X, R, rho, method, thr, layer=None):
    from vimure_amd.reporters import reporter_table_np
    gt, gl, gn, _ = eng.get_geometric()
    want = reporter_table_np(X, R, rho, gt, gl, gn, eng.mutuality, method, thr)
    q = _quanta(eng, X)
    if layer is not None:
        want = {k: v[layer:layer + 1] for k, v in want.items()}
        q = q[layer:layer + 1]
    got = eng.reporter_table(method=method, threshold=thr, layer=layer)
    assert_counts_equal(got, want)
    assert_sums_close(got, want, want["counts"][..., 0], eng.K, q)
    return got, want


def _classes(R):
    full, empty = R.all(axis=-1), ~R.any(axis=-1)
    return bool(full.any()), bool((~full & ~empty).any()), bool(empty.any())


# ---------------------------------------------------------------------------------------------- 1, 2. counts exact, sums bounded
def _counts_and_sums(K, fmt):
    for M, masked in ((5, False), (70, True)):
        c = _case(K, M)
        R = c["R"] if masked else None
        for mut in (True, False):
            eng = _engine(c["X"], R, K, c["st"], mut)
            try:
                assert eng.data_format()[0] == fmt
                for method, thr in METHODS:
                    got, _ = _check(eng, c["X"], R, c["rho"], method, thr)
                    cn = got["counts"]
                    assert cn[..., 5].min() >= 0 and cn[..., 5].sum() > 0 and cn[..., 4].sum() > 0
                    if masked:
                        assert _classes(c["R"]) == (True, True, True)                    # all-ones, partial and empty rows
                        assert cn[..., 6].sum() > 0 and len(np.unique(cn[..., 0])) > 1
                    else:
                        assert (cn[..., 6] == 0).all() and (cn[..., 0] == N * N).all()
            finally:
                eng.close()


@pytest.mark.parametrize("K", [2, 3])
def test_counts_exact_and_sums_bounded(K, vmr_format):
    _counts_and_sums(K, vmr_format)


def test_counts_exact_and_sums_bounded_general_kernels_k12():
    """More than 8 categories: the general kernels, which exist over the report lists only."""
    _counts_and_sums(12, "sparse")


@pytest.mark.parametrize("mut", [True, False])
def test_from_coo_handle_with_self_reporter_mask(mut):
    from vimure_amd.synthetic import self_reporter_mask
    g = np.random.RandomState(9)
    n = 70
    R = np.asarray(self_reporter_mask(1, n, n)).astype(np.uint8)
    X = ((g.rand(1, n, n, n) < 0.3) * g.randint(1, 3, (1, n, n, n))).astype(np.uint8) * R
    out = (g.rand(1, n, n, n) < 0.002) & (R == 0)
    X[out] = 1                                                       # reports the mask discards
    rho = g.rand(1, n, n, 2)
    rho[..., 0] *= 4.0
    rho = np.ascontiguousarray(rho / rho.sum(-1, keepdims=True))
    gs, gr = g.gamma(2.0, 1.0, (1, n)) + 0.1, g.gamma(2.0, 1.0, (1, n)) + 0.1
    ps, pr = g.gamma(5.0, 1.0, (1, 2)) + 0.1, g.gamma(2.0, 1.0, (1, 2)) + 0.1
    eng = _engine(X, R, 2, (gs, gr, ps, pr, 3.0, 2.5, rho), mut, coo=True)
    try:
        assert eng.mask_format()[0] == "lists"
        for method, thr in METHODS:
            got, _ = _check(eng, X, R, rho, method, thr)
            assert got["counts"][..., 6].sum() == out.sum() > 0 and (got["counts"][..., 0] == 2 * n - 1).all()
            assert got["counts"][..., 5].sum() > 0
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 3. the merged entry points
def _agrees_with_merged(eng, got, K, q, layers, readout=None):
    from tests.reporter_table_util import sums_bound
    cn, sm = got["counts"], got["sums"]
    obs, by = eng.ppc_observed(by_reporter=True)
    assert np.array_equal(cn[..., 1:3], by)
    assert np.array_equal(cn[..., 5].sum(axis=1), obs[:, 3])
    assert cn[..., 0].sum() == eng.mean_poisson_size()
    for l in range(layers):
        subs, vals = eng.mean_poisson(layer=l)
        # np.bincount(subs[3], weights=vals) with the adds in extended precision, so that the bound is the device's alone
        order = np.argsort(subs[3], kind="stable")
        ends = np.searchsorted(subs[3][order], np.arange(eng.M + 1), side="left")
        some = ends[1:] > ends[:-1]             # (each reporter's run is added on its own: a running sum over all reporters would
        want = np.zeros(eng.M)                  # carry the rounding of the far larger total into every difference)
        want[some] = np.add.reduceat(vals[order].astype(np.longdouble), ends[:-1][some]).astype(np.float64)
        assert np.allclose(want, np.bincount(subs[3], weights=vals, minlength=eng.M), rtol=1e-9, atol=0.0)
        bound = sums_bound(want[None, :, None], cn[l:l + 1, :, 0], K, q[l:l + 1, :, 2:3])[0, :, 0]
        assert (np.abs(sm[l, :, 2] - want) <= bound).all(), float(np.abs(sm[l, :, 2] - want).max())
    if readout is not None:
        y = eng.readout(*readout)
        for l in range(layers):
            assert (cn[l, :, 3] == int((y[l] > 0).sum())).all()


@pytest.mark.parametrize("masked", [False, True])
def test_agrees_with_the_merged_entry_points(masked):
    c = _case(3, 70)
    R = c["R"] if masked else None
    eng = _engine(c["X"], R, 3, c["st"])
    try:
        for method, thr in METHODS:
            got = eng.reporter_table(method=method, threshold=thr)
            _agrees_with_merged(eng, got, 3, _quanta(eng, c["X"]), L, None if masked else (method, thr))
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 4. bit identity
def test_bit_identical_between_calls_and_after_restore():
    from oracle import vimure_oracle as vo
    from vimure_amd import CaviEngine
    from vimure_amd.synthetic import standard_sbm
    c = _case(3, 70)
    eng = _engine(c["X"], c["R"], 3, c["st"])
    try:
        a, b = eng.reporter_table(), eng.reporter_table()
        assert np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["sums"].view(np.uint64), b["sums"].view(np.uint64))
        assert (a["sums"][..., 0] > 0).any()
    finally:
        eng.close()
    net = standard_sbm(N=24, M=12, L=2, K=2, avg_degree=4.0, eta=0.4, seed=3)
    X = np.asarray(net.X).astype(np.uint8)
    R = (np.random.RandomState(0).rand(*X.shape) < 0.8).astype(np.uint8)
    pr = vo.make_priors(2, 12, 2)
    st = vo.init_state(vo.Problem(X, R, 2, True, pr), np.random.RandomState(1))
    eng = CaviEngine(X, R, K=2, mutuality=True)
    try:
        eng.set_priors(pr.alpha_theta, pr.beta_theta, pr.alpha_lambda, pr.beta_lambda, pr.alpha_eta, pr.beta_eta)
        eng.set_state(st.gamma_shp, st.gamma_rte, st.phi_shp, st.phi_rte, st.nu_shp, st.nu_rte, st.pr_rho)
        eng.step(2)
        at_snap = eng.reporter_table()
        eng.snapshot()
        eng.step(4)
        later = eng.reporter_table()
        eng.restore()
        back = eng.reporter_table()
        assert np.array_equal(back["counts"], at_snap["counts"])
        assert np.array_equal(back["sums"].view(np.uint64), at_snap["sums"].view(np.uint64))
        assert not np.array_equal(later["sums"], back["sums"])
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 5. beyond the LDS bins
def test_wide_reporter_set_beyond_the_lds_bins():
    """N = M = 2100 > PR_HIST_M = 2048: the bins live in global memory.  A self-reporter coordinate-list handle, one layer, a few
    thousand reports; checked against the sparse computation of the helper (no [N,N,M] array) and the merged entry points."""
    from vimure_amd import CaviEngine
    n, K = 2100, 2
    g = np.random.RandomState(21)
    nr = 6000
    i, j = g.randint(0, n, nr), g.randint(0, n, nr)
    m = np.where(g.rand(nr) < 0.5, i, j)
    m[:40] = (i[:40] + j[:40] + 1) % n                               # (mostly) outside the mask
    i, j, m = np.r_[i, j[:500], 17], np.r_[j, i[:500], 17], np.r_[m, m[:500], 17]      # reciprocated reports, one on the diagonal
    key = np.unique(np.ravel_multi_index((i, j, m), (n, n, n)))
    i, j, m = np.unravel_index(key, (n, n, n))
    xv = 1 + g.randint(0, 3, len(key))
    ii, jj = np.indices((n, n)).reshape(2, -1)
    ri, rj, rm = np.r_[ii, ii[ii != jj]], np.r_[jj, jj[ii != jj]], np.r_[ii, jj[ii != jj]]
    z, zr = np.zeros(len(key), np.int64), np.zeros(len(ri), np.int64)
    rho = g.rand(1, n, n, K)
    rho[..., 0] *= 8.0
    rho = np.ascontiguousarray(rho / rho.sum(-1, keepdims=True))
    gs, gr = g.gamma(2.0, 1.0, (1, n)) + 0.1, g.gamma(2.0, 1.0, (1, n)) + 0.1
    ps, pr = g.gamma(5.0, 1.0, (1, K)) + 0.1, g.gamma(2.0, 1.0, (1, K)) + 0.1
    eng = CaviEngine.from_coo((z, i, j, m), xv, (1, n, n, n), R=(zr, ri, rj, rm), K=K, mutuality=True)
    try:
        eng.set_priors(*PRI)
        eng.set_state(gs, gr, ps, pr, 3.0, 2.5, rho)
        assert eng.mask_format()[0] == "lists" and eng.M > 2048
        gt, gl, gn, _ = eng.get_geometric()
        from vimure_amd.reporters import sum_quanta
        q = sum_quanta(n, gt, gl, gn, float(xv.sum()), True)
        for method, thr in METHODS:
            got = eng.reporter_table(method=method, threshold=thr)
            want = self_reporter_table(n, (i, j, m), xv, rho[0], gt[0], gl[0], gn, True, method, thr)
            assert_counts_equal(got, want)
            assert_sums_close(got, want, want["counts"][..., 0], K, q)
            assert got["counts"][..., 6].sum() > 0 and got["counts"][..., 5].sum() > 0      # discarded and reciprocated reports exist
        _agrees_with_merged(eng, got, K, q, 1)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_and_one_layer():
    from vimure_amd import _lib
    from vimure_amd.engine import EngineError, ReporterTableArgumentError
    c = _case(2, 5)
    eng = _engine(c["X"], None, 2, None)          # no state yet: an argument is refused before the state is even looked at
    try:
        cn, sm = np.zeros((L, 5, _lib.RT_NCOUNT), np.uint64), np.zeros((L, 5, _lib.RT_NSUM))
        for args, word in (((_lib.READ_RHO_MEAN, 0.0, -1, cn.ctypes.data, sm.ctypes.data), b"method"),
                           ((_lib.READ_RHO_MAX, 0.0, L, cn.ctypes.data, sm.ctypes.data), b"layer"),
                           ((7, 0.0, -1, cn.ctypes.data, sm.ctypes.data), b"method"),
                           ((_lib.READ_RHO_MAX, 0.0, -1, None, None), b"NULL")):
            assert eng.lib.vmr_reporter_table(eng._h, *args) == _lib.VMR_EINVAL, args
            msg = eng.lib.vmr_last_error(eng._h)
            assert b"vmr_reporter_table" in msg and word in msg, msg
        assert eng.lib.vmr_reporter_table(eng._h, _lib.READ_RHO_MAX, 0.0, -1, cn.ctypes.data, sm.ctypes.data) == _lib.VMR_ESTATE
        assert not cn.any() and not sm.any()                                              # nothing was launched or written
        for kw in (dict(method="rho_mean"), dict(method="best"), dict(layer=L), dict(outputs=()), dict(outputs=("hist",))):
            with pytest.raises(ReporterTableArgumentError):
                eng.reporter_table(**kw)
        with pytest.raises(EngineError, match="vmr_set_state") as ei:
            eng.reporter_table()
        assert not isinstance(ei.value, ReporterTableArgumentError)
        eng.set_state(*c["st"])
        full = eng.reporter_table()
        one, _ = _check(eng, c["X"], None, c["rho"], "rho_max", 0.0, layer=1)
        assert one["counts"].shape == (1, 5, 7) and np.array_equal(one["counts"][0], full["counts"][1])
        assert np.array_equal(one["sums"][0].view(np.uint64), full["sums"][1].view(np.uint64))
        only = eng.reporter_table(outputs=("sums",))
        assert only["counts"] is None and np.array_equal(only["sums"].view(np.uint64), full["sums"].view(np.uint64))
        # a NaN in rho
        rho = c["rho"].copy()
        rho[1, 17, 19] = np.nan
        eng.set_state(*c["st"][:6], rho)
        with pytest.raises(ValueError, match="NaN") as ei:
            eng.reporter_table()
        assert not isinstance(ei.value, ReporterTableArgumentError)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 7. through the model
def test_through_the_model_on_a_golden_case():
    from vimure_amd import VimureModel
    from vimure_amd.reporters import ReporterTable, reporter_table_np, sum_quanta
    d = load_case("G_config1_sbm")
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = VimureModel(mutuality=bool(d["mutuality"]), undirected=und)
        m.fit(d["X"], R=d["R"], seed=seed, rho_prior=rho_prior, K=K, keep_engine=True, **priors, **fitargs)
    try:
        assert m._rho_f is None
        t = m.reporter_table()
        assert m._rho_f is None                           # read where rho lives
        assert isinstance(t, ReporterTable)
        X, R = np.asarray(d["X"]), np.asarray(d["R"])
        want = reporter_table_np(X, R, m.rho_f, m.G_exp_theta_f, m.G_exp_lambda_f, m.G_exp_nu_f, mut)
        q = sum_quanta(m.N, m.G_exp_theta_f, m.G_exp_lambda_f, m.G_exp_nu_f, float(X.astype(np.int64).sum()), mut)
        got = {"counts": t.counts, "sums": t.sums}
        assert_counts_equal(got, want)
        assert_sums_close(got, want, want["counts"][..., 0], K, q)
        f = t.frame()
        assert len(f) == m.L * m.M and np.array_equal(f["theta"].to_numpy(), np.asarray(m.G_exp_theta_f).reshape(-1))
        assert np.allclose(t.theta_mean, m.gamma_shp_f / m.gamma_rte_f)
        assert t.theta_interval.shape == (m.L, m.M, 2) and (t.theta_interval[..., 0] < t.theta_interval[..., 1]).all()
        thr = m.reporter_table(method="fixed_threshold", threshold=0.3, layer=0)
        want = reporter_table_np(X, R, m.rho_f, m.G_exp_theta_f, m.G_exp_lambda_f, m.G_exp_nu_f, mut, "threshold", 0.3)
        assert_counts_equal({"counts": thr.counts}, {"counts": want["counts"][:1]})
        with pytest.raises(ValueError):
            m.reporter_table(method="rho_mean")
    finally:
        m.close()
