"""CPU: the posterior-predictive check's host pieces -- `vimure_amd.utils.calculate_AUC` against the reference's recorded AUCs
(tools/make_golden_ppc.py) and sklearn, the NumPy restatement of `_calculate_mean_poisson` against the reference's recorded
values, and the new C entry points' argument checks (no GPU needed)."""
import ctypes
import warnings

import numpy as np
import pytest

from tests.golden_util import case_config, load_case
from tests.ppc_util import PPC_CASES, dense_of, load_ppc, mean_poisson_np


@pytest.mark.parametrize("case", PPC_CASES)
def test_calculate_auc_matches_reference(case):
    from vimure_amd.utils import calculate_AUC
    d, p = load_case(case), load_ppc(case)
    X, R = d["X"], d["R"]
    mp = dense_of(p["mp_subs"], p["mp_vals"], X.shape)
    for l in range(X.shape[0]):
        assert abs(calculate_AUC(mp[l], X[l], mask=R[l]) - p["auc_layer"][l]) <= 1e-12
    assert abs(calculate_AUC(mp, X, mask=R) - float(p["auc_all"])) <= 1e-12


def test_calculate_auc_heavy_ties_matches_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    from vimure_amd.utils import calculate_AUC
    g = np.random.RandomState(5)
    for trial in range(5):
        pred = g.randint(0, 6, size=(3, 17, 17)).astype(np.float64) / 4.0   # few distinct values: many exact ties
        data = g.poisson(0.6, size=pred.shape)
        mask = g.rand(*pred.shape) < 0.7
        lab = (data > 0).astype(int)
        ref = metrics.auc(*metrics.roc_curve(lab[mask], pred[mask])[:2])
        assert abs(calculate_AUC(pred, data, mask=mask) - ref) <= 1e-12
        ref0 = metrics.auc(*metrics.roc_curve(lab.flatten(), pred.flatten())[:2])
        assert abs(calculate_AUC(pred, data) - ref0) <= 1e-12


def test_calculate_auc_exact_ties_rational():
    from vimure_amd.utils import calculate_AUC
    pred = np.array([1.0, 1.0, 2.0, 1.0, 2.0, 0.5])
    data = np.array([1, 0, 1, 0, 0, 3])
    # positives 1.0, 2.0, 0.5; negatives 1.0, 1.0, 2.0: 2 + 1 half-pairs ... (1.0: 0 + 2 ties; 2.0: 2 + 1 tie; 0.5: 0)
    assert calculate_AUC(pred, data) == (0 + 2 * 0.5 + 2 + 0.5 + 0) / 9


def test_calculate_auc_without_positives_is_nan_with_warning():
    from vimure_amd.utils import calculate_AUC
    with pytest.warns(UserWarning):
        assert np.isnan(calculate_AUC(np.ones(4), np.zeros(4)))
    with pytest.warns(UserWarning):
        assert np.isnan(calculate_AUC(np.ones(4), np.array([1, 0, 0, 0]), mask=np.array([1, 0, 0, 0])))


@pytest.mark.parametrize("case", PPC_CASES)
def test_numpy_restatement_reproduces_reference_values(case):
    d, p = load_case(case), load_ppc(case)
    K, mut, und, seed, priors, fitargs, rho_prior = case_config(d)
    subs, vals = mean_poisson_np(d["X"], d["R"], d["fit_rho_f"], d["fit_G_exp_theta_f"], d["fit_G_exp_lambda_f"],
                                 float(d["fit_G_exp_nu_f"]), mut)
    assert np.array_equal(np.stack(subs), p["mp_subs"].astype(np.int64))   # np.nonzero order: the reference's for a dense R
    np.testing.assert_allclose(vals, p["mp_vals"], rtol=1e-13, atol=0)


def test_entry_points_refuse_null_handle():
    from vimure_amd import _lib
    lib = _lib.load()
    n, a, p, q = ctypes.c_uint64(), ctypes.c_double(), ctypes.c_uint64(), ctypes.c_uint64()
    v = np.zeros(4)
    assert lib.vmr_mean_poisson_size(None, -1, ctypes.byref(n)) == _lib.VMR_EINVAL
    assert lib.vmr_mean_poisson(None, -1, 4, None, None, None, None, v.ctypes.data, 0) == _lib.VMR_EINVAL
    assert lib.vmr_report_auc(None, -1, ctypes.byref(a), ctypes.byref(p), ctypes.byref(q)) == _lib.VMR_EINVAL
    assert lib.vmr_report_auc(None, 0, ctypes.byref(a), None, None) == _lib.VMR_EINVAL


def test_model_without_fit_names_keep_engine_and_x():
    from vimure_amd import VimureModel
    m = VimureModel()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match="keep_engine=True"):
            m.calculate_mean_poisson()
        with pytest.raises(ValueError, match="X="):
            m.report_auc()
