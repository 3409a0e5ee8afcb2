"""CPU: the host pieces of the edge table -- the new C entry points' export, binding and NULL-handle answers, and, with a stub
engine that answers `edge_table` from the NumPy restatement (tests/edge_table_util.py), `VimureModel.get_inferred_edgelist`
(columns, dtypes, the method / threshold resolution of `get_inferred_model`, its errors) and `batch.karnataka_edgelist` against
`batch.karnataka_tables` on a small dense example with a hand-set rho_f.  No GPU needed."""
import ctypes
import warnings

import numpy as np
import pandas as pd
import pytest

from tests.edge_table_util import COLUMNS, StubEngine, edge_table_np

EDGELIST_COLUMNS = ["layer", "source", "target", "y", "probability", "mean", "n_reports", "total_reports", "n_mask", "source_report",
                    "target_report", "reciprocated_y", "reciprocated_n_reports", "reciprocated_total"]


def test_entry_points_exported_bound_and_refuse_null_handle():
    from vimure_amd import _lib
    lib = _lib.load()
    assert "vmr_edge_table_size" in _lib.SIGNATURES and "vmr_edge_table" in _lib.SIGNATURES
    assert (_lib.EDGE_REPORTED, _lib.EDGE_INFERRED) == (1, 2)
    assert lib.vmr_edge_table_size(None, _lib.READ_RHO_MAX, 0.0, 3, -1, ctypes.byref(ctypes.c_uint64())) == -1
    assert lib.vmr_edge_table_size(None, _lib.READ_RHO_MAX, 0.0, 3, -1, None) == -1
    assert lib.vmr_edge_table(None, _lib.READ_RHO_MAX, 0.0, 3, -1, 0, *([None] * 14), 0) == -1
    from vimure_amd.engine import EDGE_COLUMNS, EdgeTableArgumentError, EngineError
    assert tuple((c, np.dtype(t)) for c, t in EDGE_COLUMNS) == tuple((c, np.dtype(t)) for c, t in COLUMNS)
    assert issubclass(EdgeTableArgumentError, EngineError) and issubclass(EdgeTableArgumentError, ValueError)


def _example(K=2, mutuality=True, seed=0):
    """A small dense data set and a 'fitted' model by hand: N = M = 7, asymmetric counts 0..2, a self-reporter mask."""
    from vimure_amd import VimureModel
    from vimure_amd.synthetic import self_reporter_mask
    g = np.random.RandomState(seed)
    L, N, M = 1, 7, 7
    R = np.asarray(self_reporter_mask(L, N, M)).astype(np.uint8)
    X = ((g.rand(L, N, N, M) < 0.35) * g.randint(1, 3, (L, N, N, M))).astype(np.uint8)
    X[0, 1, 2, :] = 0
    X[0, 1, 2, 1] = X[0, 1, 2, 2] = 1          # both ends report once: in the intersection
    X[0, 3, 4, :] = 0                          # nobody reports (3, 4) ...
    rho = g.rand(L, N, N, K)
    rho[0, 3, 4, 1] = 5.0                      # ... and the model infers it
    rho = rho / rho.sum(-1, keepdims=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = VimureModel(mutuality=mutuality)
    m.L, m.N, m.M, m.K = L, N, M, K
    m.EPS = 1e-12
    m.gamma_shp_f = np.ones((L, M))
    m.rho_f = rho
    m.G_exp_nu = np.float64(0.9)
    m.G_exp_lambda_f = g.rand(L, K) + 0.1
    m.G_exp_theta_f = g.rand(L, M) + 0.1
    m.num_realisations, m.max_iter, m.seed, m.maxL = 1, 21, 3, -12.5
    m.trace = pd.DataFrame({"realisation": [0], "seed": [3], "iter": [10], "elbo": [-12.5], "runtime": [0.1], "reached_convergence": [False]})
    m._engine = StubEngine(X, R, rho)
    return m, X, R, rho


def test_edgelist_columns_dtypes_and_values():
    m, X, R, rho = _example()
    df = m.get_inferred_edgelist()
    assert list(df.columns) == EDGELIST_COLUMNS
    assert all(df[c].dtype == np.int64 for c in EDGELIST_COLUMNS if c not in ("probability", "mean"))
    assert df["probability"].dtype == np.float64 and df["mean"].dtype == np.float64
    want = edge_table_np(X, R, rho, "rho_max", 0.0, 3)
    assert 0 < len(df) < X.shape[1] ** 2 and len(df) == len(want["l"])
    for col, key in zip(EDGELIST_COLUMNS, [c for c, _ in COLUMNS]):
        assert np.array_equal(df[col].to_numpy(), want[key].astype(df[col].dtype)), col
    assert np.array_equal(df["probability"].to_numpy(), rho[0, df["source"], df["target"], 1])     # K = 2: rho_1 itself
    assert df["n_mask"].max() <= 2 and (df["n_reports"] == 0).any() and (df["y"] == 0).any()
    # the selection and the layer reach the engine as given
    m.get_inferred_edgelist(select=("inferred",), layer=0)
    assert m._engine.calls[-1] == ("rho_max", 0.0, ("inferred",), 0)
    only = m.get_inferred_edgelist(select="inferred")
    assert (only["y"] > 0).all() and len(only) == int((np.argmax(rho, -1) > 0).sum())


def test_methods_and_thresholds_resolve_as_get_inferred_model():
    m, X, R, rho = _example()
    m.get_inferred_edgelist(method="fixed_threshold", threshold=0.25)
    assert m._engine.calls[-1][:2] == ("threshold", 0.25)
    df = m.get_inferred_edgelist(method="heuristic_threshold", select="inferred")
    assert m._engine.calls[-1][:2] == ("threshold", float(0.54 * m.G_exp_nu - 0.01))
    Y = m.get_inferred_model(method="heuristic_threshold")
    l, i, j = np.nonzero(Y)
    assert np.array_equal(df[["layer", "source", "target"]].to_numpy(), np.stack([l, i, j], 1))
    for thr in (None, -0.1, 1.5):
        with pytest.raises(ValueError, match="fixed_threshold"):
            m.get_inferred_edgelist(method="fixed_threshold", threshold=thr)
    with pytest.raises(ValueError, match="'method' should be one of"):
        m.get_inferred_edgelist(method="argmax")
    with pytest.raises(ValueError, match="rho_mean"):
        m.get_inferred_edgelist(method="rho_mean")
    # mutuality off, or K > 2 with a threshold method: the warning of get_inferred_model, then rho_max
    for kw, method in ((dict(mutuality=False), "heuristic_threshold"), (dict(mutuality=False), "rho_mean"), (dict(K=3), "fixed_threshold")):
        m2, X2, R2, rho2 = _example(**kw)
        with pytest.warns(UserWarning, match='Using "rho_max" method'):
            df = m2.get_inferred_edgelist(method=method, threshold=0.5, select="inferred")
        assert m2._engine.calls[-1][:2] == ("rho_max", 0.0)
        with pytest.warns(UserWarning, match='Using "rho_max" method'):
            Y = m2.get_inferred_model(method=method, threshold=0.5)
        assert np.array_equal(df[["source", "target"]].to_numpy(), np.stack(np.nonzero(Y)[1:], 1))
        assert np.array_equal(df["y"].to_numpy(), Y[np.nonzero(Y)])


def test_errors_unfitted_and_mask_without_data():
    from vimure_amd import VimureModel
    m, X, R, rho = _example()
    with pytest.raises(ValueError, match="R= is taken with X= only"):
        m.get_inferred_edgelist(R=R)
    m._engine = None
    with pytest.raises(ValueError, match="keep_engine=True"):
        m.get_inferred_edgelist()
    with pytest.raises(ValueError, match="has not been fitted"):
        VimureModel().get_inferred_edgelist()


def test_karnataka_edgelist_reproduces_karnataka_tables():
    from vimure_amd import batch
    m, X, R, rho = _example()
    want = batch.karnataka_tables(m, X, R, "vil", "money", 7, 1.5)["edgelist"]
    got = batch.karnataka_edgelist(m, "vil", "money", 7)
    assert m._engine.calls[-1] == ("threshold", float(0.54 * m.G_exp_nu - 0.01), ("reported", "inferred"), None)
    assert len(want) > 0 and want["in_intersection"].any() and (want["in_vimure"] & ~want["in_union"]).any()
    assert want["source_report"].any() and want["target_report"].any() and want["reciprocated_in_vimure"].any()
    pd.testing.assert_frame_equal(got, want)
    m3, *_ = _example(K=3)
    with pytest.raises(ValueError, match="K = 2"):
        batch.karnataka_edgelist(m3, "vil", "money", 7)
