"""CPU: the host pieces of the posterior predictive check -- the new C entry points' export, binding and argument checks, the
NumPy restatement of the statistics the GPU tests use (tests/ppc_rep_util.py) on a hand-written case, the result object's
arithmetic, and the host draw of the replicates' parameters.  No GPU needed."""
import ctypes

import numpy as np
import pytest

from tests.ppc_rep_util import STAT_NAMES, stats_coo, stats_np


def test_entry_points_exported_bound_and_refuse_null_handle():
    from vimure_amd import _lib
    lib = _lib.load()
    assert "vmr_ppc_replicates" in _lib.SIGNATURES and "vmr_ppc_observed" in _lib.SIGNATURES
    assert _lib.PPC_NSTAT == 6 and tuple(_lib.PPC_STAT_NAMES) == STAT_NAMES
    th, la, et = np.ones((2, 1, 3)), np.ones((2, 1, 2)), np.zeros(2)
    counts = np.zeros((2, 1, 6), np.uint64)
    assert lib.vmr_ppc_replicates(None, 2, 1, 2, 1, th.ctypes.data, la.ctypes.data, et.ctypes.data, counts.ctypes.data, None) == _lib.VMR_EINVAL
    assert lib.vmr_ppc_replicates(None, 0, 1, 2, 0, None, None, None, None, None) == _lib.VMR_EINVAL
    assert lib.vmr_ppc_observed(None, counts.ctypes.data, None) == _lib.VMR_EINVAL
    assert lib.vmr_ppc_observed(None, None, None) == _lib.VMR_EINVAL
    assert lib.vmr_ppc_replicates.argtypes[2] is ctypes.c_uint64 and lib.vmr_ppc_replicates.argtypes[3] is ctypes.c_uint64


def _hand_case():
    X = np.zeros((1, 3, 3, 3), np.int64)
    R = np.zeros((1, 3, 3, 3), np.int64)
    for (i, j, m), x, r in [((0, 1, 0), 3, 1),    # a count of 3: sumsq != total; reciprocated by ...
                            ((1, 0, 0), 1, 1),    # ... the same reporter on the mirror tie
                            ((0, 2, 1), 2, 1),    # its mirror report ...
                            ((2, 0, 1), 4, 0),    # ... is positive but outside S: not mutual, not counted
                            ((1, 1, 2), 1, 1),    # a diagonal entry in S: counted, never mutual
                            ((0, 1, 1), 1, 1),    # a second positive reporter on tie (0, 1): agreed
                            ((1, 0, 1), 0, 1),    # in S, no report
                            ((2, 1, 2), 5, 0),    # outside S
                            ((1, 2, 0), 0, 1)]:
        X[0, i, j, m], R[0, i, j, m] = x, r
    return X, R


def test_stats_np_on_a_hand_written_case():
    X, R = _hand_case()
    counts, by_rep = stats_np(X, R)
    assert counts.shape == (1, 6) and by_rep.shape == (1, 3, 2) and counts.dtype == by_rep.dtype == np.int64
    # n_pos, total, sumsq, mutual, ties_reported {(0,1), (1,0), (0,2), (1,1)}, ties_agreed {(0,1)}
    assert counts[0].tolist() == [5, 8, 16, 2, 4, 1]
    assert by_rep[0].tolist() == [[2, 4], [2, 3], [1, 1]]
    # without a mask everything is in S: the reports of (2,0,1) and (2,1,2) enter, (0,2,1) / (2,0,1) become mutual
    c1, b1 = stats_np(X, None)
    assert c1[0].tolist() == [7, 17, 16 + 16 + 25, 4, 6, 1]
    assert b1[0].tolist() == [[2, 4], [3, 7], [2, 6]]
    # the coordinate-list restatement agrees
    for Rm in (R, None):
        c2, b2 = stats_coo(np.nonzero(X), X[np.nonzero(X)], None if Rm is None else np.nonzero(Rm), X.shape)
        want = stats_np(X, Rm)
        assert np.array_equal(c2, want[0]) and np.array_equal(b2, want[1])


def _fabricated():
    obs = np.array([[4, 10, 30, 2, 3, 1], [0, 0, 0, 0, 0, 0]])
    rep = np.array([[[4, 12, 30, 0, 3, 1], [0, 0, 0, 0, 0, 0]],
                    [[5, 10, 20, 2, 3, 0], [1, 1, 1, 0, 1, 0]],
                    [[3, 9, 40, 4, 2, 1], [0, 0, 0, 0, 0, 0]],
                    [[4, 11, 31, 2, 5, 1], [2, 4, 8, 2, 1, 1]]])
    return obs, rep


def test_predictive_check_p_values_with_ties():
    from vimure_amd.predictive import PredictiveCheck
    obs, rep = _fabricated()
    r = PredictiveCheck(obs, rep, support=[20, 20], seed_y=3, seed_x=3 + 2 ** 32, eta_redraws=2)
    assert (r.n_rep, r.L) == (4, 2) and r.STATISTICS == STAT_NAMES and r.eta_redraws == 2
    pv = r.p_values()
    assert pv.shape == (2, 6)
    # layer 0: n_pos 4 vs (4,5,3,4): 1 above, 2 equal -> (1 + 1) / 4; total 10 vs (12,10,9,11): (2 + .5) / 4; ...
    assert pv[0].tolist() == [0.5, 0.625, 0.625, 0.5, 0.5, 0.375]
    # layer 1: all zeros observed; replicates (0, 1, 0, 2) -> (2 + 1) / 4 for n_pos
    assert pv[1].tolist() == [0.75, 0.75, 0.75, 0.625, 0.75, 0.625]
    o, v = r.statistic("mutual")
    assert o.tolist() == [2, 0] and v[:, 0].tolist() == [0, 2, 4, 2]
    assert r.p_values_by_reporter() is None
    ro, rv = r.report_reciprocity
    assert ro[0] == 2 / 4 and np.isnan(ro[1])
    assert np.array_equal(rv, np.array([[0.0, np.nan], [2 / 5, 0.0], [4 / 3, np.nan], [2 / 4, 1.0]]), equal_nan=True)
    do, dv = r.dispersion
    mean = 10 / 20
    assert do[0] == (30 / 20) / (mean * mean) - 1.0 - 1.0 / mean and np.isnan(do[1])          # no mean to compare with at total 0
    assert dv.shape == (4, 2) and np.isnan(dv[0, 1]) and not np.isnan(dv[:, 0]).any()
    assert PredictiveCheck(obs, rep).dispersion is None
    # per reporter
    ob = np.array([[[1, 2], [0, 0]]])
    rb = np.array([[[[1, 2], [0, 0]]], [[[2, 5], [1, 1]]]])
    rr = PredictiveCheck(obs[:1], rep[:2, :1], observed_by_reporter=ob, replicated_by_reporter=rb)
    assert rr.p_values_by_reporter().tolist() == [[[0.75, 0.75], [0.75, 0.75]]]
    with pytest.raises(ValueError):
        PredictiveCheck(obs[:, :5], rep)


def test_predictive_check_summary_rows_and_quantiles():
    from vimure_amd.predictive import PredictiveCheck
    obs, rep = _fabricated()
    r = PredictiveCheck(obs, rep, support=[20, 20])
    q = (0.1, 0.5, 0.9)
    df = r.summary(q=q)
    assert len(df) == 6 * r.L
    assert list(df.columns) == ["statistic", "layer", "observed", "q0.1", "q0.5", "q0.9", "p_value"]
    pv = r.p_values()
    for k, name in enumerate(STAT_NAMES):
        for l in range(r.L):
            row = df[(df["layer"] == l) & (df["statistic"] == name)]
            assert len(row) == 1
            assert row["observed"].item() == obs[l, k] and row["p_value"].item() == pv[l, k]
            assert np.array_equal(row[["q0.1", "q0.5", "q0.9"]].to_numpy()[0], np.quantile(rep[:, l, k].astype(np.float64), q))
    assert list(r.summary().columns)[3:6] == ["q0.025", "q0.5", "q0.975"]
    d = r.summary(derived=True)
    assert len(d) == 8 * r.L and set(d["statistic"]) == set(STAT_NAMES) | {"report_reciprocity", "dispersion"}
    row = d[(d["statistic"] == "report_reciprocity") & (d["layer"] == 0)]
    assert row["observed"].item() == 0.5 and row["p_value"].item() == (1 + 0.5 * 1) / 4


def _posterior(g, L=2, M=5, K=3):
    return (g.gamma(2.0, 1.0, (L, M)) + 0.5, g.gamma(2.0, 1.0, (L, M)) + 0.5, g.gamma(3.0, 1.0, (L, K)) + 0.5,
            g.gamma(2.0, 1.0, (L, K)) + 0.5)


def test_parameter_draws_reproducible_and_in_build_x_order():
    from vimure_amd.predictive import draw_parameters
    gs, gr, ps, pr = _posterior(np.random.RandomState(0))
    a = draw_parameters(gs, gr, ps, pr, 2.0, 40.0, 3, 17)
    b = draw_parameters(gs, gr, ps, pr, 2.0, 40.0, 3, 17)
    c = draw_parameters(gs, gr, ps, pr, 2.0, 40.0, 3, 18)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    assert not np.array_equal(a[0], c[0])
    assert a[0].shape == (3, 2, 5) and a[1].shape == (3, 2, 3) and a[2].shape == (3,) and a[3] == 0
    # the order of PosteriorSyntheticNetwork.build_X: theta, lambda, eta from one RandomState, replicate after replicate
    prng = np.random.RandomState(17)
    for r in range(3):
        assert np.array_equal(a[0][r], prng.gamma(shape=gs, scale=1.0 / gr, size=(2, 5)))
        assert np.array_equal(a[1][r], prng.gamma(shape=ps, scale=1.0 / pr, size=(2, 3)))
        assert a[2][r] == prng.gamma(shape=2.0, scale=1.0 / 40.0, size=1)[0]
    m = draw_parameters(gs, gr, ps, pr, 2.0, 40.0, 4, 17, params="mean")
    assert np.array_equal(m[0], np.broadcast_to(gs / gr, (4, 2, 5))) and np.array_equal(m[1][3], ps / pr)
    assert np.array_equal(m[2], np.full(4, 0.05)) and m[3] == 0


def test_eta_redraws_and_errors():
    from vimure_amd.predictive import draw_parameters
    gs, gr, ps, pr = _posterior(np.random.RandomState(1))
    shp, rte = 2.0, 2.0 / 0.9      # mean 0.9: about a third of the draws lie at or above 1
    th, la, eta, redraws = draw_parameters(gs, gr, ps, pr, shp, rte, 50, 5)
    assert redraws > 0 and np.all(eta < 1.0) and np.all(eta >= 0.0)
    again = draw_parameters(gs, gr, ps, pr, shp, rte, 50, 5)
    assert again[3] == redraws and np.array_equal(again[2], eta) and np.array_equal(again[0], th)
    # the stream: every draw >= 1 is followed by another eta draw before the next replicate's theta
    prng = np.random.RandomState(5)
    n = 0
    for r in range(50):
        prng.gamma(shape=gs, scale=1.0 / gr, size=gs.shape)
        prng.gamma(shape=ps, scale=1.0 / pr, size=ps.shape)
        e = prng.gamma(shape=shp, scale=1.0 / rte, size=1)[0]
        while e >= 1.0:
            e = prng.gamma(shape=shp, scale=1.0 / rte, size=1)[0]
            n += 1
        assert e == eta[r]
    assert n == redraws
    with pytest.raises(ValueError, match="redraws"):
        draw_parameters(gs, gr, ps, pr, 2000.0, 1.0, 2, 5)           # eta ~ 2000: never below 1
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        draw_parameters(gs, gr, ps, pr, 3.0, 2.0, 2, 5, params="mean")
    gr0 = gr.copy()
    gr0[0, 0] = 0.0
    with pytest.raises(ValueError, match="theta_rte has some zero entries!"):
        draw_parameters(gs, gr0, ps, pr, shp, rte, 2, 5)
    with pytest.raises(ValueError, match="mutuality_rte has some zero entries!"):
        draw_parameters(gs, gr, ps, pr, shp, 0.0, 2, 5)
    with pytest.raises(ValueError, match="params"):
        draw_parameters(gs, gr, ps, pr, shp, rte, 2, 5, params="mode")
