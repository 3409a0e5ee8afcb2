"""CPU: the host pieces of the posterior network statistics -- the new C entry points' argument checks, `vimure_amd.utils`'
reciprocity helpers against the reference's recorded values (tools/make_golden_netstats.py), the result object's arithmetic,
and the NumPy restatement of the contract the GPU tests use (tests/netstats_util.py).  No GPU needed."""
import ctypes

import numpy as np
import pytest

from tests.golden_util import load_case
from tests.netstats_util import NETSTATS_CASES, load_netstats, stats_np


def test_entry_points_exported_bound_and_refuse_null_handle():
    from vimure_amd import _lib
    lib = _lib.load()
    assert "vmr_sample_stats" in _lib.SIGNATURES and "vmr_expected_stats" in _lib.SIGNATURES
    counts = np.zeros((2, 1, 4), np.uint64)
    out = np.zeros((1, 4))
    assert lib.vmr_sample_stats(None, 1, 2, 1, None, 0, counts.ctypes.data, None, None) == _lib.VMR_EINVAL
    assert lib.vmr_sample_stats(None, 1, 0, 0, None, 0, None, None, None) == _lib.VMR_EINVAL
    assert lib.vmr_expected_stats(None, out.ctypes.data) == _lib.VMR_EINVAL
    assert lib.vmr_expected_stats(None, None) == _lib.VMR_EINVAL
    assert lib.vmr_sample_stats.argtypes[1] is ctypes.c_uint64


@pytest.mark.parametrize("case", NETSTATS_CASES)
def test_reciprocity_helpers_match_reference(case):
    from vimure_amd.utils import calculate_expected_reciprocity, calculate_overall_reciprocity
    d, q = load_case(case), load_netstats(case)
    rho = d["fit_rho_f"]
    L, N = rho.shape[0], rho.shape[1]
    Y = np.argmax(rho, axis=-1)
    for l in range(L):
        assert int((Y[l] > 0).sum()) == int(q["edges"][l]) > 0
        assert calculate_overall_reciprocity(Y[l]) == q["reciprocity"][l]          # two integers, one rounding
        p = rho[l][..., 1:].sum(-1)
        got = calculate_expected_reciprocity(p)
        rtol = 2 * N * N * 2.0 ** -53    # N^2 non-negative products summed in any order
        assert abs(got - q["expected_reciprocity"][l]) <= rtol * abs(q["expected_reciprocity"][l])


def test_overall_reciprocity_of_empty_network_is_nan():
    from vimure_amd.utils import calculate_overall_reciprocity
    assert np.isnan(calculate_overall_reciprocity(np.zeros((5, 5), np.int64)))
    with pytest.raises(ValueError):
        calculate_overall_reciprocity(np.zeros((2, 5, 5)))


def _fabricated():
    # S = 4 samples, L = 2 layers, N = 10
    return {
        "edges": np.array([[10, 0], [20, 5], [30, 5], [40, 8]]),
        "weight": np.array([[12, 0], [20, 10], [45, 5], [40, 8]]),
        "mutual": np.array([[4, 0], [10, 2], [9, 5], [0, 8]]),
        "tp": np.array([[5, 0], [10, 5], [15, 1], [40, 4]]),
    }


def test_result_object_arithmetic():
    from vimure_amd.netstats import NetworkStats
    c = _fabricated()
    ref = np.array([25, 4])
    exp = {"edges": np.array([24.0, 0.0]), "weight": np.array([30.0, 0.0]), "mutual": np.array([6.0, 0.0]),
           "edges_var": np.array([3.0, 0.0])}
    r = NetworkStats(10, c, expected=exp, ref_edges=ref, seed=7, n_trials=1)
    assert (r.S, r.L) == (4, 2)
    assert r.edges.dtype == np.int64 and np.array_equal(r.mutual, c["mutual"])
    want = np.array([[4 / 12, np.nan], [10 / 20, 2 / 10], [9 / 45, 5 / 5], [0 / 40, 8 / 8]])
    assert np.array_equal(r.reciprocity, want, equal_nan=True)
    assert np.isnan(r.reciprocity[0, 1])
    assert np.array_equal(r.density, c["edges"] / 100.0)
    assert np.array_equal(r.precision, np.array([[5 / 10, np.nan], [10 / 20, 5 / 5], [15 / 30, 1 / 5], [40 / 40, 4 / 8]]), equal_nan=True)
    assert np.array_equal(r.recall, c["tp"] / ref[None, :].astype(float))
    assert np.array_equal(r.f1, 2 * c["tp"] / (c["edges"] + ref[None, :]).astype(float))
    assert r.expected["expected_reciprocity"][0] == 6.0 / 24.0 and np.isnan(r.expected["expected_reciprocity"][1])
    assert r.expected["edges_var"][0] == 3.0
    # without a reference network: no precision / recall / F1
    r0 = NetworkStats(10, {k: c[k] for k in c})
    assert r0.f1 is None and r0.expected is None and "f1" not in r0.statistics()


def test_summary_rows_and_quantiles():
    from vimure_amd.netstats import NetworkStats
    c = _fabricated()
    r = NetworkStats(10, c, ref_edges=np.array([25, 4]))
    q = (0.1, 0.5, 0.9)
    df = r.summary(q=q)
    stats = r.statistics()
    assert len(df) == r.L * len(stats)
    assert list(df.columns) == ["layer", "statistic", "mean", "std", "q0.1", "q0.5", "q0.9"]
    for l in range(r.L):
        for name, arr in stats.items():
            row = df[(df["layer"] == l) & (df["statistic"] == name)]
            assert len(row) == 1
            v = np.asarray(arr[:, l], dtype=np.float64)
            v = v[~np.isnan(v)]
            assert row["mean"].item() == v.mean() and row["std"].item() == v.std()
            assert np.array_equal(row[["q0.1", "q0.5", "q0.9"]].to_numpy()[0], np.quantile(v, q))
    d = r.summary()
    assert list(d.columns)[4:] == ["q0.025", "q0.5", "q0.975"]


def test_stats_np_agrees_with_overall_reciprocity():
    from vimure_amd.utils import calculate_overall_reciprocity
    g = np.random.RandomState(0)
    Ys = (g.rand(5, 2, 9, 9) < 0.4) * g.randint(1, 4, (5, 2, 9, 9))
    Yref = g.rand(2, 9, 9) < 0.5
    st = stats_np(Ys, Yref)
    for s in range(5):
        for l in range(2):
            Y = Ys[s, l]
            assert st["mutual"][s, l] / st["weight"][s, l] == calculate_overall_reciprocity(Y)
            assert st["edges"][s, l] == np.count_nonzero(Y) == st["deg_out"][s, l].sum() == st["deg_in"][s, l].sum()
            assert st["tp"][s, l] == np.count_nonzero(Y[Yref[l]])
            assert st["deg_out"][s, l, 3] == np.count_nonzero(Y[3, :]) and st["deg_in"][s, l, 3] == np.count_nonzero(Y[:, 3])
    assert not stats_np(Ys)["tp"].any()
