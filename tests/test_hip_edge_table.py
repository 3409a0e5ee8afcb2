"""GPU: the inferred network as an edge table built on the device (vmr_edge_table, vmr_edge_table_size).  Every column is held,
integer for integer and bit for bit, to the NumPy restatement (tests/edge_table_util.py) from the dense X, R and the rho given to
`set_state` -- over both data layouts, every mask layout, coordinate-list handles, a wide reporter set, the K = 3 and K = 12
kernels, a stale rho after plain sweeps, a restored snapshot -- and to the merged entry points (`readout`, `ppc_observed`,
`get_inferred_model`, `batch.karnataka_tables`)."""
import ctypes
import warnings

import numpy as np
import pandas as pd
import pytest

from tests.edge_table_util import COLUMNS, assert_tables_equal, edge_table_np

pytestmark = pytest.mark.gpu

PRI = (0.1, 0.1, 10.0, 10.0, 0.5, 1.0)


def _random_state(g, L, N, M, K):
    gs, gr = g.gamma(2.0, 1.0, (L, M)) + 0.1, g.gamma(2.0, 1.0, (L, M)) + 0.1
    ps, pr = g.gamma(5.0, 1.0, (L, K)) + 0.1, g.gamma(2.0, 1.0, (L, K)) + 0.1
    rho = g.rand(L, N, N, K)
    rho[..., 0] *= 3.0
    rho = rho / rho.sum(-1, keepdims=True)
    return gs, gr, ps, pr, 3.0, 2.5, rho


def _engine_for(X, R, K, st, mut=True, coo=False):
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


def _check(eng, X, R, rho, method="rho_max", threshold=0.0, select=3, layer=None):
    want = edge_table_np(X, R, rho, method, threshold, select, layer)
    n = eng.edge_table_size(method, threshold, select, layer)
    assert n == len(want["l"]), (n, len(want["l"]))
    got = eng.edge_table(method, threshold, select, layer)
    assert_tables_equal(got, want)
    return got


# ---------------------------------------------------------------------------------------------- 1. the base case
_CASE1 = {}


def _case1():
    """L = 2, N = 23 (odd), M = 70 (crosses a 64-bit mask word), K = 2; sparse asymmetric counts 0..3; a Bernoulli(0.3) mask with
    rows forced empty and full."""
    if not _CASE1:
        g = np.random.RandomState(5)
        L, N, M, K = 2, 23, 70, 2
        X = (g.rand(L, N, N, M) < 0.02).astype(np.uint8) * g.randint(1, 4, (L, N, N, M)).astype(np.uint8)
        X[:, 5:9, :, :] = 0                       # ties nobody reports, whichever way rho leans
        R = (g.rand(L, N, N, M) < 0.3).astype(np.uint8)
        R[0, 3, :5], R[1, 7, 10:13], R[0, 20, 22] = 0, 0, 0
        R[0, 4, :4], R[1, 22, 0], R[1, 0, 22], R[0, 9, 9] = 1, 1, 1, 1
        _CASE1.update(X=X, R=R, st=_random_state(g, L, N, M, K))
    return _CASE1


def test_base_case_every_method_selection_and_layer(vmr_format):
    c = _case1()
    X, R, rho = c["X"], c["R"], c["st"][6]
    assert not np.array_equal(X, np.swapaxes(X, 1, 2))
    eng = _engine_for(X, R, 2, c["st"])
    try:
        assert eng.data_format()[0] == vmr_format
        thr = float(rho[0, 11, 13, 1])            # a threshold that IS a rho_1: >= takes the tie
        for method, t in (("rho_max", 0.0), ("threshold", thr), ("threshold", 0.37)):
            for select in (1, 2, 3):
                for layer in (None, 1):
                    got = _check(eng, X, R, rho, method, t, select, layer)
                    n = len(got["l"])
                    assert 0 < n < (2 if layer is None else 1) * 23 * 23
        got = eng.edge_table("threshold", thr, 2)
        hit = (got["l"] == 0) & (got["i"] == 11) & (got["j"] == 13)
        assert hit.sum() == 1 and got["y"][hit][0] == 1 and got["prob"][hit][0] == thr
        # the selection by names, and without a mask
        assert_tables_equal(eng.edge_table(select=("inferred", "reported")), edge_table_np(X, R, rho, "rho_max", 0.0, 3))
        assert_tables_equal(eng.edge_table(select="reported"), edge_table_np(X, R, rho, "rho_max", 0.0, 1))
    finally:
        eng.close()
    eng = _engine_for(X, None, 2, c["st"])
    try:
        got = _check(eng, X, None, rho)
        assert (got["n_mask"] == 70).all()
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 2. mask lists, narrow and wide reporter sets
def test_self_reporter_mask_lists_through_from_coo():
    from vimure_amd.synthetic import self_reporter_mask
    g = np.random.RandomState(6)
    L, N, M, K = 1, 37, 37, 2
    R = np.asarray(self_reporter_mask(L, N, M)).astype(np.uint8)
    X = ((g.rand(L, N, N, M) < 0.04) * g.randint(1, 3, (L, N, N, M))).astype(np.uint8)     # also outside R: the counts ignore R
    own = (g.rand(L, N, N) < 0.3)
    ar = np.arange(N)
    X[0, ar[:, None], ar[None, :], ar[:, None]] = np.where(own[0], 1, X[0, ar[:, None], ar[None, :], ar[:, None]])
    st = _random_state(g, L, N, M, K)
    eng = _engine_for(X, R, K, st, coo=True)
    try:
        assert eng.mask_format()[0] == "lists"
        for select in (1, 2, 3):
            got = _check(eng, X, R, st[6], select=select)
        assert got["ego"].max() > 0 and got["alter"].max() > 0 and got["n_mask"].max() <= 2 and got["n_mask"].min() >= 1
        assert (got["n_rep"] > 2).any()           # reports from outside R are counted
    finally:
        eng.close()


def test_fewer_reporters_than_nodes():
    g = np.random.RandomState(7)
    L, N, M, K = 1, 12, 5, 2
    X = ((g.rand(L, N, N, M) < 0.4) * g.randint(1, 4, (L, N, N, M))).astype(np.uint8)
    st = _random_state(g, L, N, M, K)
    eng = _engine_for(X, None, K, st)
    try:
        got = _check(eng, X, None, st[6])
        assert (got["ego"][got["i"] >= M] == 0).all() and (got["alter"][got["j"] >= M] == 0).all()
        assert got["ego"][got["i"] < M].max() > 0 and got["alter"][got["j"] < M].max() > 0
    finally:
        eng.close()


def test_wide_reporter_set_on_the_general_kernels():
    g = np.random.RandomState(8)
    L, N, M, K = 1, 40, 9000, 2
    n = 3000
    X = np.zeros((L, N, N, M), np.uint8)
    X[0, g.randint(0, N, n), g.randint(0, N, n), g.randint(0, M, n)] = g.randint(1, 4, n)
    X[0, 3, 4, 3], X[0, 3, 4, 4], X[0, 3, 4, 8999] = 2, 1, 3
    R = (X > 0).astype(np.uint8)
    extra = (np.zeros(500, int), g.randint(0, N, 500), g.randint(0, N, 500), g.randint(0, M, 500))
    R[extra] = 1
    st = _random_state(g, L, N, M, K)
    eng = _engine_for(X, R, K, st, coo=True)
    try:
        got = _check(eng, X, R, st[6])
        hit = (got["i"] == 3) & (got["j"] == 4)
        assert got["ego"][hit][0] == 2 and got["alter"][hit][0] == 1 and got["n_rep"][hit][0] >= 3
        _check(eng, X, R, st[6], "threshold", 0.3, 1)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 3. larger K
@pytest.mark.parametrize("K", [3, 12])
def test_larger_k(K):
    g = np.random.RandomState(10 + K)
    L, N, M = 2, 19, 21
    X = ((g.rand(L, N, N, M) < 0.06) * g.randint(1, 12, (L, N, N, M))).astype(np.uint8)
    R = (g.rand(L, N, N, M) < 0.5).astype(np.uint8)
    st = _random_state(g, L, N, M, K)
    eng = _engine_for(X, R, K, st)
    try:
        assert X.max() == 11
        got = _check(eng, X, R, st[6])
        Y = eng.readout("rho_max")
        assert np.array_equal(got["y"], Y[got["l"], got["i"], got["j"]]) and got["y"].max() > 1
        assert np.array_equal(got["y_T"], Y[got["l"], got["j"], got["i"]])
        _check(eng, X, R, st[6], select=2, layer=0)
        _check(eng, X, R, st[6], "threshold", 0.2, 3)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 4. the rho the table reads
def _oracle_start(N=24, M=12, L=2, K=2):
    from oracle import vimure_oracle as vo
    from vimure_amd.synthetic import standard_sbm
    net = standard_sbm(N=N, M=M, L=L, K=K, avg_degree=4.0, eta=0.4, seed=3)
    X = np.asarray(net.X).astype(np.uint8)
    R = (np.random.RandomState(0).rand(*X.shape) < 0.8).astype(np.uint8)
    pr = vo.make_priors(L, M, K)
    st = vo.init_state(vo.Problem(X, R, K, True, pr), np.random.RandomState(1))
    pri = (pr.alpha_theta, pr.beta_theta, pr.alpha_lambda, pr.beta_lambda, pr.alpha_eta, pr.beta_eta)
    return X, R, pri, (st.gamma_shp, st.gamma_rte, st.phi_shp, st.phi_rte, st.nu_shp, st.nu_rte, st.pr_rho)


def test_rho_left_unwritten_by_plain_sweeps(monkeypatch):
    from vimure_amd import CaviEngine
    monkeypatch.setenv("VMR_DEBUG_LAZY_RHO", "1")     # every reader of rho has to bring it up to date itself
    X, R, pri, st = _oracle_start()
    eng = CaviEngine(X, R, K=2, mutuality=True)
    try:
        eng.set_priors(*pri)
        eng.set_state(*st)
        eng.step(3)
        got = eng.edge_table("threshold", 0.3)          # the first reader after the sweeps
        rho = eng.get_state()["rho"]
        assert not np.array_equal(rho, st[6])
        assert_tables_equal(got, edge_table_np(X, R, rho, "threshold", 0.3))
        Y = eng.readout("threshold", 0.3)
        assert np.array_equal(got["y"], Y[got["l"], got["i"], got["j"]])
    finally:
        eng.close()


def test_after_restore_the_table_is_the_snapshots():
    from vimure_amd import CaviEngine
    X, R, pri, st = _oracle_start()
    eng = CaviEngine(X, R, K=2, mutuality=True)
    try:
        eng.set_priors(*pri)
        eng.set_state(*st)
        eng.step(2)
        rho_snap = eng.get_state()["rho"].copy()
        eng.snapshot()
        eng.step(4)
        later = eng.edge_table()
        eng.restore()
        assert_tables_equal(eng.edge_table(), edge_table_np(X, R, rho_snap))
        assert not np.array_equal(later["prob"], edge_table_np(X, R, rho_snap)["prob"])
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 5. edges
def test_empty_table_capacity_arguments_state_and_repeatability():
    import torch
    from vimure_amd import _lib
    from vimure_amd.engine import EngineError
    c = _case1()
    X, R, st = c["X"], c["R"], c["st"]
    # nothing reported, nothing inferred: no rows, no error
    rho0 = np.zeros_like(st[6])
    rho0[..., 0] = 1.0
    eng = _engine_for(np.zeros_like(X), R, 2, st[:6] + (rho0,))
    try:
        assert eng.edge_table_size() == 0
        got = eng.edge_table()
        assert [c for c in got] == [c for c, _ in COLUMNS] and all(len(a) == 0 for a in got.values())
        assert eng.lib.vmr_edge_table(eng._h, _lib.READ_RHO_MAX, 0.0, 3, -1, 0, *([None] * 14), 0) == 0
    finally:
        eng.close()
    eng = _engine_for(X, R, 2, None)
    try:
        with pytest.raises(EngineError, match="vmr_set_state"):
            eng.edge_table()
        with pytest.raises(EngineError, match="vmr_set_state"):
            eng.edge_table_size()
        assert eng.lib.vmr_edge_table_size(eng._h, _lib.READ_RHO_MAX, 0.0, 3, -1, ctypes.byref(ctypes.c_uint64())) == _lib.VMR_ESTATE
        eng.set_state(*st)
        n = eng.edge_table_size()
        short = {c: np.full(n - 1, 0x5a, t) for c, t in COLUMNS}
        with pytest.raises(EngineError, match="rows"):
            eng.edge_table(out=short)
        assert all((a == np.full(n - 1, 0x5a, a.dtype)).all() for a in short.values())     # nothing was written
        with pytest.raises(EngineError, match="method"):
            eng.edge_table(method="rho_mean")
        for select in (0, 4, ()):
            with pytest.raises(EngineError, match="select"):
                eng.edge_table(select=select)
            with pytest.raises(EngineError, match="select"):
                eng.edge_table_size(select=select)
        with pytest.raises(ValueError):
            eng.edge_table(layer=2)
        # a larger capacity and missing columns are fine; the handle still works
        part = {"i": np.full(n + 3, -1, np.int32), "prob": np.full(n + 3, -1.0)}
        eng.edge_table(out=part)
        a, b = eng.edge_table(), eng.edge_table()
        assert all(a[c].tobytes() == b[c].tobytes() for c in a)
        assert np.array_equal(part["i"][:n], a["i"]) and np.array_equal(part["prob"][:n], a["prob"]) and (part["i"][n:] == -1).all()
        assert_tables_equal(a, edge_table_np(X, R, st[6]))
        d = eng.edge_table(device=True)
        assert all(torch.is_tensor(d[c]) and d[c].is_cuda for c in d)
        for c, t in COLUMNS:
            assert np.array_equal(d[c].cpu().numpy().view(t), a[c]), c
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 6. against the observed statistics
def test_union_and_agreement_counts_match_ppc_observed(vmr_format):
    c = _case1()
    R = c["R"]
    X = c["X"] * R                                    # within R the table's counts are those of the support
    eng = _engine_for(X, R, 2, c["st"])
    try:
        got = eng.edge_table(select=1)
        obs = eng.ppc_observed()
        for l in range(2):
            rows = got["l"] == l
            assert int((got["n_rep"][rows] > 0).sum()) == int(obs[l, 4]) > 0
            assert int((got["n_rep"][rows] >= 2).sum()) == int(obs[l, 5])
        assert obs[:, 5].sum() > 0
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 7. the model's method, the driver's table
def test_model_edgelist_and_karnataka_edgelist_end_to_end():
    from vimure_amd import VimureModel, batch
    from vimure_amd.synthetic import self_reporter_mask, standard_sbm
    net = standard_sbm(N=30, M=30, K=2, seed=0)
    X = np.asarray(net.X).astype(np.uint8)
    R = np.asarray(self_reporter_mask(1, 30, 30)).astype(np.uint8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = VimureModel().fit(X, R=R, K=2, seed=3, num_realisations=1, max_iter=21, keep_engine=True)
    got = batch.karnataka_edgelist(m, "vil", "money", 3)
    df = m.get_inferred_edgelist(method="heuristic_threshold")
    on = df[df["y"] > 0]
    assert getattr(m, "_rho_f", None) is None         # nothing has fetched rho so far
    Y = m.get_inferred_model("heuristic_threshold")
    l, i, j = np.nonzero(Y)
    assert len(l) > 0 and np.array_equal(on[["layer", "source", "target"]].to_numpy(), np.stack([l, i, j], 1))
    want = batch.karnataka_tables(m, X, R, "vil", "money", 3, 0.5)["edgelist"]
    assert len(want) > 0
    pd.testing.assert_frame_equal(got, want)
    m.close()
    again = batch.karnataka_edgelist(m, "vil", "money", 3, X=X, R=R)      # a temporary engine from the data
    pd.testing.assert_frame_equal(again, want)
