"""NumPy restatement of the edge table (vmr_edge_table, include/vimure_hip.h) from the dense X, R and the rho given to
`set_state`: the oracle of tests/test_hip_edge_table.py and the stub engine of tests/test_edge_table_host.py."""
import numpy as np

COLUMNS = (("l", np.int32), ("i", np.int32), ("j", np.int32), ("y", np.uint8), ("prob", np.float64), ("mean", np.float64),
           ("n_rep", np.uint32), ("total", np.uint64), ("n_mask", np.uint32), ("ego", np.uint32), ("alter", np.uint32),
           ("y_T", np.uint8), ("n_rep_T", np.uint32), ("total_T", np.uint64))
REPORTED, INFERRED = 1, 2


def readout_np(rho, method, threshold=0.0):
    if method == "rho_max":
        return np.argmax(rho, axis=-1).astype(np.uint8)
    assert method == "threshold"
    return (rho[..., 1] >= threshold).astype(np.uint8)


def per_tie_np(X, R, rho, method, threshold=0.0):
    """Every per-tie quantity as an [L,N,N] array."""
    X = np.asarray(X).astype(np.int64)
    L, N, _, M = X.shape
    K = rho.shape[-1]
    y = readout_np(rho, method, threshold)
    prob, mean = np.zeros((L, N, N)), np.zeros((L, N, N))
    for k in range(1, K):                       # ascending, every product and sum rounded on its own (np.sum's order differs)
        prob = prob + rho[..., k]
        mean = mean + float(k) * rho[..., k]
    n_rep, total = (X > 0).sum(axis=3), X.sum(axis=3)
    n_mask = np.full((L, N, N), M, np.int64) if R is None else (np.asarray(R) != 0).sum(axis=3)
    ego, alter = np.zeros((L, N, N), np.int64), np.zeros((L, N, N), np.int64)
    for q in range(min(N, M)):
        ego[:, q, :] = X[:, q, :, q]            # X[l,i,j,i]
        alter[:, :, q] = X[:, :, q, q]          # X[l,i,j,j]
    T = lambda a: np.swapaxes(a, 1, 2)
    return {"y": y, "prob": prob, "mean": mean, "n_rep": n_rep, "total": total, "n_mask": n_mask, "ego": ego, "alter": alter,
            "y_T": T(y), "n_rep_T": T(n_rep), "total_T": T(total)}


def _select_bits(select):
    if isinstance(select, (int, np.integer)):
        return int(select)
    if isinstance(select, str):
        select = (select,)
    return sum({"reported": REPORTED, "inferred": INFERRED}[s] for s in set(select))


def edge_table_np(X, R, rho, method="rho_max", threshold=0.0, select=3, layer=None):
    """The table as a dict of arrays with the engine's column names and dtypes, rows in lexicographic (l,i,j) order."""
    q = per_tie_np(X, R, rho, method, threshold)
    sel = _select_bits(select)
    assert sel in (1, 2, 3)
    flag = np.zeros(q["y"].shape, bool)
    if sel & REPORTED:
        flag |= q["n_rep"] > 0
    if sel & INFERRED:
        flag |= q["y"] > 0
    if layer is not None:
        keep = np.zeros_like(flag)
        keep[layer] = True
        flag &= keep
    l, i, j = np.nonzero(flag)
    out = {"l": l, "i": i, "j": j}
    for c in q:
        out[c] = q[c][l, i, j]
    return {c: np.ascontiguousarray(out[c]).astype(t) for c, t in COLUMNS}


def assert_tables_equal(got, want):
    assert list(got) == [c for c, _ in COLUMNS], list(got)
    for c, t in COLUMNS:
        g, w = np.asarray(got[c]), np.asarray(want[c])
        assert g.dtype == np.dtype(t), (c, g.dtype)
        assert g.shape == w.shape, (c, g.shape, w.shape)
        if g.dtype == np.float64:               # bit for bit
            g, w = g.view(np.uint64), w.view(np.uint64)
        assert np.array_equal(g, w), (c, np.flatnonzero(g != w)[:8])


class StubEngine:
    """What `VimureModel._ppc_engine` hands out, answering `edge_table` from the restatement (no GPU)."""

    def __init__(self, X, R, rho):
        self.X, self.R, self.rho = X, R, rho
        self.calls = []

    def edge_table(self, method="rho_max", threshold=0.0, select=("reported", "inferred"), layer=None, device=False):
        self.calls.append((method, threshold, select, layer))
        return edge_table_np(self.X, self.R, self.rho, method, threshold, select, layer)

    def close(self):
        pass
