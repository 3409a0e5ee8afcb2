#!/usr/bin/env python3
"""Time the inferred network's edge table of BASELINE config 3 (L = 4, N = 2000, M = 200, K = 2; all-ones mask) two ways:
  edge_table_ms   `eng.edge_table("threshold", thr)` (vmr_edge_table: built on the device, only the rows cross PCIe)
  host_ms         the composition that existed before: `eng.readout` (uint8 [L,N,N]) + `eng.get_state()["rho"]` (8 L N^2 K bytes)
                  + NumPy sums over the host's dense X (what batch.karnataka_tables does) + np.nonzero
from a random state (the numbers do not depend on the fit).  The host's copy of X is made before the clock starts: a user of the
host route has it already.  Each route is warmed up once and timed `--repeats` times around a device synchronise; min and median
are kept.  Checks that both give the same rows and columns.  Writes profiles/edge_table_bench.json and prints it.
Usage: python tools/bench_edge_table.py [--repeats 5] [--small]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROW_BYTES = 3 * 4 + 1 + 8 + 8 + 4 + 8 + 4 + 4 + 4 + 1 + 4 + 8      # the 14 columns of vmr_edge_table


def host_table(eng, X, thr):
    """The same table from what crosses PCIe dense: the read-out and rho, and the host's X."""
    L, N, M = eng.L, eng.N, eng.M
    Y = eng.readout("threshold", thr)
    rho = eng.get_state()["rho"]
    n_rep, total = np.empty((L, N, N), np.uint32), np.empty((L, N, N), np.uint64)
    ego, alter = np.zeros((L, N, N), np.uint32), np.zeros((L, N, N), np.uint32)
    q = np.arange(min(N, M))
    for l in range(L):           # layer by layer: a reduction's temporaries are as large as what it reads
        Xl = X[l]
        n_rep[l] = np.count_nonzero(Xl, axis=2)
        total[l] = Xl.sum(axis=2, dtype=np.uint64)
        ego[l, :len(q), :] = Xl[q, :, q]          # X[l,i,j,i]
        alter[l, :, :len(q)] = Xl[:, q, q]        # X[l,i,j,j]
    l, i, j = np.nonzero((n_rep > 0) | (Y > 0))
    return {"l": l.astype(np.int32), "i": i.astype(np.int32), "j": j.astype(np.int32), "y": Y[l, i, j], "prob": rho[l, i, j, 1],
            "mean": rho[l, i, j, 1], "n_rep": n_rep[l, i, j], "total": total[l, i, j], "n_mask": np.full(len(l), M, np.uint32),
            "ego": ego[l, i, j], "alter": alter[l, i, j], "y_T": Y[l, j, i], "n_rep_T": n_rep[l, j, i], "total_T": total[l, j, i]}


def timed(fn, repeats):
    import torch
    fn()      # warm-up: code objects, allocator
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=2)
    ap.add_argument("--small", action="store_true", help="L = 2, N = 300, M = 40: a rehearsal of the script, not a measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edge_table_bench.json"))
    a = ap.parse_args()
    import torch
    from vimure_amd import CaviEngine
    from vimure_amd.synthetic import standard_sbm
    if not torch.cuda.is_available():
        raise SystemExit("bench_edge_table.py measures on a GPU; none is visible")
    L, N, M, K = (2, 300, 40, 2) if a.small else (4, 2000, 200, 2)
    net = standard_sbm(N=N, M=M, L=L, K=2, avg_degree=10.0, eta=0.5, seed=1, device="cuda")
    eng = CaviEngine(net.X, None, K=K, mutuality=True)
    X = net.X.cpu().numpy()
    del net
    torch.cuda.empty_cache()
    g = np.random.RandomState(0)
    rho = g.rand(L, N, N, K)
    rho[..., 0] *= 20.0
    rho /= rho.sum(-1, keepdims=True)
    thr = float(np.quantile(rho[..., 1], 0.99))      # the read-out infers one tie in a hundred
    eng.set_priors(0.1, 0.1, 10.0, 10.0, 0.5, 1.0)
    eng.set_state(g.gamma(2.0, 1.0, (L, M)) + 0.1, g.gamma(2.0, 1.0, (L, M)) + 0.1, g.gamma(5.0, 1.0, (L, K)) + 0.1,
                  g.gamma(2.0, 1.0, (L, K)) + 0.1, 3.0, 2.5, rho)
    del rho
    new, t_new = timed(lambda: eng.edge_table("threshold", thr), a.repeats)
    _, t_size = timed(lambda: eng.edge_table_size("threshold", thr), a.repeats)
    _, t_dev = timed(lambda: eng.edge_table("threshold", thr, device=True), a.repeats)
    old, t_old = timed(lambda: host_table(eng, X, thr), a.host_repeats)
    same = all(new[c].shape == old[c].shape and np.array_equal(new[c].view(np.uint64) if new[c].dtype == np.float64 else new[c],
                                                                 old[c].view(np.uint64) if old[c].dtype == np.float64 else old[c])
               for c in new)
    rows = int(len(new["l"]))
    out = {"case": "small" if a.small else "config3", "L": L, "N": N, "M": M, "K": K, "format": eng.data_format()[0],
           "nnz": eng.data_format()[1], "repeats": a.repeats, "host_repeats": a.host_repeats, "threshold": thr, "rows": rows,
           "ties": L * N * N, "edge_table_ms": min(t_new), "edge_table_median_ms": float(np.median(t_new)), "edge_table_all_ms": t_new,
           "edge_table_size_ms": min(t_size), "edge_table_device_ms": min(t_dev), "edge_table_device_all_ms": t_dev,
           "host_ms": min(t_old), "host_median_ms": float(np.median(t_old)), "host_all_ms": t_old,
           "edge_table_pcie_bytes": rows * ROW_BYTES, "host_pcie_bytes": L * N * N * (1 + 8 * K), "same_table": bool(same)}
    eng.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)
    if not same:
        raise SystemExit("the two routes disagree")


if __name__ == "__main__":
    main()
