#!/usr/bin/env python3
"""Time the reporter table at BASELINE config 3 (L = 4, N = 2000, M = 200, K = 2, report lists, no mask), two ways:
  reporter_table_ms   `eng.reporter_table()` (vmr_reporter_table: one pass over rho plus the reports, where rho lives).  The call
                      includes, per layer, the tie-major index of the reports (ppc.hip: a radix sort of the layer's report slots)
                      and the tie -> position table, which every read-side entry point of a report-list handle builds.
  host_ms             the route that existed before: `eng.get_state()["rho"]` (8 L N^2 K bytes over PCIe) plus NumPy over the
                      report list (the coordinates of X > 0), timed once
and the same call at M = 50 with N unchanged: without a mask every tie's row is all ones and is added once, not once per
reporter, so the tie term must not grow with M.  Each route is warmed up once and timed around a device synchronise; the median
and all repeats are kept.  The kernels alone are not timed separately (no event brackets them): pass_ms is null, and the
fraction of the achievable HBM rate (6.3 TB/s of the 8 TB/s peak) is computed from the WHOLE call -- index build included -- so it
is a lower bound of the pass'.  pass_bytes is the algorithmic byte model of DESIGN.md: rho once (8 K B per tie), one class byte, one
4-byte position and one 4-byte row start per tie, and per report the 12 B of its index entry plus the two rho rows, two class
bytes and two positions its tie looks up.  Asserts identical counts on both routes.  Writes profiles/reporter_table_bench.json and prints it.
Usage: python tools/bench_reporter_table.py [--repeats 5] [--small]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12     # bytes / s


def host_table(eng, xs, xv, method="rho_max"):
    """counts [L, M, 7] and exp_hits [L, M] without a mask, from rho on the host and the report list (l, i, j, m), xv."""
    L, N, M = eng.L, eng.N, eng.M
    rho = eng.get_state()["rho"]
    y = np.argmax(rho, axis=-1) > 0
    l, i, j, m = xs
    counts = np.zeros((L, M, 7), np.int64)
    counts[..., 0] = N * N
    counts[..., 3] = y.reshape(L, -1).sum(axis=1)[:, None]
    lm = l * M + m
    counts[..., 1] = np.bincount(lm, minlength=L * M).reshape(L, M)
    counts[..., 2] = np.bincount(lm, weights=xv, minlength=L * M).reshape(L, M).astype(np.int64)
    counts[..., 4] = np.bincount(lm, weights=y[l, i, j], minlength=L * M).reshape(L, M).astype(np.int64)
    key = np.ravel_multi_index((l, i, j, m), (L, N, N, M))
    mir = np.ravel_multi_index((l, j, i, m), (L, N, N, M))
    mut = np.isin(mir, key) & (i != j)
    counts[..., 5] = np.bincount(lm[mut], minlength=L * M).reshape(L, M)
    return counts


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


def make_engine(L, N, M, K, seed):
    import torch
    from vimure_amd import CaviEngine
    from vimure_amd.synthetic import standard_sbm
    net = standard_sbm(N=N, M=M, L=L, K=2, avg_degree=10.0, eta=0.5, seed=seed, device="cuda")
    # (layer by layer: torch.nonzero fails on the 3.2e9 elements of config 3 at once)
    nz = torch.cat([torch.cat([torch.full((len(z), 1), l, dtype=z.dtype, device=z.device), z], 1)
                    for l, z in ((l, torch.nonzero(net.X[l])) for l in range(L))])
    xs = tuple(nz[:, q].cpu().numpy().astype(np.int64) for q in range(4))
    xv = net.X[nz[:, 0], nz[:, 1], nz[:, 2], nz[:, 3]].cpu().numpy().astype(np.int64)
    eng = CaviEngine(net.X, None, K=K, mutuality=True)
    del net, nz
    torch.cuda.empty_cache()
    g = np.random.RandomState(0)
    rho = g.rand(L, N, N, K)
    rho[..., 0] *= 20.0
    rho /= rho.sum(-1, keepdims=True)
    eng.set_priors(0.1, 0.1, 10.0, 10.0, 0.5, 1.0)
    eng.set_state(g.gamma(2.0, 1.0, (L, M)) + 0.1, g.gamma(2.0, 1.0, (L, M)) + 0.1, g.gamma(5.0, 1.0, (L, K)) + 0.1,
                  g.gamma(2.0, 1.0, (L, K)) + 0.1, 3.0, 2.5, rho)
    return eng, xs, xv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="L = 2, N = 300, M = 40 (and 10): a rehearsal of the script, not a measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reporter_table_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_reporter_table.py measures on a GPU; none is visible: the numbers stay unmeasured")
    L, N, M, M2, K = (2, 300, 40, 10, 2) if a.small else (4, 2000, 200, 50, 2)
    eng, xs, xv = make_engine(L, N, M, K, 1)
    new, t_new = timed(lambda: eng.reporter_table(), a.repeats)
    host, t_host = timed(lambda: host_table(eng, xs, xv), 1)
    same = bool(np.array_equal(new["counts"], host))
    reports = int(len(xv))
    pass_bytes = L * N * N * (8 * K + 9) + reports * (12 + 16 * K + 10)
    fmt = eng.data_format()[0]
    eng.close()
    del xs, xv
    eng2, xs2, xv2 = make_engine(L, N, M2, K, 1)
    _, t_m2 = timed(lambda: eng2.reporter_table(), a.repeats)
    reports2 = int(len(xv2))
    eng2.close()
    med = float(np.median(t_new))
    out = {"case": "small" if a.small else "config3", "L": L, "N": N, "M": M, "K": K, "format": fmt, "repeats": a.repeats,
           "ties": L * N * N, "reports": reports,
           "reporter_table_median_ms": med, "reporter_table_ms": min(t_new), "reporter_table_all_ms": t_new,
           "pass_ms": None, "pass_note": "the kernels are not bracketed by events: only the whole call (index build included) is timed",
           "pass_bytes": pass_bytes, "call_fraction_of_achievable_hbm": pass_bytes / (med * 1e-3) / HBM_ACHIEVABLE,
           "host_ms": min(t_host), "host_all_ms": t_host, "host_pcie_bytes": L * N * N * 8 * K,
           "reporter_table_pcie_bytes": int(new["counts"].nbytes + new["sums"].nbytes),
           "narrow": {"M": M2, "reports": reports2, "reporter_table_median_ms": float(np.median(t_m2)), "reporter_table_all_ms": t_m2},
           "same_counts": same}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)
    assert same, "the two routes disagree"


if __name__ == "__main__":
    main()
