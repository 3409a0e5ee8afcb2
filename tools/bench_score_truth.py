#!/usr/bin/env python3
"""Time the scoring of the posterior against a ground truth at BASELINE config 3 (L = 4, N = 2000, M = 200, K = 2) with 101
thresholds, two ways:
  score_truth_ms   `eng.score_truth(Y, thresholds)` (vmr_score_truth: one pass where rho lives, the AUC from sorted positives)
  pass_ms          the same without the AUC (`auc=False`): the histogram pass alone
  host_ms          the composition that existed before: 101 x `eng.readout("threshold", t)` (L N^2 bytes each) plus NumPy counts,
                   plus `eng.get_state()["rho"]` (8 L N^2 K bytes) and `sklearn.metrics.roc_auc_score` per layer
from a random normalised rho (the numbers do not depend on the fit) and a sparse random truth.  Each route is warmed up once and
timed around a device synchronise; min and median are kept.  Asserts identical integer counts (tp and fp at every threshold) and
AUCs within 1e-12.  The pass moves 8 K + 1 bytes per tie; bytes / pass_ms is reported as a fraction of the achievable HBM rate
(6.3 TB/s of the 8 TB/s peak) -- pass_ms is a host-side time of the whole call (truth upload, launches, read-back), so the
fraction is a lower bound of the kernel's.  Writes profiles/score_truth_bench.json and prints it.
Usage: python tools/bench_score_truth.py [--repeats 5] [--small]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12     # bytes / s


def host_scores(eng, Y, thr):
    """(tp + fp split by truth at every threshold [L, n_thr, 2], auc [L]) from dense read-outs and rho on the host."""
    from sklearn.metrics import roc_auc_score
    b = Y > 0
    above = np.empty((eng.L, len(thr), 2), np.int64)
    for q, t in enumerate(thr):
        pred = eng.readout("threshold", float(t)) > 0
        above[:, q, 1] = (pred & b).reshape(eng.L, -1).sum(axis=1)
        above[:, q, 0] = (pred & ~b).reshape(eng.L, -1).sum(axis=1)
    rho = eng.get_state()["rho"]
    auc = np.array([roc_auc_score(b[l].reshape(-1), rho[l, :, :, 1].reshape(-1)) for l in range(eng.L)])
    return above, auc


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
    ap.add_argument("--host-repeats", type=int, default=1)
    ap.add_argument("--small", action="store_true", help="L = 2, N = 300, M = 40: a rehearsal of the script, not a measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_truth_bench.json"))
    a = ap.parse_args()
    import torch
    from vimure_amd import CaviEngine
    from vimure_amd.synthetic import standard_sbm
    if not torch.cuda.is_available():
        raise SystemExit("bench_score_truth.py measures on a GPU; none is visible")
    L, N, M, K = (2, 300, 40, 2) if a.small else (4, 2000, 200, 2)
    net = standard_sbm(N=N, M=M, L=L, K=2, avg_degree=10.0, eta=0.5, seed=1, device="cuda")
    eng = CaviEngine(net.X, None, K=K, mutuality=True)
    del net
    torch.cuda.empty_cache()
    g = np.random.RandomState(0)
    Y = (g.rand(L, N, N) < 0.005).astype(np.uint8)          # a sparse truth: 10 ties per node
    rho = g.rand(L, N, N, K)
    rho[..., 0] *= 20.0
    rho[..., 1] += 5.0 * Y * g.rand(L, N, N)                # the posterior leans towards the truth
    rho /= rho.sum(-1, keepdims=True)
    thr = np.linspace(0, 1, 101)
    eng.set_priors(0.1, 0.1, 10.0, 10.0, 0.5, 1.0)
    eng.set_state(g.gamma(2.0, 1.0, (L, M)) + 0.1, g.gamma(2.0, 1.0, (L, M)) + 0.1, g.gamma(5.0, 1.0, (L, K)) + 0.1,
                  g.gamma(2.0, 1.0, (L, K)) + 0.1, 3.0, 2.5, rho)
    del rho
    Yd = torch.as_tensor(Y).cuda()
    new, t_new = timed(lambda: eng.score_truth(Y, thresholds=thr), a.repeats)
    _, t_pass = timed(lambda: eng.score_truth(Yd, thresholds=thr, auc=False), a.repeats)
    (above, auc), t_old = timed(lambda: host_scores(eng, Y, thr), a.host_repeats)
    got = np.cumsum(new["hist"][:, ::-1], axis=1)[:, ::-1][:, 1:]
    same = bool(np.array_equal(got, above)) and bool(np.all(np.abs(new["auc"] - auc) <= 1e-12))
    pass_bytes = L * N * N * (8 * K + 1)
    out = {"case": "small" if a.small else "config3", "L": L, "N": N, "M": M, "K": K, "format": eng.data_format()[0], "n_thr": len(thr),
           "repeats": a.repeats, "host_repeats": a.host_repeats, "ties": L * N * N, "positives": int(new["conf"][:, 4].sum()),
           "score_truth_ms": min(t_new), "score_truth_median_ms": float(np.median(t_new)), "score_truth_all_ms": t_new,
           "pass_ms": min(t_pass), "pass_all_ms": t_pass, "pass_bytes": pass_bytes,
           "pass_fraction_of_achievable_hbm": pass_bytes / (min(t_pass) * 1e-3) / HBM_ACHIEVABLE,
           "host_ms": min(t_old), "host_all_ms": t_old, "host_pcie_bytes": L * N * N * (len(thr) + 8 * K),
           "score_truth_pcie_bytes": L * N * N + int(new["hist"].nbytes), "same_counts": same}
    eng.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)
    assert same, "the two routes disagree"


if __name__ == "__main__":
    main()
