#!/usr/bin/env python3
"""Time the posterior mixing read-out (vmr_sample_mixing, vmr_expected_mixing) at BASELINE config 3's shape (L = 4, N = 2000,
M = 200, K = 2, report lists) from a random state (the numbers do not depend on the fit), whole calls, each against the same
answer from samples (or rho) copied over PCIe plus NumPy:
  sample_mixing_ms     `eng.sample_mixing(seed, S, groups, C)`, S = 256, C = 4: the draw, the walk with its LDS counters, the flush
  sample_overlap_ms    the same without groups: the overlap between layers alone
  sample_stats_ms      `eng.sample_stats(seed, S)` of the same engine, for scale: the same draw with k_ns_reduce behind it
  expected_mixing_ms   `eng.expected_mixing(groups, C)`: P written once, the rows' sums, the fixed-order finish
  host_sample_ms       the route that exists without it: --host-samples calls of `eng.sample(seed + s)` (L N^2 bytes over PCIe each)
                       plus `np.add.at` and boolean products, scaled to S samples (host_sample_scaled_ms)
  host_expected_ms     `eng.get_state()["rho"]` (8 L N^2 K bytes over PCIe) plus NumPy matrix products
and, at a small shape (--host-n, default L = 2, N = 500), 32 samples on both routes in full.
Each route is warmed up once and timed around a device synchronise; the median and all repeats are kept.  Asserts that the device
and the host give the same integers, and the same expectations within 1e-10.  Writes profiles/mixing_bench.json and prints it.
Usage: python tools/bench_mixing.py [--repeats 3] [--small] [--host-n 500] [--host-samples 4] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS = ("mix", "mutual", "overlap")


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
    eng = CaviEngine(net.X, None, K=K, mutuality=True)
    del net
    torch.cuda.empty_cache()
    g = np.random.RandomState(0)
    rho = g.rand(L, N, N, K)
    rho[..., 0] *= 20.0
    rho /= rho.sum(-1, keepdims=True)
    eng.set_priors(0.1, 0.1, 10.0, 10.0, 0.5, 1.0)
    eng.set_state(g.gamma(2.0, 1.0, (L, M)) + 0.1, g.gamma(2.0, 1.0, (L, M)) + 0.1, g.gamma(5.0, 1.0, (L, K)) + 0.1,
                  g.gamma(2.0, 1.0, (L, K)) + 0.1, 3.0, 2.5, rho)
    return eng


def host_route(eng, seed, S, groups, C):
    """The samples over PCIe, then NumPy: `np.add.at` per layer for the two group tables, boolean products for the overlap."""
    L, N = eng.L, eng.N
    out = {"mix": np.zeros((S, L, C, C), np.int64), "mutual": np.zeros((S, L, C, C), np.int64), "overlap": np.zeros((S, L, L), np.int64)}
    off = ~np.eye(N, dtype=bool)
    lab = (groups[:, None] >= 0) & (groups[None, :] >= 0)
    for s in range(S):
        A = (eng.sample(seed + s) > 0) & off[None]
        for l in range(L):
            i, j = np.nonzero(A[l] & lab)
            np.add.at(out["mix"][s, l], (groups[i], groups[j]), 1)
            i, j = np.nonzero(A[l] & A[l].T & lab)
            np.add.at(out["mutual"][s, l], (groups[i], groups[j]), 1)
            for l2 in range(l, L):
                out["overlap"][s, l, l2] = out["overlap"][s, l2, l] = np.count_nonzero(A[l] & A[l2])
    return out


def host_expected(eng, groups, C):
    rho = eng.get_state()["rho"]
    L, N = eng.L, eng.N
    p = rho[..., 1:].sum(-1) * (1.0 - np.eye(N))[None]
    G = (groups[:, None] == np.arange(C)[None, :]).astype(np.float64)
    out = {"mix": np.stack([G.T @ p[l] @ G for l in range(L)]), "mutual": np.stack([G.T @ (p[l] * p[l].T) @ G for l in range(L)]),
           "overlap": np.zeros((L, L))}
    for l in range(L):
        for l2 in range(L):
            out["overlap"][l, l2] = p[l].sum() if l == l2 else (p[l] * p[l2]).sum()
    return out


def rel_diff(a, b):
    return float(max(np.max(np.abs(a[k] - b[k]) / np.abs(b[k])) for k in KEYS))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-n", type=int, default=500)
    ap.add_argument("--host-samples", type=int, default=4, help="samples the host route draws at the large shape (its time is scaled to S)")
    ap.add_argument("--small", action="store_true", help="L = 2, N = 200, M = 40 and the small shape at N = 60: a rehearsal of the script, not a measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixing_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mixing.py measures on a GPU; none is visible: the numbers stay unmeasured")
    L, N, M, K = (2, 200, 40, 2) if a.small else (4, 2000, 200, 2)
    S, C, seed = (16 if a.small else 256), 4, 17
    Sh = min(S, a.host_samples)
    groups = (np.arange(N) % C).astype(np.int32)
    groups[::17] = -1
    eng = make_engine(L, N, M, K, 1)
    full, t_full = timed(lambda: eng.sample_mixing(seed, S, groups=groups, C=C), a.repeats)
    _, t_ov = timed(lambda: eng.sample_mixing(seed, S), a.repeats)
    _, t_dyads = timed(lambda: eng.sample_stats(seed, S), a.repeats)
    ex, t_exp = timed(lambda: eng.expected_mixing(groups=groups, C=C), a.repeats)
    host, t_host = timed(lambda: host_route(eng, seed, Sh, groups, C), a.repeats)
    hex_, t_hex = timed(lambda: host_expected(eng, groups, C), a.repeats)
    fmt = eng.data_format()[0]
    same = bool(all(np.array_equal(full[k][:Sh], host[k]) for k in KEYS))
    exp_diff = rel_diff(ex, hex_)
    edges = float(np.diagonal(full["overlap"], axis1=1, axis2=2).mean())
    eng.close()

    Ls, Ns, Ss = (2, 60, 8) if a.small else (2, a.host_n, 32)
    gs = (np.arange(Ns) % C).astype(np.int32)
    eng = make_engine(Ls, Ns, M, K, 2)
    dev, t_dev = timed(lambda: eng.sample_mixing(seed, Ss, groups=gs, C=C), a.repeats)
    hst, t_hst = timed(lambda: host_route(eng, seed, Ss, gs, C), a.repeats)
    same_small = bool(all(np.array_equal(dev[k], hst[k]) for k in KEYS))
    eng.close()
    med = lambda t: float(np.median(t))
    out = {"case": "small" if a.small else "config3", "L": L, "N": N, "M": M, "K": K, "S": S, "C": C, "format": fmt, "repeats": a.repeats,
           "mean_edges_per_layer": edges, "chunk_bytes_per_sample": L * N * N + (2 * C * C * L + L * L) * 8,
           "sample_mixing_median_ms": med(t_full), "sample_mixing_all_ms": t_full,
           "sample_overlap_median_ms": med(t_ov), "sample_overlap_all_ms": t_ov,
           "sample_stats_median_ms": med(t_dyads), "sample_stats_all_ms": t_dyads,
           "expected_mixing_median_ms": med(t_exp), "expected_mixing_all_ms": t_exp,
           "host_samples": Sh, "host_sample_median_ms": med(t_host), "host_sample_all_ms": t_host,
           "host_sample_scaled_ms": med(t_host) * S / Sh, "host_over_device": med(t_host) * S / Sh / med(t_full),
           "host_expected_median_ms": med(t_hex), "host_expected_all_ms": t_hex, "host_expected_over_device": med(t_hex) / med(t_exp),
           "expected_max_rel_diff": exp_diff,
           "small_shape": [Ls, Ns, Ns], "small_samples": Ss, "small_device_median_ms": med(t_dev), "small_device_all_ms": t_dev,
           "small_host_median_ms": med(t_hst), "small_host_all_ms": t_hst, "small_host_over_device": med(t_hst) / med(t_dev),
           "call_note": "whole calls are timed: allocations, the draw of the samples, the kernels, the copies back and the synchronisation",
           "same_counts": same and same_small}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)
    assert same and same_small, "the device and the host disagree"
    assert exp_diff < 1e-10, "the expectations disagree"


if __name__ == "__main__":
    main()
