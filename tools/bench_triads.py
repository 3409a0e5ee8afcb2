#!/usr/bin/env python3
"""Time the posterior triad statistics (vmr_sample_triads, vmr_expected_triads) at BASELINE config 3's shape (L = 4, N = 2000,
M = 200, K = 2, report lists) from a random state (the numbers do not depend on the fit), whole calls:
  sample_triads_ms     `eng.sample_triads(seed, S, nodes=True)`, S = 256: the draw, the bit packing, the AND + popcount reduction
  sample_triads_plain_ms   the same without the per-node arrays
  expected_triads_ms   `eng.expected_triads()`: P and U written once, the three fused tile products, the fixed tree
and, at a small shape (--host-n, default L = 1, N = 500),
  device_ms            `eng.sample_triads(seed, S_host, nodes=True)` there
  host_ms              the route that exists without it: S_host calls of `eng.sample(seed + s)` (L N^2 bytes over PCIe each) plus
                       NumPy matrix products -- in float64 through BLAS, exact for these counts and much faster than NumPy's integer
                       products, so the host is shown at its best
  device_expected_ms / host_expected_ms   `eng.expected_triads()` against `eng.get_state()["rho"]` plus NumPy
Each route is warmed up once and timed around a device synchronise; the median and all repeats are kept.  Asserts that the device
and the host give the same counts and expectations within 1e-10.  Writes profiles/triads_bench.json and prints it.
Usage: python tools/bench_triads.py [--repeats 3] [--small] [--host-n 500] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS = ("transitive", "cyclic", "two_paths", "triangles_u", "wedges_u", "edges_u")


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


def host_route(eng, seed, S):
    out = {k: np.zeros((S, eng.L), np.int64) for k in KEYS}
    out["node_tri"], out["node_deg"] = np.zeros((S, eng.L, eng.N), np.int32), np.zeros((S, eng.L, eng.N), np.int32)
    for s in range(S):
        Y = eng.sample(seed + s)
        for l in range(eng.L):
            A = (Y[l] > 0).astype(np.float64)
            np.fill_diagonal(A, 0.0)
            U = np.maximum(A, A.T)
            AA, d = A @ A, U.sum(axis=1)
            u3 = np.einsum("ij,ji->i", U @ U, U)
            vals = (((A @ A.T) * A).sum(), (AA * A.T).sum(), AA.sum() - np.trace(AA), u3.sum() / 6.0, (d * (d - 1.0) / 2.0).sum(),
                    U.sum() / 2.0)
            for k, v in zip(KEYS, vals):
                out[k][s, l] = int(round(v))
            out["node_tri"][s, l], out["node_deg"][s, l] = np.rint(u3 / 2.0), d
    return out


def host_expected(eng):
    rho = eng.get_state()["rho"]
    out = {k: np.zeros(eng.L) for k in KEYS}
    for l in range(eng.L):
        P = rho[l][..., 1:].sum(-1)
        np.fill_diagonal(P, 0.0)
        U = 1.0 - (1.0 - P) * (1.0 - P.T)
        np.fill_diagonal(U, 0.0)
        s = U.sum(axis=1)
        vals = ((P * (P @ P.T)).sum(), ((P @ P) * P.T).sum(), (P.sum(axis=0) * P.sum(axis=1)).sum() - (P * P.T).sum(),
                np.trace(U @ U @ U) / 6.0, ((s * s).sum() - (U * U).sum()) / 2.0, np.triu(U, 1).sum())
        for k, v in zip(KEYS, vals):
            out[k][l] = v
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-n", type=int, default=500)
    ap.add_argument("--host-samples", type=int, default=32)
    ap.add_argument("--small", action="store_true", help="L = 2, N = 200, M = 40 and the host route at N = 60: a rehearsal of the script, not a measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "triads_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_triads.py measures on a GPU; none is visible: the numbers stay unmeasured")
    L, N, M, K = (2, 200, 40, 2) if a.small else (4, 2000, 200, 2)
    S, seed = (16 if a.small else 256), 17
    eng = make_engine(L, N, M, K, 1)
    full, t_full = timed(lambda: eng.sample_triads(seed, S, nodes=True), a.repeats)
    _, t_plain = timed(lambda: eng.sample_triads(seed, S), a.repeats)
    _, t_dyads = timed(lambda: eng.sample_stats(seed, S, degrees=True), a.repeats)
    ex, t_exp = timed(eng.expected_triads, a.repeats)
    fmt = eng.data_format()[0]
    mean_deg = float(full["node_deg"].mean())
    eng.close()

    Lh, Nh, Sh = (1, 60, 8) if a.small else (1, a.host_n, a.host_samples)
    eng = make_engine(Lh, Nh, M, K, 2)
    dev, t_dev = timed(lambda: eng.sample_triads(seed, Sh, nodes=True), a.repeats)
    host, t_host = timed(lambda: host_route(eng, seed, Sh), a.repeats)
    dex, t_dex = timed(eng.expected_triads, a.repeats)
    hex_, t_hex = timed(lambda: host_expected(eng), a.repeats)
    same = bool(all(np.array_equal(dev[k], host[k]) for k in host))
    exp_diff = float(max(np.max(np.abs(dex[k] - hex_[k]) / np.abs(hex_[k])) for k in KEYS))
    eng.close()
    med = lambda t: float(np.median(t))
    W = (N + 63) // 64
    out = {"case": "small" if a.small else "config3", "L": L, "N": N, "M": M, "K": K, "S": S, "format": fmt, "repeats": a.repeats,
           "mean_degree_u": mean_deg, "bitset_bytes_per_sample": 16 * L * N * W,
           "sample_triads_median_ms": med(t_full), "sample_triads_all_ms": t_full,
           "sample_triads_plain_median_ms": med(t_plain), "sample_triads_plain_all_ms": t_plain,
           "sample_stats_median_ms": med(t_dyads), "sample_stats_all_ms": t_dyads,
           "expected_triads_median_ms": med(t_exp), "expected_triads_all_ms": t_exp,
           "expected_flop": 6.0 * L * N ** 3, "expected_gflops": 6.0 * L * N ** 3 / (med(t_exp) * 1e-3) / 1e9,
           "expected": {k: ex[k].tolist() for k in KEYS},
           "host_shape": [Lh, Nh, Nh], "host_samples": Sh, "device_median_ms": med(t_dev), "device_all_ms": t_dev,
           "host_median_ms": med(t_host), "host_all_ms": t_host, "host_over_device": med(t_host) / med(t_dev),
           "device_expected_median_ms": med(t_dex), "device_expected_all_ms": t_dex, "host_expected_median_ms": med(t_hex),
           "host_expected_all_ms": t_hex, "expected_max_rel_diff": exp_diff,
           "call_note": "whole calls are timed: allocations, the draw of the samples, the kernels, the copies back and the synchronisation",
           "same_counts": same}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)
    assert same, "the device and the host disagree"
    assert exp_diff < 1e-10, "the expectations disagree"


if __name__ == "__main__":
    main()
