#!/usr/bin/env python
"""Time the posterior diffusion centrality (vmr_sample_centrality, vmr_mean_centrality) on one GPU at two shapes:
  config3   BASELINE config 3's shape (L = 4, N = 2000, K = 2) and density (a state whose rho gives every node about `--degree` = 5
            ties), S = 256 samples, T = 8, q = 1 / degree
  small     L = 1, N = 500, S = 32, the same mean degree, T and q
and per shape:
  sample_centrality_<direction>   `eng.sample_centrality(seed, S, q, T, direction)`: the draw, the bit packing, the walk, the ranks,
                                  the fold into the per-node sums and the copies back; with values=True also the S L N values
  mean_centrality_out / _in       `eng.mean_centrality(q, T, direction)`: P (and P^T), T matrix-vector steps, the copy back
  sample_connectivity / sample_stats   of the same engine, for scale: the same draw (and packing) with their own reductions
  host                            the route it replaces: `eng.sample(seed + s)` over PCIe plus scipy.sparse matrix-vector products
                                  and the same reductions in NumPy (direction out); at config 3's shape on `--host-samples-large`
                                  samples, SCALED to S (host_scaled_ms)
Whole calls are timed -- allocations, the draw, the kernels, the copies back and the synchronisation -- in `--blocks` blocks of
`--repeats` calls after a warm-up call; the median over all calls, the spread (min, max) and every block's median are recorded.
The device's values agree with the host's within 2 T (N + 1) 2^-53 relative (asserted).
Also recorded: the bytes of the walk kernel computed from the shapes (rows re-read on each step).
Writes profiles/centrality_bench.json and prints it.
Usage: python tools/bench_centrality.py [--repeats 3] [--blocks 3] [--degree 5] [--small] [--no-host] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_connectivity import make_engine  # noqa: E402


def timed(fn, repeats, blocks, warm=True):
    """(last result, {median, min, max, block medians, all}) in ms over blocks x repeats synchronised calls."""
    import torch
    if warm:
        fn()      # warm-up: code objects, allocator
    out, per_block = None, []
    for _ in range(blocks):
        ts = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        per_block.append(ts)
    flat = [t for b in per_block for t in b]
    return out, {"median_ms": float(np.median(flat)), "min_ms": float(min(flat)), "max_ms": float(max(flat)),
                 "block_medians_ms": [float(np.median(b)) for b in per_block], "all_ms": flat}


def host_route(eng, seed, S, q, T, top_k):
    """The samples over PCIe, then per sample and layer T sparse matrix-vector products and the reductions of the device call."""
    from scipy.sparse import csr_matrix
    L, N = eng.L, eng.N
    values = np.zeros((S, L, N))
    for s in range(S):
        Y = eng.sample(seed + s)
        for l in range(L):
            A = Y[l] > 0
            A[np.arange(N), np.arange(N)] = False
            M = csr_matrix(A.astype(np.float64))
            x, c = np.ones(N), np.zeros(N)
            for _ in range(T):
                x = q * (M @ x)
                c += x
            values[s, l] = c
    out = {"values": values, "node_sum": values.sum(axis=0), "node_sumsq": (values * values).sum(axis=0)}
    order = np.sort(values, axis=-1)
    rank = np.stack([[N - np.searchsorted(order[s, l], values[s, l], side="right") for l in range(L)] for s in range(S)])
    out["node_rank_sum"], out["node_top"] = rank.sum(axis=0), (rank < top_k).sum(axis=0)
    return out


def agree(dev, host, S, T, N):
    """the values of the first S samples (the ranks of nodes whose values differ in the last bits may differ, so they are not held)"""
    v, w = dev["values"][:S], host["values"]
    return bool(np.all(np.abs(v - w) <= 2 * T * (N + 1) * 2.0 ** -53 * w))


def shape_run(name, L, N, M, K, S, T, a, host_samples, seed=17, top_k=10):
    from vimure_amd import _lib
    eng = make_engine(L, N, M, K, 1 if name == "config3" else 2, a.degree)
    q = 1.0 / a.degree
    W = (N + 63) // 64
    out = {"shape": [L, N, N], "K": K, "S": S, "T": T, "q": q, "top_k": top_k, "format": eng.data_format()[0],
           "workgroups_per_call": L * S, "lds_bytes_per_workgroup": 16 * 64 * W,
           "walk_row_bytes_per_call": {"out": 8 * N * W * T * L * S, "union": 16 * N * W * T * L * S},
           "walk_store_bytes_per_call": (12 * N + 16) * L * S, "pack_bytes_per_call": (N * N + 16 * N * W) * L * S}
    dev = None
    for d in _lib.CENT_DIRECTIONS:
        r, t = timed(lambda: eng.sample_centrality(seed, S, q, T, direction=d, top_k=top_k), a.repeats, a.blocks)
        out["sample_centrality_" + d] = t
    dev, out["sample_centrality_out_values"] = timed(lambda: eng.sample_centrality(seed, S, q, T, top_k=top_k, values=True), a.repeats, a.blocks)
    out["mean_centrality_total"] = float(dev["total"].mean())
    for d in ("out", "in"):
        _, out["mean_centrality_" + d] = timed(lambda: eng.mean_centrality(q, T, direction=d), a.repeats, a.blocks)
    _, out["sample_connectivity"] = timed(lambda: eng.sample_connectivity(seed, S), a.repeats, a.blocks)
    _, out["sample_stats"] = timed(lambda: eng.sample_stats(seed, S), a.repeats, a.blocks)
    ok = True
    if not a.no_host:
        Sh = min(S, host_samples)
        full = Sh == S
        host, t = timed(lambda: host_route(eng, seed, Sh, q, T, top_k), a.repeats if full else 1, a.blocks if full else 1, warm=full)
        med = out["sample_centrality_out"]["median_ms"]
        out["host"] = dict(t, samples=Sh, scaled_ms=t["median_ms"] * S / Sh, scaled_over_device=t["median_ms"] * S / Sh / med,
                           note="the host route on `samples` samples; scaled_ms is its median times S / samples")
        ok = out["host"]["agrees"] = agree(dev, host, Sh, T, N)
    eng.close()
    return out, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3, help="calls per block")
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--degree", type=float, default=5.0, help="mean out-degree of a sampled network")
    ap.add_argument("--host-n", type=int, default=500)
    ap.add_argument("--host-samples", type=int, default=32, help="samples of the small network, all of which the host route takes")
    ap.add_argument("--host-samples-large", type=int, default=4, help="samples the host route takes at the large shape (its time is scaled to S)")
    ap.add_argument("--no-host", action="store_true", help="leave the host route out (a run under a profiler)")
    ap.add_argument("--small", action="store_true", help="L = 2, N = 200 and N = 60: a rehearsal of the script, not a measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "centrality_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_centrality.py measures on a GPU; none is visible: the numbers stay unmeasured")
    T = 8
    big = (2, 200, 40, 2, 16) if a.small else (4, 2000, 200, 2, 256)
    small = (1, 60, 40, 2, 8) if a.small else (1, a.host_n, 200, 2, a.host_samples)
    out = {"case": "rehearsal" if a.small else "config3", "repeats": a.repeats, "blocks": a.blocks, "degree": a.degree,
           "call_note": "whole calls are timed: allocations, the draw of the samples, the kernels, the copies back and the synchronisation"}
    out["config3"], ok1 = shape_run("config3", *big, T, a, a.host_samples_large)
    out["small"], ok2 = shape_run("small", *small, T, a, small[4])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)
    assert ok1 and ok2, "the device and the host disagree"


if __name__ == "__main__":
    main()
