#!/usr/bin/env python
"""Time the shared partners of the posterior's ties (vmr_sample_shared_partners, vmr_network_shared_partners) on one GPU at two
shapes:
  config3   BASELINE config 3's shape (L = 4, N = 2000, K = 2) and density (a state whose rho gives every node about `--degree` = 5
            ties), S = 256 samples
  small     L = 1, N = 500, S = 32, the same mean degree
and per shape:
  sample_shared_partners[mode]   `eng.sample_shared_partners(seed, S, mode=mode, nodes=True)` in the three modes: the draw, the bit
                         packing, the count and the copy back
  with_pairs             the union call with the ties of the first sample listed as pairs
  network_shared_partners   `eng.network_shared_partners(Y, nodes=True)` of one network [L, N, N] from the host: the upload, the
                         packing, the same kernels
  sample_triad_census    of the same engine, for scale: the same draw and packing with its own count
  host                   the route it replaces: `eng.sample(seed + s)` over PCIe plus `scipy.sparse` products per layer
                         ((P @ Q.T) o T, histogram, totals, node sums), on `host.samples` samples after one sample to warm
                         up, SCALED to S (host.scaled_ms)
Whole calls are timed -- allocations, the draw, the kernels, the copies back and the synchronisation -- in `--blocks` blocks of
`--repeats` calls after a warm-up call; the median over all calls, the spread (min, max) and every block's median are recorded.
The device's counts equal the host's (asserted).
Writes profiles/partners_bench.json and prints it.
Usage: python tools/bench_partners.py [--repeats 3] [--blocks 2] [--degree 5] [--small] [--no-host] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_centrality import timed  # noqa: E402
from tools.bench_connectivity import make_engine  # noqa: E402

MODES = ("union", "mutual", "path")
KEYS = ("hist", "totals", "node_ties", "node_supported")


def host_route(eng, seed, S, mode, n_bins):
    """The samples over PCIe, then per sample and layer the counts by scipy.sparse products; the dict of the device call."""
    from scipy.sparse import csr_matrix, triu
    L, N = eng.L, eng.N
    out = {"hist": np.zeros((S, L, n_bins), np.int64), "totals": np.zeros((S, L, 4), np.int64), "node_ties": np.zeros((S, L, N), np.int32),
           "node_supported": np.zeros((S, L, N), np.int32)}
    for s in range(S):
        Y = eng.sample(seed + s)
        for l in range(L):
            B = Y[l] > 0
            B[np.arange(N), np.arange(N)] = False
            A = csr_matrix(B.astype(np.int64))
            At = A.T.tocsr()
            if mode == "path":
                P, Q, T = A, At, A
            else:
                P = ((A + At) > 0).astype(np.int64) if mode == "union" else A.multiply(At).tocsr()
                Q, T = P, triu(P, 1).tocsr()
            C = (P @ Q.T).multiply(T).tocsr()                      # partners of the ties that have any
            c = C.data[C.data > 0]
            ties = T.nnz
            h = np.bincount(np.minimum(c, n_bins - 1), minlength=n_bins)
            h[0] += ties - c.size
            Sup = (C > 0).astype(np.int64)
            out["hist"][s, l] = h
            out["totals"][s, l] = [ties, c.size, c.sum(), c.max() if c.size else 0]
            out["node_ties"][s, l] = np.asarray(T.sum(axis=1)).ravel() + np.asarray(T.sum(axis=0)).ravel()
            out["node_supported"][s, l] = np.asarray(Sup.sum(axis=1)).ravel() + np.asarray(Sup.sum(axis=0)).ravel()
    return out


def same(a, b, S=None):
    return all(np.array_equal(a[k][:S], b[k][:S]) for k in KEYS)


def shape_run(name, L, N, M, K, S, a, host_samples, seed=17, n_bins=64):
    eng = make_engine(L, N, M, K, 1 if name == "config3" else 2, a.degree)
    W = (N + 63) // 64
    out = {"shape": [L, N, N], "K": K, "S": S, "n_bins": n_bins, "format": eng.data_format()[0], "waves_per_call": N * L * S,
           "lds_bytes_per_workgroup": 4 * 2048 * 2 + 4 * 1024 + 32, "pack_bytes_per_call": (N * N + 16 * N * W) * L * S}
    dev = {}
    for mode in MODES:
        dev[mode], out["sample_shared_partners[%s]" % mode] = timed(lambda: eng.sample_shared_partners(seed, S, mode=mode, n_bins=n_bins, nodes=True),
                                                                    a.repeats, a.blocks)
        t = dev[mode]["totals"].sum(axis=(0, 1))
        out["totals[%s]" % mode] = dict(zip(("ties", "supported", "partners"), (int(x) for x in t[:3])), max_partners=int(dev[mode]["totals"][..., 3].max()))
    Y0 = eng.sample(seed)
    pairs = np.argwhere(np.triu((Y0 > 0) | (Y0 > 0).transpose(0, 2, 1), 1)).astype(np.int32)
    out["n_pairs"] = len(pairs)
    wp, out["with_pairs"] = timed(lambda: eng.sample_shared_partners(seed, S, mode="union", n_bins=n_bins, nodes=True, pairs=pairs), a.repeats, a.blocks)
    ok = same(wp, dev["union"]) and bool((wp["pair_present"] >= 1).all())
    net, out["network_shared_partners"] = timed(lambda: eng.network_shared_partners(Y0, mode="union", n_bins=n_bins, nodes=True, pairs=pairs), a.repeats,
                                                a.blocks)
    ok = ok and all(np.array_equal(net[k], dev["union"][k][0]) for k in KEYS) and bool((net["pair_partners"] >= 0).all())
    out["network_equals_sample"] = ok
    _, out["sample_triad_census"] = timed(lambda: eng.sample_triad_census(seed, S), a.repeats, a.blocks)
    if not a.no_host:
        Sh = min(S, host_samples)
        out["host"] = {}
        host_route(eng, seed, 1, "union", n_bins)      # (scipy.sparse's import and first products are not the route's cost)
        for mode in MODES:
            host, t = timed(lambda: host_route(eng, seed, Sh, mode, n_bins), 1, 1, warm=False)
            med = out["sample_shared_partners[%s]" % mode]["median_ms"]
            agrees = same(dev[mode], host, Sh)
            out["host"][mode] = dict(t, library="scipy.sparse", samples=Sh, scaled_ms=t["median_ms"] * S / Sh,
                                     scaled_over_device=t["median_ms"] * S / Sh / med, agrees=agrees,
                                     note="the host route ran once on `samples` samples; scaled_ms is its time times S / samples")
            ok = ok and agrees
    eng.close()
    return out, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3, help="calls per block")
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--degree", type=float, default=5.0, help="mean out-degree of a sampled network")
    ap.add_argument("--host-n", type=int, default=500)
    ap.add_argument("--samples", type=int, default=32, help="samples of the small network")
    ap.add_argument("--host-samples", type=int, default=8, help="samples the host route takes at the small shape (its time is scaled to S)")
    ap.add_argument("--host-samples-large", type=int, default=2, help="samples the host route takes at the large shape (its time is scaled to S)")
    ap.add_argument("--no-host", action="store_true", help="leave the host route out (a run under a profiler)")
    ap.add_argument("--small", action="store_true", help="L = 2, N = 200 and N = 60: a rehearsal of the script, not a measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "partners_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_partners.py measures on a GPU; none is visible: the numbers stay unmeasured")
    big = (2, 200, 40, 2, 16) if a.small else (4, 2000, 200, 2, 256)
    small = (1, 60, 40, 2, 8) if a.small else (1, a.host_n, 200, 2, a.samples)
    out = {"case": "rehearsal" if a.small else "config3", "repeats": a.repeats, "blocks": a.blocks, "degree": a.degree,
           "call_note": "whole calls are timed: allocations, the draw of the samples, the kernels, the copies back and the synchronisation"}
    out["small"], ok2 = shape_run("small", *small, a, a.host_samples)
    print(json.dumps({"small": out["small"]}), flush=True)
    out["config3"], ok1 = shape_run("config3", *big, a, a.host_samples_large)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)
    assert ok1 and ok2, "the device and the host disagree"


if __name__ == "__main__":
    main()
