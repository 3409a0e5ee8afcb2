#!/usr/bin/env python
"""Time the posterior betweenness centrality (vmr_sample_betweenness, vmr_network_betweenness) on one GPU at two shapes:
  config3   BASELINE config 3's shape (L = 4, N = 2000, K = 2) and density (a state whose rho gives every node about `--degree` = 5
            ties), S = 256 samples
  small     L = 1, N = 500, S = 32, the same mean degree
and per shape:
  sample_betweenness_<direction>  `eng.sample_betweenness(seed, S, direction)`: the draw, the bit packing, Brandes' algorithm from
                                  every source, the fold over the source blocks, the ranks, the fold into the per-node sums and
                                  the copies back; with values=True also the S L N values
  network_betweenness             `eng.network_betweenness(Y)` of one network [L, N, N] from the host: the upload, the packing, the
                                  same kernels
  sample_connectivity / sample_centrality   of the same engine, for scale: the same draw and packing with their own reductions
  host                            the route it replaces: `eng.sample(seed + s)` over PCIe plus `networkx.betweenness_centrality(
                                  normalized=False)` per layer (scipy.sparse by levels when networkx is absent; `host.library` says
                                  which), direction directed, on `host.samples` samples, SCALED to S (host.scaled_ms)
Whole calls are timed -- allocations, the draw, the kernels, the copies back and the synchronisation -- in `--blocks` blocks of
`--repeats` calls after a warm-up call; the median over all calls, the spread (min, max) and every block's median are recorded.
The device's values agree with the host's within 10 N 2^-53 relative (asserted).
Also recorded: the bytes of the row reads computed from the shapes (three reads of every reached row per source: an upper bound).
Writes profiles/betweenness_bench.json and prints it.
Usage: python tools/bench_betweenness.py [--repeats 2] [--blocks 2] [--degree 5] [--small] [--no-host] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_centrality import timed  # noqa: E402
from tools.bench_connectivity import make_engine  # noqa: E402


def levels_betweenness(A):
    """Brandes by levels from all sources at once with scipy.sparse: b [N] of the bool graph A (directed)."""
    from scipy.sparse import csr_matrix
    N = A.shape[0]
    Gs = csr_matrix(A.astype(np.float64))
    GsT = Gs.T.tocsr()
    D = np.full((N, N), -1, np.int32)
    D[np.arange(N), np.arange(N)] = 0
    sigma, deepest = np.eye(N), 0
    for lvl in range(1, N):
        paths = (GsT @ np.where(D == lvl - 1, sigma, 0.0).T).T
        new = (paths > 0) & (D < 0)
        if not new.any():
            break
        D[new], sigma[new], deepest = lvl, paths[new], lvl
    delta = np.zeros((N, N))
    with np.errstate(divide="ignore", invalid="ignore"):
        for lvl in range(deepest - 1, 0, -1):
            acc = (Gs @ np.where(D == lvl + 1, (1.0 + delta) / sigma, 0.0).T).T
            here = D == lvl
            delta[here] = sigma[here] * acc[here]
    return delta.sum(axis=0)


def host_route(eng, seed, S):
    """The samples over PCIe, then per sample and layer the library's betweenness; (values [S, L, N], the library's name)."""
    try:
        import networkx as nx
    except ImportError:
        nx = None
    L, N = eng.L, eng.N
    values = np.zeros((S, L, N))
    for s in range(S):
        Y = eng.sample(seed + s)
        for l in range(L):
            A = Y[l] > 0
            A[np.arange(N), np.arange(N)] = False
            if nx is None:
                values[s, l] = levels_betweenness(A)
            else:
                b = nx.betweenness_centrality(nx.from_numpy_array(A.astype(np.uint8), create_using=nx.DiGraph), normalized=False)
                values[s, l] = [b[v] for v in range(N)]
    return values, "scipy.sparse" if nx is None else "networkx " + nx.__version__


def shape_run(name, L, N, M, K, S, a, host_samples, seed=17, top_k=10):
    from vimure_amd import _lib
    eng = make_engine(L, N, M, K, 1 if name == "config3" else 2, a.degree)
    W = (N + 63) // 64
    nblk = (N + 15) // 16
    kpt = (N + 255) // 256
    kpt = 1 if kpt <= 1 else 2 if kpt <= 2 else 4 if kpt <= 4 else 8
    out = {"shape": [L, N, N], "K": K, "S": S, "top_k": top_k, "format": eng.data_format()[0],
           "workgroups_per_call": nblk * L * S, "sources_per_workgroup": 16, "lds_bytes_per_workgroup": 16 * N + 136 * W + 512 * kpt + 256,
           "row_bytes_per_call_at_most": {"directed": 3 * 8 * N * W * N * L * S, "union": 6 * 8 * N * W * N * L * S},
           "share_bytes_per_call": 2 * 8 * N * nblk * L * S, "pack_bytes_per_call": (N * N + 16 * N * W) * L * S}
    for d in _lib.BTW_DIRECTIONS:
        _, out["sample_betweenness_" + d] = timed(lambda: eng.sample_betweenness(seed, S, direction=d, top_k=top_k), a.repeats, a.blocks)
    dev, out["sample_betweenness_directed_values"] = timed(lambda: eng.sample_betweenness(seed, S, top_k=top_k, values=True), a.repeats, a.blocks)
    out["mean_total"] = float(dev["total"].mean())
    Y0 = eng.sample(seed)
    net, out["network_betweenness"] = timed(lambda: eng.network_betweenness(Y0), a.repeats, a.blocks)
    ok = bool(np.array_equal(net, dev["values"][0]))
    out["network_equals_sample_values"] = ok
    _, out["sample_connectivity"] = timed(lambda: eng.sample_connectivity(seed, S), a.repeats, a.blocks)
    _, out["sample_centrality"] = timed(lambda: eng.sample_centrality(seed, S, 1.0 / a.degree, 8), a.repeats, a.blocks)
    if not a.no_host:
        Sh = min(S, host_samples)
        (host, library), t = timed(lambda: host_route(eng, seed, Sh), 1, 1, warm=False)
        med = out["sample_betweenness_directed"]["median_ms"]
        agrees = bool(np.all(np.abs(dev["values"][:Sh] - host) <= 10 * N * 2.0 ** -53 * host))
        out["host"] = dict(t, library=library, samples=Sh, scaled_ms=t["median_ms"] * S / Sh, scaled_over_device=t["median_ms"] * S / Sh / med,
                           agrees=agrees, note="the host route ran once on `samples` samples; scaled_ms is its time times S / samples")
        ok = ok and agrees
    eng.close()
    return out, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=2, help="calls per block")
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--degree", type=float, default=5.0, help="mean out-degree of a sampled network")
    ap.add_argument("--host-n", type=int, default=500)
    ap.add_argument("--samples", type=int, default=32, help="samples of the small network")
    ap.add_argument("--host-samples", type=int, default=4, help="samples the host route takes at the small shape (its time is scaled to S)")
    ap.add_argument("--host-samples-large", type=int, default=1, help="samples the host route takes at the large shape (its time is scaled to S)")
    ap.add_argument("--no-host", action="store_true", help="leave the host route out (a run under a profiler)")
    ap.add_argument("--small", action="store_true", help="L = 2, N = 200 and N = 60: a rehearsal of the script, not a measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "betweenness_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_betweenness.py measures on a GPU; none is visible: the numbers stay unmeasured")
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
