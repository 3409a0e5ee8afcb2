#!/usr/bin/env python
"""Time the posterior triad census (vmr_sample_triad_census, vmr_network_triad_census) on one GPU at two shapes:
  config3   BASELINE config 3's shape (L = 4, N = 2000, K = 2) and density (a state whose rho gives every node about `--degree` = 5
            ties), S = 256 samples
  small     L = 1, N = 500, S = 32, the same mean degree
and per shape:
  sample_triad_census    `eng.sample_triad_census(seed, S)`: the draw, the bit packing, the count and the copy back
  network_triad_census   `eng.network_triad_census(Y)` of one network [L, N, N] from the host: the upload, the packing, the same kernel
  sample_triads / sample_stats   of the same engine, for scale: the same draw (and packing) with their own reductions
  host                   the route it replaces: `eng.sample(seed + s)` over PCIe plus `networkx.triadic_census` per layer (the
                         all-triples count of tests/census_util.py when networkx is absent; `host.library` says which), on
                         `host.samples` samples, SCALED to S (host.scaled_ms)
Whole calls are timed -- allocations, the draw, the kernels, the copies back and the synchronisation -- in `--blocks` blocks of
`--repeats` calls after a warm-up call; the median over all calls, the spread (min, max) and every block's median are recorded.
The device's counts equal the host's (asserted).
Also recorded: the row words the count reads, computed from the samples' ties (two rows of W words per connected pair, both
bitsets), beside the bytes the draw writes and the packing reads.
Writes profiles/census_bench.json and prints it.
Usage: python tools/bench_census.py [--repeats 3] [--blocks 2] [--degree 5] [--small] [--no-host] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_centrality import timed  # noqa: E402
from tools.bench_connectivity import make_engine  # noqa: E402


def host_route(eng, seed, S):
    """The samples over PCIe, then per sample and layer the library's census; (counts [S, L, 16], the library's name)."""
    from vimure_amd.census import CLASS_NAMES
    try:
        import networkx as nx
    except ImportError:
        nx = None
        from tests.census_util import census_one
    L, N = eng.L, eng.N
    counts = np.zeros((S, L, 16), np.int64)
    for s in range(S):
        Y = eng.sample(seed + s)
        for l in range(L):
            A = Y[l] > 0
            A[np.arange(N), np.arange(N)] = False
            if nx is None:
                counts[s, l] = census_one(A)
            else:
                c = nx.triadic_census(nx.from_numpy_array(A.astype(np.uint8), create_using=nx.DiGraph))
                counts[s, l] = [c[k] for k in CLASS_NAMES]
    return counts, "numpy" if nx is None else "networkx " + nx.__version__


def shape_run(name, L, N, M, K, S, a, host_samples, seed=17):
    eng = make_engine(L, N, M, K, 1 if name == "config3" else 2, a.degree)
    W = (N + 63) // 64
    out = {"shape": [L, N, N], "K": K, "S": S, "format": eng.data_format()[0], "waves_per_call": N * L * S,
           "lds_bytes_per_workgroup": 4 * 2048 * 2 + 16 * 8, "pack_bytes_per_call": (N * N + 16 * N * W) * L * S}
    dev, out["sample_triad_census"] = timed(lambda: eng.sample_triad_census(seed, S), a.repeats, a.blocks)
    from vimure_amd.census import dyads_of
    m, asym, _ = dyads_of(dev, N)      # the connected pairs follow from the census
    out["connected_pairs_per_call"] = int((m + asym).sum())
    in_registers = W <= 64 and W & (W - 1) == 0      # row i's words stay in registers: only row j is read per connected pair
    out["count_row_bytes_per_call"] = int((m + asym).sum()) * (2 if in_registers else 4) * W * 8      # both bitsets
    out["mean_census"] = dev.mean(axis=(0, 1)).tolist()
    Y0 = eng.sample(seed)
    net, out["network_triad_census"] = timed(lambda: eng.network_triad_census(Y0), a.repeats, a.blocks)
    ok = bool(np.array_equal(net, dev[0]))
    out["network_equals_sample"] = ok
    _, out["sample_triads"] = timed(lambda: eng.sample_triads(seed, S), a.repeats, a.blocks)
    _, out["sample_stats"] = timed(lambda: eng.sample_stats(seed, S), a.repeats, a.blocks)
    if not a.no_host:
        Sh = min(S, host_samples)
        (host, library), t = timed(lambda: host_route(eng, seed, Sh), 1, 1, warm=False)
        med = out["sample_triad_census"]["median_ms"]
        agrees = bool(np.array_equal(dev[:Sh], host))
        out["host"] = dict(t, library=library, samples=Sh, scaled_ms=t["median_ms"] * S / Sh, scaled_over_device=t["median_ms"] * S / Sh / med,
                           agrees=agrees, note="the host route ran once on `samples` samples; scaled_ms is its time times S / samples")
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "census_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_census.py measures on a GPU; none is visible: the numbers stay unmeasured")
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
