#!/usr/bin/env python
"""Time the posterior cut points (vmr_sample_cutpoints, vmr_network_cutpoints) on one GPU at two shapes:
  config3   BASELINE config 3's shape (L = 4, N = 2000, K = 2) and density (a state whose rho gives every node about `--degree` = 5
            ties), S = 256 samples
  small     L = 1, N = 500, S = 32, the same mean degree
and per shape, in both modes:
  sample_cutpoints_<mode>   `eng.sample_cutpoints(seed, S, mode)`: the draw, the bit packing, the graph's bits, the removal
                            experiments, the ranks and the summary, the two folds into the per-node sums and the copies back;
                            for union with values=True also the S L N values
  network_cutpoints         `eng.network_cutpoints(Y)` of one network [L, N, N] from the host: the upload, the packing, the same
                            kernels
  sample_connectivity / sample_stats   of the same engine, for scale: the same draw (and packing) with their own reductions --
                            `sample_connectivity` runs three closures per block of 64 nodes where this call runs about one,
                            plus its rounds
  rounds_per_block_<mode>   the rounds that seed in a block of 64 removal experiments = the largest number of branches among
                            the block's nodes, from the values the device returns: mean and max over the blocks
  host                      the route it replaces: `eng.sample(seed + s)` over PCIe plus `networkx.articulation_points`,
                            `networkx.bridges` and one component search per removed cut point (a node that is no cut point
                            cuts no pair: the search is spared), mode union, on `host.samples` samples, SCALED to S
                            (host.scaled_ms).  Without networkx the restatement of tests/cutpoints_util.py takes its place;
                            `host.library` says which
Whole calls are timed -- allocations, the draw, the kernels, the copies back and the synchronisation -- in `--blocks` blocks of
`--repeats` calls after a warm-up call; the median over all calls, the spread (min, max) and every block's median are recorded.
The device's values equal the host's (asserted).
Writes profiles/cutpoints_bench.json and prints it.
Usage: python tools/bench_cutpoints.py [--repeats 3] [--blocks 2] [--degree 5] [--small] [--no-host] [--out FILE]"""
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
    """The samples over PCIe, then per sample and layer the library's cut points and bridges of the undirected graph and, per cut
    point, the component sizes without it; (pairs_cut, is_cut, bridges [S, L, N], the library's name)."""
    try:
        import networkx as nx
    except ImportError:
        nx = None
        from tests.cutpoints_util import cut_values
    L, N = eng.L, eng.N
    pairs, cut, bridges = (np.zeros((S, L, N), np.int64) for _ in range(3))
    for s in range(S):
        Y = eng.sample(seed + s)
        for l in range(L):
            A = Y[l] > 0
            A[np.arange(N), np.arange(N)] = False
            if nx is None:
                p, b, g = cut_values(A | A.T)
                pairs[s, l], cut[s, l], bridges[s, l] = p, b >= 2, g
                continue
            G = nx.from_numpy_array((A | A.T).astype(np.uint8))
            for u, v in nx.bridges(G):
                bridges[s, l, u] += 1
                bridges[s, l, v] += 1
            size = {}
            for c in nx.connected_components(G):
                for v in c:
                    size[v] = len(c)
            for v in nx.articulation_points(G):
                cut[s, l, v] = 1
                H = G.subgraph(nx.node_connected_component(G, v) - {v})
                sz = np.asarray([len(c) for c in nx.connected_components(H)], np.int64)
                assert sz.sum() == size[v] - 1
                pairs[s, l, v] = (sz.sum() ** 2 - (sz * sz).sum()) // 2
    return (pairs, cut, bridges), "numpy" if nx is None else "networkx " + nx.__version__


def rounds_per_block(branches):
    """{"mean", "max"} over the (sample, layer, block of 64 nodes) of the largest number of branches in the block."""
    S, L, N = branches.shape
    W = (N + 63) // 64
    b = np.zeros((S, L, W * 64), np.int64)
    b[..., :N] = branches
    r = b.reshape(S, L, W, 64).max(axis=-1)
    return {"mean": float(r.mean()), "max": int(r.max())}


def shape_run(name, L, N, M, K, S, a, host_samples, seed=17, top_k=10):
    from vimure_amd import _lib
    eng = make_engine(L, N, M, K, 1 if name == "config3" else 2, a.degree)
    W = (N + 63) // 64
    out = {"shape": [L, N, N], "K": K, "S": S, "top_k": top_k, "format": eng.data_format()[0],
           "workgroups_per_call": W * L * S, "lds_bytes_per_workgroup": 24 * 64 * W + 768,
           "graph_bytes_per_call": 24 * N * W * L * S, "pack_bytes_per_call": (N * N + 16 * N * W) * L * S}
    res = {}
    for m in _lib.CUT_MODES:
        res[m], out["sample_cutpoints_" + m] = timed(lambda: eng.sample_cutpoints(seed, S, mode=m, top_k=top_k), a.repeats, a.blocks)
        for k in _lib.CUT_SUMMARY:
            out["mean_%s_%s" % (k, m)] = float(res[m][k].mean())
        vals = eng.sample_cutpoints(seed, min(S, 8), mode=m, top_k=top_k, values=True)
        out["rounds_per_block_" + m] = rounds_per_block(vals["branches"])
    dev, out["sample_cutpoints_union_values"] = timed(lambda: eng.sample_cutpoints(seed, S, top_k=top_k, values=True), a.repeats, a.blocks)
    Y0 = eng.sample(seed)
    net, out["network_cutpoints"] = timed(lambda: eng.network_cutpoints(Y0), a.repeats, a.blocks)
    ok = all(bool(np.array_equal(net[k], dev[k][0])) for k in ("pairs_cut", "branches", "bridges"))
    out["network_equals_sample_values"] = ok
    _, out["sample_connectivity"] = timed(lambda: eng.sample_connectivity(seed, S), a.repeats, a.blocks)
    _, out["sample_stats"] = timed(lambda: eng.sample_stats(seed, S), a.repeats, a.blocks)
    out["over_sample_connectivity"] = {m: out["sample_cutpoints_" + m]["median_ms"] / out["sample_connectivity"]["median_ms"]
                                       for m in _lib.CUT_MODES}
    if not a.no_host:
        Sh = min(S, host_samples)
        ((hp, hc, hb), library), t = timed(lambda: host_route(eng, seed, Sh), 1, 1, warm=False)
        med = out["sample_cutpoints_union"]["median_ms"]
        agrees = bool(np.array_equal(dev["pairs_cut"][:Sh], hp) and np.array_equal(dev["branches"][:Sh] >= 2, hc > 0) and
                      np.array_equal(dev["bridges"][:Sh], hb))
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
    ap.add_argument("--host-samples-large", type=int, default=1, help="samples the host route takes at the large shape (its time is scaled to S)")
    ap.add_argument("--no-host", action="store_true", help="leave the host route out (a run under a profiler)")
    ap.add_argument("--small", action="store_true", help="L = 2, N = 200 and N = 60: a rehearsal of the script, not a measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cutpoints_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_cutpoints.py measures on a GPU; none is visible: the numbers stay unmeasured")
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
