#!/usr/bin/env python
"""Time Burt's structural holes of the posterior (vmr_sample_structural_holes, vmr_network_structural_holes) on one GPU at two
shapes:
  config3   BASELINE config 3's shape (L = 4, N = 2000, K = 2) and density (a state whose rho gives every node about `--degree` = 5
            ties), S = 256 samples
  small     L = 1, N = 500, S = 32, the same mean degree
and per shape:
  sample_structural_holes[mode]   `eng.sample_structural_holes(seed, S, mode=mode)` in both modes: the draw, the bit packing, the
                         strengths, the node walk, the ranks, the folds and the copy back
  with_values            the union call with values=True: five more [S, L, N] arrays cross PCIe
  network_structural_holes   `eng.network_structural_holes(Y, summary=True)` of one network [L, N, N] from the host: the upload,
                         the packing, the same kernels
  sample_shared_partners of the same engine (union, nodes=True), for scale: the same draw and packing with its own walk
  host                   the route it replaces: `eng.sample(seed + s)` over PCIe plus `networkx.constraint` and
                         `networkx.effective_size` per layer, on `host.samples` samples and the first `host.layers` layers
                         after one small graph to warm up, SCALED to S samples and L layers (host.scaled_ms)
Whole calls are timed -- allocations, the draw, the kernels, the copies back and the synchronisation -- in `--blocks` blocks of
`--repeats` calls after a warm-up call; the median over all calls, the spread (min, max) and every block's median are recorded.
The device's values agree with networkx's to 1e-12 relative on the nodes networkx defines (asserted).
Writes profiles/holes_bench.json and prints it.
Usage: python tools/bench_holes.py [--repeats 3] [--blocks 2] [--degree 5] [--small] [--no-host] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_centrality import timed  # noqa: E402
from tools.bench_connectivity import make_engine  # noqa: E402

MODES = ("union", "weighted")


def host_route(eng, seed, S, mode, layers=None):
    """The samples over PCIe, then per sample and layer (the first `layers` of them) networkx's two measures: (effective_size,
    constraint) [S, layers, N], NaN where networkx gives NaN."""
    import networkx as nx
    L, N = (eng.L if layers is None else layers), eng.N
    es, con = np.full((S, L, N), np.nan), np.full((S, L, N), np.nan)
    for s in range(S):
        Y = eng.sample(seed + s)
        for l in range(L):
            B = Y[l] > 0
            B[np.arange(N), np.arange(N)] = False
            G = nx.DiGraph()
            G.add_nodes_from(range(N))
            G.add_edges_from(zip(*np.nonzero(B)))
            H = G.to_undirected() if mode == "union" else G
            e, c = nx.effective_size(H), nx.constraint(H)
            es[s, l] = [e[v] for v in range(N)]
            con[s, l] = [c[v] for v in range(N)]
    return es, con


def agrees(dev, host, Sh, tol=1e-12):
    """The device's values against networkx's on the nodes networkx defines; every node networkx defines is defined here."""
    ok = True
    for k, h in zip(("effective_size", "constraint"), host):
        d = dev[k][:Sh, :h.shape[1]]
        there = ~np.isnan(h)
        ok = ok and not np.isnan(d[there]).any() and bool((np.abs(d[there] - h[there]) <= tol * np.abs(h[there])).all())
    return ok


def shape_run(name, L, N, M, K, S, a, host_samples, host_layers, seed=17):
    eng = make_engine(L, N, M, K, 1 if name == "config3" else 2, a.degree)
    W = (N + 63) // 64
    out = {"shape": [L, N, N], "K": K, "S": S, "format": eng.data_format()[0], "waves_per_call": N * L * S,
           "lds_bytes_per_workgroup": {"k_sh_node": 4 * 2048 * 2, "k_sh_rank": 2 * 256 * 8 + 16 * 8 + 16},
           "pack_bytes_per_call": (N * N + 16 * N * W) * L * S}
    ok = True
    for mode in MODES:
        _, out["sample_structural_holes[%s]" % mode] = timed(lambda: eng.sample_structural_holes(seed, S, mode=mode), a.repeats, a.blocks)
    dev = {mode: eng.sample_structural_holes(seed, S, mode=mode, values=True) for mode in MODES}
    for mode in MODES:
        out["summary[%s]" % mode] = {"defined_share": float(dev[mode]["n_defined"].mean() / N),
                                     "mean_effective_size": float(dev[mode]["effective_size_sum"].sum() / dev[mode]["n_defined"].sum()),
                                     "mean_constraint": float(dev[mode]["constraint_sum"].sum() / dev[mode]["n_defined"].sum())}
    _, out["with_values"] = timed(lambda: eng.sample_structural_holes(seed, S, mode="union", values=True), a.repeats, a.blocks)
    Y0 = eng.sample(seed)
    net, out["network_structural_holes"] = timed(lambda: eng.network_structural_holes(Y0, mode="union", summary=True), a.repeats, a.blocks)
    same = all(net[k].tobytes() == dev["union"][k][0].tobytes() for k in ("degree", "strength", "redundancy", "effective_size", "constraint"))
    out["network_equals_sample"] = same
    ok = ok and same
    _, out["sample_shared_partners"] = timed(lambda: eng.sample_shared_partners(seed, S, mode="union", nodes=True), a.repeats, a.blocks)
    if not a.no_host:
        import networkx as nx
        Sh, Lh = min(S, host_samples), min(L, host_layers)
        out["host"] = {}
        nx.constraint(nx.path_graph(4)), nx.effective_size(nx.path_graph(4))      # (networkx's import is not the route's cost)
        for mode in MODES:
            host, t = timed(lambda: host_route(eng, seed, Sh, mode, Lh), 1, 1, warm=False)
            med = out["sample_structural_holes[%s]" % mode]["median_ms"]
            good = agrees(dev[mode], host, Sh)
            scaled = t["median_ms"] * S / Sh * L / Lh
            out["host"][mode] = dict(t, library="networkx " + nx.__version__, samples=Sh, layers=Lh, scaled_ms=scaled,
                                     scaled_over_device=scaled / med, agrees=good,
                                     note="the host route ran once on `samples` samples and `layers` layers; scaled_ms is its time times "
                                          "S / samples times L / layers")
            ok = ok and good
    eng.close()
    return out, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3, help="calls per block")
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--degree", type=float, default=5.0, help="mean out-degree of a sampled network")
    ap.add_argument("--host-n", type=int, default=500)
    ap.add_argument("--samples", type=int, default=32, help="samples of the small network")
    ap.add_argument("--host-samples", type=int, default=2, help="samples the host route takes at the small shape (its time is scaled to S)")
    ap.add_argument("--host-samples-large", type=int, default=1, help="samples the host route takes at the large shape (its time is scaled to S)")
    ap.add_argument("--host-layers-large", type=int, default=1, help="layers the host route takes at the large shape (its time is scaled to L)")
    ap.add_argument("--no-host", action="store_true", help="leave the host route out (a run under a profiler)")
    ap.add_argument("--small", action="store_true", help="L = 2, N = 200 and N = 60: a rehearsal of the script, not a measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "holes_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_holes.py measures on a GPU; none is visible: the numbers stay unmeasured")
    big = (2, 200, 40, 2, 16) if a.small else (4, 2000, 200, 2, 256)
    small = (1, 60, 40, 2, 8) if a.small else (1, a.host_n, 200, 2, a.samples)
    out = {"case": "rehearsal" if a.small else "config3", "repeats": a.repeats, "blocks": a.blocks, "degree": a.degree,
           "call_note": "whole calls are timed: allocations, the draw of the samples, the kernels, the copies back and the synchronisation"}
    out["small"], ok2 = shape_run("small", *small, a, a.host_samples, small[0])
    print(json.dumps({"small": out["small"]}), flush=True)
    out["config3"], ok1 = shape_run("config3", *big, a, a.host_samples_large, a.host_layers_large)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)
    assert ok1 and ok2, "the device and the host disagree"


if __name__ == "__main__":
    main()
