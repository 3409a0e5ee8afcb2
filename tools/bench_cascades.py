#!/usr/bin/env python
"""Time the posterior cascades (vmr_sample_outreach, vmr_sample_seed_outreach, vmr_network_outreach) on one GPU at two shapes:
  config3   BASELINE config 3's shape (L = 4, N = 2000, K = 2) and density (a state whose rho gives every node about `--degree` = 5
            ties), S = 256 samples
  small     L = 1, N = 500, S = 32, the same mean degree
with `--cascades` = 16 cascades per sample, q the default of `VimureModel.posterior_cascades` (min(1, N / expected edges) per
layer), and per shape:
  sample_outreach_T3 / _T64       `eng.sample_outreach(seed, S, q, T)`, direction out: the draw, the bit packing, per cascade the
                                  thinning and the closure, the ranks and the summary, the fold and the copies back
  sample_outreach_union_T3        the same over A | A.T
  sample_seed_outreach_T3         `eng.sample_seed_outreach` of 64 seed sets of 5 nodes, curve and node_hits asked for
  network_outreach_T3             `eng.network_outreach(Y)` of one network [L, N, N] from the host
  sample_outreach_q1_K1           q = 1, T = N, ONE cascade: the work of one of the three closures of ...
  sample_connectivity / sample_stats   ... of the same engine, for scale: the same draw (and packing) with their own reductions
  host                            the route it replaces: `eng.sample(seed + s)` over PCIe plus the NumPy / SciPy restatement
                                  (tests/cascade_util.py) at T = 3, on `host.samples` samples and `host.cascades` cascades,
                                  SCALED to S and to the call's cascades (host.scaled_ms)
Whole calls are timed -- allocations, the draw, the kernels, the copies back and the synchronisation -- in `--blocks` blocks of
`--repeats` calls after a warm-up call; the median over all calls, the spread (min, max) and every block's median are recorded.
The device's values equal the host's, and at q = 1 connectivity's node_reach_out (asserted).
Writes profiles/cascades_bench.json and prints it.
Usage: python tools/bench_cascades.py [--repeats 3] [--blocks 2] [--degree 5] [--cascades 16] [--small] [--no-host] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_centrality import timed  # noqa: E402
from tools.bench_connectivity import make_engine  # noqa: E402


def host_route(eng, seed, S, cs, K, q, T):
    """The samples over PCIe, then the restatement's cascades on them: values [S, L, N]."""
    from tests.cascade_util import outreach_values
    Ys = np.asarray([eng.sample(seed + s) for s in range(S)])
    return outreach_values(Ys, cs, K, q, T, "out")


def shape_run(name, L, N, M, K, S, a, host_samples, seed=17, top_k=10, cs=5):
    from vimure_amd.centrality import default_q
    eng = make_engine(L, N, M, K, 1 if name == "config3" else 2, a.degree)
    W = (N + 63) // 64
    q = default_q(N, eng.expected_stats()["edges"])
    Kc = a.cascades
    out = {"shape": [L, N, N], "K": K, "S": S, "n_cascades": Kc, "q": [float(x) for x in q], "top_k": top_k, "format": eng.data_format()[0],
           "launches_per_chunk": 2 * Kc, "workgroups_per_closure_launch": W * L * S, "lds_bytes_per_workgroup": 24 * 64 * W,
           "live_row_bytes_per_sample": 8 * N * W * L, "pack_bytes_per_call": (N * N + 16 * N * W) * L * S}
    kw = dict(n_cascades=Kc, cascade_seed=cs, top_k=top_k)
    r3, out["sample_outreach_T3"] = timed(lambda: eng.sample_outreach(seed, S, q, T=3, **kw), a.repeats, a.blocks)
    r64, out["sample_outreach_T64"] = timed(lambda: eng.sample_outreach(seed, S, q, T=64, **kw), a.repeats, a.blocks)
    _, out["sample_outreach_union_T3"] = timed(lambda: eng.sample_outreach(seed, S, q, T=3, direction="union", **kw), a.repeats, a.blocks)
    out["mean_outreach_T3"], out["mean_outreach_T64"] = float(r3["node_sum"].mean() / S), float(r64["node_sum"].mean() / S)
    sets = [[(5 * b + i) % N for i in range(5)] for b in range(64)]
    _, out["sample_seed_outreach_T3"] = timed(lambda: eng.sample_seed_outreach(seed, S, sets, q, T=3, n_cascades=Kc, cascade_seed=cs,
                                                                               node_hits=True), a.repeats, a.blocks)
    Y0 = eng.sample(seed)
    net, out["network_outreach_T3"] = timed(lambda: eng.network_outreach(Y0, q, T=3, n_cascades=Kc, cascade_seed=cs), a.repeats, a.blocks)
    one = eng.sample_outreach(seed, 1, q, T=3, values=True, **kw)["values"][0]
    ok = bool(np.array_equal(net, one))
    out["network_equals_sample_values"] = ok
    full, out["sample_outreach_q1_K1"] = timed(lambda: eng.sample_outreach(seed, S, 1.0, T=N, n_cascades=1, top_k=top_k, values=True),
                                               a.repeats, a.blocks)
    conn, out["sample_connectivity"] = timed(lambda: eng.sample_connectivity(seed, S, nodes=True), a.repeats, a.blocks)
    out["q1_equals_connectivity"] = bool(np.array_equal(full["values"], conn["node_reach_out"].astype(np.uint32)))
    ok = ok and out["q1_equals_connectivity"]
    _, out["sample_stats"] = timed(lambda: eng.sample_stats(seed, S), a.repeats, a.blocks)
    if not a.no_host:
        Sh, Kh = min(S, host_samples), min(Kc, a.host_cascades)
        host, t = timed(lambda: host_route(eng, seed, Sh, cs, Kh, q, 3), 1, 1, warm=False)
        dev = eng.sample_outreach(seed, Sh, q, T=3, n_cascades=Kh, cascade_seed=cs, values=True)["values"]
        scaled = t["median_ms"] * (S / Sh) * (Kc / Kh)
        agrees = bool(np.array_equal(dev, host))
        out["host"] = dict(t, library="numpy " + np.__version__, samples=Sh, cascades=Kh, scaled_ms=scaled,
                           scaled_over_device=scaled / out["sample_outreach_T3"]["median_ms"], agrees=agrees,
                           note="the host route ran once on `samples` samples and `cascades` cascades; scaled_ms is its time times "
                                "S / samples times n_cascades / cascades")
        ok = ok and agrees
    eng.close()
    return out, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3, help="calls per block")
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--degree", type=float, default=5.0, help="mean out-degree of a sampled network")
    ap.add_argument("--cascades", type=int, default=16)
    ap.add_argument("--host-n", type=int, default=500)
    ap.add_argument("--samples", type=int, default=32, help="samples of the small network")
    ap.add_argument("--host-samples", type=int, default=4, help="samples the host route takes at the small shape (its time is scaled to S)")
    ap.add_argument("--host-samples-large", type=int, default=1, help="samples the host route takes at the large shape (its time is scaled to S)")
    ap.add_argument("--host-cascades", type=int, default=2, help="cascades the host route takes (its time is scaled to --cascades)")
    ap.add_argument("--no-host", action="store_true", help="leave the host route out (a run under a profiler)")
    ap.add_argument("--small", action="store_true", help="L = 2, N = 200 and N = 60: a rehearsal of the script, not a measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cascades_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_cascades.py measures on a GPU; none is visible: the numbers stay unmeasured")
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
