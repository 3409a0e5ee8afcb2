#!/usr/bin/env python
"""Time the posterior connectivity (vmr_sample_connectivity) at BASELINE config 3's shape (L = 4, N = 2000, K = 2) and density
(a state whose rho gives every node about `--degree` = 5 ties), S = 256 samples, on one GPU:
  sample_connectivity_ms        `eng.sample_connectivity(seed, S, nodes=True)`: the draw, the bit packing, the three closures per
                                block of 64 sources, the tally of the components and the copies back
  sample_connectivity_plain_ms  the same without the node arrays (counts and the distance histogram only)
  sample_triads_ms / sample_stats_ms   `eng.sample_triads(seed, S)` and `eng.sample_stats(seed, S)` of the same engine, for scale:
                                the same draw (and the same packing) with their own reductions behind it
  host_ms                       the route it replaces, on `--host-samples` samples: `eng.sample(seed + s)` over PCIe plus
                                scipy.sparse.csgraph (connected_components weak and strong, shortest_path(unweighted=True)), timed
                                once and SCALED to S samples (host_scaled_ms): it is too slow to run in full
and against the host route in full on a small network (default L = 1, N = 500, 32 samples, the same mean degree):
  device_ms / host_ms           `eng.sample_connectivity(seed, S_host, nodes=True)` against the route above on all S_host samples
Whole calls are timed -- allocations, the draw, the kernels, the copies back and the synchronisation -- `--repeats` times after a
warm-up call; medians and every single time are recorded.  The device and the host give the same integers (asserted).
Writes profiles/connectivity_bench.json and prints it.
Usage: python tools/bench_connectivity.py [--repeats 5] [--degree 5] [--small] [--no-host] [--host-n 500] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, repeats, warm=True):
    import torch
    if warm:
        fn()      # warm-up: code objects, allocator
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, ts


def make_engine(L, N, M, K, seed, degree):
    """Reports of a synthetic network, and a state whose rho puts a mean of degree / N on "tie" (uniform on [0, 2 degree / N])."""
    import torch
    from vimure_amd import CaviEngine
    from vimure_amd.synthetic import standard_sbm
    net = standard_sbm(N=N, M=M, L=L, K=2, avg_degree=10.0, eta=0.5, seed=seed, device="cuda")
    eng = CaviEngine(net.X, None, K=K, mutuality=True)
    del net
    torch.cuda.empty_cache()
    g = np.random.RandomState(0)
    rho = np.zeros((L, N, N, K))
    p = g.rand(L, N, N) * min(1.0, 2.0 * degree / N)
    rho[..., 1:] = (p / (K - 1))[..., None]
    rho[..., 0] = 1.0 - p
    eng.set_priors(0.1, 0.1, 10.0, 10.0, 0.5, 1.0)
    eng.set_state(g.gamma(2.0, 1.0, (L, M)) + 0.1, g.gamma(2.0, 1.0, (L, M)) + 0.1, g.gamma(5.0, 1.0, (L, K)) + 0.1,
                  g.gamma(2.0, 1.0, (L, K)) + 0.1, 3.0, 2.5, rho)
    return eng


def host_route(eng, seed, S):
    from tests.connectivity_util import connectivity_np
    return connectivity_np([eng.sample(seed + s) for s in range(S)])


def same_integers(dev, host, S=None):
    return bool(all(np.array_equal(dev[k][:S], host[k]) for k in host))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--degree", type=float, default=5.0, help="mean out-degree of a sampled network")
    ap.add_argument("--host-n", type=int, default=500)
    ap.add_argument("--host-samples", type=int, default=32, help="samples of the small network, all of which the host route takes")
    ap.add_argument("--host-samples-large", type=int, default=2, help="samples the host route takes at the large shape (its time is scaled to S)")
    ap.add_argument("--no-host", action="store_true", help="leave the host route out (a run under a profiler)")
    ap.add_argument("--small", action="store_true", help="L = 2, N = 200, M = 40 and the host route at N = 60: a rehearsal of the script, not a measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "connectivity_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_connectivity.py measures on a GPU; none is visible: the numbers stay unmeasured")
    L, N, M, K = (2, 200, 40, 2) if a.small else (4, 2000, 200, 2)
    S, seed = (16 if a.small else 256), 17
    med = lambda t: float(np.median(t))
    eng = make_engine(L, N, M, K, 1, a.degree)
    full, t_full = timed(lambda: eng.sample_connectivity(seed, S, nodes=True), a.repeats)
    plain, t_plain = timed(lambda: eng.sample_connectivity(seed, S), a.repeats)
    _, t_tri = timed(lambda: eng.sample_triads(seed, S), a.repeats)
    _, t_dyads = timed(lambda: eng.sample_stats(seed, S), a.repeats)
    W = (N + 63) // 64
    out = {"case": "small" if a.small else "config3", "L": L, "N": N, "M": M, "K": K, "S": S, "format": eng.data_format()[0],
           "repeats": a.repeats, "degree": a.degree, "mean_out_degree": float(plain["dist_hist"][..., 0].mean() / N),
           "workgroups_per_call": W * L * S, "lds_bytes_per_workgroup": 24 * 64 * W, "bitset_bytes_per_sample": 16 * L * N * W,
           "mean": {k: float(full[k].mean()) for k in ("components_w", "giant_w", "giant_s", "reach_pairs", "diameter")},
           "mean_avg_path_length": float((full["dist_sum"] / np.maximum(full["reach_pairs"], 1)).mean()),
           "sample_connectivity_median_ms": med(t_full), "sample_connectivity_all_ms": t_full,
           "sample_connectivity_plain_median_ms": med(t_plain), "sample_connectivity_plain_all_ms": t_plain,
           "sample_triads_median_ms": med(t_tri), "sample_triads_all_ms": t_tri,
           "sample_stats_median_ms": med(t_dyads), "sample_stats_all_ms": t_dyads,
           "plain_equals_full": same_integers(full, plain),
           "call_note": "whole calls are timed: allocations, the draw of the samples, the kernels, the copies back and the synchronisation"}
    same = out["plain_equals_full"]
    if not a.no_host:
        Sl = min(S, a.host_samples_large)
        host, t_host = timed(lambda: host_route(eng, seed, Sl), 1, warm=False)
        out.update({"host_samples": Sl, "host_ms": t_host[0], "host_scaled_ms": t_host[0] * S / Sl,
                    "host_note": "the host route ran once on host_samples samples; host_scaled_ms is that time times S / host_samples",
                    "host_scaled_over_device": t_host[0] * S / Sl / med(t_full), "same_integers": same_integers(full, host, Sl)})
        same = same and out["same_integers"]
    eng.close()

    if not a.no_host:
        Lh, Nh, Sh = (1, 60, 8) if a.small else (1, a.host_n, a.host_samples)
        eng = make_engine(Lh, Nh, M, K, 2, a.degree)
        dev, t_dev = timed(lambda: eng.sample_connectivity(seed, Sh, nodes=True), a.repeats)
        host, t_host = timed(lambda: host_route(eng, seed, Sh), a.repeats)
        eng.close()
        out["small"] = {"shape": [Lh, Nh, Nh], "samples": Sh, "device_median_ms": med(t_dev), "device_all_ms": t_dev,
                        "host_median_ms": med(t_host), "host_all_ms": t_host, "host_over_device": med(t_host) / med(t_dev),
                        "mean_giant_w": float(dev["giant_w"].mean()), "mean_diameter": float(dev["diameter"].mean()),
                        "same_integers": same_integers(dev, host)}
        same = same and out["small"]["same_integers"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)
    assert same, "the device and the host disagree"


if __name__ == "__main__":
    main()
