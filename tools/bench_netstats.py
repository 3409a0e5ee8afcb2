#!/usr/bin/env python3
"""Time the posterior network statistics on the device against the host route to the same numbers, on
  config3      BASELINE config 3 (L = 4, N = 2000, M = 200, K = 2)
  karnataka    one self-reporter layer shaped like a Karnataka village (N = M = 600, K = 2)
  k12          the general kernels: L = 1, N = 500, M = 50, K = 12
from a random state (the numbers do not depend on the fit), S = 256 samples:
  sample_stats_ms     `eng.sample_stats(seed, S, degrees=True)` (vmr_sample_stats)
  host_route_ms       S calls of `eng.sample(seed + s)` plus the NumPy reductions of the same columns and degrees
  expected_stats_ms   `eng.expected_stats()` (vmr_expected_stats)
  host_expected_ms    `eng.get_state()["rho"]` plus NumPy
and checks that both routes give the same counts.  Prints one JSON line per case.
Usage: python tools/bench_netstats.py [case ...]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def host_route(eng, seed, S):
    out = {k: np.zeros((S, eng.L), np.int64) for k in ("edges", "weight", "mutual")}
    dout, din = np.zeros((S, eng.L, eng.N), np.int32), np.zeros((S, eng.L, eng.N), np.int32)
    for s in range(S):
        Y = eng.sample(seed + s)
        for l in range(eng.L):
            on = Y[l] > 0
            out["edges"][s, l] = on.sum()
            out["weight"][s, l] = Y[l].sum(dtype=np.int64)
            out["mutual"][s, l] = np.logical_and(on, on.T).sum()
            dout[s, l], din[s, l] = on.sum(axis=1), on.sum(axis=0)
    out["deg_out"], out["deg_in"] = dout, din
    return out


def host_expected(eng):
    rho = eng.get_state()["rho"]
    p = rho[..., 1:].sum(-1)
    return {"edges": p.sum(axis=(1, 2)), "weight": (rho * np.arange(rho.shape[-1])).sum(axis=(1, 2, 3)),
            "mutual": np.einsum("lij,lji->l", p, p), "edges_var": (p * (1.0 - p)).sum(axis=(1, 2))}


def run(name, L, N, M, K, self_reporter=False, S=256, repeats=3):
    import torch
    from vimure_amd import CaviEngine
    from vimure_amd.synthetic import standard_sbm
    net = standard_sbm(N=N, M=M, L=L, K=2, avg_degree=10.0, eta=0.5, seed=1, flag_self_reporter=self_reporter, device="cuda")
    eng = CaviEngine(net.X, net.R if self_reporter else None, K=K, mutuality=True)
    del net
    torch.cuda.empty_cache()
    g = np.random.RandomState(0)
    rho = g.rand(L, N, N, K)
    rho[..., 0] *= 20.0
    rho /= rho.sum(-1, keepdims=True)
    eng.set_priors(0.1, 0.1, 10.0, 10.0, 0.5, 1.0)
    eng.set_state(g.gamma(2.0, 1.0, (L, M)) + 0.1, g.gamma(2.0, 1.0, (L, M)) + 0.1, g.gamma(5.0, 1.0, (L, K)) + 0.1,
                  g.gamma(2.0, 1.0, (L, K)) + 0.1, 3.0, 2.5, rho)
    del rho
    out = {"case": name, "L": L, "N": N, "M": M, "K": K, "S": S, "format": eng.data_format()[0]}
    seed = 17
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        dev = eng.sample_stats(seed, S, degrees=True)
        ts.append(time.perf_counter() - t0)
    out["sample_stats_ms"] = min(ts) * 1e3
    t0 = time.perf_counter()
    eng.sample_stats(seed, S)
    out["sample_stats_no_degrees_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    eng.sample(seed)
    out["one_sample_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    host = host_route(eng, seed, S)
    out["host_route_ms"] = (time.perf_counter() - t0) * 1e3
    out["same_counts"] = bool(all(np.array_equal(dev[k], host[k]) for k in host))
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        ex = eng.expected_stats()
        ts.append(time.perf_counter() - t0)
    out["expected_stats_ms"] = min(ts) * 1e3
    t0 = time.perf_counter()
    hx = host_expected(eng)
    out["host_expected_ms"] = (time.perf_counter() - t0) * 1e3
    out["expected_max_rel_diff"] = float(max(np.max(np.abs(ex[k] - hx[k]) / np.abs(hx[k])) for k in hx))
    out["speedup_samples"] = out["host_route_ms"] / out["sample_stats_ms"]
    out["mean_reciprocity"] = float(np.mean(dev["mutual"] / dev["weight"]))
    eng.close()
    print(json.dumps(out), flush=True)


CASES = {"config3": dict(L=4, N=2000, M=200, K=2), "karnataka": dict(L=1, N=600, M=600, K=2, self_reporter=True),
         "k12": dict(L=1, N=500, M=50, K=12)}

if __name__ == "__main__":
    for c in (sys.argv[1:] or ["k12", "karnataka", "config3"]):
        run(c, **CASES[c])
