#!/usr/bin/env python3
"""Time the posterior-predictive check on the device: `CaviEngine.mean_poisson(layer=l, device=True)` (vmr_mean_poisson, output
left on the GPU) and `CaviEngine.report_auc()` (vmr_report_auc), on
  config3      BASELINE config 3 (L = 4, N = 2000, M = 200, K = 2) with a full mask: L N^2 M = 3.2 G support entries
  karnataka    one self-reporter layer shaped like a Karnataka village (N = M = 600, K = 2)
  k12          the general kernels: L = 1, N = 500, M = 50, K = 12
from a random state (the numbers do not depend on the fit).  Prints one JSON line per case.
Usage: python tools/bench_ppc.py [case ...]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(name, L, N, M, K, self_reporter=False, repeats=3):
    import torch
    from vimure_amd import CaviEngine
    from vimure_amd.synthetic import standard_sbm
    net = standard_sbm(N=N, M=M, L=L, K=2, avg_degree=10.0, eta=0.5, seed=1, flag_self_reporter=self_reporter, device="cuda")
    eng = CaviEngine(net.X, net.R if self_reporter else None, K=K, mutuality=True)
    del net
    torch.cuda.empty_cache()
    g = np.random.RandomState(0)
    rho = g.rand(L, N, N, K)
    rho /= rho.sum(-1, keepdims=True)
    eng.set_priors(0.1, 0.1, 10.0, 10.0, 0.5, 1.0)
    eng.set_state(g.gamma(2.0, 1.0, (L, M)) + 0.1, g.gamma(2.0, 1.0, (L, M)) + 0.1, g.gamma(5.0, 1.0, (L, K)) + 0.1,
                  g.gamma(2.0, 1.0, (L, K)) + 0.1, 3.0, 2.5, rho)
    del rho
    out = {"case": name, "L": L, "N": N, "M": M, "K": K, "format": eng.data_format()[0], "nnz": eng.data_format()[1],
           "support": eng.mean_poisson_size()}
    t_mp = []
    for _ in range(repeats):
        ts = []
        for l in range(L):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            subs, vals = eng.mean_poisson(layer=l, device=True)
            ts.append(time.perf_counter() - t0)
            del subs, vals
        t_mp.append(ts)
    torch.cuda.empty_cache()
    out["mean_poisson_layer_ms"] = min(min(ts) for ts in t_mp) * 1e3
    t_auc = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        auc, P, Q = eng.report_auc()
        t_auc.append(time.perf_counter() - t0)
    out.update({"report_auc_ms": min(t_auc) * 1e3, "auc": auc, "n_pos": P, "n_neg": Q})
    eng.close()
    print(json.dumps(out), flush=True)


CASES = {"config3": dict(L=4, N=2000, M=200, K=2), "karnataka": dict(L=1, N=600, M=600, K=2, self_reporter=True),
         "k12": dict(L=1, N=500, M=50, K=12)}

if __name__ == "__main__":
    for c in (sys.argv[1:] or ["k12", "karnataka", "config3"]):
        run(c, **CASES[c])
