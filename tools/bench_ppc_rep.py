#!/usr/bin/env python3
"""Time one posterior predictive replicate of BASELINE config 3 (L = 4, N = 2000, M = 200, K = 2; all-ones mask) two ways:
  ppc_replicates_ms   `eng.ppc_replicates(...)` with n_rep = 1 (vmr_ppc_replicates: the replicate is drawn and reduced, never written)
  composed_ms         the route that existed before: `eng.sample` on the device -> a torch gather of lambda -> vmr_generate_x (the
                      dense uint8 replicate) -> torch reductions to the same six integers
from a random state (the numbers do not depend on the fit), and the peak device memory each route adds to the engine's own
(free memory polled while the call runs: both routes allocate outside torch's allocator as well).  Each route is warmed up once
and timed `--repeats` times around a device synchronise; min and median are kept.  Checks that both give the same counts
(rates are chosen so that the uint8 replicate never clamps).  Writes profiles/ppc_rep_bench.json and prints it.
Usage: python tools/bench_ppc_rep.py [--repeats 5] [--small]"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class PeakUse:
    """Lowest free device memory seen while the block runs, against the free memory at entry."""

    def __enter__(self):
        import torch
        self.torch = torch
        torch.cuda.synchronize()
        self.free0 = torch.cuda.mem_get_info()[0]
        self.low, self.stop = self.free0, False
        self.th = threading.Thread(target=self.poll, daemon=True)
        self.th.start()
        return self

    def poll(self):
        while not self.stop:
            self.low = min(self.low, self.torch.cuda.mem_get_info()[0])
            time.sleep(0.0005)

    def __exit__(self, *a):
        self.stop = True
        self.th.join()
        self.bytes = self.free0 - self.low


def composed(eng, theta, lam, eta, seed_y, seed_x):
    """counts int64 [L, 6] of replicate 0 through the dense tensor."""
    import torch
    from vimure_amd.synthetic import device_build_x
    dev = torch.device("cuda", eng.device)
    Y = torch.empty((eng.L, eng.N, eng.N), dtype=torch.uint8, device=dev)
    eng.sample(seed_y, 1, out=Y)
    table = torch.as_tensor(lam[0], device=dev)
    lam_t = torch.gather(table, 1, Y.reshape(eng.L, -1).long()).reshape(eng.L, eng.N, eng.N).contiguous()
    del Y
    X = device_build_x(None, theta[0], float(eta[0]), seed_x, lam=lam_t)
    del lam_t
    out = torch.zeros((eng.L, 6), dtype=torch.int64, device=dev)
    for l in range(eng.L):      # layer by layer: the temporaries of a reduction are as large as what it reads
        x = X[l]
        pos = x > 0
        out[l, 0] = pos.sum()
        out[l, 1] = x.sum(dtype=torch.int64)
        out[l, 2] = (x.to(torch.int32) ** 2).sum(dtype=torch.int64)
        out[l, 3] = (pos & pos.transpose(0, 1)).sum()      # (the diagonal of a replicate holds no report)
        per_tie = pos.sum(dim=2)
        out[l, 4] = (per_tie > 0).sum()
        out[l, 5] = (per_tie > 1).sum()
    res = out.cpu().numpy()
    assert int(X.max()) < 255, "the dense replicate clamps: lower the rates"
    return res


def timed(fn, repeats):
    import torch
    fn()      # warm-up: code objects, allocator
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    torch.cuda.empty_cache()      # (what the warm-up left in torch's cache would hide the route's own allocations)
    with PeakUse() as p:
        fn()
    return out, ts, p.bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="L = 2, N = 300, M = 40: a rehearsal of the script, not a measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppc_rep_bench.json"))
    a = ap.parse_args()
    import torch
    from vimure_amd import CaviEngine
    from vimure_amd.synthetic import standard_sbm
    if not torch.cuda.is_available():
        raise SystemExit("bench_ppc_rep.py measures on a GPU; none is visible")
    L, N, M, K = (2, 300, 40, 2) if a.small else (4, 2000, 200, 2)
    net = standard_sbm(N=N, M=M, L=L, K=2, avg_degree=10.0, eta=0.5, seed=1, device="cuda")
    eng = CaviEngine(net.X, None, K=K, mutuality=True)
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
    theta = 0.5 + 1.5 * g.rand(1, L, M)
    lam = np.broadcast_to(np.array([0.01, 1.5]), (1, L, K)).copy()
    eta = np.array([0.3])
    seed_y, seed_x = 17, 17 + 2 ** 32
    new, t_new, m_new = timed(lambda: eng.ppc_replicates(theta, lam, eta, seed_y, seed_x)[0], a.repeats)
    old, t_old, m_old = timed(lambda: composed(eng, theta, lam, eta, seed_y, seed_x), a.repeats)
    torch.cuda.empty_cache()
    out = {"case": "small" if a.small else "config3", "L": L, "N": N, "M": M, "K": K, "format": eng.data_format()[0], "repeats": a.repeats,
           "support_elements": L * N * N * M, "pair_draws": L * N * (N - 1) // 2 * M,
           "ppc_replicates_ms": min(t_new), "ppc_replicates_median_ms": float(np.median(t_new)), "ppc_replicates_all_ms": t_new,
           "composed_ms": min(t_old), "composed_median_ms": float(np.median(t_old)), "composed_all_ms": t_old,
           "ppc_replicates_peak_bytes": int(m_new), "composed_peak_bytes": int(m_old),
           "replicate_Y_bytes": L * N * N, "dense_replicate_bytes": L * N * N * M,
           "same_counts": bool(np.array_equal(new, old)), "counts": new.tolist()}
    eng.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
