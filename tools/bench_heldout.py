#!/usr/bin/env python3
"""Time the held-out log-likelihood at BASELINE config 3's shape (L = 4, N = 2000, M = 200, K = 2, report lists, no mask): one
`eng.heldout_loglik(...)` call (vmr_heldout_loglik) over a list of n entries drawn from the support, three ways:
  sorted_ms     the list sorted by (l, i, j, m): the entries of a tie sit in neighbouring lanes and read one rho row -- the fast case
  shuffled_ms   the same entries shuffled inside every layer (the list stays non-decreasing in l): a gather over rho, a row per lane
  host_ms       the route that existed before: `eng.get_state()["rho"]` (8 L N^2 K bytes over PCIe) plus the NumPy restatement
                `crossval.heldout_loglik_np` on the same list, timed once
The lists and the per-entry outputs live on the device (int32 / float64 tensors), so the call is the tie -> position table of
each layer, the pass and its second stage, and 64 B of sums and counts coming back.  Each route is warmed up once and timed
around a device synchronise; the median and all repeats are kept.  entries_per_s = n / median; rho_bytes_per_s = 8 K n / median
is the rate at which rho rows are consumed -- the sorted list reads far fewer distinct bytes than that, the shuffled one about
that many 64-byte sectors.  Asserts that the three routes agree (counts exact, the sorted and shuffled per-entry values bit for
bit, the host's within 1e-9).  Writes profiles/heldout_bench.json and prints it.
Usage: python tools/bench_heldout.py [--repeats 5] [--small] [--entries N]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    return out, ts


def make_engine(L, N, M, K, seed):
    import torch
    from vimure_amd import CaviEngine
    from vimure_amd.synthetic import standard_sbm
    net = standard_sbm(N=N, M=M, L=L, K=2, avg_degree=10.0, eta=0.5, seed=seed, device="cuda")
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
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--entries", type=int, default=1 << 22)
    ap.add_argument("--small", action="store_true", help="L = 2, N = 300, M = 40, 2^16 entries: a rehearsal of the script, not a measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heldout_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_heldout.py measures on a GPU; none is visible: the numbers stay unmeasured")
    from vimure_amd.crossval import heldout_loglik_np
    L, N, M, K = (2, 300, 40, 2) if a.small else (4, 2000, 200, 2)
    n = min(a.entries, 1 << 16) if a.small else a.entries
    eng = make_engine(L, N, M, K, 1)
    g = np.random.RandomState(2)
    # ties drawn at random, a run of reporters at each: what a fold of a pair-wise split looks like
    per = 8
    nt = n // per
    l, i, j = np.sort(g.randint(0, L, nt)), g.randint(0, N, nt), g.randint(0, N, nt)
    m0 = g.randint(0, M - per + 1, nt)
    subs = [np.repeat(l, per), np.repeat(i, per), np.repeat(j, per), (m0[:, None] + np.arange(per)[None, :]).reshape(-1)]
    n = len(subs[0])
    x = ((g.rand(n) < 0.1) * g.randint(1, 4, n)).astype(np.int64)
    xt = ((g.rand(n) < 0.1) * g.randint(1, 4, n)).astype(np.int64)
    order = np.lexsort(subs[::-1])
    shuf = np.concatenate([np.flatnonzero(subs[0] == q)[g.permutation(int((subs[0] == q).sum()))] for q in range(L)])
    theta, lam, eta = g.gamma(2.0, 0.5, (L, M)) + 0.05, g.gamma(2.0, 1.0, (L, K)) + 0.05, 0.3
    dev = torch.device("cuda", eng.device)

    def on_device(idx):
        return [torch.as_tensor(np.ascontiguousarray(v[idx], dtype=np.int32), device=dev) for v in subs + [x, xt]]
    ds, dsh = on_device(order), on_device(shuf)

    def call(d):
        return eng.heldout_loglik(tuple(d[:4]), d[4], d[5], theta=theta, lam=lam, eta=eta, device=True)
    rs, t_sorted = timed(lambda: call(ds), a.repeats)
    rh, t_shuf = timed(lambda: call(dsh), a.repeats)

    def host():
        rho = eng.get_state()["rho"]
        return heldout_loglik_np(rho, tuple(v[order] for v in subs), x[order], xt[order], theta, lam, eta)
    (lp_h, mn_h, _, cn_h), t_host = timed(host, 1)
    inv = np.empty(n, np.int64)
    inv[shuf] = np.arange(n)
    lp_s, lp_sh = rs["logp"].cpu().numpy(), rh["logp"].cpu().numpy()
    same = bool(np.array_equal(rs["counts"], rh["counts"]) and np.array_equal(rs["counts"], cn_h)
                and np.array_equal(lp_s, lp_sh[inv[order]]) and np.allclose(lp_s, lp_h, rtol=1e-9, atol=1e-9))
    fmt = eng.data_format()[0]
    eng.close()
    ms, msh = float(np.median(t_sorted)), float(np.median(t_shuf))
    out = {"case": "small" if a.small else "config3", "L": L, "N": N, "M": M, "K": K, "format": fmt, "repeats": a.repeats,
           "entries": n, "ties_in_list": nt,
           "sorted_median_ms": ms, "sorted_all_ms": t_sorted, "sorted_entries_per_s": n / (ms * 1e-3),
           "sorted_rho_bytes_per_s": 8 * K * n / (ms * 1e-3),
           "shuffled_median_ms": msh, "shuffled_all_ms": t_shuf, "shuffled_entries_per_s": n / (msh * 1e-3),
           "shuffled_rho_bytes_per_s": 8 * K * n / (msh * 1e-3),
           "host_ms": min(t_host), "host_all_ms": t_host, "host_entries_per_s": n / (min(t_host) * 1e-3),
           "host_pcie_bytes": L * N * N * 8 * K,
           "call_note": "the whole call is timed: the tie -> position table of every layer, the pass, its second stage",
           "same_results": same}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)
    assert same, "the routes disagree"


if __name__ == "__main__":
    main()
