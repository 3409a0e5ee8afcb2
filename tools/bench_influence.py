#!/usr/bin/env python3
"""Time the reporter influence (vmr_reporter_influence) at BASELINE config 3's shape (L = 4, N = 2000, M = 200, K = 2, report lists,
no mask: 3.2e9 support elements), whole calls of `eng.reporter_influence(...)`:
  aggregates_ms   an aggregates-only call over the top-n grid (4096 edges): one walk of the support -- the leave-one-out row of
                  every element, the reporters' bins, the histogram; no row is written
and, at the largest shape of the same family whose support the host can hold (--host-n, default L = 1, N = 200: 8e6 elements),
  device_ms       the aggregates-only call there
  flips_ms        what `VimureModel.reporter_influence()` does, there: the size call, the count and fill passes, the flips' marks
  host_ms         the route that exists without it: rho over PCIe (`eng.get_state`), then `influence.influence_np` on the host
Each route is warmed up once and timed around a device synchronise; the median and all repeats are kept.  elements_per_s =
support / median.  Asserts that the device and the host agree (counts exact, the sums to 1e-9 relative).  Writes
profiles/influence_bench.json and prints it.
Usage: python tools/bench_influence.py [--repeats 3] [--small] [--host-n 200]"""
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


def make_engine(L, N, M, K, seed, keep_x=False):
    import torch
    from scipy.special import psi
    from vimure_amd import CaviEngine
    from vimure_amd.synthetic import standard_sbm
    net = standard_sbm(N=N, M=M, L=L, K=2, avg_degree=10.0, eta=0.5, seed=seed, device="cuda")
    eng = CaviEngine(net.X, None, K=K, mutuality=True)
    X = net.X.cpu().numpy().astype(np.int64) if keep_x else None
    del net
    torch.cuda.empty_cache()
    g = np.random.RandomState(0)
    rho = g.rand(L, N, N, K)
    rho[..., 0] *= 20.0
    rho /= rho.sum(-1, keepdims=True)
    gs, gr = g.gamma(2.0, 1.0, (L, M)) + 0.1, g.gamma(2.0, 1.0, (L, M)) + 0.1
    ps, pr = g.gamma(5.0, 1.0, (L, K)) + 0.1, g.gamma(2.0, 1.0, (L, K)) + 0.1
    eng.set_priors(0.1, 0.1, 10.0, 10.0, 0.5, 1.0)
    eng.set_state(gs, gr, ps, pr, 3.0, 2.5, rho)
    tabs = (gs / gr, psi(gs) - np.log(gr), ps / pr, psi(ps) - np.log(pr), float(np.exp(psi(3.0) - np.log(2.5))))
    return eng, X, tabs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-n", type=int, default=200)
    ap.add_argument("--small", action="store_true", help="L = 2, N = 200, M = 40 and the host route at N = 60: a rehearsal of the script, not a measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "influence_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_influence.py measures on a GPU; none is visible: the numbers stay unmeasured")
    from vimure_amd.influence import grid_edges, influence_np
    L, N, M, K = (2, 200, 40, 2) if a.small else (4, 2000, 200, 2)
    eng, _, tabs = make_engine(L, N, M, K, 1)
    edges = grid_edges()

    def aggregates(e=eng, t=tabs):
        return e.reporter_influence(*t, select="none", edges=edges, rows=False)
    agg, t_agg = timed(aggregates, a.repeats)
    support = int(agg["counts"][:, :, 0].sum())
    fmt = eng.data_format()[0]
    eng.close()

    # the host route, where the support fits on the host
    Lh, Nh = (1, 60) if a.small else (1, a.host_n)
    eng, X, tabs = make_engine(Lh, Nh, M, K, 2, keep_x=True)
    dev, t_dev = timed(lambda: aggregates(eng, tabs), a.repeats)
    flips, t_flips = timed(lambda: eng.reporter_influence(*tabs), a.repeats)
    n_flips = int(flips["counts"][:, :, 3].sum())
    flips_ok = bool(len(flips["l"]) == n_flips == int((flips["lost"] | flips["gained"]).sum()))

    def by_host():
        rho = eng.get_state()["rho"]
        return influence_np(rho, X, None, *tabs, mutuality=True, select="none", edges=edges)
    host, t_host = timed(by_host, a.repeats)
    n_host = int(dev["counts"][:, :, 0].sum())
    same = bool(np.array_equal(dev["counts"], host["counts"]) and np.allclose(dev["sums"], host["sums"], rtol=1e-9, atol=1e-9))
    eng.close()
    ma, mf, md, mh = (float(np.median(t)) for t in (t_agg, t_flips, t_dev, t_host))
    out = {"case": "small" if a.small else "config3", "L": L, "N": N, "M": M, "K": K, "format": fmt, "repeats": a.repeats,
           "support": support, "edges": len(edges),
           "aggregates_median_ms": ma, "aggregates_all_ms": t_agg, "aggregates_elements_per_s": support / (ma * 1e-3),
           "flips": n_flips, "flips_median_ms": mf, "flips_all_ms": t_flips, "flips_rows_ok": flips_ok,
           "host_shape": [Lh, Nh, Nh, M], "host_entries": n_host, "device_median_ms": md, "device_all_ms": t_dev,
           "device_elements_per_s": n_host / (md * 1e-3), "host_median_ms": mh, "host_all_ms": t_host,
           "host_elements_per_s": n_host / (mh * 1e-3), "host_over_device": mh / md, "rho_bytes": 8 * Lh * Nh * Nh * K,
           "call_note": "whole calls are timed: the per-layer set-up (the tie-major index and the tie -> position table of a "
                        "report-list handle), the passes, the scan, the copies back and the synchronisation",
           "same_results": same}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)
    assert same, "the device and the host disagree"
    assert flips_ok, "the rows are not the flips"


if __name__ == "__main__":
    main()
