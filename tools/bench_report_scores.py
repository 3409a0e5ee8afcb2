#!/usr/bin/env python3
"""Time the report scores (vmr_report_scores) at BASELINE config 3's shape (L = 4, N = 2000, M = 200, K = 2, report lists, no mask:
3.2e9 support elements), whole calls of `eng.report_scores(...)`:
  aggregates_ms   an aggregates-only call over the top-n grid (4096 edges): one walk of the support -- the likelihood at every
                  element, the histogram, the counts and sums; no row is written
  top1000_ms      what `VimureModel.surprising_reports(top=1000)` does: the aggregates-only call, the threshold read off its
                  histogram, the size call, the count and fill passes, the sort of the rows on the host
and, at the largest shape of the same family whose support still fits in a list (--list-n, default L = 1, N = 1000: 2e8 elements),
  walk_ms         the aggregates-only call there
  list_ms         the route that exists without it: `eng.mean_poisson(device=True)` writes the support out (24 B per element), the
                  counts and mirrored counts are gathered from X on the device, and `eng.heldout_loglik(..., device=True)` scores
                  the list
Each route is warmed up once and timed around a device synchronise; the median and all repeats are kept.  elements_per_s =
support / median.  Asserts that the walk and the list agree (counts exact, the sum of logp to 1e-9 relative) and that the top rows
are sorted.  Writes profiles/report_scores_bench.json and prints it.
Usage: python tools/bench_report_scores.py [--repeats 3] [--small] [--list-n 1000]"""
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
    from vimure_amd import CaviEngine
    from vimure_amd.synthetic import standard_sbm
    net = standard_sbm(N=N, M=M, L=L, K=2, avg_degree=10.0, eta=0.5, seed=seed, device="cuda")
    eng = CaviEngine(net.X, None, K=K, mutuality=True)
    X = net.X if keep_x else None
    del net
    torch.cuda.empty_cache()
    g = np.random.RandomState(0)
    rho = g.rand(L, N, N, K)
    rho[..., 0] *= 20.0
    rho /= rho.sum(-1, keepdims=True)
    eng.set_priors(0.1, 0.1, 10.0, 10.0, 0.5, 1.0)
    eng.set_state(g.gamma(2.0, 1.0, (L, M)) + 0.1, g.gamma(2.0, 1.0, (L, M)) + 0.1, g.gamma(5.0, 1.0, (L, K)) + 0.1,
                  g.gamma(2.0, 1.0, (L, K)) + 0.1, 3.0, 2.5, rho)
    theta, lam = g.gamma(2.0, 0.5, (L, M)) + 0.05, g.gamma(2.0, 1.0, (L, K)) + 0.05
    return eng, X, theta, lam, 0.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--list-n", type=int, default=1000)
    ap.add_argument("--small", action="store_true", help="L = 2, N = 200, M = 40 and a list at N = 100: a rehearsal of the script, not a measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "report_scores_bench.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_report_scores.py measures on a GPU; none is visible: the numbers stay unmeasured")
    from vimure_amd.residuals import grid_edges, threshold_for_top, top_rows
    L, N, M, K = (2, 200, 40, 2) if a.small else (4, 2000, 200, 2)
    top = 1000
    eng, _, theta, lam, eta = make_engine(L, N, M, K, 1)
    edges = grid_edges()

    def aggregates(e=eng, th=theta, la=lam):
        return e.report_scores(th, la, eta, np.inf, edges=edges, rows=False, by_reporter=False)

    def top_call():
        agg = aggregates()
        thr, _ = threshold_for_top(agg["hist"], agg["edges"], top)
        res = eng.report_scores(theta, lam, eta, thr)
        return thr, top_rows(res, top), int(res["counts"][:, 3].sum())
    agg, t_agg = timed(aggregates, a.repeats)
    (thr, rows, fetched), t_top = timed(top_call, a.repeats)
    support = int(agg["counts"][:, 0].sum())
    sorted_ok = bool((np.diff(rows["logp"]) >= 0).all() and len(rows["logp"]) == min(top, fetched) and (-rows["logp"] >= thr).all())
    fmt = eng.data_format()[0]
    eng.close()

    # the list route, where the list fits
    Ll, Nl = (1, 100) if a.small else (1, a.list_n)
    eng, X, theta, lam, eta = make_engine(Ll, Nl, M, K, 2, keep_x=True)
    walk, t_walk = timed(lambda: aggregates(eng, theta, lam), a.repeats)

    def by_list():
        subs, _ = eng.mean_poisson(device=True)
        l, i, j, m = (s.long() for s in subs)
        x, xt = X[l, i, j, m].int().contiguous(), X[l, j, i, m].int().contiguous()
        return eng.heldout_loglik(tuple(subs), x, xt, theta=theta, lam=lam, eta=eta, device=True)
    lst, t_list = timed(by_list, a.repeats)
    n_list = int(walk["counts"][:, 0].sum())
    same = bool(np.array_equal(walk["counts"][:, :3], lst["counts"][:, :3]) and (lst["counts"][:, 3] == lst["counts"][:, 0]).all()
                and np.allclose(walk["sums"], lst["sums"], rtol=1e-9, atol=0.0))
    eng.close()
    ma, mt, mw, ml = (float(np.median(t)) for t in (t_agg, t_top, t_walk, t_list))
    out = {"case": "small" if a.small else "config3", "L": L, "N": N, "M": M, "K": K, "format": fmt, "repeats": a.repeats,
           "support": support, "edges": len(edges),
           "aggregates_median_ms": ma, "aggregates_all_ms": t_agg, "aggregates_elements_per_s": support / (ma * 1e-3),
           "top": top, "top_threshold": thr, "top_rows_fetched": fetched, "top1000_median_ms": mt, "top1000_all_ms": t_top,
           "top_rows_sorted": sorted_ok,
           "list_shape": [Ll, Nl, Nl, M], "list_entries": n_list, "walk_median_ms": mw, "walk_all_ms": t_walk,
           "walk_elements_per_s": n_list / (mw * 1e-3), "list_median_ms": ml, "list_all_ms": t_list,
           "list_elements_per_s": n_list / (ml * 1e-3), "list_bytes": 40 * n_list,
           "call_note": "whole calls are timed: the per-layer set-up (the tie-major index and the tie -> position table of a "
                        "report-list handle), the passes, the scan, the copies back and the synchronisation",
           "same_results": same}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)
    assert same, "the walk and the list disagree"
    assert sorted_ok, "the top rows are not the sorted rows at or above the threshold"


if __name__ == "__main__":
    main()
