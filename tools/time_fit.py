#!/usr/bin/env python3
"""Where `VimureModel.fit` spends its time on BASELINE config 3 (development aid; run on the GPU box), with the initial rho prior
drawn on the host (the default) and on the device (`fit(init_on_device=True)`).

    python tools/time_fit.py [--wide] [--json OUT]

--wide also times the start of a fit of tools/bench_wide.py's 9000-node survey at K = 2 and K = 11, in both modes: the initial
state (prior + gammas + vmr_set_state) and the first sweep after it.  Ends with one JSON line of every number."""
import argparse
import json
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from vimure_amd import CaviEngine, VimureModel
from vimure_amd import _hostlib
from vimure_amd.synthetic import standard_sbm


def _fit(eng, X, K, R, on_device):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = VimureModel(mutuality=True)
        t = time.perf_counter()
        m.fit(X, K=K, seed=1, engine=eng, num_realisations=R, max_iter=500, init_on_device=on_device)
        return m, time.perf_counter() - t


def _draw_call(eng, L, N, K, undirected, reps=5):
    """Wall time of the host walk (mt_block_states) and of one vmr_draw_pr_rho call (state upload, kernels, synchronise)."""
    walk, draw = [], []
    for r in range(reps + 1):
        p = np.random.RandomState(1 + r)
        t = time.perf_counter()
        blocks = _hostlib.mt_block_states(p, L, N, K)
        t1 = time.perf_counter()
        eng.draw_pr_rho(blocks, 0.0, undirected)
        t2 = time.perf_counter()
        if r:   # (the first call also allocates the device slot and loads the kernels)
            walk.append(t1 - t)
            draw.append(t2 - t1)
    return {"blocks": int(len(blocks[2])), "walk_s": float(np.median(walk)), "draw_call_s": float(np.median(draw))}


def config3(out):
    L, N, M, K = 4, 2000, 200, 2
    net = standard_sbm(N=N, M=M, L=L, K=K, C=2, avg_degree=5.0, sparsify=True, eta=0.5, seed=0, device="cuda:0")
    eng = CaviEngine(net.X, None, K=K, mutuality=True, device=0)
    sum_x, cov = eng.data_stats()
    t = time.perf_counter(); buf = eng.staging(0); print("pinned staging alloc %.3f s" % (time.perf_counter() - t))
    p = np.random.RandomState(1)
    t = time.perf_counter(); _hostlib.draw_pr_rho(p, (L, N, N, K), 0.0, cov, out=buf); print("C draw into pinned %.3f s" % (time.perf_counter() - t))
    p = np.random.RandomState(1)
    t = time.perf_counter(); u = p.rand(L, N, N, K); print("numpy rand alone %.3f s" % (time.perf_counter() - t))
    del u
    for und in (False, True):
        d = _draw_call(eng, L, N, K, und)
        out[f"config3_draw{'_undirected' if und else ''}"] = d
        print(f"device draw{' (undirected)' if und else ''}: {d['blocks']} blocks, host walk {d['walk_s'] * 1e3:.1f} ms, "
              f"vmr_draw_pr_rho {d['draw_call_s'] * 1e3:.2f} ms", flush=True)
    for on_dev in (False, True):
        mode = "device" if on_dev else "host"
        for R in (1, 1, 5):   # (the first R = 1 fit warms the mode up)
            m, dt = _fit(eng, net.X, K, R, on_dev)
            assert m.pr_rho_drawn_on == mode
            print("%-6s fit R=%d: %.3f s  (loops %.3f s, waited for states %.3f s), iterations %s" % (
                mode, R, dt, m.loop_seconds, m.draw_seconds, m.trace.groupby("realisation")["iter"].max().tolist()), flush=True)
            out[f"config3_{mode}_R{R}"] = {"fit_seconds": dt, "loop_seconds": m.loop_seconds, "draw_seconds": m.draw_seconds,
                                           "maxL": float(m.maxL)}
    eng.close()


def wide(out):
    from tools.bench_wide import survey
    from vimure_amd._io import read_from_edgelist
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = read_from_edgelist(survey(9000, 5000), K=2)
    X, R = net.X, net.R
    L, N, _, M = (int(s) for s in X.shape)
    for K in (2, 11):
        eng = CaviEngine.from_coo(X.subs, np.asarray(X.vals, np.int64), (L, N, N, M), R=R.subs, K=K, mutuality=True)
        sum_x, cov = eng.data_stats()
        eng.set_priors(0.1, 0.1, 10.0, 10.0, 0.5, 1.0)
        for on_dev in (True, False):
            mode = "device" if on_dev else "host"
            m = VimureModel(mutuality=True)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                m._check_fit_params(X, (10.0, 10.0), (0.1, 0.1), (0.5, 1.0), None, 1, R=R, K=K, engine=eng)
            m.sumX = sum_x
            eng.sync()
            t0 = time.perf_counter()
            if on_dev:
                pr = eng.draw_pr_rho(_hostlib.mt_block_states(m.prng, L, N, K), 0.0, False)
            else:
                pr = m._draw_pr_rho(cov, 0.0)
            st = m._draw_gammas(sum_x)
            t1 = time.perf_counter()
            eng.set_state(st["gamma_shp"], st["gamma_rte"], st["phi_shp"], st["phi_rte"], st["nu_shp"], st["nu_rte"], pr)
            t2 = time.perf_counter()
            eng.step(1)
            eng.sync()
            t3 = time.perf_counter()
            del pr
            r = {"prior_s": t1 - t0, "set_state_s": t2 - t1, "to_first_sweep_s": t2 - t0, "first_sweep_s": t3 - t2}
            out[f"wide_K{K}_{mode}"] = r
            print(f"9000-node survey K = {K:2d} {mode:6s}: prior {r['prior_s']:.3f} s, set_state {r['set_state_s']:.3f} s, "
                  f"to the first sweep {r['to_first_sweep_s']:.3f} s, first sweep {r['first_sweep_s']:.3f} s", flush=True)
        eng.close()
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wide", action="store_true", help="also the 9000-node survey at K = 2 and K = 11")
    ap.add_argument("--json", help="also write the JSON line to this file")
    a = ap.parse_args()
    out = {}
    config3(out)
    if a.wide:
        wide(out)
    line = json.dumps(out)
    print(line, flush=True)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
