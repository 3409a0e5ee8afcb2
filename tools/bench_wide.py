#!/usr/bin/env python3
"""A survey wider than the 13-bit reporter keys (development aid; run on the GPU box): a synthetic self-reporter edgelist with
N = M = 9000, L = 1, K = 2 and a few thousand edge rows (the reader's mask: 2 (N - 1) entries per reporter, 81 M ties of which
every one with a reporter is a partial row of one or two), fitted through vmr_create_coo and the general kernels.

Prints the time vmr_create_coo takes, then ms per plain sweep and per ELBO sweep -- with the packed two-reporter rows of the
general pass (vmr_ctx::rm2) and without them (VMR_NO_RM2=1, read once at handle creation: the mask-list walk of before) -- and
one JSON line with the same numbers.

    python tools/bench_wide.py [--n 9000] [--rows 5000] [--sweeps 20] [--repeats 3] [--profile]
"""
import argparse
import json
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def survey(N, rows, seed=5):
    """Pairs (2r, 2r + 1) reported by one of them, then edges from the odd nodes reported by their ego (rows in all)."""
    import pandas as pd
    g = np.random.RandomState(seed)
    npair = min(N // 2, rows)
    r = np.arange(npair)
    ego, alter = 2 * r, 2 * r + 1
    rep = np.where(r % 2 == 0, ego, alter)
    extra = max(0, rows - npair)
    e2 = (2 * np.arange(extra) + 1) % N
    a2 = (e2 + 1 + 2 * g.randint(0, max(1, N // 2 - 1), extra)) % N
    ego, alter, rep = np.concatenate([ego, e2]), np.concatenate([alter, a2]), np.concatenate([rep, e2])
    return pd.DataFrame({"reporter": [f"n{v}" for v in rep], "ego": [f"n{v}" for v in ego], "alter": [f"n{v}" for v in alter],
                         "weight": 1, "layer": "L0"})


def timed_sweeps(eng, n, elbo):
    eng.sync()
    t0 = time.perf_counter()
    if elbo:
        for _ in range(n):
            eng.step(1, want_elbo=True)
    else:
        eng.step(n)
    eng.sync()
    return 1e3 * (time.perf_counter() - t0) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=9000)
    ap.add_argument("--rows", type=int, default=5000)
    ap.add_argument("--sweeps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--profile", action="store_true", help="also split a plain sweep by kernel class")
    a = ap.parse_args()
    from vimure_amd import CaviEngine
    from vimure_amd._io import read_from_edgelist
    K = 2
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        net = read_from_edgelist(survey(a.n, a.rows), K=K)
    X, R = net.X, net.R
    L, N, _, M = (int(s) for s in X.shape)
    xs = [np.ascontiguousarray(s, np.int32) for s in X.subs] + [np.ascontiguousarray(X.vals, np.int32)]
    rs = [np.ascontiguousarray(s, np.int32) for s in R.subs]
    print(f"N = M = {N}, L = {L}, K = {K}: {len(X.vals)} reports, {len(R.vals)} mask entries (host build {time.perf_counter() - t0:.1f} s)",
          flush=True)
    g = np.random.RandomState(0)
    pr = 1.0 + 0.01 * g.rand(L, N, N, K)
    pr /= pr.sum(-1)[..., None]
    init = (0.1 + 0.1 * g.rand(L, M), 0.1 + 0.1 * g.rand(L, M), 10 + 10 * g.rand(L, K), 10 + 10 * g.rand(L, K), 0.7,
            1.0 + float(np.sum(X.vals)), pr)
    out = {"N": N, "M": M, "L": L, "K": K, "reports": int(len(X.vals)), "mask_entries": int(len(R.vals))}
    for tag, no_rm2 in (("rm2", False), ("lists", True)):
        if no_rm2:
            os.environ["VMR_NO_RM2"] = "1"
        else:
            os.environ.pop("VMR_NO_RM2", None)
        create = []
        for _ in range(a.repeats):   # (the first creation also pays the library's first-use costs)
            t0 = time.perf_counter()
            eng = CaviEngine.from_coo(xs[:4], xs[4], X.shape, R=rs, K=K, mutuality=True)
            eng.sync()
            create.append(1e3 * (time.perf_counter() - t0))
            if len(create) < a.repeats:
                eng.close()
        eng.set_priors(0.1, 0.1, 10.0, 10.0, 0.5, 1.0)
        eng.set_state(*init)
        eng.step(3)   # (warm-up)
        plain = [timed_sweeps(eng, a.sweeps, False) for _ in range(a.repeats)]
        elbo = [timed_sweeps(eng, max(2, a.sweeps // 2), True) for _ in range(a.repeats)]
        if a.profile:   # where a plain sweep's time goes, per kernel class (HIP events around every launch: a little slower)
            eng.profile(True)
            eng.step(a.sweeps)
            eng.sync()
            prof = {k: v for k, v in eng.profile_read().items() if v["launches"]}
            eng.profile(False)
            out[f"profile_{tag}"] = {k: [round(v["ms"] / a.sweeps, 3), int(v["launches"])] for k, v in prof.items()}
            print(f"{tag:6s} per plain sweep (ms, launches in {a.sweeps} sweeps):", out[f"profile_{tag}"], flush=True)
        eng.close()
        out[f"create_ms_{tag}"] = [round(v, 1) for v in create]
        out[f"plain_ms_{tag}"] = [round(v, 3) for v in plain]
        out[f"elbo_ms_{tag}"] = [round(v, 3) for v in elbo]
        print(f"{tag:6s} vmr_create_coo {min(create):8.1f} ms   plain sweep {min(plain):8.3f} ms (of {plain})   "
              f"ELBO sweep {min(elbo):8.3f} ms", flush=True)
    os.environ.pop("VMR_NO_RM2", None)
    for k in ("plain", "elbo"):
        out[f"{k}_gain"] = round(1.0 - min(out[f"{k}_ms_rm2"]) / min(out[f"{k}_ms_lists"]), 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
