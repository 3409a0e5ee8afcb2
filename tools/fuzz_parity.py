#!/usr/bin/env python3
"""Randomised parity sweep (GPU box): random shapes, K, mutuality, mask kinds, count ranges and engine shapes against the
coordinate-list oracle -- three sweeps with the ELBO each, state compared at the end.  `python tools/fuzz_parity.py [n] [seed] [wide|long|range|seq] [plain]`.
plain (with the standard family, wide or long): some of the three sweeps without the ELBO, consecutive ones as one step(n) or not.
long: many reports per tie with mirrored counts (the sweep's general body, ties sorted by the second key, level-0 rounds), two passes
and far lists forced at random.
range: the rho update where the reference's raw exponentials leave the range of a double (tests/exp_range_util.py: all-zero rows,
subnormal sums, NaN rows) with random K, mask kind, engine shape and layer scales -- one rho update from the drawn state, tie by tie.
seq: a random legal sequence of engine calls (tests/call_sequence_util.py: set_state, step, sub-steps, elbo, sweep_local + commit_nu,
fit_loop, snapshot, restore, refused calls, readers) on a handle of a random kind with N, M and K perturbed within the kind's family,
every call against the host model."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PRI = (0.1, 0.1, 10.0, 10.0, 0.5, 1.0)


def plain_schedule(case):
    """The calls of a `plain` case: [(sweeps, want_elbo)], three sweeps in all.  Its own generator (the case draw stays as it is):
    which sweeps evaluate the ELBO -- at least one does not -- and whether consecutive plain sweeps go as one step(n), whose inner
    rhos are never written."""
    gp = np.random.RandomState(1000003 + case)
    while True:
        flags = [bool(gp.rand() < 0.5) for _ in range(3)]
        if not all(flags):
            break
    group = bool(gp.rand() < 0.5)
    calls = []
    for f in flags:
        if not f and group and calls and not calls[-1][1]:
            calls[-1] = (calls[-1][0] + 1, False)
        else:
            calls.append((1, f))
    return calls


def one(case, g, wide=False, long_=False, plain=False, oracle_only=False):
    """plain: the three sweeps follow `plain_schedule(case)` -- ELBO sweeps compare their ELBO, plain ones nothing; after the last
    sweep the stand-alone ELBO and the state are compared.  A case whose oracle ELBO is NaN at any sweep is no plain case: None.
    oracle_only (no GPU): the case draw and the oracle alone -- True, or None for such a case (how the committed seeds were chosen).
    wide: the inputs beyond the specialised kernels -- K up to 70 (the reference's default K = max(X) + 1 gives such K) and counts
    beyond 11 bits / table rows beyond 2^20 (two-word entries) -- which the general kernels (csrc/sweep_gen.hip) take."""
    from oracle import cavi_coo
    from vimure_amd import CaviEngine
    L = int(g.choice([1, 1, 2, 3]))
    N = int(g.choice([5, 17, 33, 64, 65, 100, 130] if not wide else [5, 17, 33, 64, 65]))
    M = int(g.choice([1, 3, 16, 17, 40, 64, 65, 130]))
    K = int(g.choice([2, 2, 2, 3, 3, 4, 5, 8] if not wide else [2, 3, 9, 12, 16, 21, 33, 70]))
    mut = bool(g.rand() < 0.7)
    dens = float(g.choice([0.01, 0.05, 0.2, 0.5]))
    xmax = int(g.choice([1, 3, 10, 63] if not wide else [3, 40, 120, 255, 3000]))
    if long_:   # 9..40 reports per tie, many of them mirrored (levels >= 1), some ties reported by nearly everybody
        N = int(g.choice([17, 33, 64, 65, 90]))
        M = int(g.choice([64, 65, 130, 300, 640]))
        K = int(g.choice([2, 2, 3, 3, 4, 5, 8]))
        mut = bool(g.rand() < 0.85)
        dens = float(g.choice([10, 14, 19, 30, 40])) / M
        xmax = int(g.choice([1, 2, 3, 6]))
    X = ((g.rand(L, N, N, M) < dens) * g.randint(1, xmax + 1, size=(L, N, N, M))).astype(np.uint8 if xmax <= 255 else np.int32)
    if long_:
        mir = (np.transpose(X, (0, 2, 1, 3)) > 0) & (g.rand(L, N, N, M) < float(g.choice([0.0, 0.3, 0.6])))
        X = np.maximum(X, mir * g.randint(1, xmax + 1, size=(L, N, N, M))).astype(X.dtype)
        heavy = g.rand(L, N, N) < 0.01
        X[heavy] = np.maximum(X[heavy], (g.rand(int(heavy.sum()), M) < 0.9) * g.randint(1, xmax + 1, size=(int(heavy.sum()), M))).astype(X.dtype)
    mk = g.choice(["ones", "none", "random", "sparse", "self"])
    if mk == "none":
        R = None
    elif mk == "ones":
        R = np.ones_like(X)
    elif mk == "random":
        R = (g.rand(L, N, N, M) < 0.7).astype(np.uint8)
    elif mk == "sparse":
        R = (g.rand(L, N, N, M) < 0.03).astype(np.uint8)
    else:   # self-reporter-like: reporter m may report on ties that involve node m
        R = np.zeros_like(X)
        for m in range(min(M, N)):
            R[:, m, :, m] = 1
            R[:, :, m, m] = 1
    env = {}
    fmt = g.choice(["sparse", "dense", "auto"])
    if fmt != "auto":
        env["VMR_FORMAT"] = fmt
    if g.rand() < 0.3:
        env["VMR_ST_TPB"] = str(int(g.choice([64, 256, 1024])))
    if g.rand() < 0.3:
        env.update({"VMR_TWO_PASS": str(int(g.rand() < 0.5)), "VMR_YT": str(int(g.randint(0, 4))), "VMR_HC": str(int(g.randint(0, 4)))})
    if g.rand() < 0.3:
        env["VMR_TPB"] = str(int(g.choice([64, 128, 256, 512, 1024])))
    if long_:
        env["VMR_FORMAT"] = "sparse"
        env.pop("VMR_YT", None); env.pop("VMR_HC", None)
        r = g.rand()
        if r < 0.5:
            env["VMR_TWO_PASS"] = "1"
            if g.rand() < 0.3:
                env["VMR_HC"] = str(int(g.randint(1, 4)))
        elif r < 0.7:
            env["VMR_TWO_PASS"] = "0"
        else:
            env.pop("VMR_TWO_PASS", None)
        if g.rand() < 0.2:
            env["VMR_NO_LEVEL_SORT"] = "1"
        if g.rand() < 0.15:
            env["VMR_NO_LEVEL0"] = "1"
        if g.rand() < 0.15:
            env["VMR_NO_LV0R"] = "1"
    old = {k: os.environ.get(k) for k in ("VMR_FORMAT", "VMR_ST_TPB", "VMR_TWO_PASS", "VMR_YT", "VMR_HC", "VMR_TPB", "VMR_NO_LEVEL_SORT", "VMR_NO_LEVEL0",
                                          "VMR_NO_LV0R")}
    for k in old:
        os.environ.pop(k, None)
    os.environ.update(env)
    desc = f"case {case}: L{L} N{N} M{M} K{K} mut={int(mut)} dens={dens} xmax={xmax} mask={mk} env={env}"
    try:
        use_coo = M <= 8192 and (xmax > 255 or (fmt != "dense" and g.rand() < 0.4))   # the coordinate-list entry point (vmr_create_coo)
        if use_coo:
            desc += " [coo]"
        if oracle_only:
            sx = np.nonzero(X)
            gs = np.random.RandomState(case)
            pr = gs.rand(L, N, N, K) + 0.05
            pr /= pr.sum(-1, keepdims=True)
            init = (0.5 + gs.rand(L, M), 0.5 + gs.rand(L, M), 1 + gs.rand(L, K), 1 + gs.rand(L, K), 0.7, 1.0 + float(X.sum(dtype=np.int64)), pr)
            c = cavi_coo.CooRef((sx, X[sx]), None if R is None else np.nonzero(R), (L, N, N, M), K, mut, PRI, *init)
            for it in range(3):
                c.cavi_step()
                if np.isnan(c.elbo()):
                    return None
            return True
        try:
            if use_coo:
                sx0 = np.nonzero(X)
                eng = CaviEngine.from_coo(sx0, X[sx0], X.shape, R=None if R is None else np.nonzero(R), K=K, mutuality=mut, device=0)
            else:
                eng = CaviEngine(X, R, K=K, mutuality=mut, device=0)
        except ValueError as e:   # a refused combination: the dense tiles forced beyond 8 categories
            print(desc, "-> refused:", str(e)[:80], flush=True)
            return fmt == "dense" and K > 8 and not use_coo
        sum_x, cov = eng.data_stats()
        gs = np.random.RandomState(case)
        pr = gs.rand(L, N, N, K) + 0.05
        pr /= pr.sum(-1, keepdims=True)
        init = (0.5 + gs.rand(L, M), 0.5 + gs.rand(L, M), 1 + gs.rand(L, K), 1 + gs.rand(L, K), 0.7, 1.0 + float(sum_x), pr)
        sx = np.nonzero(X)
        c = cavi_coo.CooRef((sx, X[sx]), None if R is None else np.nonzero(R), (L, N, N, M), K, mut, PRI, *init)
        eng.set_priors(*PRI)
        eng.set_state(*init)
        ok = True
        if plain:
            desc += f" plain={plain_schedule(case)}"
            want_e, nan_at = [], None      # the oracle first: its ELBO after every sweep decides whether this is a plain case
            for n, want in plain_schedule(case):
                for _ in range(n):
                    c.cavi_step()
                    ec = c.elbo()
                    nan_at = len(want_e) + 1 if (np.isnan(ec) and nan_at is None) else nan_at
                    want_e.append(ec)
            if nan_at is not None:
                print(desc, f"-> no plain case: the oracle's ELBO is NaN at sweep {nan_at}", flush=True)
                eng.close()
                return None
            it = 0
            for n, want in plain_schedule(case):
                it += n
                ec = want_e[it - 1]
                e = eng.step(n, want_elbo=want)
                if want and not abs(e - ec) <= 1e-9 * max(1.0, abs(ec)):
                    ok = False
                    print(desc, f"-> ELBO mismatch at sweep {it}: {e} vs {ec}", flush=True)
                    break
            if ok:
                e = eng.elbo()
                if not abs(e - ec) <= 1e-9 * max(1.0, abs(ec)):
                    ok = False
                    print(desc, f"-> stand-alone ELBO mismatch after sweep {it}: {e} vs {ec}", flush=True)
        for it in range(0 if plain else 3):
            c.cavi_step()
            ec = c.elbo()
            try:
                e = eng.step(1, want_elbo=True)
            except ValueError as ex:   # "ELBO is NaN!!!!" (model.py:1015-1016): fine when the oracle's is NaN too
                if np.isnan(ec):
                    print(desc, f"-> both NaN at sweep {it + 1}", flush=True)
                    eng.close()
                    return True
                ok = False
                print(desc, f"-> GPU raised '{ex}' at sweep {it + 1}, oracle ELBO {ec}", flush=True)
                break
            if not abs(e - ec) <= 1e-9 * max(1.0, abs(ec)):
                ok = False
                print(desc, f"-> ELBO mismatch at sweep {it + 1}: {e} vs {ec}", flush=True)
                break
        if ok:
            st = eng.get_state()
            for name in ("gamma_shp", "gamma_rte", "phi_shp", "phi_rte"):
                a, b = st[name], getattr(c, name)
                if not np.allclose(a, b, rtol=1e-9, atol=1e-12):
                    ok = False
                    print(desc, f"-> {name} mismatch {np.max(np.abs(a - b) / (np.abs(b) + 1e-300)):.3e}", flush=True)
            if not np.allclose(st["rho"], c.rho, rtol=1e-7, atol=1e-12):
                ok = False
                print(desc, f"-> rho mismatch {np.max(np.abs(st['rho'] - c.rho)):.3e}", flush=True)
        fmt_used = eng.data_format()[0]
        eng.close()
        if ok:
            print(desc, "->", fmt_used, "ok", flush=True)
        return ok
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def one_range(case, g):
    """The builder of tests/exp_range_util.py with random K, mask kind, large counts or none, engine shape and scales of the two
    layers' E[theta]; rho after one update against the oracle band by band (the subnormal-sum bound 2u (1 + K rho) / S included, with
    the argument term of exp_range_util.argument_bound where S > 2^43 u: a random draw may put rows there that the exp bound alone
    cannot cover), then nu, gamma and phi from that rho -- relative 1e-9 where the oracle is finite, the same NaN entries where it
    is not.  Returns True / False, or None for a draw that is no case: a tie at an edge that last bits would decide."""
    from tests import exp_range_util as u
    from vimure_amd import CaviEngine, _lib
    K = int(g.choice([2, 2, 3, 4, 5, 8, 9, 16]))
    mask = str(g.choice(["partial", "ones"]))
    kind = str(g.choice(["finite", "overflow"]))
    seed = int(g.randint(1, 1 << 20))
    X, R, pri, st = u.build_case(K, mask, seed, kind)
    # layer 0 stays mild, layer 1 around the edges of the range: under a partial mask T differs tie by tie and any scale leaves
    # ties on both sides; under the all-ones mask T E[lambda] is one number, 752 min_k at scale 1 -- 0.95..1.1 keeps the ties
    # without reports between subnormal sums (714) and all zero (827) and those with reports straddling the lower edge
    scale = np.array([g.uniform(0.5, 2.0), g.uniform(0.95, 1.1) if mask == "ones" else g.uniform(0.7, 1.5)])
    st = (st[0] * scale[:, None],) + tuple(st[1:])
    env = {}
    if K <= 8:
        fmt = str(g.choice(["sparse", "sparse", "dense"]))
        env["VMR_FORMAT"] = fmt
        if fmt == "sparse":
            r = g.rand()
            if r < 0.35:
                env["VMR_TWO_PASS"] = "1"
                for name in ("VMR_NO_LEVEL0", "VMR_NO_X0", "VMR_NO_LV0R"):
                    if g.rand() < 0.2:
                        env[name] = "1"
            elif r < 0.6:
                env.update({"VMR_TWO_PASS": "0", "VMR_YT": str(int(g.randint(0, 3))), "VMR_HC": str(int(g.randint(0, 3)))})
            if K == 2 and g.rand() < 0.3:
                env["VMR_NO_LPD"] = "1"
            if g.rand() < 0.3:
                env["VMR_TPB"] = str(int(g.choice([64, 128, 256, 512])))
    names = ("VMR_FORMAT", "VMR_TWO_PASS", "VMR_YT", "VMR_HC", "VMR_NO_LEVEL0", "VMR_NO_X0", "VMR_NO_LV0R", "VMR_NO_LPD", "VMR_TPB")
    old = {k: os.environ.get(k) for k in names}
    for k in names:
        os.environ.pop(k, None)
    os.environ.update(env)
    use_coo = bool(g.rand() < 0.3) and env.get("VMR_FORMAT") != "dense"
    desc = f"case {case}: range K{K} mask={mask} {kind} seed={seed} scale={scale.round(3).tolist()} env={env}" + (" [coo]" if use_coo else "")
    try:
        a, mag = u.log_rho(X, R, st, magnitude=True)
        band, rho_np, S = u.bands(a)
        d_zero, d_max, dec = u.edge_distances(a, rho_np)
        if d_zero <= 1e-6 or d_max <= 1e-6 or dec <= 1.0:   # last bits of exp would decide a tie's band: not a case (the conditions
            print(desc, f"-> skipped: a tie at an edge ({d_zero:.2g}, {d_max:.2g}, {dec:.2g})", flush=True)   # of tests/test_exp_range_host.py)
            return None
        c = u.coo_oracle(X, R, K, pri, st)
        if use_coo:
            sx = np.nonzero(X)
            eng = CaviEngine.from_coo(sx, X[sx], X.shape, R=np.nonzero(R), K=K, mutuality=True, device=0)
        else:
            eng = CaviEngine(X, R, K=K, mutuality=True, device=0)
        eng.set_priors(*pri)
        eng.set_state(*st)
        eng.sub_step(_lib.STEP_RHO)
        c.update_rho()
        ok = True
        try:
            u.assert_rho(eng.get_state(rho=True)["rho"], c.rho, band, S, K, what="rho", mag=mag)
        except AssertionError as ex:
            ok = False
            print(desc, "->", str(ex).strip().splitlines()[0], flush=True)
        for step, upd, names_ in ((_lib.STEP_NU, c.update_nu, ("nu_shp",)), (_lib.STEP_GAMMA, c.update_gamma, ("gamma_shp", "gamma_rte")),
                                  (_lib.STEP_PHI, c.update_phi, ("phi_shp", "phi_rte"))):
            eng.sub_step(step)
            upd()
            got = eng.get_state(rho=False)
            for n in names_:
                a, b = np.asarray(got[n], dtype=float), np.asarray(getattr(c, n), dtype=float)
                fin = np.isfinite(b)
                if not np.array_equal(np.isnan(a), np.isnan(b)) or not np.allclose(a[fin], b[fin], rtol=1e-9, atol=0.0):
                    ok = False
                    print(desc, f"-> {n} mismatch", flush=True)
        counts = [int((band == b).sum()) for b in range(5)]
        fmt_used = eng.data_format()[0]
        eng.close()
        if ok:
            print(desc, "->", fmt_used, dict(zip(u.BAND_NAMES, counts)), "ok", flush=True)
        return ok
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def one_seq(case, g):
    """Handle kind, shape perturbation and a sequence of 20 to 40 operations at random; True / False."""
    from tests import call_sequence_util as u
    kind = str(g.choice(list(u.KINDS)))
    spec = u.KINDS[kind]
    n0, m0 = u.SHAPES[spec["data"]]
    N = n0 + int(g.randint(-6, 7))
    M = N if spec["data"] == "self" else m0 + int(g.randint(-5, 6))      # (lists_two_pass draws M on both sides of 64, one mask word and two)
    K = spec["K"] if spec["K"] in (2, 9) else int(g.choice([3, 4, 5]))
    K = int(g.choice([9, 12, 16])) if spec["K"] == 9 else K
    seed, n_ops = int(g.randint(1 << 20)), int(g.randint(20, 41))
    X, R = u.build_data(spec["data"], seed=seed, N=N, M=M)
    ops = u.draw_sequence(seed, kind, n_ops=n_ops)
    desc = f"case {case}: seq {kind} N{N} M{M} K{K} seed={seed} ops={n_ops}"
    old = {k: os.environ.get(k) for k in u.SWITCHES}
    for k in old:
        os.environ.pop(k, None)
    os.environ.update(spec["env"])
    try:
        try:
            u.run_sequence(kind, ops, X, R, K=K, label=desc)
        except AssertionError as ex:
            print(desc, "->", str(ex).strip().splitlines()[0][:400], flush=True)
            return False
        print(desc, "-> ok", flush=True)
        return True
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    wide = len(sys.argv) > 3 and sys.argv[3] == "wide"
    long_ = len(sys.argv) > 3 and sys.argv[3] == "long"
    range_ = len(sys.argv) > 3 and sys.argv[3] == "range"
    seq = len(sys.argv) > 3 and sys.argv[3] == "seq"
    g = np.random.RandomState(seed)
    t0 = time.time()
    plain = "plain" in sys.argv[3:]
    res = [(one_seq(i, g) if seq else one_range(i, g) if range_ else one(i, g, wide, long_, plain)) for i in range(n)]
    bad = sum(1 for r in res if r is not None and not r)
    print(f"{n} cases, {bad} failed, {sum(1 for r in res if r is None)} skipped, {time.time() - t0:.0f} s", flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
