"""GPU: the rho update where the reference's raw exponentials leave the range of a double, held to the oracle tie by tie.

The reference takes exp(a_k) without max-subtraction and normalises only where the sum is positive (model.py:807-811): all-zero
rows where everything underflows, NaN where something overflows.  The engine reproduces that with K - 1 accumulated categories and
per-tie deficits D = x (1 - sum rho), the K = 2 bounds test and its literal code, the `tame` switch of K >= 3, and copies of the
literal update in the dense and the general kernels.  tests/exp_range_util.py builds the cases (L = 2, N = 48, M = 64: ties of every
band inside single waves) and classifies the ties; tests/test_exp_range_host.py shows on the CPU that the cases are what they claim.

Tolerances: rho relative 1e-9 + absolute 1e-13 on safe and literal rows, exact zeros, equal NaN masks, 2u (1 + K rho) / S on rows
with a subnormal sum S (u = 2^-1074: two exp implementations, each within one unit); gamma, phi, nu relative 1e-9; the stand-alone
ELBO relative 1e-10, the ELBO of a sweep 1e-9."""
import functools

import numpy as np
import pytest

from tests import exp_range_util as u

pytestmark = pytest.mark.gpu

RTOL = 1e-9
SWITCHES = ("VMR_FORMAT", "VMR_NO_LPD", "VMR_TWO_PASS", "VMR_YT", "VMR_HC", "VMR_FARL", "VMR_NO_LEVEL0", "VMR_NO_X0", "VMR_NO_LV0R",
            "VMR_DETERMINISTIC", "VMR_DEBUG_LAZY_RHO", "VMR_TPB", "VMR_ST_TPB")
LISTS = {"VMR_FORMAT": "sparse"}
TWO_PASS = dict(LISTS, VMR_TWO_PASS="1")
# name -> (environment, expected (passes, levels) of sweep_shape(); None: not asserted)
SHAPES = {
    "lists": (LISTS, (1, None)),
    "no_lpd": (dict(LISTS, VMR_NO_LPD="1"), (1, None)),
    "two_pass": (TWO_PASS, (2, None)),
    "one_pass_no_levels": (dict(LISTS, VMR_TWO_PASS="0", VMR_YT="0", VMR_HC="0"), (1, 0)),
    # far lists are only chosen for N > 1024 (vmr_create): at this size VMR_FARL=1 leaves one pass that keeps two levels in LDS and
    # adds the reports of the levels beyond to global memory itself -- the far-list kernel is not reached at any M
    "farl_two_levels": (dict(LISTS, VMR_FARL="1", VMR_YT="2", VMR_HC="2"), (1, 2)),
    "two_pass_no_level0": (dict(TWO_PASS, VMR_NO_LEVEL0="1"), (2, None)),
    "two_pass_no_x0": (dict(TWO_PASS, VMR_NO_X0="1"), (2, None)),
    "two_pass_no_lv0r": (dict(TWO_PASS, VMR_NO_LV0R="1"), (2, None)),
    "dense": ({"VMR_FORMAT": "dense"}, None),
    "general": ({}, None),
    "general_coo": ({}, None),
}
LEGS = ([("lists", K, mask) for K in (2, 3, 5, 8) for mask in ("partial", "ones")]
        + [("no_lpd", 2, mask) for mask in ("partial", "ones")]
        + [(s, K, "partial") for s in ("two_pass", "one_pass_no_levels", "farl_two_levels", "two_pass_no_level0", "two_pass_no_x0",
                                       "two_pass_no_lv0r") for K in (2, 3)]
        + [("two_pass", 5, "ones"), ("one_pass_no_levels", 8, "ones")]
        + [("dense", K, mask) for K in (2, 3, 5) for mask in ("partial", "ones")]
        + [(s, K, mask) for s in ("general", "general_coo") for K in (9, 16) for mask in ("partial", "ones")])


def _env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _engine(X, R, K, pri, st, shape="lists", mutuality=True):
    from vimure_amd import CaviEngine
    if shape == "general_coo":
        sx = np.nonzero(X)
        eng = CaviEngine.from_coo(sx, X[sx], X.shape, R=np.nonzero(R), K=K, mutuality=mutuality)
    else:
        eng = CaviEngine(X, R, K=K, mutuality=mutuality)
    fmt = eng.data_format()[0]
    assert fmt == ("dense" if shape == "dense" else "sparse"), fmt
    want = SHAPES[shape][1]
    if want is not None:
        passes, levels, far = eng.sweep_shape()
        assert passes == want[0] and (want[1] is None or levels == want[1]), (shape, passes, levels, far)
        assert far == 0, (shape, far)   # no leg is on the far-list kernel: a change of its threshold must not move one there unseen
    eng.set_priors(*pri)
    eng.set_state(*st)
    return eng


@functools.lru_cache(maxsize=None)
def _reference(K, mask, kind, mutuality=True):
    """The oracle's sub-steps from the case's state, computed once per case and shared (read-only) by every engine shape."""
    X, R, pri, st = u.build_case(K, mask, 1, kind)
    if not mutuality:   # (nu as the reference sets it without mutuality, model.py:596-600)
        st = st[:4] + (1e-6, 1.0) + st[6:]
    band, _, S = u.bands(u.log_rho(X, R, st, mutuality))
    c = u.coo_oracle(X, R, K, pri, st, mutuality)
    ref = {"X": X, "R": R, "pri": pri, "st": st, "band": band, "S": S}
    c.update_rho()
    ref["rho"] = c.rho.copy()
    g_nu_before = c.s.g_nu_cache
    c.update_nu()
    ref["nu_shp"] = c.nu_shp
    c.update_gamma()
    ref["gamma_shp"], ref["gamma_rte"] = c.gamma_shp.copy(), c.gamma_rte.copy()
    c.update_phi()
    ref["phi_shp"], ref["phi_rte"] = c.phi_shp.copy(), c.phi_rte.copy()
    # The engine's stand-alone ELBO takes exp(E[log nu]) from before the last nu update: what the reference's cache holds at the
    # end of a sweep (model.py:684, :970).  In this order the oracle's gamma and phi updates have refreshed the cache after nu.
    c.s.g_nu_cache = g_nu_before
    ref["elbo"] = c.elbo()
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def _close(got, want, name):
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=0.0, err_msg=name)


def _substeps(eng, ref, K, kind, what):
    from vimure_amd import _lib
    eng.sub_step(_lib.STEP_RHO)
    rho = eng.get_state(rho=True)["rho"]
    u.assert_rho(rho, ref["rho"], ref["band"], ref["S"], K, rtol=RTOL, atol=1e-13, what=what)
    seq = ((_lib.STEP_NU, ("nu_shp",)), (_lib.STEP_GAMMA, ("gamma_shp", "gamma_rte")), (_lib.STEP_PHI, ("phi_shp", "phi_rte")))
    for step, names in seq:
        eng.sub_step(step)
        g = eng.get_state(rho=False)
        for n in names:
            if kind == "overflow":   # NaN rows are arithmetic: the same entries are NaN, nothing more is asked
                assert np.array_equal(np.isnan(g[n]), np.isnan(ref[n])), f"{what}: NaN pattern of {n}"
            else:
                _close(g[n], ref[n], f"{what}: {n}")
    if np.isnan(ref["elbo"]):
        with pytest.raises(ValueError):
            eng.elbo()
    else:
        e = eng.elbo()
        assert abs(e - ref["elbo"]) <= 1e-10 * max(1.0, abs(ref["elbo"])), (what, e, ref["elbo"])
    return rho


@pytest.mark.parametrize("kind", ["finite", "overflow"])
@pytest.mark.parametrize("shape,K,mask", LEGS)
def test_substeps_on_every_band(shape, K, mask, kind, monkeypatch):
    """set_state, rho, nu, gamma, phi, ELBO -- each against the oracle's update from the same rho, in every engine shape."""
    _env(monkeypatch, SHAPES[shape][0])
    ref = _reference(K, mask, kind)
    assert (ref["band"][1] == u.ZERO).sum() >= 230 and (ref["band"][1] == u.SUBNORMAL).sum() >= 5
    assert np.isnan(ref["elbo"]) == (kind == "overflow")
    eng = _engine(ref["X"], ref["R"], K, ref["pri"], ref["st"], shape)
    _substeps(eng, ref, K, kind, f"{shape} K={K} {mask} {kind}")
    eng.close()


@pytest.mark.parametrize("kind", ["finite", "overflow"])
def test_substeps_mutuality_off(kind, monkeypatch):
    _env(monkeypatch, LISTS)
    ref = _reference(3, "partial", kind, False)
    eng = _engine(ref["X"], ref["R"], 3, ref["pri"], ref["st"], "lists", mutuality=False)
    from vimure_amd import _lib
    eng.sub_step(_lib.STEP_RHO)
    u.assert_rho(eng.get_state(rho=True)["rho"], ref["rho"], ref["band"], ref["S"], 3, rtol=RTOL, atol=1e-13, what="mutuality off")
    for step, names in ((_lib.STEP_GAMMA, ("gamma_shp", "gamma_rte")), (_lib.STEP_PHI, ("phi_shp", "phi_rte"))):
        eng.sub_step(step)
        g = eng.get_state(rho=False)
        for n in names:
            if kind == "overflow":
                assert np.array_equal(np.isnan(g[n]), np.isnan(ref[n])), n
            else:
                _close(g[n], ref[n], n)
    if kind == "finite":   # (the ELBO carries the constant -5e5 of the nu term here: an absolute bound, as tests/test_hip_configs.py)
        assert abs(eng.elbo() - ref["elbo"]) <= 1e-6
    eng.close()


@pytest.mark.parametrize("shape,K,mask", [("lists", 2, "partial"), ("lists", 3, "ones"), ("two_pass", 3, "partial"), ("dense", 5, "partial"),
                                          ("general", 9, "partial")])
def test_prior_rows_that_do_not_sum_to_one(shape, K, mask, monkeypatch):
    """A user-supplied prior with rows short of 1 and all-zero rows: rho = pr_rho carries deficits before any rho update -- the
    first gamma and phi after set_state, then the rest of the sweep, and one fused sweep from the same state."""
    from vimure_amd import _lib
    _env(monkeypatch, SHAPES[shape][0])
    X, R, pri, st = u.build_case(K, mask, 1, "prior")
    assert (np.abs(st[6].sum(axis=-1) - 1.0) > 0.05).mean() > 0.05 and (st[6].sum(axis=-1) == 0).sum() >= 5
    c = u.coo_oracle(X, R, K, pri, st)
    eng = _engine(X, R, K, pri, st, shape)
    eng.sub_step(_lib.STEP_GAMMA)
    c.update_gamma()
    g = eng.get_state(rho=False)
    _close(g["gamma_shp"], c.gamma_shp, "first gamma_shp")
    _close(g["gamma_rte"], c.gamma_rte, "first gamma_rte")
    eng.sub_step(_lib.STEP_PHI)
    c.update_phi()
    g = eng.get_state(rho=False)
    _close(g["phi_shp"], c.phi_shp, "first phi_shp")
    _close(g["phi_rte"], c.phi_rte, "first phi_rte")
    # one full sweep from the same state
    eng.set_state(*st)
    c = u.coo_oracle(X, R, K, pri, st)
    e = eng.step(1, want_elbo=True)
    c.cavi_step()
    e_cpu = c.elbo()
    assert abs(e - e_cpu) <= 1e-9 * max(1.0, abs(e_cpu)), (e, e_cpu)
    g = eng.get_state(rho=False)
    for n in ("gamma_shp", "gamma_rte", "phi_shp", "phi_rte"):
        _close(g[n], getattr(c, n), n)
    _close(g["nu_shp"], c.nu_shp, "nu_shp")
    eng.close()


@pytest.mark.parametrize("shape,K,mask", [("lists", 2, "partial"), ("lists", 3, "ones"), ("dense", 2, "partial"), ("general", 9, "partial")])
def test_readout_on_irregular_rows(shape, K, mask, monkeypatch):
    """argmax, threshold and get_state after the rho step equal NumPy on the oracle's rho, all-zero rows included (report lists
    keep rho by sorted position: the read-outs go back through the permutation).  Rows whose two largest entries are closer than
    their tolerance are compared through the device's own rho; no all-zero, safe or literal row is among them."""
    from vimure_amd import _lib
    _env(monkeypatch, SHAPES[shape][0])
    ref = _reference(K, mask, "finite")
    eng = _engine(ref["X"], ref["R"], K, ref["pri"], ref["st"], shape)
    eng.sub_step(_lib.STEP_RHO)
    rho = eng.get_state(rho=True)["rho"]
    u.assert_rho(rho, ref["rho"], ref["band"], ref["S"], K, rtol=RTOL, atol=1e-13, what="get_state")
    top = np.sort(ref["rho"], axis=-1)
    s_pos = np.where(ref["S"] > 0, ref["S"], 1.0)
    tol = np.where(ref["band"] == u.SUBNORMAL, u.subnormal_bound(ref["rho"], s_pos, K).max(axis=-1), RTOL * top[..., -1] + 1e-13)
    clear = (top[..., -1] - top[..., -2] > 2 * tol) | (ref["band"] == u.ZERO)
    assert clear[ref["band"] != u.SUBNORMAL].all()
    y = eng.readout("rho_max")
    assert np.array_equal(y, np.argmax(rho, axis=-1))
    assert np.array_equal(y[clear], np.argmax(ref["rho"], axis=-1)[clear])
    assert not y[ref["band"] == u.ZERO].any()
    for thr in (0.0, 0.3, 0.5):
        t = eng.readout("threshold", thr)
        assert np.array_equal(t, (rho[..., 1] >= thr).astype(np.uint8))
        far = np.abs(ref["rho"][..., 1] - thr) > 2 * tol
        assert np.array_equal(t[far], (ref["rho"][..., 1] >= thr).astype(np.uint8)[far])
    eng.close()


# ------------------------------------------------------------------------------------------------------------------------------
# whole sweeps: the strong priors keep a share of the rows all zero sweep after sweep (tests/test_exp_range_host.py)
# ------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _sweep_reference(K, mask="partial", seed=1):
    """Three sweeps of the oracle: the ELBO after each, and the state after the third with the bands of its last rho update."""
    X, R, pri, st = u.build_case(K, mask, seed, "sweep")
    c = u.coo_oracle(X, R, K, pri, st)
    elbos = []
    for it in range(3):
        if it < 2:
            c.cavi_step()
        else:   # the same four updates one by one, to classify the ties of the last rho update
            c.update_gamma()
            c.update_phi()
            mid = (c.gamma_shp.copy(), c.gamma_rte.copy(), c.phi_shp.copy(), c.phi_rte.copy(), c.nu_shp, st[5], st[6])
            band, _, S = u.bands(u.log_rho(X, R, mid))
            c.update_rho()
            c.update_nu()
        elbos.append(c.elbo())
    assert (band == u.ZERO).mean() > 0.5
    return {"X": X, "R": R, "pri": pri, "st": st, "elbos": elbos, "c": c, "band": band, "S": S}


def _assert_sweep_state(st, ref, K):
    """The bounds of tests/test_hip_configs.py::_assert_state; rows whose sum is subnormal get the exp bound on top."""
    c, band = ref["c"], ref["band"]
    tol = 1e-7 * np.abs(c.rho) + 1e-12 + np.where((band == u.SUBNORMAL)[..., None], u.subnormal_bound(c.rho, np.where(ref["S"] > 0, ref["S"], 1.0), K), 0.0)
    assert np.array_equal(st["rho"] == 0, c.rho == 0), "zero pattern"
    assert (np.abs(st["rho"] - c.rho) <= tol).all(), float(np.abs(st["rho"] - c.rho).max())
    for n in ("gamma_shp", "gamma_rte", "phi_shp", "phi_rte"):
        _close(st[n], getattr(c, n), n)
    _close(st["nu_shp"], c.nu_shp, "nu_shp")


def _two_legs(K, ref, shape="lists"):
    """Three ELBO sweeps, then from the same start one ELBO sweep and two plain ones (the K - 1 + deficit statistics without the
    ELBO variants): every ELBO and the final state of both legs against the oracle.  Returns the legs' ELBOs and states."""
    out = []
    for leg in ("elbo", "plain"):
        eng = _engine(ref["X"], ref["R"], K, ref["pri"], ref["st"], shape)
        if leg == "elbo":
            es = [eng.step(1, want_elbo=True) for _ in range(3)]
        else:
            es = [eng.step(1, want_elbo=True)]
            eng.step(2)
        for e, e_cpu in zip(es, ref["elbos"]):
            assert abs(e - e_cpu) <= 1e-9 * max(1.0, abs(e_cpu)), (leg, es, ref["elbos"])
        st = eng.get_state(rho=True)
        _assert_sweep_state(st, ref, K)
        if leg == "plain":
            e_cpu = ref["elbos"][2]
            assert abs(eng.elbo() - e_cpu) <= 1e-9 * max(1.0, abs(e_cpu))
        out.append((es, st))
        eng.close()
    return out


@pytest.mark.parametrize("shape,K", [("lists", 2), ("lists", 3), ("two_pass", 2), ("two_pass", 3)])
def test_whole_sweeps_keep_zero_rows(shape, K, monkeypatch):
    _env(monkeypatch, SHAPES[shape][0])
    _two_legs(K, _sweep_reference(K), shape)


def _same(a, b):
    for (ea, sa), (eb, sb) in zip(a, b):
        assert ea == eb
        for k in ("gamma_shp", "gamma_rte", "phi_shp", "phi_rte", "nu_shp", "rho"):
            assert np.array_equal(np.asarray(sa[k]), np.asarray(sb[k])), k


@pytest.mark.parametrize("K", [2, 3])
def test_whole_sweeps_deterministic_and_lazy_rho(K, monkeypatch):
    """VMR_DETERMINISTIC=1 (the deficits added in fixed point): against the oracle, twice for bit equality, and with
    VMR_DEBUG_LAZY_RHO=1 (no plain sweep writes rho; the re-run replays it) bit-identical again."""
    ref = _sweep_reference(K)
    _env(monkeypatch, dict(LISTS, VMR_DETERMINISTIC="1"))
    a = _two_legs(K, ref)
    b = _two_legs(K, ref)
    _same(a, b)
    _env(monkeypatch, dict(LISTS, VMR_DETERMINISTIC="1", VMR_DEBUG_LAZY_RHO="1"))
    _same(a, _two_legs(K, ref))


@pytest.mark.parametrize("K", [2, 3])
def test_lockstep_loop_keeps_zero_rows(K, monkeypatch):
    """fit_loop_batch over three such handles (from_coo, as tests/test_hip_lockstep.py), each with its own reports, mask, prior rows
    and state (seeds 1, 2, 3 of the whole-sweep cases) and held to its own oracle leg: a workgroup of the shared launches that took
    another unit's tables, deficits or parameters would show.  Three iterations; the loop returns the ELBO of the last.
    The lockstep branch itself cannot be observed from outside (profiling bypasses it): the handles are asserted to be what
    vmr_fit_loop_batch takes into it -- report lists, one pass, no far lists, listed mask rows, no switch set."""
    from vimure_amd import CaviEngine
    _env(monkeypatch, {})
    refs = [_sweep_reference(K, "partial", seed) for seed in (1, 2, 3)]
    assert not np.array_equal(refs[0]["X"], refs[1]["X"]) and not np.array_equal(refs[1]["R"], refs[2]["R"])
    assert len({r["elbos"][2] for r in refs}) == 3
    engs = []
    for ref in refs:
        X, R = ref["X"], ref["R"]
        sx = np.nonzero(X)
        eng = CaviEngine.from_coo(sx, X[sx], X.shape, R=np.nonzero(R), K=K, mutuality=True)
        passes, levels, far = eng.sweep_shape()
        assert eng.data_format()[0] == "sparse" and passes == 1 and far == 0 and eng.mask_format()[0] == "lists"
        eng.set_priors(*ref["pri"])
        eng.set_state(*ref["st"])
        engs.append(eng)
    res = CaviEngine.fit_loop_batch(engs, 3, 1e-300, 100)
    for eng, ref, (rows, elbo, its, conv) in zip(engs, refs, res):
        assert its == 3 and not conv
        e_cpu = ref["elbos"][2]
        assert abs(elbo - e_cpu) <= 1e-9 * max(1.0, abs(e_cpu)), (elbo, e_cpu)
        _assert_sweep_state(eng.get_state(rho=True), ref, K)
        eng.close()
