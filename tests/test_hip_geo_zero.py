"""GPU: sweeps where a geometric expectation is exactly 0 (the reference's 0 / 0 -> 0 rule, model.py:685-696) against the
oracle, call by call.

Every case x variant of tests/geo_zero_util.py runs its schedules through the C ABI on a handle asserted to be of the case's family
(`plain_sweeps_util.make_engine`).  After EVERY call the small state and `get_geometric()` are held to the oracle, on the calls a
schedule marks rho too; G_theta, G_lambda and G_nu are exactly 0 where the oracle's are and non-zero elsewhere; nothing is NaN or
infinite.  `loop` puts `fit_loop`'s own ELBO trace and stop decision through the regime.  A second handle under
VMR_DEBUG_LAZY_RHO=1 runs the same schedules; the deterministic cases run twice instead and must give the same bits.  The handles
with a level-0 shortcut switched off and the one with all of them on are each held to the oracle, not to each other.  One read-side
leg holds `reporter_influence` of the zeroed layer to its NumPy restatement.  The bounds are the project's (`cs.ratio`): ELBO 1e-9
max(1, |ELBO|); gamma, phi, nu and the geometric expectations rtol 1e-9; rho rtol 1e-7; atol 1e-12.  tests/test_geo_zero_host.py
shows on the host that no row of these inputs needs a band of its own."""
import numpy as np
import pytest

from tests import call_sequence_util as cs
from tests import geo_zero_util as gz
from tests import plain_sweeps_util as pu

pytestmark = pytest.mark.gpu

_ORACLE = {}


def _oracle(case, variant, schedule):
    if (case, variant, schedule) not in _ORACLE:
        _ORACLE[(case, variant, schedule)] = gz.run_model(case, variant, schedule, pu.oracle_of(case))
    return _ORACLE[(case, variant, schedule)]


def _engine(case, variant, monkeypatch, extra=None):
    return pu.make_engine(case, monkeypatch, extra, data=gz.data(case, variant), priors=gz.priors(case, variant))


def _run(eng, case, variant, schedule):
    """The schedule on the handle: [(return value, small state with the geometric expectations, and rho on the marked calls)]."""
    out = []
    for op in gz.schedule_ops(case, schedule):
        if op["op"] == "set_state":
            eng.set_state(*gz.state(case, variant, op["state_seed"]))
            ret = None
        elif op["op"] == "step":
            ret = eng.step(op["n"], want_elbo=op["want_elbo"])
        else:
            rows, elbo, its, conv = eng.fit_loop(op["max_iter"], op["tol"], op["decision"])
            ret = ([r[0] for r in rows], [r[1] for r in rows], elbo, its, conv)
        s = cs.engine_small_state(eng)
        if op["compare"]:
            s["rho"] = eng.get_state(rho=True)["rho"]
        out.append((ret, s))
    return out


def _hold(got, case, variant, schedule, leg):
    want = _oracle(case, variant, schedule)
    ops = gz.schedule_ops(case, schedule)
    for i, ((rg, sg), (rw, sw)) in enumerate(zip(got, want)):
        what = f"{case} / {variant} / {schedule} / {leg}: call {i} ({ {k: v for k, v in ops[i].items() if k != 'compare'} })"
        for n, v in sg.items():
            assert np.isfinite(v).all(), f"{what}: {n} holds a NaN or an infinity"
        for n in ("G_theta", "G_lambda", "g_nu", "g_nu_stale"):
            assert np.array_equal(np.asarray(sg[n]) == 0.0, np.asarray(sw[n]) == 0.0), f"{what}: the zeros of {n} are not the oracle's"
        r =gz.call_ratios(rg, sg, rw, sw, ops[i]["op"], "rho" in sg)
        print(f"{what}: worst {max(r.values()):.3g} of a tolerance")
        bad = {n: v for n, v in r.items() if not v <= 1.0}
        assert not bad, f"{what}: beyond the tolerance (in units of it): {bad}"


def _same(a, b):
    for (ra, sa), (rb, sb) in zip(a, b):
        assert ra == rb
        for n in sa:
            assert np.array_equal(np.asarray(sa[n]), np.asarray(sb[n])), n


@pytest.mark.parametrize("case,variant", gz.COMBOS)
def test_sweeps_with_a_zero_expectation_match_the_oracle(case, variant, monkeypatch):
    det = pu.CASES[case].get("det")
    for leg, extra in (("written", None),) + (() if det else (("lazy", {"VMR_DEBUG_LAZY_RHO": "1"}),)):
        eng = _engine(case, variant, monkeypatch, extra)
        try:
            for schedule in gz.schedules_of(case):
                got = _run(eng, case, variant, schedule)
                _hold(got, case, variant, schedule, leg)
                if det:      # sums across workgroups in a fixed order: a second run is the same bits
                    _same(got, _run(eng, case, variant, schedule))
        finally:
            eng.close()


def test_reporter_influence_takes_the_rule(monkeypatch):
    """`k3_lists` x `both` after the `inner` schedule: the leave-one-out rows of the zeroed layer, whose tables hold exp(.) = 0
    for the zeroed reporters and category, against `influence.influence_np` within tests/influence_util.py's bound."""
    from tests import influence_util as iu
    from vimure_amd.influence import influence_np
    case, variant = "k3_lists", "both"
    X, R = gz.data(case, variant)
    K, mut = pu.built(case)[2:4]
    zl, rep, cat, _ = gz.zeroed(case, variant)
    eng = _engine(case, variant, monkeypatch)
    try:
        _hold(_run(eng, case, variant, "inner"), case, variant, "inner", "before the read")
        s = eng.get_state(rho=True)
        st = (s["gamma_shp"], s["gamma_rte"], s["phi_shp"], s["phi_rte"], s["nu_shp"], s["nu_rte"], s["rho"])
        c = dict(name=f"{case} {variant}", X=np.asarray(X).astype(np.int64), R=R, K=K, mut=mut, st=st, rho=s["rho"], tabs=iu.tables(st, mut))
        assert (np.exp(c["tabs"][1][zl][rep]) == 0.0).all() and np.exp(c["tabs"][3][zl, cat]) == 0.0 and c["tabs"][4] > 0.0
        al = influence_np(c["rho"], c["X"], c["R"], *c["tabs"], mutuality=mut, select="none", min_tv=0.0, layer=zl)
        assert rep[al["m"]].sum() >= 20 and (al["x"][rep[al["m"]]] > 0).sum() >= 20, "too few elements of the zeroed reporters"
        full = eng.reporter_influence(*c["tabs"], select="none", min_tv=0.0, layer=zl, flips=False)
        for k in iu.ROWS:
            assert np.array_equal(full[k], al[k]), k
        iu.compare_values(full, dict(al=al, T=iu.term_size(c, al)), np.ones(len(al["l"]), bool), c["name"])
    finally:
        eng.close()
