"""GPU: plain sweeps (rho updates without the ELBO) of every kernel regime against the oracle, call by call.

Every case of tests/plain_sweeps_util.py runs every schedule through the C ABI on a handle asserted to be of the case's family
(`data_format`, `mask_format`, `sweep_shape`): `each` compares every written rho, `inner` leaves two rhos unwritten and then shows
in an ELBO sweep what plain sweep 3 left behind (H, the mask sums, the nu finished inside the pass), `mixed` reads the unwritten
rho through the stand-alone ELBO.  A second handle under VMR_DEBUG_LAZY_RHO=1 runs the same schedules with every rho read through
`ensure_rho`'s re-run (bit-identity with the written leg is shown by tests/test_hip_lpd.py on deterministic K = 2 all-ones
handles only, and the deterministic cases here get no lazy leg: the bounds hold everywhere).  One further run under `profile(True)` asserts the
kernel classes launched.  The bounds are the project's: ELBO 1e-9 max(1, |ELBO|); gamma, phi, nu rtol 1e-9; rho rtol 1e-7;
atol 1e-12."""
import numpy as np
import pytest

from tests import call_sequence_util as cs
from tests import plain_sweeps_util as u

pytestmark = pytest.mark.gpu

_ORACLE = {}


def _oracle(case, schedule):
    if (case, schedule) not in _ORACLE:
        _ORACLE[(case, schedule)] = u.run_model(case, schedule, u.oracle_of(case))
    return _ORACLE[(case, schedule)]


_engine = u.make_engine      # (the handle and the assertions on its family: shared with tests/test_hip_geo_zero.py)


def _run(eng, case, schedule):
    """The schedule on the handle, in the form of `plain_sweeps_util.run_model`."""
    out = []
    for op in u.schedule_ops(case, schedule):
        if op["op"] == "set_state":
            eng.set_state(*u.case_state(case, op["state_seed"]))
            ret = None
        elif op["op"] == "step":
            ret = eng.step(op["n"], want_elbo=op["want_elbo"])
        else:
            ret = eng.elbo()
        out.append((ret, eng.get_state(rho=True) if op["compare"] else None))
    return out


def _hold(got, case, schedule, leg):
    want = _oracle(case, schedule)
    ops = u.schedule_ops(case, schedule)
    for i, ((rg, sg), (rw, sw)) in enumerate(zip(got, want)):
        what = f"{case} / {schedule} / {leg}: call {i} ({ {k: v for k, v in ops[i].items() if k != 'compare'} })"
        r = {}
        if rw is not None:
            assert rg is not None and np.isfinite(rg), what
            r["elbo"] = cs.ratio(rg, rw, "elbo")
        if sw is not None:
            r.update({n: cs.ratio(sg[n], sw[n], n) for n in cs.PARAMS + ("rho",)})
        bad = {n: v for n, v in r.items() if not v <= 1.0}
        assert not bad, f"{what}: beyond the tolerance (in units of it): {bad}"


def _same(a, b):
    for (ra, sa), (rb, sb) in zip(a, b):
        assert ra == rb
        if sa is not None:
            for n in cs.PARAMS + ("rho",):
                assert np.array_equal(np.asarray(sa[n]), np.asarray(sb[n])), n


@pytest.mark.parametrize("case", list(u.CASES))
def test_plain_sweeps_match_the_oracle(case, monkeypatch):
    spec = u.CASES[case]
    eng = _engine(case, monkeypatch)
    try:
        for schedule in u.schedules_of(case):
            got = _run(eng, case, schedule)
            _hold(got, case, schedule, "written")
            if spec.get("det"):      # sums across workgroups in a fixed order: a second run is the same bits
                _same(got, _run(eng, case, schedule))
        # the kernel classes: the inner sweeps of step(3) leave rho unwritten where launch_rho's `lazy` condition holds
        schedule = u.schedules_of(case)[-1] if spec.get("graph") or spec.get("det") else "inner"
        eng.profile(True)
        got = _run(eng, case, schedule)
        n = {k: v["launches"] for k, v in eng.profile_read().items()}
        eng.profile(False)
        _hold(got, case, schedule, "profiled")
        # (far lists whose fused ELBO variant would drop a level: the ELBO sweep is the plain pass and an ELBO-only pass)
        assert n["rho"] > 0 and n["elbo" if spec.get("far") and u.shape_of(case)["elbo"]["yt"] != u.shape_of(case)["yt"] else "rho_elbo"] > 0, n
        assert (n["rho_nostore"] > 0) == (u.NOSTORE in spec["kernels"]), (case, n)
    finally:
        eng.close()
    if spec.get("det"):
        return
    eng = _engine(case, monkeypatch, {"VMR_DEBUG_LAZY_RHO": "1"})
    try:
        for schedule in u.schedules_of(case):
            _hold(_run(eng, case, schedule), case, schedule, "lazy")
    finally:
        eng.close()
