"""No GPU: every case x variant of tests/geo_zero_util.py meets the conditions tests/test_hip_geo_zero.py relies on -- that test
compares every row and leaves none out, so its inputs have to be ones on which the oracle alone is clean.

* Zeros and margins: after every call of every schedule G_theta, G_lambda and G_nu of the oracle are 0 exactly where the variant
  says (`enter`, `enter_rows`: from the first sweep on), every zeroed entry has E[log .] <= -800 and every other one is above
  1e-200: no entry's side depends on the last bit of an exp or a digamma.
* Coverage of the rule: the zeroed entries' reports number at least 10 at mirror count 0 and at least 10 at mirror count >= 1.
* Clean oracle: no NaN, every rho row sums to 1 within 1e-12 (`enter_rows`: once a sweep has run), a finite ELBO; the stop
  decisions of the `loop` schedule are not within 1e-6 max(1, |ELBO|) of the tolerance.
* Oracle pair: the C oracle of the case and the NumPy oracle agree within the project's tolerances.
* Sensitivity: each of `geo_zero_util.WRONG` deviates from the model by at least 100 tolerances (or by a NaN) on every case x
  variant it applies to."""
import numpy as np
import pytest
from scipy.special import psi

from tests import call_sequence_util as cs
from tests import geo_zero_util as gz
from tests import plain_sweeps_util as pu

_RUNS = {}


def _run(case, variant, schedule, backend=None):
    backend = backend or pu.oracle_of(case)
    key = (case, variant, schedule, backend)
    if key not in _RUNS:
        _RUNS[key] = gz.run_model(case, variant, schedule, backend)
    return _RUNS[key]


def test_the_combinations_are_the_stated_ones():
    assert len(set(gz.COMBOS)) == len(gz.COMBOS)
    assert {c for c, _ in gz.COMBOS} <= set(pu.CASES)
    for c in gz._FULL:
        assert {v for cc, v in gz.COMBOS if cc == c} == set(gz.VARIANTS)
    for c in gz._PAIR:
        assert {"both", "nu_theta"} <= {v for cc, v in gz.COMBOS if cc == c}
    for c in gz.LOOP_CASES:
        assert "loop" in gz.schedules_of(c)


@pytest.mark.parametrize("case,variant", gz.COMBOS)
def test_the_rule_has_reports_on_both_sides(case, variant):
    if variant == "enter":      # (construction one: the reporters report nothing in their layer -- asserted instead)
        X, _ = gz.data(case, variant)
        zl, rep, _, _ = gz.zeroed(case, variant)
        assert rep.sum() >= 2 and not np.asarray(X[zl])[..., rep].any() and np.asarray(X[zl]).any()
        R = pu.built(case)[1]
        assert R is None or np.asarray(R[zl])[..., rep].any(axis=(0, 1)).all(), "a silent reporter outside the mask"
        return
    n0, n1 = gz.rule_counts(case, variant)
    print(f"{case} {variant}: {n0} reports of the zeroed entries at mirror count 0, {n1} at mirror count >= 1")
    assert n0 >= 10 and n1 >= 10, (case, variant, n0, n1)
    if variant == "enter_rows":
        zl, rep, _, _ = gz.zeroed(case, variant)
        pr = gz.state(case, variant, 1)[6]
        zero = ~pr[zl].any(-1)
        assert zero.sum() >= 10 and (~zero).sum() >= 10 and not zero[(np.asarray(pu.built(case)[0][zl])[..., rep] == 0).all(-1)].any()


@pytest.mark.parametrize("case,variant", gz.COMBOS)
def test_zeros_margins_and_a_clean_oracle(case, variant):
    mut = pu.built(case)[3]
    for schedule in gz.schedules_of(case):
        ops = gz.schedule_ops(case, schedule)
        for i, (ret, s) in enumerate(_run(case, variant, schedule)):
            what = (case, variant, schedule, i)
            zt, zla, znu = gz.expected_zeros(case, variant, swept=i > 0)
            for name, z, el in (("G_theta", zt, psi(s["gamma_shp"]) - np.log(s["gamma_rte"])),
                                ("G_lambda", zla, psi(s["phi_shp"]) - np.log(s["phi_rte"]))):
                assert np.array_equal(s[name] == 0.0, z), (what, name)
                assert (el[z] <= -800.0).all() and (s[name][~z] > 1e-200).all(), (what, name)
            for name in ("g_nu", "g_nu_stale"):
                assert (s[name] == 0.0) == znu and (znu or s[name] > 1e-200), (what, name, s[name])
            assert not mut or not znu or psi(s["nu_shp"]) - np.log(s["nu_rte"]) <= -800.0, what
            for n in cs.PARAMS:
                assert np.isfinite(s[n]).all(), (what, n)
            rho = s["rho"]
            assert np.isfinite(rho).all(), what
            if i > 0 or variant != "enter_rows":
                assert np.abs(rho.sum(-1) - 1.0).max() <= 1e-12, (what, float(np.abs(rho.sum(-1) - 1.0).max()))
            if ops[i]["op"] == "fit_loop":
                _, elbos, last, its, _ = ret      # (the ELBO of iteration 10 is the trace's row, that of iteration 12 the last)
                assert its == 12 and len(elbos) == 1 and np.isfinite(elbos[0]) and np.isfinite(last), what
                assert abs(abs(last - elbos[0]) - ops[i]["tol"]) > 1e-6 * max(1.0, abs(last)), (what, last - elbos[0])
            elif ret is not None:
                assert np.isfinite(ret), what


@pytest.mark.parametrize("case,variant", [cv for cv in gz.COMBOS if not pu.CASES[cv[0]].get("no_numpy")])
def test_the_two_oracles_agree(case, variant):
    for schedule in gz.schedules_of(case):
        ops = gz.schedule_ops(case, schedule)
        w, where = gz.worst_ratio(_run(case, variant, schedule), _run(case, variant, schedule, "numpy"), ops)
        print(f"{case} {variant} {schedule}: oracle pair {w:.3g} of a tolerance at {where}")
        assert w <= 1.0, (case, variant, schedule, w, where)


@pytest.mark.parametrize("wrong", gz.WRONG)
def test_a_wrong_model_is_noticed_on_every_case(wrong):
    found = {}
    for case, variant in gz.COMBOS:
        if pu.CASES[case].get("no_numpy") or not gz.applies(wrong, case, variant):
            continue
        schedule = gz.schedules_of(case)[0]
        ops = gz.schedule_ops(case, schedule)
        found[(case, variant)] = gz.worst_ratio(gz.run_model(case, variant, schedule, wrong=wrong), _run(case, variant, schedule, "numpy"), ops)
    print(wrong, {k: f"{v[0]:.3g} at {v[1]}" for k, v in found.items()})
    assert len(found) >= 15 or wrong == "nu_share_unguarded" and len(found) >= 10, len(found)
    missed = {k: v for k, v in found.items() if not v[0] >= 100.0}
    assert not missed, missed
