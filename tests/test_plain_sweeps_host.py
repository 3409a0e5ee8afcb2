"""No GPU: the plain-sweep cases of tests/plain_sweeps_util.py are what they claim to be, the two oracles agree on every case and
schedule to a tenth of the tolerances the device is held to, and three models with a plain-sweep mistake built in are noticed.

* Class: read from X, R and `shape_of` alone -- mirror counts beyond the LDS levels the plain variant keeps, steps of more than
  SL_PF rounds, the plain and the ELBO variant of `tight_lds` keeping different levels, the two conditions of `create_tail` for
  far lists (N > 1024; more than 1/1024 and at most 1/8 of the reports beyond the levels), the dense two-pass threshold.
* Oracle pair: `PlainModel` on oracle/cavi_coo.c (oracle/cavi_ref.c for the dense tiles) against the same model on the
  NumPy oracle; the far-list case, 1 GB as a dense tensor, runs on the coordinate-list oracle alone and is held to finite,
  normalised rows.  No NaN, no tie whose exponentials all underflow.
* Sensitivity: each of PLAIN_FORGETFUL differs from the true model by more than 1000 tolerances on some case and schedule."""
import numpy as np
import pytest

from tests import call_sequence_util as cs
from tests import plain_sweeps_util as u

PAIR_BOUND = 0.1      # of a tolerance
_WORST = {}


@pytest.mark.parametrize("case", list(u.CASES))
def test_case_is_in_its_class(case):
    spec = u.CASES[case]
    X, R, K, mut, entry, seed = u.built(case)
    L, N, _, M = X.shape
    assert N <= 130 and M <= 1008 or "far" in spec["claims"], (N, M)
    sh = u.shape_of(case)
    _, vals = u.coo_of(X)
    mir = u.mirror_counts(X)
    if R is not None:
        assert not (np.asarray(X) * (1 - R)).any(), "a report outside the mask"
    assert set(spec["env"]) <= set(cs.SWITCHES), "a switch the tests do not clear"
    if spec["passes"] is not None and not sh.get("general"):
        assert sh["two_pass"] == (spec["passes"] == 2), sh
    if spec.get("levels") is not None:
        assert sh["hc"] == spec["levels"], sh
    if "beyond" in spec["claims"]:
        p = sh["plain"]
        assert int(mir.max()) >= max(p["yt"], p["hc"]) and int(vals.max()) >= max(p["yt"], p["hc"]), (int(mir.max()), p)
        assert int((mir >= p["yt"]).sum()) >= 64 and int((mir >= p["hc"]).sum()) >= 64, "too few reports on the slow path"
        assert sh["Y"] > max(p["yt"], p["hc"])
    if "long" in spec["claims"]:
        assert int(u.reports_per_tie(X).max()) > u.SL_PF      # (a step has the rounds of its longest tie)
        assert float(np.median(u.reports_per_tie(X))) > u.SL_PF, "most steps are to be long ones"
    if "tight" in spec["claims"]:
        p, e = sh["plain"], sh["elbo"]
        assert (p["yt"], p["hc"]) != (e["yt"], e["hc"]), (p, e)
        assert (p["yt"], p["hc"]) == (sh["yt"], sh["hc"]) and p["smem"] <= u.SP_LDS_MAX < p["smem"] + 2048, (p, e)
        assert not sh["two_pass"]
    if "far" in spec["claims"]:
        assert N > 1024 and sh["farl"] and not sh["two_pass"], sh
        assert 1.0 / 1024 < sh["far_frac"] <= 0.125, sh["far_frac"]
        assert sh["plain"]["hc"] == sh["stat"]["hc"] == sh["hc"], "the far lists need the same levels in every variant that adds to H"
    if "dense_two_pass" in spec["claims"]:
        assert sh["dense_smem"] > 80000, sh
    if spec["fmt"] == "dense":
        assert not sh.get("general") and K <= u.KMAX
    if case.startswith("general"):
        assert sh.get("general") and entry == "coo"
    if case == "general_wide":
        assert int(vals.max()) > 2047
    if spec["mask"] == "lists":
        assert sh["ml"], sh
    if spec["mask"] == "words":
        assert not sh["ml"] and not sh["all_full"], sh


def test_every_compiled_workgroup_cap_is_met():
    """The plain update variant's caps 1024, 768, 512, 256 and both ALLFULL values at every K of the specialised kernels."""
    caps = {(u.built(c)[2], u.shape_of(c)["all_full"]): u.sl_tpb_max(u.built(c)[2], False, u.shape_of(c)["all_full"])
            for c in u.CASES if c[0] == "k" and c[1].isdigit()}
    assert set(caps) == {(K, a) for K in range(2, 9) for a in (True, False)}
    assert set(caps.values()) == {1024, 768, 512, 256}
    assert {u.sl_tpb_max(K, True, True) for K in range(2, 9)} == {768, 512, 256}


def _healthy(run, case):
    for ret, obs in run:
        assert ret is None or np.isfinite(ret), (case, ret)
        if obs is not None:
            rho = obs["rho"]
            assert np.isfinite(rho).all(), case
            assert np.abs(rho.sum(-1) - 1.0).max() < 1e-9, f"{case}: a tie whose exponentials all underflow"
            for n in cs.PARAMS:
                assert np.isfinite(obs[n]).all(), (case, n)


@pytest.mark.parametrize("case", list(u.CASES))
def test_the_two_oracles_agree_to_a_tenth_of_the_tolerances(case):
    for schedule in u.schedules_of(case):
        a = u.run_model(case, schedule, u.oracle_of(case))
        _healthy(a, case)
        if u.CASES[case].get("no_numpy"):
            continue
        b = u.run_model(case, schedule, "numpy")
        _healthy(b, case)
        w, where = u.worst_ratio(a, b)
        _WORST[(case, schedule)] = w
        print(f"{case} {schedule}: oracle pair {w:.3g} of a tolerance at {where}")
        assert w <= PAIR_BOUND, (case, schedule, w, where)


SENSITIVE = ("levels_beyond_k3_21", "k3_words", "tight_lds", "two_pass_k2")


@pytest.mark.parametrize("forget", u.PLAIN_FORGETFUL)
def test_a_forgetful_model_is_noticed(forget):
    found = {}
    for case in SENSITIVE:
        drop = u.shape_of(case)["plain"]["yt"] if forget == "plain_drops_far_levels" else None
        if drop is not None and drop >= u.shape_of(case)["Y"]:
            continue
        for schedule in u.SCHEDULES:
            w, where = u.worst_ratio(u.run_model(case, schedule, "coo", forget, drop), u.run_model(case, schedule, "coo"))
            found[(case, schedule)] = (w, where)
    print(forget, {k: f"{v[0]:.3g}" for k, v in found.items()})
    assert max(v[0] for v in found.values()) > 1000.0, found
    if forget != "rerun_current_nu":      # what a plain sweep leaves behind shows in the ELBO sweep after it
        assert found[("levels_beyond_k3_21", "inner")][0] > 1000.0, found
