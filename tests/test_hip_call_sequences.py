"""GPU: random legal sequences of engine calls on small handles of every kernel family, every call held to the host model.

The suite's other files reach every kernel from a few fixed call orders; the handle's bookkeeping (which statistics, mask sums and
rho a call may trust) is decided by the order.  tests/call_sequence_util.py draws the sequences -- set_state (with new priors),
step(n) with and without the ELBO, sub-steps in every order the hook admits, elbo(), sweep_local + commit_nu, fit_loop, snapshot, restore and the
calls a restored or deterministic handle refuses -- and mirrors them on `oracle/cavi_coo.c`; tests/test_call_sequence_host.py
shows on the CPU what the committed sequences cover, that the model does not depend on the oracle's implementation (the NumPy oracle
agrees to within a hundredth of every tolerance) and that a model with a bookkeeping mistake built in would differ by more than 1000
tolerances.  After EVERY operation the small state (get_state(rho=False), get_geometric) is compared, after the marked ones also
rho, the read-outs, the sampler (bit for bit on the rho read in the same state), expected_stats and edge_table_size.

Tolerances, the project's: ELBO 1e-9 max(1, |ELBO|); gamma, phi, nu and the geometric means rtol 1e-9, atol 1e-12; rho rtol 1e-7,
atol 1e-12; integers equal, a read-out element decided within 1e-9 of a tie compared on the device's own rho (below 1 % of a
sequence's elements).  A failure names the kind, the seed, the index and name of the first diverging operation and the observable."""
import functools

import numpy as np
import pytest

from tests import call_sequence_util as u

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _data(family):
    X, R = u.build_data(family)
    X.setflags(write=False)
    if R is not None:
        R.setflags(write=False)
    return X, R


def _env(monkeypatch, kind):
    for k in u.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in u.spec_of(kind)["env"].items():
        monkeypatch.setenv(k, v)      # (a handle reads its switches once, at creation)


@pytest.mark.parametrize("seed", u.SEEDS)
@pytest.mark.parametrize("kind", list(u.KINDS))
def test_random_call_sequence_against_the_model(kind, seed, monkeypatch):
    _env(monkeypatch, kind)
    X, R = _data(u.KINDS[kind]["data"])
    ops = u.draw_sequence(seed, kind)
    first = []
    u.run_sequence(kind, ops, X, R, label=f"{kind} seed {seed}", record=first)
    if u.KINDS[kind].get("det"):      # VMR_DETERMINISTIC=1: the same sequence once more, bit for bit
        again = []
        u.run_sequence(kind, ops, X, R, label=f"{kind} seed {seed} (second run)", record=again)
        _bit_equal(first, again, f"{kind} seed {seed}")


def _run(kind, ops, monkeypatch, label, record=None):
    _env(monkeypatch, kind)
    X, R = _data(u.spec_of(kind)["data"])
    full = list(u.MARKED_READERS)
    u.run_sequence(kind, [dict(op, readers=op.get("readers", full)) for op in ops], X, R, label=label, record=record)


def _bit_equal(first, again, label):
    for i, ((ra, sa), (rb, sb)) in enumerate(zip(first, again)):
        assert ra == rb, f"{label}: operation {i}: return values of two runs differ: {ra} {rb}"
        for n in sa:
            assert np.array_equal(sa[n], sb[n]), f"{label}: operation {i}: {n} differs between two runs"


@pytest.mark.parametrize("kind", ["lists_k2_words", "lists_k3_selfmask", "lists_two_pass", "dense_k3", "general_k9"])
def test_sub_steps_out_of_a_sweeps_order_then_whole_sweeps(kind, monkeypatch):
    """A hand-written sequence per family around the mask sums and statistics a sub-step leaves behind: rho twice (the first one's
    sums are never consumed), gamma, nu before phi, a plain step on top, the ELBO between two plain steps, phi twice, and phi
    refused wherever no gamma sub-step has prepared its rate since rho last changed."""
    sub = lambda w: {"op": "sub_step", "which": w}
    no_phi = {"op": "refused", "call": "sub_step_phi", "message": u.NO_PHI}
    ops = [{"op": "set_state", "state_seed": 11, "priors": None}, no_phi, sub("RHO"), sub("RHO"), sub("GAMMA"), sub("NU"), sub("PHI"),
           {"op": "step", "n": 2, "want_elbo": False}, {"op": "elbo"}, {"op": "step", "n": 1, "want_elbo": False}, no_phi,
           sub("NU"), sub("GAMMA"), sub("PHI"), sub("PHI"), sub("RHO"), no_phi, {"op": "sweep_commit", "want_elbo": True},
           sub("GAMMA"), sub("NU"), sub("PHI"), {"op": "step", "n": 1, "want_elbo": True}]
    _run(kind, ops, monkeypatch, f"{kind} sub-steps")


@pytest.mark.parametrize("kind", ["lists_k2_ones", "graphs", "lazy", "det"])
def test_second_realisation_on_a_handle_with_graphs_and_a_snapshot(kind, monkeypatch):
    """fit_loop, snapshot, a second set_state with other priors, the old snapshot restored and every sweeping call refused, a third
    set_state, step(11) across a graph chunk, sweep_local + commit_nu after the loop."""
    refused = [{"op": "refused", "call": c, "message": u.READ_ONLY} for c in ("step", "elbo", "sweep_commit", "commit_nu", "fit_loop", "sub_step")]
    ops = ([{"op": "set_state", "state_seed": 21, "priors": None}, {"op": "fit_loop", "max_iter": 21, "tol": 1e-300, "decision": 1},
            {"op": "snapshot"}, {"op": "set_state", "state_seed": 22, "priors": (0.2, 0.15, 8.0, 12.0, 0.7, 1.5)},
            {"op": "step", "n": 3, "want_elbo": False}, {"op": "restore"}] + refused
           + [{"op": "set_state", "state_seed": 23, "priors": None}, {"op": "step", "n": 11, "want_elbo": False}, {"op": "elbo"},
              {"op": "sweep_commit", "want_elbo": False}, {"op": "sweep_commit", "want_elbo": True}, {"op": "step", "n": 2, "want_elbo": True}])
    _run(kind, ops, monkeypatch, f"{kind} second realisation")


@pytest.mark.parametrize("kind", ["lists_k2_words", "general_k9"])
def test_restore_keeps_the_priors_of_the_handle(kind, monkeypatch):
    """Regression (found by the random sequences): vmr_restore copied the whole parameter block of the snapshot, the priors of
    the snapshot's time included, so a set_priors between snapshot and restore was silently undone for every later realisation."""
    ops = [{"op": "set_state", "state_seed": 31, "priors": None}, {"op": "step", "n": 1, "want_elbo": False}, {"op": "snapshot"},
           {"op": "set_state", "state_seed": 32, "priors": (0.2, 0.15, 8.0, 12.0, 0.7, 1.5)}, {"op": "restore"},
           {"op": "set_state", "state_seed": 33, "priors": None}, {"op": "step", "n": 1, "want_elbo": True}]
    _run(kind, ops, monkeypatch, f"{kind} priors across restore")


@pytest.mark.parametrize("kind", ["lists_k2_ones", "dense_k3", "general_k9"])
def test_phi_sub_step_needs_the_rate_of_a_gamma_sub_step(kind, monkeypatch):
    """Regression (found by the random sequences): STEP_PHI commits the rate the finalize of STEP_GAMMA prepares.  Without one since
    rho last changed it used to commit the rate of another rho -- after set_state the one of the last realisation, or nothing at
    all -- and is refused now; after a gamma sub-step it is the oracle's update, nu in between or not, once or twice."""
    sub = lambda w: {"op": "sub_step", "which": w}
    no_phi = {"op": "refused", "call": "sub_step_phi", "message": u.NO_PHI}
    ops = [{"op": "set_state", "state_seed": 41, "priors": None}, no_phi, sub("GAMMA"), sub("PHI"), sub("RHO"), no_phi,
           {"op": "step", "n": 1, "want_elbo": False}, no_phi, sub("GAMMA"), sub("NU"), sub("PHI"), sub("PHI"),
           {"op": "set_state", "state_seed": 42, "priors": None}, no_phi, {"op": "step", "n": 2, "want_elbo": True}]
    _run(kind, ops, monkeypatch, f"{kind} phi sub-step")


def test_mutuality_off_gamma_sub_step_commits_phi(monkeypatch):
    """Without mutuality the finalize of STEP_GAMMA commits phi as well and STEP_PHI does nothing: the model's rule, held here."""
    sub = lambda w: {"op": "sub_step", "which": w}
    ops = [{"op": "set_state", "state_seed": 51, "priors": None}, sub("PHI"), sub("RHO"), sub("GAMMA"), sub("PHI"), sub("NU"),
           {"op": "step", "n": 1, "want_elbo": True}, sub("GAMMA"), {"op": "elbo"}]
    _run("nomut", ops, monkeypatch, "nomut sub-steps")


def test_phi_after_a_gamma_sub_step_and_replayed_sweeps_is_refused(monkeypatch):
    """Regression: a replayed graph runs none of the launch helpers that mark phi's pending rate as another rho's.  An eager sweep
    and a captured graph of two, a gamma sub-step (the rate is pending), two sweeps from the graph cache: phi must be refused."""
    sub = lambda w: {"op": "sub_step", "which": w}
    no_phi = {"op": "refused", "call": "sub_step_phi", "message": u.NO_PHI}
    ops = [{"op": "set_state", "state_seed": 61, "priors": None}, {"op": "step", "n": 3, "want_elbo": False}, sub("GAMMA"),
           {"op": "step", "n": 2, "want_elbo": False}, no_phi, sub("GAMMA"), {"op": "fit_loop", "max_iter": 11, "tol": 1e-300, "decision": 1},
           no_phi, sub("GAMMA"), sub("PHI"), {"op": "step", "n": 11, "want_elbo": True}, no_phi]
    _run("graphs", ops, monkeypatch, "graphs phi after replayed sweeps")


@pytest.mark.parametrize("kind", ["det", "det_k3_words", "det_lists"])
def test_deterministic_handle_is_bit_equal_on_mask_words_and_on_reporter_lists(kind, monkeypatch):
    """Regression: the kernel that sums rho over mask WORDS (rows of more than 64 reporters, large networks, VMR_NO_RLISTS=1) added
    with floating-point atomics on deterministic handles too, and two runs differed in the last bits of gamma_rte.  Its sums go in
    fixed point now.  Whole sweeps, a loop, the ELBO and a second realisation twice on a handle that keeps its partial mask as
    words (K = 2 and 3) and on one with reporter lists: against the model, and bit for bit between the two runs."""
    ops = [{"op": "set_state", "state_seed": 71, "priors": None}, {"op": "step", "n": 1, "want_elbo": True}, {"op": "step", "n": 3, "want_elbo": False},
           {"op": "elbo"}, {"op": "fit_loop", "max_iter": 11, "tol": 1e-300, "decision": 1}, {"op": "sweep_commit", "want_elbo": True},
           {"op": "set_state", "state_seed": 72, "priors": (0.2, 0.15, 8.0, 12.0, 0.7, 1.5)}, {"op": "step", "n": 11, "want_elbo": True}]
    first, again = [], []
    _run(kind, ops, monkeypatch, f"{kind} first run", record=first)
    _run(kind, ops, monkeypatch, f"{kind} second run", record=again)
    _bit_equal(first, again, kind)
