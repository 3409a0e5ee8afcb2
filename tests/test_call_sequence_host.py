"""CPU: the host model of the call-sequence tests (tests/call_sequence_util.py) is implementation-independent, the committed
sequences cover what they are meant to cover, and they would notice the bookkeeping mistakes they are there for.

* Every committed (seed, kind) sequence runs through `SeqModel` on `oracle/cavi_coo.c` and on the NumPy oracle with the same rules:
  after every operation every observable agrees to the tolerances the device is held to.  The largest deviation per observable, in
  units of its tolerance, is what DESIGN section 5 quotes; it must stay below a tenth, or the tolerance has to be re-derived.
* No ELBO of a committed sequence is NaN and no row of rho underflows (rows sum to 1).
* Coverage: every operation at least 10 times, every legal ordered pair of operations at least twice, every operation followed by
  every reader, and in every kind a restore -> refused call -> set_state -> sweep.
* Sensitivity: each of four forgetful models differs from the true one by more than 1000 tolerances on some committed sequence."""
import collections
import functools

import numpy as np
import pytest

from tests import call_sequence_util as u

COMMITTED = [(seed, kind) for kind in u.KINDS for seed in u.SEEDS]


@functools.lru_cache(maxsize=None)
def _data(family):
    X, R = u.build_data(family)
    X.setflags(write=False)
    if R is not None:
        R.setflags(write=False)
    return X, R


def _model(kind, backend, forget=None):
    spec = u.KINDS[kind]
    X, R = _data(spec["data"])
    return u.SeqModel(X, R, spec["K"], spec.get("mut", True), backend, forget)


def test_data_is_what_the_kinds_ask_for():
    for family, (N, M) in u.SHAPES.items():
        X, R = _data(family)
        assert X.shape == (2, N, N, M) and N % 16 and X.max() == 3 and X[X > 0].min() == 1
        assert R is None or not (X[R == 0] > 0).any()       # every report inside R
        assert X.sum() < 200_000
    X, R = _data("ones")
    assert (X.sum(axis=3) == 0).mean() > 0.2                # some ties unreported
    X, R = _data("long")
    per_tie = (X > 0).sum(axis=3)
    assert 8 <= np.percentile(per_tie, 5) and np.percentile(per_tie, 95) <= 24
    assert ((X > 0) & (np.transpose(X, (0, 2, 1, 3)) > 0)).mean() > 0.05       # mirrored counts
    X, R = _data("self")
    assert R.sum(axis=3).max() == 2 and R.sum(axis=3).min() == 1


@pytest.mark.parametrize("kind", list(u.KINDS))
def test_model_agrees_across_the_two_oracles(kind, record_property):
    worst = collections.defaultdict(float)
    for seed in u.SEEDS:
        ops = u.draw_sequence(seed, kind)
        assert 10 <= len(ops) <= 16 and set(ops[-1]["readers"]) == set(u.MARKED_READERS)
        a, b = _model(kind, "coo"), _model(kind, "numpy")
        for i, op in enumerate(ops):
            ra, rb = a.apply(op), b.apply(op)
            ratios = u.result_ratios(rb, ra, op["op"])
            oa, ob = a.observe(), b.observe()
            ratios.update(u.state_ratios(ob, oa))
            assert np.isfinite(oa["rho"]).all() and np.abs(oa["rho"].sum(-1) - 1.0).max() < 1e-12, (kind, seed, i, "a row of rho underflows")
            for n, v in ratios.items():
                worst[n] = max(worst[n], v)
            bad = {n: v for n, v in ratios.items() if not v <= 1.0}
            assert not bad, f"{kind} seed {seed}: operation {i} ({op['op']}): the two oracles differ beyond the tolerance: {bad}"
    print(kind, "oracle pair, largest deviation in units of the tolerance:", {n: round(v, 4) for n, v in worst.items()})
    for n, v in worst.items():
        record_property(n, v)
    # a tenth of the tolerance is what the oracle pair may use before the tolerance has to be widened to 10 times its deviation
    assert max(worst.values()) <= 0.1, dict(worst)


def test_committed_sequences_cover_operations_pairs_and_readers():
    ops, pairs, reads = collections.Counter(), collections.Counter(), collections.Counter()
    blocks = collections.Counter()
    for seed, kind in COMMITTED:
        seq = u.draw_sequence(seed, kind)
        assert seq == u.draw_sequence(seed, kind)                    # deterministic
        n, p, r = u.sequence_elements(seq)
        ops.update(n)
        pairs.update(p)
        reads.update(r)
        blocks[kind] += u.has_restore_block(seq)
        sweeps, longs = 0.0, 0
        for op in seq:
            if op["op"] == "set_state":
                sweeps, longs = 0.0, 0
            long_ = (op["op"] == "step" and op["n"] == 11) or (op["op"] == "fit_loop" and op["max_iter"] > 1)
            longs += long_
            sweeps += 0 if long_ else {"step": op.get("n", 0), "sub_step": 0.25, "sweep_commit": 1, "fit_loop": 1}.get(op["op"], 0)
            assert sweeps < u.MAX_SWEEPS + 1 and longs <= 1, (seed, kind)      # (below the cap before the last short call, which adds at most 1)
            if u.KINDS[kind].get("det"):
                assert op["op"] != "sub_step"
    assert all(ops[o] >= 10 for o in u.OPS), dict(ops)
    short = {p: pairs[p] for p in u.LEGAL_PAIRS if pairs[p] < 2}
    assert not short, short
    assert not [p for p in pairs if not u.legal_pair(*p)]
    missing = [(o, r) for o in u.OPS for r in u.READERS if reads[(o, r)] < 1]
    assert not missing, missing
    assert all(blocks[k] >= 1 for k in u.KINDS), dict(blocks)
    det_refusals = [op for seed, kind in COMMITTED if u.KINDS[kind].get("det") for op in u.draw_sequence(seed, kind)
                    if op["op"] == "refused" and op["message"] == u.NO_SUB_STEP]
    assert det_refusals
    ns = collections.Counter(op["n"] for seed, kind in COMMITTED for op in u.draw_sequence(seed, kind) if op["op"] == "step")
    assert all(ns[n] >= 2 for n in (0, 1, 2, 3, 11)), dict(ns)
    subs = collections.Counter(op["which"] for seed, kind in COMMITTED for op in u.draw_sequence(seed, kind) if op["op"] == "sub_step")
    assert all(subs[w] >= 3 for w in u.SUBS), dict(subs)
    its = collections.Counter(op["max_iter"] for seed, kind in COMMITTED for op in u.draw_sequence(seed, kind) if op["op"] == "fit_loop")
    assert all(its[n] >= 2 for n in (1, 11, 21)), dict(its)


@pytest.mark.parametrize("forget", u.FORGETFUL)
def test_a_forgetful_model_is_noticed(forget):
    """The sequences can only catch a class of bug if the model with that bug built in differs visibly from the true one."""
    best = 0.0
    for seed, kind in COMMITTED:
        if forget == "gamma_after_rho_old_mask_sums" and u.KINDS[kind].get("det"):
            continue
        ops = u.draw_sequence(seed, kind)
        a, b = _model(kind, "coo"), _model(kind, "coo", forget)
        for op in ops:
            ra, rb = a.apply(op), b.apply(op)
            ratios = u.state_ratios(b.observe(), a.observe())
            if ra is not None:
                ratios["elbo"] = u.ratio(rb[2] if op["op"] == "fit_loop" else rb, ra[2] if op["op"] == "fit_loop" else ra, "elbo")
            best = max(best, max(ratios.values()))
        if best > 1000.0:
            return
    raise AssertionError(f"{forget}: the largest difference over the committed sequences is {best} tolerances")
