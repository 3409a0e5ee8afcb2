"""Sweeps in the regime where a geometric expectation exp(E[log .]) is exactly 0: the variants, the cases and the host model
(no GPU here, no device code imported).

The reference replaces a zero denominator of its weights by 1 (model.py:685-696): with z1 = G_theta_m G_lambda_k and z2 = G_nu y,
w1 = z1 / (z1 + z2) and w2 = z2 / (z1 + z2) are both 0 where z1 + z2 == 0.  A Gamma shape of 1e-3 is enough for that:
psi(1e-3) = -1000.4, below the -745.13 at which exp rounds to 0, so such a reporter's (category's) reports carry weight 0 even at
mirror count 0 -- where every shortcut of the engine takes the weight for 1.  The zero is absorbing: with weight 0 on all its
reports the entry's next shape is its prior's shape again, which is why a zeroed entry gets 1e-3 in the state AND in its prior.

`VARIANTS` say which expectations are zero; they sit in the last layer only (layer 1 of the two-layer cases), so that layer 0 keeps
its level-0 shortcuts in the same launch in which the last layer drops them:

  theta       reporters m % stride == 0 (stride 5 unless STRIDE says otherwise)
  lambda      category K - 1 (at K = 2 every reporter then reads one finite and one infinite entry of the dense tiles' table)
  both        the reporters and the category
  nu_theta    G_nu (alpha_eta = nu_shp = 1e-3) and the reporters: z1 + z2 == 0 at EVERY mirror count
  enter       nothing in the state, the priors of `theta`: the reporters' G_theta is non-zero at the first launch and becomes 0 in
              the finalize step that consumes the sums gathered with it.  Construction one: the reporters stay in the mask, their
              reports in the last layer are taken out of the case's data
  enter_rows  the same through construction two: the data is the case's, and the initial rho (`set_state` takes any rows) is all
              zero on every tie of the last layer on which one of the reporters reports -- the first gamma update sums
              rho_k x w1 = 0 for them over ties that are irregular (a row that does not sum to 1)

Without mutuality the weights are not used at all (w1 = 1): a zeroed reporter's shape is its prior's plus its counts after the
first gamma update, so the zeros of `theta` are gone after the first sweep and nothing but the factor E[log theta] saw them.

`COMBOS` lists what runs: all six variants on one handle per family of kernels (K = 2 mask words, K = 3 mask lists, two passes, dense
K = 2 and K = 3, general), `both` and `nu_theta` -- the two that between them zero every factor of z1 and z2 -- on the smallest
handle of every other code site, `theta` alone without mutuality.  `general_wide` takes `both` only: its count of 3000 stays in
range through the mutuality term alone (plain_sweeps_util._wide_case), which a zero G_nu removes.  `far_lists` and `tight_lds`
(a thousand reporters) run once, `both` under the schedule `inner`.

`GeoModel` is `plain_sweeps_util.PlainModel` with the variant's data, priors and state; `WRONG` names three models with a mistake
of this regime built in (NumPy oracle), for the sensitivity test."""
import numpy as np

from tests import call_sequence_util as cs
from tests import plain_sweeps_util as pu

TINY = 1e-3                      # a Gamma shape whose exp(E[log .]) is 0: psi(1e-3) = -1000.4
VARIANTS = ("theta", "lambda", "both", "nu_theta", "enter", "enter_rows")
ENTER = ("enter", "enter_rows")
STRIDE = {}                      # case -> reporter stride where 5 leaves the rule's two sides short (test_geo_zero_host.py)

_FULL = ("k2_words", "k3_lists", "two_pass_k3", "dense_k2", "dense_k3", "general_k9")
_PAIR = ("k2_ones", "k2_words_nolpd", "levels_beyond_k2_11", "levels_beyond_k3_00", "long_steps_k2_words", "long_steps_k3_ones",
         "two_pass_k2", "two_pass_k3_no_level0", "two_pass_k3_no_x0", "two_pass_k3_no_lv0r", "dense_k5", "dense_two_pass",
         "general_k9", "det_k2_words", "det_two_pass")
_ONCE = ("far_lists", "tight_lds")      # variant `both`, schedule `inner`
COMBOS = ([(c, v) for c in _FULL for v in VARIANTS] + [(c, v) for c in _PAIR if c not in _FULL for v in ("both", "nu_theta")]
          + [("general_wide", "both")] + [(c, "both") for c in _ONCE] + [(c, "theta") for c in ("nomut_lists", "nomut_dense", "nomut_general")])
LOOP = {"op": "fit_loop", "max_iter": 12, "tol": 0.1, "decision": 1, "compare": True}      # ELBO at iterations 1, 10 and 12
LOOP_CASES = ("k2_words", "dense_k3")


def schedules_of(case):
    return ("inner",) if case in _ONCE or pu.CASES[case].get("det") else ("each", "inner") + (("loop",) if case in LOOP_CASES else ())


def schedule_ops(case, schedule):
    if schedule == "loop":
        return pu.schedule_ops(case, "each")[:1] + [dict(LOOP)]
    return pu.schedule_ops(case, schedule)


# --------------------------------------------------------------------------------------------------------------- the variants
def zeroed(case, variant):
    """(layer, reporters [M] bool, category or None, nu) the variant zeroes, in the state or -- `enter` -- in the first finalize."""
    X, _, K = pu.built(case)[:3]
    L, M = X.shape[0], X.shape[3]
    rep = np.zeros(M, bool)
    if variant != "lambda":
        rep[::STRIDE.get(case, 5)] = True
    return L - 1, rep, K - 1 if variant in ("lambda", "both") else None, variant == "nu_theta"


_DATA = {}


def data(case, variant):
    """(X, R) of the case; `enter`: without the zeroed reporters' reports in their layer (they stay in the mask)."""
    X, R = pu.built(case)[:2]
    if variant != "enter":
        return X, R
    if (case, variant) not in _DATA:
        zl, rep, _, _ = zeroed(case, variant)
        Xe = np.array(X)
        Xe[zl][..., rep] = 0
        Xe.flags.writeable = False
        _DATA[(case, variant)] = Xe
    return _DATA[(case, variant)], R


def priors(case, variant):
    X, _, K = pu.built(case)[:3]
    L, M = X.shape[0], X.shape[3]
    zl, rep, cat, nu = zeroed(case, variant)
    a_th, a_la = np.full((L, M), cs.PRI[0]), np.full((L, K), cs.PRI[2])
    a_th[zl, rep] = TINY
    if cat is not None:
        a_la[zl, cat] = TINY
    return (a_th, cs.PRI[1], a_la, cs.PRI[3], TINY if nu else cs.PRI[4], cs.PRI[5])


def state(case, variant, state_seed):
    """`plain_sweeps_util.case_state` with the variant's shapes at TINY (`enter`: ordinary shapes; `enter_rows`: zero rows)."""
    st = [np.array(a) if isinstance(a, np.ndarray) else a for a in pu.case_state(case, state_seed)]
    zl, rep, cat, nu = zeroed(case, variant)
    if variant == "enter_rows":
        X = pu.built(case)[0]
        st[6][zl][(np.asarray(X[zl])[..., rep] > 0).any(-1)] = 0.0
    elif variant != "enter":
        st[0][zl, rep] = TINY
        if cat is not None:
            st[2][zl, cat] = TINY
        if nu:
            st[4] = TINY
    return tuple(st)


def expected_zeros(case, variant, swept):
    """Where G_theta [L, M], G_lambda [L, K] and G_nu are exactly 0; swept: at least one sweep has run since `set_state`."""
    X, _, K, mut = pu.built(case)[:4]
    L, M = X.shape[0], X.shape[3]
    zl, rep, cat, nu = zeroed(case, variant)
    zt, zla = np.zeros((L, M), bool), np.zeros((L, K), bool)
    if (swept and mut) if variant in ENTER else (mut or not swept):
        zt[zl] = rep
        if cat is not None:
            zla[zl, cat] = True
    return zt, zla, bool(nu) or not mut      # (without mutuality G_nu is 0 by definition, model.py:600)


def rule_counts(case, variant):
    """Reports of the zeroed entries in their layer at mirror count 0 and at mirror count >= 1 (`lambda`: every report)."""
    X, _ = data(case, variant)
    zl, rep, _, _ = zeroed(case, variant)
    (l, _, _, m), _ = pu.coo_of(X)
    w = (l == zl) & (rep[m] if rep.any() else True)
    y = pu.mirror_counts(X)[w]
    return int((y == 0).sum()), int((y >= 1).sum())


# ------------------------------------------------------------------------------------------------------------------ the model
WRONG = ("level0_weight_one", "tile_weight_nan", "nu_share_unguarded")


class _NpWrong(cs._Np):
    """The NumPy oracle with one of WRONG in its weights --
      level0_weight_one: w1 = 1 at mirror count 0 whatever G is (a level-0 shortcut left on);
      tile_weight_nan: in the rho update, where z1 == 0 the weight is 0 at mirror count 0 only and NaN beyond (1 / (1 + inf y) by
        a reciprocal with a Newton step);
      nu_share_unguarded: the nu update's z2 / (z1 + z2) without the rule."""

    def __init__(self, *a, wrong):
        super().__init__(*a)
        self.wrong = wrong

    def elbo(self, g_nu):      # (a NaN is this model's deviation, not an error of the run)
        try:
            return super().elbo(g_nu)
        except ValueError:
            return float("nan")

    def update(self, which):
        vo, true, wrong = self.vo, self.vo._weights, self.wrong

        def weights(pb, st):
            xw1, xw2 = true(pb, st)
            if not pb.mutuality:
                return xw1, xw2
            l, _, _, m = pb.nz
            G_th, G_la, _ = vo.geometric_means(st)
            z1 = G_th[l, m][:, None] * G_la[l, :]
            z2 = (st.G_nu_cache * pb.xT_nz)[:, None]
            x = pb.x_nz[:, None]
            if wrong == "level0_weight_one":
                xw1 = np.where(pb.xT_nz[:, None] == 0, x, xw1)
            elif wrong == "tile_weight_nan" and which == "RHO":
                xw1 = np.where((z1 == 0) & (pb.xT_nz[:, None] > 0), np.nan, xw1)
            elif wrong == "nu_share_unguarded" and which == "NU":
                with np.errstate(invalid="ignore"):
                    xw2 = x * (z2 / (z1 + z2))
            return xw1, xw2
        vo._weights = weights
        try:
            super().update(which)
        finally:
            vo._weights = true


def applies(wrong, case, variant):
    """Whether the wrong model can differ at all: the weights need mutuality and a report of a zeroed entry (`enter`'s reporters
    have none: no weight is ever taken with their G_theta); the nu share is 0 / 0 only where G_nu is 0 too."""
    return pu.built(case)[3] and variant != "enter" and (wrong != "nu_share_unguarded" or variant == "nu_theta")


class GeoModel(pu.PlainModel):
    def __init__(self, case, variant, backend="coo", wrong=None):
        assert wrong is None or wrong in WRONG
        super().__init__(case, "numpy" if wrong else backend)
        self.variant = variant
        self.X, self.R = data(case, variant)
        self.pri = priors(case, variant)
        if wrong:
            self.backend = lambda *a: _NpWrong(*a, wrong=wrong)

    def _start_state(self, state_seed):
        return state(self.case, self.variant, state_seed)

    def _elbo(self):      # (a wrong model may well give NaN: that is its deviation, not an error of the run)
        return self.b.elbo(self.g_stale)


def run_model(case, variant, schedule, backend="coo", wrong=None):
    """[(return value, every observable)] per call of the schedule."""
    model = GeoModel(case, variant, backend, wrong)
    out = []
    for op in schedule_ops(case, schedule):
        ret = model.apply(op)
        out.append((ret, model.observe()))
    return out


def call_ratios(got_ret, got, want_ret, want, opname, with_rho):
    """{observable: deviation in tolerances} of one call: its return value, the small state, the geometric expectations, rho."""
    r = cs.result_ratios(got_ret, want_ret, opname)
    r.update(cs.state_ratios(got, want, with_rho=with_rho))
    return r


def worst_ratio(a, b, ops):
    """Largest deviation between two runs in tolerances, and where; NaN (one side only) counts as infinite."""
    worst, where = 0.0, None
    for i, ((ra, sa), (rb, sb)) in enumerate(zip(a, b)):
        try:
            r = call_ratios(ra, sa, rb, sb, ops[i]["op"], True)
        except AssertionError:      # (fit_loop: another iteration count or stop decision)
            r = {"decision": np.inf}
        for n, v in r.items():
            v = np.inf if np.isnan(v) else v
            if v > worst:
                worst, where = v, (i, n)
    return worst, where
