"""Shared by tests/test_hip_influence.py: the inputs, the reference and the bounds that hold vmr_reporter_influence to its NumPy
restatement (`influence.influence_np`).

Exact: `counts`, `hist`, and the set and order of the flagged rows with their x and xt.  What makes exactness fair: no element is
borderline, and `reference` asserts that about the test's own inputs, leaving no element out --
  the readout margin of EVERY element (rho_max: |q_0 - max_{k>=1} q_k|; threshold: |q_1 - threshold|) is at least GAP_RULE = 1000
  times the element's float bound;
  `pick` puts min_tv and every edge at the MIDPOINT OF A GAP between consecutive distinct reference tv values whose width is at
  least 1000 times the bound of both its neighbours.
Floating point, of every element (a second call with min_tv = 0):
  prob, prob_loo, tv   |got - want| <= C_INF 2^-52 (T + 1),  T = max over the categories with rho_k > 0 of
                       |x w1_k (elog_theta + elog_lambda_k)| + e_theta e_lambda_k: the size of the terms in the exponent
  sums                 n_scope q / 2 (`influence.sum_quantum`: every term rounded to the fixed point) plus the elements' own bounds,
                       plus n 2^-52 sum |v| for the reference's own double sum of n terms

C_INF is four times the worst |got - want| / (2^-52 (T + 1)) measured on an MI355X over the cases of tests/test_hip_influence.py
against the restatement, and never above 64: see the figure beside the constant.  A dropped or wrong term is an error of order
min(1, T), about 2^52 times the bound: the constant hides nothing."""
import numpy as np
from scipy.special import psi

from tests.golden_util import case_config, load_case

U = 2.0 ** -52
C_INF = 2.27   # 4 x the measured worst 0.5658 (prob_loo, golden B_random_mask_K3; K12: 0.4570, M70_K3: 0.4377; prob: 0 everywhere)
GAP_RULE = 1000.0
PRI = (0.1, 0.1, 10.0, 10.0, 0.5, 1.0)
ROWS = ("l", "i", "j", "m", "x", "xt")
VALS = ("prob", "prob_loo", "tv")

# the synthetic shapes: the smallest that reach every branch (seed, L, N, M, K, density)
SHAPES = {
    "M70_K3": (41, 2, 18, 70, 3, 0.5),     # two rounds per tie, two mask words, several workgroups, empty and all-ones rows, a zero category
    "M70_K2": (42, 2, 18, 70, 2, 0.5),     # the same layout with K = 2
    "N48_K2": (43, 1, 48, 5, 2, None),     # G = 8, 2304 ties > one workgroup's 2048, no mask
    "K12": (44, 2, 12, 9, 12, 0.4),        # K > KMAX: the row streamed
}
_cache = {}


def tables(st, mut):
    """(e_theta, elog_theta, e_lambda, elog_lambda, g_nu) of a state (gamma_shp, gamma_rte, phi_shp, phi_rte, nu_shp, nu_rte, ..)."""
    gs, gr, ps, pr = (np.asarray(a, dtype=np.float64) for a in st[:4])
    g_nu = float(np.exp(psi(float(st[4])) - np.log(float(st[5])))) if mut else 0.0
    return gs / gr, psi(gs) - np.log(gr), ps / pr, psi(ps) - np.log(pr), g_nu


def synthetic(name, mut=True):
    """The `_synthetic` recipe of tests/test_hip_report_scores.py at one of SHAPES."""
    key = (name, mut)
    if key in _cache:
        return _cache[key]
    seed, L, N, M, K, density = SHAPES[name]
    g = np.random.RandomState(seed)
    X = ((g.rand(L, N, N, M) < 0.2) * g.randint(1, 5, (L, N, N, M))).astype(np.int64)
    R = None
    if density is not None:
        R = (g.rand(L, N, N, M) < density).astype(np.uint8)
        R[:, 2] = 0                               # empty rows
        R[:, 3], R[0, :, 5] = 1, 1                # rows made all ones
    rho = g.rand(L, N, N, K)
    rho[..., 0] *= 4.0
    if K > 2:
        rho[:, ::3, 1::2, K - 2] = 0.0            # a zero category
    rho = np.ascontiguousarray(rho / rho.sum(-1, keepdims=True))
    gs, gr = g.gamma(2.0, 1.0, (L, M)) + 0.1, g.gamma(2.0, 1.0, (L, M)) + 0.1
    ps, pr = g.gamma(5.0, 1.0, (L, K)) + 0.1, g.gamma(2.0, 1.0, (L, K)) + 0.1
    st = (gs, gr, ps, pr, 3.0, 2.5, rho)
    _cache[key] = dict(name=f"{name}{'' if mut else ' nomut'}", X=X, R=R, K=K, mut=mut, st=st, rho=rho, tabs=tables(st, mut), ref={})
    return _cache[key]


def golden(name):
    """A golden fit: the state of its `fit_*_f` arrays."""
    if name in _cache:
        return _cache[name]
    d = load_case(name)
    K, mut, _, _, _, _, _ = case_config(d)
    X, R = np.asarray(d["X"]).astype(np.int64), np.asarray(d["R"])
    st = (d["fit_gamma_shp_f"], d["fit_gamma_rte_f"], d["fit_phi_shp_f"], d["fit_phi_rte_f"], float(d["fit_nu_shp_f"]),
          float(d["fit_nu_rte_f"]), np.ascontiguousarray(d["fit_rho_f"]))
    _cache[name] = dict(name=name, X=X, R=None if R.all() else R, K=K, mut=mut, st=st, rho=st[6], tabs=tables(st, mut), ref={})
    return _cache[name]


def engine(c, coo=False):
    from vimure_amd import CaviEngine
    X, R = c["X"], c["R"]
    if coo:
        xs = np.nonzero(X)
        eng = CaviEngine.from_coo(xs, X[xs], X.shape, R=None if R is None else np.nonzero(R), K=c["K"], mutuality=c["mut"])
    else:
        eng = CaviEngine(X.astype(np.uint8), R, K=c["K"], mutuality=c["mut"])
    eng.set_priors(*PRI)
    eng.set_state(*c["st"])
    return eng


def term_size(c, al):
    """T [n] of the elements of a reference table (see the module docstring)."""
    from vimure_amd.influence import _exp_table
    e_th, el_th, e_la, el_la, g_nu = c["tabs"]
    l, m = al["l"], al["m"]
    z1 = _exp_table(el_th)[l, m][:, None] * _exp_table(el_la)[l]
    den = z1 + (g_nu * al["xt"])[:, None]
    den[den == 0.0] = 1.0
    t = np.abs(al["x"][:, None] * (z1 / den) * (el_th[l, m][:, None] + el_la[l])) + e_th[l, m][:, None] * e_la[l]
    r = c["rho"][al["l"], al["i"], al["j"]]
    return np.where(r > 0.0, t, 0.0).max(axis=1)


def reference(c, method="rho_max", threshold=0.0):
    """Every element of the support by the restatement, its T and float bound, and the gaps between distinct tv values that
    satisfy the rule: a dict with al, T, bound, gaps = [(midpoint, width)], vals.  Asserts that no readout is borderline."""
    from vimure_amd.influence import influence_np
    key = (method, threshold)
    if key in c["ref"]:
        return c["ref"][key]
    al = influence_np(c["rho"], c["X"], c["R"], *c["tabs"], mutuality=c["mut"], method=method, threshold=threshold, select="none",
                      min_tv=0.0)
    T = term_size(c, al)
    bound = C_INF * U * (T + 1.0)
    q = al["q"]
    margin = np.abs(q[:, 1] - threshold) if method == "threshold" else np.abs(q[:, 0] - q[:, 1:].max(axis=1))
    worst = float((margin / bound).min())
    print(f"{c['name']} {method}: {len(T)} elements, T up to {T.max():.3f}, smallest readout margin {margin.min():.3e} = {worst:.3e} bounds")
    assert worst >= GAP_RULE, (c["name"], worst)
    vals, inv = np.unique(al["tv"], return_inverse=True)
    vb = np.zeros(len(vals))
    np.maximum.at(vb, inv, bound)                                      # the widest bound among the elements that share a value
    width = np.diff(vals)
    ok = width >= GAP_RULE * np.maximum(vb[:-1], vb[1:])
    gaps = [(0.5 * (vals[k] + vals[k + 1]), width[k]) for k in np.flatnonzero(ok)]
    c["ref"][key] = dict(al=al, T=T, bound=bound, gaps=gaps, vals=vals)
    return c["ref"][key]


def pick(c, ref, n_edges=9):
    """min_tv -- the midpoint of the qualifying gap nearest to the 98 % quantile of tv, so that about one element in fifty is
    flagged by its shift -- and edges at qualifying gaps spread over the distinct values."""
    gaps, vals, tv = ref["gaps"], ref["vals"], ref["al"]["tv"]
    assert len(gaps) >= n_edges, (len(gaps), len(vals))
    q98 = float(np.quantile(tv, 0.98))
    thr = min(gaps, key=lambda g: abs(g[0] - q98))
    assert vals[0] < thr[0] < vals[-1]
    edges = sorted({gaps[int(round(p * (len(gaps) - 1)))][0] for p in np.linspace(0.0, 1.0, n_edges)} | {thr[0]})
    print(f"{c['name']}: min_tv {thr[0]:.6f} in a gap of {thr[1]:.3e}; {len(edges)} edges; {len(vals)} distinct tv, "
          f"{len(gaps)} gaps satisfy the rule ({100.0 * len(gaps) / max(1, len(vals) - 1):.1f} %)")
    return float(thr[0]), np.array(edges)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def compare_values(got, ref, w, what):
    """prob, prob_loo and tv of every element (rows w of the reference) within C_INF 2^-52 (T + 1); prints the worst ratio."""
    al, T = ref["al"], ref["T"][w]
    worst = 0.0
    for k in VALS:
        g, v = np.asarray(got[k]), al[k][w]
        assert g.shape == v.shape and not np.isnan(g).any(), (what, k)
        ratio = np.abs(g - v) / (U * (T + 1.0))
        worst = max(worst, float(ratio.max(initial=0.0)))
        print(f"{what}: {k} worst ratio |got - want| / (2^-52 (T + 1)) = {ratio.max(initial=0.0):.4f}")
        assert (ratio <= C_INF).all(), (what, k, float(ratio.max()))
    return worst


def compare_sums(got_sums, got_counts, ref, layers, N, what):
    """The fixed-point sums [L', M, 2] against the double sums of the reference's terms."""
    from vimure_amd.influence import sum_quantum
    al, bound = ref["al"], ref["bound"]
    qn = sum_quantum(N)
    M = got_sums.shape[1]
    for a, l in enumerate(layers):
        for col, term in ((0, al["tv"]), (1, al["prob_loo"] - al["prob"])):
            w = al["l"] == l
            want, n, mag, eb = (np.bincount(al["m"][w], weights=v[w], minlength=M) for v in (term, np.ones(len(term)), np.abs(term),
                                                                                              bound * (2.0 if col else 1.0)))
            assert np.array_equal(n.astype(np.int64), got_counts[a, :, 0])
            lim = n * qn / 2 + eb + n * U * mag
            err = np.abs(got_sums[a, :, col] - want)
            print(f"{what} layer {l} sum {col}: worst |got - want| {err.max():.3e}, its bound {lim[np.argmax(err)]:.3e}")
            assert (err <= lim).all(), (what, l, col, float((err - lim).max()))
