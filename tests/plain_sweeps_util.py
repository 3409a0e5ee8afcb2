"""Plain sweeps (a rho update without the ELBO) in every kernel regime: the cases, the schedules of calls, the host model they are
held to and a host restatement of the launch shape (no GPU here, no device code imported).

A fit runs nine plain sweeps for every ELBO sweep, and a plain sweep is not the ELBO sweep minus a term: other kernel variants
(`k_sweep_sl<K, true, false, ..>`, `k_rho<.., true, false, ..>`, mode 0 of `gen_rho`) with their own workgroup caps, the 8-byte
log-prior difference at K = 2, another launch shape on the same handle where LDS is tight, a rho that is not written (mode 4,
read back through `ensure_rho` with the stale nu factor), and statistics that only the NEXT sweep reads.  `CASES` names the
smallest handle of each regime, `SCHEDULES` the call orders that expose what a plain sweep leaves behind; `PlainModel` mirrors
them call by call on an oracle with the rules of `tests.call_sequence_util.SeqModel` (the ELBO's nu factor is that model's).

`shape_of` restates `sl_smem`, the shrink loop of `sl_shape`, `sl_tpb_max` / `sl_wpe` (vimure_amd/csrc/sweep_sl.h) and the level
choice of `create_tail` (`best`, `waves`; vimure_amd/csrc/create.hip) from their header comments and formulas, so that a case
can say on the host which levels each variant keeps in LDS.

tests/test_plain_sweeps_host.py holds every case to its class, the two oracles to each other and shows three forgetful models
caught; tests/test_hip_plain_sweeps.py runs cases x schedules on the device (`make_engine`: the handle, asserted to be of the
case's family); tests/geo_zero_util.py reuses the cases, the model and the handle where a geometric expectation is 0."""
import numpy as np

from tests import call_sequence_util as cs

SL_PF = 8                    # rounds of a step the straight-line bodies hold (sweep_sl.h)
SP_LDS_MAX = 160 * 1024      # LDS of one workgroup on gfx950
HC_MAX = 3                   # dense tiles: levels of H in LDS at most
KMAX = 8                     # categories of the specialised kernels
NCU = 256                    # compute units of an MI355X (the small-dataset rule of create_tail halves the workgroups by it)
TPB_DENSE = 256              # workgroup of the dense tile kernels
QCAP = 6


# ------------------------------------------------------------------------------------------------------------------ the data
class CooTensor:
    """A count tensor given by its coordinates only (the far-list case: N > 1024 with M = 1000 is 1 GB as a dense array)."""

    def __init__(self, subs, vals, shape):
        self.subs, self.vals, self.shape = tuple(np.asarray(s) for s in subs), np.asarray(vals), tuple(shape)

    def sum(self, dtype=None):
        return self.vals.sum(dtype=dtype)


def coo_of(X):
    """((l, i, j, m), counts) of a dense tensor or a CooTensor."""
    if isinstance(X, CooTensor):
        return X.subs, X.vals
    sx = np.nonzero(X)
    return sx, X[sx]


def mirror_counts(X):
    """Per report: the count the same reporter gave the reversed tie, X[l, j, i, m] (the report's level)."""
    (l, i, j, m), v = coo_of(X)
    if not isinstance(X, CooTensor):
        return X[l, j, i, m].astype(np.int64)
    L, N, _, M = X.shape
    key = ((l.astype(np.int64) * N + i) * N + j) * M + m
    rkey = ((l.astype(np.int64) * N + j) * N + i) * M + m
    order = np.argsort(key)
    pos = np.searchsorted(key[order], rkey)
    pos[pos >= key.size] = 0
    hit = key[order][pos] == rkey
    return np.where(hit, v[order][pos], 0).astype(np.int64)


def reports_per_tie(X):
    (l, i, j, m), _ = coo_of(X)
    L, N, _, M = X.shape
    return np.bincount((l.astype(np.int64) * N + i) * N + j, minlength=L * N * N)


def _mirrored(g, L, N, M, dens, p_mirror, xmax=3):
    """Counts 1..xmax at density dens; a share p_mirror of the reports is answered on the reversed tie by the same reporter."""
    X = (g.rand(L, N, N, M) < dens) * g.randint(1, xmax + 1, size=(L, N, N, M))
    mir = (np.transpose(X, (0, 2, 1, 3)) > 0) & (g.rand(L, N, N, M) < p_mirror)
    return np.maximum(X, mir * g.randint(1, xmax + 1, size=(L, N, N, M)))


def _mask(g, shape, kind):
    if kind == "ones":
        return None
    return (g.rand(*shape) < 0.7).astype(np.uint8)


def _family(family, K, N, M, seed, mut=True, coo=False):
    def build():
        X, R = cs.build_data(family, seed=seed, N=N, M=M)
        return X, R, K, mut, "coo" if coo else "dense", seed
    return build


def _mirror_case(K, N, M, dens, mask, seed, p_mirror=0.5):
    def build():
        g = np.random.RandomState([seed, K, N, M])
        X = _mirrored(g, 2, N, M, dens, p_mirror)
        R = _mask(g, X.shape, mask)
        if R is not None:
            X = X * R
        return np.ascontiguousarray(X, dtype=np.uint8), R, K, True, "dense", seed
    return build


def _wide_case(seed):
    """One reporter gives a tie and its reverse a count of 3000 (beyond 11 bits: two-word entries).  Alone such a count overflows the
    reference's raw exponentials (x log(rate) without the constant log x!); answered by the same count on the reversed tie, and with
    E[nu] of the order of one in the state (nu_mean), the mutuality term carries it and the update stays in range."""
    def build():
        X, R = cs.build_data("words", seed=seed, N=33, M=40)
        X = X.astype(np.int32)
        l, i, j, m = (int(a[0]) for a in np.nonzero(X * (np.arange(33)[:, None, None] != np.arange(33)[None, :, None])))
        X[l, i, j, m] = X[l, j, i, m] = 3000
        R[l, i, j, m] = R[l, j, i, m] = 1
        return X, R, 3, True, "coo", seed
    return build


def _far_case(seed):
    """N = 1025 nodes, 1000 reporters, K = 3 (the wide reporter dimension of BASELINE config 5): five ties per node, eight reports
    per tie, half of them answered on the reversed tie; counts 1 and 2, and 3 for one report in ten -- the level beyond the three
    that fit in LDS beside the other table."""
    def build():
        g = np.random.RandomState(seed)
        N, M = 1025, 1000
        i = np.repeat(np.arange(N), 5)
        j = (i + 1 + g.randint(0, N - 1, size=i.size)) % N
        i, j = np.repeat(i, 8), np.repeat(j, 8)
        m = g.randint(0, M, size=i.size)
        back = g.rand(i.size) < 0.5
        i, j, m = np.concatenate([i, j[back]]), np.concatenate([j, i[back]]), np.concatenate([m, m[back]])
        key, first = np.unique((i.astype(np.int64) * N + j) * M + m, return_index=True)
        i, j, m = i[first], j[first], m[first]
        v = np.where(g.rand(i.size) < 0.1, 3, g.randint(1, 3, size=i.size)).astype(np.int32)
        X = CooTensor((np.zeros(i.size, np.int64), i, j, m), v, (1, N, N, M))
        return X, None, 3, True, "coo", seed
    return build


# ----------------------------------------------------------------------------------------------------------------- the cases
SP = {"VMR_FORMAT": "sparse"}
RHO, NOSTORE = "rho", "rho_nostore"      # names of vimure_amd._lib.KERNEL_NAMES


def _c(build, env, fmt, mask=None, passes=None, lazy_kernel=False, claims=(), **kw):
    """lazy_kernel: a one-pass handle on which `launch_rho`'s `lazy` condition holds (the inner sweeps of step(n) are
    VMR_KERNEL_RHO_NOSTORE launches); claims: the classes tests/test_plain_sweeps_host.py asserts from X, R and shape_of."""
    return dict(build=build, env=dict(env), fmt=fmt, mask=mask, passes=passes, kernels=(RHO, NOSTORE) if lazy_kernel else (RHO,),
                claims=tuple(claims), **kw)


CASES = {}
for _K in range(2, 9):
    _N = 33 if _K % 2 == 0 else 65      # (no multiple of 16 or 64; 65 * 65 ties: more than one workgroup's steps)
    CASES[f"k{_K}_ones"] = _c(_family("ones", _K, _N, 17, 10 + _K), SP, "sparse", passes=1, lazy_kernel=True)
    CASES[f"k{_K}_words"] = _c(_family("words", _K, _N, 40, 20 + _K), dict(SP, VMR_NO_RLISTS="1"), "sparse", "words", 1)
    CASES[f"k{_K}_lists"] = _c(_family("self", _K, _N, 40, 30 + _K), SP, "sparse", "lists", 1, lazy_kernel=True)
for _m, _e in (("ones", {}), ("words", {"VMR_NO_RLISTS": "1"}), ("lists", {})):      # K = 2 reading the log prior itself
    CASES[f"k2_{_m}_nolpd"] = dict(CASES[f"k2_{_m}"], env=dict(CASES[f"k2_{_m}"]["env"], VMR_NO_LPD="1", **_e))
for _K, _mk in ((2, "ones"), (3, "words")):
    for _yt, _hc in ((1, 1), (2, 1), (0, 0)):
        CASES[f"levels_beyond_k{_K}_{_yt}{_hc}"] = _c(
            _mirror_case(_K, 65, 40, 0.08, _mk, 40 + _K), dict(SP, VMR_TWO_PASS="0", VMR_YT=str(_yt), VMR_HC=str(_hc)), "sparse",
            passes=1, lazy_kernel=True, claims=("beyond",), levels=_hc)
CASES["tight_lds"] = _c(_mirror_case(3, 40, 1000, 0.004, "ones", 50), SP, "sparse", passes=1, lazy_kernel=True,
                        claims=("beyond", "tight"), levels=3, theta_scale=0.02)
for _K in (2, 3):
    for _mk in ("ones", "words"):
        CASES[f"long_steps_k{_K}_{_mk}"] = _c(_mirror_case(_K, 65, 64, 0.3, _mk, 60 + _K, p_mirror=0.0), SP, "sparse", passes=1,
                                              lazy_kernel=True, claims=("long",))
for _K in (2, 3):
    for _sw in ("", "VMR_NO_LEVEL0", "VMR_NO_X0", "VMR_NO_LV0R"):
        CASES[f"two_pass_k{_K}" + ("_" + _sw[4:].lower() if _sw else "")] = _c(
            _mirror_case(_K, 65, 130, 0.06, "ones", 70 + _K), dict(SP, VMR_TWO_PASS="1", **({_sw: "1"} if _sw else {})), "sparse", passes=2)
CASES["far_lists"] = _c(_far_case(80), dict(SP, VMR_FARL="1"), "sparse", passes=1, claims=("far", "beyond"), levels=3, theta_scale=0.02,
                        far=True, no_numpy=True)
for _K in (2, 3, 5):
    CASES[f"dense_k{_K}"] = _c(_family("words", _K, 33, 40, 90 + _K), {"VMR_FORMAT": "dense"}, "dense", passes=1)
CASES["dense_two_pass"] = _c(_family("words", 3, 33, 300, 95), {"VMR_FORMAT": "dense"}, "dense", passes=2, claims=("dense_two_pass",),
                             theta_scale=0.1)
for _K in (9, 16, 70):
    CASES[f"general_k{_K}"] = _c(_family("ones", _K, 33, 40, 100 + _K, coo=True), {}, "sparse")
CASES["general_wide"] = _c(_wide_case(110), {}, "sparse", nu_mean=0.3)
CASES["nomut_lists"] = _c(_family("words", 2, 33, 40, 120, mut=False), SP, "sparse", "lists", 1, lazy_kernel=True)
CASES["nomut_dense"] = _c(_family("words", 3, 33, 40, 121, mut=False), {"VMR_FORMAT": "dense"}, "dense", passes=1)
CASES["nomut_general"] = _c(_family("ones", 9, 33, 40, 122, mut=False, coo=True), {}, "sparse")
CASES["det_k2_words"] = dict(CASES["k2_words"], env=dict(CASES["k2_words"]["env"], VMR_DETERMINISTIC="1"), det=True)
CASES["det_two_pass"] = dict(CASES["two_pass_k3"], env=dict(CASES["two_pass_k3"]["env"], VMR_DETERMINISTIC="1"), det=True)
CASES["graphs"] = dict(CASES["k5_words"], env=dict(CASES["k5_words"]["env"], VMR_GRAPH="1"), graph=True)


def _step(n, elbo=False, compare=True):
    return {"op": "step", "n": n, "want_elbo": elbo, "compare": compare}


# every schedule starts from set_state (added by `schedule_ops`); compare: get_state() with rho is held after the call
SCHEDULES = {
    "each": [_step(1), _step(1), _step(1)],
    "inner": [_step(3), _step(1, elbo=True)],
    "mixed": [_step(2, compare=False), {"op": "elbo", "compare": False}, _step(2, elbo=True)],
}
GRAPH_SCHEDULE = [_step(11), _step(1, elbo=True)]      # a 9-sweep chunk plus 2, then what they left behind


def schedule_ops(case, schedule):
    seed = built(case)[5]
    ops = GRAPH_SCHEDULE if schedule == "graph" else SCHEDULES[schedule]
    return [{"op": "set_state", "state_seed": 1000 + seed, "priors": None, "compare": False}] + [dict(o) for o in ops]


def schedules_of(case):
    spec = CASES[case]
    return ("inner",) if spec.get("det") else ("graph",) if spec.get("graph") else tuple(SCHEDULES)


_BUILT = {}


def built(case):
    """(X, R, K, mutuality, entry point, seed) of a case, built once and read-only from then on."""
    if case not in _BUILT:
        out = CASES[case]["build"]()
        for a in out[:2]:
            if isinstance(a, np.ndarray):
                a.flags.writeable = False
        _BUILT[case] = out
    return _BUILT[case]


# ------------------------------------------------------------------------------------------------------------ the launch shape
def sl_light(K, elbo, allfull, update):
    return (not elbo) and allfull and (K <= 2 or ((not update) and K <= 4))      # the variant fits 128 registers


def sl_tpb_max(K, elbo, allfull, update=True):
    """Largest workgroup a sweep variant is compiled for."""
    if elbo:
        return 768 if K <= 2 else 512 if K <= 4 else 256
    return 1024 if sl_light(K, elbo, allfull, update) else 768 if K <= 3 else 512 if K <= 7 else 256


def sl_wpe(K, elbo, allfull, update=True):
    """... and its waves per SIMD."""
    if elbo:
        return 3 if K <= 2 else 2 if K <= 4 else 1
    return 4 if sl_light(K, elbo, allfull, update) else 3 if K <= 3 else 2 if K <= 7 else 1


def sl_smem(Mp, W, K, ml, yt, hc, update, elbo, hist):
    """LDS bytes of one workgroup of the sweep kernel: yt levels of F and hc of H ([Mp][K] doubles each), E[theta] (and its
    logarithm for the update), the mask words' sums, the list table of a handle with mask lists, the reduction scratch and --
    ELBO variants only -- the 2 KB logarithm table."""
    lb = Mp * K * 8
    return ((yt * lb if update else 0) + (hc * lb if hist else 0) + Mp * 8 * (2 if update else 1) + W * 8 + 128
            + ((lb + Mp * 8) if ml else 0) + (64 + (256 if elbo else 0)) * 8 + 16)


def sl_shape(geo, update, elbo, hist):
    """The handle's workgroup and levels, shrunk one level at a time (F first while it holds as many as H) until they fit."""
    tpb_h = geo["sp_tpb"] if (update or elbo) else geo["st_tpb"]
    tpb = max(64, min(tpb_h, sl_tpb_max(geo["K"], elbo, geo["all_full"], update)) & ~63)
    yt, hc = (geo["yt"] if update else 0), (geo["hc"] if hist else 0)
    size = lambda: sl_smem(geo["Mp"], geo["W"], geo["K"], geo["ml"], yt, hc, update, elbo, hist)
    while size() > SP_LDS_MAX and (yt > 0 or hc > 0):
        if yt >= hc and yt > 0:
            yt -= 1
        else:
            hc -= 1
    return dict(tpb=tpb, yt=yt, hc=hc, smem=size())


def shmem_rho_dense(N, M, K, mut, hc, two_pass, update, elbo):
    """LDS of the dense tile kernel k_rho (shmem_rho): the tile pair of edge b, the per-reporter tables, hc levels of H."""
    Mp, W = (M + 15) // 16 * 16, (M + 63) // 64
    stride = Mp if (Mp // 16) % 2 == 1 else Mp + 16
    shmem_q = (TPB_DENSE // 64) * 64 * QCAP * 2
    tables = Mp * 8 * (2 + (K if mut else 0)) + W * 8 + shmem_q + 256
    b = 8
    while b > 1 and (2 * b * b * stride > 48 * 1024 or 2 * b * b * (stride + W * 8 + 2 * K * 8 + 4) + tables > 160 * 1024):
        b >>= 1
    nt = 2 * b * b
    n = nt * stride + nt * W * 8 + W * 8 + Mp * 8 + 64 + (Mp * K * 8 if mut else 0) + 2 * nt * K * 8 + shmem_q
    if update and not two_pass:
        n += hc * Mp * K * 8
    if elbo:
        n += Mp * 8 + nt * 4
    return n + 16


def shape_of(case):
    """What `create_tail` settles on for the case's handle and the shapes `sl_shape` gives its variants: a dict with Mp, W, Y
    (mirror-count levels: max count + 1 with mutuality), ml (mask lists), all_full, two_pass, yt / hc (the handle's), sp_tpb /
    st_tpb, and `plain`, `elbo`, `stat`: {tpb, yt, hc, smem} of the update variant without ELBO, the fused ELBO variant and the
    statistics-only pass.  Handles of the general kernels (K > 8, two-word entries) keep nothing in LDS; dense handles give
    `dense_smem` (the update variant's LDS in one pass) and two_pass."""
    X, R, K, mut, entry, _ = built(case)
    env = CASES[case]["env"]
    L, N, _, M = X.shape
    _, vals = coo_of(X)
    xmax = int(vals.max())
    Y = xmax + 1 if mut else 1
    Mp, W = (M + 15) // 16 * 16, (M + 63) // 64
    out = dict(K=K, Mp=Mp, W=W, Y=Y, N=N, L=L)
    if K > KMAX or xmax > 2047 or (xmax + 1) * Mp > (1 << 20):
        return dict(out, general=True, two_pass=False, yt=0, hc=0)
    if env.get("VMR_FORMAT") == "dense":
        hc = min(Y, HC_MAX)
        one = shmem_rho_dense(N, M, K, mut, hc, False, True, False)
        return dict(out, dense=True, dense_smem=one, two_pass=one > 80000, hc=hc, yt=0)
    all_full = R is None or bool(np.all(R))
    ml = False
    if not all_full:      # partial rows become reporter lists when the longest is short (small networks: whatever the bytes)
        rows = R.sum(axis=-1)
        ml = "VMR_NO_RLISTS" not in env and int(rows[rows < M].max()) <= 64 and N <= 1024
    cap = lambda upd: sl_tpb_max(K, False, all_full, upd)
    wcu = lambda upd: 4 * sl_wpe(K, False, all_full, upd)
    def waves(tpb, yt, hc, upd, hist):
        b = sl_smem(Mp, W, K, ml, yt, hc, upd, False, hist)
        if b > SP_LDS_MAX or tpb > cap(upd):
            return 0
        nw = tpb // 64
        return min(SP_LDS_MAX // b, wcu(upd) // nw) * nw

    def best(upd, hist, min_waves):
        min_waves = min(min_waves, wcu(upd))
        for lv in range(want, 0, -1):
            bw, bt = 0, 256
            for tpb in (1024, 768, 512, 256):
                w = waves(tpb, lv if upd else 0, lv if hist else 0, upd, hist)
                if w > bw:
                    bw, bt = w, tpb
            if bw >= min_waves:
                return lv, bt
        return None
    want = max(1, min(Y, 64))
    one = best(True, True, 16)
    far_frac, farl = None, False
    if one and one[0] < want and N > 1024:      # not every level fits: one pass only while the reports beyond are rare
        far_frac = float((mirror_counts(X) >= one[0]).mean())
        if far_frac > 1.0 / 1024:
            if mut and "VMR_DETERMINISTIC" not in env and env.get("VMR_FARL") == "1" and far_frac <= 0.125:
                farl = True
            else:
                one = None
    forced = env.get("VMR_TWO_PASS")
    if forced == "1":
        one = None
    if one:
        yt = hc = one[0]
        sp_tpb = st_tpb = one[1]
        two_pass = False
    else:
        two_pass = True
        r = best(True, False, 16) or best(True, False, 4) or (0, 256)
        s = best(False, True, 16) or best(False, True, 4) or (0, 256)
        yt, sp_tpb, hc, st_tpb = r[0], r[1], s[0], s[1]
    NS = (N * N + 63) // 64

    def spread(t):      # small datasets: smaller workgroups, so that the steps spread over every compute unit
        while t > 64 and NS * L < NCU * (t // 64):
            t = max(64, (t // 2) & ~63)
        return t
    sp_tpb, st_tpb = spread(sp_tpb), spread(st_tpb)
    if "VMR_YT" in env:
        yt = int(env["VMR_YT"])
    if "VMR_HC" in env:
        hc = int(env["VMR_HC"])
    yt, hc = max(0, min(Y, yt)), max(0, min(Y, hc))
    geo = dict(K=K, Mp=Mp, W=W, ml=ml, all_full=all_full, yt=yt, hc=hc, sp_tpb=sp_tpb, st_tpb=st_tpb)
    hist = not two_pass
    out.update(geo, two_pass=two_pass, farl=farl, far_frac=far_frac, want=want,
               plain=sl_shape(geo, True, False, hist), elbo=sl_shape(geo, True, True, hist), stat=sl_shape(geo, False, False, True))
    return out


# ------------------------------------------------------------------------------------------------------------- the host model
class _CooSparse(cs._Coo):
    """oracle/cavi_coo.c on a CooTensor."""

    def __init__(self, X, R, K, mut, pri, st):
        from oracle import cavi_coo
        assert R is None
        self.c = cavi_coo.CooRef((X.subs, X.vals.astype(np.int32)), None, X.shape, K, mut, pri, *st)


class _Ref(cs._Coo):
    """oracle/cavi_ref.c (the dense C oracle) behind the same interface."""

    def __init__(self, X, R, K, mut, pri, st):
        from oracle import cavi_ref
        self.c = cavi_ref.CRef(X, R, K, mut, pri, *st)


BACKENDS = dict(cs.BACKENDS, ref=_Ref)


def oracle_of(case):
    """The C oracle of a case: cavi_ref for the dense tiles, cavi_coo for the report lists."""
    return "ref" if CASES[case]["fmt"] == "dense" else "coo"


PLAIN_FORGETFUL = ("plain_keeps_old_statistics", "plain_drops_far_levels", "rerun_current_nu")


def case_state(case, state_seed):
    """The state a schedule starts from: `call_sequence_util.draw_state`, E[theta] scaled down where a thousand reporters' worth
    of it in the exponent would underflow every category of a tie (theta_scale), E[nu] = nu_mean where a case asks for it."""
    X, _, K, mut = built(case)[:4]
    st = cs.draw_state(np.random.RandomState(state_seed), X, K, mut)
    nu_shp = st[4] if "nu_mean" not in CASES[case] else CASES[case]["nu_mean"] * st[5]
    return (st[0] * CASES[case].get("theta_scale", 1.0),) + tuple(st[1:4]) + (nu_shp,) + tuple(st[5:])


class PlainModel(cs.SeqModel):
    """`SeqModel` for the calls of SCHEDULES on a case (its `_update`, `_sweep` and `_elbo` are the rules: the ELBO's nu factor is
    the one from before the last nu update).  forget: one of PLAIN_FORGETFUL --
      plain_keeps_old_statistics: after a plain sweep, gamma and phi of the next sweep see the rho of the sweep before;
      plain_drops_far_levels: a plain sweep's statistics (the next gamma / phi shapes, its own nu) miss the reports whose mirror
        count is >= `drop_from` (they are taken out of the tensor the statistics are summed over);
      rerun_current_nu: a rho read (or a stand-alone ELBO) after a plain step sees a rho re-made with the CURRENT nu factor."""

    def __init__(self, case, backend="coo", forget=None, drop_from=None):
        X, R, K, mut = built(case)[:4]
        assert forget is None or forget in PLAIN_FORGETFUL
        super().__init__(X, R, K, mut, "coo", None)
        self.backend = BACKENDS[backend]
        if isinstance(X, CooTensor):
            assert backend == "coo"
            self.backend = _CooSparse
        self.case, self.pforget, self.drop_from = case, forget, drop_from
        self.stat_rho = self.Xd = None
        self.after_plain = False
        if forget == "plain_drops_far_levels":
            Xd = np.array(X)
            Xd[np.transpose(X, (0, 2, 1, 3)) >= drop_from] = 0
            self.Xd = Xd

    def _start_state(self, state_seed):
        return case_state(self.case, state_seed)

    def _on(self, Xalt, whichs, keys):
        """Updates `whichs` computed over another tensor from the present state; only `keys` come back."""
        s = self.b.get()
        alt = self.backend(Xalt, self.R, self.K, self.mut, self.pri, self.state)
        alt.put(s)
        for w in whichs:
            alt.update(w)
        t = alt.get()
        self.b.put({k: t[k] for k in keys})

    def _plain_sweep(self, plain):
        if self.pforget == "plain_keeps_old_statistics" and self.stat_rho is not None:
            rho = self.b.get()["rho"]
            self.b.put({"rho": self.stat_rho})
            self._update("GAMMA")
            self._update("PHI")
            self.b.put({"rho": rho})
        elif self.Xd is not None and self.after_plain:
            self.prte = True
            self._on(self.Xd, ("GAMMA", "PHI"), cs.PARAMS[:4])
        else:
            self._update("GAMMA")
            self._update("PHI")
        before = self.b.get()["rho"]
        self._update("RHO")
        pre = self.b.get()
        self._update("NU")      # (keeps the ELBO's factor)
        if self.Xd is not None and plain and self.mut:
            self.b.put({"nu_shp": pre["nu_shp"], "nu_rte": pre["nu_rte"]})
            self._on(self.Xd, ("NU",), ("nu_shp", "nu_rte"))
        self.stat_rho = before if plain else None
        self.after_plain = plain

    def apply(self, op):
        name = op["op"]
        if name == "set_state":
            self.last = name
            self.state = self._start_state(op["state_seed"])
            self.b = self.backend(self.X, self.R, self.K, self.mut, self.pri, self.state)
            self.g_stale = self._g()
            self.restored, self.hidden_rho, self.rho_before, self.prte, self.old_rho = False, None, None, False, None
            self.stat_rho, self.after_plain = None, False
            return None
        if name == "step":
            self.last = name
            self.hidden_rho = None
            for q in range(op["n"]):
                self._plain_sweep(not (op["want_elbo"] and q == op["n"] - 1))
            if self.pforget == "rerun_current_nu" and op["n"] > 0 and not op["want_elbo"]:
                s = self.b.get()
                self.b.update("RHO")      # gamma and phi are the pass's, nu is not: the commit came after it
                self.hidden_rho = self.b.get()["rho"]
                self.b.put(s)
            return self._elbo() if op["want_elbo"] else None
        if name == "elbo" and self.hidden_rho is not None:
            s = self.b.get()
            self.b.put({"rho": self.hidden_rho})
            e = self._elbo()
            self.b.put(s)
            return e
        return super().apply(op)


def run_model(case, schedule, backend="coo", forget=None, drop_from=None):
    """[(return value, observables or None)] per call of the schedule."""
    model = PlainModel(case, backend, forget, drop_from)
    out = []
    for op in schedule_ops(case, schedule):
        ret = model.apply(op)
        out.append((ret, model.observe() if op["compare"] else None))
    return out


def make_engine(case, monkeypatch, extra=None, data=None, priors=cs.PRI):
    """The case's handle under its switches (and `extra`), asserted to be of the case's family; data: (X, R) other than the
    case's own (tests/geo_zero_util.py takes reports out), priors: what `set_priors` gets."""
    from vimure_amd import CaviEngine
    spec = CASES[case]
    for k in cs.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(spec["env"], **(extra or {})).items():
        monkeypatch.setenv(k, v)
    X, R, K, mut, entry, _ = built(case)
    if data is not None:
        X, R = data
    if entry == "coo":
        subs, vals = coo_of(X)
        eng = CaviEngine.from_coo(subs, vals, X.shape, R=None if R is None else np.nonzero(R), K=K, mutuality=mut)
    else:
        eng = CaviEngine(X, R, K=K, mutuality=mut)
    fmt, mask, (passes, levels, far) = eng.data_format()[0], eng.mask_format()[0], eng.sweep_shape()
    assert fmt == spec["fmt"], (case, fmt)
    assert spec["mask"] is None or mask == spec["mask"], (case, mask)
    assert spec["passes"] is None or passes == spec["passes"], (case, passes, levels, far)
    assert spec.get("levels") is None or levels == spec["levels"], (case, passes, levels, far)
    assert (far > 0) == bool(spec.get("far")), (case, passes, levels, far)
    eng.set_priors(*priors)
    return eng


def worst_ratio(a, b):
    """Largest deviation between two runs of `run_model` (or a device run in the same form), in tolerances; and where."""
    worst, where = 0.0, None
    for i, ((ra, sa), (rb, sb)) in enumerate(zip(a, b)):
        r = {}
        if rb is not None:
            r["elbo"] = cs.ratio(ra, rb, "elbo")
        if sb is not None:
            r.update({n: cs.ratio(sa[n], sb[n], n) for n in cs.PARAMS + ("rho",)})
        for n, v in r.items():
            if not v <= worst:
                worst, where = v, (i, n)
    return worst, where
