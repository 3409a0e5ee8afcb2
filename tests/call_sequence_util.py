"""Random legal sequences of engine calls and the host model they are held to (no GPU here).

The engine never recomputes what it believes is still current: flags in its handle decide which kernels a call launches and which
buffers it trusts.  A mistake there gives no fault and no NaN, only a stale statistic.  `draw_sequence` draws call sequences the
suite's fixed orders never issue; `SeqModel` mirrors every call on an oracle (`oracle.cavi_coo` or the NumPy `oracle.vimure_oracle`)
with the rules of include/vimure_hip.h and DESIGN section 8:

* `STEP_GAMMA`, `STEP_PHI`, `STEP_RHO`, `STEP_NU` and whole sweeps use exp(E[log nu]) of the CURRENT nu;
* `STEP_PHI` commits the rate that the finalize of `STEP_GAMMA` prepares (one pass over the mask sums serves both): it is refused on
  the host unless a `STEP_GAMMA` ran since rho last changed (`set_state`, `STEP_RHO`, any sweep); `STEP_NU` in between is fine.
  Without mutuality `STEP_GAMMA` commits gamma and phi, and `STEP_PHI` does nothing;
* the stand-alone and the fused ELBO use its value from BEFORE the last nu update (`SC_G_NU_STALE`; at `set_state` both are equal);
* `sweep_local` + `commit_nu` on a handle that owns every layer is a sweep, its ELBO assembled as vimure_amd/sharded.py does;
* `snapshot` keeps the posteriors with both factors, `restore` brings them back and leaves the handle read-only: every sweeping
  call is refused on the host and changes nothing, until the next `set_state`;
* a snapshot outlives `set_state`.

tests/test_call_sequence_host.py holds the model on one oracle to the model on the other, asserts the coverage of the committed
sequences and that four forgetful variants of the model would be noticed; tests/test_hip_call_sequences.py runs the sequences on
the device; tools/fuzz_parity.py `seq` draws longer ones."""
import numpy as np
from scipy.special import gammaln, psi

PRI = (0.1, 0.1, 10.0, 10.0, 0.5, 1.0)
OPS = ("set_state", "step", "sub_step", "elbo", "sweep_commit", "fit_loop", "snapshot", "restore", "refused")
SWEEPING = ("step", "sub_step", "elbo", "sweep_commit", "fit_loop")
SUBS = ("GAMMA", "PHI", "RHO", "NU")
# readers: the two small ones run after EVERY operation on the device, the others where the generator marks them
SMALL_READERS = ("get_state_small", "get_geometric")
MARKED_READERS = ("get_state_rho", "readout", "sample", "expected_stats", "edge_table_size")
READERS = SMALL_READERS + MARKED_READERS
PARAMS = ("gamma_shp", "gamma_rte", "phi_shp", "phi_rte", "nu_shp", "nu_rte")
GEO = ("G_theta", "G_lambda", "g_nu", "g_nu_stale")
MAX_SWEEPS = 8          # sweep-equivalents between two set_states, beside at most one long call (step(11), fit_loop)
READ_ONLY = "read-only until the next vmr_set_state"
NO_SUB_STEP = "vmr_sub_step is not available with VMR_DETERMINISTIC=1"
NO_SNAPSHOT = "vmr_snapshot must be called before vmr_restore"
NO_PHI = "VMR_STEP_PHI commits the rate that VMR_STEP_GAMMA prepares"

# kind -> data family, K, mutuality, switches, coordinate-list entry point, what the handle must report
#   fmt: data_format()[0]; mask: mask_format()[0] (None: not asserted, no partial row); passes: sweep_shape()[0]
KINDS = {
    "lists_k2_ones": dict(data="ones", K=2, env={"VMR_FORMAT": "sparse"}, fmt="sparse", mask=None, passes=1),
    # (a small network gets reporter lists for any partial mask: VMR_NO_RLISTS=1 keeps the mask words; `nomut` takes the lists)
    "lists_k2_words": dict(data="words", K=2, env={"VMR_FORMAT": "sparse", "VMR_NO_RLISTS": "1"}, fmt="sparse", mask="words", passes=1),
    "lists_k3_selfmask": dict(data="self", K=3, env={"VMR_FORMAT": "sparse"}, fmt="sparse", mask="lists", passes=1),
    "lists_two_pass": dict(data="long", K=3, env={"VMR_FORMAT": "sparse", "VMR_TWO_PASS": "1"}, fmt="sparse", mask=None, passes=2),
    "dense_k3": dict(data="words", K=3, env={"VMR_FORMAT": "dense"}, fmt="dense", mask=None, passes=None),
    "general_k9": dict(data="ones", K=9, env={}, coo=True, fmt="sparse", mask=None, passes=None),
    "nomut": dict(data="words", K=2, env={"VMR_FORMAT": "sparse"}, mut=False, fmt="sparse", mask="lists", passes=1),
    "graphs": dict(data="ones", K=2, env={"VMR_FORMAT": "sparse", "VMR_GRAPH": "1"}, fmt="sparse", mask=None, passes=1),
    "lazy": dict(data="self", K=3, env={"VMR_FORMAT": "sparse", "VMR_DEBUG_LAZY_RHO": "1"}, fmt="sparse", mask="lists", passes=1),
    "det": dict(data="words", K=2, env={"VMR_FORMAT": "sparse", "VMR_NO_RLISTS": "1", "VMR_DETERMINISTIC": "1"}, det=True, fmt="sparse", mask="words",
                passes=1),
}
# handles for hand-written sequences only (no committed random sequence draws them)
EXTRA_KINDS = {
    "det_lists": dict(data="words", K=2, env={"VMR_FORMAT": "sparse", "VMR_DETERMINISTIC": "1"}, det=True, fmt="sparse", mask="lists", passes=1),
    "det_k3_words": dict(data="words", K=3, env={"VMR_FORMAT": "sparse", "VMR_NO_RLISTS": "1", "VMR_DETERMINISTIC": "1"}, det=True, fmt="sparse",
                         mask="words", passes=1),
}


def spec_of(kind):
    return KINDS[kind] if kind in KINDS else EXTRA_KINDS[kind]
SWITCHES = ("VMR_FORMAT", "VMR_NO_LPD", "VMR_TWO_PASS", "VMR_YT", "VMR_HC", "VMR_FARL", "VMR_NO_LEVEL0", "VMR_NO_X0", "VMR_NO_LV0R",
            "VMR_DETERMINISTIC", "VMR_DEBUG_LAZY_RHO", "VMR_TPB", "VMR_ST_TPB", "VMR_GRAPH", "VMR_NO_LEVEL_SORT", "VMR_NO_RLISTS", "VMR_NO_RM2", "VMR_NO_LP0", "VMR_ALWAYS_STORE_RHO")
SEEDS = (0, 1, 2, 3, 4)
SALT = 57   # of the draw: chosen so that the committed seeds meet the coverage counts of tests/test_call_sequence_host.py
SHAPES = {"ones": (33, 17), "words": (33, 40), "self": (40, 40), "long": (33, 65)}   # (N, M); L = 2: no multiple of 16 or 64 in N


def build_data(family, seed=0, N=None, M=None, L=2):
    """X (counts 1..3, every report inside R) and R (None: every reporter on every tie) of one data family."""
    n0, m0 = SHAPES[family]
    N, M = n0 if N is None else N, m0 if M is None else M
    g = np.random.RandomState([seed, sorted(SHAPES).index(family), N, M])
    cnt = lambda: g.randint(1, 4, size=(L, N, N, M))
    if family == "ones":      # some ties without any report
        X, R = (g.rand(L, N, N, M) < 0.06) * cnt(), None
    elif family == "words":
        R = (g.rand(L, N, N, M) < 0.7).astype(np.uint8)
        X = (g.rand(L, N, N, M) < 0.08) * cnt() * R
    elif family == "self":    # reporter m reports on the ties that involve node m
        R = np.zeros((L, N, N, M), np.uint8)
        for m in range(min(M, N)):
            R[:, m, :, m] = 1
            R[:, :, m, m] = 1
        X = (g.rand(L, N, N, M) < 0.25) * cnt() * R
    else:                     # long: 9..20 reports per tie, half of them mirrored
        R = (g.rand(L, N, N, M) < 0.9).astype(np.uint8)
        dens = g.uniform(9.5, 19.5, size=(L, N, N, 1)) / (0.9 * M * 1.4)
        X = (g.rand(L, N, N, M) < dens) * cnt()
        mir = (np.transpose(X, (0, 2, 1, 3)) > 0) & (g.rand(L, N, N, M) < 0.5)
        X = np.maximum(X, mir * cnt()) * R
    return np.ascontiguousarray(X, dtype=np.uint8), R


def draw_priors(g):
    return (float(g.uniform(0.05, 0.3)), float(g.uniform(0.05, 0.3)), float(g.uniform(5, 15)), float(g.uniform(5, 15)),
            float(g.uniform(0.3, 0.9)), float(g.uniform(0.5, 2.0)))


def draw_state(g, X, K, mutuality):
    L, N, _, M = X.shape
    pr = g.rand(L, N, N, K) + 0.05
    pr /= pr.sum(-1, keepdims=True)
    nu = (0.4 + 0.6 * g.rand(), 1.0 + float(X.sum(dtype=np.int64))) if mutuality else (1e-6, 1.0)
    return (0.5 + g.rand(L, M), 0.5 + g.rand(L, M), 1 + g.rand(L, K), 1 + g.rand(L, K), float(nu[0]), float(nu[1]), pr)


# ------------------------------------------------------------------------------------------------------ the sequence generator
def legal_pair(a, b):
    """Whether operation b may directly follow operation a on some handle (after `restore` only readers, `restore`, `snapshot`,
    refused calls and `set_state`)."""
    return not (a == "restore" and b in SWEEPING)


LEGAL_PAIRS = tuple((a, b) for a in OPS for b in OPS if legal_pair(a, b))


def draw_sequence(seed, kind, n_ops=None, sid=None):
    """The operations of (seed, kind): a list of dicts {"op", parameters, "readers": marked readers run after it}.  Deterministic.
    10 to 16 operations unless n_ops says otherwise; at most MAX_SWEEPS sweep-equivalents between two set_states beside one long
    call; one block restore -> refused -> set_state -> sweep in every sequence; the last operation gets every reader.
    sid steers the draw towards three of LEGAL_PAIRS so that the committed seeds cover all of them."""
    spec = KINDS[kind]
    kidx = list(KINDS).index(kind)
    g = np.random.RandomState([seed, kidx, SALT])
    det, mut = bool(spec.get("det")), spec.get("mut", True)
    if n_ops is None:
        n_ops = int(g.randint(10, 17))
    if sid is None:
        sid = seed * len(KINDS) + kidx
    targets = [LEGAL_PAIRS[(3 * sid + q) % len(LEGAL_PAIRS)] for q in range(3)] * 2
    block_at = int(g.randint(4, max(5, n_ops - 4)))
    ops = []
    ctx = dict(budget=0.0, long=False, snap=False, restored=False, n_set=0, prte=False)

    def allowed(ctx_):
        if ctx_["restored"]:
            return {"refused": 1.0, "restore": 0.8, "snapshot": 0.4, "set_state": 3.0}
        w = {"set_state": 0.5, "elbo": 3.0, "snapshot": 0.8, "step": 3.0}
        room = ctx_["budget"] < MAX_SWEEPS
        if room:
            w["sweep_commit"] = 1.5
            if not det:
                w["sub_step"] = 4.5
            w["fit_loop"] = 1.2
        if ctx_["snap"]:
            w["restore"] = 0.3
        if det or not ctx_["snap"]:
            w["refused"] = 1.6
        return w

    def emit(name):
        op = {"op": name}
        if name == "set_state":
            op["state_seed"] = int(g.randint(1 << 30))
            op["priors"] = draw_priors(g) if (ctx["n_set"] > 0 and g.rand() < 0.5) else None
            ctx.update(budget=0.0, long=False, restored=False, n_set=ctx["n_set"] + 1, prte=False)
        elif name == "step":
            room = int(MAX_SWEEPS - ctx["budget"])
            ns = [n for n in (0, 1, 2, 3) if n <= room] + ([11] if not ctx["long"] else [])
            n = int(ns[g.randint(len(ns))])
            op["n"], op["want_elbo"] = n, bool(g.rand() < 0.5)
            if n == 11:
                ctx["long"] = True
            else:
                ctx["budget"] += n
            if n > 0:
                ctx["prte"] = False
        elif name == "sub_step":
            op["which"] = SUBS[g.randint(4)]
            if ops[-1].get("which") == "RHO" and g.rand() < 0.6:      # (the mask sums of a rho sub-step, consumed by the next gamma)
                op["which"] = "GAMMA"
            elif ctx["prte"] and g.rand() < 0.5:
                op["which"] = "PHI"
            if op["which"] == "PHI" and mut and not ctx["prte"]:      # no rate pending: the refusal, or the gamma that prepares one
                if g.rand() < 0.5:
                    op.update(op="refused", call="sub_step_phi", message=NO_PHI)
                    del op["which"]
                else:
                    op["which"] = "GAMMA"
            if op["op"] == "sub_step":
                ctx["budget"] += 0.25
                ctx["prte"] = {"GAMMA": True, "RHO": False}.get(op["which"], ctx["prte"])
        elif name == "sweep_commit":
            op["want_elbo"] = bool(g.rand() < 0.5)
            ctx["budget"] += 1
            ctx["prte"] = False
        elif name == "fit_loop":
            op["max_iter"] = 1 if ctx["long"] else int((1, 11, 21)[g.randint(3)])
            op["tol"], op["decision"] = ((1e-300, 1), (1e6, 0), (1e6, 1))[g.randint(3)]
            if op["max_iter"] == 1:
                ctx["budget"] += 1
            else:
                ctx["long"] = True
            ctx["prte"] = False
        elif name == "snapshot":
            ctx["snap"] = True
        elif name == "restore":
            ctx["restored"] = True
        elif name == "refused":
            if ctx["restored"]:
                calls = [c for c in SWEEPING if not (det and c == "sub_step")] + (["sub_step"] if det else []) + ["commit_nu"]
                op["call"], op["message"] = str(calls[g.randint(len(calls))]), READ_ONLY
            elif det and (ctx["snap"] or g.rand() < 0.7):
                op["call"], op["message"] = "sub_step", NO_SUB_STEP
            else:
                op["call"], op["message"] = "restore", NO_SNAPSHOT
        k = 2 if len(ops) < n_ops - 1 else len(MARKED_READERS)
        op["readers"] = [MARKED_READERS[i] for i in g.choice(len(MARKED_READERS), size=k, replace=False)]      # (the first one meets the handle as the call left it)
        ops.append(op)

    emit("set_state")
    forced = ["elbo", "refused", "elbo"] if g.rand() < 0.3 else []      # (a refusal before any snapshot exists, between two ELBOs)
    while len(ops) < n_ops:
        left = n_ops - len(ops)
        if not forced and block_at is not None and len(ops) >= block_at and not ctx["restored"]:
            forced = (([] if ctx["snap"] else ["snapshot"]) + (["restore", "refused"] if g.rand() < 0.3 and left >= 7 else [])
                      + ["restore", "refused", "set_state", "sweep"])
            block_at = None
        if forced:
            name = forced.pop(0)
            if name == "sweep":
                name = ("step", "sweep_commit", "fit_loop")[g.randint(3)]
                emit(name)
                if name == "step" and ops[-1]["n"] == 0:
                    ops[-1]["n"] = 1
                    ctx["budget"] += 1
                continue
            emit(name)
            continue
        w = allowed(ctx)
        if ctx["restored"] and left <= 1:
            w = {"refused": 1.0, "restore": 1.0}
        # a pending target that needs a refusal on a handle that is not restored: before the first snapshot (or on `det`)
        early = [t for t in targets if "refused" in t and (t[0] in SWEEPING or t[1] in SWEEPING)]
        if early and not det and not ctx["snap"]:
            w.pop("snapshot", None)
            if block_at is not None:
                block_at = max(block_at, min(len(ops) + 3, n_ops - 5))
        last = ops[-1]["op"]
        if last == "sub_step" and "sub_step" in w:      # sub-steps come in runs: a phi needs the gamma before it
            w["sub_step"] *= 4.0
        pick = None
        for t in list(targets):
            if t[0] == last and t[1] in w and g.rand() < 0.9:
                pick = t[1]
                targets.remove(t)
                break
        if pick is None:
            for t in targets:
                if t[0] in w:
                    w[t[0]] *= 12.0
            names = sorted(w)
            p = np.array([w[n] for n in names])
            pick = names[g.choice(len(names), p=p / p.sum())]
        emit(pick)
    return ops


def sequence_elements(ops):
    """(operation, next operation) pairs and (operation, reader) pairs of a sequence, for the coverage counts."""
    names = [o["op"] for o in ops]
    pairs = list(zip(names[:-1], names[1:]))
    reads = [(o["op"], r) for o in ops for r in SMALL_READERS + tuple(o["readers"])]
    return names, pairs, reads


def has_restore_block(ops):
    names = [o["op"] for o in ops]
    for i in range(len(names) - 3):
        if names[i:i + 3] == ["restore", "refused", "set_state"] and names[i + 3] in ("step", "sweep_commit", "fit_loop"):
            if names[i + 3] != "step" or ops[i + 3]["n"] > 0:
                return True
    return False


# ------------------------------------------------------------------------------------------------------------ the two oracles
class _Coo:
    """oracle/cavi_coo.c behind the four updates, the ELBO with a given nu factor, and reading / writing the posteriors."""

    def __init__(self, X, R, K, mut, pri, st):
        from oracle import cavi_coo
        sx = np.nonzero(X)
        self.c = cavi_coo.CooRef((sx, X[sx].astype(np.int32)), None if R is None else np.nonzero(R), X.shape, K, mut, pri, *st)

    def update(self, which):
        getattr(self.c, "update_" + which.lower())()

    def elbo(self, g_nu):
        self.c.s.g_nu_cache = g_nu
        return float(self.c.elbo())

    def get(self):
        c = self.c
        return {"gamma_shp": c.gamma_shp.copy(), "gamma_rte": c.gamma_rte.copy(), "phi_shp": c.phi_shp.copy(), "phi_rte": c.phi_rte.copy(),
                "nu_shp": float(c.s.nu_shp), "nu_rte": float(c.s.nu_rte), "rho": c.rho.copy()}

    def put(self, d):
        c = self.c
        for k in ("gamma_shp", "gamma_rte", "phi_shp", "phi_rte", "rho"):
            if k in d:
                getattr(c, k)[...] = d[k]
        if "nu_shp" in d:
            c.s.nu_shp, c.s.nu_rte = d["nu_shp"], d["nu_rte"]


class _Np:
    """oracle/vimure_oracle.py (dense NumPy) behind the same interface."""

    def __init__(self, X, R, K, mut, pri, st):
        from oracle import vimure_oracle as vo
        self.vo = vo
        L, N, _, M = X.shape
        p = vo.make_priors(L, M, K, alpha_theta=pri[0], beta_theta=pri[1], alpha_lambda=pri[2], beta_lambda=pri[3], eta_prior=(pri[4], pri[5]))
        self.pb = vo.Problem(X, np.ones_like(X) if R is None else R, K, mut, p)
        pr = np.array(st[6], dtype=np.float64)
        self.st = vo.State(np.array(st[0], float), np.array(st[1], float), np.array(st[2], float), np.array(st[3], float), float(st[4]),
                           float(st[5]), pr.copy(), pr, np.log(pr + self.pb.eps), 0.0)

    def update(self, which):
        getattr(self.vo, "update_" + which.lower())(self.pb, self.st)

    def elbo(self, g_nu):
        self.st.G_nu_cache = g_nu
        return float(self.vo.elbo(self.pb, self.st))

    def get(self):
        s = self.st
        return {"gamma_shp": s.gamma_shp.copy(), "gamma_rte": s.gamma_rte.copy(), "phi_shp": s.phi_shp.copy(), "phi_rte": s.phi_rte.copy(),
                "nu_shp": float(s.nu_shp), "nu_rte": float(s.nu_rte), "rho": s.rho.copy()}

    def put(self, d):
        for k, v in d.items():
            setattr(self.st, k, v.copy() if isinstance(v, np.ndarray) else v)


BACKENDS = {"coo": _Coo, "numpy": _Np}
FORGETFUL = ("stale_rho_after_plain_step", "gamma_after_rho_old_mask_sums", "elbo_current_nu", "first_sweep_old_statistics")


def _gamma_term(pa, pb, qa, qb):
    return gammaln(qa) - pa * np.log(qb) + (pa - qa) * psi(qa) + qa * (1.0 - pb / qb)


class SeqModel:
    """One engine handle on the host.  `apply(op)` mirrors one call and returns what the call returns (an ELBO, `fit_loop`'s tuple
    without the run times, or None); `observe()` gives every observable.  forget: one of FORGETFUL -- a model with that bookkeeping
    mistake built in, for the sensitivity test."""

    def __init__(self, X, R, K, mutuality=True, backend="coo", forget=None):
        assert forget is None or forget in FORGETFUL
        self.X, self.R, self.K, self.mut = X, R, int(K), bool(mutuality)
        self.backend, self.forget = BACKENDS[backend], forget
        self.pri = PRI
        self.b = None
        self.snap = None
        self.restored = False
        self.n_set = 0

    # -- the rules
    def _g(self):
        s = self.b.get()
        return float(np.exp(psi(s["nu_shp"]) - np.log(s["nu_rte"]))) if self.mut else 0.0

    def _update(self, which):
        self.prte = {"GAMMA": True, "RHO": False}.get(which, self.prte)
        if which == "NU":
            if not self.mut:
                return
            self.g_stale = self._g()      # the ELBO's factor: the one from before this update
        self.b.update(which)

    def _sweep(self):
        if self.old_rho is not None:      # (forgetful variant 4: gamma and phi from the last realisation's rho)
            rho = self.b.get()["rho"]
            self.b.put({"rho": self.old_rho})
            self._update("GAMMA")
            self._update("PHI")
            self.b.put({"rho": rho})
            self.old_rho = None
        else:
            self._update("GAMMA")
            self._update("PHI")
        self._update("RHO")
        self._update("NU")

    def _elbo(self):
        e = self.b.elbo(self._g() if self.forget == "elbo_current_nu" else self.g_stale)
        assert not np.isnan(e), "ELBO is NaN"
        return e

    # -- the calls
    def apply(self, op):
        name = op["op"]
        prev, self.last = getattr(self, "last", None), name
        if name == "set_state":
            if op.get("priors") is not None:
                self.pri = tuple(op["priors"])
            st = draw_state(np.random.RandomState(op["state_seed"]), self.X, self.K, self.mut)
            self.old_rho = self.b.get()["rho"] if (self.forget == "first_sweep_old_statistics" and self.b is not None) else None
            self.b = self.backend(self.X, self.R, self.K, self.mut, self.pri, st)
            self.state = st
            self.g_stale = self._g()
            self.restored, self.hidden_rho, self.rho_before, self.prte = False, None, None, False
            self.n_set += 1
            return None
        if name == "refused":
            return None
        if name == "snapshot":
            self.snap = (self.b.get(), self.g_stale, self.hidden_rho)
            return None
        if name == "restore":
            d, self.g_stale, self.hidden_rho = self.snap
            self.b.put(d)
            self.restored = True
            return None
        assert not self.restored, "a sweeping call on a restored handle"
        self.hidden_rho = None
        if name == "step":
            before = self.b.get()["rho"] if self.forget == "stale_rho_after_plain_step" else None
            for _ in range(op["n"]):
                self._sweep()
            if before is not None and op["n"] > 0 and not op["want_elbo"]:
                self.hidden_rho = before
            return self._elbo() if op["want_elbo"] else None
        if name == "sub_step":
            w = op["which"]
            if w == "RHO":
                self.rho_before = self.b.get()["rho"]
            if w == "GAMMA" and prev == "sub_step" and self.forget == "gamma_after_rho_old_mask_sums" and self.rho_before is not None:
                new = self.b.get()["rho"]
                self._update("GAMMA")
                shp = self.b.get()["gamma_shp"]
                self.b.put({"rho": self.rho_before})
                self._update("GAMMA")
                self.b.put({"rho": new, "gamma_shp": shp})
            elif w == "PHI":
                assert self.prte or not self.mut, "STEP_PHI without a pending rate"
                if self.mut:
                    self._update(w)
            else:
                self._update(w)
                if w == "GAMMA" and not self.mut:      # (the finalize of gamma commits phi as well)
                    self._update("PHI")
            if w != "RHO":
                self.rho_before = None
            return None
        self.rho_before = None
        if name == "elbo":
            return self._elbo()
        if name == "sweep_commit":      # vimure_amd/sharded.py: the total of one owner is its own partial
            self._sweep()
            return self._elbo() if op["want_elbo"] else None
        if name == "fit_loop":
            from tests.test_hip_lockstep import _oracle_loop
            model = self

            class _Loop:
                cavi_step = staticmethod(model._sweep)
                elbo = staticmethod(model._elbo)
            rows, elbo, its, reached = _oracle_loop(_Loop, op["max_iter"], op["tol"], op["decision"])
            return ([r[0] for r in rows], [r[1] for r in rows], elbo, its, bool(reached))
        raise ValueError(name)

    def observe(self):
        s = self.b.get()
        if self.hidden_rho is not None:
            s["rho"] = self.hidden_rho
        s["G_theta"] = np.exp(psi(s["gamma_shp"]) - np.log(s["gamma_rte"]))
        s["G_lambda"] = np.exp(psi(s["phi_shp"]) - np.log(s["phi_rte"]))
        s["g_nu"], s["g_nu_stale"] = self._g(), self.g_stale
        return s


def sharded_elbo(parts, nu_shp, nu_rte, a_eta, b_eta):
    """The ELBO of a layer-sharded sweep from its three sums, as vimure_amd/sharded.py assembles it."""
    return float(parts[1] - (nu_shp / nu_rte) * parts[2] + _gamma_term(a_eta, b_eta, nu_shp, nu_rte))


# --------------------------------------------------------------------------------------------------------------- tolerances
RTOL = {"rho": 1e-7}      # everything else 1e-9; atol 1e-12 throughout; the ELBO 1e-9 max(1, |ELBO|)


def ratio(got, want, name):
    """Largest deviation of an observable in units of its tolerance."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if name == "elbo":
        return float(np.max(np.abs(got - want) / (1e-9 * np.maximum(1.0, np.abs(want))))) if got.size else 0.0
    return float(np.max(np.abs(got - want) / (1e-12 + RTOL.get(name, 1e-9) * np.abs(want))))


def result_ratios(got, want, opname):
    """{observable: ratio} of a call's return value (an ELBO or fit_loop's tuple); the integer parts must be equal."""
    if want is None:
        assert got is None, (opname, got)
        return {}
    if opname == "fit_loop":
        assert got[0] == want[0] and got[3] == want[3] and got[4] == want[4], (opname, got, want)
        return {"elbo": max(ratio(got[1], want[1], "elbo"), ratio(got[2], want[2], "elbo"))}
    return {"elbo": ratio(got, want, "elbo")}


def state_ratios(got, want, with_rho=True):
    return {n: ratio(got[n], want[n], n) for n in PARAMS + GEO + (("rho",) if with_rho else ())}


# ------------------------------------------------------------------------------------------------------- the device's side
def make_engine(kind, X, R, K=None):
    """The handle of a kind (its switches must be in the environment already), asserted to be of the family it is meant to reach."""
    from vimure_amd import CaviEngine
    spec = spec_of(kind)
    K = spec["K"] if K is None else K
    mut = spec.get("mut", True)
    if spec.get("coo"):
        sx = np.nonzero(X)
        eng = CaviEngine.from_coo(sx, X[sx], X.shape, R=None if R is None else np.nonzero(R), K=K, mutuality=mut)
    else:
        eng = CaviEngine(X, R, K=K, mutuality=mut)
    fmt, mask, (passes, levels, far) = eng.data_format()[0], eng.mask_format()[0], eng.sweep_shape()
    assert fmt == spec["fmt"], (kind, fmt)
    assert spec["mask"] is None or mask == spec["mask"], (kind, mask)
    assert spec["passes"] is None or passes == spec["passes"], (kind, passes, levels, far)
    assert far == 0, (kind, far)
    eng.set_priors(*PRI)
    return eng


def engine_apply(eng, op, model):
    """One operation on the device -> what it returns, in the form of SeqModel.apply.  A refused call must raise with its message."""
    from vimure_amd import _lib
    from vimure_amd.engine import EngineError
    name = op["op"]
    if name == "set_state":
        if op.get("priors") is not None:
            eng.set_priors(*op["priors"])
        eng.set_state(*model.state)      # (the model has drawn it)
        return None
    if name == "step":
        return eng.step(op["n"], want_elbo=op["want_elbo"])
    if name == "sub_step":
        return eng.sub_step(getattr(_lib, "STEP_" + op["which"]))
    if name == "elbo":
        return eng.elbo()
    if name == "sweep_commit":
        parts = eng.sweep_local(want_elbo=op["want_elbo"])
        eng.commit_nu(parts[0])
        if not op["want_elbo"]:
            return None
        nu_shp = model.pri[4] + parts[0] if model.mut else model.state[4]
        return sharded_elbo(parts, nu_shp, model.state[5], model.pri[4], model.pri[5])
    if name == "fit_loop":
        rows, elbo, its, conv = eng.fit_loop(op["max_iter"], op["tol"], op["decision"])
        return ([r[0] for r in rows], [r[1] for r in rows], elbo, its, conv)
    if name == "snapshot":
        return eng.snapshot()
    if name == "restore":
        return eng.restore()
    assert name == "refused"
    call = {"step": lambda: eng.step(1), "sub_step": lambda: eng.sub_step(_lib.STEP_GAMMA), "elbo": eng.elbo,
            "sweep_commit": lambda: eng.sweep_local(False), "fit_loop": lambda: eng.fit_loop(3, 0.1, 1), "restore": eng.restore,
            "sub_step_phi": lambda: eng.sub_step(_lib.STEP_PHI), "commit_nu": lambda: eng.commit_nu(1.0)}[op["call"]]
    try:
        call()
    except EngineError as e:
        assert op["message"] in str(e), (op, str(e))
        return None
    raise AssertionError(f"{op['call']} was not refused")


def engine_small_state(eng):
    s = eng.get_state(rho=False)
    s["G_theta"], s["G_lambda"], s["g_nu"], s["g_nu_stale"] = eng.get_geometric()
    return s


def check_readers(eng, readers, want, X, R, seed, tally):
    """The marked readers against the model's observables `want`.  Returns {observable: ratio}; integer outputs are asserted here.
    tally: [elements decided within 1e-9 of a tie and compared on the device's own rho, read-out elements]."""
    from tests import draws_ref, edge_table_util, netstats_util
    out = {}
    K = want["rho"].shape[-1]
    own = None

    def own_rho():      # (whatever a reader is compared with is itself held to the model)
        nonlocal own
        if own is None:
            own = eng.get_state(rho=True)["rho"]
        out["rho"] = max(out.get("rho", 0.0), ratio(own, want["rho"], "rho"))
        return own
    for r in readers:
        if r == "get_state_rho":
            s = eng.get_state(rho=True)
            own = s["rho"]
            out["rho"] = max(out.get("rho", 0.0), ratio(s["rho"], want["rho"], "rho"))
            for n in PARAMS:
                out[n] = max(out.get(n, 0.0), ratio(s[n], want[n], n))
        elif r == "readout":
            rho = want["rho"]
            top = np.sort(rho, axis=-1)
            clear = top[..., -1] - top[..., -2] > 1e-9
            y = eng.readout("rho_max")
            wrong = clear & (y != np.argmax(rho, axis=-1))
            assert not wrong.any(), (f"readout rho_max: {int(wrong.sum())} ties differ from the model's arg-max; the device's own rho is "
                                     f"{np.abs(own_rho() - rho)[wrong].max():.3e} from the model's there, {ratio(own_rho(), rho, 'rho'):.3g} tolerances overall")
            thr = 0.5 if K == 2 else 0.3
            t = eng.readout("threshold", thr)
            far = np.abs(rho[..., 1] - thr) > 1e-9
            assert np.array_equal(t[far], (rho[..., 1] >= thr).astype(np.uint8)[far]), "readout threshold"
            n_close = int((~clear).sum() + (~far).sum())
            if n_close:
                assert np.array_equal(y[~clear], np.argmax(own_rho(), axis=-1)[~clear]), "readout rho_max at a tie"
                assert np.array_equal(t[~far], (own_rho()[..., 1] >= thr).astype(np.uint8)[~far]), "readout threshold at a tie"
            tally[0] += n_close
            tally[1] += 2 * y.size
            out["rho_mean"] = ratio(eng.readout("rho_mean"), (rho * np.arange(K)).sum(-1), "rho")
        elif r == "sample":
            y = eng.sample(seed)
            assert np.array_equal(y, draws_ref.sample_ref(own_rho(), seed, 1)), "sample: not drawn from the current rho"
        elif r == "expected_stats":
            got, ref = eng.expected_stats(), netstats_util.expected_np(own_rho())
            N = X.shape[1]
            terms = {"edges": N * N * K, "weight": N * N * K, "mutual": N * N, "edges_var": N * N}
            for k in ref:      # (the bound of tests/test_hip_netstats.py, against the rho read in the same state)
                np.testing.assert_allclose(got[k], ref[k], rtol=2 * terms[k] * 2.0 ** -53, atol=0, err_msg="expected_stats " + k)
        elif r == "edge_table_size":
            n = eng.edge_table_size("rho_max", 0.0, ("reported", "inferred"))
            ref = edge_table_util.edge_table_np(X, R, own_rho(), "rho_max", 0.0, 3)
            assert n == len(ref["l"]), ("edge_table_size", n, len(ref["l"]))
        else:
            raise ValueError(r)
    return out


def run_sequence(kind, ops, X, R, K=None, label="", record=None, worst=None):
    """The sequence on a device handle of the kind, every operation against the model.  Raises AssertionError naming the kind, the
    index and name of the first diverging operation and the observable.  record: a list that receives, per operation, the return
    value and the device's small state (the deterministic kind compares two runs of it bit for bit).  worst: a dict that receives the
    largest ratio to tolerance per observable."""
    spec = spec_of(kind)
    K = spec["K"] if K is None else K
    model = SeqModel(X, R, K, spec.get("mut", True), "coo")
    eng = make_engine(kind, X, R, K)
    tally = [0, 0]
    try:
        for i, op in enumerate(ops):
            where = f"{label or kind}: operation {i} ({op['op']} {({k: v for k, v in op.items() if k not in ('op', 'readers')})})"
            before = engine_small_state(eng) if op["op"] == "refused" else None
            want_ret = model.apply(op)
            try:
                got_ret = engine_apply(eng, op, model)
                ratios = result_ratios(got_ret, want_ret, op["op"])
            except AssertionError as e:
                raise AssertionError(f"{where}: return value: {e}") from None
            want = model.observe()
            got = engine_small_state(eng)
            if before is not None:
                for n in PARAMS + GEO:
                    assert np.array_equal(np.asarray(before[n]), np.asarray(got[n])), f"{where}: the refused call changed {n}"
            ratios.update(state_ratios(got, want, with_rho=False))
            bad = {n: v for n, v in ratios.items() if not v <= 1.0}
            assert not bad, f"{where}: observables beyond their tolerance (in units of it): {bad}"
            try:
                for n, v in check_readers(eng, op["readers"], want, X, R, 1000 + i, tally).items():
                    ratios[n] = max(ratios.get(n, 0.0), v)
            except AssertionError as e:
                raise AssertionError(f"{where}: reader: {e}") from None
            bad = {n: v for n, v in ratios.items() if not v <= 1.0}
            assert not bad, f"{where}: observables beyond their tolerance (in units of it): {bad}"
            if worst is not None:
                for n, v in ratios.items():
                    worst[n] = max(worst.get(n, 0.0), v)
            if record is not None:
                record.append((got_ret, {n: np.array(got[n]) for n in PARAMS + GEO}))
        assert tally[0] <= 0.01 * max(1, tally[1]), f"{label or kind}: {tally[0]} of {tally[1]} read-out elements decided at a tie"
        if record is not None:
            record.append((None, {"rho": eng.get_state(rho=True)["rho"]}))
    finally:
        eng.close()
