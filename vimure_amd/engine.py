"""Object wrapper over the C-ABI: one `CaviEngine` = one dataset on one MI355X.

The engine owns the device copies of X (uint8) and R (bit mask) and the variational
state; the host (`vimure_amd.model.VimureModel`) only draws the RandomState-seeded
initial values and applies the ELBO stop rule.
"""
import ctypes as C

import numpy as np

from . import _lib


class EngineError(RuntimeError):
    pass


class EdgeTableArgumentError(EngineError, ValueError):
    """An argument `edge_table` / `edge_table_size` refuse (VMR_EINVAL): a method that gives no categories, an empty or
    unknown selection, outputs shorter than the table."""


class ScoreArgumentError(EngineError, ValueError):
    """An argument `score_truth` refuses (VMR_EINVAL): an unknown score, thresholds that are not finite, that decrease or that
    are too many, a ground truth of another shape, no output asked for."""


class ReporterTableArgumentError(EngineError, ValueError):
    """An argument `reporter_table` refuses (VMR_EINVAL): a method that gives no categories, a layer out of range, no output
    asked for."""


class HeldoutArgumentError(EngineError, ValueError):
    """An argument `heldout_loglik` refuses (VMR_EINVAL): an empty list, a subscript out of range, a negative count, a list that
    decreases in the layer, a negative or non-finite table entry."""


class ReportScoresArgumentError(EngineError, ValueError):
    """An argument `report_scores` / `report_scores_size` refuse (VMR_EINVAL): a selection other than reports, omissions or both,
    a NaN or -inf threshold, edges that are not finite, that decrease or that are too many, a negative or non-finite table
    entry, a layer out of range, a table shorter than the flagged rows."""


class ReporterInfluenceArgumentError(EngineError, ValueError):
    """An argument `reporter_influence` / `reporter_influence_size` refuse (VMR_EINVAL): a method that gives no categories, a
    selection other than lost, gained, both or none, a NaN or negative min_tv, edges that are not finite, that decrease or that
    are too many, a table entry out of range, a layer out of range, a table shorter than the flagged rows."""


class TriadArgumentError(EngineError, ValueError):
    """An argument `sample_triads` / `expected_triads` refuse (VMR_EINVAL): n_samples or n_trials below 1, temporaries that do
    not fit in the free device memory."""


class MixingArgumentError(EngineError, ValueError):
    """An argument `sample_mixing` / `expected_mixing` refuse (VMR_EINVAL): C outside [1, 64] with groups given, a label outside
    [-1, C), more than 32 layers with the overlap asked for, n_samples or n_trials below 1, nothing asked for, temporaries that do
    not fit in the free device memory."""


class ConnectivityArgumentError(EngineError, ValueError):
    """An argument `sample_connectivity` refuses (VMR_EINVAL): n_samples or n_trials below 1, more nodes than the closure's
    working set holds (`_lib.CONN_NMAX`), temporaries that do not fit in the free device memory."""


class CentralityArgumentError(EngineError, ValueError):
    """An argument `sample_centrality` / `mean_centrality` refuse (VMR_EINVAL): a direction other than out, in or union, T outside
    [1, `_lib.CENT_TMAX`], top_k outside [1, N], a q that is not finite or outside [0, 1], n_samples or n_trials below 1, more
    nodes than the walk's working set holds (`_lib.CENT_NMAX`, sampled call only), temporaries that do not fit in the free device
    memory."""


class BetweennessArgumentError(EngineError, ValueError):
    """An argument `sample_betweenness` / `network_betweenness` refuse (VMR_EINVAL): a direction other than directed or union,
    top_k outside [1, N], n_samples or n_trials below 1, networks of another shape than the handle's, more nodes than a source's
    working set holds (`_lib.BTW_NMAX`), temporaries that do not fit in the free device memory."""


class CoresArgumentError(EngineError, ValueError):
    """An argument `sample_cores` / `network_cores` refuse (VMR_EINVAL): a mode other than union, total, in or out, k_min outside
    [0, 2 (N - 1)], top_k outside [1, N], n_samples or n_trials below 1, networks of another shape than the handle's, more nodes
    than the peel's working set holds (`_lib.CORE_NMAX`), temporaries that do not fit in the free device memory."""


class CutpointArgumentError(EngineError, ValueError):
    """An argument `sample_cutpoints` / `network_cutpoints` refuse (VMR_EINVAL): a mode other than union or mutual, top_k outside
    [1, N], n_samples or n_trials below 1, networks of another shape than the handle's, more nodes than the removal experiments'
    working set holds (`_lib.CUT_NMAX`), temporaries that do not fit in the free device memory."""


class CascadeArgumentError(EngineError, ValueError):
    """An argument `sample_outreach` / `sample_seed_outreach` / `network_outreach` / `network_seed_outreach` refuse (VMR_EINVAL): a
    direction other than out, in or union, T outside [1, `_lib.CASC_TMAX`], n_cascades outside [1, `_lib.CASC_KMAX`], top_k
    outside [1, N], a q that is not finite or outside [0, 1], seed sets that are more than `_lib.CASC_SETS`, that name a node out
    of range or that do not match n_sets, n_samples or n_trials below 1, networks of another shape than the handle's, more nodes
    than the closure's working set holds (`_lib.CASC_NMAX`), temporaries that do not fit in the free device memory."""


class CensusArgumentError(EngineError, ValueError):
    """An argument `sample_triad_census` / `network_triad_census` refuse (VMR_EINVAL): n_samples or n_trials below 1, networks of
    another shape than the handle's, temporaries that do not fit in the free device memory."""


class PartnersArgumentError(EngineError, ValueError):
    """An argument `sample_shared_partners` / `network_shared_partners` refuse (VMR_EINVAL): n_samples or n_trials below 1, an
    unknown mode, n_bins outside [2, `_lib.SP_MAX_BINS`], a pair whose layer or node is out of range or that names one node twice,
    networks of another shape than the handle's, temporaries that do not fit in the free device memory."""


class StructuralHolesArgumentError(EngineError, ValueError):
    """An argument `sample_structural_holes` / `network_structural_holes` refuse (VMR_EINVAL): n_samples or n_trials below 1, a
    mode other than union or weighted, top_k outside [1, N], networks of another shape than the handle's, temporaries that do not
    fit in the free device memory."""


SCORE_OUTPUTS = ("hist", "conf", "sums", "auc", "auc_pairs")
INF_SELECT = {"none": 0, "lost": _lib.INF_LOST, "gained": _lib.INF_GAINED, "both": _lib.INF_LOST | _lib.INF_GAINED}
# columns of the table of `CaviEngine.reporter_influence`, in the order of vmr_reporter_influence's row pointers
INF_COLUMNS = (("l", np.int32), ("i", np.int32), ("j", np.int32), ("m", np.int32), ("x", np.int32), ("xt", np.int32),
               ("prob", np.float64), ("prob_loo", np.float64), ("tv", np.float64))
RS_SELECT = {"reports": _lib.RS_REPORTS, "omissions": _lib.RS_OMISSIONS, "both": _lib.RS_REPORTS | _lib.RS_OMISSIONS}
# columns of the table of `CaviEngine.report_scores`, in the order of vmr_report_scores' row pointers
RS_COLUMNS = (("l", np.int32), ("i", np.int32), ("j", np.int32), ("m", np.int32), ("x", np.int32), ("xt", np.int32),
              ("logp", np.float64), ("mean", np.float64))

# columns of `CaviEngine.edge_table`, in the order of vmr_edge_table's output pointers (device=True: the unsigned 32 / 64-bit columns
# are torch.int32 / torch.int64 tensors holding the same bits -- every value is below 2^31 / 2^63)
EDGE_COLUMNS = (("l", np.int32), ("i", np.int32), ("j", np.int32), ("y", np.uint8), ("prob", np.float64), ("mean", np.float64),
                ("n_rep", np.uint32), ("total", np.uint64), ("n_mask", np.uint32), ("ego", np.uint32), ("alter", np.uint32),
                ("y_T", np.uint8), ("n_rep_T", np.uint32), ("total_T", np.uint64))
_TORCH_NAME = {"uint32": "int32", "uint64": "int64"}
_CORE_STATS = ("degeneracy", "main_core_size", "core_sum", "kcore_size")   # the columns of the k-core calls' summary


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def host_buffer(n_doubles, pinned=True):
    """float64 staging buffer for rho-sized transfers: page-locked (through torch) when that is available and worth it."""
    if pinned and n_doubles * 8 >= (8 << 20):
        try:
            import torch
            if torch.cuda.is_available():
                t = torch.empty(int(n_doubles), dtype=torch.float64, pin_memory=True)
                a = t.numpy()
                return a, t   # (the tensor owns the memory: keep it alive with the array)
        except Exception:
            pass
    return np.empty(int(n_doubles), np.float64), None


class CaviEngine:
    def __init__(self, X, R=None, K=2, mutuality=True, eps=1e-12, device=None):
        self._h = C.c_void_p()
        self._staging = []   # pinned float64 buffers reused across realisations / fits on this engine
        self.lib = _lib.load()
        on_dev = _is_torch(X)
        if on_dev:
            if not X.is_cuda or X.dtype.__str__() != "torch.uint8" or not X.is_contiguous():
                raise ValueError("device X must be a contiguous torch.uint8 tensor on the GPU")
            if R is not None and (not _is_torch(R) or not R.is_cuda or R.dtype.__str__() != "torch.uint8"
                                  or not R.is_contiguous() or tuple(R.shape) != tuple(X.shape)):
                raise ValueError("device R must be a contiguous torch.uint8 GPU tensor shaped like X")
            if device is None:
                device = X.device.index or 0
            import torch
            torch.cuda.synchronize(X.device)
            xp, rp = X.data_ptr(), (R.data_ptr() if R is not None else None)
            shape = tuple(X.shape)
        else:
            if getattr(X, "dtype", np.uint8) != np.uint8 and np.size(X) and (np.min(X) < 0 or np.max(X) > 255):
                raise ValueError("dense X is a uint8 tensor (counts in [0, 255]); larger counts go through CaviEngine.from_coo")
            X = np.ascontiguousarray(X, dtype=np.uint8)
            if R is not None:
                R = np.ascontiguousarray(R, dtype=np.uint8)
                if R.shape != X.shape:
                    raise ValueError("Dimensions of reporter mask (R) do not match L x N x N x M")
            xp, rp = X.ctypes.data, (R.ctypes.data if R is not None else None)
            shape = X.shape
            if device is None:
                device = 0
        if len(shape) != 4 or shape[1] != shape[2]:
            raise ValueError("X must have shape (L, N, N, M)")
        self.L, self.N, _, self.M = (int(s) for s in shape)
        self.K, self.mutuality, self.device = int(K), bool(mutuality), int(device)
        rc = self.lib.vmr_create(C.byref(self._h), self.device, self.L, self.N, self.M, self.K, int(self.mutuality),
                                 xp, rp, int(on_dev), float(eps))
        if rc != 0:
            msg = self.lib.vmr_last_error(None).decode()
            self._h = C.c_void_p()
            raise (ValueError if rc == _lib.VMR_EINVAL else EngineError)(msg)
        self._keep = (X, R)

    @classmethod
    def from_coo(cls, subs, vals, shape, R=None, K=2, mutuality=True, eps=1e-12, device=None):
        """Dataset from coordinate lists -- the reference's own containers (`X.subs`, `X.vals`, `R.subs`; reference
        model.py:136-171) -- without a dense [L,N,N,M] tensor on the host or the device (vmr_create_coo).
        subs: 4 index arrays (l, i, j, m); vals: counts in [1, 2^31); R: None (every reporter may report on every tie) or 4
        index arrays of the mask's non-zeros; NumPy arrays or torch GPU tensors (int32 / int64).
        Limits (ValueError naming the one exceeded): M <= 65535 (tensor.M_COO_MAX: 16-bit reporters in the mask lists),
        L N^2 2^ceil(log2 M) < 2^64 (the sort keys), (largest count + 1) * M < 2^32; M > 8192 runs the general kernels."""
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        self._staging = []
        self.lib = _lib.load()
        on_dev = _is_torch(vals)
        L, N, N2, M = (int(s) for s in shape)
        if N != N2:
            raise ValueError("X must have shape (L, N, N, M)")

        def cols(arrs):
            if on_dev:
                import torch
                out = [a.to(torch.int32).contiguous() for a in arrs]
                return out, [a.data_ptr() for a in out]
            out = [np.ascontiguousarray(a, dtype=np.int32) for a in arrs]
            return out, [a.ctypes.data for a in out]
        if len(subs) != 4:
            raise ValueError("subs must be the 4 index arrays (l, i, j, m)")
        xk, xp = cols(list(subs) + [vals])
        nx = int(xk[0].shape[0])
        if any(int(a.shape[0]) != nx for a in xk):
            raise ValueError("Subscripts and values must be of equal length")
        if R is None:
            rk, rp, nr = [], [None] * 4, -1
        else:
            if len(R) != 4:
                raise ValueError("R must be the 4 index arrays (l, i, j, m) of the mask's non-zeros")
            rk, rp = cols(list(R))
            nr = int(rk[0].shape[0])
        if device is None:
            device = (vals.device.index or 0) if on_dev else 0
        if on_dev:
            import torch
            torch.cuda.synchronize(vals.device)
        self.L, self.N, self.M = L, N, M
        self.K, self.mutuality, self.device = int(K), bool(mutuality), int(device)
        rc = self.lib.vmr_create_coo(C.byref(self._h), self.device, L, N, M, self.K, int(self.mutuality), nx, *xp, nr, *rp,
                                     int(on_dev), float(eps))
        if rc != 0:
            msg = self.lib.vmr_last_error(None).decode()
            self._h = C.c_void_p()
            raise (ValueError if rc == _lib.VMR_EINVAL else EngineError)(msg)
        self._keep = (xk, rk)
        return self

    # -- helpers
    def _check(self, rc, einval=None):
        """einval: the exception a refused argument (VMR_EINVAL) raises in place of ValueError."""
        if rc == 0:
            return
        msg = self.lib.vmr_last_error(self._h).decode()
        if rc == _lib.VMR_EINVAL and einval is not None:
            raise einval(msg)
        if rc in (_lib.VMR_EINVAL, _lib.VMR_ENAN):
            raise ValueError(msg)
        raise EngineError(msg)

    def staging(self, i):
        """The i-th rho-sized host staging buffer of this engine (allocated on first use, pinned when possible)."""
        while len(self._staging) <= i:
            self._staging.append(host_buffer(self.L * self.N * self.N * self.K))
        return self._staging[i][0].reshape(self.L, self.N, self.N, self.K)

    def can_upload_ahead(self):
        """Page-locked staging buffers (through torch) exist for this engine's rho size, i.e. `upload_ahead` works."""
        if not hasattr(self, "_can_ahead"):
            self.staging(0)
            self._can_ahead = self._staging[0][1] is not None
        return self._can_ahead

    def upload_ahead(self, i, slot):
        """Copy staging buffer i to a device buffer of this engine (two in rotation: `slot` 0 / 1) on a stream of its own and
        wait for the copy; returns the device tensor (what `set_state` then takes with a device-to-device copy), or None
        when the staging buffer is not page-locked / torch is not there.  For the thread that draws the next realisation
        while the GPU sweeps the current one: the 5 ms upload of a 256 MB pr_rho leaves the critical path."""
        arr, ten = self._staging[i]
        if ten is None:
            return None
        import torch
        if not hasattr(self, "_ahead"):
            self._ahead = [None, None]
        if not hasattr(self, "_ahead_stream"):   # (draw_pr_rho may have made the slots without it)
            self._ahead_stream = torch.cuda.Stream(device=self.device)
        if self._ahead[slot] is None:
            self._ahead[slot] = torch.empty((self.L, self.N, self.N, self.K), dtype=torch.float64, device=f"cuda:{self.device}")
        with torch.cuda.stream(self._ahead_stream):
            self._ahead[slot].view(-1).copy_(ten, non_blocking=True)
        self._ahead_stream.synchronize()
        return self._ahead[slot]

    def draw_pr_rho(self, blocks, bias0, undirected, out=None):
        """The initial rho prior drawn on the device (vmr_draw_pr_rho) from the block descriptors (cuts, keys, pos) of
        `_hostlib.mt_block_states`, bit for bit the host draw, one-hot where this engine's coverage is 0.  out: a float64 CUDA
        tensor [L,N,N,K], a C-contiguous float64 NumPy array (filled through one copy: for tests), or None: the engine's device
        slot 0 of `upload_ahead`.  No host staging buffer is involved.  Returns out; the engine's stream has finished the draw,
        so `set_state` takes a device tensor as it is."""
        cuts, keys, pos = blocks
        cuts = np.ascontiguousarray(cuts, dtype=np.int64)
        keys = np.ascontiguousarray(keys, dtype=np.uint32)
        pos = np.ascontiguousarray(pos, dtype=np.int32)
        nblk = int(pos.shape[0])
        if cuts.shape != (nblk + 1,) or keys.shape != (nblk, 624):
            raise ValueError("blocks: cuts[nblk + 1], keys[nblk, 624] and pos[nblk] expected")
        shape = (self.L, self.N, self.N, self.K)
        if out is None:
            import torch
            if not hasattr(self, "_ahead"):
                self._ahead = [None, None]
            if self._ahead[0] is None:
                self._ahead[0] = torch.empty(shape, dtype=torch.float64, device=f"cuda:{self.device}")
            out = self._ahead[0]
        if _is_torch(out):
            import torch
            assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float64 and tuple(out.shape) == shape
            ptr, dev = out.data_ptr(), 1
        else:
            assert out.dtype == np.float64 and out.flags.c_contiguous and out.shape == shape
            ptr, dev = out.ctypes.data, 0
        self._check(self.lib.vmr_draw_pr_rho(self._h, nblk, cuts.ctypes.data, keys.ctypes.data, pos.ctypes.data, float(bias0),
                                             int(bool(undirected)), ptr, dev))
        return out

    def close(self):
        self._ahead = [None, None]
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.vmr_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- data
    def data_stats(self, coverage=True):
        s = C.c_double()
        cov = np.empty((self.L, self.N, self.N), np.uint8) if coverage else None
        self._check(self.lib.vmr_data_stats(self._h, C.byref(s), cov.ctypes.data if coverage else None))
        return s.value, cov

    # -- parameters
    def set_priors(self, alpha_theta, beta_theta, alpha_lambda, beta_lambda, alpha_eta, beta_eta):
        at = _f64(np.broadcast_to(alpha_theta, (self.L, self.M)))
        bt = _f64(np.broadcast_to(beta_theta, (self.L, self.M)))
        al = _f64(np.broadcast_to(alpha_lambda, (self.L, self.K)))
        bl = _f64(np.broadcast_to(beta_lambda, (self.L, self.K)))
        self._check(self.lib.vmr_set_priors(self._h, at.ctypes.data, bt.ctypes.data, al.ctypes.data, bl.ctypes.data,
                                            float(alpha_eta), float(beta_eta)))

    def set_state(self, gamma_shp, gamma_rte, phi_shp, phi_rte, nu_shp, nu_rte, pr_rho):
        gs, gr, ps, pr = _f64(gamma_shp), _f64(gamma_rte), _f64(phi_shp), _f64(phi_rte)
        assert gs.shape == (self.L, self.M) and gr.shape == gs.shape
        assert ps.shape == (self.L, self.K) and pr.shape == ps.shape
        if _is_torch(pr_rho):
            assert pr_rho.is_cuda and pr_rho.is_contiguous() and tuple(pr_rho.shape) == (self.L, self.N, self.N, self.K)
            import torch
            assert pr_rho.dtype == torch.float64
            if not any(pr_rho is t for t in getattr(self, "_ahead", [])):   # (upload_ahead has waited for its copy already)
                torch.cuda.synchronize(pr_rho.device)
            pp, dev = pr_rho.data_ptr(), 1
        else:
            pr_rho = _f64(pr_rho)
            assert pr_rho.shape == (self.L, self.N, self.N, self.K)
            pp, dev = pr_rho.ctypes.data, 0
        self._check(self.lib.vmr_set_state(self._h, gs.ctypes.data, gr.ctypes.data, ps.ctypes.data, pr.ctypes.data,
                                           float(nu_shp), float(nu_rte), pp, dev))

    # -- CAVI
    def step(self, n_iters=1, want_elbo=False):
        if want_elbo:
            e = C.c_double()
            self._check(self.lib.vmr_step(self._h, int(n_iters), C.byref(e)))
            return e.value
        self._check(self.lib.vmr_step(self._h, int(n_iters), None))
        return None

    def fit_loop(self, max_iter, tol, decision):
        """The realisation's convergence loop on the engine's side (reference model.py:405-426, 1021-1056).
        Returns (trace rows [(iter, elbo, runtime, reached)], last ELBO, iterations, converged)."""
        cap = max_iter // 10 + 2
        n, its, conv, e = C.c_int(), C.c_int(), C.c_int(), C.c_double()
        ri, rr = np.empty(cap, np.int32), np.empty(cap, np.int32)
        re, rt = np.empty(cap), np.empty(cap)
        self._check(self.lib.vmr_fit_loop(self._h, int(max_iter), float(tol), int(decision), cap, C.byref(n), ri.ctypes.data,
                                          re.ctypes.data, rt.ctypes.data, rr.ctypes.data, C.byref(e), C.byref(its), C.byref(conv)))
        k = n.value
        return list(zip(ri[:k].tolist(), re[:k].tolist(), rt[:k].tolist(), [bool(v) for v in rr[:k]])), e.value, its.value, bool(conv.value)

    @staticmethod
    def fit_loop_batch(engines, max_iter, tol, decision):
        """`fit_loop` of several engines in lockstep (vmr_fit_loop_batch): the sweeps of all of them share one launch per kernel.
        Every engine must have had its `set_state`.  Returns one `fit_loop` result per engine, in order."""
        engines = list(engines)
        n = len(engines)
        if n == 0:
            return []
        lib = engines[0].lib
        cap = max_iter // 10 + 2
        hs = (C.c_void_p * n)(*[e._h for e in engines])
        nr, its, conv, rcs = (np.zeros(n, np.int32) for _ in range(4))
        e = np.zeros(n)
        ri, rr = np.empty((n, cap), np.int32), np.empty((n, cap), np.int32)
        re, rt = np.empty((n, cap)), np.empty((n, cap))
        rc = lib.vmr_fit_loop_batch(hs, n, int(max_iter), float(tol), int(decision), cap, nr.ctypes.data, ri.ctypes.data,
                                    re.ctypes.data, rt.ctypes.data, rr.ctypes.data, e.ctypes.data, its.ctypes.data,
                                    conv.ctypes.data, rcs.ctypes.data)
        out = []
        for u, eng in enumerate(engines):
            eng._check(int(rcs[u]))
        if rc != 0:   # (a failure before the per-unit codes were written: argument checks)
            engines[0]._check(int(rc))
        for u, eng in enumerate(engines):
            k = int(nr[u])
            out.append((list(zip(ri[u, :k].tolist(), re[u, :k].tolist(), rt[u, :k].tolist(), [bool(v) for v in rr[u, :k]])),
                        float(e[u]), int(its[u]), bool(conv[u])))
        return out

    def elbo(self):
        e = C.c_double()
        self._check(self.lib.vmr_elbo(self._h, C.byref(e)))
        return e.value

    def sweep_local(self, want_elbo=False):
        """Layer-sharded fits: one sweep on the local layers without committing nu -> (nu_partial, elbo_main, elbo_q)."""
        out = (C.c_double * 3)()
        self._check(self.lib.vmr_sweep_local(self._h, int(want_elbo), out))
        return out[0], out[1], out[2]

    def commit_nu(self, nu_partial_total):
        self._check(self.lib.vmr_commit_nu(self._h, float(nu_partial_total)))

    def stream_ptr(self):
        """The handle's hipStream_t (for collectives queued between the engine's kernels: torch.cuda.ExternalStream)."""
        return int(self.lib.vmr_stream(self._h) or 0)

    def sweep_local_dev(self, out3, want_elbo=False):
        """`sweep_local` that leaves (nu_partial, elbo_main, elbo_q) in the float64 CUDA tensor `out3` (3 elements),
        asynchronously on the engine's stream."""
        assert out3.is_cuda and out3.numel() >= 3 and out3.is_contiguous()
        self._check(self.lib.vmr_sweep_local_dev(self._h, int(want_elbo), out3.data_ptr()))

    def commit_nu_dev(self, total):
        """`commit_nu` from a float64 CUDA tensor holding the summed nu partial in element 0 (no host hop)."""
        self._check(self.lib.vmr_commit_nu_dev(self._h, total.data_ptr()))

    def sample(self, seed, n_trials=1, out=None):
        """One posterior sample of Y [L,N,N] uint8 drawn on the device from the current rho: per tie the most frequent
        category of n_trials categorical trials (`Generator.multinomial(n_trials, rho).argmax(-1)`, reference
        model.py:1062-1096), Philox stream keyed by `seed`.  out: a uint8 CUDA tensor to keep the sample on the device."""
        if out is not None:
            assert out.is_cuda and out.is_contiguous() and out.numel() == self.L * self.N * self.N
            self._check(self.lib.vmr_sample(self._h, int(seed) & (2 ** 64 - 1), int(n_trials), out.data_ptr(), 1))
            return out
        y = np.empty((self.L, self.N, self.N), np.uint8)
        self._check(self.lib.vmr_sample(self._h, int(seed) & (2 ** 64 - 1), int(n_trials), y.ctypes.data, 0))
        return y

    def sample_stats(self, seed, n_samples, n_trials=1, Y_ref=None, degrees=False):
        """Network statistics of n_samples posterior samples, computed on the device (vmr_sample_stats): sample s is
        `self.sample(seed + s, n_trials)`, and only the counts come back.  Returns a dict of NumPy arrays: `edges` #{Y > 0},
        `weight` sum Y, `mutual` #{Y_ij > 0 and Y_ji > 0}, `tp` #{Y > 0 and Y_ref > 0} (zeros without Y_ref), each int64 [S, L]
        over all (i, j) of a layer; with degrees=True also `deg_out`, `deg_in` int32 [S, L, N].  Y_ref: [L,N,N], a NumPy array
        (compared with 0) or a uint8 CUDA tensor."""
        S = int(n_samples)
        shape = (self.L, self.N, self.N)
        yp, ydev, keep = None, 0, None
        if Y_ref is not None:
            if _is_torch(Y_ref):
                import torch
                if (not Y_ref.is_cuda or Y_ref.dtype != torch.uint8 or not Y_ref.is_contiguous()
                        or tuple(Y_ref.shape) != shape):
                    raise ValueError(f"device Y_ref must be a contiguous torch.uint8 GPU tensor of shape {shape}")
                torch.cuda.synchronize(Y_ref.device)
                yp, ydev, keep = Y_ref.data_ptr(), 1, Y_ref
            else:
                Y_ref = np.asarray(Y_ref)
                if Y_ref.shape != shape:
                    raise ValueError(f"Y_ref has shape {Y_ref.shape}, the engine's networks {shape}")
                keep = np.ascontiguousarray(Y_ref > 0, dtype=np.uint8)
                yp = keep.ctypes.data
        counts = np.zeros((max(S, 0), self.L, 4), np.uint64)
        dout = np.zeros((max(S, 0), self.L, self.N), np.int32) if degrees else None
        din = np.zeros((max(S, 0), self.L, self.N), np.int32) if degrees else None
        self._check(self.lib.vmr_sample_stats(self._h, int(seed) & (2 ** 64 - 1), S, int(n_trials), yp, ydev, counts.ctypes.data,
                                              dout.ctypes.data if degrees else None, din.ctypes.data if degrees else None))
        del keep
        c = counts.astype(np.int64)
        out = {"edges": c[..., 0], "weight": c[..., 1], "mutual": c[..., 2], "tp": c[..., 3]}
        if degrees:
            out["deg_out"], out["deg_in"] = dout, din
        return out

    def expected_stats(self):
        """The statistics of `sample_stats` in expectation under q(Y) = prod rho (vmr_expected_stats), with p_ij = sum_{k>=1}
        rho_ijk: dict of float64 [L] arrays `edges` sum p, `weight` sum_ij sum_k k rho_ijk, `mutual` sum_ij p_ij p_ji (all ordered
        pairs: the diagonal enters as p_ii^2) and `edges_var` sum p (1 - p)."""
        out = np.zeros((self.L, 4), np.float64)
        self._check(self.lib.vmr_expected_stats(self._h, out.ctypes.data))
        return {"edges": out[:, 0].copy(), "weight": out[:, 1].copy(), "mutual": out[:, 2].copy(), "edges_var": out[:, 3].copy()}

    def sample_triads(self, seed, n_samples, n_trials=1, nodes=False):
        """Triad statistics of n_samples posterior samples, computed on the device (vmr_sample_triads): sample s is
        `self.sample(seed + s, n_trials)`, A = (Y > 0) with the diagonal cleared, U = A | A.T.  Returns a dict of int64 [S, L]
        arrays: `transitive` #{i->j, j->k, i->k}, `cyclic` #{i->j, j->k, k->i} (ordered: a 3-cycle counts 3 times), `two_paths`
        #{i->j, j->k}, `triangles_u`, `wedges_u` sum_i d_i (d_i - 1) / 2 and `edges_u` of U; with nodes=True also `node_tri` (the
        triangles of U through each node) and `node_deg` (its degree in U), int32 [S, L, N].  A refused argument raises
        `TriadArgumentError`."""
        S = int(n_samples)
        counts = np.zeros((max(S, 0), self.L, _lib.TRIAD_NSTAT), np.uint64)
        ntri = np.zeros((max(S, 0), self.L, self.N), np.int32) if nodes else None
        ndeg = np.zeros((max(S, 0), self.L, self.N), np.int32) if nodes else None
        self._check(self.lib.vmr_sample_triads(self._h, int(seed) & (2 ** 64 - 1), S, int(n_trials), counts.ctypes.data,
                                               ntri.ctypes.data if nodes else None, ndeg.ctypes.data if nodes else None),
                    TriadArgumentError)
        c = counts.astype(np.int64)
        out = {k: np.ascontiguousarray(c[..., q]) for q, k in enumerate(_lib.TRIAD_NAMES)}
        if nodes:
            out["node_tri"], out["node_deg"] = ntri, ndeg
        return out

    def expected_triads(self):
        """The six counts of `sample_triads` in expectation under q(Y) = prod rho (vmr_expected_triads), no sampling: dict of
        float64 [L] arrays under the same names.  Expectations of counts: a ratio of two of them is not the expectation of the
        ratio."""
        out = np.zeros((self.L, _lib.TRIAD_NSTAT), np.float64)
        self._check(self.lib.vmr_expected_triads(self._h, out.ctypes.data), TriadArgumentError)
        return {k: out[:, q].copy() for q, k in enumerate(_lib.TRIAD_NAMES)}

    def sample_connectivity(self, seed, n_samples, n_trials=1, hist=True, nodes=False):
        """Connectivity of n_samples posterior samples, computed on the device (vmr_sample_connectivity): sample s is
        `self.sample(seed + s, n_trials)`, A = (Y > 0) with the diagonal cleared, U = A | A.T, d(i, j) the length of a shortest
        directed path in A.  Returns a dict of int64 [S, L] arrays keyed by `_lib.CONN_NAMES`: `components_w`, `giant_w`, `pairs_w`
        (ordered pairs in one weak component), `isolates`, `components_s`, `giant_s`, `pairs_s` (ordered pairs that reach each
        other), `reach_pairs` #{i != j : d(i, j) finite}, `dist_sum` (the sum of those distances) and `diameter` (their maximum);
        with hist=True also `dist_hist` int64 [S, L, 64], bin d - 1 the ordered pairs at distance d, the last bin every distance
        >= 64; with nodes=True also `node_comp_w`, `node_comp_s` (the smallest node index of the node's weak / strong component),
        `node_reach_out`, `node_reach_in` (nodes it reaches / is reached by) and `node_dist_out`, `node_dist_in` (the sums of
        those distances), int32 [S, L, N].  N is at most `_lib.CONN_NMAX`.  A refused argument raises
        `ConnectivityArgumentError`."""
        S = int(n_samples)
        counts = np.zeros((max(S, 0), self.L, _lib.CONN_NSTAT), np.uint64)
        dh = np.zeros((max(S, 0), self.L, _lib.CONN_NDIST), np.uint64) if hist else None
        na = [np.zeros((max(S, 0), self.L, self.N), np.int32) if nodes else None for _ in _lib.CONN_NODE_NAMES]
        self._check(self.lib.vmr_sample_connectivity(self._h, int(seed) & (2 ** 64 - 1), S, int(n_trials), counts.ctypes.data,
                                                     dh.ctypes.data if hist else None, *[a.ctypes.data if nodes else None for a in na]),
                    ConnectivityArgumentError)
        c = counts.astype(np.int64)
        out = {k: np.ascontiguousarray(c[..., q]) for q, k in enumerate(_lib.CONN_NAMES)}
        if hist:
            out["dist_hist"] = dh.astype(np.int64)
        if nodes:
            out.update(zip(_lib.CONN_NODE_NAMES, na))
        return out

    @staticmethod
    def _name_code(value, names, what, error):
        """The code of a direction or mode given by name; a name that is none of `names` is refused here."""
        if isinstance(value, str):
            if value not in names:
                raise error(f"{what} must be one of {names}, got {value!r}")
            return names.index(value)
        return int(value)

    def _centrality_args(self, q, direction):
        """(q float64 [L], the direction's code) for the centrality calls; what is not a number or a name is refused here."""
        try:
            qa = np.ascontiguousarray(np.broadcast_to(np.asarray(q, dtype=np.float64), (self.L,)))
        except (TypeError, ValueError):
            raise CentralityArgumentError(f"q must be a scalar or {self.L} numbers, one per layer") from None
        return qa, self._name_code(direction, _lib.CENT_DIRECTIONS, "direction", CentralityArgumentError)

    def _node_outputs(self, S, stats, stat_dtype, values_dtype, counters=()):
        """What a call of the node-score fold writes: (pointers, result).  pointers, in the calls' order: node_sum, node_sumsq
        (float64 [L, N]), node_rank_sum (uint64), node_top and the unit's `counters` (uint32), the summary `stat_dtype` [S, L,
        len(stats)] and the values `values_dtype` [S, L, N] (None: not asked for).  result() is the call's dict: the integers as
        int64, a `stats` name for each column of the summary, `values` when asked for."""
        S, LN = max(int(S), 0), (self.L, self.N)
        sums = {"node_sum": np.zeros(LN, np.float64), "node_sumsq": np.zeros(LN, np.float64)}
        ints = {"node_rank_sum": np.zeros(LN, np.uint64), "node_top": np.zeros(LN, np.uint32)}
        for k in counters:
            ints[k] = np.zeros(LN, np.uint32)
        sm = np.zeros((S, self.L, len(stats)), stat_dtype)
        vals = None if values_dtype is None else np.zeros((S,) + LN, values_dtype)
        stat_out = np.float64 if stat_dtype is np.float64 else np.int64

        def result():
            out = dict(sums)
            for k, a in ints.items():
                out[k] = a.astype(np.int64)
            for q, name in enumerate(stats):
                out[name] = sm[..., q].astype(stat_out)
            if vals is not None:
                out["values"] = vals
            return out
        ptrs = [a.ctypes.data for a in sums.values()] + [a.ctypes.data for a in ints.values()]
        return ptrs + [sm.ctypes.data, None if vals is None else vals.ctypes.data], result

    def _network_ties(self, Y, error):
        """(ties uint8 [n, L, N, N], one) for the `network_*` calls: Y [L, N, N] (one: True) or [n, L, N, N], an entry > 0 a tie."""
        Ya = np.asarray(Y)
        one = Ya.ndim == 3
        if one:
            Ya = Ya[None]
        if Ya.ndim != 4 or Ya.shape[1:] != (self.L, self.N, self.N):
            raise error(f"Y has shape {np.shape(Y)}, the engine's networks {(self.L, self.N, self.N)}")
        return np.ascontiguousarray(Ya > 0, dtype=np.uint8), one

    def sample_centrality(self, seed, n_samples, q, T, direction="out", top_k=10, n_trials=1, values=False):
        """Diffusion centrality of n_samples posterior samples, computed on the device (vmr_sample_centrality): sample s is
        `self.sample(seed + s, n_trials)`, A = (Y > 0) with the diagonal cleared, M = A ("out": walks leave the node), A.T ("in")
        or A | A.T ("union"), and c = sum_{t=1..T} (q_l M)^t 1 per layer l; q: a scalar or [L], each in [0, 1]; T in [1,
        `_lib.CENT_TMAX`].  rank[v] = #{u : c[u] > c[v]} (0: the most central node; ties share the smaller rank).  Returns a dict:
        `node_sum`, `node_sumsq` float64 [L, N] (sum_s c, sum_s c^2), `node_rank_sum` int64 [L, N], `node_top` int64 [L, N]
        (#{s : rank < top_k}), `total`, `max` float64 [S, L] (sum_v c[v], max_v c[v]); with values=True also `values` float64
        [S, L, N].  Every number is the same from run to run and for any chunking.  N is at most `_lib.CENT_NMAX`.  A refused
        argument raises `CentralityArgumentError`."""
        qa, d = self._centrality_args(q, direction)
        ptrs, result = self._node_outputs(n_samples, ("total", "max"), np.float64, np.float64 if values else None)
        self._check(self.lib.vmr_sample_centrality(self._h, int(seed) & (2 ** 64 - 1), int(n_samples), int(n_trials), qa.ctypes.data, int(T), d,
                                                   int(top_k), *ptrs), CentralityArgumentError)
        return result()

    def mean_centrality(self, q, T, direction="out"):
        """The diffusion centrality of the posterior MEAN network (vmr_mean_centrality), no sampling: float64 [L, N],
        sum_{t=1..T} (q_l M)^t 1 with M = P ("out"; p_ij = sum_{k>=1} rho_ijk, p_ii := 0), P.T ("in") or U ("union"; u_ij = 1 -
        (1 - p_ij)(1 - p_ji)).  A plug-in: for "out" and "in" with T <= 2 it is also the expectation of the sampled centrality,
        for T >= 3 or "union" it is not.  Any N.  A refused argument raises `CentralityArgumentError`."""
        qa, d = self._centrality_args(q, direction)
        out = np.zeros((self.L, self.N), np.float64)
        self._check(self.lib.vmr_mean_centrality(self._h, qa.ctypes.data, int(T), d, out.ctypes.data), CentralityArgumentError)
        return out

    def sample_betweenness(self, seed, n_samples, direction="directed", top_k=10, n_trials=1, values=False):
        """Betweenness centrality of n_samples posterior samples, computed on the device (vmr_sample_betweenness): sample s is
        `self.sample(seed + s, n_trials)`, A = (Y > 0) with the diagonal cleared, the search graph A ("directed") or A | A.T
        ("union"), and b[v] = sum over s != v != t of the share of the shortest s -> t paths through v: unnormalised, endpoints
        excluded, every unordered pair once for "union" -- `networkx.betweenness_centrality(normalized=False)`.  rank[v] =
        #{u : b[u] > b[v]} (0: the first broker; ties share the smaller rank).  Returns a dict: `node_sum`, `node_sumsq` float64
        [L, N] (sum_s b, sum_s b^2), `node_rank_sum` int64 [L, N], `node_top` int64 [L, N] (#{s : rank < top_k}), `total`, `max`
        float64 [S, L] (sum_v b[v], max_v b[v]); with values=True also `values` float64 [S, L, N].  Every number is the same from
        run to run and for any chunking.  N is at most `_lib.BTW_NMAX`.  A refused argument raises `BetweennessArgumentError`."""
        d = self._name_code(direction, _lib.BTW_DIRECTIONS, "direction", BetweennessArgumentError)
        ptrs, result = self._node_outputs(n_samples, ("total", "max"), np.float64, np.float64 if values else None)
        self._check(self.lib.vmr_sample_betweenness(self._h, int(seed) & (2 ** 64 - 1), int(n_samples), int(n_trials), d, int(top_k), *ptrs),
                    BetweennessArgumentError)
        return result()

    def network_betweenness(self, Y, direction="directed"):
        """The betweenness of `sample_betweenness` of networks the caller supplies (vmr_network_betweenness), by the same kernels:
        Y [L, N, N] -> float64 [L, N], or [n, L, N, N] -> [n, L, N]; an entry > 0 is a tie, the diagonal is ignored.  The engine
        gives the shape and the device only: no state is needed and rho is not touched.  A refused argument raises
        `BetweennessArgumentError`."""
        d = self._name_code(direction, _lib.BTW_DIRECTIONS, "direction", BetweennessArgumentError)
        ties, one = self._network_ties(Y, BetweennessArgumentError)
        out = np.zeros((ties.shape[0], self.L, self.N), np.float64)
        self._check(self.lib.vmr_network_betweenness(self._h, ties.ctypes.data, ties.shape[0], d, out.ctypes.data), BetweennessArgumentError)
        return out[0] if one else out

    def sample_cores(self, seed, n_samples, mode="union", k_min=0, top_k=10, n_trials=1, values=False):
        """The k-core decomposition of n_samples posterior samples, computed on the device (vmr_sample_cores): sample s is
        `self.sample(seed + s, n_trials)`, A = (Y > 0) with the diagonal cleared, core[v] the largest k such that v lies in a node
        set whose every node has degree >= k inside the set; the degree is the distinct neighbours in A | A.T ("union":
        `networkx.core_number` of the undirected graph), in-degree plus out-degree ("total": `networkx.core_number` of the
        DiGraph), the in-degree ("in") or the out-degree ("out").  rank[v] = #{u : core[u] > core[v]}: a whole shell shares a
        rank, the main core has rank 0.  Returns a dict: `node_sum`, `node_sumsq` float64 [L, N] (sum_s core, sum_s core^2, exact
        integers), `node_rank_sum`, `node_top` (#{s : rank < top_k}), `node_main` (#{s : core = the sample's degeneracy}),
        `node_atleast` (#{s : core >= k_min}) int64 [L, N], and `degeneracy`, `main_core_size`, `core_sum`, `kcore_size` int64
        [S, L] (max_v core, the nodes that attain it, sum_v core, #{v : core >= k_min}); with values=True also `values` uint16
        [S, L, N].  Every number is the same from run to run and for any chunking.  N is at most `_lib.CORE_NMAX`.  A refused
        argument raises `CoresArgumentError`."""
        md = self._name_code(mode, _lib.CORE_MODES, "mode", CoresArgumentError)
        ptrs, result = self._node_outputs(n_samples, _CORE_STATS, np.uint32, np.uint16 if values else None, counters=("node_main", "node_atleast"))
        self._check(self.lib.vmr_sample_cores(self._h, int(seed) & (2 ** 64 - 1), int(n_samples), int(n_trials), md, int(k_min), int(top_k), *ptrs),
                    CoresArgumentError)
        return result()

    def network_cores(self, Y, mode="union", k_min=0, summary=False):
        """The coreness of `sample_cores` of networks the caller supplies (vmr_network_cores), by the same kernel: Y [L, N, N] ->
        uint16 [L, N], or [n, L, N, N] -> [n, L, N]; an entry > 0 is a tie, the diagonal is ignored.  summary=True: returns
        (values, dict of `degeneracy`, `main_core_size`, `core_sum`, `kcore_size`, int64 [L] or [n, L]).  The engine gives the
        shape and the device only: no state is needed and rho is not touched.  A refused argument raises `CoresArgumentError`."""
        md = self._name_code(mode, _lib.CORE_MODES, "mode", CoresArgumentError)
        ties, one = self._network_ties(Y, CoresArgumentError)
        out = np.zeros((ties.shape[0], self.L, self.N), np.uint16)
        sm = np.zeros((ties.shape[0], self.L, 4), np.uint32) if summary else None
        self._check(self.lib.vmr_network_cores(self._h, ties.ctypes.data, ties.shape[0], md, int(k_min), out.ctypes.data,
                                               sm.ctypes.data if summary else None), CoresArgumentError)
        if not summary:
            return out[0] if one else out
        smd = {name: (sm[0, :, q] if one else sm[..., q]).astype(np.int64) for q, name in enumerate(_CORE_STATS)}
        return (out[0] if one else out), smd

    def sample_cutpoints(self, seed, n_samples, mode="union", top_k=10, n_trials=1, values=False):
        """Cut points, bridges and fragmentation of n_samples posterior samples, computed on the device (vmr_sample_cutpoints):
        sample s is `self.sample(seed + s, n_trials)`, A = (Y > 0) with the diagonal cleared, G the undirected graph A | A.T
        ("union": networkx on `G.to_undirected()`) or A & A.T ("mutual": the reciprocated ties).  The branches of node v are the
        components of v's component once v is taken out, of sizes s_1..s_b: branches[v] = b (0 for an isolate; v is a cut point
        iff b >= 2), pairs_cut[v] = sum_{i<j} s_i s_j the pairs of other nodes that lose every path with v, bridges[v] the branches
        that hold exactly one neighbour of v (the tie to it is a bridge of G).  rank[v] = #{u : pairs_cut[u] > pairs_cut[v]}: all
        non-cut nodes share a rank, so `node_top` can count more than top_k nodes per sample.  Returns a dict: `node_sum`,
        `node_sumsq` float64 [L, N] (sum_s pairs_cut, sum_s pairs_cut^2, exact integers), `node_rank_sum`, `node_top` (#{s : rank <
        top_k}), `node_cut` (#{s : branches >= 2}), `node_branch_sum`, `node_bridge_sum` int64 [L, N], and `n_cut`, `n_bridges`,
        `max_pairs_cut`, `connected_pairs` int64 [S, L] (the cut points, the bridges, max_v pairs_cut and the connected unordered
        pairs of G); with values=True also `pairs_cut` uint32, `branches`, `bridges` uint16 [S, L, N].  Every number is the same
        from run to run and for any chunking.  N is at most `_lib.CUT_NMAX`.  A refused argument raises `CutpointArgumentError`."""
        md = self._name_code(mode, _lib.CUT_MODES, "mode", CutpointArgumentError)
        S, LN = max(int(n_samples), 0), (self.L, self.N)
        sums = {"node_sum": np.zeros(LN, np.float64), "node_sumsq": np.zeros(LN, np.float64)}
        ints = {"node_rank_sum": np.zeros(LN, np.uint64), "node_top": np.zeros(LN, np.uint32), "node_cut": np.zeros(LN, np.uint32),
                "node_branch_sum": np.zeros(LN, np.uint64), "node_bridge_sum": np.zeros(LN, np.uint64)}
        sm = np.zeros((S, self.L, 4), np.uint32)
        vals = {"pairs_cut": np.zeros((S,) + LN, np.uint32), "branches": np.zeros((S,) + LN, np.uint16),
                "bridges": np.zeros((S,) + LN, np.uint16)} if values else {}
        ptrs = [a.ctypes.data for a in sums.values()] + [a.ctypes.data for a in ints.values()] + [sm.ctypes.data]
        ptrs += [a.ctypes.data for a in vals.values()] if values else [None] * 3
        self._check(self.lib.vmr_sample_cutpoints(self._h, int(seed) & (2 ** 64 - 1), int(n_samples), int(n_trials), md, int(top_k), *ptrs),
                    CutpointArgumentError)
        out = dict(sums)
        out.update({k: a.astype(np.int64) for k, a in ints.items()})
        out.update({name: sm[..., q].astype(np.int64) for q, name in enumerate(_lib.CUT_SUMMARY)})
        out.update(vals)
        return out

    def network_cutpoints(self, Y, mode="union", summary=False):
        """The numbers of `sample_cutpoints` of networks the caller supplies (vmr_network_cutpoints), by the same kernels: Y [L, N,
        N] -> a dict of `pairs_cut` uint32, `branches`, `bridges` uint16 [L, N], or [n, L, N, N] -> [n, L, N]; an entry > 0 is a
        tie, the diagonal is ignored.  summary=True: the dict also holds `n_cut`, `n_bridges`, `max_pairs_cut`, `connected_pairs`,
        int64 [L] or [n, L].  The engine gives the shape and the device only: no state is needed and rho is not touched.  A
        refused argument raises `CutpointArgumentError`."""
        md = self._name_code(mode, _lib.CUT_MODES, "mode", CutpointArgumentError)
        ties, one = self._network_ties(Y, CutpointArgumentError)
        n = ties.shape[0]
        out = {"pairs_cut": np.zeros((n, self.L, self.N), np.uint32), "branches": np.zeros((n, self.L, self.N), np.uint16),
               "bridges": np.zeros((n, self.L, self.N), np.uint16)}
        sm = np.zeros((n, self.L, 4), np.uint32) if summary else None
        self._check(self.lib.vmr_network_cutpoints(self._h, ties.ctypes.data, n, md, out["pairs_cut"].ctypes.data, out["branches"].ctypes.data,
                                                   out["bridges"].ctypes.data, sm.ctypes.data if summary else None), CutpointArgumentError)
        if summary:
            out.update({name: sm[..., q].astype(np.int64) for q, name in enumerate(_lib.CUT_SUMMARY)})
        return {k: a[0] for k, a in out.items()} if one else out

    def _cascade_args(self, q, direction):
        """(q float64 [L], the direction's code) for the cascade calls; what is not a number or a name is refused here."""
        try:
            qa = np.ascontiguousarray(np.broadcast_to(np.asarray(q, dtype=np.float64), (self.L,)))
        except (TypeError, ValueError):
            raise CascadeArgumentError(f"q must be a scalar or {self.L} numbers, one per layer") from None
        return qa, self._name_code(direction, _lib.CASC_DIRECTIONS, "direction", CascadeArgumentError)

    def seed_words(self, seed_sets):
        """(words uint64 [N], n_sets) of seed sets for the `*_seed_outreach` calls: bit b of word v is set iff node v is in set b.
        seed_sets: a sequence of node-index sequences (a set may be empty, a node may be in several sets), or the words
        themselves as a uint64 [N] array (then n_sets is 64 unless the call names it)."""
        if isinstance(seed_sets, np.ndarray) and seed_sets.dtype == np.uint64:
            if seed_sets.shape != (self.N,):
                raise CascadeArgumentError(f"seed words of shape {seed_sets.shape}, expected ({self.N},)")
            return np.ascontiguousarray(seed_sets), _lib.CASC_SETS
        sets = list(seed_sets)
        if not 1 <= len(sets) <= _lib.CASC_SETS:
            raise CascadeArgumentError(f"between 1 and {_lib.CASC_SETS} seed sets expected, got {len(sets)}")
        words = np.zeros(self.N, np.uint64)
        for b, nodes in enumerate(sets):
            idx = np.asarray(list(nodes), dtype=np.int64).reshape(-1)
            if idx.size and (idx.min() < 0 or idx.max() >= self.N):
                raise CascadeArgumentError(f"seed set {b} names a node outside [0, {self.N})")
            words[idx] |= np.uint64(1) << np.uint64(b)
        return words, len(sets)

    def _seed_outputs(self, n, n_sets, curve, node_hits):
        """The arrays of a `*_seed_outreach` call for n samples or networks: (values, curve or None, node_hits or None)."""
        vals = np.zeros((max(int(n), 0), self.L, n_sets), np.uint32)
        cv = np.zeros((self.L, n_sets, _lib.CASC_NPER), np.uint64) if curve else None
        nh = np.zeros((self.L, n_sets, self.N), np.uint32) if node_hits else None
        return vals, cv, nh

    @staticmethod
    def _seed_result(vals, cv, nh):
        out = {"values": vals}
        if cv is not None:
            out["curve"] = cv.astype(np.int64)
        if nh is not None:
            out["node_hits"] = nh.astype(np.int64)
        return out

    def sample_outreach(self, seed, n_samples, q, T=3, direction="out", n_cascades=16, cascade_seed=0, top_k=10, n_trials=1, values=False):
        """The outreach of every node as a single seed under the independent-cascade model, over n_samples posterior samples and
        n_cascades cascades each, computed on the device (vmr_sample_outreach): sample s is `self.sample(seed + s, n_trials)`,
        A = (Y > 0) with the diagonal cleared; cascade k of sample s keeps tie (l, i, j) iff u < q_l, u the sampler's uniform from
        Philox4x32-10 with key cascade_seed + s and counter (tie index, k, 1); the spread follows A ("out"), A.T ("in") or
        A | A.T ("union", one draw per pair); the outreach of v is the number of other nodes reached within T periods.  q: a
        scalar or [L], each in [0, 1]; T in [1, `_lib.CASC_TMAX`]; n_cascades in [1, `_lib.CASC_KMAX`].  The node score is c =
        sum_k outreach / n_cascades, rank[v] = #{u : c[u] > c[v]} (0: the best entry point; ties share the smaller rank).  Returns
        a dict: `node_sum`, `node_sumsq` float64 [L, N] (sum_s c, sum_s c^2), `node_rank_sum`, `node_top` (#{s : rank < top_k})
        int64 [L, N], `total`, `max` int64 [S, L] (sum_v and max_v of the summed outreach; the sum is taken mod 2^32); with
        values=True also `values` uint32 [S, L, N], the outreach summed over the cascades.  Every number is an exact integer or a
        quotient of two, the same from run to run and for any chunking.  N is at most `_lib.CASC_NMAX`.  A refused argument
        raises `CascadeArgumentError`."""
        qa, d = self._cascade_args(q, direction)
        ptrs, result = self._node_outputs(n_samples, ("total", "max"), np.uint32, np.uint32 if values else None)
        self._check(self.lib.vmr_sample_outreach(self._h, int(seed) & (2 ** 64 - 1), int(n_samples), int(n_trials), int(cascade_seed) & (2 ** 64 - 1),
                                                 int(n_cascades), qa.ctypes.data, int(T), d, int(top_k), *ptrs), CascadeArgumentError)
        return result()

    def sample_seed_outreach(self, seed, n_samples, seed_sets, q, T=3, direction="out", n_cascades=16, cascade_seed=0, n_trials=1, curve=True,
                             node_hits=False, n_sets=None):
        """The outreach of up to `_lib.CASC_SETS` seed sets under the model of `sample_outreach`, computed on the device
        (vmr_sample_seed_outreach).  seed_sets: what `seed_words` takes (n_sets: for words given as an array).  Returns a dict:
        `values` uint32 [S, L, n_sets], the nodes outside the set that are reached within T periods, summed over the cascades;
        with curve=True `curve` int64 [L, n_sets, `_lib.CASC_NPER`], bin t - 1 the nodes newly reached at period t summed over
        samples and cascades (the last bin: every period >= 64); with node_hits=True `node_hits` int64 [L, n_sets, N], the
        (sample, cascade) pairs in which the node is informed after T periods, seeds included.  A refused argument raises
        `CascadeArgumentError`."""
        qa, d = self._cascade_args(q, direction)
        words, ns = self.seed_words(seed_sets)
        ns = ns if n_sets is None else int(n_sets)
        vals, cv, nh = self._seed_outputs(n_samples, max(ns, 1), curve, node_hits)
        self._check(self.lib.vmr_sample_seed_outreach(self._h, int(seed) & (2 ** 64 - 1), int(n_samples), int(n_trials),
                                                      int(cascade_seed) & (2 ** 64 - 1), int(n_cascades), qa.ctypes.data, int(T), d,
                                                      words.ctypes.data, ns, vals.ctypes.data, None if cv is None else cv.ctypes.data,
                                                      None if nh is None else nh.ctypes.data), CascadeArgumentError)
        return self._seed_result(vals, cv, nh)

    def network_outreach(self, Y, q, T=3, direction="out", n_cascades=16, cascade_seed=0, summary=False):
        """The summed outreach of `sample_outreach` of networks the caller supplies (vmr_network_outreach), by the same kernels:
        Y [L, N, N] -> uint32 [L, N], or [n, L, N, N] -> [n, L, N]; an entry > 0 is a tie, the diagonal is ignored; network i
        draws its cascades with the key cascade_seed + i.  summary=True: returns (values, dict of `total`, `max`, int64 [L] or
        [n, L]).  The engine gives the shape and the device only: no state is needed and rho is not touched.  A refused
        argument raises `CascadeArgumentError`."""
        qa, d = self._cascade_args(q, direction)
        ties, one = self._network_ties(Y, CascadeArgumentError)
        out = np.zeros((ties.shape[0], self.L, self.N), np.uint32)
        sm = np.zeros((ties.shape[0], self.L, 2), np.uint32) if summary else None
        self._check(self.lib.vmr_network_outreach(self._h, ties.ctypes.data, ties.shape[0], int(cascade_seed) & (2 ** 64 - 1), int(n_cascades),
                                                  qa.ctypes.data, int(T), d, out.ctypes.data, sm.ctypes.data if summary else None),
                    CascadeArgumentError)
        if not summary:
            return out[0] if one else out
        smd = {name: (sm[0, :, k] if one else sm[..., k]).astype(np.int64) for k, name in enumerate(("total", "max"))}
        return (out[0] if one else out), smd

    def network_seed_outreach(self, Y, seed_sets, q, T=3, direction="out", n_cascades=16, cascade_seed=0, curve=True, node_hits=False,
                              n_sets=None):
        """`sample_seed_outreach` of networks the caller supplies (vmr_network_seed_outreach): Y [L, N, N] or [n, L, N, N]; the
        dict's `values` is uint32 [L, n_sets] or [n, L, n_sets], `curve` and `node_hits` sum over the networks.  No state is
        needed.  A refused argument raises `CascadeArgumentError`."""
        qa, d = self._cascade_args(q, direction)
        ties, one = self._network_ties(Y, CascadeArgumentError)
        words, ns = self.seed_words(seed_sets)
        ns = ns if n_sets is None else int(n_sets)
        vals, cv, nh = self._seed_outputs(ties.shape[0], max(ns, 1), curve, node_hits)
        self._check(self.lib.vmr_network_seed_outreach(self._h, ties.ctypes.data, ties.shape[0], int(cascade_seed) & (2 ** 64 - 1), int(n_cascades),
                                                       qa.ctypes.data, int(T), d, words.ctypes.data, ns, vals.ctypes.data,
                                                       None if cv is None else cv.ctypes.data, None if nh is None else nh.ctypes.data),
                    CascadeArgumentError)
        return self._seed_result(vals[0] if one else vals, cv, nh)

    def sample_triad_census(self, seed, n_samples, n_trials=1):
        """The triad census of n_samples posterior samples, computed on the device (vmr_sample_triad_census): sample s is
        `self.sample(seed + s, n_trials)`, A = (Y > 0) with the diagonal cleared, and every unordered triple of nodes is counted
        in its Holland-Leinhardt class.  Returns int64 [S, L, 16] in the order of `_lib.CENSUS_NAMES` -- 003 012 102 021D 021U
        021C 111D 111U 030T 030C 201 120D 120U 120C 210 300, `networkx.triadic_census`'s order and naming; the 16 numbers of a
        sample and layer sum to C(N, 3).  Exact integers, the same from run to run and for any chunking.  A refused argument
        raises `CensusArgumentError`."""
        S = int(n_samples)
        counts = np.zeros((max(S, 0), self.L, _lib.CENSUS_NCLASS), np.uint64)
        self._check(self.lib.vmr_sample_triad_census(self._h, int(seed) & (2 ** 64 - 1), S, int(n_trials), counts.ctypes.data), CensusArgumentError)
        return counts.astype(np.int64)

    def network_triad_census(self, Y):
        """The census of `sample_triad_census` of networks the caller supplies (vmr_network_triad_census), by the same kernel:
        Y [L, N, N] -> int64 [L, 16], or [n, L, N, N] -> [n, L, 16]; an entry > 0 is a tie, the diagonal is ignored.  The engine
        gives the shape and the device only: no state is needed and rho is not touched.  A refused argument raises
        `CensusArgumentError`."""
        ties, one = self._network_ties(Y, CensusArgumentError)
        out = np.zeros((ties.shape[0], self.L, _lib.CENSUS_NCLASS), np.uint64)
        self._check(self.lib.vmr_network_triad_census(self._h, ties.ctypes.data, ties.shape[0], out.ctypes.data), CensusArgumentError)
        out = out.astype(np.int64)
        return out[0] if one else out

    def _partners_args(self, mode, n_bins, n, nodes, pairs):
        """(mode code, n_bins, hist, totals, the two node arrays or None, pairs int32 [P, 3] or None) for the shared-partner calls
        on n samples or networks."""
        if mode not in _lib.SP_MODES:
            raise PartnersArgumentError(f"mode must be one of {_lib.SP_MODES}, got {mode!r}")
        B = int(n_bins)
        hist = np.zeros((max(n, 0), self.L, max(B, 0)), np.uint64)
        totals = np.zeros((max(n, 0), self.L, _lib.SP_NTOTAL), np.uint64)
        nt = np.zeros((max(n, 0), self.L, self.N), np.int32) if nodes else None
        ns = np.zeros((max(n, 0), self.L, self.N), np.int32) if nodes else None
        pa = None
        if pairs is not None:
            pa = np.ascontiguousarray(pairs, dtype=np.int32)
            if pa.ndim != 2 or pa.shape[1] != 3:
                raise PartnersArgumentError(f"pairs has shape {np.shape(pairs)}, expected (n_pairs, 3): rows of (layer, i, j)")
        return _lib.SP_MODES.index(mode), B, hist, totals, nt, ns, pa

    @staticmethod
    def _partners_result(hist, totals, nt, ns, one=False):
        out = {"hist": hist.astype(np.int64), "totals": totals.astype(np.int64)}
        if nt is not None:
            out["node_ties"], out["node_supported"] = nt, ns
        return {k: v[0] for k, v in out.items()} if one else out

    def sample_shared_partners(self, seed, n_samples, n_trials=1, mode="union", n_bins=64, nodes=False, pairs=None):
        """Shared partners of the ties of n_samples posterior samples, computed on the device (vmr_sample_shared_partners): sample
        s is `self.sample(seed + s, n_trials)`, A = (Y > 0) with the diagonal cleared.  mode "union": the unordered pairs tied
        either way, a partner is tied (either way) to both ends; "mutual": the pairs tied both ways, a partner is tied both ways to
        both (Simmelian ties); "path": the ordered ties i -> j, a partner k has i -> k -> j.  Returns a dict: `hist` int64 [S, L,
        n_bins] (ties with exactly b partners; the last bin holds b >= n_bins - 1), `totals` int64 [S, L, 4] in the order of
        `_lib.SP_TOTALS` (ties, supported ties, partners summed over the ties, the largest count); with nodes=True `node_ties`
        and `node_supported` int32 [S, L, N] (the counted ties a node is an end of; those with a partner); with pairs (rows of
        (layer, i, j)) `pair_present`, `pair_supported`, `pair_partners` int64 [n_pairs]: the samples in which the pair is a
        counted tie, those in which it also has a partner, and its partners summed over the former.  Exact integers, the same from
        run to run and for any chunking.  A refused argument raises `PartnersArgumentError`."""
        S = int(n_samples)
        m, B, hist, totals, nt, ns, pa = self._partners_args(mode, n_bins, S, nodes, pairs)
        P = 0 if pa is None else len(pa)
        pr, ps, pp = np.zeros(P, np.uint32), np.zeros(P, np.uint32), np.zeros(P, np.uint64)
        ptr = lambda a: None if a is None else a.ctypes.data
        self._check(self.lib.vmr_sample_shared_partners(self._h, int(seed) & (2 ** 64 - 1), S, int(n_trials), m, B, hist.ctypes.data,
                                                        totals.ctypes.data, ptr(nt), ptr(ns), ptr(pa), P, pr.ctypes.data, ps.ctypes.data,
                                                        pp.ctypes.data), PartnersArgumentError)
        out = self._partners_result(hist, totals, nt, ns)
        if pa is not None:
            out.update(pair_present=pr.astype(np.int64), pair_supported=ps.astype(np.int64), pair_partners=pp.astype(np.int64))
        return out

    def network_shared_partners(self, Y, mode="union", n_bins=64, nodes=False, pairs=None):
        """The counts of `sample_shared_partners` of networks the caller supplies (vmr_network_shared_partners), by the same
        kernels: Y [L, N, N] or [n, L, N, N] (an entry > 0 is a tie, the diagonal is ignored) -> the same dict without or with the
        leading axis; with pairs `pair_partners` int32 [n, n_pairs]: the partners of every listed pair, -1 where it is not a
        counted tie.  The engine gives the shape and the device only: no state is needed and rho is not touched.  A refused
        argument raises `PartnersArgumentError`."""
        ties, one = self._network_ties(Y, PartnersArgumentError)
        n = ties.shape[0]
        m, B, hist, totals, nt, ns, pa = self._partners_args(mode, n_bins, n, nodes, pairs)
        P = 0 if pa is None else len(pa)
        pp = np.zeros((n, P), np.int32)
        ptr = lambda a: None if a is None else a.ctypes.data
        self._check(self.lib.vmr_network_shared_partners(self._h, ties.ctypes.data, n, m, B, hist.ctypes.data, totals.ctypes.data, ptr(nt), ptr(ns),
                                                         ptr(pa), P, pp.ctypes.data), PartnersArgumentError)
        out = self._partners_result(hist, totals, nt, ns, one)
        if pa is not None:
            out["pair_partners"] = pp[0] if one else pp
        return out

    @staticmethod
    def _holes_values(deg, st, red, es, con, sm, one=False):
        """The per-network dict of the structural-holes calls: the integers as they are (redundancy as int64), the two measures
        with NaN where the node is isolated (degree 0), the summary's columns under `_lib.SH_SUMMARY` when it was asked for."""
        undefined = deg == 0
        out = {"degree": deg, "strength": st, "redundancy": red.astype(np.int64), "effective_size": np.where(undefined, np.nan, es),
               "constraint": np.where(undefined, np.nan, con)}
        if sm is not None:
            out.update({name: np.ascontiguousarray(sm[..., q]) for q, name in enumerate(_lib.SH_SUMMARY)})
        return {k: v[0] for k, v in out.items()} if one else out

    def sample_structural_holes(self, seed, n_samples, n_trials=1, mode="union", top_k=10, values=False):
        """Burt's structural holes of n_samples posterior samples, computed on the device (vmr_sample_structural_holes): sample s
        is `self.sample(seed + s, n_trials)`, A = (Y > 0) with the diagonal cleared, U = A | A.T.  mode "union": the weights z = U,
        `networkx.effective_size` / `constraint` of the undirected graph; "weighted": z = A + A.T in {0, 1, 2}, networkx on the
        DiGraph -- but defined for every node with a tie, an in-tie included.  With d the degree in U and s the row sum of z: the
        redundancy numerator R (an exact integer), the effective size ES = d - R / (2 s), evaluated as (2 s d - R) / (2 s), and
        the constraint c = sum_j ((z_ij + sum_q z_iq z_qj / s_q) / s_i)^2; include/vimure_hip.h has the contract.  An isolated
        node is undefined.  rank[v] = #{defined u : ES_u > ES_v} by effective size and #{defined u : c_u < c_v} by constraint (0:
        the first broker), #defined for an undefined node.  Returns a dict: `node_sum`, `node_sumsq` float64 [2, L, N] (index 0 the
        effective size, 1 the constraint; an undefined sample adds 0), `node_rank_sum`, `node_top` (#{s : rank < top_k}) int64
        [2, L, N], `node_defined` int64 [L, N] (the samples in which the node has a tie) and, float64 [S, L] under the names of
        `_lib.SH_SUMMARY`, `n_defined`, `effective_size_sum`, `constraint_sum`; with values=True also `degree`, `strength` int32,
        `redundancy` int64 and `effective_size`, `constraint` float64 [S, L, N], NaN where the node is isolated.  Every number is
        the same from run to run and for any chunking.  Any N.  A refused argument raises `StructuralHolesArgumentError`."""
        md = self._name_code(mode, _lib.SH_MODES, "mode", StructuralHolesArgumentError)
        S, LN = max(int(n_samples), 0), (self.L, self.N)
        acc = {"node_sum": np.zeros((2,) + LN, np.float64), "node_sumsq": np.zeros((2,) + LN, np.float64),
               "node_rank_sum": np.zeros((2,) + LN, np.uint64), "node_top": np.zeros((2,) + LN, np.uint32), "node_defined": np.zeros(LN, np.uint32)}
        sm = np.zeros((S, self.L, len(_lib.SH_SUMMARY)), np.float64)
        per = [np.zeros((S,) + LN, t) for t in (np.int32, np.int32, np.uint64, np.float64, np.float64)] if values else [None] * 5
        self._check(self.lib.vmr_sample_structural_holes(self._h, int(seed) & (2 ** 64 - 1), int(n_samples), int(n_trials), md, int(top_k),
                                                         *[a.ctypes.data for a in acc.values()], sm.ctypes.data,
                                                         *[None if a is None else a.ctypes.data for a in per]), StructuralHolesArgumentError)
        out = {k: (a if a.dtype == np.float64 else a.astype(np.int64)) for k, a in acc.items()}
        out.update({name: np.ascontiguousarray(sm[..., q]) for q, name in enumerate(_lib.SH_SUMMARY)})
        if values:
            out.update(self._holes_values(*per, None))
        return out

    def network_structural_holes(self, Y, mode="union", summary=False):
        """The measures of `sample_structural_holes` of networks the caller supplies (vmr_network_structural_holes), by the same
        kernels: Y [L, N, N] or [n, L, N, N] (an entry > 0 is a tie, the diagonal is ignored) -> a dict of `degree`, `strength`
        int32, `redundancy` int64 and `effective_size`, `constraint` float64 (NaN where the node is isolated), [L, N] or [n, L, N];
        with summary=True also `n_defined`, `effective_size_sum`, `constraint_sum` float64 [L] or [n, L].  The engine gives the
        shape and the device only: no state is needed and rho is not touched.  A refused argument raises
        `StructuralHolesArgumentError`."""
        md = self._name_code(mode, _lib.SH_MODES, "mode", StructuralHolesArgumentError)
        ties, one = self._network_ties(Y, StructuralHolesArgumentError)
        n, LN = ties.shape[0], (self.L, self.N)
        es, con = np.zeros((n,) + LN, np.float64), np.zeros((n,) + LN, np.float64)
        deg, st, red = np.zeros((n,) + LN, np.int32), np.zeros((n,) + LN, np.int32), np.zeros((n,) + LN, np.uint64)
        sm = np.zeros((n, self.L, len(_lib.SH_SUMMARY)), np.float64) if summary else None
        self._check(self.lib.vmr_network_structural_holes(self._h, ties.ctypes.data, n, md, es.ctypes.data, con.ctypes.data, deg.ctypes.data,
                                                          st.ctypes.data, red.ctypes.data, sm.ctypes.data if summary else None),
                    StructuralHolesArgumentError)
        return self._holes_values(deg, st, red, es, con, sm, one)

    def _mixing_args(self, groups, C):
        """(codes int32 [N] or None, C) for the mixing calls: C None is the largest code + 1."""
        if groups is None:
            return None, 0
        g = np.asarray(groups)
        if g.shape != (self.N,) or g.dtype.kind not in "iu":
            raise ValueError(f"groups must be {self.N} integer codes (-1: the node is left out), got {g.dtype} {g.shape}")
        g = np.ascontiguousarray(np.clip(g.astype(np.int64), -2, 2 ** 31 - 1), dtype=np.int32)   # (out of range stays out of range)
        return g, int(g.max(initial=-1)) + 1 if C is None else int(C)

    def sample_mixing(self, seed, n_samples, groups=None, C=None, n_trials=1, skip_diagonal=True, overlap=True):
        """Mixing by node attribute and overlap between layers of n_samples posterior samples, computed on the device
        (vmr_sample_mixing): sample s is `self.sample(seed + s, n_trials)`.  groups: N integer codes in [0, C), -1 for a node that is
        left out of `mix` and `mutual` (C None: the largest code + 1); skip_diagonal leaves (i, i) out of every table.  Returns a
        dict of int64 arrays: with groups `mix` [S, L, C, C], mix[s, l, a, b] = #{(i, j) : g_i = a, g_j = b, Y_lij > 0}, and
        `mutual`, the same over the ties with Y_lji > 0 too (ordered pairs: symmetric in (a, b), a kept self-loop counts once);
        with overlap=True `overlap` [S, L, L], #{(i, j) : Y_lij > 0 and Y_l'ij > 0} over all nodes, labelled or not (its diagonal
        is the edge count).  A refused argument raises `MixingArgumentError` with the library's message."""
        S = int(n_samples)
        g, C = self._mixing_args(groups, C)
        grp = g is not None
        shape = (max(S, 0), self.L, max(C, 0), max(C, 0))
        mix = np.zeros(shape, np.uint64) if grp else None
        mut = np.zeros(shape, np.uint64) if grp else None
        ov = np.zeros((max(S, 0), self.L, self.L), np.uint64) if overlap else None
        self._check(self.lib.vmr_sample_mixing(self._h, int(seed) & (2 ** 64 - 1), S, int(n_trials), g.ctypes.data if grp else None, C,
                                               int(bool(skip_diagonal)), mix.ctypes.data if grp else None,
                                               mut.ctypes.data if grp else None, ov.ctypes.data if overlap else None), MixingArgumentError)
        out = {}
        if grp:
            out["mix"], out["mutual"] = mix.astype(np.int64), mut.astype(np.int64)
        if overlap:
            out["overlap"] = ov.astype(np.int64)
        return out

    def expected_mixing(self, groups=None, C=None, skip_diagonal=True, overlap=True):
        """The tables of `sample_mixing` in expectation under q(Y) = prod rho (vmr_expected_mixing), no sampling, with p_lij =
        sum_{k>=1} rho_lijk: dict of float64 arrays `mix` [L, C, C] sum p_lij and `mutual` sum p_lij p_lji over g_i = a, g_j = b (a
        kept diagonal enters as p_ii^2), `overlap` [L, L] sum_ij p_lij p_l'ij (sum p_lij on its diagonal).  Expectations of counts:
        a ratio of two of them is not the expectation of the ratio."""
        g, C = self._mixing_args(groups, C)
        grp = g is not None
        mix = np.zeros((self.L, max(C, 0), max(C, 0)), np.float64) if grp else None
        mut = np.zeros((self.L, max(C, 0), max(C, 0)), np.float64) if grp else None
        ov = np.zeros((self.L, self.L), np.float64) if overlap else None
        self._check(self.lib.vmr_expected_mixing(self._h, g.ctypes.data if grp else None, C, int(bool(skip_diagonal)),
                                                 mix.ctypes.data if grp else None, mut.ctypes.data if grp else None,
                                                 ov.ctypes.data if overlap else None), MixingArgumentError)
        out = {}
        if grp:
            out["mix"], out["mutual"] = mix, mut
        if overlap:
            out["overlap"] = ov
        return out

    def sub_step(self, which):
        self._check(self.lib.vmr_sub_step(self._h, int(which)))

    def sync(self):
        self._check(self.lib.vmr_sync(self._h))

    def readout(self, method, threshold=0.0):
        """Read-out of the current rho on the device: "rho_max" / "threshold" -> uint8 [L,N,N], "rho_mean" -> float64."""
        code = {"rho_max": _lib.READ_RHO_MAX, "rho_mean": _lib.READ_RHO_MEAN, "threshold": _lib.READ_THRESHOLD}[method]
        out = np.empty((self.L, self.N, self.N), np.float64 if method == "rho_mean" else np.uint8)
        self._check(self.lib.vmr_readout(self._h, code, float(threshold), out.ctypes.data, 0))
        return out

    def _layer_arg(self, layer):
        if layer is None:
            return -1
        layer = int(layer)
        if not 0 <= layer < self.L:
            raise ValueError(f"layer {layer} out of range [0, {self.L})")
        return layer

    def mean_poisson_size(self, layer=None):
        """|S|: the number of (l,i,j,m) with R != 0 (every one without R), of one layer or of all."""
        n = C.c_uint64()
        self._check(self.lib.vmr_mean_poisson_size(self._h, self._layer_arg(layer), C.byref(n)))
        return int(n.value)

    def mean_poisson(self, layer=None, device=False):
        """Expected reports of the current state over the support of R (`_calculate_mean_poisson`, reference
        model.py:1220-1293): (subs, vals) with subs = 4 int32 arrays (l, i, j, m) in lexicographic order, the real layer index
        in l.  device=True: torch tensors on the engine's GPU (vmr_mean_poisson writes them there)."""
        la = self._layer_arg(layer)
        n = self.mean_poisson_size(layer)
        if device:
            import torch
            dev = torch.device("cuda", self.device)
            subs = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4)]
            vals = torch.empty(n, dtype=torch.float64, device=dev)
            torch.cuda.synchronize(dev)
            ptrs, vp = [t.data_ptr() for t in subs], vals.data_ptr()
        else:
            subs = [np.empty(n, np.int32) for _ in range(4)]
            vals = np.empty(n, np.float64)
            ptrs, vp = [a.ctypes.data for a in subs], vals.ctypes.data
        if n:
            self._check(self.lib.vmr_mean_poisson(self._h, la, n, *ptrs, vp, int(bool(device))))
        return tuple(subs), vals

    def report_auc(self, layer=None):
        """(auc, n_pos, n_neg): AUC of the expected reports against X > 0 over the support of R (`utils.calculate_AUC` with
        mask = R, reference utils.py:40-66), exact; NaN when either class is empty."""
        a, p, q = C.c_double(), C.c_uint64(), C.c_uint64()
        self._check(self.lib.vmr_report_auc(self._h, self._layer_arg(layer), C.byref(a), C.byref(p), C.byref(q)))
        return a.value, int(p.value), int(q.value)

    def ppc_replicates(self, theta, lam, eta, seed_y, seed_x, n_trials=1, by_reporter=False):
        """Discrepancy statistics of posterior predictive replicates, drawn and reduced on the device (vmr_ppc_replicates): no
        replicate is written.  theta [n_rep, L, M], lam [n_rep, L, K], eta [n_rep] (each in [0, 1)): the parameters of every
        replicate.  Replicate r: Y = `self.sample(seed_y + r, n_trials)`, lambda of a tie = lam[r, l, Y], and over the support of
        this engine's R the counts `synthetic.device_build_x(None, theta[r], eta[r], seed_x + r, lam=...)` would hold, unclamped.
        Returns counts int64 [n_rep, L, 6] -- `_lib.PPC_STAT_NAMES`: n_pos, total, sumsq, mutual, ties_reported, ties_agreed --
        and, with by_reporter=True, also int64 [n_rep, L, M, 2]: (n_pos, total) of every reporter."""
        theta, lam = _f64(theta), _f64(lam)
        eta = _f64(np.atleast_1d(eta))
        n_rep = int(eta.shape[0])
        if theta.shape != (n_rep, self.L, self.M) or lam.shape != (n_rep, self.L, self.K) or eta.ndim != 1:
            raise ValueError(f"theta {theta.shape}, lam {lam.shape}, eta {eta.shape}: expected (n_rep, {self.L}, {self.M}), "
                             f"(n_rep, {self.L}, {self.K}), (n_rep,)")
        counts = np.zeros((n_rep, self.L, _lib.PPC_NSTAT), np.uint64)
        rep = np.zeros((n_rep, self.L, self.M, 2), np.uint64) if by_reporter else None
        self._check(self.lib.vmr_ppc_replicates(self._h, n_rep, int(seed_y) & (2 ** 64 - 1), int(seed_x) & (2 ** 64 - 1), int(n_trials),
                                                theta.ctypes.data, lam.ctypes.data, eta.ctypes.data, counts.ctypes.data,
                                                rep.ctypes.data if by_reporter else None))
        counts = counts.astype(np.int64)
        return (counts, rep.astype(np.int64)) if by_reporter else counts

    def ppc_observed(self, by_reporter=False):
        """The statistics of `ppc_replicates` of this engine's own X over the support of R (vmr_ppc_observed): int64 [L, 6], and
        with by_reporter=True also int64 [L, M, 2]."""
        counts = np.zeros((self.L, _lib.PPC_NSTAT), np.uint64)
        rep = np.zeros((self.L, self.M, 2), np.uint64) if by_reporter else None
        self._check(self.lib.vmr_ppc_observed(self._h, counts.ctypes.data, rep.ctypes.data if by_reporter else None))
        counts = counts.astype(np.int64)
        return (counts, rep.astype(np.int64)) if by_reporter else counts

    def _edge_args(self, method, threshold, select, layer):
        codes = {"rho_max": _lib.READ_RHO_MAX, "rho_mean": _lib.READ_RHO_MEAN, "threshold": _lib.READ_THRESHOLD}
        if method not in codes:
            raise ValueError("'method' should be one of \"rho_max\", \"threshold\".")
        if isinstance(select, str):
            select = (select,)
        if isinstance(select, (int, np.integer)):
            sel = int(select)
        else:
            bits = {"reported": _lib.EDGE_REPORTED, "inferred": _lib.EDGE_INFERRED}
            sel = 0
            for s in select:
                if s not in bits:
                    raise ValueError("'select' holds \"reported\", \"inferred\" or both.")
                sel |= bits[s]
        return codes[method], float(threshold), sel, self._layer_arg(layer)

    def edge_table_size(self, method="rho_max", threshold=0.0, select=("reported", "inferred"), layer=None):
        """Rows of `edge_table` for the same arguments (vmr_edge_table_size)."""
        code, thr, sel, la = self._edge_args(method, threshold, select, layer)
        n = C.c_uint64()
        self._check(self.lib.vmr_edge_table_size(self._h, code, thr, sel, la, C.byref(n)), EdgeTableArgumentError)
        return int(n.value)

    def edge_table(self, method="rho_max", threshold=0.0, select=("reported", "inferred"), layer=None, device=False, out=None):
        """The inferred network of the current rho as an edge table built on the device (vmr_edge_table): a row per tie (l,i,j)
        that someone reported (`n_rep > 0`; select "reported") and / or that the read-out infers (`y > 0`; "inferred"), in
        lexicographic order.  method "rho_max" or "threshold" (`rho_1 >= threshold`), as `readout`.  Returns a dict of arrays, one
        entry per `EDGE_COLUMNS`: l, i, j (int32), y (uint8, `readout`'s byte), prob (sum_{k>=1} rho_k), mean (sum_k k rho_k),
        n_rep #{m : X > 0}, total sum_m X, n_mask #{m : R != 0}, ego X[l,i,j,i], alter X[l,i,j,j] and y_T, n_rep_T, total_T of
        the mirror tie (l,j,i); counts over all reporters, R ignored.  select may also be the bit mask 1 | 2; layer: that layer
        only.  device=True: torch tensors on the engine's GPU.  out: a dict of preallocated arrays (all of one length, the
        capacity; any column may be missing) to fill instead; a capacity below the row count is refused before anything is
        written."""
        code, thr, sel, la = self._edge_args(method, threshold, select, layer)
        if out is not None:
            cap = {int(a.shape[0]) for a in out.values()}
            if len(cap) != 1:
                raise ValueError("out: arrays of one length expected")
            n, cols = cap.pop(), out
        else:
            n = self.edge_table_size(method, threshold, sel, layer)
            if device:
                import torch
                dev = torch.device("cuda", self.device)
                cols = {c: torch.empty(n, dtype=getattr(torch, _TORCH_NAME.get(np.dtype(t).name, np.dtype(t).name)), device=dev)
                        for c, t in EDGE_COLUMNS}
            else:
                cols = {c: np.empty(n, t) for c, t in EDGE_COLUMNS}
        ptrs = []
        for c, t in EDGE_COLUMNS:
            a = cols.get(c)
            if a is None:
                ptrs.append(None)
            elif _is_torch(a):
                assert a.is_cuda and a.is_contiguous() and a.element_size() == np.dtype(t).itemsize
                ptrs.append(a.data_ptr())
            else:
                assert a.dtype == np.dtype(t) and a.flags.c_contiguous
                ptrs.append(a.ctypes.data)
        on_dev = any(_is_torch(a) for a in cols.values())
        if on_dev:
            import torch
            torch.cuda.synchronize(torch.device("cuda", self.device))
        if n or out is not None:
            self._check(self.lib.vmr_edge_table(self._h, code, thr, sel, la, n, *ptrs, int(on_dev)), EdgeTableArgumentError)
        return cols

    def score_truth(self, Y_true, thresholds=None, score="rho1", skip_diagonal=False, auc=True, outputs=None):
        """The current rho scored against a ground-truth network on the device (vmr_score_truth): one pass over rho and one byte
        of truth per tie; neither rho nor a read-out crosses PCIe.  Y_true: [L,N,N], a NumPy array of categories (clipped to 255;
        only `> 0` and equality with the arg-max matter) or a uint8 CUDA tensor.  thresholds: finite, non-decreasing, at most
        `_lib.SCORE_MAX_THR` (None: np.linspace(0, 1, 101)).  score: "rho1" (rho[..., 1], what `readout("threshold", t)` compares)
        or "prob" (sum_{k>=1} rho_k).  Returns a dict of NumPy arrays: hist int64 [L, n_thr + 1, 2] (hist[l, c, b]: ties with
        exactly c thresholds <= s, by truth), conf int64 [L, 5], sums float64 [L, 4], auc float64 [L] and auc_pairs int64 [L, 2]
        = (U2, Q) (both None with auc=False: the sort of the positives' scores is skipped), n_ties int64 [L], thresholds --
        what `scoring.TruthScore` takes.  outputs: the subset of `SCORE_OUTPUTS` to ask the device for (the others are None)."""
        from .scoring import SCORES
        if score not in SCORES:
            raise ScoreArgumentError("score must be \"rho1\" or \"prob\"")
        try:
            thr = np.ascontiguousarray(np.atleast_1d(np.linspace(0, 1, 101) if thresholds is None else thresholds), dtype=np.float64)
        except (TypeError, ValueError) as e:
            raise ScoreArgumentError(f"thresholds: {e}") from None
        if thr.ndim != 1:
            raise ScoreArgumentError("thresholds: a 1-D sequence expected")
        if outputs is None:
            outputs = SCORE_OUTPUTS if auc else SCORE_OUTPUTS[:3]
        outputs = tuple(outputs)
        if any(o not in SCORE_OUTPUTS for o in outputs):
            raise ScoreArgumentError(f"outputs: a subset of {SCORE_OUTPUTS} expected")
        shape = (self.L, self.N, self.N)
        if Y_true is None:
            raise ScoreArgumentError("Y_true is None")
        if _is_torch(Y_true):
            import torch
            if not Y_true.is_cuda or Y_true.dtype != torch.uint8 or not Y_true.is_contiguous() or tuple(Y_true.shape) != shape:
                raise ScoreArgumentError(f"device Y_true must be a contiguous torch.uint8 GPU tensor of shape {shape}")
            torch.cuda.synchronize(Y_true.device)
            yp, ydev, keep = Y_true.data_ptr(), 1, Y_true
        else:
            Y_true = np.asarray(Y_true)
            if Y_true.shape != shape:
                raise ScoreArgumentError(f"Y_true has shape {Y_true.shape}, the engine's networks {shape}")
            if Y_true.size and Y_true.min() < 0:
                raise ScoreArgumentError("Y_true holds a negative category")
            keep = np.ascontiguousarray(np.minimum(Y_true, 255), dtype=np.uint8)
            yp, ydev = keep.ctypes.data, 0
        n_thr = int(thr.shape[0])
        bufs = {"hist": np.zeros((self.L, n_thr + 1, 2), np.uint64), "conf": np.zeros((self.L, _lib.SCORE_NCONF), np.uint64),
                "sums": np.zeros((self.L, _lib.SCORE_NSUM), np.float64), "auc": np.full(self.L, np.nan),
                "auc_pairs": np.zeros((self.L, 2), np.uint64)}
        ptrs = [bufs[o].ctypes.data if o in outputs else None for o in SCORE_OUTPUTS]
        rc = self.lib.vmr_score_truth(self._h, yp, ydev, SCORES.index(score), int(bool(skip_diagonal)), n_thr,
                                      thr.ctypes.data if n_thr else None, *ptrs)
        del keep
        self._check(rc, ScoreArgumentError)
        out = {o: (bufs[o].astype(np.int64) if bufs[o].dtype == np.uint64 else bufs[o]) if o in outputs else None for o in SCORE_OUTPUTS}
        out["n_ties"] = np.full(self.L, self.N * self.N - (self.N if skip_diagonal else 0), np.int64)
        out["thresholds"] = thr
        return out

    def reporter_table(self, method="rho_max", threshold=0.0, layer=None, outputs=("counts", "sums")):
        """Each reporter's reports against the current rho, on the device (vmr_reporter_table): one pass over rho plus the
        reports; neither rho nor the support crosses PCIe.  method "rho_max" or "threshold" (`rho_1 >= threshold`), as `readout`.
        Returns {"counts": int64 [L', M, 7], "sums": float64 [L', M, 3]} -- `_lib.RT_COUNT_NAMES`: n_scope, n_rep, total,
        n_inferred, hits, mutual, n_out; `_lib.RT_SUM_NAMES`: exp_ties, exp_hits, exp_total -- what `reporters.ReporterTable`
        takes.  L' = L, or 1 with layer=.  outputs: which of the two to ask for (the other is None).  Bit-identical from run to
        run: the sums are accumulated in fixed point (`reporters.sum_quanta`)."""
        codes = {"rho_max": _lib.READ_RHO_MAX, "rho_mean": _lib.READ_RHO_MEAN, "threshold": _lib.READ_THRESHOLD}
        if method not in codes:
            raise ReporterTableArgumentError("'method' should be one of \"rho_max\", \"threshold\".")
        outputs = tuple(outputs)
        if any(o not in ("counts", "sums") for o in outputs):
            raise ReporterTableArgumentError("outputs: a subset of (\"counts\", \"sums\") expected")
        if layer is not None and not 0 <= int(layer) < self.L:
            raise ReporterTableArgumentError(f"layer {layer} out of range [0, {self.L})")
        Lq = self.L if layer is None else 1
        counts = np.zeros((Lq, self.M, _lib.RT_NCOUNT), np.uint64) if "counts" in outputs else None
        sums = np.zeros((Lq, self.M, _lib.RT_NSUM), np.float64) if "sums" in outputs else None
        rc = self.lib.vmr_reporter_table(self._h, codes[method], float(threshold), self._layer_arg(layer),
                                         None if counts is None else counts.ctypes.data, None if sums is None else sums.ctypes.data)
        self._check(rc, ReporterTableArgumentError)
        return {"counts": None if counts is None else counts.astype(np.int64), "sums": sums}

    def heldout_loglik(self, subs, x, xt=None, theta=None, lam=None, eta=0.0, per_entry=True, device=False):
        """The log predictive density of held-out reports under the current rho, on the device (vmr_heldout_loglik).  subs: the 4
        index arrays (l, i, j, m) of the entries, non-decreasing in l (a list sorted by (l, i, j, m) is the fast case); x: their
        held-out counts (>= 0); xt: the mirrored counts X[l,j,i,m] to condition on (None: 0); NumPy arrays, or int32 CUDA tensors
        (all of them).  theta [L, M], lam [L, K], eta: the caller's tables -- the rate of category k is theta[l,m] lam[l,k] + eta xt.
        This engine's X is not read; its mask only counts the entries that lie inside it.  Returns {"logp": [n], "mean": [n]
        (None without per_entry; torch tensors on the GPU with device=True), "sums": float64 [L, 4] (`_lib.HO_SUM_NAMES`: the sum
        of the finite logp, of (x - mean)^2, of x, of mean), "counts": int64 [L, 4] (`_lib.HO_COUNT_NAMES`: entries, entries
        with x > 0, entries with logp = -inf, entries inside the mask)}.  Bit-identical from run to run."""
        if theta is None or lam is None:
            raise HeldoutArgumentError("theta and lam are needed: the tables the held-out reports are scored under")
        theta, lam = _f64(theta), _f64(lam)
        if theta.shape != (self.L, self.M) or lam.shape != (self.L, self.K):
            raise HeldoutArgumentError(f"theta {theta.shape}, lam {lam.shape}: expected ({self.L}, {self.M}), ({self.L}, {self.K})")
        if len(subs) != 4:
            raise HeldoutArgumentError("subs must be the 4 index arrays (l, i, j, m)")
        cols = list(subs) + [x] + ([] if xt is None else [xt])
        on_dev = _is_torch(x)
        if any(_is_torch(a) != on_dev for a in cols):
            raise HeldoutArgumentError("subs, x and xt must be all NumPy arrays or all GPU tensors")
        if on_dev:
            import torch
            if any(not _is_torch(a) or not a.is_cuda or a.dtype != torch.int32 or not a.is_contiguous() for a in cols):
                raise HeldoutArgumentError("device lists must be contiguous torch.int32 GPU tensors, all of them")
            torch.cuda.synchronize(x.device)
            ptrs = [a.data_ptr() for a in cols]
        else:
            for a in cols:   # (what fits is handed on: the entry point names a subscript out of range or a negative count)
                a = np.asarray(a)
                if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
                    raise HeldoutArgumentError("subscripts and counts travel as 32-bit integers: a value does not fit")
            cols = [np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=np.int32) for a in cols]
            ptrs = [a.ctypes.data for a in cols]
        n = int(cols[0].shape[0])
        if any(int(a.shape[0]) != n or a.ndim != 1 for a in cols):
            raise HeldoutArgumentError("subs, x and xt: 1-D arrays of one length expected")
        if xt is None:
            ptrs.append(None)
        logp = mean = None
        lp_ptr = mn_ptr = None
        if per_entry:
            if device:
                import torch
                dev = torch.device("cuda", self.device)
                logp, mean = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
                torch.cuda.synchronize(dev)
                lp_ptr, mn_ptr = logp.data_ptr(), mean.data_ptr()
            else:
                logp, mean = np.empty(n), np.empty(n)
                lp_ptr, mn_ptr = logp.ctypes.data, mean.ctypes.data
        sums = np.zeros((self.L, _lib.HO_NSUM), np.float64)
        counts = np.zeros((self.L, _lib.HO_NCOUNT), np.uint64)
        rc = self.lib.vmr_heldout_loglik(self._h, n, *ptrs, int(on_dev), theta.ctypes.data, lam.ctypes.data, float(eta), lp_ptr, mn_ptr,
                                         int(bool(device and per_entry)), sums.ctypes.data, counts.ctypes.data)
        del cols
        self._check(rc, HeldoutArgumentError)
        return {"logp": logp, "mean": mean, "sums": sums, "counts": counts.astype(np.int64)}

    def _rs_args(self, theta, lam, eta, threshold, select, layer):
        if theta is None or lam is None:
            raise ReportScoresArgumentError("theta and lam are needed: the tables the reports are scored under")
        theta, lam = _f64(theta), _f64(lam)
        if theta.shape != (self.L, self.M) or lam.shape != (self.L, self.K):
            raise ReportScoresArgumentError(f"theta {theta.shape}, lam {lam.shape}: expected ({self.L}, {self.M}), ({self.L}, {self.K})")
        if isinstance(select, str):
            if select not in RS_SELECT:
                raise ReportScoresArgumentError("select must be \"reports\", \"omissions\" or \"both\"")
            select = RS_SELECT[select]
        if layer is not None and not 0 <= int(layer) < self.L:
            raise ReportScoresArgumentError(f"layer {layer} out of range [0, {self.L})")
        return theta, lam, float(eta), float(threshold), int(select), self._layer_arg(layer)

    def report_scores_size(self, theta, lam, eta, threshold, select="both", layer=None):
        """Rows of `report_scores` for the same arguments (vmr_report_scores_size): the flagged elements."""
        theta, lam, eta, thr, sel, la = self._rs_args(theta, lam, eta, threshold, select, layer)
        n = C.c_uint64()
        self._check(self.lib.vmr_report_scores_size(self._h, la, theta.ctypes.data, lam.ctypes.data, eta, sel, thr, C.byref(n)),
                    ReportScoresArgumentError)
        return int(n.value)

    def report_scores(self, theta, lam, eta, threshold, select="both", layer=None, edges=None, rows=True, by_reporter=True, device=False,
                      out=None):
        """Every element (l, i, j, m) of the support scored under the current rho, on the device (vmr_report_scores): x the
        engine's own count, xt its mirror X[l,j,i,m] (mutuality), logp and mean what `heldout_loglik` gives the entry under
        theta [L, M], lam [L, K], eta; the surprise is -logp.  An element is flagged when its class is in select ("reports": x > 0,
        "omissions": x = 0, "both") and -logp >= threshold (finite, or +inf: only the elements with logp = -inf).  Returns a dict:
        "counts" int64 [L', 4] (`_lib.RS_COUNT_NAMES`: elements, reports, elements with logp = -inf, flagged), "sums" float64
        [L', 4] (`_lib.RS_SUM_NAMES`; sums[:, 0] is the in-sample log predictive density), "hist" int64 [L', n_edges + 1, 2] with
        edges= (finite, non-decreasing, at most `_lib.RS_MAX_EDGES`: hist[l, c, b] counts the elements of ALL the support with
        exactly c edges <= -logp, b = 0 reports, 1 omissions; else None) and "edges", "by_reporter" int64 [L', M, 2] (the flagged
        elements of a reporter by class; None with by_reporter=False), and with rows=True the table, one row per flagged element
        in lexicographic order: "l", "i", "j", "m", "x", "xt" (int32), "logp", "mean" (torch tensors on the GPU with device=True;
        None with rows=False, and then no table pass runs).  L' = L, or 1 with layer=.  out: a dict of preallocated columns (one
        length, the capacity) to fill instead: a capacity below the flagged count is refused before anything is written.
        Bit-identical from run to run."""
        theta, lam, eta, thr, sel, la = self._rs_args(theta, lam, eta, threshold, select, layer)
        Lq = self.L if layer is None else 1
        ed = None
        if edges is not None:
            try:
                ed = np.ascontiguousarray(np.atleast_1d(edges), dtype=np.float64)
            except (TypeError, ValueError) as e:
                raise ReportScoresArgumentError(f"edges: {e}") from None
            if ed.ndim != 1:
                raise ReportScoresArgumentError("edges: a 1-D sequence expected")
        n_edges = 0 if ed is None else int(ed.shape[0])
        hist = None if ed is None else np.zeros((Lq, n_edges + 1, 2), np.uint64)
        sums = np.zeros((Lq, _lib.RS_NSUM), np.float64)
        counts = np.zeros((Lq, _lib.RS_NCOUNT), np.uint64)
        rep = np.zeros((Lq, self.M, 2), np.uint64) if by_reporter else None
        cols, n = {}, 0
        if out is not None:
            cap = {int(a.shape[0]) for a in out.values()}
            if len(cap) != 1:
                raise ValueError("out: arrays of one length expected")
            n, cols = cap.pop(), out
        elif rows:
            n = self.report_scores_size(theta, lam, eta, thr, sel, layer)
            if device:
                import torch
                dev = torch.device("cuda", self.device)
                cols = {c: torch.empty(n, dtype=getattr(torch, np.dtype(t).name), device=dev) for c, t in RS_COLUMNS}
            else:
                cols = {c: np.empty(n, t) for c, t in RS_COLUMNS}
        ptrs = []
        for c, t in RS_COLUMNS:
            a = cols.get(c)
            if a is None:
                ptrs.append(None)
            elif _is_torch(a):
                assert a.is_cuda and a.is_contiguous() and a.element_size() == np.dtype(t).itemsize
                ptrs.append(a.data_ptr())
            else:
                assert a.dtype == np.dtype(t) and a.flags.c_contiguous
                ptrs.append(a.ctypes.data)
        on_dev = any(_is_torch(a) for a in cols.values())
        if on_dev:
            import torch
            torch.cuda.synchronize(torch.device("cuda", self.device))
        rc = self.lib.vmr_report_scores(self._h, la, theta.ctypes.data, lam.ctypes.data, eta, sel, thr, n_edges,
                                        ed.ctypes.data if n_edges else None, None if hist is None else hist.ctypes.data,
                                        sums.ctypes.data, counts.ctypes.data, None if rep is None else rep.ctypes.data,
                                        n if (rows or out is not None) else 0, *ptrs, int(on_dev))
        self._check(rc, ReportScoresArgumentError)
        res = {"counts": counts.astype(np.int64), "sums": sums, "hist": None if hist is None else hist.astype(np.int64), "edges": ed,
               "by_reporter": None if rep is None else rep.astype(np.int64),
               "layers": np.arange(self.L) if layer is None else np.array([int(layer)]), "threshold": thr, "select": sel}
        n_rows = int(res["counts"][:, 3].sum())
        for c, _ in RS_COLUMNS:
            a = cols.get(c)
            res[c] = None if a is None else (a if out is not None else a[:n_rows])
        return res

    def _inf_args(self, e_theta, elog_theta, e_lambda, elog_lambda, g_nu, method, threshold, select, min_tv, layer):
        if any(a is None for a in (e_theta, elog_theta, e_lambda, elog_lambda)):
            raise ReporterInfluenceArgumentError("e_theta, elog_theta, e_lambda and elog_lambda are needed: the tables of the update")
        tabs = [_f64(a) for a in (e_theta, elog_theta, e_lambda, elog_lambda)]
        want = [(self.L, self.M), (self.L, self.M), (self.L, self.K), (self.L, self.K)]
        if any(a.shape != w for a, w in zip(tabs, want)):
            raise ReporterInfluenceArgumentError(f"tables of shapes {[a.shape for a in tabs]}: expected {want}")
        codes = {"rho_max": _lib.READ_RHO_MAX, "rho_mean": _lib.READ_RHO_MEAN, "threshold": _lib.READ_THRESHOLD}
        if isinstance(method, str):
            if method not in codes:
                raise ReporterInfluenceArgumentError("'method' should be one of \"rho_max\", \"threshold\".")
            method = codes[method]
        if isinstance(select, str):
            if select not in INF_SELECT:
                raise ReporterInfluenceArgumentError("select must be \"lost\", \"gained\", \"both\" or \"none\"")
            select = INF_SELECT[select]
        if layer is not None and not 0 <= int(layer) < self.L:
            raise ReporterInfluenceArgumentError(f"layer {layer} out of range [0, {self.L})")
        return tabs, float(g_nu), int(method), float(threshold), int(select), float(min_tv), self._layer_arg(layer)

    def reporter_influence_size(self, e_theta, elog_theta, e_lambda, elog_lambda, g_nu, method="rho_max", threshold=0.0, select="both",
                                min_tv=np.inf, layer=None):
        """Rows of `reporter_influence` for the same arguments (vmr_reporter_influence_size): the flagged elements."""
        tabs, g_nu, code, thr, sel, mtv, la = self._inf_args(e_theta, elog_theta, e_lambda, elog_lambda, g_nu, method, threshold, select,
                                                            min_tv, layer)
        n = C.c_uint64()
        self._check(self.lib.vmr_reporter_influence_size(self._h, la, *[a.ctypes.data for a in tabs], g_nu, code, thr, sel, mtv,
                                                         C.byref(n)), ReporterInfluenceArgumentError)
        return int(n.value)

    def reporter_influence(self, e_theta, elog_theta, e_lambda, elog_lambda, g_nu, method="rho_max", threshold=0.0, select="both",
                           min_tv=np.inf, layer=None, edges=None, rows=True, device=False, out=None, flips=True):
        """The leave-one-reporter-out posterior of every element (l, i, j, m) of the support, on the device
        (vmr_reporter_influence): the tie's row of the current rho with reporter m's factor of the CAVI update divided out, under
        the tables e_theta, elog_theta [L, M] (E[theta], E[log theta]), e_lambda, elog_lambda [L, K] and g_nu = exp(E[log nu]).
        The parameters are held fixed and one factor leaves one tie: an exact refit of that row only when rho is the update's
        fixed point for these tables.  prob = sum_{k>=1} rho_k, prob_loo the same of the leave-one-out row, tv the total variation
        between the two rows; an element is LOST when the readout (method "rho_max", or "threshold": rho_1 >= threshold) infers
        the tie and the leave-one-out row does not, GAINED the other way round; it is flagged when it is lost and select holds
        "lost", gained and select holds "gained" ("both", "none"), or tv >= min_tv (+inf: flips only).  Returns a dict: "counts"
        int64 [L', M, 4] (`_lib.INF_COUNT_NAMES`: n_scope, lost, gained, flagged), "sums" float64 [L', M, 2]
        (`_lib.INF_SUM_NAMES`: sum tv, sum prob_loo - prob; fixed point, `influence.sum_quantum`), "hist" int64 [L', n_edges + 1, 2]
        with edges= (exactly c edges <= tv; class 0: x > 0, 1: x = 0; else None) and "edges", and with rows=True the table, one
        row per flagged element in lexicographic order: "l", "i", "j", "m", "x", "xt" (int32), "prob", "prob_loo", "tv" (torch
        tensors on the GPU with device=True; None with rows=False, and then no table pass runs) and, with flips=True and host
        rows, the boolean marks "lost" and "gained" of every row (two more calls that fetch the flips' subscripts alone, made only
        where a flip exists).  L' = L, or 1 with layer=.  out: a dict of preallocated columns (one length, the capacity) to fill
        instead: a capacity below the flagged count is refused before anything is written.  Bit-identical from run to run."""
        tabs, g_nu, code, thr, sel, mtv, la = self._inf_args(e_theta, elog_theta, e_lambda, elog_lambda, g_nu, method, threshold, select,
                                                            min_tv, layer)
        tp = [a.ctypes.data for a in tabs]
        Lq = self.L if layer is None else 1
        ed = None
        if edges is not None:
            try:
                ed = np.ascontiguousarray(np.atleast_1d(edges), dtype=np.float64)
            except (TypeError, ValueError) as e:
                raise ReporterInfluenceArgumentError(f"edges: {e}") from None
            if ed.ndim != 1:
                raise ReporterInfluenceArgumentError("edges: a 1-D sequence expected")
        n_edges = 0 if ed is None else int(ed.shape[0])
        hist = None if ed is None else np.zeros((Lq, n_edges + 1, 2), np.uint64)
        counts = np.zeros((Lq, self.M, _lib.INF_NCOUNT), np.uint64)
        sums = np.zeros((Lq, self.M, _lib.INF_NSUM), np.float64)
        cols, n = {}, 0
        if out is not None:
            cap = {int(a.shape[0]) for a in out.values()}
            if len(cap) != 1:
                raise ValueError("out: arrays of one length expected")
            n, cols = cap.pop(), out
        elif rows:
            n = self.reporter_influence_size(*tabs, g_nu, code, thr, sel, mtv, layer)
            if device:
                import torch
                dev = torch.device("cuda", self.device)
                cols = {c: torch.empty(n, dtype=getattr(torch, np.dtype(t).name), device=dev) for c, t in INF_COLUMNS}
            else:
                cols = {c: np.empty(n, t) for c, t in INF_COLUMNS}
        ptrs = []
        for c, t in INF_COLUMNS:
            a = cols.get(c)
            if a is None:
                ptrs.append(None)
            elif _is_torch(a):
                assert a.is_cuda and a.is_contiguous() and a.element_size() == np.dtype(t).itemsize
                ptrs.append(a.data_ptr())
            else:
                assert a.dtype == np.dtype(t) and a.flags.c_contiguous
                ptrs.append(a.ctypes.data)
        on_dev = any(_is_torch(a) for a in cols.values())
        if on_dev:
            import torch
            torch.cuda.synchronize(torch.device("cuda", self.device))
        rc = self.lib.vmr_reporter_influence(self._h, la, *tp, g_nu, code, thr, sel, mtv, n_edges, ed.ctypes.data if n_edges else None,
                                             None if hist is None else hist.ctypes.data, counts.ctypes.data, sums.ctypes.data,
                                             n if (rows or out is not None) else 0, *ptrs, int(on_dev))
        self._check(rc, ReporterInfluenceArgumentError)
        res = {"counts": counts.astype(np.int64), "sums": sums, "hist": None if hist is None else hist.astype(np.int64), "edges": ed,
               "layers": np.arange(self.L) if layer is None else np.array([int(layer)]), "method": code, "threshold": thr,
               "select": sel, "min_tv": mtv}
        n_rows = int(res["counts"][:, :, 3].sum())
        for c, _ in INF_COLUMNS:
            a = cols.get(c)
            res[c] = None if a is None else (a if out is not None else a[:n_rows])
        if flips and rows and out is None and not on_dev:
            # which rows are flips: the subscripts of the lost (gained) elements alone, looked up among the rows
            shape = (self.L, self.N, self.N, self.M)
            key = np.ravel_multi_index(tuple(res[c].astype(np.int64) for c in "lijm"), shape) if n_rows else np.zeros(0, np.int64)
            for name, bit, col in (("lost", _lib.INF_LOST, 1), ("gained", _lib.INF_GAINED, 2)):
                mark = np.zeros(n_rows, bool)
                nf = int(res["counts"][:, :, col].sum())
                if nf and n_rows:
                    sub = {c: np.empty(nf, np.int32) for c in "lijm"}
                    p4 = [sub[c].ctypes.data for c in "lijm"] + [None] * 5
                    self._check(self.lib.vmr_reporter_influence(self._h, la, *tp, g_nu, code, thr, bit, np.inf, 0, None, None, None,
                                                                None, nf, *p4, 0), ReporterInfluenceArgumentError)
                    mark = np.isin(key, np.ravel_multi_index(tuple(sub[c].astype(np.int64) for c in "lijm"), shape))
                res[name] = mark
        return res

    def snapshot(self):
        """Keep the current posteriors on the device (`_update_optimal_parameters`, reference model.py:925-942)."""
        self._check(self.lib.vmr_snapshot(self._h))

    def restore(self):
        """Make the snapshot the current state again."""
        self._check(self.lib.vmr_restore(self._h))

    def get_state(self, rho=True, rho_out=None):
        """Posteriors as NumPy arrays; rho_out: a C-contiguous float64 buffer to receive rho (e.g. pinned memory)."""
        out = {
            "gamma_shp": np.empty((self.L, self.M)), "gamma_rte": np.empty((self.L, self.M)),
            "phi_shp": np.empty((self.L, self.K)), "phi_rte": np.empty((self.L, self.K)),
        }
        ns, nr = C.c_double(), C.c_double()
        r = None
        if rho:
            r = rho_out if rho_out is not None else np.empty((self.L, self.N, self.N, self.K))
            assert r.dtype == np.float64 and r.flags.c_contiguous and r.size == self.L * self.N * self.N * self.K
            r = r.reshape(self.L, self.N, self.N, self.K)
        self._check(self.lib.vmr_get_state(
            self._h, out["gamma_shp"].ctypes.data, out["gamma_rte"].ctypes.data, out["phi_shp"].ctypes.data,
            out["phi_rte"].ctypes.data, C.addressof(ns), C.addressof(nr), r.ctypes.data if rho else None))
        out["nu_shp"], out["nu_rte"] = ns.value, nr.value
        if rho:
            out["rho"] = r
        return out

    def get_geometric(self):
        gt, gl, gn, gc = np.empty((self.L, self.M)), np.empty((self.L, self.K)), C.c_double(), C.c_double()
        self._check(self.lib.vmr_get_geometric(self._h, gt.ctypes.data, gl.ctypes.data, C.addressof(gn),
                                               C.addressof(gc)))
        return gt, gl, gn.value, gc.value

    def data_format(self):
        """("sparse" | "dense", non-zero counts in X): the layout vmr_create chose for this dataset."""
        sp, nnz = C.c_int(), C.c_uint64()
        self._check(self.lib.vmr_data_format(self._h, C.byref(sp), C.byref(nnz)))
        return ("sparse" if sp.value else "dense"), int(nnz.value)

    def mask_format(self):
        """("lists" | "words", listed reporters): whether partial mask rows are also held as short reporter lists."""
        li, n = C.c_int(), C.c_uint64()
        self._check(self.lib.vmr_mask_format(self._h, C.byref(li), C.byref(n)))
        return ("lists" if li.value else "words"), int(n.value)

    def sweep_shape(self):
        """(passes over the entries per sweep, mirror-count levels of the statistics kept in LDS, reports in the far lists): the
        shape vmr_create chose for a sweep of this dataset (vmr_sweep_shape)."""
        p, lv, n = C.c_int(), C.c_int(), C.c_uint64()
        self._check(self.lib.vmr_sweep_shape(self._h, C.byref(p), C.byref(lv), C.byref(n)))
        return int(p.value), int(lv.value), int(n.value)

    # -- measurement
    def profile(self, enable=True):
        """HIP events around the engine's kernels; enable=2: only around the passes over the data (not the finalize kernels)."""
        self._check(self.lib.vmr_profile(self._h, int(enable)))

    def profile_read(self):
        out = {}
        for i, name in enumerate(_lib.KERNEL_NAMES):
            ms, n, b = C.c_double(), C.c_int64(), C.c_double()
            self._check(self.lib.vmr_profile_read(self._h, i, C.byref(ms), C.byref(n)))
            self._check(self.lib.vmr_kernel_bytes(self._h, i, C.byref(b)))
            out[name] = {"ms": ms.value, "launches": n.value, "bytes_per_launch": b.value}
        return out
