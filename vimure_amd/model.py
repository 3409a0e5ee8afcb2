"""Host side of the estimator: the reference's `VimureModel` API over the HIP engine.

Mirrors latentnetworks/vimure `src/python/vimure/model.py`: constructor (:39-71), `fit`
(:327-448) with the same keyword set, warnings and error messages (:79-325), the
RandomState draw order of `_set_rho_prior` / `_initialize_priors` (:458-605) so fixed-seed
fits start from the reference's state, the ELBO stop rule (:1021-1056), best-realisation
selection (:428-437, :925-942) and the read-out methods (:1062-1214).

What does NOT happen here: any CAVI arithmetic.  The sweeps and the ELBO run in
libvimure_hip.so (`vimure_amd.engine.CaviEngine`); without it `fit` raises.
"""
import contextlib
import time
import warnings

import numpy as np
import pandas as pd
import scipy.special as sp
from scipy.stats import poisson

from ._log import setup_logging
from .engine import CaviEngine, host_buffer
from .tensor import M_COO_NARROW, SparseTensor, engine_data, is_sparse_like, to_dense_u8

try:  # the reference is an sklearn estimator (model.py:28); keep that surface when sklearn is there
    from sklearn.base import BaseEstimator, TransformerMixin
except Exception:  # pragma: no cover
    class BaseEstimator:  # type: ignore
        pass

    class TransformerMixin:  # type: ignore
        pass

INF = 1e10
DEFAULT_EPS = 1e-12
DEFAULT_BIAS0 = 0.0
DEFAULT_MAX_ITER = 500
DEFAULT_NUM_REALISATIONS = 1

_EXTRA = ["R", "EPS", "K", "bias0", "max_iter", "alpha_lambda", "beta_lambda", "alpha_teta", "beta_teta",
          "num_realisations"]  # the reference's whitelist, typos included (model.py:90-101)
_OURS = ["device", "alpha_theta", "beta_theta", "engine", "keep_engine", "init_on_device"]


def _is_torch(x):
    return type(x).__module__.startswith("torch")


class VimureModel(TransformerMixin, BaseEstimator):
    """ViMuRe: latent network Y (rho), reporter reliabilities (theta), tie-strength rates
    (lambda) and mutuality (eta), by coordinate-ascent variational inference on an MI355X."""

    def __init__(self, undirected: bool = False, mutuality: bool = True, convergence_tol: float = 0.1,
                 decision: int = 1, verbose: bool = False):
        self.undirected = undirected
        if undirected:
            warnings.warn("Overriding mutuality to False because the network is undirected")
            self.mutuality = False
        else:
            self.mutuality = mutuality
        self.convergence_tol = convergence_tol
        self.decision = decision
        self.verbose = verbose
        self.logger = setup_logging("vm.model.VimureModel", verbose)

    # ------------------------------------------------------------------ parameters (model.py:79-325)
    def _check_fit_params(self, X, lambda_prior, theta_prior, eta_prior, rho_prior, seed, **extra):
        for p in extra:
            if p not in _EXTRA and p not in _OURS:
                self.logger.warning("Ignoring unrecognised parameter %s." % p)

        if isinstance(X, pd.DataFrame) or type(X).__name__ == "Graph":
            from ._io import read_from_edgelist, read_from_igraph
            net = read_from_edgelist(X) if isinstance(X, pd.DataFrame) else read_from_igraph(X)
            X = net.X
            self.nodeNames, self.layerNames = net.nodeNames, net.layerNames
            self.R = net.R
            if extra.get("K") is None:
                self.K = net.K

        dev_tensor = _is_torch(X)
        # a coordinate container (the reference's sptensor surface: subs / vals / shape) goes to the device as it is
        # (vmr_create_coo) when the report lists can hold it; no dense [L,N,N,M] array is built then
        # (and so does a dense array whose counts pass 255: the engine takes any count the reference's int64 holds, below 2^31)
        coo = False
        if dev_tensor or (extra.get("engine") is not None and is_sparse_like(X)):
            Xd = X   # (with `engine` the data is on the device already: only the shape is needed)
            shape = tuple(int(s) for s in X.shape)
        else:
            Xd = engine_data(X, "X") if extra.get("engine") is None else to_dense_u8(X, "X")
            if self.undirected and is_sparse_like(Xd) and int(Xd.shape[3]) <= M_COO_NARROW and (len(Xd.vals) == 0 or np.max(Xd.vals) <= 255):
                Xd = to_dense_u8(Xd, "X")   # (the symmetry check below reads the array)
            coo = is_sparse_like(Xd)
            shape = tuple(int(s) for s in Xd.shape)
        if len(shape) != 4 or shape[1] != shape[2]:
            raise ValueError("X must have shape (L, N, N, M)")
        self.L, self.N, self.M = shape[0], shape[1], shape[3]

        if self.undirected:
            if coo:   # counts beyond a byte: compare the coordinate lists with their (i, j)-swapped selves
                sl, si, sj, sm = (np.asarray(a, dtype=np.int64) for a in Xd.subs)
                v = np.asarray(Xd.vals)
                ka = np.ravel_multi_index((sl, si, sj, sm), shape)
                kb = np.ravel_multi_index((sl, sj, si, sm), shape)
                oa, ob = np.argsort(ka), np.argsort(kb)
                sym = bool(np.array_equal(ka[oa], kb[ob]) and np.array_equal(v[oa], v[ob]))
            else:
                sym = bool((Xd == Xd.transpose(1, 2)).all()) if dev_tensor else np.array_equal(Xd, Xd.transpose(0, 2, 1, 3))
            if not sym:
                msg = "If undirected is True, the given network has to be symmetric wrt l and m!"
                self.logger.error(msg)
                raise ValueError(msg)

        if not hasattr(self, "K"):
            if extra.get("K") is not None:
                self.K = int(extra["K"])
            else:
                self.K = (int(np.max(Xd.vals)) if is_sparse_like(Xd) else int(Xd.max())) + 1
                warnings.warn(f"Parameter K was None. Defaulting to: {self.K}", UserWarning)

        if not hasattr(self, "R"):
            if "R" in extra and extra["R"] is not None:
                R = extra["R"]
                if tuple(int(s) for s in R.shape) != (self.L, self.N, self.N, self.M):
                    msg = "Dimensions of reporter mask (R) do not match L x N x N x M"
                    self.logger.error(msg)
                    raise ValueError(msg)
                self.R = R
            else:
                msg = "Reporters Mask was not informed (parameter R). "
                msg += "The model will assume that every reporter can report on any tie."
                warnings.warn(msg, UserWarning)
                self.R = None  # the engine treats NULL as all ones; no [L,N,N,M] float64 array is built
        Rd = self.R
        if extra.get("engine") is not None:
            Rd = None   # the engine already holds X and R on the device: no pass over the host copies
        elif coo and (Rd is None or is_sparse_like(Rd)):
            pass        # coordinate lists: handed to the engine as they are
        elif coo:       # X as lists, R dense: the lists of its non-zeros
            Rd = SparseTensor.fromarray(np.asarray(Rd) != 0)
        elif Rd is not None and not _is_torch(Rd):
            Rd = to_dense_u8(Rd, "R")
            if Rd.dtype != np.uint8 or Rd.max(initial=0) > 1:
                Rd = (Rd != 0).astype(np.uint8)

        self.EPS = float(extra["EPS"]) if "EPS" in extra else DEFAULT_EPS
        self.bias0 = float(extra["bias0"]) if "bias0" in extra else DEFAULT_BIAS0
        self.max_iter = int(extra["max_iter"]) if "max_iter" in extra else DEFAULT_MAX_ITER
        self.num_realisations = int(extra["num_realisations"]) if "num_realisations" in extra else DEFAULT_NUM_REALISATIONS

        if "alpha_theta" in extra or "beta_theta" in extra:
            self.alpha_theta, self.beta_theta = extra["alpha_theta"], extra["beta_theta"]
            if np.shape(self.alpha_theta) != (self.L, self.M):
                msg = "alpha_theta matrix is not valid. When using this parameter, make sure to inform a %d x %d matrix."
                self.logger.error(msg)
                raise ValueError(msg % (self.L, self.M))
            if np.shape(self.beta_theta) != (self.L, self.M):
                msg = "beta_theta matrix is not valid. When using this parameter, make sure to inform a %d x %d matrix."
                self.logger.error(msg)
                raise ValueError(msg % (self.L, self.M))
        else:
            if type(theta_prior) is not tuple or len(theta_prior) != 2:
                msg = "theta_prior must be a 2D tuple!"
                self.logger.error(msg)
                raise ValueError(msg)
            self.alpha_theta, self.beta_theta = theta_prior

        if "alpha_lambda" in extra or "beta_lambda" in extra:
            self.alpha_lambda, self.beta_lambda = extra["alpha_lambda"], extra["beta_lambda"]
            for nm, arr in (("alpha_lambda", self.alpha_lambda), ("beta_lambda", self.beta_lambda)):
                if np.shape(arr) != (self.L, self.K):
                    sh = np.shape(arr)
                    msg = f"{nm} matrix is not valid (dimensions = %d x %d)."
                    msg += "When using this parameter, make sure to pass a %d x %d matrix."
                    msg = msg % (sh[0] if len(sh) > 0 else 0, sh[1] if len(sh) > 1 else 0, self.L, self.K)
                    self.logger.error(msg)
                    raise ValueError(msg)
        else:
            if type(lambda_prior) is not tuple or len(lambda_prior) != 2:
                msg = "lambda_prior must be a 2D tuple!"
                self.logger.error(msg)
                raise ValueError(msg)
            self.alpha_lambda, self.beta_lambda = lambda_prior

        if type(eta_prior) is not tuple or len(eta_prior) != 2:
            msg = "eta_prior must be a 2D tuple!"
            self.logger.error(msg)
            raise ValueError(msg)
        self.alpha_mutuality, self.beta_mutuality = eta_prior

        if rho_prior is not None and np.shape(rho_prior) != (self.L, self.N, self.N):
            msg = "rho_prior has to have shape equal to (L, N, N)!"
            self.logger.error(msg)
            raise ValueError(msg)
        self.rho_prior = rho_prior
        self._change_seed(seed)
        return Xd, Rd

    def _change_seed(self, seed):
        self.seed = seed
        self.prng = np.random.RandomState(seed)

    # ------------------------------------------------------------------ initial state (model.py:458-605)
    def _draw_pr_rho(self, coverage, bias0, prng=None, out=None):
        """`_set_rho_prior` (model.py:458-559).  The common case (no informative prior, directed network) runs as one C
        pass that is bit-identical to the NumPy statements below (vimure_amd/csrc/host_init.c), into `out` if given."""
        prng = self.prng if prng is None else prng
        L, N, K = self.L, self.N, self.K
        if self.rho_prior is None and not self.undirected:
            from . import _hostlib
            pr = _hostlib.draw_pr_rho(prng, (L, N, N, K), bias0, coverage, out=out)
            if pr is not None:
                return pr
        if self.rho_prior is None:
            pr = 1.0 + 0.01 * prng.rand(L, N, N, K)
            pr[..., 0] += bias0
            if self.undirected:
                pr = (pr + pr.transpose(0, 2, 1, 3)) / 2.0
            pr /= pr.sum(axis=-1)[..., None]
        else:
            pr = np.zeros((L, N, N, K))
            sub = np.nonzero(self.rho_prior)
            n = sub[0].shape[0]
            for k in range(K):
                pr[sub + (np.full(n, k),)] = poisson.pmf(k, self.rho_prior[sub]) + 1.0 * prng.rand(n)
            if self.undirected:
                pr = (pr + pr.transpose(0, 2, 1, 3)) / 2.0
            pr[sub] /= pr[sub].sum(axis=-1)[:, None]
        onehot = np.zeros(K)
        onehot[0] = 1.0
        pr[coverage == 0] = onehot  # ties no reporter covers / nobody reported (model.py:508-556)
        if out is not None:
            out[...] = pr
            return out
        return pr

    def _device_draw_possible(self):
        """`fit(init_on_device=True)` draws on the GPU: no informative prior (scipy's Poisson pmf has no bit-exact device
        counterpart), an MT19937 generator and the host helper that walks it."""
        from . import _hostlib
        return self.rho_prior is None and self.prng.get_state()[0] == "MT19937" and _hostlib.load() is not None

    def _draw_gammas(self, sumX, prng=None):
        """`_initialize_priors` (model.py:561-605): the draws that follow the rho prior, in the reference's order."""
        prng = self.prng if prng is None else prng
        L, M, K = self.L, self.M, self.K
        st = {}
        st["gamma_shp"] = self.alpha_theta * prng.random_sample(size=(L, M)) + self.alpha_theta
        st["phi_shp"] = self.alpha_lambda * prng.random_sample(size=(L, K)) + self.alpha_lambda
        st["gamma_rte"] = self.beta_theta * prng.random_sample(size=(L, M)) + self.beta_theta
        st["phi_rte"] = self.beta_lambda * prng.random_sample(size=(L, K)) + self.beta_lambda
        if self.mutuality:
            st["nu_shp"] = self.alpha_mutuality * prng.random_sample(1)[0] + self.alpha_mutuality
            st["nu_rte"] = self.beta_mutuality + sumX  # fixed once and for all (model.py:593-595)
        else:
            st["nu_shp"], st["nu_rte"] = 0.000001, 1.0
        if prng is self.prng:
            for k, v in st.items():
                setattr(self, k, v)
        return st

    def _staging_index(self, eng, r):
        """Which pinned staging buffer realisation r is drawn into: with upload-ahead (see fit) buffer 1 is free again as soon as
        its copy to the device is done, so two buffers serve any number of realisations; otherwise three in rotation."""
        if self.num_realisations > 1 and getattr(eng, "can_upload_ahead", lambda: False)():
            return 0 if r == 0 else 1
        return r % 3

    def _initial_states(self, eng, coverage, on_device=False):
        """Initial state of every realisation, in order: (r, seed of r, state dict incl. pr_rho, seed after r).  CAVI
        consumes no randomness (reference model.py:386-437), so the whole seed chain is a function of the first seed
        and realisation r + 1 can be drawn while r runs on the GPU.  pr_rho lands in the engine's staging buffers
        (three in rotation: one being uploaded, one queued, one being drawn).  on_device: the generator is only walked
        (`_hostlib.mt_block_states`); pr_rho is None and the state holds the block descriptors of the device draw
        ("pr_rho_blocks", with its "bias0"), which `CaviEngine.draw_pr_rho` turns into the same prior."""
        from . import _hostlib
        seed, prng = self.seed, self.prng
        for r in range(self.num_realisations):
            bias = DEFAULT_BIAS0 if r < 5 else (r - 4) * self.bias0
            if on_device:
                blocks = _hostlib.mt_block_states(prng, self.L, self.N, self.K)
                pr = None
            else:
                pr = self._draw_pr_rho(coverage, bias, prng=prng, out=eng.staging(self._staging_index(eng, r)))
            st = self._draw_gammas(self.sumX, prng=prng)
            st["pr_rho"] = pr
            if on_device:
                st["pr_rho_blocks"], st["bias0"] = blocks, bias
            step = prng.randint(1, 500)
            nxt = step if seed is None else seed + step
            yield r, seed, st, nxt
            seed, prng = nxt, np.random.RandomState(nxt)

    # ------------------------------------------------------------------ fit (model.py:327-448)
    def fit(self, X, theta_prior=(0.1, 0.1), lambda_prior=(10.0, 10.0), eta_prior=(0.5, 1.0), rho_prior=None,
            seed: int = None, **extra_params):
        """Same contract as the reference's `fit`; extra keywords: `device` picks the GPU (default 0, or the
        device of a torch tensor X); `engine` reuses a `CaviEngine` already holding this X, R, K (many seeds
        of one dataset: the data is uploaded once, see vimure_amd/batch.py); `keep_engine=True` leaves the posteriors on
        the GPU after the fit: `get_inferred_model` / `predict` then run there (vmr_readout) and `rho_f` is only copied
        to the host if something asks for it (`close()` frees the device memory).  `init_on_device=True` draws the initial rho
        prior of every realisation on the GPU (vmr_draw_pr_rho), bit for bit the host draw: the host only walks the generator
        and no L N^2 K array is built or uploaded.  An informative `rho_prior` keeps the host draw; `pr_rho_drawn_on` says
        which one ran ("device" or "host").

        Host work per realisation is the RandomState draw of the initial state (bit-exact with the reference); with
        several realisations the next draw runs on a host thread while the GPU sweeps, the best realisation is kept on
        the device (vmr_snapshot) and rho crosses PCIe once, at the end.  `rho` (without `_f`) holds the best
        realisation too (the reference leaves the last one there; nothing reads it after `fit`)."""
        Xd, Rd = self._check_fit_params(X, lambda_prior, theta_prior, eta_prior, rho_prior, seed, **extra_params)
        self.close()   # a device state kept by an earlier fit(keep_engine=True)
        self._engine, self._rho_f = None, None
        eng = extra_params.get("engine")
        own_engine = eng is None
        keep = bool(extra_params.get("keep_engine", False)) and own_engine
        if own_engine and is_sparse_like(Xd):
            eng = CaviEngine.from_coo(Xd.subs, Xd.vals, (self.L, self.N, self.N, self.M), R=None if Rd is None else Rd.subs,
                                      K=self.K, mutuality=self.mutuality, eps=self.EPS, device=extra_params.get("device"))
        elif own_engine:
            eng = CaviEngine(Xd, Rd, K=self.K, mutuality=self.mutuality, eps=self.EPS, device=extra_params.get("device"))
        elif (eng.L, eng.N, eng.M, eng.K, eng.mutuality) != (self.L, self.N, self.M, self.K, bool(self.mutuality)):
            raise ValueError("engine does not match the shape / K / mutuality of this fit")
        producer = None
        try:
            self.sumX, coverage = eng.data_stats()
            eng.set_priors(self.alpha_theta, self.beta_theta, self.alpha_lambda, self.beta_lambda,
                           self.alpha_mutuality, self.beta_mutuality)
            maxL, trace, best = -INF, [], None
            self.loop_seconds = 0.0   # wall time inside the CAVI loops of all realisations (device work included)
            self.draw_seconds = 0.0   # host time the loops waited for an initial state (with init_on_device: its GPU draw too)
            on_dev = bool(extra_params.get("init_on_device", False)) and self._device_draw_possible()
            self.pr_rho_drawn_on = "device" if on_dev else "host"
            states = self._initial_states(eng, coverage, on_device=on_dev)
            if self.num_realisations > 1:   # draw realisation r + 1 while r runs
                import queue
                import threading
                q = queue.Queue(maxsize=1)   # one finished state waits while the next is drawn (three staging buffers)
                stop = threading.Event()     # set on any exit from fit(): the producer draws nothing further
                # upload-ahead keeps two device slots in rotation: slot r % 2 may only be overwritten once set_state(r) has
                # consumed it (set_state synchronises the engine's stream before it returns)
                slot_free = [threading.Event(), threading.Event()]
                for ev in slot_free:
                    ev.set()

                def put(item):
                    while not stop.is_set():
                        try:
                            q.put(item, timeout=0.1)
                            return True
                        except queue.Full:
                            continue
                    return False

                def work():
                    try:
                        for item in states:
                            if stop.is_set():
                                return
                            r_ = item[0]
                            pr_ = item[2]["pr_rho"]
                            if pr_ is not None:   # (a host draw; the device draw runs in the consumer, from the block states)
                                si = self._staging_index(eng, r_)
                                if r_ > 0 and getattr(eng, "can_upload_ahead", lambda: False)() and isinstance(pr_, np.ndarray) and np.shares_memory(pr_, eng.staging(si)):
                                    slot = r_ % 2
                                    while not slot_free[slot].wait(timeout=0.1):
                                        if stop.is_set():
                                            return
                                    slot_free[slot].clear()
                                    dev = eng.upload_ahead(si, slot)   # (realisation 0 is waited for: nothing to hide its upload behind)
                                    if dev is not None:
                                        item[2]["pr_rho"] = dev
                                        item[2]["_slot"] = slot
                                    else:
                                        slot_free[slot].set()
                            if not put(item):
                                return
                        put(None)
                    except BaseException as e:   # surfaces in the consumer
                        put(e)
                producer = threading.Thread(target=work, daemon=True)
                producer.start()

                def next_state():
                    item = q.get()
                    if isinstance(item, BaseException):
                        raise item
                    return item
            else:
                def next_state():
                    return next(states, None)
            final_seed = self.seed
            while True:
                t_draw = time.perf_counter()
                item = next_state()
                if item is not None and item[2]["pr_rho"] is None:   # init_on_device: the prior of the block states, on the GPU
                    item[2]["pr_rho"] = eng.draw_pr_rho(item[2]["pr_rho_blocks"], item[2]["bias0"], self.undirected)
                self.draw_seconds += time.perf_counter() - t_draw
                if item is None:
                    break
                r, seed_r, st, final_seed = item
                eng.set_state(st["gamma_shp"], st["gamma_rte"], st["phi_shp"], st["phi_rte"], st["nu_shp"], st["nu_rte"],
                              st["pr_rho"])   # (synchronises: the staging buffer is free again)
                if "_slot" in st:   # the device slot of upload_ahead has been read: the producer may reuse it
                    slot_free[st["_slot"]].set()
                t_loop = time.perf_counter()
                if not self.verbose:   # the whole loop on the engine's side (vmr_fit_loop): one call per realisation
                    rows, elbo, _, _ = eng.fit_loop(self.max_iter, self.convergence_tol, self.decision)
                    trace.extend((r, seed_r, it_, e_, rt_, rc_) for it_, e_, rt_, rc_ in rows)
                else:
                    elbo = self._loop_verbose(eng, r, seed_r, trace)
                eng.sync()
                self.loop_seconds += time.perf_counter() - t_loop
                self._pull_params(eng)   # the small arrays of this realisation (rho stays on the device)
                if maxL < elbo:
                    maxL, best = elbo, self._params_copy()
                    if self.num_realisations > 1:
                        eng.snapshot()
            if best is not None:
                if self.num_realisations > 1:
                    eng.restore()
                self._update_optimal_parameters(best, eng, lazy_rho=keep)
            self._change_seed(final_seed)
            if keep:
                self._engine, own_engine = eng, False
        finally:
            if producer is not None:   # stop the producer and wait for it BEFORE the engine (and its staging buffers) go away
                stop.set()
                while producer.is_alive():
                    try:
                        q.get(timeout=0.05)
                    except queue.Empty:
                        pass
                producer.join()
            if own_engine:
                eng.close()
        cols = ["realisation", "seed", "iter", "elbo", "runtime", "reached_convergence"]
        self.trace = pd.DataFrame(trace, columns=cols)
        self.maxL = maxL
        return self

    def _loop_verbose(self, eng, r, seed_r, trace):
        """The reference's while-loop (model.py:405-426) step by step, with its DEBUG line per ELBO evaluation."""
        coincide, it, reached, elbo = 0, 1, False, -INF
        while not reached and it <= self.max_iter:
            nxt = it if (it == 1 or it % 10 == 0 or it == self.max_iter) else min(self.max_iter, (it // 10 + 1) * 10)
            if nxt > it:
                eng.step(nxt - it)
                it = nxt
                eng.sync()
            t0 = time.time()
            old, elbo = elbo, eng.step(1, want_elbo=True)
            runtime = time.time() - t0
            coincide = coincide + 1 if abs(elbo - old) < self.convergence_tol else 0
            if coincide > self.decision:
                reached = True
            self.logger.debug(f"Realisation {r:2} | Iter {it:4} | ELBO value: {elbo:6.12f} | Reached convergence: {reached}")
            it += 1
            if (it - 1) % 10 == 0:
                trace.append((r, seed_r, it - 1, elbo, runtime, reached))
        return elbo

    _SMALL = ("gamma_shp", "gamma_rte", "phi_shp", "phi_rte", "nu_shp", "nu_rte")

    def _pull_params(self, eng):
        st = eng.get_state(rho=False)
        self.gamma_shp, self.gamma_rte = st["gamma_shp"], st["gamma_rte"]
        self.phi_shp, self.phi_rte = st["phi_shp"], st["phi_rte"]
        self.nu_shp, self.nu_rte = np.float64(st["nu_shp"]), np.float64(st["nu_rte"])
        self.G_exp_theta = np.exp(sp.psi(self.gamma_shp) - np.log(self.gamma_rte))
        self.G_exp_lambda = np.exp(sp.psi(self.phi_shp) - np.log(self.phi_rte))
        # what the last cache refresh held, i.e. computed before the last nu update (model.py:684 vs :822)
        self.G_exp_nu = np.float64(eng.get_geometric()[3]) if self.mutuality else 0.0

    def _params_copy(self):
        return {k: np.copy(getattr(self, k)) for k in self._SMALL}

    def _update_optimal_parameters(self, best, eng, lazy_rho=False):
        """model.py:925-942; rho of the best realisation is the engine's current state here (vmr_restore)."""
        self.gamma_shp_f, self.gamma_rte_f = best["gamma_shp"], best["gamma_rte"]
        self.phi_shp_f, self.phi_rte_f = best["phi_shp"], best["phi_rte"]
        self.nu_shp_f, self.nu_rte_f = best["nu_shp"], best["nu_rte"]
        self._rho_f = None
        if not lazy_rho:
            self._fetch_rho(eng)
        self.G_exp_theta_f = np.exp(sp.psi(self.gamma_shp_f) - np.log(self.gamma_rte_f))
        self.G_exp_lambda_f = np.exp(sp.psi(self.phi_shp_f) - np.log(self.phi_rte_f))
        self.G_exp_nu_f = np.exp(sp.psi(self.nu_shp_f) - np.log(self.nu_rte_f))

    # rho_f / rho: on the host once fetched; with fit(keep_engine=True) still on the GPU until something reads them
    def _fetch_rho(self, eng):
        buf, keepalive = host_buffer(self.L * self.N * self.N * self.K)
        self._rho_f = eng.get_state(rho=True, rho_out=buf)["rho"]
        self._rho_keepalive = keepalive   # page-locked memory behind rho_f, when it is
        return self._rho_f

    @property
    def rho_f(self):
        if getattr(self, "_rho_f", None) is None:
            eng = getattr(self, "_engine", None)
            if eng is None:
                raise AttributeError("rho_f: the model has not been fitted")
            self._fetch_rho(eng)
        return self._rho_f

    @rho_f.setter
    def rho_f(self, value):
        self._rho_f = value

    @property
    def rho(self):
        return self.rho_f

    def close(self):
        """Free the device state kept by fit(keep_engine=True); rho_f is fetched first if nothing has read it yet."""
        eng = getattr(self, "_engine", None)
        if eng is not None:
            if getattr(self, "_rho_f", None) is None:
                self._fetch_rho(eng)
            eng.close()
            self._engine = None

    def __del__(self):
        eng = getattr(self, "_engine", None)
        if eng is not None:
            try:
                eng.close()
            except Exception:
                pass

    # ------------------------------------------------------------------ read-out (model.py:1062-1214)
    def sample_inferred_model(self, N=1, seed=None, device=False):
        """Reference model.py:1062-1096: N samples of Y, sample i = `default_rng(seed + i).multinomial(N, rho_f).argmax(-1)`.
        device=True (after `fit(keep_engine=True)`): the same draw on the GPU from the rho kept there (vmr_sample) -- per tie
        the most frequent category of N categorical trials, a Philox stream keyed by seed + i instead of NumPy's PCG64 (same
        distribution, reproducible for a seed, different numbers) -- so rho (8 L N^2 K bytes) never crosses PCIe."""
        if seed is None:
            seed = self.seed
        if device:
            eng = getattr(self, "_engine", None)
            if eng is None:
                raise ValueError("device=True needs the posteriors on the GPU: fit(..., keep_engine=True)")
            return [eng.sample(seed + i, n_trials=N).astype(np.int64) for i in range(N)]

        def sample_y(s):
            g = np.random.default_rng(s)
            return g.multinomial(n=N, pvals=self.rho_f, size=(self.L, self.N, self.N)).argmax(axis=-1)

        return [sample_y(seed + i) for i in range(N)]

    def get_inferred_model(self, method="rho_max", threshold=None):
        options = ["rho_max", "rho_mean", "fixed_threshold", "heuristic_threshold"]
        if method not in options:
            raise ValueError("'method' should be one of {}.".format(", ".join(['"' + x + '"' for x in options])))
        if (not self.mutuality and method != "rho_max") or (self.K > 2 and "threshold" in method):
            msg = ('threshold methods is incompatible with VIMuRe\'s mutuality=False '
                   'or for data with more than 2 categories. Using "rho_max" method.')
            warnings.warn(msg, UserWarning)
            method = "rho_max"
        # rho still on the GPU (fit(keep_engine=True), nothing has read rho_f): the read-out runs there (vmr_readout)
        dev = getattr(self, "_engine", None) if getattr(self, "_rho_f", None) is None else None
        if method == "rho_max":
            if dev is not None:
                return dev.readout("rho_max").astype("int")
            return np.argmax(self.rho_f, axis=-1).astype("int")
        if method == "rho_mean":
            if dev is not None:
                return dev.readout("rho_mean")
            return np.dot(self.rho_f, range(0, self.rho_f.shape[-1]))
        if method == "fixed_threshold":
            if threshold is None or threshold > 1 or threshold < 0:
                raise ValueError('For method="fixed_threshold", you must set the threshold to a value in [0,1].')
        else:  # heuristic threshold, reference utils.py:200-217
            threshold = 0.54 * self.G_exp_nu - 0.01
        if dev is not None:
            Y = dev.readout("threshold", threshold)
            return Y.astype(np.float64) if method == "fixed_threshold" else Y.astype("int")
        Y = np.copy(self.rho_f[:, :, :, 1])
        Y[Y < threshold] = 0
        Y[Y >= threshold] = 1
        return Y if method == "fixed_threshold" else Y.astype("int")

    def _edge_method(self, method, threshold):
        """(engine method, threshold) of an edge table: `get_inferred_model`'s resolution of method and threshold, warning and
        errors included; "rho_mean" gives no categories and is refused."""
        options = ["rho_max", "rho_mean", "fixed_threshold", "heuristic_threshold"]
        if method not in options:
            raise ValueError("'method' should be one of {}.".format(", ".join(['"' + x + '"' for x in options])))
        if (not self.mutuality and method != "rho_max") or (self.K > 2 and "threshold" in method):
            msg = ('threshold methods is incompatible with VIMuRe\'s mutuality=False '
                   'or for data with more than 2 categories. Using "rho_max" method.')
            warnings.warn(msg, UserWarning)
            method = "rho_max"
        if method == "rho_mean":
            raise ValueError('method="rho_mean" gives expected weights, not categories: an edge list needs "rho_max", '
                             '"fixed_threshold" or "heuristic_threshold" (the table\'s `mean` column holds the expected weight).')
        if method == "rho_max":
            return "rho_max", 0.0
        if method == "fixed_threshold":
            if threshold is None or threshold > 1 or threshold < 0:
                raise ValueError('For method="fixed_threshold", you must set the threshold to a value in [0,1].')
        else:  # heuristic threshold, reference utils.py:200-217
            threshold = 0.54 * self.G_exp_nu - 0.01
        return "threshold", float(threshold)

    def get_inferred_edgelist(self, method="rho_max", threshold=None, select=("reported", "inferred"), layer=None, X=None, R=None):
        """The inferred network as an edge list built on the GPU (vmr_edge_table) -- what the reference's experiment driver
        assembles from dense arrays (karnataka.py:200-318) -- instead of `get_inferred_model`'s [L,N,N] array: a row per tie that
        someone reported (select "reported") and / or that the read-out infers (`y > 0`; "inferred"), in (layer, source, target)
        order; neither rho nor a dense read-out crosses PCIe.  method and threshold as `get_inferred_model` takes them (same
        warning and fall-back, same errors); "rho_mean" is a ValueError.  Columns: layer, source, target, y (the category
        `get_inferred_model` gives the tie), probability (sum_{k>=1} rho_k), mean (sum_k k rho_k), n_reports #{m : X > 0},
        total_reports sum_m X, n_mask #{m : R != 0}, source_report X[l,i,j,i], target_report X[l,i,j,j] (counts over all
        reporters, R ignored) and reciprocated_y, reciprocated_n_reports, reciprocated_total of the tie (l,j,i).  layer: that
        layer only.  Engine as in `calculate_mean_poisson`."""
        if not hasattr(self, "gamma_shp_f"):
            raise ValueError("the model has not been fitted: call fit(..., keep_engine=True) first, or fit it and pass X=")
        code, thr = self._edge_method(method, threshold)
        with self._read_engine(X, R) as eng:
            t = eng.edge_table(method=code, threshold=thr, select=select, layer=layer)
        return pd.DataFrame({
            "layer": np.asarray(t["l"], np.int64), "source": np.asarray(t["i"], np.int64), "target": np.asarray(t["j"], np.int64),
            "y": np.asarray(t["y"], np.int64), "probability": np.asarray(t["prob"], np.float64),
            "mean": np.asarray(t["mean"], np.float64), "n_reports": np.asarray(t["n_rep"], np.int64),
            "total_reports": np.asarray(t["total"], np.int64), "n_mask": np.asarray(t["n_mask"], np.int64),
            "source_report": np.asarray(t["ego"], np.int64), "target_report": np.asarray(t["alter"], np.int64),
            "reciprocated_y": np.asarray(t["y_T"], np.int64), "reciprocated_n_reports": np.asarray(t["n_rep_T"], np.int64),
            "reciprocated_total": np.asarray(t["total_T"], np.int64)})

    # ------------------------------------------------------------------ posterior-predictive check (model.py:1220-1293)
    def _ppc_engine(self, X, R):
        """(engine, temporary): the engine kept by fit(keep_engine=True) when X is None, else a temporary one holding X and R
        (routed as `fit` routes them) set to the model's best state (`*_f`, rho_f as the prior)."""
        if not hasattr(self, "gamma_shp_f"):
            raise ValueError("the model has not been fitted: call fit(..., keep_engine=True) first, or fit it and pass X=")
        if X is None:
            eng = getattr(self, "_engine", None)
            if eng is None:
                raise ValueError("no device state to read: fit(..., keep_engine=True) keeps one; otherwise pass the data as X= "
                                 "(and R=)")
            if R is not None:
                raise ValueError("R= is taken with X= only: the kept engine holds the R of the fit")
            return eng, False
        if isinstance(X, pd.DataFrame) or type(X).__name__ == "Graph":
            from ._io import read_from_edgelist, read_from_igraph
            net = read_from_edgelist(X) if isinstance(X, pd.DataFrame) else read_from_igraph(X)
            X = net.X
            if R is None:
                R = net.R
        if R is None:
            R = getattr(self, "R", None)
        Xd = X if _is_torch(X) else engine_data(X, "X")
        shape = tuple(int(s) for s in Xd.shape)
        if shape != (self.L, self.N, self.N, self.M):
            raise ValueError(f"X has shape {shape}, the fitted model {(self.L, self.N, self.N, self.M)}")
        if R is not None and tuple(int(s) for s in R.shape) != shape:
            raise ValueError("Dimensions of reporter mask (R) do not match L x N x N x M")
        coo = is_sparse_like(Xd)
        Rd = R
        if R is None or _is_torch(R):
            pass
        elif coo:
            Rd = R if is_sparse_like(R) else SparseTensor.fromarray(np.asarray(R) != 0)
        else:
            Rd = to_dense_u8(R, "R")
            if Rd.dtype != np.uint8 or Rd.max(initial=0) > 1:
                Rd = (Rd != 0).astype(np.uint8)
        if coo:
            eng = CaviEngine.from_coo(Xd.subs, Xd.vals, shape, R=None if Rd is None else Rd.subs, K=self.K,
                                      mutuality=self.mutuality, eps=self.EPS)
        else:
            eng = CaviEngine(Xd, Rd, K=self.K, mutuality=self.mutuality, eps=self.EPS)
        try:
            eng.set_priors(self.alpha_theta, self.beta_theta, self.alpha_lambda, self.beta_lambda,
                           self.alpha_mutuality, self.beta_mutuality)
            eng.set_state(self.gamma_shp_f, self.gamma_rte_f, self.phi_shp_f, self.phi_rte_f, self.nu_shp_f, self.nu_rte_f,
                          self.rho_f)
        except BaseException:
            eng.close()
            raise
        return eng, True

    @contextlib.contextmanager
    def _read_engine(self, X, R):
        """The engine of `_ppc_engine` for the length of a read-out; a temporary one is closed on the way out."""
        eng, tmp = self._ppc_engine(X, R)
        try:
            yield eng
        finally:
            if tmp:
                eng.close()

    def calculate_mean_poisson(self, X=None, R=None, layer=None, device=False):
        """Expected reports of the best realisation over the support of R -- the reference's `_calculate_mean_poisson`
        (model.py:1220-1293) computed on the GPU (vmr_mean_poisson): a SparseTensor of shape (L, N, N, M) whose subs are the
        (l, i, j, m) with R != 0 (every one without R) in lexicographic order -- np.nonzero's; for a coordinate-list R the
        reference keeps R.subs' order instead -- and vals = sum_k rho_f (G_exp_theta_f G_exp_lambda_f + G_exp_nu_f X^T).
        X None: the engine kept by fit(keep_engine=True); else X (and R, default the fit's) go to a temporary engine, as in
        `fit`.  layer: that layer only.  device=True: subs and vals are torch tensors on the GPU."""
        with self._read_engine(X, R) as eng:
            subs, vals = eng.mean_poisson(layer=layer, device=device)
        shape = (self.L, self.N, self.N, self.M)
        if not device:
            return SparseTensor(subs, vals, shape=shape)
        st = SparseTensor.__new__(SparseTensor)   # (tensors stay on the device: no conversion)
        st.subs, st.vals, st.shape, st.ndim, st.dtype = tuple(subs), vals, shape, 4, vals.dtype
        return st

    def report_auc(self, X=None, R=None, layer=None):
        """AUC of the expected reports against the observed ones (X > 0) over the support of R: `utils.calculate_AUC(mp, X,
        mask=R)` (reference utils.py:40-66), exact, on the GPU (vmr_report_auc); of one layer or of the whole tensor.  NaN with
        a warning when the support holds no positive or no negative.  Engine as in `calculate_mean_poisson`."""
        with self._read_engine(X, R) as eng:
            auc, n_pos, n_neg = eng.report_auc(layer=layer)
        if n_pos == 0 or n_neg == 0:
            warnings.warn("No %s reports in the support: the AUC is undefined" % ("positive" if n_pos == 0 else "negative"),
                          UserWarning)
        return float(auc)

    def posterior_network_stats(self, n_samples=100, seed=None, n_trials=1, Y_true=None, degrees=False, X=None, R=None,
                                triads=False, local_clustering=False):
        """Posterior distribution of the network's summary statistics, computed on the GPU (vmr_sample_stats,
        vmr_expected_stats): n_samples draws of Y from q(Y) -- sample s is `sample_inferred_model(N=n_trials, seed=seed + s,
        device=True)[0]` -- reduced where rho lives to edges, weight, mutual pairs and, with Y_true [L,N,N], true positives (and
        the degrees when asked); only those counts cross PCIe.  Returns a `netstats.NetworkStats`: the counts, reciprocity
        (`utils.calculate_overall_reciprocity` per sample), density, precision / recall / F1 against Y_true, the analytic
        expectations (`expected`) and `summary()`.  seed None: the fit's.  Engine as in `calculate_mean_poisson`.
        triads=True: also the triad counts of the same samples (vmr_sample_triads: transitive and cyclic triples, two-paths,
        and triangles, wedges and edges of the symmetrised network, self-loops left out), the transitivity and cyclicity
        ratios per sample and the expected counts (vmr_expected_triads) as `expected["exp_<name>"]`; local_clustering=True
        (implies triads): also every node's triangles and degree, its local clustering coefficient and their average."""
        from .netstats import NetworkStats
        triads = bool(triads or local_clustering)
        if seed is None:
            seed = self.seed
        ref_edges = None
        if Y_true is not None and not _is_torch(Y_true):
            Y_true = np.asarray(Y_true)
            if Y_true.shape != (self.L, self.N, self.N):
                raise ValueError(f"Y_true has shape {Y_true.shape}, the fitted model's networks {(self.L, self.N, self.N)}")
            ref_edges = (Y_true > 0).sum(axis=(1, 2))
        with self._read_engine(X, R) as eng:
            counts = eng.sample_stats(seed, n_samples, n_trials=n_trials, Y_ref=Y_true, degrees=degrees)
            expected = eng.expected_stats()
            tri = exp_tri = None
            if triads:
                tri = eng.sample_triads(seed, n_samples, n_trials=n_trials, nodes=bool(local_clustering))
                exp_tri = eng.expected_triads()
        if Y_true is not None and ref_edges is None:
            ref_edges = (Y_true > 0).sum(dim=(1, 2)).cpu().numpy()
        return NetworkStats(self.N, counts, expected=expected, ref_edges=ref_edges, seed=seed, n_trials=n_trials, triads=tri,
                            expected_triads=exp_tri)

    def posterior_mixing(self, groups=None, n_samples=100, seed=None, n_trials=1, skip_diagonal=True, overlap=True, X=None, R=None):
        """Who is tied to whom, by group, and how far the layers' ties coincide, over the posterior of the network, computed on
        the GPU (vmr_sample_mixing, vmr_expected_mixing): n_samples draws of Y from q(Y) -- sample s is
        `sample_inferred_model(N=n_trials, seed=seed + s, device=True)[0]` -- reduced where rho lives to the mixing matrix
        mix[s, l, a, b] = #{(i, j) : g_i = a, g_j = b, Y_lij > 0}, its reciprocated part and the overlap between layers
        #{(i, j) : Y_lij > 0 and Y_l'ij > 0}; only those integers cross PCIe.
        groups: N labels of any kind in node order (strings, ints; None or NaN: the node is left out of the mixing matrix, not
        of the overlap), or a dict / pandas Series keyed by node name (the `nodeNames` of a model fitted from an edge list, the
        node's index otherwise; an unknown name is a ValueError, a node that is not named is left out;
        `mixing.groups_from_frame` makes one from a node table).  Codes follow `np.unique`'s order, 64 groups at most.
        groups None: the overlap only.  skip_diagonal leaves the self-loops out of every table.  Returns a `mixing.MixingStats`:
        the integer tables, assortativity, E-I index, block densities and reciprocities, the layers' Jaccard index, the analytic
        expectations (`expected`: their ratios are ratios of expectations), `summary()` and `frame()`.  seed None: the fit's.
        Engine as in `calculate_mean_poisson`."""
        from .mixing import MixingStats, encode_groups
        if seed is None:
            seed = self.seed
        codes = labels = None
        if groups is not None:
            names = getattr(self, "nodeNames", None)
            if names is not None:
                names = names.sort_values("id")["name"].tolist()
            codes, labels = encode_groups(groups, self.N, names)
            if len(labels) < 1:
                raise ValueError("groups labels no node")
        elif not overlap:
            raise ValueError("nothing to compute: no groups and overlap=False")
        with self._read_engine(X, R) as eng:
            C = None if codes is None else len(labels)
            counts = eng.sample_mixing(seed, n_samples, groups=codes, C=C, n_trials=n_trials, skip_diagonal=skip_diagonal, overlap=overlap)
            expected = eng.expected_mixing(groups=codes, C=C, skip_diagonal=skip_diagonal, overlap=overlap)
        return MixingStats(self.N, counts, codes=codes, labels=labels, expected=expected, skip_diagonal=skip_diagonal, seed=seed,
                           n_trials=n_trials)

    def posterior_connectivity(self, n_samples=100, seed=None, n_trials=1, nodes=False, X=None, R=None):
        """Does the inferred network hang together, how large is its giant component, who reaches whom and in how many steps --
        over the posterior of the network, computed on the GPU (vmr_sample_connectivity): n_samples draws of Y from q(Y) -- sample
        s is `sample_inferred_model(N=n_trials, seed=seed + s, device=True)[0]` -- reduced where rho lives to the weak and strong
        components, the reachable ordered pairs, the sum, the histogram and the maximum of their shortest-path lengths (self-loops
        left out); only those integers cross PCIe.  nodes=True: also every node's component labels, how many nodes it reaches
        and is reached by and the sums of those distances.  Returns a `connectivity.ConnectivityStats`: the integers, the giant
        components' fractions, connectedness, average path length, global efficiency, with nodes the closeness centralities and
        `same_component(i, j)`, `summary()` and `frame()`.  There is no closed form under the mean field, hence no expectations.
        At most 2048 nodes.  seed None: the fit's.  Engine as in `calculate_mean_poisson`."""
        from .connectivity import ConnectivityStats
        if seed is None:
            seed = self.seed
        with self._read_engine(X, R) as eng:
            counts = eng.sample_connectivity(seed, n_samples, n_trials=n_trials, hist=True, nodes=bool(nodes))
        return ConnectivityStats(self.N, counts, seed=seed, n_trials=n_trials)

    def posterior_centrality(self, q=None, T=3, direction="out", n_samples=100, seed=None, n_trials=1, top_k=10, values=False,
                             X=None, R=None):
        """Who is central, and how sure is the posterior of it?  Diffusion centrality (Banerjee et al. 2013) of every node over
        the posterior of the network, computed on the GPU (vmr_sample_centrality, vmr_mean_centrality): n_samples draws of Y from
        q(Y) -- sample s is `sample_inferred_model(N=n_trials, seed=seed + s, device=True)[0]` -- and per draw and layer
        c = sum_{t=1..T} (q M)^t 1 with M = A = (Y > 0) without self-loops (direction "out": how far a node's word travels), A.T
        ("in") or A | A.T ("union"); reduced where rho lives to every node's sum and sum of squares of c, the sum of its ranks and
        how often it is among the top_k, and each draw's total and maximum; only those cross PCIe (values=True: also every
        draw's c).  T = 1 is q times the degree; T large with q below 1 / lambda_1 is Katz centrality.
        q: a scalar or one value per layer in [0, 1].  q None takes, per layer, min(1, N / expected edges) from `expected_stats()`:
        the reciprocal of the expected mean degree, at which a walk's expected offspring is one -- a choice of scale, not the
        literature's 1 / lambda_1.  Returns a `centrality.CentralityStats`: mean, sd, expected_rank, top_prob, the plug-in
        centrality of the mean network (`plug_in`: the expectation of c only for "out" / "in" with T <= 2), `top()`, `frame()` and
        `summary()`.  At most 2048 nodes.  seed None: the fit's.  Engine as in `calculate_mean_poisson`."""
        from .centrality import CentralityStats, default_q
        if seed is None:
            seed = self.seed
        with self._read_engine(X, R) as eng:
            if q is None:
                q = default_q(self.N, eng.expected_stats()["edges"])
            counts = eng.sample_centrality(seed, n_samples, q, T, direction=direction, top_k=top_k, n_trials=n_trials, values=bool(values))
            plug_in = eng.mean_centrality(q, T, direction=direction)
        return CentralityStats(self.N, counts, np.broadcast_to(np.asarray(q, dtype=np.float64), (self.L,)).copy(), T, direction=direction,
                               top_k=top_k, plug_in=plug_in, seed=seed, n_trials=n_trials)

    def posterior_betweenness(self, direction="directed", n_samples=100, seed=None, n_trials=1, top_k=10, values=False, X=None, R=None):
        """Who brokers, and how sure is the posterior of it?  Betweenness centrality of every node -- the share of the shortest
        paths between the others that pass through it, unnormalised, `networkx.betweenness_centrality(normalized=False)` -- over
        the posterior of the network, computed on the GPU (vmr_sample_betweenness): n_samples draws of Y from q(Y) -- sample s is
        `sample_inferred_model(N=n_trials, seed=seed + s, device=True)[0]` -- and per draw and layer Brandes' algorithm on A =
        (Y > 0) without self-loops (direction "directed") or on A | A.T ("union"); reduced where rho lives to every node's sum and
        sum of squares of b, the sum of its ranks and how often it is among the top_k, and each draw's total and maximum; only
        those cross PCIe (values=True: also every draw's b).  Returns a `betweenness.BetweennessStats`: mean, sd, expected_rank,
        top_prob, the betweenness of the point estimate `get_inferred_model()` (`inferred`, by the same kernels), `normalized()`,
        `top()`, `frame()` and `summary()`.  At most 2048 nodes.  seed None: the fit's.  Engine as in `calculate_mean_poisson`."""
        from .betweenness import BetweennessStats
        if seed is None:
            seed = self.seed
        with self._read_engine(X, R) as eng:
            counts = eng.sample_betweenness(seed, n_samples, direction=direction, top_k=top_k, n_trials=n_trials, values=bool(values))
            inferred = eng.network_betweenness(self.get_inferred_model(), direction=direction)
        return BetweennessStats(self.N, counts, direction=direction, top_k=top_k, inferred=inferred, seed=seed, n_trials=n_trials)

    def posterior_cores(self, mode="union", k=None, n_samples=100, seed=None, n_trials=1, top_k=10, values=False, X=None, R=None):
        """Where is the dense core of the network, who sits in it and who is periphery -- and how sure is the posterior of it?
        The k-core decomposition (`networkx.core_number`) over the posterior of the network, computed on the GPU
        (vmr_sample_cores): n_samples draws of Y from q(Y) -- sample s is `sample_inferred_model(N=n_trials, seed=seed + s,
        device=True)[0]` -- and per draw and layer the coreness of every node on A = (Y > 0) without self-loops: the largest k
        such that the node lies in a set whose every node has degree >= k inside the set.  mode: "union" (distinct neighbours in
        A | A.T: the undirected graph), "total" (in plus out: a reciprocated pair counts 2, networkx on the DiGraph), "in" or
        "out".  Reduced where rho lives to every node's sum and sum of squares of the coreness, the sum of its ranks, how often it
        is among the top_k, in the main core and in the k-core, and each draw's degeneracy, main-core size and k-core size; only
        those cross PCIe (values=True: also every draw's coreness).
        k: the core whose membership is counted (`kcore_prob`, `kcore_size`, `core_members()`).  k None takes the degeneracy of
        the point estimate `get_inferred_model()` -- ONE number for all layers, the smallest over the layers, so that the k-core of
        the point estimate is not empty in any layer; pass a k to choose another.
        Returns a `cores.CoreStats`: mean, sd, expected_rank, top_prob, main_core_prob, kcore_prob, the coreness of the point
        estimate (`inferred`, by the same kernel), `top()`, `core_members()`, `frame()` and `summary()`.  At most 2048 nodes.
        seed None: the fit's.  Engine as in `calculate_mean_poisson`."""
        from .cores import CoreStats
        if seed is None:
            seed = self.seed
        with self._read_engine(X, R) as eng:
            inferred = eng.network_cores(self.get_inferred_model(), mode=mode)
            if k is None:
                k = int(inferred.max(axis=1).min())
            counts = eng.sample_cores(seed, n_samples, mode=mode, k_min=k, top_k=top_k, n_trials=n_trials, values=bool(values))
        return CoreStats(self.N, counts, mode=mode, k_min=k, top_k=top_k, inferred=inferred, seed=seed, n_trials=n_trials)

    def posterior_cutpoints(self, mode="union", n_samples=100, seed=None, top_k=10, n_trials=1, values=False, X=None, R=None):
        """Who holds the network together -- whose departure would split a component, into how many pieces, how many pairs of
        people would lose every path between them, which single ties are the only connection between two parts -- and how sure
        is the posterior of it?  Cut points (`networkx.articulation_points`), bridges (`networkx.bridges`) and Borgatti's
        key-player fragmentation over the posterior of the network, computed on the GPU (vmr_sample_cutpoints): n_samples draws of
        Y from q(Y) -- sample s is `sample_inferred_model(N=n_trials, seed=seed + s, device=True)[0]` -- and per draw and layer,
        on the undirected graph A | A.T (mode "union") or A & A.T ("mutual", the reciprocated ties) of A = (Y > 0) without
        self-loops, for every node the branches its component falls into without it, the pairs of other nodes that removal
        disconnects (pairs_cut) and its bridges.  Reduced where rho lives to every node's sum and sum of squares of pairs_cut, the
        sum of its ranks, how often it is among the top_k and a cut point, the sums of its branches and bridges, and each draw's
        cut points, bridges, largest pairs_cut and connected pairs; only those cross PCIe (values=True: also every draw's
        pairs_cut, branches and bridges).  All non-cut nodes share a rank, so `top_prob` can count more than top_k nodes.
        Returns a `cutpoints.CutpointStats`: cut_prob, mean, sd, expected_rank, top_prob, mean_branches, mean_bridges, the same
        numbers of the point estimate `get_inferred_model()` (`inferred`, by the same kernels), `fragmentation()`, `quantiles()`,
        `top()`, `key_players()`, `frame()` and `summary()`.  There is no closed form under the mean field, hence no
        expectations.  At most 2048 nodes.  seed None: the fit's.  Engine as in `calculate_mean_poisson`."""
        from .cutpoints import CutpointStats
        if seed is None:
            seed = self.seed
        with self._read_engine(X, R) as eng:
            inferred = eng.network_cutpoints(self.get_inferred_model(), mode=mode)
            counts = eng.sample_cutpoints(seed, n_samples, mode=mode, top_k=top_k, n_trials=n_trials, values=bool(values))
        return CutpointStats(self.N, counts, mode=mode, top_k=top_k, inferred=inferred, seed=seed, n_trials=n_trials)

    def posterior_cascades(self, q=None, T=3, direction="out", seeds=None, n_cascades=16, n_samples=100, seed=None, cascade_seed=None,
                           n_trials=1, top_k=10, values=False, X=None, R=None):
        """If information enters the network at these nodes and every tie passes it on with probability q, how many nodes has it
        reached after T periods, who is the best single entry point -- and how sure is the posterior of either?  The
        independent-cascade model over the posterior of the network, computed on the GPU (vmr_sample_outreach,
        vmr_sample_seed_outreach): n_samples draws of Y from q(Y) -- sample s is `sample_inferred_model(N=n_trials, seed=seed + s,
        device=True)[0]` -- and on each n_cascades cascades: a cascade keeps every tie of A = (Y > 0) without self-loops with
        probability q_l (a counter-based draw keyed by cascade_seed + s, the cascade and the tie), the information spreads along
        the kept ties of A (direction "out"), A.T ("in") or A | A.T ("union", one draw per pair) for T periods, and the outreach
        is the number of nodes informed beyond the seeds.  Unlike `posterior_centrality` a node reached twice counts once;
        `posterior_connectivity` is the case q = 1 without a bound on T.  Exact integers: only they cross PCIe.
        seeds None: every node as a single seed; returns a `cascades.CascadeStats` -- mean, sd, expected_rank, top_prob, the
        outreach of the point estimate `get_inferred_model()` (`inferred`, by the same kernels), `top()`, `frame()` and
        `summary()` (values=True: also every draw's outreach summed over its cascades).  seeds {label: nodes}, up to 64 sets, the
        nodes by name (the `nodeNames` of a model fitted from an edge list) or by index: returns a `cascades.SeedOutreach` --
        per set the mean and sd over the samples, `quantiles()`, `curve()` (the cumulative share reached by period),
        `reach_prob()` (how often each node is informed), `frame()` and `summary()`.
        q: a scalar or one value per layer in [0, 1]; q None takes `posterior_centrality`'s scale, per layer min(1, N / expected
        edges), the reciprocal of the expected mean degree.  cascade_seed None: the sampling seed.  At most 2048 nodes.  seed
        None: the fit's.  Engine as in `calculate_mean_poisson`."""
        from .cascades import CascadeStats, SeedOutreach, resolve_seed_sets
        from .centrality import default_q
        if seed is None:
            seed = self.seed
        if cascade_seed is None:
            cascade_seed = seed
        labels = sets = None
        if seeds is not None:
            names = getattr(self, "nodeNames", None)
            if names is not None:
                names = names.sort_values("id")["name"].tolist()
            labels, sets = resolve_seed_sets(seeds, self.N, names)
        with self._read_engine(X, R) as eng:
            if q is None:
                q = default_q(self.N, eng.expected_stats()["edges"])
            qa = np.broadcast_to(np.asarray(q, dtype=np.float64), (self.L,)).copy()
            kw = dict(T=T, direction=direction, n_cascades=n_cascades, cascade_seed=cascade_seed)
            if sets is not None:
                res = eng.sample_seed_outreach(seed, n_samples, sets, qa, n_trials=n_trials, curve=True, node_hits=True, **kw)
                return SeedOutreach(self.N, res, labels, sets, qa, T, direction=direction, n_cascades=n_cascades, seed=seed,
                                    cascade_seed=cascade_seed, n_trials=n_trials)
            counts = eng.sample_outreach(seed, n_samples, qa, top_k=top_k, n_trials=n_trials, values=bool(values), **kw)
            inferred = eng.network_outreach(self.get_inferred_model(), qa, **kw)
        return CascadeStats(self.N, counts, qa, T, direction=direction, n_cascades=n_cascades, top_k=top_k, inferred=inferred, seed=seed,
                            cascade_seed=cascade_seed, n_trials=n_trials)

    def posterior_triad_census(self, n_samples=100, seed=None, n_trials=1, X=None, R=None):
        """Which local structures does the network hold, and how sure is the posterior of them?  The Holland-Leinhardt triad
        census (`networkx.triadic_census`: the unordered triples of nodes in each of the 16 classes 003 012 102 021D 021U 021C
        111D 111U 030T 030C 201 120D 120U 120C 210 300) over the posterior of the network, computed on the GPU
        (vmr_sample_triad_census): n_samples draws of Y from q(Y) -- sample s is `sample_inferred_model(N=n_trials, seed=seed + s,
        device=True)[0]` -- counted where rho lives on A = (Y > 0) without self-loops; only the 16 integers per sample and layer
        cross PCIe.  It says what the six aggregates of `posterior_network_stats(triads=True)` cannot: whether closed triads are
        transitive (030T, 120D, 120U) or cyclic (030C), whether brokered two-paths stay open (021C, 111D, 111U, 201), whether
        hierarchies (021D, 021U, 120D, 120U) are over-represented given the dyads.
        Returns a `census.TriadCensus`: counts, mean, sd, `quantiles()`, the census of the point estimate `get_inferred_model()`
        (`inferred`, by the same kernel), `dyads()`, `expected_under_man()` (the expectation given each sample's own mutual,
        asymmetric and null dyads), `excess()`, `transitive_share()`, `frame()` and `summary()`.  seed None: the fit's.  Engine as
        in `calculate_mean_poisson`."""
        from .census import TriadCensus
        if seed is None:
            seed = self.seed
        with self._read_engine(X, R) as eng:
            inferred = eng.network_triad_census(self.get_inferred_model())
            counts = eng.sample_triad_census(seed, n_samples, n_trials=n_trials)
        return TriadCensus(self.N, counts, inferred=inferred, seed=seed, n_trials=n_trials)

    def posterior_shared_partners(self, mode="union", n_samples=100, seed=None, n_trials=1, n_bins=64, nodes=False, ties="inferred", X=None,
                                  R=None):
        """Which ties does the posterior say are embedded, and which are bridges?  The shared partners of every tie over the
        posterior of the network, computed on the GPU (vmr_sample_shared_partners): n_samples draws of Y from q(Y) -- sample s is
        `sample_inferred_model(N=n_trials, seed=seed + s, device=True)[0]` -- reduced where rho lives on A = (Y > 0) without
        self-loops; rho does not cross PCIe.  mode "union": the unordered pairs tied either way, a partner is tied (either way) to
        both ends -- the support of Jackson, Rodriguez-Barraquer and Tan is the share of ties with a partner, a local bridge a tie
        with none; "mutual": the pairs tied both ways and partners tied both ways to both (Krackhardt's Simmelian ties); "path":
        the ordered ties i -> j and the k with i -> k -> j, the edgewise shared partners behind ERGM's GWESP.  n_bins: the bins
        of the histogram of ties by partner count, whose last bin pools the larger counts.  nodes=True: also per node its ties
        and its supported ties.  ties: the ties to follow one by one -- "inferred": those of `get_inferred_model()` under the
        mode's tie rule; an array of (layer, i, j) rows; None: none.
        Returns a `partners.SharedPartners`: hist, totals, `support()`, `mean_partners()`, `local_bridges()`, mean, sd,
        `quantiles()`, `gwesp(decay)`, `node_support()`, the same counts of the point estimate (`inferred`, by the same kernels),
        `ties_frame()`, `bridges()`, `frame()` and `summary()`.  seed None: the fit's.  Engine as in `calculate_mean_poisson`."""
        from .partners import SharedPartners
        if seed is None:
            seed = self.seed
        point = self.get_inferred_model()
        if isinstance(ties, str):
            if ties != "inferred":
                raise ValueError(f'ties must be "inferred", None or an array of (layer, i, j) rows, got {ties!r}')
            A = np.asarray(point) > 0
            A &= ~np.eye(self.N, dtype=bool)
            At = A.transpose(0, 2, 1)
            T = A if mode == "path" else np.triu(A & At if mode == "mutual" else A | At, 1)
            pairs = np.argwhere(T).astype(np.int32)
        else:
            pairs = None if ties is None else np.asarray(ties, dtype=np.int32).reshape(-1, 3)
        with self._read_engine(X, R) as eng:
            inferred = eng.network_shared_partners(point, mode=mode, n_bins=n_bins, nodes=nodes, pairs=pairs)
            res = eng.sample_shared_partners(seed, n_samples, n_trials=n_trials, mode=mode, n_bins=n_bins, nodes=nodes, pairs=pairs)
        return SharedPartners(self.N, mode, res["hist"], res["totals"], node_ties=res.get("node_ties"), node_supported=res.get("node_supported"),
                              pairs=pairs, pair_present=res.get("pair_present"), pair_supported=res.get("pair_supported"),
                              pair_partners=res.get("pair_partners"), inferred=inferred, seed=seed, n_trials=n_trials)

    def posterior_structural_holes(self, mode="union", n_samples=100, seed=None, n_trials=1, top_k=10, values=False, X=None, R=None):
        """Whose contacts are disconnected from one another -- who brokers between groups that do not talk -- and how sure is the
        posterior of it?  Burt's structural holes over the posterior of the network, computed on the GPU
        (vmr_sample_structural_holes): n_samples draws of Y from q(Y) -- sample s is `sample_inferred_model(N=n_trials, seed=seed
        + s, device=True)[0]` -- and per draw and layer, on A = (Y > 0) without self-loops, every node's effective size (its
        non-redundant contacts) and constraint (how far its ties are concentrated in one interconnected group).  mode "union": the
        symmetrised binary network, `networkx.effective_size` / `networkx.constraint` of the undirected graph; "weighted": Burt's
        weights A + A.T on the directed network, networkx on the DiGraph -- but defined for every node with a tie.  A node
        without a tie is undefined in that draw.  Reduced where rho lives to every node's sum and sum of squares of both measures,
        the sums of its ranks among the defined nodes, how often it is among the top_k (the largest effective sizes, the smallest
        constraints) and in how many draws it is defined; rho does not cross PCIe (values=True: also every draw's degree,
        strength, redundancy and the two measures).  Local and cheap: any N, unlike `posterior_betweenness`.
        Returns a `holes.StructuralHoles`: the views `.effective_size` and `.constraint` (mean and sd over the draws in which the
        node is defined, expected_rank, top_prob, `top()`, `frame()`), `defined_prob`, `efficiency()`, `brokers()`, the measures
        of the point estimate `get_inferred_model()` (`inferred`, by the same kernels), `frame()` and `summary()`.  seed None: the
        fit's.  Engine as in `calculate_mean_poisson`."""
        from .holes import StructuralHoles
        if seed is None:
            seed = self.seed
        with self._read_engine(X, R) as eng:
            inferred = eng.network_structural_holes(self.get_inferred_model(), mode=mode)
            counts = eng.sample_structural_holes(seed, n_samples, n_trials=n_trials, mode=mode, top_k=top_k, values=bool(values))
        return StructuralHoles(self.N, counts, mode=mode, top_k=top_k, inferred=inferred, seed=seed, n_trials=n_trials)

    def posterior_predictive_check(self, n_rep=100, seed=None, params="draw", n_trials=1, by_reporter=False, X=None, R=None):
        """Does data drawn from the fitted model look like the data it was fitted to?  n_rep replicated datasets are drawn on the
        GPU over the support of R and reduced there (vmr_ppc_replicates; no replicate is written) to the integers of
        `predictive.PredictiveCheck` -- positive reports, their sum and sum of squares, reciprocated reports, ties reported by
        anyone and by at least two -- and the observed data is reduced the same way (vmr_ppc_observed).
        Replicate r: Y from rho with seed + r (`sample_inferred_model(N=n_trials, seed=seed + r, device=True)`), the reports with
        seed + 2^32 + r.  params="draw": theta, lambda, eta of every replicate from their Gamma posteriors with
        `np.random.RandomState(seed)` (`PosteriorSyntheticNetwork.build_X`'s draw; an eta >= 1 is drawn again); "mean": the
        posterior means.  by_reporter=True: also (n_pos, total) of every reporter.  seed None: the fit's.  Returns the
        `PredictiveCheck`: `p_values()`, `summary()`.  Engine as in `calculate_mean_poisson`."""
        from .predictive import PredictiveCheck, draw_parameters
        if seed is None:
            seed = self.seed
        seed = int(seed)
        if not hasattr(self, "gamma_shp_f"):
            raise ValueError("the model has not been fitted: call fit(..., keep_engine=True) first, or fit it and pass X=")
        theta, lam, eta, redraws = draw_parameters(self.gamma_shp_f, self.gamma_rte_f, self.phi_shp_f, self.phi_rte_f, self.nu_shp_f,
                                                   self.nu_rte_f, n_rep, seed, params=params)
        seed_y, seed_x = seed, seed + 2 ** 32
        with self._read_engine(X, R) as eng:
            rep = eng.ppc_replicates(theta, lam, eta, seed_y, seed_x, n_trials=n_trials, by_reporter=by_reporter)
            obs = eng.ppc_observed(by_reporter=by_reporter)
            support = [eng.mean_poisson_size(layer=l) for l in range(self.L)]
        rep, rep_m = rep if by_reporter else (rep, None)
        obs, obs_m = obs if by_reporter else (obs, None)
        return PredictiveCheck(obs, rep, observed_by_reporter=obs_m, replicated_by_reporter=rep_m, support=support, seed_y=seed_y,
                               seed_x=seed_x, n_trials=n_trials, theta=theta, lam=lam, eta=eta, eta_redraws=redraws, params=params)

    def score_truth(self, Y_true, thresholds=None, score="rho1", skip_diagonal=False, auc=True, X=None, R=None):
        """How well does rho recover a known network?  The scores of the reference's synthetic experiments -- F1 of `rho_1 >=
        threshold` at every threshold (unreliable_reporters.py:189-200; `utils.get_optimal_threshold`), of the arg-max
        read-out, AUC, Brier score, calibration -- as a `scoring.TruthScore`.  While rho is still on the GPU
        (fit(keep_engine=True) and nothing has read rho_f: `get_inferred_model`'s rule), or with X= (a temporary engine, as in
        `calculate_mean_poisson`), one pass on the device (vmr_score_truth) returns a few integers per layer and threshold;
        otherwise `scoring.score_truth_np` runs on rho_f.  Y_true [L,N,N]: an array, a COO container or a uint8 GPU tensor.
        thresholds None: np.linspace(0, 1, 101).  score "rho1" or "prob" (sum_{k>=1} rho_k).  The reference's heuristic
        threshold 0.54 G_exp_nu - 0.01 (utils.py:200-217) is scored too and reported by `summary()`."""
        from .scoring import TruthScore, check_thresholds, score_truth_np, SCORES
        if getattr(self, "_rho_f", None) is None and getattr(self, "_engine", None) is None:
            raise ValueError("the model has not been fitted: call fit first")
        if score not in SCORES:
            raise ValueError("score must be \"rho1\" or \"prob\"")
        thr = check_thresholds(thresholds)
        if Y_true is None:
            raise ValueError("Y_true is None")
        if not _is_torch(Y_true):
            Y_true = Y_true.toarray() if hasattr(Y_true, "toarray") else np.asarray(Y_true)
        if tuple(int(q) for q in Y_true.shape) != (self.L, self.N, self.N):
            raise ValueError(f"Y_true has shape {tuple(Y_true.shape)}, the fitted model's networks {(self.L, self.N, self.N)}")
        heur = np.array([0.54 * float(self.G_exp_nu) - 0.01]) if np.isfinite(getattr(self, "G_exp_nu", np.nan)) else None
        dev = getattr(self, "_engine", None) if getattr(self, "_rho_f", None) is None else None
        if X is not None or dev is not None:
            with self._read_engine(X, R) as eng:
                res = eng.score_truth(Y_true, thresholds=thr, score=score, skip_diagonal=skip_diagonal, auc=auc)
                hh = None if heur is None else eng.score_truth(Y_true, thresholds=heur, score=score, skip_diagonal=skip_diagonal,
                                                               auc=False, outputs=("hist",))
        else:
            if R is not None:
                raise ValueError("R= is taken with X= only")
            Yh = Y_true.cpu().numpy() if _is_torch(Y_true) else Y_true
            res = score_truth_np(self.rho_f, Yh, thr, score, skip_diagonal)
            hh = None if heur is None else score_truth_np(self.rho_f, Yh, heur, score, skip_diagonal)
            if not auc:
                res["auc"], res["auc_pairs"] = None, None
        return TruthScore(res, thr, heuristic=None if hh is None else (heur[0], hh["hist"]), score=score, skip_diagonal=bool(skip_diagonal))

    def reporter_table(self, method="rho_max", threshold=None, layer=None, X=None, R=None):
        """Which reporters are reliable, read off the fitted model on the GPU (vmr_reporter_table): per layer and reporter, how
        many of their reports fall on ties the model infers (hits, false_reports, precision), how many inferred ties within their
        scope they left out (omissions, recall), and how their report total compares with the expected one (exp_total, residual,
        ratio) -- a `reporters.ReporterTable`; `frame()` gives one row per (layer, reporter).  One pass over rho plus the
        reports: neither rho nor the support of R crosses PCIe.  method and threshold as `get_inferred_edgelist` takes them
        (same warning and fall-back, same errors); layer: that layer only.  Beside the table: theta = G_exp_theta_f, theta_mean
        = gamma_shp_f / gamma_rte_f and theta_interval, the central 95 % interval of the Gamma posterior (scipy.stats; left out,
        None, where scipy is not installed).  Engine as in `calculate_mean_poisson`."""
        from .reporters import ReporterTable
        if not hasattr(self, "gamma_shp_f"):
            raise ValueError("the model has not been fitted: call fit(..., keep_engine=True) first, or fit it and pass X=")
        code, thr = self._edge_method(method, threshold)
        if layer is not None and not 0 <= int(layer) < self.L:
            raise ValueError(f"layer {layer} out of range [0, {self.L})")
        with self._read_engine(X, R) as eng:
            res = eng.reporter_table(method=code, threshold=thr, layer=layer)
        rows = slice(None) if layer is None else slice(int(layer), int(layer) + 1)
        shp, rte = np.asarray(self.gamma_shp_f, dtype=np.float64)[rows], np.asarray(self.gamma_rte_f, dtype=np.float64)[rows]
        interval = None
        try:
            from scipy import stats
            interval = np.stack([stats.gamma.ppf(0.025, shp, scale=1.0 / rte), stats.gamma.ppf(0.975, shp, scale=1.0 / rte)], axis=-1)
        except ImportError:
            pass
        return ReporterTable(res, layers=np.arange(self.L)[rows], theta=np.asarray(self.G_exp_theta_f)[rows], theta_mean=shp / rte,
                             theta_interval=interval, method=code, threshold=thr if code == "threshold" else None)

    def heldout_loglik(self, subs, x, xt=None, estimate="mean", X=None, R=None):
        """The log predictive density of reports the fit never saw, scored on the GPU under the best realisation
        (vmr_heldout_loglik): subs the 4 index arrays (l, i, j, m) of the held-out entries (non-decreasing in l), x their counts,
        xt the mirrored counts X[l,j,i,m] their rates condition on (None: taken from X= when it is given and the model has
        mutuality, else 0).  estimate "mean" plugs in the posterior means of theta, lambda and eta, "geometric" the g_theta,
        g_lambda, g_nu `calculate_mean_poisson` uses (`crossval.plug_in_tables`).  Returns the dict of
        `CaviEngine.heldout_loglik`: logp and mean per entry, and per layer the sums and counts -- `counts[:, 3]` is the number of
        entries that lie INSIDE the engine's mask, i.e. that the fit has seen.  `crossval.cross_validate` drives whole folds
        through this.  Engine as in `calculate_mean_poisson`."""
        from .crossval import mirror_counts, plug_in_tables
        if not hasattr(self, "gamma_shp_f"):
            raise ValueError("the model has not been fitted: call fit(..., keep_engine=True) first, or fit it and pass X=")
        if xt is None and X is not None and self.mutuality and not (isinstance(X, pd.DataFrame) or type(X).__name__ == "Graph"):
            xt = mirror_counts(X, subs)
        with self._read_engine(X, R) as eng:
            theta, lam, eta = plug_in_tables(self, eng, estimate)
            return eng.heldout_loglik(subs, x, xt, theta=theta, lam=lam, eta=eta)

    def surprising_reports(self, top=100, threshold=None, select="both", estimate="mean", layer=None, max_rows=10_000_000, X=None,
                           R=None):
        """Which individual reports does the fitted model disbelieve, and which omissions?  Every element (l, i, j, m) of the
        support of R is scored on the GPU (vmr_report_scores) under the best realisation: its surprise is -log p of the observed
        count (or zero) under the posterior mixture of Poissons, the likelihood of `heldout_loglik`; neither rho nor the support
        crosses PCIe.  Exactly one of `top` and `threshold` is given (top=None with threshold=): threshold -- one call, every
        selected element with surprise >= threshold, in (layer, source, target, reporter) order; top -- a first pass over a fixed
        grid of surprise levels (4096 edges, 1/64 nat apart, from 0) finds the largest level with at least `top` selected elements
        at or above it (0 when there is none), a second one fetches those rows (more than `max_rows` of them: ValueError naming
        the count), which are sorted by (-surprise, layer, source, target, reporter) and cut to `top`.  select "reports" (x > 0),
        "omissions" (x = 0) or "both"; estimate as `heldout_loglik` ("mean", "geometric"); layer: that layer only.  Returns a
        `residuals.ReportScores`: `frame()` (layer, source, target, reporter, x, x_mirror, logp, surprise, expected, residual),
        `reporters()`, `lppd` -- the exact in-sample log predictive density per layer, the training-side figure beside
        `crossval.CVResult.lpd` -- and with `top` the histogram of the surprise over the grid.  Engine as in
        `calculate_mean_poisson`."""
        from .crossval import plug_in_tables
        from .residuals import ReportScores, grid_edges, select_code, threshold_for_top, top_rows
        if (top is None) == (threshold is None):
            raise ValueError("exactly one of top and threshold is given (top=None with threshold=)")
        sel = select_code(select)
        if top is not None and int(top) < 1:
            raise ValueError("top must be at least 1")
        if not hasattr(self, "gamma_shp_f"):
            raise ValueError("the model has not been fitted: call fit(..., keep_engine=True) first, or fit it and pass X=")
        if layer is not None and not 0 <= int(layer) < self.L:
            raise ValueError(f"layer {layer} out of range [0, {self.L})")
        with self._read_engine(X, R) as eng:
            theta, lam, eta = plug_in_tables(self, eng, estimate)
            if threshold is not None:
                return ReportScores(eng.report_scores(theta, lam, eta, float(threshold), select=sel, layer=layer), estimate=estimate)
            agg = eng.report_scores(theta, lam, eta, np.inf, select=sel, layer=layer, edges=grid_edges(), rows=False, by_reporter=False)
            thr, _ = threshold_for_top(agg["hist"], agg["edges"], top, sel, max_rows=max_rows)
            res = eng.report_scores(theta, lam, eta, thr, select=sel, layer=layer)
        res.update(top_rows(res, top))
        res["hist"], res["edges"] = agg["hist"], agg["edges"]
        return ReportScores(res, estimate=estimate, top=int(top))

    def influence_tables(self):
        """(e_theta [L,M], elog_theta [L,M], e_lambda [L,K], elog_lambda [L,K], g_nu) of the best realisation, the tables of the
        CAVI update of rho: shp / rte and psi(shp) - log(rte) of gamma_*_f and phi_*_f, exp(psi(nu_shp_f) - log(nu_rte_f)); g_nu
        is 0 without mutuality."""
        gs, gr = np.asarray(self.gamma_shp_f, dtype=np.float64), np.asarray(self.gamma_rte_f, dtype=np.float64)
        ps, pr = np.asarray(self.phi_shp_f, dtype=np.float64), np.asarray(self.phi_rte_f, dtype=np.float64)
        g_nu = float(np.exp(sp.psi(float(self.nu_shp_f)) - np.log(float(self.nu_rte_f)))) if self.mutuality else 0.0
        return gs / gr, sp.psi(gs) - np.log(gr), ps / pr, sp.psi(ps) - np.log(pr), g_nu

    def reporter_influence(self, method="rho_max", threshold=None, select="both", min_shift=None, top=None, layer=None,
                           max_rows=10_000_000, X=None, R=None):
        """Whose word does an inferred tie rest on?  For every element (l, i, j, m) of the support of R the tie's row of rho is
        recomputed on the GPU without reporter m's report (vmr_reporter_influence): the CAVI update of a row is additive over the
        reporters of its mask, so dividing one reporter's factor out of the fitted row gives the row the update would have
        produced with R[l,i,j,m] = 0; neither rho nor the support crosses PCIe.
        What the numbers are: the parameters (theta, lambda, nu of the best realisation) are held fixed and one reporter's factor
        is removed from one tie.  They are an exact refit of that row only when rho is the update's fixed point for those
        parameters -- a converged fit is close to one -- and never a refit of the whole model.
        method and threshold as `get_inferred_edgelist` takes them (same warning and fall-back, same errors).  An element is LOST
        when the tie is inferred and its leave-one-out row is not, GAINED the other way round; its shift is the total variation
        tv between the two rows.  select "lost", "gained", "both" or "none": which flips are listed; min_shift: also every
        element with tv >= min_shift; top=n instead: the n elements with the largest tv -- a first pass over a fixed grid of 4096
        edges over [0, 1] finds the largest level with at least n elements at or above it, a second one fetches those rows (more
        than `max_rows`: ValueError naming the count), sorted by (-tv, layer, source, target, reporter) and cut.  layer: that
        layer only.  Returns an `influence.ReporterInfluence`: `frame()` one row per (layer, reporter) -- n_scope, lost, gained,
        mean_tv, mean_shift -- `rows()` the listed elements, `fragile_ties()` those whose removal loses the tie.  Engine as in
        `calculate_mean_poisson`."""
        from .influence import ReporterInfluence, grid_edges, min_tv_for_top, select_code, top_rows
        if top is not None and min_shift is not None:
            raise ValueError("at most one of top and min_shift is given")
        sel = select_code(select)
        if top is not None and int(top) < 1:
            raise ValueError("top must be at least 1")
        if min_shift is not None and not float(min_shift) >= 0.0:
            raise ValueError("min_shift must lie in [0, +inf]")
        if not hasattr(self, "gamma_shp_f"):
            raise ValueError("the model has not been fitted: call fit(..., keep_engine=True) first, or fit it and pass X=")
        code, thr = self._edge_method(method, threshold)
        if layer is not None and not 0 <= int(layer) < self.L:
            raise ValueError(f"layer {layer} out of range [0, {self.L})")
        tabs = self.influence_tables()
        with self._read_engine(X, R) as eng:
            if top is None:
                min_tv = np.inf if min_shift is None else float(min_shift)
                return ReporterInfluence(eng.reporter_influence(*tabs, method=code, threshold=thr, select=sel, min_tv=min_tv, layer=layer))
            agg = eng.reporter_influence(*tabs, method=code, threshold=thr, select=0, min_tv=np.inf, layer=layer, edges=grid_edges(),
                                         rows=False)
            min_tv, _ = min_tv_for_top(agg["hist"], agg["edges"], top, max_rows=max_rows)
            res = eng.reporter_influence(*tabs, method=code, threshold=thr, select=0, min_tv=min_tv, layer=layer)
        res.update(top_rows(res, top))
        res["hist"], res["edges"] = agg["hist"], agg["edges"]
        return ReporterInfluence(res, top=int(top))

    def predict(self, X=None, method="rho_max", threshold=None):
        """Alias of `get_inferred_model` (the reference's experiment wrapper calls it predict)."""
        return self.get_inferred_model(method=method, threshold=threshold)

    def get_posterior_estimates(self):
        return {"nu": self.G_exp_nu_f, "theta": self.G_exp_theta_f, "lambda": self.G_exp_lambda_f, "rho": self.rho_f}
