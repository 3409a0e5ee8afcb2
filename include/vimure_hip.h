/*
 * vimure_hip.h -- C-ABI of libvimure_hip.so, the MI355X (gfx950) CAVI engine for the
 * VIMuRe latent-network model.
 *
 * The reference (latentnetworks/vimure) has no FFI: its hot path is a set of private
 * methods of `VimureModel` that mutate NumPy arrays held in `self`
 * (src/python/vimure/model.py).  This header is the seam a maintainer would bind with
 * ctypes; every entry point names the reference code it replaces.
 *
 * Conventions
 *   - plain pointers and sizes only; all floating point is IEEE double, as in the reference;
 *   - arrays are C-order: X,R [L,N,N,M] (layer, ego, alter, reporter), rho/pr_rho [L,N,N,K],
 *     gamma_* [L,M], phi_* [L,K];
 *   - every function returns 0 on success and a negative VMR_E* code on failure;
 *     vmr_last_error() gives the message (pass NULL for errors of vmr_create);
 *   - one handle <-> one device <-> one HIP stream; a handle is not re-entrant, distinct
 *     handles are independent (that is the multi-GPU model: one process per GPU);
 *   - host pointers are only read/written during the call; the library owns all device memory.
 */
#ifndef VIMURE_HIP_H
#define VIMURE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vmr_ctx* vmr_handle;

enum {
  VMR_OK = 0,
  VMR_EINVAL = -1,   /* bad argument / unsupported size (ValueError in the host class) */
  VMR_EHIP = -2,     /* HIP runtime error (RuntimeError) */
  VMR_ENAN = -3,     /* ELBO is NaN (model.py:1015-1016 raises ValueError("ELBO is NaN!!!!")) */
  VMR_ESTATE = -4    /* call order violated (priors/state not set) */
};

/* sub-steps of one sweep, for vmr_sub_step (model.py:643-656) */
enum { VMR_STEP_GAMMA = 0, VMR_STEP_PHI = 1, VMR_STEP_RHO = 2, VMR_STEP_NU = 3 };

/* read-out methods for vmr_readout (model.py:1099-1188) */
enum { VMR_READ_RHO_MAX = 0, VMR_READ_RHO_MEAN = 1, VMR_READ_THRESHOLD = 2 };

/* kernel classes for vmr_profile_read */
enum {
  VMR_KERNEL_GAMMA_MASK = 0,   /* masked reduction over R: A[l,m,k] = sum_ij R rho           */
  VMR_KERNEL_GAMMA_COUNTS = 1, /* sweep over X for gamma_shp (and phi_shp when mutuality off) */
  VMR_KERNEL_PHI = 2,          /* sweep over X for phi_shp (mutuality on)                     */
  VMR_KERNEL_RHO = 3,          /* sweep over X,R: rho update (+ nu partial)                   */
  VMR_KERNEL_ELBO = 4,         /* stand-alone ELBO sweep                                      */
  VMR_KERNEL_FINALIZE = 5,     /* the small reduce/parameter kernels                          */
  VMR_KERNEL_RHO_ELBO = 6,     /* rho update with the ELBO data terms reduced in the same pass */
  VMR_KERNEL_RHO_NOSTORE = 7,  /* rho update whose rho is used (statistics, nu) but not written: the inner sweeps of a vmr_step call, whose rho
                                  the next sweep overwrites unread */
  VMR_KERNEL_COUNT = 8
};

/*
 * Dataset handle.  Replaces the data set-up half of `__check_fit_params`
 * (model.py:134-213).  The dense count tensor is turned into REPORT LISTS on the device -- one 4-byte entry per non-zero
 * count carrying the mirrored count X[l,j,i,m], so X^T (model.py:141-161 `data_T`, `data_T_vals`) is never
 * materialised -- and then freed; tensors that are not sparse enough (or with M > 8192) stay as
 * dense uint8 tiles with R packed to one bit per (l,i,j,m).  vmr_data_format tells which.
 *   X  [L,N,N,M] uint8 counts (values <= 255).
 *   R  [L,N,N,M] uint8 0/1, or NULL = every reporter may report on every tie
 *      (model.py:206-211 default).
 *   data_on_device != 0: X and R are device pointers on `device` (e.g. torch tensors).
 *   mutuality: 0/1 (model.py:60-65; the host class forces 0 for undirected networks).
 *   eps: the EPS white-noise constant (model.py:215-218), normally 1e-12.
 * The handle is reusable across realisations and seeds (vmr_set_state restarts it).
 * Environment, read here: VMR_DETERMINISTIC=1 makes the handle's sweeps bit-reproducible run to run (the reference's
 * single-threaded NumPy, model.py:623-660, is): every sum whose order varies from run to run is a 64-bit integer sum in fixed
 * point.  It covers every handle on report lists, the specialised kernels (K <= 8, packed entries) and the general ones (any K,
 * two-word entries) alike, whether a partial mask is held as reporter lists or as words; handles on dense tiles return VMR_EINVAL, and vmr_sub_step returns VMR_ESTATE on such a handle.
 * Cost: DESIGN.md §3c.
 */
int vmr_create(vmr_handle* out, int device, int L, int N, int M, int K, int mutuality,
               const uint8_t* X, const uint8_t* R, int data_on_device, double eps);

/*
 * The same dataset handle from COORDINATE LISTS -- what the reference actually holds: `X.subs` / `X.vals` of the
 * sptensor built by `read_from_edgelist` (_io.py:132-295) or `preprocess` (utils.py:220-248), and `R.subs` of a sparse
 * reporter mask; `__check_fit_params` derives `data_T_vals` from them with an O(nnz^2) lookup (model.py:148-161).  No dense
 * [L,N,N,M] tensor is built anywhere: the lists are sorted on the device and become the report lists directly.
 *   nx reports: xl, xi, xj, xm (int32 subscripts) and xv (counts, 1 .. 2^31 - 1); no duplicates.
 *   nr mask entries rl, ri, rj, rm (R = 1 there, 0 elsewhere); nr < 0: every reporter may report on every tie
 *   (model.py:206-211).
 *   data_on_device != 0: all index arrays are device pointers on `device`.
 * Limits (VMR_EINVAL with a message naming the one exceeded, checked before the kernels that need them): M <= 65535 (the
 * mask lists hold 16-bit reporters); L N^2 2^mb < 2^64 with mb = max(13, ceil(log2 Mp)) reporter bits of the 64-bit sort keys
 * (Mp: M rounded up to 16); (largest count + 1) * Mp < 2^32; fewer than 2^31 coordinates per list, fewer than 2^31 ties and
 * fewer than 2^32 entry slots per layer.  M <= 8192 with (largest count + 1) * M <= 2^20 and K <= 8 runs the specialised
 * kernels; beyond that the general ones (wider M: reporter tables read through L2).  VMR_DETERMINISTIC=1 (see vmr_create) covers
 * every handle this function creates, whichever kernels it runs.
 */
int vmr_create_coo(vmr_handle* out, int device, int L, int N, int M, int K, int mutuality,
                   int64_t nx, const int32_t* xl, const int32_t* xi, const int32_t* xj, const int32_t* xm, const int32_t* xv,
                   int64_t nr, const int32_t* rl, const int32_t* ri, const int32_t* rj, const int32_t* rm,
                   int data_on_device, double eps);

void vmr_destroy(vmr_handle h);

const char* vmr_last_error(vmr_handle h);

/* Data statistics the host-side initialisation needs:
 *   sum_x     = X.vals.sum()  (model.py:174, enters nu_rte at model.py:593-595)
 *   coverage  [L,N,N] uint8, 1 iff the tie has at least one R entry AND at least one
 *             non-zero report; ties with 0 get the one-hot rho prior (model.py:508-556).
 *             May be NULL. */
int vmr_data_stats(vmr_handle h, double* sum_x, uint8_t* coverage);

/* Hyper-parameters, already broadcast to full arrays by the host (model.py:238-317):
 * alpha/beta_theta [L,M], alpha/beta_lambda [L,K], eta prior scalars. */
int vmr_set_priors(vmr_handle h, const double* alpha_theta, const double* beta_theta,
                   const double* alpha_lambda, const double* beta_lambda,
                   double alpha_eta, double beta_eta);

/* Start of a realisation: `_initialize_priors` + `_initialize_old_variables`
 * (model.py:561-617).  The host draws the values from RandomState (model.py:470-482,
 * 570-592) so fixed-seed fits match the reference; the library sets rho <- pr_rho and
 * logpr_rho <- log(pr_rho + eps) (model.py:559, 602).
 * pr_rho_on_device != 0: pr_rho is a device pointer. */
int vmr_set_state(vmr_handle h, const double* gamma_shp, const double* gamma_rte,
                  const double* phi_shp, const double* phi_rte, double nu_shp, double nu_rte,
                  const double* pr_rho, int pr_rho_on_device);

/* The initial rho prior of a realisation drawn on the device, bit for bit what `_set_rho_prior` (model.py:470-482, 509-559)
 * draws from a RandomState without an informative prior: 1 + 0.01 * rand(L,N,N,K) (MT19937, genrand_res53), + bias0 on
 * category 0, symmetrised when undirected != 0, normalised per tie in NumPy's summation order, one-hot (1, 0, .., 0) where the
 * handle's coverage (vmr_data_stats) is 0.  The host only walks the generator: block b holds the ties [tie_cuts[b],
 * tie_cuts[b + 1]) (2K 32-bit words each) and starts from the generator state mt_keys[b * 624 .. +624], mt_pos[b] (the key and
 * position of RandomState.get_state(), pos in [0, 624]).  tie_cuts[nblk + 1] must rise strictly from 0 to L*N*N.
 * out: [L,N,N,K] in natural order, device memory (out_on_device != 0) or host memory (filled through one copy).
 * Runs on the handle's stream and synchronises it, so vmr_set_state(..., out, 1) takes out as it is.
 * Invalid descriptors return VMR_EINVAL before anything is launched. */
int vmr_draw_pr_rho(vmr_handle h, int nblk, const int64_t* tie_cuts, const uint32_t* mt_keys, const int32_t* mt_pos,
                    double bias0, int undirected, double* out, int out_on_device);

/* n_iters full sweeps of `_update_CAVI` (model.py:623-660): gamma -> phi -> rho -> nu, each
 * with the cache refresh of model.py:662-696 fused in.  Asynchronous on the handle's stream
 * unless elbo_out != NULL, in which case the ELBO (`__ELBO`, model.py:948-1019) is reduced
 * inside the last sweep's rho pass and returned (this synchronises). */
int vmr_step(vmr_handle h, int n_iters, double* elbo_out);

/* The convergence loop of `fit` for the realisation set up by vmr_set_state (model.py:405-426 with the stop rule of
 * `_check_for_convergence`, model.py:1021-1056): sweeps until the ELBO -- evaluated at iteration 1, every 10th and
 * max_iter -- has changed by less than `tol` on more than `decision` consecutive evaluations, or max_iter is reached.
 * Trace rows as the reference appends them (iterations that are multiples of 10, model.py:423-426): iteration, ELBO,
 * wall time of that iteration's sweep in seconds, reached flag; at most `cap` rows.  *elbo = last ELBO, *iters =
 * iterations run, *converged = the stop rule fired.  One call per realisation instead of one per iteration: host
 * threads that drive several small fits at once then meet in the GPU, not in the caller's interpreter. */
int vmr_fit_loop(vmr_handle h, int max_iter, double tol, int decision, int cap, int* n_rows, int* row_iter, double* row_elbo,
                 double* row_runtime, int* row_reached, double* elbo, int* iters, int* converged);

/* The same loop for n handles in lockstep -- the realisations of many small fits (the reference's Karnataka experiment,
 * notebooks/python/experiments/karnataka.py:170-191: a village layer of N = 200-800 is two dependent 20-40 us launches per
 * sweep that leave the GPU nearly empty).  Every handle must have had its vmr_set_state.  The handles of the first one's kind
 * (report lists in one pass, same K / mutuality / mask kind, same device) share ONE launch of each kernel per sweep, their
 * ELBOs come back in one copy, a handle that converges leaves the launch; handles of another kind run their loops one after the
 * other.  Each handle's results are exactly those of vmr_fit_loop.  Arrays are per handle: n_rows[n], row_*[n * cap] (handle u
 * at u * cap), elbo[n], iters[n], converged[n], rc[n] (a handle's own return code; its message via vmr_last_error).  Returns the
 * first non-zero rc, else VMR_OK.  Replaces n calls of model.py:405-426 running side by side. */
int vmr_fit_loop_batch(vmr_handle* hs, int n, int max_iter, double tol, int decision, int cap, int* n_rows, int* row_iter,
                       double* row_elbo, double* row_runtime, int* row_reached, double* elbo, int* iters, int* converged, int* rc);

/* Stand-alone ELBO of the current state (model.py:948-1019 incl. the stale G_exp_nu of
 * model.py:970).  Synchronises.  Returns VMR_ENAN when the value is NaN. */
int vmr_elbo(vmr_handle h, double* out);

/* Fits whose LAYERS are spread over several handles / GPUs (BASELINE config 5).  nu is one scalar shared by
 * all layers (model.py:589-596, 822-825) and the ELBO stop rule is joint (model.py:1039-1047), so the owners
 * exchange three doubles per sweep:
 *   vmr_sweep_local runs gamma, phi, rho on the local layers, does NOT commit nu, synchronises and returns
 *     out3[0] = local sum x w2 rho (the local part of nu_shp - alpha_eta),
 *     out3[1] = local ELBO terms that do not involve nu (only when want_elbo; data, entropy, theta/lambda Gamma terms),
 *     out3[2] = local sum_t (sum_k rho_k) Q_t  (enters the ELBO as -E[nu] * total; only when want_elbo);
 *   the caller sums the three over all owners (2-3 doubles all-reduce, latency-bound) and gives every owner
 *   vmr_commit_nu(total of out3[0]).  ELBO = total out3[1] - E[nu] * total out3[2] + Gamma term of nu
 *   (model.py:1006-1011), with nu_rte = beta_eta + sum of X over ALL layers set through vmr_set_state. */
int vmr_sweep_local(vmr_handle h, int want_elbo, double* out3);
int vmr_commit_nu(vmr_handle h, double nu_partial_total);

/* The same exchange without a host hop per sweep (RCCL on GPUs): vmr_sweep_local_dev queues the sweep and leaves the three
 * doubles in the caller's DEVICE buffer out3_dev (asynchronous on the handle's stream); the caller all-reduces that buffer
 * ON THE HANDLE'S STREAM (vmr_stream returns the hipStream_t; e.g. torch.cuda.ExternalStream) and vmr_commit_nu_dev reads the
 * total from device memory, again on that stream.  Only ELBO evaluations (every 10th sweep) bring numbers to the host. */
int vmr_sweep_local_dev(vmr_handle h, int want_elbo, double* out3_dev);
int vmr_commit_nu_dev(vmr_handle h, const double* nu_partial_total_dev);
void* vmr_stream(vmr_handle h);

/* One update of a sweep (test hook for step-level parity with model.py:643-656).  GAMMA, RHO and NU may come in any order, each is
 * the reference's update from the current state with exp(E[log nu]) of the current nu.  VMR_STEP_PHI commits phi's rate as the
 * finalize of VMR_STEP_GAMMA prepares it (one pass over the mask sums serves gamma's rate and phi's): it returns VMR_ESTATE unless
 * a VMR_STEP_GAMMA ran since rho last changed (vmr_set_state, VMR_STEP_RHO, any sweep); VMR_STEP_NU in between is fine, and a second
 * VMR_STEP_PHI is the reference's update once more.  Without mutuality VMR_STEP_GAMMA commits gamma AND phi and VMR_STEP_PHI does
 * nothing.  Not available with VMR_DETERMINISTIC=1 (VMR_ESTATE). */
int vmr_sub_step(vmr_handle h, int which);

/* Copy the posteriors to the host: what `_update_optimal_parameters` snapshots
 * (model.py:925-942).  Any pointer may be NULL.  Synchronises. */
int vmr_get_state(vmr_handle h, double* gamma_shp, double* gamma_rte, double* phi_shp,
                  double* phi_rte, double* nu_shp, double* nu_rte, double* rho);

/* Best-realisation bookkeeping on the device: vmr_snapshot keeps a copy of rho and of every parameter -- what
 * `_update_optimal_parameters` copies into the `*_f` attributes (model.py:925-942), without moving rho (8 L N^2 K bytes)
 * to the host after every realisation; vmr_restore makes the snapshot the current state again, so that
 * vmr_get_state / vmr_get_geometric read the best realisation once, at the end of `fit`.  Asynchronous on the
 * handle's stream.  The snapshot does not hold the log prior of its realisation: after vmr_restore the state can be read
 * (vmr_get_*, vmr_readout, vmr_sample) but the sweeping entry points (vmr_commit_nu and vmr_commit_nu_dev among them) return
 * VMR_ESTATE until the next vmr_set_state.  The priors are the handle's, not the snapshot's: vmr_restore leaves what the last
 * vmr_set_priors set.  A snapshot outlives vmr_set_state. */
int vmr_snapshot(vmr_handle h);
int vmr_restore(vmr_handle h);

/* Posterior read-out of the CURRENT rho on the device -- `get_inferred_model` (model.py:1099-1188) and
 * `apply_rho_threshold` (utils.py:207-217) -- so that a 16 MB answer crosses PCIe instead of the 256 MB of rho:
 *   VMR_READ_RHO_MAX    out uint8 [L,N,N]   argmax_k rho (first maximum, as np.argmax)
 *   VMR_READ_RHO_MEAN   out double [L,N,N]  sum_k k rho_k
 *   VMR_READ_THRESHOLD  out uint8 [L,N,N]   rho[...,1] >= threshold
 * out_on_device != 0: `out` is a device pointer.  Synchronises. */
int vmr_readout(vmr_handle h, int method, double threshold, void* out, int out_on_device);

/* Posterior samples of Y on the device -- `sample_inferred_model` (model.py:1062-1096; also the draw of
 * `PosteriorSyntheticNetwork`, synthetic.py:964-1177): per tie, n_trials categorical trials from the CURRENT rho and the most
 * frequent category (first maximum), i.e. Generator.multinomial(n_trials, rho).argmax(-1).  out uint8 [L,N,N].  The uniforms
 * are Philox4x32-10 with key = seed and counter = (tie index, trial): reproducible for a seed, independent of the data
 * layout, NOT NumPy's PCG64 stream (the host class keeps that exact mode).  rho (8 L N^2 K bytes) stays on the device.
 * out_on_device != 0: `out` is a device pointer.  Synchronises. */
int vmr_sample(vmr_handle h, uint64_t seed, int n_trials, uint8_t* out, int out_on_device);

/* Posterior expected reports on the device -- `_calculate_mean_poisson` (model.py:1220-1293; its `pd.merge` of R.subs with data_T
 * at :1272-1285) -- over the support S = {(l,i,j,m) : R[l,i,j,m] != 0} (every (l,i,j,m), the diagonal included, without R):
 *   mp[l,i,j,m] = sum_k rho[l,i,j,k] (G_theta[l,m] G_lambda[l,k] + G_nu XT[l,i,j,m]),  k ascending,
 *   XT[l,i,j,m] = X[l,j,i,m] with mutuality, else 0 (model.py:141-145, 164-170),
 * from the CURRENT rho (after vmr_restore: the snapshot's) and the G_* that vmr_get_geometric returns as g_theta, g_lambda, g_nu.
 * Order: lexicographic in (l,i,j,m), np.nonzero's -- also for handles made by vmr_create_coo, where the reference keeps the
 * order of R.subs.  layer < 0: every layer; else that one (sl then holds it).  vmr_mean_poisson_size gives |S|; n is the
 * capacity of the outputs (VMR_EINVAL below |S|); subscripts (int32) and vals: any subscript pointer may be NULL; device
 * pointers when out_on_device != 0.  Each value is one lane's sum: bit-identical from run to run.  VMR_ENAN when a value is NaN.
 * Synchronise; temporaries (a tie-major index of the reports, 24 B per report slot of a layer; support offsets, 16 B per tie)
 * are freed before return, and one that does not fit in the free device memory is refused with VMR_EINVAL. */
int vmr_mean_poisson_size(vmr_handle h, int layer, uint64_t* n);
int vmr_mean_poisson(vmr_handle h, int layer, uint64_t n, int32_t* sl, int32_t* si, int32_t* sj, int32_t* sm,
                     double* vals, int out_on_device);

/* AUC of the expected reports against the observed ones over the support -- `utils.calculate_AUC(mp, X, mask=R)`
 * (utils.py:40-66, i.e. sklearn's roc_curve + auc) -- of one layer, or of all (layer < 0):
 *   P = #{S : X > 0}, Q = |S| - P,  AUC = (#{(p,n) : mp_p > mp_n} + #{(p,n) : mp_p = mp_n} / 2) / (P Q).
 * The pair counts are exact 64-bit integer sums (bit-identical from run to run); VMR_EINVAL when 2 P Q reaches 2^63 or P 2^31.
 * P = 0 or Q = 0: *auc = NaN (sklearn's answer, with its warning left to the caller).  n_pos / n_neg may be NULL.  Rules of
 * vmr_mean_poisson otherwise. */
int vmr_report_auc(vmr_handle h, int layer, double* auc, uint64_t* n_pos, uint64_t* n_neg);

/* Network statistics of n_samples posterior samples of Y, computed where rho lives: sample s is exactly what
 * vmr_sample(h, seed + s, n_trials, ..) writes (seed + s mod 2^64; the same Philox draw), and only the statistics come back.
 * counts: host uint64 [n_samples][L][4], over ALL (i, j) of a layer, the diagonal included:
 *   0 edges   #{Y > 0}                          (Y > 0).sum()
 *   1 weight  sum Y                             Y.sum()
 *   2 mutual  #{(i,j) : Y_ij > 0 and Y_ji > 0}  np.logical_and(Y > 0, Y.T > 0).sum()  -- mutual / weight is the reference's
 *                                               utils.calculate_overall_reciprocity (utils.py:69-70)
 *   3 tp      #{Y > 0 and y_ref > 0}            0 without y_ref
 * y_ref: uint8 [L,N,N] (a device pointer when y_ref_on_device != 0) or NULL.  deg_out / deg_in: host int32 [n_samples][L][N],
 * deg_out[s][l][i] = #{j : Y_ij > 0}, deg_in[s][l][j] = #{i : Y_ij > 0}; either may be NULL.
 * Reads the CURRENT rho (after vmr_restore: the snapshot's), once per chunk of samples; any K, any n_trials >= 1, both data
 * formats.  All sums are integer sums: bit-identical from run to run.  The chunk's temporaries (L N^2 bytes per sample, half
 * of the free device memory at most, 256 samples at most) are freed before return; a single sample that does not fit is
 * refused with VMR_EINVAL.  n_samples < 1, n_trials < 1 or counts NULL: VMR_EINVAL; before vmr_set_state: VMR_ESTATE.
 * Synchronises. */
int vmr_sample_stats(vmr_handle h, uint64_t seed, int n_samples, int n_trials, const uint8_t* y_ref, int y_ref_on_device,
                     uint64_t* counts, int32_t* deg_out, int32_t* deg_in);

/* The same quantities in expectation under q(Y) = prod rho, no sampling: with p_ij = sum_{k>=1} rho_ijk (k ascending),
 *   out[l] = (sum p_ij, sum_ij sum_k k rho_ijk, sum_ij p_ij p_ji, sum p_ij (1 - p_ij))        host double [L][4]
 * -- expected edges, expected weight, the numerator of the expected reciprocity (all ordered pairs: the diagonal enters as
 * p_ii^2; out[2] / out[0] is the quotient for K = 2) and the variance of `edges`.  Doubles summed by a fixed two-stage tree
 * (no atomics): bit-identical from run to run.  Temporary: 8 L N^2 bytes (VMR_EINVAL when that does not fit).  Synchronises. */
int vmr_expected_stats(vmr_handle h, double* out);

/* Triad statistics of n_samples posterior samples of Y, computed where rho lives -- what a user otherwise gets from `A @ A` in
 * NumPy on every `sample_inferred_model` draw.  Sample s is exactly what vmr_sample(h, seed + s, n_trials, ..) writes (mod 2^64).
 * Per sample and layer: A_ij = (Y_ij > 0) with the DIAGONAL CLEARED (a self-loop belongs to no triad), U = A | A^T, and i, j, k
 * pairwise distinct.  counts: host uint64 [n_samples][L][VMR_TRIAD_NSTAT]:
 *   0 transitive   #{(i,j,k) : i->j, j->k, i->k}                      ((A @ A.T) * A).sum()
 *   1 cyclic       #{(i,j,k) : i->j, j->k, k->i}, ordered: a 3-cycle counts 3 times    ((A @ A) * A.T).sum()
 *   2 two_paths    #{(i,j,k) : i->j, j->k}                            (A @ A).sum() - np.trace(A @ A)
 *   3 triangles_u  triangles of U, each once                          np.trace(U @ U @ U) // 6
 *   4 wedges_u     sum_i d_i (d_i - 1) / 2, d_i the degree of i in U
 *   5 edges_u      #{i < j : U_ij}
 * node_tri[s][l][i]: triangles of U through node i; node_deg[s][l][i] = d_i; host int32 [n_samples][L][N], either may be NULL.
 * The samples are packed into bit rows (64-bit words, out- and in-neighbours) and counted by AND + popcount.  All sums are
 * integer sums: bit-identical from run to run.  Reads the CURRENT rho once per chunk of samples; any K, any n_trials >= 1, both
 * data formats.  A chunk (L N^2 + 16 L N ceil(N/64) bytes per sample plus the outputs; half of the free device memory at most,
 * 256 samples at most, VMR_NETSTATS_CHUNK at most) is freed before return; a single sample that does not fit is refused with
 * VMR_EINVAL.  n_samples < 1, n_trials < 1 or counts NULL: VMR_EINVAL; before vmr_set_state: VMR_ESTATE.  Synchronises. */
#define VMR_TRIAD_NSTAT 6
int vmr_sample_triads(vmr_handle h, uint64_t seed, int n_samples, int n_trials, uint64_t* counts, int32_t* node_tri,
                      int32_t* node_deg);

/* The same six quantities in expectation under q(Y) = prod rho, no sampling -- instead of NumPy matrix products on the rho of
 * `get_state`.  p_ij = sum_{k>=1} rho_ijk (k ascending, the number of vmr_expected_stats), p_ii := 0, and for i != j
 * u_ij = 1 - (1 - p_ij)(1 - p_ji).  Distinct ties, and distinct unordered pairs, are independent under the mean field, so these
 * products are exact expectations of the counts:
 *   out[l] = (sum_ij p_ij (P P^T)_ij, sum_ij (P P)_ij p_ji, sum_j cin_j cout_j - sum_ij p_ij p_ji, tr(U^3) / 6,
 *             sum_i (s_i^2 - sum_j u_ij^2) / 2 with s_i = sum_j u_ij, sum_{i<j} u_ij)             host double [L][VMR_TRIAD_NSTAT]
 * They are expectations of COUNTS: a ratio of two of them (a transitivity) is not the expectation of the ratio -- take that from
 * the samples.  Doubles summed by a fixed two-stage tree on a grid that depends on N only (no atomics): bit-identical from run
 * to run.  Temporaries: P and U, 16 L N^2 bytes (VMR_EINVAL when they do not fit).  out NULL: VMR_EINVAL; before vmr_set_state:
 * VMR_ESTATE.  Synchronises. */
int vmr_expected_triads(vmr_handle h, double* out);

/* Mixing by node attribute and overlap between layers of n_samples posterior samples of Y, computed where rho lives -- what a
 * user otherwise gets from `np.add.at` and boolean products in NumPy on every `sample_inferred_model` draw.  Sample s is exactly
 * what vmr_sample(h, seed + s, n_trials, ..) writes (seed + s mod 2^64).  group: host int32 [N], group[i] in [0, C), or -1 for a
 * node that is left out of mix and mutual (it still counts in overlap); skip_diagonal != 0 leaves (i, i) out of all three tables.
 * Host outputs, any of which may be NULL but not all three:
 *   mix[s][l][a][b]     #{(i,j) : g_i = a, g_j = b, Y_lij > 0}                                    uint64 [n_samples][L][C][C]
 *   mutual[s][l][a][b]  #{(i,j) : g_i = a, g_j = b, Y_lij > 0 and Y_lji > 0}, ordered pairs: symmetric in (a, b); a kept
 *                       self-loop counts once, as in vmr_sample_stats                              uint64 [n_samples][L][C][C]
 *   overlap[s][l][l']   #{(i,j) : Y_lij > 0 and Y_l'ij > 0}: symmetric, its diagonal is the edge count   uint64 [n_samples][L][L]
 * group = NULL with C = 0 is allowed when only overlap is asked for.  VMR_EINVAL, with a message that names the argument: C
 * outside [1, VMR_MIX_CMAX] while mix or mutual is asked for (or group NULL then), a label outside [-1, C), L > VMR_MIX_LMAX with
 * overlap asked for, n_samples < 1, n_trials < 1, all three outputs NULL.  Before vmr_set_state: VMR_ESTATE.
 * One workgroup per (strip of 64 rows, sample) walks the strip's tiles with the layers innermost: the L bytes of a tie meet in one
 * thread (ballots and popcounts give the overlap), the transposed tile goes through LDS (mutual), the counters are integers in
 * LDS (per row and layer one LDS atomic instruction, lane b adding the row's edges into group b: at most one add per edge),
 * flushed with 64-bit global integer atomics.  All sums are integer sums: bit-identical from run
 * to run.  Reads the CURRENT rho (after vmr_restore: the snapshot's) once per chunk of samples; any K, both data formats.  A
 * chunk (L N^2 bytes per sample plus the tables; half of the free device memory at most, 256 samples at most, VMR_NETSTATS_CHUNK
 * at most) is freed before return, on every exit path; a single sample that does not fit is refused with VMR_EINVAL.
 * Synchronises. */
#define VMR_MIX_CMAX 64   /* groups at most */
#define VMR_MIX_LMAX 32   /* layers at most when overlap is asked for */
int vmr_sample_mixing(vmr_handle h, uint64_t seed, int n_samples, int n_trials, const int32_t* group, int C, int skip_diagonal,
                      uint64_t* mix, uint64_t* mutual, uint64_t* overlap);

/* The same tables in expectation under q(Y) = prod rho, no sampling: with p_lij = sum_{k>=1} rho_lijk (k ascending, the number
 * of vmr_expected_stats),
 *   mix[l][a][b]     sum_{g_i = a, g_j = b} p_lij                                                  host double [L][C][C]
 *   mutual[l][a][b]  sum_{g_i = a, g_j = b} p_lij p_lji; a kept diagonal enters as p_ii^2, as in vmr_expected_stats   [L][C][C]
 *   overlap[l][l']   sum_ij p_lij p_l'ij for l != l', sum_ij p_lij for l = l'                         host double [L][L]
 * Distinct ties, and distinct layers, are independent under the mean field, so these are exact expectations of the counts (but
 * for the kept diagonal of mutual); a ratio of two of them is not the expectation of the ratio.  Doubles summed in a fixed order
 * -- a wave per row with a fixed shuffle tree per group, then one thread per entry over the rows in ascending i -- on grids that
 * depend on N, L and C only, no atomics: bit-identical from run to run.  Arguments as for vmr_sample_mixing.  Temporaries: P,
 * 8 L N^2 bytes, and the rows' sums, 16 L N C + 8 N L^2 bytes; one that does not fit is refused with VMR_EINVAL.  Synchronises. */
int vmr_expected_mixing(vmr_handle h, const int32_t* group, int C, int skip_diagonal, double* mix, double* mutual, double* overlap);

/* Connectivity of n_samples posterior samples of Y, computed where rho lives -- what a user otherwise gets from
 * `scipy.sparse.csgraph` (connected_components, shortest_path) on every `sample_inferred_model` draw.  Sample s is exactly what
 * vmr_sample(h, seed + s, n_trials, ..) writes (seed + s mod 2^64).  Per sample and layer: A_ij = (Y_ij > 0) with the DIAGONAL
 * CLEARED, U = A | A^T; d(i,j) is the length of a shortest directed path in A, infinite if there is none, d(i,i) = 0.  Weak
 * components are the components of U, strong components the classes of mutual reachability in A.
 * counts: host uint64 [n_samples][L][VMR_CONN_NSTAT]:
 *   0 components_w  weak components, isolated nodes included
 *   1 giant_w       size of the largest weak component
 *   2 pairs_w       #{(i,j), i != j, same weak component} = sum_c n_c (n_c - 1)
 *   3 isolates      nodes of degree 0 in U (a self-loop does not count)
 *   4 components_s  strong components
 *   5 giant_s       size of the largest strong component
 *   6 pairs_s       #{(i,j), i != j, d(i,j) < inf and d(j,i) < inf}
 *   7 reach_pairs   #{(i,j), i != j, d(i,j) < inf}
 *   8 dist_sum      sum of d(i,j) over those pairs
 *   9 diameter      the largest finite d(i,j); 0 when A is empty
 * dist_hist: host uint64 [n_samples][L][VMR_CONN_NDIST]: bin b = d - 1 counts the ordered pairs at distance d, 1 <= d <
 * VMR_CONN_NDIST; the last bin collects every pair at distance >= VMR_CONN_NDIST.  dist_sum and diameter are exact whatever the
 * bins hold.  Node arrays, host int32 [n_samples][L][N]:
 *   node_comp_w, node_comp_s      the smallest node index in the node's weak / strong component
 *   node_reach_out[i] = #{j != i : d(i,j) < inf}      node_reach_in[j] = #{i != j : d(i,j) < inf}
 *   node_dist_out[i] = sum_j d(i,j)                    node_dist_in[j] = sum_i d(i,j), over the reachable pairs only
 *                                                      (at most N (N - 1) / 2 each)
 * dist_hist and every node array may be NULL; counts may not.
 * The samples are packed into the bit rows of vmr_sample_triads; one workgroup per (block of 64 sources, layer, sample) runs a
 * breadth-first search from its 64 sources at once over 64-bit words in LDS (seen, frontier, next frontier: 24 N bytes), three
 * times: over U, A and A^T.  That working set bounds N: N <= VMR_CONN_NMAX = 2048 (48 KiB of LDS per workgroup, three workgroups
 * to a compute unit); a larger N is refused with VMR_EINVAL and a message that names the bound, whatever the state of the
 * handle.  All sums are integer sums, the diameter an integer maximum, the labels integer minima: bit-identical from run to run
 * and for any chunking.  Reads the CURRENT rho (after vmr_restore: the snapshot's) once per chunk of samples; any K, any
 * n_trials >= 1, both data formats.  A chunk (L N^2 + 16 L N ceil(N/64) + 24 L N bytes per sample -- the six node arrays stay on
 * the device whether or not they are asked for -- plus the counts and the histogram when it is asked for; half of the free
 * device memory at most, 256 samples at most, VMR_NETSTATS_CHUNK at most) is freed before return; a single
 * sample that does not fit is refused with VMR_EINVAL.  n_samples < 1, n_trials < 1 or counts NULL: VMR_EINVAL, with a message
 * that names the argument; before vmr_set_state: VMR_ESTATE.  Synchronises. */
#define VMR_CONN_NSTAT 10
#define VMR_CONN_NDIST 64
#define VMR_CONN_NMAX 2048   /* nodes at most */
int vmr_sample_connectivity(vmr_handle h, uint64_t seed, int n_samples, int n_trials, uint64_t* counts, uint64_t* dist_hist,
                            int32_t* node_comp_w, int32_t* node_comp_s, int32_t* node_reach_out, int32_t* node_reach_in,
                            int32_t* node_dist_out, int32_t* node_dist_in);

/* Diffusion centrality of n_samples posterior samples of Y, computed where rho lives -- what a user otherwise gets from
 * `scipy.sparse` matrix-vector products on every `sample_inferred_model` draw.  Sample s is exactly what vmr_sample(h, seed + s,
 * n_trials, ..) writes (seed + s mod 2^64).  Per sample and layer l: A_ij = (Y_ij > 0) with the DIAGONAL CLEARED, and M chosen by
 * direction: VMR_CENT_OUT M = A (walks leave the node: how far its word travels), VMR_CENT_IN M = A^T, VMR_CENT_UNION
 * M = A | A^T.  x_0 = 1, x_t = q_l (M x_{t-1}), c = x_1 + x_2 + .. + x_T added in ascending t: c = sum_{t=1..T} (q_l M)^t 1, the
 * expected number of times a message from the node is heard within T rounds when each tie passes it with probability q_l
 * (Banerjee et al. 2013).  T = 1 is q times the degree; large T with q < 1 / lambda_1 is Katz centrality.
 * rank[v] = #{u : c[u] > c[v]}, strict comparisons of the device's own c: 0 is the most central node, tied nodes share the
 * smaller rank.
 * q: host double [L], each finite and in [0, 1]; T in [1, VMR_CENT_TMAX]; top_k in [1, N].  Host outputs:
 *   node_sum, node_sumsq   sum_s c and sum_s c^2 (the square rounded, then added), in ascending s     double [L][N]
 *   node_rank_sum          sum_s rank                                                                uint64 [L][N]
 *   node_top               #{s : rank < top_k}                                                       uint32 [L][N]
 *   summary                (sum_v c[v] by a fixed tree, max_v c[v])                                  double [n_samples][L][2]
 *   values                 the c of every sample                                                     double [n_samples][L][N]
 * node_sum may not be NULL, every other output may be.
 * The samples are packed into the bit rows of vmr_sample_triads; one workgroup per (layer, sample) keeps x_{t-1} and x_t in LDS
 * (16 N bytes) and re-reads the rows from L2 on each step.  That working set bounds N: N <= VMR_CENT_NMAX = 2048 (32 KiB of LDS
 * per workgroup); a larger N is refused with VMR_EINVAL and a message that names the bound.  A row's sum, the sum over t, the
 * per-node sums over s and the summary's tree have a fixed order and nothing is added with floating-point atomics: every output is
 * bit-identical from run to run and for any chunking.  When q_l = 2^-k and the walk counts are small enough every number is
 * exact.  Reads the CURRENT rho (after vmr_restore: the snapshot's) once per chunk of samples; any K, any n_trials >= 1, both
 * data formats.  A chunk (L N^2 + 16 L N ceil(N/64) + 12 L N bytes per sample plus the summary when asked for, beside 28 L N
 * bytes of per-node accumulators per call; half of the free device memory at most, 256 samples at most, VMR_NETSTATS_CHUNK at
 * most) is freed before return; a single sample that does not fit is refused with VMR_EINVAL.
 * VMR_EINVAL, with a message that names the argument and whatever the state of the handle: N above the bound, direction outside
 * 0..2, T or top_k out of range, q NULL or an entry non-finite or outside [0, 1], node_sum NULL, n_samples < 1, n_trials < 1.
 * Before vmr_set_state: VMR_ESTATE.  Synchronises. */
#define VMR_CENT_OUT 0
#define VMR_CENT_IN 1
#define VMR_CENT_UNION 2
#define VMR_CENT_TMAX 64     /* steps at most */
#define VMR_CENT_NMAX 2048   /* nodes at most (vmr_sample_centrality) */
int vmr_sample_centrality(vmr_handle h, uint64_t seed, int n_samples, int n_trials, const double* q, int T, int direction, int top_k,
                          double* node_sum, double* node_sumsq, uint64_t* node_rank_sum, uint32_t* node_top, double* summary,
                          double* values);

/* The same recursion on the posterior mean network, no sampling: p_ij = sum_{k>=1} rho_ijk (k ascending, the number of
 * vmr_expected_stats), p_ii := 0, and M = P (VMR_CENT_OUT), P^T (VMR_CENT_IN) or U with u_ij = 1 - (1 - p_ij)(1 - p_ji)
 * (VMR_CENT_UNION); out[l] = sum_{t=1..T} (q_l M)^t 1, host double [L][N].
 * What this number is: a PLUG-IN, the centrality of the mean network.  For OUT and IN with T <= 2 it is also the exact
 * expectation of the sampled c: a walk of length <= 2 without self-loops uses distinct ties, and distinct ties are independent
 * under the mean field.  What it is not: for T >= 3 it is not that expectation (a walk i -> j -> i -> j uses a tie twice, and
 * E[a^2] = p, not p^2), and for UNION it is not at any T >= 2 (u_ij and u_ji are one variable).  Take the expectation from
 * vmr_sample_centrality then.
 * Any N: x lives in global memory.  P (or P^T, or U) is formed once -- IN and UNION keep it beside P, written through a transposed
 * tile so that every step reads along rows -- then T batched FP64 matrix-vector steps, a wave per row with a fixed shuffle tree,
 * no atomics, on a grid that depends on N and L only: bit-identical from run to run.  Temporaries: 8 L N^2 bytes, 16 L N^2 for IN
 * and UNION; refused with VMR_EINVAL when they do not fit.  q, T and direction as for vmr_sample_centrality; out NULL:
 * VMR_EINVAL.  Before vmr_set_state: VMR_ESTATE.  Synchronises. */
int vmr_mean_centrality(vmr_handle h, const double* q, int T, int direction, double* out);

/* Betweenness centrality of n_samples posterior samples of Y, computed where rho lives -- what a user otherwise gets from
 * `networkx.betweenness_centrality(normalized=False)` on every `sample_inferred_model` draw.  Sample s is exactly what
 * vmr_sample(h, seed + s, n_trials, ..) writes (seed + s mod 2^64).  Per sample and layer: A_ij = (Y_ij > 0) with the DIAGONAL
 * CLEARED and the search graph G = A (VMR_BTW_DIRECTED) or A | A^T (VMR_BTW_UNION).  With sigma_st the number of shortest s -> t
 * paths in G and sigma_st(v) the number of those through v,
 *   b(v) = sum over s != v != t, s != t, t reachable from s, of sigma_st(v) / sigma_st:
 * unnormalised, endpoints excluded; for UNION the sum over the ordered pairs is halved, so that every unordered pair counts
 * once.  There is no "in" direction: reversing the graph leaves b unchanged.  sigma is carried in FP64 -- exact while it is
 * <= 2^53, and for every power of two beyond; it never wraps; past 1.8e308 it is infinite and b undefined.
 * rank[v] = #{u : b[u] > b[v]}, strict comparisons of the device's own b: 0 is the first broker, tied nodes share the smaller
 * rank.  top_k in [1, N].  Host outputs:
 *   node_sum, node_sumsq   sum_s b and sum_s b^2 (the square rounded, then added), in ascending s     double [L][N]
 *   node_rank_sum          sum_s rank                                                                uint64 [L][N]
 *   node_top               #{s : rank < top_k}                                                       uint32 [L][N]
 *   summary                (sum_v b[v] by a fixed tree, max_v b[v])                                  double [n_samples][L][2]
 *   values                 the b of every sample                                                     double [n_samples][L][N]
 * node_sum may not be NULL, every other output may be.
 * The samples are packed into the bit rows of vmr_sample_triads; one workgroup per (block of 16 consecutive sources, layer,
 * sample) runs Brandes' algorithm by levels with the levels, sigma and delta of one source in LDS (18 N bytes) and reads every
 * bit row three times per source from L2.  That working set bounds N: N <= VMR_BTW_NMAX = 2048; a larger N is refused with
 * VMR_EINVAL and a message that names the bound.  The block of sources depends on N only; a node's neighbours are added in a
 * fixed order, the sources of a block in ascending order, the blocks in ascending order, the samples in ascending s, the total by
 * a fixed tree, and nothing is added with floating-point atomics: every output is bit-identical from run to run and for any
 * chunking.  Every level loop ends after N - 1 levels at the latest.  Reads the CURRENT rho (after vmr_restore: the snapshot's)
 * once per chunk of samples; any K, any n_trials >= 1, both data formats.  A chunk (L N^2 + 16 L N ceil(N/64) +
 * 8 L N ceil(N/16) + 12 L N bytes per sample plus the summary when asked for, beside 28 L N bytes of per-node accumulators per
 * call; half of the free device memory at most, 256 samples at most, VMR_NETSTATS_CHUNK at most) is freed before return; a single
 * sample that does not fit is refused with VMR_EINVAL.
 * VMR_EINVAL, with a message that names the argument and whatever the state of the handle: n_samples < 1, n_trials < 1, N above
 * the bound, direction outside 0..1, top_k out of range, node_sum NULL.  Before vmr_set_state: VMR_ESTATE.  Synchronises. */
#define VMR_BTW_DIRECTED 0
#define VMR_BTW_UNION 1
#define VMR_BTW_NMAX 2048   /* nodes at most */
int vmr_sample_betweenness(vmr_handle h, uint64_t seed, int n_samples, int n_trials, int direction, int top_k, double* node_sum,
                           double* node_sumsq, uint64_t* node_rank_sum, uint32_t* node_top, double* summary, double* values);

/* The same b, by the same packing and the same kernels, of n networks the caller supplies -- the inferred network, a ground
 * truth, a designed graph.  Y: HOST uint8 [n][L][N][N]; an entry > 0 is a tie, the diagonal is ignored.  values: host double
 * [n][L][N].  The handle gives N, L, the device and the stream and nothing else: the call works before vmr_set_state and does not
 * touch rho.  Network q of a call equals what vmr_sample_betweenness returns in `values` for a sample with the same ties, bit
 * for bit.  The networks are uploaded in chunks (the bytes of vmr_sample_betweenness per network, without the ranks).
 * VMR_EINVAL, with a message that names the argument: n < 1, N above VMR_BTW_NMAX, direction outside 0..1, Y or values NULL,
 * a single network whose temporaries do not fit.  Synchronises. */
int vmr_network_betweenness(vmr_handle h, const uint8_t* Y, int n, int direction, double* values);

/* The k-core decomposition of n_samples posterior samples of Y, computed where rho lives -- what a user otherwise gets from
 * `networkx.core_number` on every `sample_inferred_model` draw.  Sample s is exactly what vmr_sample(h, seed + s, n_trials, ..)
 * writes (seed + s mod 2^64).  Per sample and layer: A_ij = (Y_ij > 0) with the DIAGONAL CLEARED.  The k-core is the largest node
 * set in which every node has degree >= k, counted inside the set; core(v) is the largest k whose core holds v, the degeneracy is
 * max_v core(v) and the main core the nodes that attain it.  The degree is chosen by mode:
 *   VMR_CORE_UNION   the distinct neighbours in A | A^T          (`networkx.core_number(G.to_undirected())`)
 *   VMR_CORE_TOTAL   in-degree plus out-degree in A: a reciprocated pair counts 2   (`networkx.core_number` of a DiGraph)
 *   VMR_CORE_IN      the in-degree, VMR_CORE_OUT the out-degree
 * core(v) <= N - 1, and <= 2 (N - 1) for TOTAL: an exact integer, no floating point enters the search.
 * rank[v] = #{u : core[u] > core[v]}: 0 is the innermost shell, and a WHOLE SHELL SHARES A RANK -- every node of the main core
 * has rank 0, so node_top can count more than top_k nodes per sample (all N of them on a regular graph).
 * k_min in [0, 2 (N - 1)]; top_k in [1, N].  Host outputs:
 *   node_sum, node_sumsq   sum_s core and sum_s core^2, in ascending s (integers below 2^53: exact)   double [L][N]
 *   node_rank_sum          sum_s rank                                                                uint64 [L][N]
 *   node_top               #{s : rank < top_k}                                                       uint32 [L][N]
 *   node_main              #{s : core = the sample's degeneracy in that layer}                       uint32 [L][N]
 *   node_atleast           #{s : core >= k_min}                                                      uint32 [L][N]
 *   summary                (degeneracy, main-core size, sum_v core(v), #{v : core(v) >= k_min})      uint32 [n_samples][L][4]
 *   values                 the coreness of every sample                                              uint16 [n_samples][L][N]
 * node_sum may not be NULL, every other output may be.
 * The samples are packed into the bit rows of vmr_sample_triads; one workgroup per (layer, sample) keeps every node's remaining
 * degree and the row of alive nodes in LDS (12.4 KiB whatever N) and peels in rounds: the alive nodes of degree <= k get core = k
 * and leave together, their rows are read once and their alive neighbours lose a degree each (integer LDS atomics); when nobody
 * can leave, k jumps to the smallest remaining degree.  At most 2 N rounds by construction.  That working set bounds N: N <=
 * VMR_CORE_NMAX = 2048; a larger N is refused with VMR_EINVAL and a message that names the bound.  Integer adds commute and the
 * samples are folded in ascending s: every output is bit-identical from run to run and for any chunking.  Reads the CURRENT rho
 * (after vmr_restore: the snapshot's) once per chunk of samples; any K, any n_trials >= 1, both data formats.  A chunk (L N^2 +
 * 16 L N ceil(N/64) + 14 L N + 16 L bytes per sample, whichever outputs are asked for, beside 36 L N bytes of per-node
 * accumulators per call; half of the free device memory at most, 256 samples at most, VMR_NETSTATS_CHUNK at most) is freed before
 * return; a single sample that does not fit is refused with VMR_EINVAL.
 * VMR_EINVAL, with a message that names the call and the argument, whatever the state of the handle: n_samples < 1, n_trials < 1,
 * N above the bound, mode outside 0..3, k_min or top_k out of range, node_sum NULL.  Before vmr_set_state: VMR_ESTATE.
 * Synchronises. */
#define VMR_CORE_UNION 0
#define VMR_CORE_TOTAL 1
#define VMR_CORE_IN 2
#define VMR_CORE_OUT 3
#define VMR_CORE_NMAX 2048   /* nodes at most */
int vmr_sample_cores(vmr_handle h, uint64_t seed, int n_samples, int n_trials, int mode, int k_min, int top_k, double* node_sum,
                     double* node_sumsq, uint64_t* node_rank_sum, uint32_t* node_top, uint32_t* node_main, uint32_t* node_atleast,
                     uint32_t* summary, uint16_t* values);

/* The same coreness, by the same packing and the same kernel, of n networks the caller supplies -- the inferred network, a ground
 * truth, a designed graph.  Y: HOST uint8 [n][L][N][N]; an entry > 0 is a tie, the diagonal is ignored.  values: host uint16
 * [n][L][N]; summary: host uint32 [n][L][4] as above, or NULL.  The handle gives N, L, the device and the stream and nothing
 * else: the call works before vmr_set_state and does not touch rho.  Network q of a call equals what vmr_sample_cores returns in
 * `values` for a sample with the same ties.  The networks are uploaded in chunks (L N^2 + 16 L N ceil(N/64) + 2 L N + 16 L bytes
 * per network).  VMR_EINVAL, with a message that names the call and the argument: n < 1, N above VMR_CORE_NMAX, mode outside
 * 0..3, k_min out of range, Y or values NULL, a single network whose temporaries do not fit.  Synchronises. */
int vmr_network_cores(vmr_handle h, const uint8_t* Y, int n, int mode, int k_min, uint16_t* values, uint32_t* summary);

/* Cascades on n_samples posterior samples of Y, computed where rho lives: the independent-cascade model -- if information enters
 * at a node (or a set of nodes) and every tie passes it on with probability q_l, how many nodes has it reached after T periods?
 * Sample s is exactly what vmr_sample(h, seed + s, n_trials, ..) writes (seed + s mod 2^64).  Per sample and layer l:
 * A = (Y > 0) with the DIAGONAL CLEARED and U = A | A^T.
 * The model, one definition for the four calls.  Cascade k in [0, n_cascades) of network s keeps every tie independently with
 * probability q_l (the live-edge form of the independent-cascade model): tie (l, i, j) is LIVE iff u < q_l, where u is the
 * sampler's 53-bit uniform ((w0 >> 5) 2^26 + (w1 >> 6)) 2^-53 from words 0 and 1 of ONE Philox4x32-10 call with
 *   key     = (cascade_seed + s) mod 2^64, low word first; s is the GLOBAL sample index of the call (never chunk-local), or the
 *             network index for the calls that take the caller's networks;
 *   counter = (t low, t high, k, 1), t the tie's index in [L,N,N] order, t = (l N + i) N + j.  Word 3 = 1 keeps the stream apart
 *             from the sampler's (.., 0) even when cascade_seed == seed.
 * The spread follows A_uv (u informs v) for VMR_CASC_OUT, A_vu for VMR_CASC_IN and U for VMR_CASC_UNION; under UNION the pair
 * {i, j} is ONE variable, drawn at the tie index of (l, min(i, j), max(i, j)), so the live graph is symmetric.  The draw belongs
 * to the tie, not to the direction it is walked in: OUT and IN see the same live ties.
 * active_0 = the seed set; active_t = active_{t-1} + {v : a live tie leads from a node of active_{t-1} to v}.  The OUTREACH after
 * T periods is |active_T| - |active_0|.  q_l = 1 makes every tie live (u < 1 always), q_l = 0 none.  Nothing is floating-point
 * except the one comparison u < q_l, whose operands are exact on both sides: every output is an exact integer (node_sum and
 * node_sumsq are sums of quotients of two integers).
 * q: host double [L], each finite and in [0, 1]; T in [1, VMR_CASC_TMAX]; n_cascades in [1, VMR_CASC_KMAX] (a uint32 total cannot
 * wrap: 65536 * 2047 < 2^32); direction in 0..2; N <= VMR_CASC_NMAX = 2048, the 24 N bytes of LDS of the connectivity closure
 * (seen, frontier, next frontier: 48 KiB).
 *
 * vmr_sample_outreach: every node as a single seed.  Host outputs:
 *   values                 sum_k outreach of {v} in cascade k                                         uint32 [n_samples][L][N]
 *   summary                (sum_v values mod 2^32 -- exact while n_cascades N (N - 1) < 2^32 --, max_v values)   uint32 [n_samples][L][2]
 *   node_sum, node_sumsq   sum_s c and sum_s c^2 (the square rounded, then added), in ascending s, c = values / n_cascades: one
 *                          FP64 division of two integers                                             double [L][N]
 *   node_rank_sum          sum_s rank, rank[v] = #{u : c[u] > c[v]}: 0 is the best entry point, tied nodes share the smaller
 *                          rank (c is monotone in values and distinct values give distinct c: the integers are compared)   uint64 [L][N]
 *   node_top               #{s : rank < top_k}, top_k in [1, N]                                       uint32 [L][N]
 * node_sum may not be NULL, every other output may be.
 * vmr_sample_seed_outreach: n_sets in [1, VMR_CASC_SETS] seed sets at once.  seed_words: HOST uint64 [N], shared by the layers:
 * bit b of word v is set iff node v is in set b; a bit at or above n_sets is refused.  A set may be empty or hold every node.
 *   values      sum_k outreach of set b                                                  uint32 [n_samples][L][n_sets], not NULL
 *   curve       bin t - 1: the nodes newly reached at period t, summed over samples and cascades; the last bin collects every
 *               period >= VMR_CASC_NPER, so a set's bins sum to its total outreach whatever T is   uint64 [L][n_sets][VMR_CASC_NPER] or NULL
 *   node_hits   #{(s, k) : v in active_T}, seeds included (n_samples n_cascades < 2^32 is the caller's)   uint32 [L][n_sets][N] or NULL
 * The kernels.  The samples are packed into the bit rows of vmr_sample_triads.  Per cascade, one pass over the chunk's bit rows
 * (a thread per word, one Philox call per set bit) writes the LIVE rows of the one row set the closure walks; then a breadth-first
 * search over 64-bit words in LDS, at most T levels.  Every node as a seed: one workgroup per (block of 64 sources, layer, sample)
 * walks the live rows of the direction OPPOSITE to the spread, so that popc(seen[v]) - [v in the block] is v's own outreach
 * towards the block's nodes; one integer add per node at its end.  Seed sets: one workgroup per (layer, sample) starts from
 * seed_words and walks along the spread; a period's new bits are counted per set with integer LDS atomics.  Only integers are
 * added, the samples are folded in ascending s: every output is identical from run to run and for any chunking.  Reads the
 * CURRENT rho once per chunk of samples; any K, any n_trials >= 1, both data formats.  A chunk (vmr_sample_outreach: L N^2 +
 * 24 L N ceil(N/64) + 16 L N + 8 L bytes per sample beside 28 L N + 8 L bytes per call; vmr_sample_seed_outreach: L N^2 +
 * 24 L N ceil(N/64) + 4 L n_sets bytes per sample beside 8 N + 8 L + 512 L n_sets + 4 L n_sets N per call; half of the free
 * device memory at most, 256 samples at most, VMR_NETSTATS_CHUNK at most) is freed before return; a single sample that does not
 * fit is refused with VMR_EINVAL.
 * VMR_EINVAL, with a message that names the call and the argument, whatever the state of the handle: n_samples < 1, n_trials < 1,
 * N above the bound, direction, T, n_cascades, n_sets or top_k out of range, q NULL or an entry non-finite or outside [0, 1], a
 * seed bit at or above n_sets, seed_words NULL, a required output NULL.  Before vmr_set_state: VMR_ESTATE.  Synchronises. */
#define VMR_CASC_OUT 0
#define VMR_CASC_IN 1
#define VMR_CASC_UNION 2
#define VMR_CASC_NMAX 2048    /* nodes at most */
#define VMR_CASC_TMAX 65535   /* periods at most */
#define VMR_CASC_KMAX 65536   /* cascades per network at most */
#define VMR_CASC_SETS 64      /* seed sets per call at most */
#define VMR_CASC_NPER 64      /* period bins of the curve */
int vmr_sample_outreach(vmr_handle h, uint64_t seed, int n_samples, int n_trials, uint64_t cascade_seed, int n_cascades, const double* q, int T,
                        int direction, int top_k, double* node_sum, double* node_sumsq, uint64_t* node_rank_sum, uint32_t* node_top,
                        uint32_t* summary, uint32_t* values);
int vmr_sample_seed_outreach(vmr_handle h, uint64_t seed, int n_samples, int n_trials, uint64_t cascade_seed, int n_cascades, const double* q,
                             int T, int direction, const uint64_t* seed_words, int n_sets, uint32_t* values, uint64_t* curve,
                             uint32_t* node_hits);

/* The same numbers, by the same packing and the same kernels, of n networks the caller supplies -- the inferred network, a ground
 * truth, a designed graph.  Y: HOST uint8 [n][L][N][N]; an entry > 0 is a tie, the diagonal is ignored.  Network q of a call
 * equals a sample with the same ties and s = q: its key is (cascade_seed + q) mod 2^64.  values, summary, curve and node_hits as
 * above with n in place of n_samples; values may not be NULL, the others may.  The handle gives N, L, the device and the stream
 * and nothing else: the calls work before vmr_set_state and do not touch rho.  The networks are uploaded in chunks (the bytes
 * above per network, without the 12 L N of c and the ranks).  VMR_EINVAL, with a message that names the call and the argument:
 * n < 1, N above VMR_CASC_NMAX, direction, T, n_cascades or n_sets out of range, q as above, a seed bit at or above n_sets, Y,
 * seed_words or values NULL, a single network whose temporaries do not fit.  Synchronise. */
int vmr_network_outreach(vmr_handle h, const uint8_t* Y, int n, uint64_t cascade_seed, int n_cascades, const double* q, int T, int direction,
                         uint32_t* values, uint32_t* summary);
int vmr_network_seed_outreach(vmr_handle h, const uint8_t* Y, int n, uint64_t cascade_seed, int n_cascades, const double* q, int T, int direction,
                              const uint64_t* seed_words, int n_sets, uint32_t* values, uint64_t* curve, uint32_t* node_hits);

/* The Holland-Leinhardt triad census of n_samples posterior samples of Y, computed where rho lives -- what a user otherwise gets
 * from `networkx.triadic_census` (`sna::triad.census`, `igraph_triad_census`) on every `sample_inferred_model` draw.  Sample s is
 * exactly what vmr_sample(h, seed + s, n_trials, ..) writes (seed + s mod 2^64).  Per sample and layer: A_ij = (Y_ij > 0) with the
 * DIAGONAL CLEARED, and every unordered triple of distinct nodes is counted in the one of the 16 isomorphism classes of its
 * induced subgraph.  A class is named by its mutual, asymmetric and null dyads and a letter; in the order of the output, which is
 * networkx's:
 *    0 003                      4 021U  a -> b <- c           8 030T  a -> b <- c, a -> c      12 120U  a -> b <- c, a <-> c
 *    1 012   a -> b             5 021C  a -> b -> c           9 030C  a -> b -> c -> a         13 120C  a -> b -> c, a <-> c
 *    2 102   a <-> b            6 111D  a <-> b <- c         10 201   a <-> b <-> c            14 210   a -> b <-> c, a <-> c
 *    3 021D  a <- b -> c        7 111U  a <-> b -> c         11 120D  a <- b -> c, a <-> c     15 300   all three mutual
 * counts: host uint64 [n_samples][L][VMR_CENSUS_NCLASS]; the 16 numbers of a sample and layer sum to C(N, 3).  N < 3 is legal and
 * gives zeros.  Exact integers: for every connected pair i < j the thirds k are counted by the popcounts of the 15 combinations
 * of (the state of k seen from i, the state seen from j) other than (none, none), the thirds tied to neither are N - 2 - their
 * sum, a triad found from each of its c connected dyads is divided by c, and 003 is what is left of C(N, 3).  The work is
 * proportional to ties x ceil(N / 64); any N the handle has.  Integer adds commute: every output is identical from run to run and
 * for any chunking.  The samples are packed into the bit rows of vmr_sample_triads.  Reads the CURRENT rho (after vmr_restore:
 * the snapshot's) once per chunk of samples; any K, any n_trials >= 1, both data formats.  A chunk (L N^2 + 16 L N ceil(N/64) +
 * 128 L bytes per sample; half of the free device memory at most, 256 samples at most, VMR_NETSTATS_CHUNK at most) is freed before
 * return; a single sample that does not fit is refused with VMR_EINVAL.
 * VMR_EINVAL, with a message that names the call and the argument, whatever the state of the handle: n_samples < 1, n_trials < 1,
 * counts NULL.  Before vmr_set_state: VMR_ESTATE.  Synchronises. */
#define VMR_CENSUS_NCLASS 16   /* 003 012 102 021D 021U 021C 111D 111U 030T 030C 201 120D 120U 120C 210 300 (networkx's order and naming) */
int vmr_sample_triad_census(vmr_handle h, uint64_t seed, int n_samples, int n_trials, uint64_t* counts /* [n_samples][L][16] */);

/* The same census, by the same packing and the same kernel, of n networks the caller supplies -- the inferred network, a ground
 * truth, a designed graph.  Y: HOST uint8 [n][L][N][N]; an entry > 0 is a tie, the diagonal is ignored.  counts: host uint64
 * [n][L][VMR_CENSUS_NCLASS].  The handle gives N, L, the device and the stream and nothing else: the call works before
 * vmr_set_state and does not touch rho.  Network q of a call equals what vmr_sample_triad_census returns for a sample with the
 * same ties.  The networks are uploaded in chunks (L N^2 + 16 L N ceil(N/64) + 128 L bytes per network).  VMR_EINVAL, with a
 * message that names the call and the argument: n < 1, Y or counts NULL, a single network whose temporaries do not fit.
 * Synchronises. */
int vmr_network_triad_census(vmr_handle h, const uint8_t* Y /* host [n][L][N][N] */, int n, uint64_t* counts /* [n][L][16] */);

/* Shared partners of the ties of n_samples posterior samples of Y, computed where rho lives: the posterior TIE BY TIE -- the
 * support of Jackson, Rodriguez-Barraquer and Tan (the share of ties whose two ends have a partner in common), the embeddedness
 * of every tie, the local bridges (ties with no common partner), Krackhardt's Simmelian ties and the edgewise-shared-partner
 * distribution behind GWESP.  Sample s is exactly what vmr_sample(h, seed + s, n_trials, ..) writes (seed + s mod 2^64).  Per
 * sample and layer A_ij = (Y_ij > 0) with the DIAGONAL CLEARED, and `mode` names the ties that are counted and their partners:
 *   VMR_SP_UNION    unordered pairs i < j tied either way    k tied (either way) to i and to j
 *   VMR_SP_MUTUAL   unordered pairs tied both ways           k tied both ways to both (a Simmelian tie has one)
 *   VMR_SP_PATH     ordered ties i -> j                      k with i -> k -> j: the tie closes a two-path (transitive embeddedness)
 * A partner is neither i nor j.  Outputs, host memory:
 *   hist    uint64 [n_samples][L][n_bins]   the ties with exactly b partners; the LAST bin holds those with n_bins - 1 or more
 *   totals  uint64 [n_samples][L][VMR_SP_NTOTAL]   ties, supported ties (>= 1 partner), the partners summed over the ties, the
 *           largest partner count of a tie
 *   node_ties, node_supported   int32 [n_samples][L][N], each optional (NULL) and independent of the other: the counted ties
 *           node v is an end of, and those of them with >= 1 partner (in path mode i -> j and j -> i are two ties of both nodes)
 *   pairs   int32 [n_pairs][3] = (layer, i, j), i != j, or NULL with n_pairs = 0: ties to follow over the samples.  In union and
 *           mutual mode (i, j) and (j, i) name the same tie; a pair may be listed more than once.  Per listed pair:
 *           pair_present uint32 [n_pairs] the samples in which it is a counted tie, pair_supported uint32 [n_pairs] those in
 *           which it also has >= 1 partner, pair_partners uint64 [n_pairs] its partners summed over the samples in which it is a
 *           tie.  Required when n_pairs > 0, untouched otherwise.
 * The partners of (i, j) are popcounts of two bit rows, popc(P_i & Q_j) over ceil(N / 64) words: the work is proportional to
 * ties x ceil(N / 64), integers only, any N the handle has; N < 3 is legal and no tie has a partner.  Every output is an exact
 * integer, identical from run to run and for any chunking (integer adds and an integer maximum; 64-bit beyond a workgroup).  The
 * samples are packed into the bit rows of vmr_sample_triads.  Reads the CURRENT rho (after vmr_restore: the snapshot's) once per
 * chunk of samples; any K, any n_trials >= 1, both data formats.  A chunk (L N^2 + 16 L N ceil(N/64) + 8 L (n_bins + 4) bytes per
 * sample, + 4 L N per node array; half of the free device memory at most, 256 samples at most, VMR_NETSTATS_CHUNK at most) and
 * the pairs with their accumulators (28 n_pairs bytes per call) are freed before return; a single sample that does not fit is
 * refused with VMR_EINVAL.
 * VMR_EINVAL, with a message that names the call and the argument, whatever the state of the handle: n_samples < 1, n_trials < 1,
 * mode outside 0..2, n_bins outside [2, VMR_SP_MAX_BINS], hist or totals NULL, n_pairs < 0, pairs or a pair output NULL with
 * n_pairs > 0, a pair whose layer or node is out of range or with i == j (checked on the host before any launch).  Before
 * vmr_set_state: VMR_ESTATE.  Synchronises. */
#define VMR_SP_UNION 0
#define VMR_SP_MUTUAL 1
#define VMR_SP_PATH 2
#define VMR_SP_MAX_BINS 1024
#define VMR_SP_NTOTAL 4    /* ties, supported ties (>= 1 partner), sum of partners over ties, largest partner count */
int vmr_sample_shared_partners(vmr_handle h, uint64_t seed, int n_samples, int n_trials, int mode, int n_bins,
                               uint64_t* hist,            /* [n_samples][L][n_bins] */
                               uint64_t* totals,          /* [n_samples][L][4] */
                               int32_t* node_ties,        /* [n_samples][L][N] or NULL */
                               int32_t* node_supported,   /* [n_samples][L][N] or NULL */
                               const int32_t* pairs, int n_pairs,   /* [n_pairs][3] = (layer, i, j), or NULL / 0 */
                               uint32_t* pair_present, uint32_t* pair_supported, uint64_t* pair_partners /* [n_pairs] each */);

/* The same counts, by the same packing and the same kernels, of n networks the caller supplies -- the inferred network, a ground
 * truth, a designed graph.  Y: HOST uint8 [n][L][N][N]; an entry > 0 is a tie, the diagonal is ignored.  hist [n][L][n_bins],
 * totals [n][L][4] and the node arrays [n][L][N] as above.  pair_partners: host int32 [n][n_pairs], the partners of every listed
 * pair in every network, -1 where the pair is not a counted tie; required when n_pairs > 0.  The handle gives N, L, the device
 * and the stream and nothing else: the call works before vmr_set_state and does not touch rho.  Network q of a call equals what
 * vmr_sample_shared_partners returns for a sample with the same ties.  The networks are uploaded in chunks (the bytes above + 4
 * n_pairs per network).  VMR_EINVAL, with a message that names the call and the argument: n < 1, Y NULL, and the cases above but
 * n_samples and n_trials; a single network whose temporaries do not fit.  Synchronises. */
int vmr_network_shared_partners(vmr_handle h, const uint8_t* Y /* host [n][L][N][N] */, int n, int mode, int n_bins, uint64_t* hist,
                                uint64_t* totals, int32_t* node_ties, int32_t* node_supported, const int32_t* pairs, int n_pairs,
                                int32_t* pair_partners /* [n][n_pairs]: partners, -1 where not a tie */);

/* Burt's structural holes of n_samples posterior samples of Y, computed where rho lives: the posterior NODE BY NODE as an ego
 * network -- whose own contacts are disconnected from one another -- what a user otherwise gets from `networkx.effective_size`
 * and `networkx.constraint` on every `sample_inferred_model` draw.  Sample s is exactly what vmr_sample(h, seed + s, n_trials, ..)
 * writes (seed + s mod 2^64).  Per sample and layer A = (Y > 0) with the DIAGONAL CLEARED, U = A | A^T, Mu = A & A^T, and `mode`
 * names the weights z:
 *   VMR_SH_UNION     z_ij = U_ij: the symmetrised binary network -- networkx on `G.to_undirected()`
 *   VMR_SH_WEIGHTED  z_ij = A_ij + A_ji = U_ij + Mu_ij in {0, 1, 2}: Burt's mutual weights on the directed network -- networkx on
 *                    the DiGraph, which reports NaN for a node without out-ties whatever its in-ties; here only isolates are undefined
 * For node i: the degree d_i = sum_j U_ij, the strength s_i = sum_j z_ij, p_ij = z_ij / s_i, and mx_j = max_x z_jx, which is 2
 * exactly when j has a mutual tie in weighted mode (s_j > d_j) and 1 otherwise.  The measures:
 *   redundancy numerator  R_i = sum_{j in U_i} f_j sum_q z_iq z_jq, f_j = 2 / mx_j in {1, 2}: an exact integer, <= 2 s_i (d_i - 1)
 *   effective size        ES_i = d_i - R_i / (2 s_i), evaluated as (2 s_i d_i - R_i) / (2 s_i): the numerator is an exact integer,
 *                         so ES is the correctly rounded value of the rational and a host reproduces it from (d, s, R) with ==.
 *                         Union mode: Borgatti's n - 2 t / n; weighted mode: Burt's sum_j (1 - sum_q p_iq m_jq), m_jq = z_jq / mx_j
 *   constraint            c_i = sum_{j in U_i} ((z_ij + sum_{q in U_i & U_j} z_iq z_qj / s_q) / s_i)^2, every operation rounded as
 *                         written (no contraction); the sums in an order that depends on N only
 *   efficiency            ES_i / d_i is left to the caller
 * A node with d_i = 0 is UNDEFINED: both measures are stored as 0.0 and the caller masks them by the degree.  Ranks are taken
 * among the defined nodes: by effective size rank_v = #{defined u : ES_u > ES_v}, by constraint rank_v = #{defined u : c_u < c_v}
 * (0: the first broker; equal values share the smaller rank); an undefined node gets rank = #defined.  Outputs, host memory; index
 * 0 of the leading [2] is the effective size, 1 the constraint:
 *   node_sum, node_sumsq   sum_s value and sum_s value^2 (the square rounded before it is added), ascending s   double [2][L][N]
 *   node_rank_sum          sum_s rank                                                                          uint64 [2][L][N]
 *   node_top               #{s : rank < top_k}                                                                 uint32 [2][L][N]
 *   node_defined           #{s : d > 0}: the samples in which the node is not isolated                         uint32 [L][N]
 *   summary                (#defined, sum_v ES_v, sum_v c_v) over the defined nodes                             double [n_samples][L][3]
 *   degree, strength       d and s                                                                             int32 [n_samples][L][N]
 *   redundancy             R                                                                                   uint64 [n_samples][L][N]
 *   effective_size, constraint   the two measures of every sample                                              double [n_samples][L][N]
 * node_sum may not be NULL, every other output may be, each on its own.
 * The samples are packed into the bit rows of vmr_sample_triads.  One wave per (node, layer, sample) lists the node's neighbours
 * and walks their rows: the integers are popcounts, the FP64 sum of a pair walks the common neighbours in ascending order; no
 * atomics, a node is owned by one wave.  The work is proportional to ties x ceil(N / 64) plus the common neighbours, the ranks are
 * N^2 comparisons out of LDS; any N the handle has.  Every output is bit-identical from run to run and for any chunking.  Reads
 * the CURRENT rho (after vmr_restore: the snapshot's) once per chunk of samples; any K, any n_trials >= 1, both data formats.  A
 * chunk (L N^2 + 16 L N ceil(N/64) + 40 L N + 24 L bytes per sample, whichever outputs are asked for, beside 60 L N bytes of
 * per-node accumulators per call; half of the free device memory at most, 256 samples at most, VMR_NETSTATS_CHUNK at most) is
 * freed before return; a single sample that does not fit is refused with VMR_EINVAL.
 * VMR_EINVAL, with a message that names the call and the argument, whatever the state of the handle: n_samples < 1, n_trials < 1,
 * mode outside 0..1, top_k outside [1, N], node_sum NULL.  Before vmr_set_state: VMR_ESTATE.  Synchronises. */
#define VMR_SH_UNION 0
#define VMR_SH_WEIGHTED 1
#define VMR_SH_NSUMMARY 3   /* defined nodes, sum of their effective sizes, sum of their constraints */
int vmr_sample_structural_holes(vmr_handle h, uint64_t seed, int n_samples, int n_trials, int mode, int top_k,
                                double* node_sum /* [2][L][N]: effective size, constraint; required */, double* node_sumsq,
                                uint64_t* node_rank_sum, uint32_t* node_top /* [2][L][N] each, or NULL */,
                                uint32_t* node_defined /* [L][N] */, double* summary /* [n_samples][L][3] */, int32_t* degree,
                                int32_t* strength, uint64_t* redundancy, double* effective_size,
                                double* constraint /* [n_samples][L][N] each, or NULL */);

/* The same measures, by the same packing and the same kernels, of n networks the caller supplies -- the inferred network, a
 * ground truth, a designed graph.  Y: HOST uint8 [n][L][N][N]; an entry > 0 is a tie, the diagonal is ignored.  effective_size,
 * constraint: host double [n][L][N], required; degree, strength int32 [n][L][N], redundancy uint64 [n][L][N], summary double
 * [n][L][3] as above, or NULL.  The handle gives N, L, the device and the stream and nothing else: the call works before
 * vmr_set_state and does not touch rho.  Network q of a call equals, bit for bit, what vmr_sample_structural_holes returns for a
 * sample with the same ties.  The networks are uploaded in chunks (L N^2 + 16 L N ceil(N/64) + 24 L N bytes per network, + 8 L N
 * with redundancy, + 24 L with summary).  VMR_EINVAL, with a message that names the call and the argument: n < 1, mode outside
 * 0..1, Y, effective_size or constraint NULL, a single network whose temporaries do not fit.  Synchronises. */
int vmr_network_structural_holes(vmr_handle h, const uint8_t* Y /* host [n][L][N][N] */, int n, int mode, double* effective_size,
                                 double* constraint /* [n][L][N], required */, int32_t* degree, int32_t* strength,
                                 uint64_t* redundancy, double* summary /* or NULL */);

/* Who holds the network together: the cut points, the bridges and Borgatti's key-player fragmentation of n_samples posterior
 * samples of Y, computed where rho lives -- what a user otherwise gets from `networkx.articulation_points`, `networkx.bridges` and
 * one component search per removed node on every `sample_inferred_model` draw.  Sample s is exactly what vmr_sample(h, seed + s,
 * n_trials, ..) writes (seed + s mod 2^64).  Per sample and layer: A_ij = (Y_ij > 0) with the DIAGONAL CLEARED, and G the
 * undirected simple graph chosen by mode:
 *   VMR_CUT_UNION    a tie either way, A | A^T   (networkx on `G.to_undirected()`)
 *   VMR_CUT_MUTUAL   a tie both ways, A & A^T    (the reciprocated network, the one the model's mutuality speaks about)
 * For node v let C(v) be its component in G; the BRANCHES of v are the components of C(v) with v removed, of sizes s_1..s_b.
 *   branches[v]    b; 0 for an isolate; v is a CUT POINT iff b >= 2
 *   pairs_cut[v]   sum_{i<j} s_i s_j = ((sum_i s_i)^2 - sum_i s_i^2) / 2: the unordered pairs of OTHER nodes that are connected
 *                  in G and no longer connected once v is taken out; at most C(2047, 2): it fits 32 bits
 *   bridges[v]     the branches that hold exactly one neighbour of v: the tie {v, u} is a bridge of G (the only connection
 *                  between two parts; global, not the local bridges of vmr_sample_shared_partners) iff u is the only neighbour
 *                  of v in its branch.  sum_v bridges[v] = 2 x the number of bridges
 *   rank[v]        #{u : pairs_cut[u] > pairs_cut[v]}: 0 is the node whose removal cuts most, and ALL NON-CUT NODES SHARE A
 *                  RANK (their pairs_cut is 0) -- as a shell does in vmr_sample_cores, so node_top can count more than top_k
 *                  nodes per sample (all N of them on a graph without cut points)
 * Exact integers: no floating point enters the search.  top_k in [1, N].  Host outputs:
 *   node_sum, node_sumsq   sum_s pairs_cut and sum_s pairs_cut^2, in ascending s (integers below 2^53: exact)   double [L][N]
 *   node_rank_sum          sum_s rank                                                                uint64 [L][N]
 *   node_top               #{s : rank < top_k}                                                       uint32 [L][N]
 *   node_cut               #{s : branches >= 2}                                                      uint32 [L][N]
 *   node_branch_sum        sum_s branches                                                            uint64 [L][N]
 *   node_bridge_sum        sum_s bridges                                                             uint64 [L][N]
 *   summary                (cut points, bridges, max_v pairs_cut, the connected unordered pairs of G =
 *                          sum over the components of C(|C|, 2) = sum_v sum_i s_i(v) / 2)            uint32 [n_samples][L][4]
 *   pairs_cut              of every sample                                                           uint32 [n_samples][L][N]
 *   branches, bridges      of every sample                                                           uint16 [n_samples][L][N]
 * node_sum may not be NULL, every other output may be.  pairs_cut over the summary's connected pairs is the share of the
 * sample's connected pairs that the removal of v disconnects.
 * The samples are packed into the bit rows of vmr_sample_triads and G is formed from them once per chunk.  One workgroup per
 * (block of 64 nodes, layer, sample) runs the 64 removal experiments of its block at once with the 64-source breadth-first search
 * of vmr_sample_connectivity: node u carries a 64-bit word in LDS whose bit q belongs to the experiment "node 64 b + q has been
 * removed"; the removed node starts as seen in its own experiment and is never expanded.  The branches are found in rounds: every
 * experiment with an unvisited neighbour of its removed node seeds the lowest-numbered one (an integer LDS atomic minimum), the
 * search runs to closure for all 64 experiments, and the nodes the round reached are counted per experiment.  seen, the frontier
 * and the next frontier take 24 N bytes of LDS, which bounds N: N <= VMR_CUT_NMAX = 2048; a larger N is refused with VMR_EINVAL
 * and a message that names the bound.  Integer adds, minima and ORs only, and the samples are folded in ascending s: every
 * output is bit-identical from run to run and for any chunking.  Reads the CURRENT rho (after vmr_restore: the snapshot's) once
 * per chunk of samples; any K, any n_trials >= 1, both data formats.  A chunk (L N^2 + 24 L N ceil(N/64) + 22 L N + 16 L bytes
 * per sample, whichever outputs are asked for, beside 48 L N bytes of per-node accumulators per call; half of the free device
 * memory at most, 256 samples at most, VMR_NETSTATS_CHUNK at most) is freed before return; a single sample that does not fit is
 * refused with VMR_EINVAL.
 * VMR_EINVAL, with a message that names the call and the argument, whatever the state of the handle: n_samples < 1, n_trials < 1,
 * N above the bound, mode outside 0..1, top_k out of range, node_sum NULL.  Before vmr_set_state: VMR_ESTATE.  Synchronises. */
#define VMR_CUT_UNION 0
#define VMR_CUT_MUTUAL 1
#define VMR_CUT_NMAX 2048   /* nodes at most */
int vmr_sample_cutpoints(vmr_handle h, uint64_t seed, int n_samples, int n_trials, int mode, int top_k, double* node_sum,
                         double* node_sumsq, uint64_t* node_rank_sum, uint32_t* node_top, uint32_t* node_cut, uint64_t* node_branch_sum,
                         uint64_t* node_bridge_sum, uint32_t* summary, uint32_t* pairs_cut, uint16_t* branches, uint16_t* bridges);

/* The same numbers, by the same packing and the same kernels, of n networks the caller supplies -- the inferred network, a ground
 * truth, a designed graph.  Y: HOST uint8 [n][L][N][N]; an entry > 0 is a tie, the diagonal is ignored.  pairs_cut: host uint32
 * [n][L][N], required; branches, bridges: host uint16 [n][L][N], summary: host uint32 [n][L][4] as above, or NULL.  The handle
 * gives N, L, the device and the stream and nothing else: the call works before vmr_set_state and does not touch rho.  Network q
 * of a call equals what vmr_sample_cutpoints returns for a sample with the same ties.  The networks are uploaded in chunks (L N^2
 * + 24 L N ceil(N/64) + 10 L N + 16 L bytes per network).  VMR_EINVAL, with a message that names the call and the argument: n <
 * 1, N above VMR_CUT_NMAX, mode outside 0..1, Y or pairs_cut NULL, a single network whose temporaries do not fit.  Synchronises. */
int vmr_network_cutpoints(vmr_handle h, const uint8_t* Y, int n, int mode, uint32_t* pairs_cut, uint16_t* branches, uint16_t* bridges,
                          uint32_t* summary);

/* Posterior predictive checks: n_rep replicated datasets drawn from the fitted model over the support of the handle's own R and
 * reduced where they are drawn -- no replicate is ever written -- and the same reduction of the observed data.
 * Replicate r: Y_r is exactly what vmr_sample(h, seed_y + r, n_trials, ..) writes (mod 2^64; the CURRENT rho, after vmr_restore
 * the snapshot's); lam[l,i,j] = lambda[r][l][Y_r[l,i,j]] (the table as given, per layer); for every unordered pair i < j, layer l
 * and reporter m with R[l,i,j,m] != 0 or R[l,j,i,m] != 0 the pair draw of vmr_generate_x with seed seed_x + r, rates
 * lam[l,i,j] theta[r][l][m] and lam[l,j,i] theta[r][l][m], and eta[r]: the numbers vmr_generate_x(lam_dev = lam, theta[r], eta[r],
 * seed_x + r) puts at (l,i,j,m) and (l,j,i,m), not clamped.  A direction whose own R entry is 0 is dropped; a draw depends on
 * (seed, l, i, j, m) only.  Diagonal ties hold no replicated report.  S and "without R" as for vmr_mean_poisson.
 * counts: host uint64 [n_rep][L][VMR_PPC_NSTAT], exact integer sums over S of a layer (x: the count at a support element):
 *   0 n_pos          #{S : x > 0}
 *   1 total          sum x
 *   2 sumsq          sum x^2
 *   3 mutual         #{(i,j,m) in S, i != j : x_ijm > 0, (j,i,m) in S and x_jim > 0}   (ordered: a reciprocated pair counts twice)
 *   4 ties_reported  #{(i,j) : some m in S with x > 0}                                  (the union baseline)
 *   5 ties_agreed    #{(i,j) : at least two m in S with x > 0}                          (the intersection of the self-reporter setting)
 * by_reporter: host uint64 [n_rep][L][M][2], (n_pos, total) of every reporter, or NULL.  theta [n_rep][L][M], lambda [n_rep][L][K],
 * eta [n_rep] are host arrays.  Any K, any n_trials >= 1, both data formats, every mask layout, handles of vmr_create_coo.
 * A chunk of replicates keeps L N^2 bytes of Y per replicate on the device (half of the free memory at most, 256 replicates at
 * most; freed before return; VMR_EINVAL when one does not fit).  VMR_EINVAL before any launch: n_rep < 1, n_trials < 1, a NULL
 * theta / lambda / eta / counts, an eta outside [0, 1), a negative or non-finite theta or lambda.  VMR_ESTATE before
 * vmr_set_state.  Bit-identical from run to run.  Synchronises.
 * vmr_ppc_observed: the same statistics of the handle's own X over S (counts [L][VMR_PPC_NSTAT], by_reporter [L][M][2] or NULL);
 * observed diagonal counts enter where S holds the diagonal.  Report-list handles: the temporaries of vmr_mean_poisson. */
#define VMR_PPC_NSTAT 6
int vmr_ppc_replicates(vmr_handle h, int n_rep, uint64_t seed_y, uint64_t seed_x, int n_trials, const double* theta,
                       const double* lambda, const double* eta, uint64_t* counts, uint64_t* by_reporter);
int vmr_ppc_observed(vmr_handle h, uint64_t* counts, uint64_t* by_reporter);

/* The inferred network as an edge table, built on the device -- the edge list of the reference's experiment driver
 * (notebooks/python/experiments/karnataka.py:200-318: the thresholded posterior beside the union and intersection baselines) for
 * any K and any mask, instead of `get_inferred_model`'s dense [L,N,N] array (model.py:1099-1188) and the 8 L N^2 K bytes of rho.
 * Per tie t = (l,i,j), from the handle's own X and R and the CURRENT rho (after vmr_restore: the snapshot's):
 *   y        the byte vmr_readout(h, method, threshold, ..) writes for the tie; method VMR_READ_RHO_MAX or VMR_READ_THRESHOLD
 *            (VMR_READ_RHO_MEAN: VMR_EINVAL)
 *   prob     sum_{k>=1} rho_k, added in ascending k as in vmr_expected_stats (K = 2: the double rho_1, bit for bit)
 *   mean     sum_k k rho_k, k ascending, every product and every sum rounded on its own (NumPy's loop; VMR_READ_RHO_MEAN's value up
 *            to the rounding of a fused multiply-add)
 *   n_rep    #{m : X[l,i,j,m] > 0}              total    sum_m X[l,i,j,m]
 *   n_mask   #{m : R[l,i,j,m] != 0} (M without R)
 *   ego      X[l,i,j,i], 0 where i >= M          alter    X[l,i,j,j], 0 where j >= M
 *   y_T, n_rep_T, total_T   y, n_rep, total of the mirror tie (l,j,i); a diagonal tie is its own mirror
 * n_rep, total, ego and alter are over ALL reporters, R ignored -- the driver's np.sum(X, axis=3) -- unlike the statistics of
 * vmr_ppc_observed, which are over the support of R.
 * A tie is a row iff (select & VMR_EDGE_REPORTED and n_rep > 0) or (select & VMR_EDGE_INFERRED and y > 0); select is 1, 2 or 3.
 * Rows come in lexicographic (l,i,j) order, np.nonzero's; layer < 0: every layer, else that one.  vmr_edge_table_size gives the
 * row count; n is the capacity of the outputs (VMR_EINVAL below the row count, before anything is written); any output pointer
 * may be NULL; device pointers when out_on_device != 0.  Any K, both data formats, every mask layout, handles of vmr_create_coo;
 * fewer than 2^31 ties per layer.  Integer reductions and per-lane sums only: bit-identical from run to run.  VMR_ESTATE before
 * vmr_set_state.  Synchronise; temporaries (report-list handles: the tie-major index of vmr_mean_poisson and the tie -> position
 * table; 20 B per tie of a layer; host outputs: a layer's rows) are freed before return, and one that does not fit in the free
 * device memory is refused with VMR_EINVAL. */
enum { VMR_EDGE_REPORTED = 1, VMR_EDGE_INFERRED = 2 };
int vmr_edge_table_size(vmr_handle h, int method, double threshold, int select, int layer, uint64_t* n);
int vmr_edge_table(vmr_handle h, int method, double threshold, int select, int layer, uint64_t n,
                   int32_t* sl, int32_t* si, int32_t* sj,
                   uint8_t* y, double* prob, double* mean,
                   uint32_t* n_rep, uint64_t* total, uint32_t* n_mask, uint32_t* ego, uint32_t* alter,
                   uint8_t* y_T, uint32_t* n_rep_T, uint64_t* total_T, int out_on_device);

/* The posterior scored against a ground-truth network, where rho lives -- the `f1_score` / `GridSearchCV` scoring of the
 * reference's synthetic experiments (notebooks/python/experiments/unreliable_reporters.py:189-200, 358-361), the F1 of its
 * known-answer tests (test/test_model.py:117-334) and `utils.get_optimal_threshold` -- instead of one dense read-out per
 * threshold (L N^2 bytes each) plus, for an AUC or a calibration curve, the 8 L N^2 K bytes of rho.
 * y_true: uint8 [L,N,N] in natural order, a device pointer when y_true_on_device != 0; every output is a host array and may be
 * NULL (not all of them).  Reads the CURRENT rho (after vmr_restore: the snapshot's).  Per tie t = (l,i,j), over all ordered
 * pairs of a layer, the diagonal included unless skip_diagonal != 0:
 *   b     y_true > 0
 *   s     the score: VMR_SCORE_RHO1 rho[t][1], what vmr_readout(VMR_READ_THRESHOLD) compares; VMR_SCORE_PROB sum_{k>=1} rho_k
 *         added in ascending k, `prob` of vmr_edge_table (K = 2: the same double)
 *   a     the first maximum of rho[t][.], the byte of vmr_readout(VMR_READ_RHO_MAX)
 *   mean  sum_k k rho_k, every product and sum rounded on its own: `mean` of vmr_edge_table
 * hist  [L][n_thr + 1][2]: hist[l][c][b] = #{ties with c = #{tau : thresholds[tau] <= s}}; thresholds finite and non-decreasing
 *       (duplicates allowed), n_thr in [0, VMR_SCORE_MAX_THR].  tp(tau) = sum_{c > tau} hist[l][c][1], fp(tau) likewise with
 *       [0]: the suffix sums are the caller's.  With VMR_SCORE_RHO1, tp(tau) + fp(tau) is the number of ones
 *       vmr_readout(h, VMR_READ_THRESHOLD, thresholds[tau], ..) writes.  Without hist the thresholds are not read.
 * conf  [L][VMR_SCORE_NCONF]: #{a > 0 and b}, #{a > 0 and not b}, #{a = 0 and b}, #{a = y_true}, P = #{b}
 * sums  [L][VMR_SCORE_NSUM]: sum s, sum_{b} s, sum (s - [b])^2 (the Brier numerator), sum (mean - y_true)^2 (the experiment's MSE
 *       numerator); doubles summed by a fixed two-stage tree whose grid depends on N only, no floating-point atomics
 * auc_pairs [L][2]: (U2, Q), U2 = 2 #{(p,n) : s_p > s_n} + #{(p,n) : s_p = s_n} over ties p with b and n without, Q = #{not b};
 * auc [L] = U2 / (2 P Q), NaN when P = 0 or Q = 0 (vmr_report_auc's rule).  Exact 64-bit integer counts; the positives' scores
 * are sorted (8 B per positive, twice, plus the sort's scratch) and every negative tie searches them; nothing of this runs
 * when auc and auc_pairs are both NULL.
 * Any K, both data formats, every mask layout, handles of vmr_create_coo.  All results are bit-identical from run to run.
 * VMR_EINVAL with a message, before any launch: NULL y_true, every output NULL, score not 0 / 1, n_thr out of range, hist with
 * n_thr > 0 and thresholds NULL, a non-finite or decreasing threshold, a temporary that does not fit in the free device
 * memory (L N^2 bytes for a host y_true; 8 (n_thr + 1) 2 L bytes; 32 B per workgroup); for the AUC, once P is counted,
 * P >= 2^31 or 2 P Q >= 2^63.  VMR_ESTATE before vmr_set_state.  VMR_ENAN if any s is NaN (the outputs are then unspecified).
 * Synchronises; temporaries are freed on every exit path. */
enum { VMR_SCORE_RHO1 = 0, VMR_SCORE_PROB = 1 };
#define VMR_SCORE_NCONF 5
#define VMR_SCORE_NSUM 4
#define VMR_SCORE_MAX_THR 4096
int vmr_score_truth(vmr_handle h, const uint8_t* y_true, int y_true_on_device, int score, int skip_diagonal,
                    int n_thr, const double* thresholds,
                    uint64_t* hist,       /* [L][n_thr + 1][2] or NULL */
                    uint64_t* conf,       /* [L][VMR_SCORE_NCONF] or NULL */
                    double*   sums,       /* [L][VMR_SCORE_NSUM] or NULL */
                    double*   auc,        /* [L] or NULL */
                    uint64_t* auc_pairs   /* [L][2] or NULL */);

/* The reporter table: each reporter's reports against the posterior, computed where rho lives -- the per-reporter counterpart of
 * vmr_edge_table and vmr_ppc_observed(by_reporter), without the 8 L N^2 K bytes of rho crossing PCIe and without writing the
 * support (vmr_mean_poisson: |S| elements of 24 B).  From the CURRENT rho (after vmr_restore: the snapshot's), the handle's own X
 * and R, and the g_theta, g_lambda, g_nu of vmr_get_geometric.  With S_m = {(i,j) : R[l,i,j,m] != 0} (without R every (i,j), the
 * diagonal included: vmr_mean_poisson's support), x = X[l,i,j,m], y the byte vmr_readout(h, method, threshold, ..) writes for the
 * tie (method VMR_READ_RHO_MAX or VMR_READ_THRESHOLD; VMR_READ_RHO_MEAN: VMR_EINVAL), prob = sum_{k>=1} rho_k (k ascending, `prob`
 * of vmr_edge_table) and mp the value vmr_mean_poisson defines for (l,i,j,m):
 * counts [L'][M][VMR_RT_NCOUNT], exact integer sums:
 *   0 n_scope     #S_m                                 1 n_rep   #{S_m : x > 0}             2 total  sum_{S_m} x
 *   3 n_inferred  #{S_m : y > 0}                       4 hits    #{S_m : x > 0 and y > 0}
 *   5 mutual      #{(i,j) in S_m, i != j : x_ijm > 0, (j,i) in S_m, x_jim > 0}   (ordered; statistic 3 of vmr_ppc_observed, per reporter)
 *   6 n_out       #{(i,j) not in S_m : x > 0}          (reports the mask discards; 0 without R)
 * sums [L'][M][VMR_RT_NSUM]:
 *   0 exp_ties    sum_{S_m} prob                       1 exp_hits  sum_{S_m, x > 0} prob     2 exp_total  sum_{S_m} mp
 * L' = L for layer < 0, else 1 (that layer's rows at index 0).  Host arrays; either may be NULL, not both.
 * Cost: one pass over rho plus the reports (and the mask entries of partial rows) -- a tie whose mask row is all ones is added
 * once, not once per reporter -- so O(ties + reports), not O(|S|).
 * Determinism: every accumulator is a 64-bit integer; the sums are accumulated in FIXED POINT (no floating-point atomics, no
 * order-dependent sum), so all outputs are bit-identical from run to run.  With b = ceil(log2 N^2), e_l the exponent with
 * max G_lambda < 2^e_l (frexp; over the layers asked for) and e_x the exponent with sum X < 2^e_x (vmr_data_stats' sum_x + 1, frexp):
 *   exp_ties, exp_hits   every prob (<= 1) is rounded to a multiple of q = 2^-(61 - b)
 *   exp_total            = g_theta[l,m] Q + g_nu U:  Q = sum_{S_m} sum_k rho_k g_lambda_k, terms (<= max G_lambda) rounded to
 *                        2^-(61 - b - e_l);  U = sum_{S_m} (sum_k rho_k) X[l,j,i,m], terms rounded to 2^-(61 - e_x); per term
 *                        q = g_theta[l,m] 2^-(61 - b - e_l) + g_nu 2^-(61 - e_x)   (mp <= g_theta max G_lambda + g_nu max X)
 * A sum of n terms is therefore within n q / 2 of the exact sum of its terms (n <= n_scope).  A row of rho that sums to more than
 * 2 does not fit this fixed point: VMR_EINVAL.
 * Any K, both data formats, every mask layout, handles of vmr_create_coo, mutuality on or off; fewer than 2^31 ties per layer.
 * VMR_EINVAL with a message, before any launch: counts and sums both NULL, a bad method, layer >= L, a temporary that does not fit
 * in the free device memory (88 B per reporter and layer; report-list handles: the tie-major index of vmr_mean_poisson and the
 * tie -> position table).  NULL handle: VMR_EINVAL.  VMR_ESTATE before vmr_set_state.  VMR_ENAN if a sum is NaN.  Synchronises;
 * temporaries are freed on every exit path. */
#define VMR_RT_NCOUNT 7
#define VMR_RT_NSUM 3
int vmr_reporter_table(vmr_handle h, int method, double threshold, int layer,
                       uint64_t* counts /* [L'][M][VMR_RT_NCOUNT] */, double* sums /* [L'][M][VMR_RT_NSUM] */);

/* The log predictive density of HELD-OUT reports under the fitted posterior, scored where rho lives -- what k-fold
 * cross-validation needs to compare K, mutuality or priors on data without a ground truth (ELBOs of different K are not
 * comparable).  It stands beside the data term of `__ELBO` (model.py:948-1019), which is the same Poisson likelihood in
 * expectation over the entries INSIDE the mask, and `_calculate_mean_poisson` (model.py:1220-1293), whose value `mean` is.  An
 * entry (l,i,j,m) with R = 0 is outside the model: its count is discarded and it adds nothing to the rates (vmr_reporter_table
 * counts such reports as n_out); this function evaluates the likelihood at such entries, which no other entry point does.
 * The list: n entries el, ei, ej, em (int32 subscripts), ex the held-out counts (>= 0), ext the mirrored counts X[l,j,i,m] to
 * condition on (>= 0; NULL: all 0); device pointers when in_on_device != 0.  It must be non-decreasing in el; entries need not be
 * sorted otherwise and may repeat.  A list sorted by (l,i,j,m) reads each rho row from neighbouring lanes and is the fast case.
 * theta host [L][M], lambda host [L][K] and eta are the caller's (as vmr_ppc_replicates takes its tables): the function is a
 * pure function of (rho, the list, theta, lambda, eta, the handle's mask).  The handle's X is never read and no tie-major index
 * is built; report-list handles take the tie -> position table of vmr_mean_poisson (4 B per tie of a layer).
 * Per entry e, with rho the CURRENT row of tie (l,i,j) (after vmr_restore: the snapshot's) and x = ex[e]:
 *   mu_k    = theta[l][m] lambda[l][k] + eta ext[e]
 *   mean[e] = sum_k rho_k mu_k, k ascending, every product and every sum rounded on its own (`mean` of vmr_edge_table's convention)
 *   logp[e] = log sum_k rho_k Poisson(x; mu_k), as a log-sum-exp over the categories with rho_k > 0 of
 *             b_k = x log(mu_k) - mu_k + log(rho_k), lgamma(x + 1) subtracted once.  mu_k = 0 and x = 0 contributes log(rho_k);
 *             mu_k = 0 and x > 0 contributes nothing; if no category contributes, logp[e] = -inf.
 * logp, mean: [n] or NULL, device pointers when out_on_device != 0.  Per layer, over the layer's entries:
 *   sums   host [L][VMR_HO_NSUM] or NULL:    0 sum logp over the entries with finite logp    1 sum (x - mean)^2    2 sum x    3 sum mean
 *   counts host [L][VMR_HO_NCOUNT] or NULL:  0 entries    1 entries with x > 0    2 entries with logp = -inf (left out of sums[l][0])
 *          3 entries whose (l,i,j,m) lies INSIDE the handle's own mask: in-sample entries, not an error (a cross-validation
 *            driver asserts 0)
 * K <= 8: one lane per entry (K = 2: the row in one 16-byte load); larger K, up to 256: a group of 16 lanes per entry, which folds
 * the running maximum and the scaled sum by shuffles in a fixed order.  All sums are doubles reduced by a fixed two-stage tree
 * (a workgroup per 1024 consecutive entries of a layer's segment, then one workgroup per layer) whose shape depends on the
 * segment length alone: no floating-point atomics, no tickets, bit-identical from run to run.
 * VMR_EINVAL with a message, before any launch: NULL handle (no message), a NULL subscript or count array, all four outputs NULL,
 * n = 0 or n >= 2^31, NULL theta or lambda, a negative or non-finite theta, lambda or eta, a temporary that does not fit in the free
 * device memory (host lists: 24 n B; host logp / mean: 8 n B each; 64 B per 1024 entries).  VMR_ESTATE before vmr_set_state.
 * VMR_EINVAL from the kernels: a subscript out of range, a negative ex or ext, a decreasing el -- the entry sets a flag, reads
 * nothing and adds nothing; the outputs are then unspecified.  VMR_ENAN, after the kernel: a logp or a mean is NaN.
 * Any K, both data formats, every mask layout, handles of vmr_create_coo; fewer than 2^31 ties per layer.  Synchronises;
 * temporaries are freed on every exit path. */
#define VMR_HO_NSUM 4
#define VMR_HO_NCOUNT 4
int vmr_heldout_loglik(vmr_handle h, uint64_t n,
                       const int32_t* el, const int32_t* ei, const int32_t* ej, const int32_t* em,
                       const int32_t* ex,   /* the held-out counts, >= 0 */
                       const int32_t* ext,  /* the mirrored counts X[l,j,i,m] to condition on, or NULL = 0 */
                       int in_on_device,
                       const double* theta /* host [L][M] */, const double* lambda /* host [L][K] */, double eta,
                       double* logp /* [n] or NULL */, double* mean /* [n] or NULL */, int out_on_device,
                       double* sums   /* host [L][VMR_HO_NSUM] or NULL */,
                       uint64_t* counts /* host [L][VMR_HO_NCOUNT] or NULL */);

/* Every report of the support scored under the posterior, where rho lives: which individual reports, and which omissions, does
 * the fitted model disbelieve -- the per-report counterpart of vmr_reporter_table, and the exact in-sample log predictive density
 * beside the held-out one of vmr_heldout_loglik.  The in-sample support cannot be handed to vmr_heldout_loglik as a list (24 B
 * per element; L N^2 M elements without a mask); this walks it, keeps integer histograms and a few sums, and writes out only the
 * rows worth reading.
 * The support S = {(l,i,j,m) : R != 0}; without R every (i,j,m), the diagonal included: vmr_mean_poisson's support, walked in its
 * lexicographic (l,i,j,m) order.  For an element e of S, from the handle's own data and the CURRENT rho (after vmr_restore: the
 * snapshot's):  x = X[l,i,j,m];  xt = X[l,j,i,m] with mutuality, else 0;  theta host [L][M], lambda host [L][K] and eta are the
 * caller's tables, as vmr_heldout_loglik takes them;  mean[e] and logp[e] are what vmr_heldout_loglik defines for the entry
 * (l,i,j,m) with ex = x and ext = xt -- the same device functions, term for term, with the same -inf and NaN rules, so the same
 * bits.  The score is s = -logp (+inf where logp = -inf).  An element is a REPORT when x > 0, an OMISSION when x = 0; it is FLAGGED
 * iff its class is in `select` (VMR_RS_REPORTS | VMR_RS_OMISSIONS: 1, 2 or 3) and s >= threshold (finite, or +inf: only the
 * elements with logp = -inf).
 * Outputs, host arrays unless noted, any of them NULL (not all); L' = L for layer < 0, else 1:
 *   hist   [L'][n_edges + 1][2]: over ALL of S whatever `select` is, hist[l][c][b] = #{e : c = #{tau : edges[tau] <= s}}, b = 0
 *          for reports, 1 for omissions; edges finite and non-decreasing, n_edges in [0, VMR_RS_MAX_EDGES] (vmr_score_truth's
 *          convention; s = +inf lands in the last bin).  Without hist the edges are not read.
 *   sums   [L'][VMR_RS_NSUM]:   0 sum logp over the elements with finite logp (the in-sample log predictive density)
 *          1 sum (x - mean)^2    2 sum x    3 sum mean          (the columns of VMR_HO_NSUM)
 *   counts [L'][VMR_RS_NCOUNT]: 0 elements    1 reports    2 elements with logp = -inf    3 flagged elements
 *   by_reporter [L'][M][2]: the flagged elements of reporter m, by class
 *   the table: one row per flagged element in lexicographic (l,i,j,m) order -- sl, si, sj, sm, x, xt (int32), logp, mean; n is the
 *          capacity: below the row count VMR_EINVAL before anything is written; n = 0 and every row pointer NULL: no table pass;
 *          device pointers when out_on_device != 0.
 * vmr_report_scores_size gives the row count, the sum over the layers of counts[.][3], for the same arguments.
 * A count pass walks the support (a group of lanes per tie, the tie's support reporters in ascending m): the likelihood at every
 * element, the integer bins in LDS first (reporters up to 2048, the histogram where it fits beside them, global integer atomics
 * beyond), a tie's flagged count; an exclusive 64-bit sum of those gives a tie's first row, and a fill pass -- only when rows are
 * asked for, only over ties that hold one -- writes a flagged element at its tie's offset plus its rank among the group's lanes.
 * The sums are doubles: a workgroup owns a fixed contiguous range of ties, a lane adds its elements in walk order, the waves fold
 * by shuffles, the workgroup in LDS, and a last kernel adds the workgroups' partials in index order.  No floating-point atomics,
 * no tickets, a tree that depends on N and M alone: every output is bit-identical from run to run.
 * Any K up to 256, both data formats, every mask layout, handles of vmr_create_coo, counts up to 2^31 - 1; fewer than 2^31 ties per
 * layer.  Layers are processed one at a time; report-list handles take the tie-major index of vmr_mean_poisson and the tie ->
 * position table per layer.
 * VMR_EINVAL with a message, before any launch: NULL handle (no message), NULL theta or lambda, a negative or non-finite theta,
 * lambda or eta, select outside 1..3, a NaN or -inf threshold, layer >= L, every output NULL, n_edges out of range, hist with
 * n_edges > 0 and edges NULL, a non-finite or decreasing edge, a temporary that does not fit in the free device memory (8 B per
 * tie of a layer, and of every layer asked for when rows are; 64 B per workgroup; the bins; host rows: 40 B per row of a layer).
 * VMR_ESTATE before vmr_set_state.  VMR_ENAN, after the count pass: a logp or a mean is NaN (no row is then written).
 * Synchronises; temporaries are freed on every exit path. */
enum { VMR_RS_REPORTS = 1, VMR_RS_OMISSIONS = 2 };
#define VMR_RS_NSUM 4
#define VMR_RS_NCOUNT 4
#define VMR_RS_MAX_EDGES 4096
int vmr_report_scores_size(vmr_handle h, int layer, const double* theta, const double* lambda, double eta,
                           int select, double threshold, uint64_t* n);
int vmr_report_scores(vmr_handle h, int layer, const double* theta /* host [L][M] */, const double* lambda /* host [L][K] */, double eta,
                      int select, double threshold,
                      int n_edges, const double* edges,
                      uint64_t* hist        /* [L'][n_edges + 1][2] or NULL */,
                      double*   sums        /* [L'][VMR_RS_NSUM] or NULL */,
                      uint64_t* counts      /* [L'][VMR_RS_NCOUNT] or NULL */,
                      uint64_t* by_reporter /* [L'][M][2] or NULL */,
                      uint64_t n, int32_t* sl, int32_t* si, int32_t* sj, int32_t* sm,
                      int32_t* x, int32_t* xt, double* logp, double* mean, int out_on_device);

/* Reporter influence: whose word does an inferred tie rest on?  For every element (l,i,j,m) of the support, the row of rho the
 * tie would hold had reporter m said nothing about it -- the leave-one-reporter-out posterior, computed where rho lives.
 * vmr_reporter_table says whether a reporter agrees with the posterior and vmr_report_scores which reports the posterior
 * disbelieves; this says which reports DECIDE it.  The CAVI update of a tie's row is additive over the reporters of its mask
 * (`_update_rho`, model.py:763-818):  log rho_k = logpr_k + sum_m c_mk + const,  so dividing reporter m's factor exp(c_mk) out
 * of the row and normalising again gives exactly the row the update would have produced with R[l,i,j,m] = 0 -- closed form, no
 * refit.  The parameters are held fixed and ONE factor leaves ONE tie: the numbers are an exact refit of that row only when rho
 * is the update's fixed point for the tables given.
 * The caller's tables, host arrays as vmr_report_scores takes theta and lambda: e_theta [L][M] = E[theta] (shape / rate),
 * elog_theta [L][M] = E[log theta] (psi(shape) - log(rate)), e_lambda [L][K], elog_lambda [L][K] likewise, and g_nu =
 * exp(E[log nu]) (ignored, 0, on a handle without mutuality).  The entry forms g_theta = exp(elog_theta), g_lambda =
 * exp(elog_lambda) on the host.
 * The support S is vmr_mean_poisson's, walked in its lexicographic (l,i,j,m) order.  Per element, from the handle's own data and
 * the CURRENT rho (after vmr_restore: the snapshot's): x = X[l,i,j,m]; xt = X[l,j,i,m] with mutuality, else 0; rho the tie's row.
 * Every product, quotient and sum below is rounded on its own (no fused multiply-add), in the order written:
 *   z1_k  = g_theta[l][m] g_lambda[l][k];   den_k = z1_k + (g_nu xt), a zero den_k replaced by 1;   w1_k = z1_k / den_k
 *   c_k   = (elog_theta[l][m] + elog_lambda[l][k]) (x w1_k) - e_theta[l][m] e_lambda[l][k]      reporter m's factor, d_k = -c_k
 *   over the categories with rho_k > 0 only (the others keep q_k = 0):  mx = max d_k;  u_k = rho_k exp(d_k - mx);
 *   S = sum u_k, k ascending;  q_k = u_k / S.      A row of all zeros (one the engine keeps) gives q = 0.
 *   prob     = sum_{k>=1} rho_k, k ascending (`prob` of vmr_edge_table; K = 2: rho_1 bit for bit)
 *   prob_loo = sum_{k>=1} q_k, k ascending;     tv = (sum_k |q_k - rho_k|) / 2, k ascending: the total variation between the rows
 *   y  the byte vmr_readout(h, method, threshold, ..) writes for the tie, y' the same rule applied to q: VMR_READ_RHO_MAX the
 *      first maximum, VMR_READ_THRESHOLD q_1 >= threshold (VMR_READ_RHO_MEAN: VMR_EINVAL)
 *   LOST: y > 0 and y' = 0 (the inferred tie rests on this report);  GAINED: y = 0 and y' > 0 (this report alone holds it down).
 * An element is FLAGGED iff it is lost and select & VMR_INF_LOST, or gained and select & VMR_INF_GAINED, or tv >= min_tv
 * (select in 0..3; min_tv in [0, +inf], +inf: flips only).
 * Outputs, host arrays unless noted, any of them NULL (not all); L' = L for layer < 0, else 1:
 *   counts [L'][M][VMR_INF_NCOUNT], exact:  0 n_scope = #S_m (column 0 of vmr_reporter_table)   1 lost   2 gained   3 flagged
 *   sums   [L'][M][VMR_INF_NSUM]:  0 sum_{S_m} tv    1 sum_{S_m} (prob_loo - prob)
 *          accumulated in FIXED POINT, as vmr_reporter_table's exp_ties: with b = ceil(log2 N^2) every term is rounded to a
 *          multiple of q = 2^-(61 - b) and added by signed 64-bit integer atomics, so a reporter's sum is within n_scope q / 2 of
 *          the exact sum of its terms.  A term beyond 2 in size (a row of rho that sums to more than 2) does not fit: VMR_EINVAL.
 *   hist   [L'][n_edges + 1][2]: over ALL of S, hist[l][c][b] = #{e : c = #{tau : edges[tau] <= tv}}, b = 0 for x > 0, 1 for
 *          x = 0; edges finite and non-decreasing, n_edges in [0, VMR_INF_MAX_EDGES].  Without hist the edges are not read.
 *   the table: one row per flagged element in lexicographic (l,i,j,m) order -- sl, si, sj, sm, x, xt (int32), prob, prob_loo, tv
 *          (double), each column optional; n is the capacity: below the row count VMR_EINVAL before anything is written; n = 0 and
 *          every row pointer NULL: no table pass; device pointers when out_on_device != 0.
 * vmr_reporter_influence_size gives the row count, the sum of counts[.][.][3], for the same arguments.
 * The passes are vmr_report_scores': a count pass (a group of lanes per tie, the tie's support reporters in ascending m; the
 * integer bins in LDS first -- reporters up to 2048, the histogram where it fits beside them in 128 KB, global integer atomics
 * beyond), an exclusive 64-bit sum of the ties' flagged counts, and a fill pass that places a row by its ballot rank.  K = 2 and
 * K <= 8 keep the row in registers, larger K streams it; the variants perform the same operations.  Every accumulator is an
 * integer: no floating-point atomics, every output bit-identical from run to run.
 * Any K up to 256, both data formats, every mask layout, handles of vmr_create_coo, mutuality on or off; fewer than 2^31 ties
 * per layer.  VMR_EINVAL with a message, before any launch: NULL handle (no message), a NULL table, e_theta or e_lambda negative
 * or not finite, elog_theta or elog_lambda not finite (or with an exp that overflows), g_nu negative or not finite, a bad method,
 * select outside 0..3, min_tv NaN or negative, layer >= L, every output NULL, n_edges out of range, hist with n_edges > 0 and
 * edges NULL, a non-finite or decreasing edge, a temporary that does not fit in the free device memory (8 B per tie of a layer,
 * and of every layer asked for when rows are; 48 B per reporter and layer; host rows: 48 B per row of a layer).  VMR_ESTATE before
 * vmr_set_state.  VMR_ENAN, after the count pass: a prob, prob_loo or tv is NaN (no row is then written).  Synchronises;
 * temporaries are freed on every exit path. */
enum { VMR_INF_LOST = 1, VMR_INF_GAINED = 2 };
#define VMR_INF_NCOUNT 4
#define VMR_INF_NSUM 2
#define VMR_INF_MAX_EDGES 4096
int vmr_reporter_influence_size(vmr_handle h, int layer, const double* e_theta, const double* elog_theta, const double* e_lambda,
                                const double* elog_lambda, double g_nu, int method, double threshold, int select, double min_tv,
                                uint64_t* n);
int vmr_reporter_influence(vmr_handle h, int layer,
                           const double* e_theta /* host [L][M] */, const double* elog_theta /* host [L][M] */,
                           const double* e_lambda /* host [L][K] */, const double* elog_lambda /* host [L][K] */, double g_nu,
                           int method, double threshold, int select, double min_tv,
                           int n_edges, const double* edges,
                           uint64_t* hist   /* [L'][n_edges + 1][2] or NULL */,
                           uint64_t* counts /* [L'][M][VMR_INF_NCOUNT] or NULL */,
                           double*   sums   /* [L'][M][VMR_INF_NSUM] or NULL */,
                           uint64_t n, int32_t* sl, int32_t* si, int32_t* sj, int32_t* sm,
                           int32_t* x, int32_t* xt, double* prob, double* prob_loo, double* tv, int out_on_device);

/* exp(E[log .]) of theta [L,M], lambda [L,K], nu from the current shape/rate parameters
 * (model.py:676-684), plus g_nu_cache = the G_exp_nu the last cache refresh held, i.e. the
 * value computed BEFORE the last nu update -- what `model.G_exp_nu` reads after `fit` and what
 * the ELBO uses (model.py:684 vs :822, :970).  Any pointer may be NULL. */
int vmr_get_geometric(vmr_handle h, double* g_theta, double* g_lambda, double* g_nu, double* g_nu_cache);

/* Wait for all work queued on the handle's stream. */
int vmr_sync(vmr_handle h);

/* Per-kernel-class timing with HIP events on the handle's stream (for bench.py's roofline
 * line).  enable=1 starts recording and clears totals; enable=2 records only the passes over the data (classes
 * GAMMA_COUNTS, RHO, ELBO, RHO_ELBO), not the small finalize kernels.  vmr_profile_read synchronises. */
int vmr_profile(vmr_handle h, int enable);
int vmr_profile_read(vmr_handle h, int kernel_class, double* total_ms, int64_t* launches);

/* Algorithmic bytes one launch of a kernel class moves under the handle's data format, see DESIGN.md:
 * report lists (4 B per non-zero count, 4 B per tie, mask words of partial rows, rho/logpr_rho 8 B) or the
 * dense encoding (X 1 B/elt, R 1 bit/elt, rho/logpr_rho 8 B). */
int vmr_kernel_bytes(vmr_handle h, int kernel_class, double* bytes);

/* Data format chosen by vmr_create: *sparse = 1 for report lists (default whenever they are at most half the
 * dense bytes; env VMR_FORMAT=dense|sparse overrides), 0 for the dense tiles.  *nnz = non-zero counts in X
 * (0 when the dense format was forced before counting).  Either pointer may be NULL. */
int vmr_data_format(vmr_handle h, int* sparse, uint64_t* nnz);

/* Mask layout: *lists = 1 when the partial rows of R are also held as short reporter lists (rows with few
 * reporters, e.g. the self-reporter mask of _io.py:230-242; env VMR_NO_RLISTS=1 disables), *listed = reporters in
 * those lists.  The bit-packed mask is kept either way.  Either pointer may be NULL. */
int vmr_mask_format(vmr_handle h, int* lists, uint64_t* listed);

/* Shape of a sweep over the report lists (no reference equivalent; what `_update_CAVI`, model.py:623-660, costs here):
 * *passes = passes over the entries per sweep (1, or 2 where the tables of a wide reporter dimension do not fit in LDS side
 * by side), *lds_levels = mirror-count levels of the statistics H the pass keeps in LDS, *far_reports = reports of the
 * levels beyond that a one-pass handle built with env VMR_FARL=1 also keeps as a compact list (k_far_hist adds their
 * statistics after the pass; default: two passes instead).  Dense tiles: 1 (2), the LDS levels, 0.  Any pointer may be NULL. */
int vmr_sweep_shape(vmr_handle h, int* passes, int* lds_levels, uint64_t* far_reports);

/* Synthetic generators on the device (no handle: they produce the inputs of vmr_create).
 * vmr_generate_y replaces the ground-truth draw of the reference's StandardSBM (synthetic.py:548-571, 639-667):
 * Y[l,i,j] ~ Poisson(w[grp[i]][grp[j]]) clipped to K - 1, zero diagonal.  w [C][C] and grp [N] are host arrays, Y_dev a
 * uint8 [L][N][N] array in device memory.
 * vmr_generate_x replaces `_build_X` (synthetic.py:63-352; the pair-wise draw :159-231): for every unordered pair a fair coin
 * picks the direction drawn first, first ~ Poisson((own + eta * mirror) / (1 - eta^2)), second ~ Poisson(own + eta * first), with
 * own = lambda * theta[l,m] in float64; lambda from Y_dev (0.01 where Y = 0, else Y, or 0.01 + lambda_diff when lambda_diff > 0;
 * synthetic.py:140-157) or given as lam_dev (double [L][N][N], device; Y_dev may then be NULL).  theta [L][M] is a host array.
 * self_reporter != 0: only a tie's own two nodes report (`_io.py:230-242`; M == N) and X_dev must come zeroed.
 * X_dev: uint8 [L][N][N][M] in device memory, counts clamped to 255 -- what vmr_create(data_on_device = 1) takes.
 * Counter-based stream (Philox4x32-10 keyed by seed; counter = layer, pair, reporter): a draw depends on (seed, l, i, j, m) only.
 * NOT the reference's RandomState stream: the host classes keep that exact mode (vimure_amd/synthetic.py).  Both synchronise. */
int vmr_generate_y(int device, int L, int N, int K, int C, const double* w, const int32_t* grp, uint64_t seed, uint8_t* Y_dev);
int vmr_generate_x(int device, int L, int N, int M, const uint8_t* Y_dev, const double* lam_dev, const double* theta, double eta,
                   double lambda_diff, uint64_t seed, int self_reporter, uint8_t* X_dev);

/* Library/version string. */
const char* vmr_version(void);

#ifdef __cplusplus
}
#endif
#endif /* VIMURE_HIP_H */
