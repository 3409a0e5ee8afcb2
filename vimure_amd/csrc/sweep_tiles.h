// sweep_tiles.h -- the dense tile path (sweep_tiles.hip): the sweeps of a handle that keeps the uint8 tensor X[L,N,N,Mp] because
// it is dense enough that 1 byte per (tie, reporter) is less to read than the report lists.  k_hist and k_rho stage the (I,J)
// tile of ties and its mirror (J,I) in LDS; the launch logic of vimure_hip.hip calls them through the two entries below and
// vmr_create (create.hip) sizes a handle with the geometry and the LDS sizes.
#ifndef VMR_SWEEP_TILES_H
#define VMR_SWEEP_TILES_H

#include "vmr_internal.h"

// tile edge, lanes per tie, prefetch depth and the mask kernel's grid from (L, N, M, K, mut)
// lists_only: a vmr_create_coo handle, which never launches the dense tiles (their LDS bound does not limit M there)
int choose_geo(Geo& g, int ncu, std::string& err, bool lists_only);

// LDS bytes of one workgroup of k_hist and of k_rho<., ., update, elbo, .>
size_t shmem_hist(const Geo& g);
size_t shmem_rho(const Geo& g, bool update, bool elbo);

// k_hist: H of the current rho.  The caller (launch_hist) has zeroed H, holds the profile scope and sets the validity flags.
int tiles_hist(vmr_ctx* h);
// k_rho; mode: 0 = rho update (+ H unless two_pass), 1 = rho update + fused ELBO, 2 = ELBO only; smem = shmem_rho of that mode.
// The caller (launch_rho) has zeroed H / slotF, holds the profile scope, sets the validity flags and launches k_fin_rho.
int tiles_rho(vmr_ctx* h, int mode, size_t smem);

#endif
