// create.h -- what the two ways to a handle share.  vmr_create (create.hip: a dense uint8 tensor, turned into report lists when it
// is sparse) and vmr_create_coo (create_coo.hip: coordinate lists straight to report lists) both run create_ctx, their own
// ingestion, create_state, and the shared tail that settles the LDS shapes and allocates the statistics and the scratch.
#ifndef VMR_CREATE_H
#define VMR_CREATE_H

#include "sweep_sl.h"

// context, geometry, streams and the small per-dataset arrays; reads the environment switches (read_opts), once per handle
int create_ctx(vmr_ctx** out, hipDeviceProp_t* prop, int device, int L, int N, int M, int K, int mutuality, double eps, bool lists_only = false);
// variational state and accumulation slots; reads back the data statistics (largest count, mask row classes)
int create_state(vmr_ctx* h, unsigned* xm_out);
// sorted lists: the per-tie arrays the sweeps read, by position (the tie-order originals stay for the mask kernels)
int sl_finish(vmr_ctx* h);
// LDS shapes, the statistics / factor tables, scratch; for report lists the count-mode launch (constants C[l][y][m])
int create_tail(vmr_ctx* h, const hipDeviceProp_t& prop);

// vimure_hip.hip: the sweep-time launches create_tail queues for the constants of a report-list handle
// the statistics of the far reports (k_far_hist) after a statistics pass; count: the count-mode pass of create_tail;
// nu: -1 = no nu sum in this sweep; 0 = the raw sum to elbo_dev[1]; 1 = nu committed too (as launch_hist's)
int launch_far(vmr_ctx* h, int count, int nu);
// the count-mode result in H becomes the constants C[l][y][m] (k_take_counts, H left zeroed)
int take_counts(vmr_ctx* h);

#endif
