"""ctypes binding of libvimure_hip.so (C-ABI declared in include/vimure_hip.h).

There is no CPU fallback: if the shared library is missing this module raises.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VMR_LIB", os.path.join(HERE, "libvimure_hip.so"))  # VMR_LIB: A/B builds of the engine

VMR_OK, VMR_EINVAL, VMR_EHIP, VMR_ENAN, VMR_ESTATE = 0, -1, -2, -3, -4
STEP_GAMMA, STEP_PHI, STEP_RHO, STEP_NU = 0, 1, 2, 3
KERNEL_GAMMA_MASK, KERNEL_GAMMA_COUNTS, KERNEL_PHI, KERNEL_RHO, KERNEL_ELBO, KERNEL_FINALIZE, KERNEL_RHO_ELBO, KERNEL_RHO_NOSTORE = range(8)
READ_RHO_MAX, READ_RHO_MEAN, READ_THRESHOLD = 0, 1, 2
PPC_NSTAT = 6
TRIAD_NSTAT = 6
TRIAD_NAMES = ["transitive", "cyclic", "two_paths", "triangles_u", "wedges_u", "edges_u"]
MIX_CMAX, MIX_LMAX = 64, 32
CONN_NSTAT, CONN_NDIST, CONN_NMAX = 10, 64, 2048
CONN_NAMES = ["components_w", "giant_w", "pairs_w", "isolates", "components_s", "giant_s", "pairs_s", "reach_pairs", "dist_sum",
              "diameter"]
CONN_NODE_NAMES = ["node_comp_w", "node_comp_s", "node_reach_out", "node_reach_in", "node_dist_out", "node_dist_in"]
CENT_NMAX, CENT_TMAX = 2048, 64
CENT_DIRECTIONS = ("out", "in", "union")   # VMR_CENT_OUT, VMR_CENT_IN, VMR_CENT_UNION
BTW_NMAX = 2048
BTW_DIRECTIONS = ("directed", "union")     # VMR_BTW_DIRECTED, VMR_BTW_UNION
CORE_NMAX = 2048
CORE_MODES = ("union", "total", "in", "out")   # VMR_CORE_UNION, VMR_CORE_TOTAL, VMR_CORE_IN, VMR_CORE_OUT
CASC_NMAX, CASC_TMAX, CASC_KMAX, CASC_SETS, CASC_NPER = 2048, 65535, 65536, 64, 64
CASC_DIRECTIONS = ("out", "in", "union")   # VMR_CASC_OUT, VMR_CASC_IN, VMR_CASC_UNION
CENSUS_NCLASS = 16
CENSUS_NAMES = ("003", "012", "102", "021D", "021U", "021C", "111D", "111U", "030T", "030C", "201", "120D", "120U", "120C", "210", "300")
SP_MODES = ("union", "mutual", "path")     # VMR_SP_UNION, VMR_SP_MUTUAL, VMR_SP_PATH
SP_MAX_BINS, SP_NTOTAL = 1024, 4
SP_TOTALS = ("ties", "supported", "partners", "max_partners")
SH_MODES = ("union", "weighted")           # VMR_SH_UNION, VMR_SH_WEIGHTED
SH_SUMMARY = ("n_defined", "effective_size_sum", "constraint_sum")   # the columns of the structural-holes calls' summary
CUT_NMAX = 2048
CUT_UNION, CUT_MUTUAL = 0, 1
CUT_MODES = ("union", "mutual")            # VMR_CUT_UNION, VMR_CUT_MUTUAL
CUT_SUMMARY = ("n_cut", "n_bridges", "max_pairs_cut", "connected_pairs")   # the columns of the cut-point calls' summary
EDGE_REPORTED, EDGE_INFERRED = 1, 2
SCORE_RHO1, SCORE_PROB = 0, 1
SCORE_NCONF, SCORE_NSUM, SCORE_MAX_THR = 5, 4, 4096
RT_NCOUNT, RT_NSUM = 7, 3
RT_COUNT_NAMES = ["n_scope", "n_rep", "total", "n_inferred", "hits", "mutual", "n_out"]
RT_SUM_NAMES = ["exp_ties", "exp_hits", "exp_total"]
HO_NSUM, HO_NCOUNT = 4, 4
HO_SUM_NAMES = ["logp", "sq_err", "total", "exp_total"]
HO_COUNT_NAMES = ["n", "n_pos", "n_inf", "n_in_mask"]
RS_REPORTS, RS_OMISSIONS = 1, 2
RS_NSUM, RS_NCOUNT, RS_MAX_EDGES = 4, 4, 4096
RS_SUM_NAMES = ["logp", "sq_err", "total", "exp_total"]
RS_COUNT_NAMES = ["n", "n_reports", "n_inf", "n_flagged"]
INF_LOST, INF_GAINED = 1, 2
INF_NCOUNT, INF_NSUM, INF_MAX_EDGES = 4, 2, 4096
INF_COUNT_NAMES = ["n_scope", "lost", "gained", "flagged"]
INF_SUM_NAMES = ["tv", "shift"]
PPC_STAT_NAMES = ["n_pos", "total", "sumsq", "mutual", "ties_reported", "ties_agreed"]
KERNEL_NAMES = ["gamma_mask", "gamma_counts", "phi", "rho", "elbo", "finalize", "rho_elbo", "rho_nostore"]

_dp = C.POINTER(C.c_double)
_u8p = C.c_void_p  # host or device pointer

# every symbol include/vimure_hip.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "vmr_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                             _u8p, _u8p, C.c_int, C.c_double]),
    "vmr_create_coo": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double]),
    "vmr_destroy": (None, [C.c_void_p]),
    "vmr_last_error": (C.c_char_p, [C.c_void_p]),
    "vmr_data_stats": (C.c_int, [C.c_void_p, _dp, C.c_void_p]),
    "vmr_set_priors": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double]),
    "vmr_set_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double,
                                C.c_void_p, C.c_int]),
    "vmr_draw_pr_rho": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_void_p, C.c_int]),
    "vmr_step": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "vmr_elbo": (C.c_int, [C.c_void_p, _dp]),
    "vmr_fit_loop": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p, _dp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "vmr_fit_loop_batch": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vmr_sub_step": (C.c_int, [C.c_void_p, C.c_int]),
    "vmr_sweep_local": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "vmr_commit_nu": (C.c_int, [C.c_void_p, C.c_double]),
    "vmr_sweep_local_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "vmr_commit_nu_dev": (C.c_int, [C.c_void_p, C.c_void_p]),
    "vmr_stream": (C.c_void_p, [C.c_void_p]),
    "vmr_sample": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_int]),
    "vmr_sample_stats": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vmr_expected_stats": (C.c_int, [C.c_void_p, C.c_void_p]),
    "vmr_sample_triads": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vmr_expected_triads": (C.c_int, [C.c_void_p, C.c_void_p]),
    "vmr_sample_mixing": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vmr_expected_mixing": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vmr_sample_connectivity": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.c_int] + [C.c_void_p] * 8),
    "vmr_sample_centrality": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6),
    "vmr_mean_centrality": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "vmr_sample_betweenness": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6),
    "vmr_network_betweenness": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "vmr_sample_cores": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 8),
    "vmr_network_cores": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vmr_sample_outreach": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_uint64, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int] +
                            [C.c_void_p] * 6),
    "vmr_sample_seed_outreach": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_uint64, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                           C.c_int] + [C.c_void_p] * 3),
    "vmr_network_outreach": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "vmr_network_seed_outreach": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int] +
                                  [C.c_void_p] * 3),
    "vmr_sample_triad_census": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_void_p]),
    "vmr_network_triad_census": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "vmr_sample_shared_partners": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_int] +
                                   [C.c_void_p] * 3),
    "vmr_network_shared_partners": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p]),
    "vmr_sample_structural_holes": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 11),
    "vmr_network_structural_holes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 6),
    "vmr_sample_cutpoints": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 11),
    "vmr_network_cutpoints": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4),
    "vmr_ppc_replicates": (C.c_int, [C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "vmr_ppc_observed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "vmr_get_state": (C.c_int, [C.c_void_p] + [C.c_void_p] * 7),
    "vmr_get_geometric": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vmr_sync": (C.c_int, [C.c_void_p]),
    "vmr_readout": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_int]),
    "vmr_mean_poisson_size": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]),
    "vmr_mean_poisson": (C.c_int, [C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_int]),
    "vmr_report_auc": (C.c_int, [C.c_void_p, C.c_int, _dp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "vmr_edge_table_size": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_uint64)]),
    "vmr_edge_table": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int, C.c_uint64] + [C.c_void_p] * 14 + [C.c_int]),
    "vmr_score_truth": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p] + [C.c_void_p] * 5),
    "vmr_reporter_table": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p]),
    "vmr_heldout_loglik": (C.c_int, [C.c_void_p, C.c_uint64] + [C.c_void_p] * 6 + [C.c_int, C.c_void_p, C.c_void_p, C.c_double,
                                     C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "vmr_report_scores_size": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_double, C.POINTER(C.c_uint64)]),
    "vmr_report_scores": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_double, C.c_int, C.c_void_p]
                          + [C.c_void_p] * 4 + [C.c_uint64] + [C.c_void_p] * 8 + [C.c_int]),
    "vmr_reporter_influence_size": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_double, C.c_int, C.c_double, C.c_int, C.c_double,
                                              C.POINTER(C.c_uint64)]),
    "vmr_reporter_influence": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_double, C.c_int, C.c_double, C.c_int, C.c_double,
                                         C.c_int, C.c_void_p] + [C.c_void_p] * 3 + [C.c_uint64] + [C.c_void_p] * 9 + [C.c_int]),
    "vmr_snapshot": (C.c_int, [C.c_void_p]),
    "vmr_restore": (C.c_int, [C.c_void_p]),
    "vmr_profile": (C.c_int, [C.c_void_p, C.c_int]),
    "vmr_profile_read": (C.c_int, [C.c_void_p, C.c_int, _dp, C.POINTER(C.c_int64)]),
    "vmr_kernel_bytes": (C.c_int, [C.c_void_p, C.c_int, _dp]),
    "vmr_data_format": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_uint64)]),
    "vmr_mask_format": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_uint64)]),
    "vmr_sweep_shape": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint64)]),
    "vmr_generate_y": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "vmr_generate_x": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double,
                                 C.c_uint64, C.c_int, C.c_void_p]),
    "vmr_version": (C.c_char_p, []),
}

_lib = None


def load():
    """Load the engine; raises (never falls back) when the HIP library is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP engine has not been built. Run `python -m vimure_amd.build` "
            "(needs hipcc, --offload-arch=gfx950). vimure_amd has no CPU fallback.")
    # PyTorch-ROCm bundles its own libamdhip64; two HIP runtimes in one process cannot both own the
    # GPU.  Import torch first (when present) so that this library binds to the runtime torch uses.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        if os.environ.get("VMR_LIB_LAX") and not hasattr(lib, name):
            continue   # (A/B timing against an older experiment build picked with VMR_LIB: entry points it lacks stay unbound)
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
