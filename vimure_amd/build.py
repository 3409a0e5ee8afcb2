"""Compile the HIP engine for gfx950 in-tree (libvimure_hip.so next to this file).

The library is a handful of translation units (vimure_amd/csrc): objects are compiled in parallel into csrc/_obj and only
those whose source or headers changed are rebuilt; the sweep kernel is one object per number of categories K (-DVMR_K).
`VMR_DEV=1` builds K = 2 only (fast iteration on a kernel)."""
import glob
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(CSRC, "_obj")
LIB = os.environ.get("VMR_LIB_OUT", os.path.join(HERE, "libvimure_hip.so"))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HOST_SRC = os.path.join(CSRC, "host_init.c")
HOST_LIB = os.path.join(HERE, "libvimure_host.so")
HEADERS = sorted(glob.glob(os.path.join(CSRC, "*.h"))) + [os.path.join(ROOT, "include", "vimure_hip.h")]   # every object depends on every header
KS = (2, 3, 4, 5, 6, 7, 8)
FLAGS = ["-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]


def units(dev=False):
    """(object name, source, extra flags) of every translation unit."""
    extra = ["-DVMR_DEV"] if dev else []
    u = [("vimure_hip", os.path.join(CSRC, "vimure_hip.hip"), extra),   # the engine proper: finalize kernels, launch logic, fit loops, the API
         ("sweep_tiles", os.path.join(CSRC, "sweep_tiles.hip"), extra),  # the dense tile path: k_hist, k_rho, geometry and LDS sizes
         ("create", os.path.join(CSRC, "create.hip"), extra),          # vmr_create, the shared tail of both creators, vmr_destroy
         ("create_coo", os.path.join(CSRC, "create_coo.hip"), extra),  # vmr_create_coo: coordinate lists straight to report lists
         ("sorted_lists", os.path.join(CSRC, "sorted_lists.hip"), extra),
         ("sweep_gen", os.path.join(CSRC, "sweep_gen.hip"), extra),   # the general kernels: any K, wide entries
         ("generate", os.path.join(CSRC, "generate.hip"), extra),     # the synthetic generators on the device
         ("draw_prior", os.path.join(CSRC, "draw_prior.hip"), extra),  # the initial rho prior on the device
         ("ppc", os.path.join(CSRC, "ppc.hip"), extra),                # expected reports and report AUC
         ("netstats", os.path.join(CSRC, "netstats.hip"), extra),      # network statistics of posterior samples
         ("triads", os.path.join(CSRC, "triads.hip"), extra),          # triad statistics of posterior samples and their expectations
         ("mixing", os.path.join(CSRC, "mixing.hip"), extra),          # mixing by node attribute and overlap between layers
         ("connectivity", os.path.join(CSRC, "connectivity.hip"), extra),  # components, reach and path lengths of posterior samples
         ("centrality", os.path.join(CSRC, "centrality.hip"), extra),  # diffusion centrality of posterior samples and of the mean network
         ("betweenness", os.path.join(CSRC, "betweenness.hip"), extra),  # betweenness centrality of posterior samples and of given networks
         ("cores", os.path.join(CSRC, "cores.hip"), extra),            # k-core decomposition of posterior samples and of given networks
         ("cascades", os.path.join(CSRC, "cascades.hip"), extra),      # independent cascades on posterior samples and on given networks
         ("census", os.path.join(CSRC, "census.hip"), extra),          # the 16-class triad census of posterior samples and of given networks
         ("partners", os.path.join(CSRC, "partners.hip"), extra),      # shared partners of the ties of posterior samples and of given networks
         ("holes", os.path.join(CSRC, "holes.hip"), extra),            # structural holes of posterior samples and of given networks
         ("cutpoints", os.path.join(CSRC, "cutpoints.hip"), extra),    # cut points, bridges and fragmentation of posterior samples and of given networks
         ("ppc_rep", os.path.join(CSRC, "ppc_rep.hip"), extra),        # posterior predictive replicates, reduced
         ("edge_table", os.path.join(CSRC, "edge_table.hip"), extra),  # the inferred network as an edge table
         ("score_truth", os.path.join(CSRC, "score_truth.hip"), extra),  # the posterior scored against a ground truth
         ("reporter_table", os.path.join(CSRC, "reporter_table.hip"), extra),  # each reporter's reports against the posterior
         ("heldout", os.path.join(CSRC, "heldout.hip"), extra),        # held-out reports scored under the posterior
         ("report_scores", os.path.join(CSRC, "report_scores.hip"), extra),  # every report of the support scored under the posterior
         ("influence", os.path.join(CSRC, "influence.hip"), extra)]    # the leave-one-reporter-out posterior of every element
    dev_ks = tuple(int(k) for k in os.environ.get("VMR_DEV_KS", "2").split(","))   # (VMR_DEV_KS=2,3: also the K = 3 sweep kernels)
    for k in (dev_ks if dev else KS):
        u.append((f"sweep_sl_k{k}", os.path.join(CSRC, "sweep_sl.hip"), extra + [f"-DVMR_K={k}"]))
    return u


def _stale(obj, src):
    if not os.path.exists(obj):
        return True
    t = os.path.getmtime(obj)
    return any(os.path.getmtime(d) > t for d in [src] + HEADERS)


def needs_build() -> bool:
    dev = bool(os.environ.get("VMR_DEV"))
    tag = os.path.join(OBJ, "dev" if dev else "full")
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(d) > t for d in [u[1] for u in units(dev)] + HEADERS) or not os.path.exists(tag)


def build(force: bool = False, verbose: bool = False) -> str:
    """VMR_CXXFLAGS adds compiler flags (kernel experiments: -DSL_WPE=5 ...), VMR_TAG keeps such a build's objects apart
    (csrc/_obj/<tag>), VMR_LIB_OUT names the library -- tools/ab_bench.sh picks builds with VMR_LIB."""
    tagged = bool(os.environ.get("VMR_TAG"))
    if not force and not tagged and not needs_build():
        return LIB
    dev = bool(os.environ.get("VMR_DEV"))
    odir = os.path.join(OBJ, os.environ.get("VMR_TAG") or ("dev" if dev else "full"))
    more = os.environ.get("VMR_CXXFLAGS", "").split()
    os.makedirs(odir, exist_ok=True)
    todo, objs = [], []
    for name, src, extra in units(dev):
        obj = os.path.join(odir, name + ".o")
        objs.append(obj)
        if force or _stale(obj, src):
            todo.append([HIPCC] + FLAGS + extra + more + ["-c", src, "-o", obj])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    jobs = os.environ.get("VMR_BUILD_JOBS") or os.environ.get("MAX_JOBS") or os.cpu_count() or 1   # (a shared machine: its CPU count is not ours)
    workers = max(1, min(len(todo), int(jobs)))
    if todo:
        with ThreadPoolExecutor(max_workers=workers) as ex:
            list(ex.map(run, todo))
    run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs)
    return LIB


def build_host(force: bool = False, verbose: bool = False) -> str:
    """The host-side helper (initial-state draw, plain C): gcc, no FMA contraction (NumPy rounds twice)."""
    if not force and os.path.exists(HOST_LIB) and os.path.getmtime(HOST_LIB) >= os.path.getmtime(HOST_SRC):
        return HOST_LIB
    cmd = [os.environ.get("CC", "gcc"), "-O3", "-fPIC", "-shared", "-std=c11", "-ffp-contract=off", "-o", HOST_LIB, HOST_SRC]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return HOST_LIB


if __name__ == "__main__":
    print(build_host(force=True, verbose=True))
    print(build(force="--force" in __import__("sys").argv, verbose=True))
