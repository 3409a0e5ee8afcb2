#!/usr/bin/env python3
"""Generate tests/golden/ppc/P_mean_poisson_<case>.npz from the REAL reference (build container only).

For the golden cases A, B, C, D, E and L, refits the reference's `VimureModel` with the configuration stored in the case's
fixture (tools/make_golden.py), checks that the refit's `*_f` arrays equal the stored `fit_*` ones, and records:
  mp_subs, mp_vals   `_calculate_mean_poisson()` (model.py:1220-1293) of the fitted model
  auc_layer [L]      `utils.calculate_AUC(mp.toarray()[l], X[l], mask=R[l])` (utils.py:40-66)
  auc_all            `utils.calculate_AUC(mp.toarray(), X, mask=R)`

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_ppc.py
The reference never travels: only these data vectors are committed.  (A directory of their own: tests/golden_util.case_names
takes every tests/golden/*.npz for a model case.)
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/src/python"
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(HERE, "oracle_stubs"))
warnings.filterwarnings("ignore")

from vimure.model import VimureModel  # noqa: E402
from vimure.utils import calculate_AUC  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(HERE), "tests", "golden")
CASES = ("A_ones_mut", "B_random_mask_K3", "C_ones_nomut", "D_self_mask", "E_undirected", "L_default_K12")


def refit(d):
    X, R = d["X"].astype(np.int64), d["R"].astype(np.int64)
    kw = {k[len("fitarg_"):]: d[k].item() for k in d.files if k.startswith("fitarg_")}
    kw.update({k[len("prior_"):]: d[k] for k in d.files if k.startswith("prior_")})
    if "K_given" not in d.files or int(d["K_given"]):
        kw["K"] = int(d["K"])
    m = VimureModel(mutuality=bool(d["mutuality"]), undirected=bool(d["undirected"]))
    m.fit(X.copy(), R=R.copy(), seed=int(d["seed"]), **kw)
    for n in ("gamma_shp_f", "gamma_rte_f", "phi_shp_f", "phi_rte_f", "nu_shp_f", "nu_rte_f", "rho_f",
              "G_exp_theta_f", "G_exp_lambda_f", "G_exp_nu_f"):
        assert np.array_equal(np.asarray(getattr(m, n), dtype=np.float64), d["fit_" + n]), n
    return m, X, R


def main():
    for case in CASES:
        d = np.load(os.path.join(GOLDEN, case + ".npz"))
        m, X, R = refit(d)
        mp = m._calculate_mean_poisson()
        dense = np.zeros(X.shape)   # (mp.toarray() with the full shape: the sptensor's own is the subscripts' extent)
        dense[tuple(np.asarray(s) for s in mp.subs)] = mp.vals
        out = {
            "mp_subs": np.stack([np.asarray(s) for s in mp.subs]).astype(np.int16),
            "mp_vals": np.asarray(mp.vals, dtype=np.float64),
            "auc_layer": np.array([calculate_AUC(dense[l], X[l], mask=R[l]) for l in range(X.shape[0])]),
            "auc_all": np.array(calculate_AUC(dense, X, mask=R)),
        }
        path = os.path.join(GOLDEN, "ppc", "P_mean_poisson_" + case.split("_")[0] + ".npz")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        np.savez_compressed(path, **out)
        print(f"{case}: |S| = {len(out['mp_vals'])}, AUC per layer {out['auc_layer']}, all {out['auc_all']} -> "
              f"{os.path.getsize(path)} B")


if __name__ == "__main__":
    main()
