#!/usr/bin/env python3
"""Generate tests/golden/netstats/Q_netstats_<case>.npz from the REAL reference (build container only).

For the golden cases A, B, C, D, E, L and M, from the case's stored `fit_rho_f` (tools/make_golden.py), per layer:
  reciprocity [L]            the reference's `utils.calculate_overall_reciprocity` (utils.py:69-70) of np.argmax(fit_rho_f, -1)[l]
  expected_reciprocity [L]   the quotient of the reference's reciprocity notebook, einsum("ij,ji->", p, p) / p.sum(), of
                             p = fit_rho_f[l][..., 1:].sum(-1)
  edges [L]                  edges of the argmax network (every layer must have some: the first quotient is then defined)

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_netstats.py
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

from vimure.utils import calculate_overall_reciprocity  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(HERE), "tests", "golden")
CASES = ("A_ones_mut", "B_random_mask_K3", "C_ones_nomut", "D_self_mask", "E_undirected", "L_default_K12", "M_K16_nomut")


def main():
    for case in CASES:
        rho = np.load(os.path.join(GOLDEN, case + ".npz"))["fit_rho_f"]
        Y = np.argmax(rho, axis=-1)
        edges = np.array([int((Y[l] > 0).sum()) for l in range(Y.shape[0])], dtype=np.int64)
        assert edges.min() > 0, (case, edges)
        rec = np.array([calculate_overall_reciprocity(Y[l]) for l in range(Y.shape[0])], dtype=np.float64)
        exp = []
        for l in range(rho.shape[0]):
            p = rho[l][..., 1:].sum(-1)
            exp.append(np.einsum("ij,ji->", p, p) / p.sum())
        out = {"reciprocity": rec, "expected_reciprocity": np.array(exp, dtype=np.float64), "edges": edges}
        path = os.path.join(GOLDEN, "netstats", "Q_netstats_" + case.split("_")[0] + ".npz")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        np.savez_compressed(path, **out)
        print(f"{case}: edges {edges}, reciprocity {rec}, expected {out['expected_reciprocity']} -> {os.path.getsize(path)} B")


if __name__ == "__main__":
    main()
