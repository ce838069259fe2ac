"""Writes tests/golden/kernel_shapes/floor.npz: for every fused case of tests/test_gpu_kernel_shapes.py (kernel variant x
sweep shape x expression, and the Student-t cases) how far an fp64 pipeline -- the formulas of tests/kern_ld.py in double
precision, SciPy's Cholesky (LAPACK dpotrf / dpotrs) for the solves -- lies from the long-double pipeline of the same module,
per dtheta entry, in units of eps64 x cond (cond = sum_ij |dL_dK_ij dK_ij/dtheta_k| from the long-double solution).  The
largest such figure of a case is what is stored; the GPU test allows ten times it, and never less than 256.

Needs no GPU and no reference tree; an x86 host (80-bit long double).

    python tools/make_golden_kernel_shapes.py
"""
import os
import sys

import numpy as np
from scipy.linalg import cho_factor, cho_solve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kern_ld as KL  # noqa: E402

NU = 4.5


def fp64_dtheta(specs, X, Y, noise, nu=None, jitter=1e-8):
    N, Dy = Y.shape
    K = KL.K(specs, X, dt=np.float64)
    Ky = K + ((0.0 if nu is not None else noise) + jitter) * np.eye(N)
    c = cho_factor(Ky, lower=True)
    Ki = cho_solve(c, np.eye(N))
    alpha = cho_solve(c, Y)
    if nu is None:
        G = 0.5 * (alpha @ alpha.T - Dy * Ki)
    else:
        G = 0.5 * ((nu + N) / (nu + np.sum(alpha * Y) - 2.0) * alpha @ alpha.T - Ki)
    return KL.dtheta(specs, G, X, dt=np.float64)[0]


def figure(specs, X, Y, noise, nu=None):
    ex = KL.exact(specs, X, Y, noise, nu)
    return KL.grad_figure(fp64_dtheta(specs, X, Y, noise, nu), ex["dtheta"], ex["dtheta_cond"])


def main():
    KL.require_ld()
    names, figs = [], []
    for v in KL.VARIANTS:
        for s in KL.SHAPES:
            c = KL.make_case(v, s)
            for label, specs, X, _ in KL.fused_exprs(c):
                names.append(KL.case_id(v, s) + "-" + label)
                figs.append(figure(specs, X, c["Y"], c["noise"]))
                if label == "plus_white" and tuple(s) == KL.STUDENTT_SHAPE:
                    names.append(KL.case_id(v, s) + "-studentt")
                    figs.append(figure(specs, X, c["Y"], 0.0, NU))
            print(names[-1], " ".join("%.1f" % f for f in figs[-4:]), flush=True)
    out = os.path.join(ROOT, "tests", "golden", "kernel_shapes", "floor.npz")
    np.savez_compressed(out, names=np.array(names), figures=np.array(figs), nu=NU)
    print("wrote", out, len(names), "cases, worst figure %.1f" % max(figs))


if __name__ == "__main__":
    main()
