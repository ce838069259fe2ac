"""Device time of one fused `exact_inference_sum` of an ICM kernel, Matern52 ARD (D = 32) x Coregionalize (P = 4), against one
plain Matern52 ARD evaluation of bench.py's headline configuration (N = 16384, D = 32) on the same inputs, with the stage times
of the library (kbuild, potrf, trtri, lauum, solve, grad, total: hipEvent timings, MI355GP_T_*).  Rows are sorted by output,
as build_XY stacks them.  Minimum over the timed repetitions.  The product costs one extra K-build per factor in the gradient
pass (each factor's gradient is weighted by the other factor's covariance) plus the bucketed pass.

    python tools/coreg_time.py [--n 16384] [--reps 5] [--shuffle]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpy_amd import _lib as L  # noqa: E402


def best(ctx, specs, noise, reps):
    """per-stage minimum over `reps` timed evaluations (after two warm-up evaluations)"""
    out = None
    for r in range(reps + 2):
        info, res = ctx.exact_inference_sum(specs, noise, want_diag=True, want_stage_ms=True)
        assert info == 0, info
        if r >= 2:
            ms = res["stage_ms"]
            out = dict(ms) if out is None else {k: min(out[k], ms[k]) for k in ms}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[16384])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shuffle", action="store_true", help="rows in random output order (many output pairs per tile)")
    a = ap.parse_args()
    D, P = 32, 4
    ls = np.linspace(2.0, 6.0, D)
    W = np.array([[0.9], [-0.5], [0.7], [0.3]])
    B = W @ W.T + np.diag([0.5, 0.4, 0.6, 0.3])
    noises = np.array([0.1, 0.05, 0.2, 0.1])
    for n in a.n:
        rng = np.random.default_rng(n)
        idx = np.sort(rng.integers(0, P, n))
        if a.shuffle:
            idx = rng.permutation(idx)
        Xin = rng.standard_normal((n, D))
        y = np.sin(Xin[:, :4].sum(1)) * (1.0 + 0.2 * idx) + 0.1 * rng.standard_normal(n)
        icm = [("matern52", 1, np.concatenate([[1.0], ls]), np.arange(D), 1),
               ("coregionalize", P, B.ravel(), np.array([D]), 1)]
        plain = [("matern52", 1, np.concatenate([[1.0], ls]), np.arange(D), 0)]
        c1, c2 = L.Context(0), L.Context(0)
        try:
            c1.set_data(np.hstack([Xin, idx[:, None].astype(float)]), y[:, None])
            coreg = best(c1, icm, noises[idx], a.reps)
            c1.close()
            c2.set_data(Xin, y[:, None])
            single = best(c2, plain, 0.1, a.reps)
        finally:
            c1.close()
            c2.close()
        print(json.dumps({"N": n, "D": D, "P": P, "shuffled": bool(a.shuffle), "icm_ms": coreg, "matern52_ms": single,
                          "ratio_total": coreg["total"] / single["total"]}))


if __name__ == "__main__":
    main()
