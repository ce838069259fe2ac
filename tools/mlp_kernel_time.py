"""Device time of one fused exact-GP evaluation at N = 16384, D = 32 (noise 0.1) of an ARD `RBF` (the yardstick), of a lone ARD
`MLP`, of a lone `Poly` (order 2) and of `RBF + MLP + Bias`, in that order in one process, with the stage times of the library
(kbuild, potrf, trtri, lauum, solve, grad, total: hipEvent timings, MI355GP_T_*).  Median over the timed evaluations after the
warm-up ones; one JSON line per size.  A library without the two kinds (the parent of the change that added them) reports the
RBF evaluation alone.  The new kernels' own times come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/mlp_kernel_time.py`.

    python tools/mlp_kernel_time.py [--n 16384] [--d 32] [--reps 5] [--warmup 3]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpy_amd import _lib as L  # noqa: E402


def median_ms(ctx, specs, reps, warmup):
    """per-stage median over `reps` timed evaluations after `warmup` untimed ones"""
    runs = []
    for r in range(warmup + reps):
        info, res = ctx.exact_inference_sum(specs, 0.1, want_stage_ms=True)
        assert info == 0, info
        if r >= warmup:
            runs.append(res["stage_ms"])
    return {k: float(np.median([m[k] for m in runs])) for k in runs[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[16384])
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    D = a.d
    dims = np.arange(D)
    rbf = ("rbf", 1, np.concatenate([[1.0], np.linspace(0.5, 2.0, D) * np.sqrt(D / 8.0)]), dims, 0)
    mlp = ("mlp", 1, np.concatenate([[1.0], np.linspace(0.5, 1.5, D) / D, [0.5]]), dims, 0)
    poly = ("poly", 0, np.array([1.0, 1.0 / D, 1.0, 2.0]), dims, 0)
    bias = ("bias", 0, np.array([0.5]), dims, 0)
    for n in a.n:
        rng = np.random.default_rng(n)
        X = rng.standard_normal((n, D))
        y = np.tanh(X @ (rng.standard_normal(D) / np.sqrt(D))) + np.sin(X[:, 0]) + 0.1 * rng.standard_normal(n)
        out = {"N": n, "D": D}
        c = L.Context(0)
        try:
            c.set_data(X, y[:, None])
            out["rbf_ms"] = median_ms(c, [rbf], a.reps, a.warmup)
            if "mlp" in L.KIND_IDS:
                try:
                    out["mlp_ms"] = median_ms(c, [mlp], a.reps, a.warmup)
                except L.MI355GPError:                     # MI355GP_LIB points at a library that predates the kinds
                    out["mlp_ms"] = None
            if out.get("mlp_ms") is not None:
                out["poly_ms"] = median_ms(c, [poly], a.reps, a.warmup)
                out["rbf_mlp_bias_ms"] = median_ms(c, [rbf, mlp, bias], a.reps, a.warmup)
                for key in ("mlp_ms", "poly_ms", "rbf_mlp_bias_ms"):
                    out["ratio_" + key[:-3] + "_total"] = out[key]["total"] / out["rbf_ms"]["total"]
        finally:
            c.close()
        print(json.dumps(out))


if __name__ == "__main__":
    main()
