"""Device time of one fused `exact_inference_sum` of the Mauna-Loa composite RBF + RBF * StdPeriodic + RatQuad + White
against one single-RBF evaluation on the same data (D = 1, calendar-year inputs), with the stage times of the library
(kbuild, potrf, trtri, lauum, solve, grad, total: hipEvent timings, MI355GP_T_*).  Minimum over the timed repetitions.
The new kernels' own times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/periodic_kernels_time.py`.

    python tools/periodic_kernels_time.py [--n 4096 16384] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpy_amd import _lib as L  # noqa: E402

COMPOSITE = [("rbf", 0, np.array([1.0, 30.0]), np.array([0]), 0), ("rbf", 0, np.array([0.3, 60.0]), np.array([0]), 1),
             ("stdperiodic", 0, np.array([1.0, 1.0, 1.2]), np.array([0]), 1),
             ("ratquad", 0, np.array([0.2, 1.5, 0.8]), np.array([0]), 0), ("white", 0, np.array([0.02]), None, 0)]
RBF = [("rbf", 0, np.array([1.0, 30.0]), np.array([0]), 0)]


def best(ctx, specs, reps):
    """per-stage minimum over `reps` timed evaluations (after two warm-up evaluations)"""
    out = None
    for r in range(reps + 2):
        info, res = ctx.exact_inference_sum(specs, 0.05, want_stage_ms=True)
        assert info == 0, info
        if r >= 2:
            ms = res["stage_ms"]
            out = dict(ms) if out is None else {k: min(out[k], ms[k]) for k in ms}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    for n in a.n:
        rng = np.random.default_rng(n)
        x = np.sort(1958.0 + 62.0 * rng.random(n))
        y = 0.02 * (x - 1958.0) + 0.5 * np.sin(2 * np.pi * x) + 0.1 * rng.standard_normal(n)
        c = L.Context(0)
        try:
            c.set_data(x[:, None], y[:, None])
            comp = best(c, COMPOSITE, a.reps)
            single = best(c, RBF, a.reps)
        finally:
            c.close()
        print(json.dumps({"N": n, "D": 1, "composite_ms": comp, "rbf_ms": single,
                          "ratio_total": comp["total"] / single["total"]}))


if __name__ == "__main__":
    main()
