"""Time of one evaluation and one prediction of the Kronecker GP session (`mi355gp_kgpr_*`, csrc/kgpr.hip) at (N1, N2) = (512, 512)
and (2048, 1024), split as the C-ABI's `get_ms` splits it -- eigh, rotations, the spectral pass, the two weighted-SYRK launches,
transfers -- and of `k_kgpr_wsyrk` alone next to `launch_gemm` (NT) on a pre-scaled copy of the same two panels:

    python tools/kgpr_time.py [--shapes 512x512,2048x1024] [--out profiles/kgpr_time_<shapes>.json]

HIP events throughout; the session's figures are medians of 7 calls after 2 warm-ups, the two kernels alone the mean of 7 launches
after one.  The GEMM computes all n^2 outputs from a copy somebody would first have to write; the SYRK kernel computes the lower
tiles and mirrors them.  A record, no bar."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gpy_amd import _lib  # noqa: E402

M_NEW = 256                    # new points per side of the timed prediction


def factor(n, ls, seed, matern):
    x = np.sort(np.random.default_rng(seed).uniform(0.0, 10.0, n))
    r = np.abs(x[:, None] - x[None, :]) / ls
    return ((1 + np.sqrt(3.) * r) * np.exp(-np.sqrt(3.) * r)) if matern else np.exp(-0.5 * r * r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="512x512,2048x1024")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for shape in a.shapes.split(","):
        N1, N2 = (int(s) for s in shape.split("x"))
        rng = np.random.default_rng(N1 + N2)
        K1, K2, Y = factor(N1, 1.5, 1, False), factor(N2, 1.0, 2, True), rng.standard_normal((N1, N2))
        ctx = _lib.KgprContext()
        ctx.set_data(Y)
        k1xf, k2xf = rng.standard_normal((M_NEW, N1)), rng.standard_normal((M_NEW, N2))
        recs = []
        for _ in range(9):
            sweeps = ctx.inference(K1, K2, 0.1)[4]
            ctx.predict(k1xf, k2xf, np.ones(M_NEW), np.ones(M_NEW))
            recs.append(ctx.last_ms())
        row = {"N1": N1, "N2": N2, "sweeps": list(sweeps), "new_points": [M_NEW, M_NEW],
               "ms": {k: float(np.median([r[k] for r in recs[2:]])) for k in recs[0]}}
        # the hot kernel alone at the shape of dL_dK1, against the tile GEMM on a pre-scaled copy
        Pa, Pb, da, db = rng.standard_normal((N1, N2)), rng.standard_normal((N1, N1)), rng.standard_normal(N2), rng.standard_normal(N1)
        C, ms_w = _lib.kgpr_wsyrk(Pa, da, Pb, db, reps=7)
        P = np.concatenate([Pa, Pb], 1)
        G, ms_g = _lib.dbg_gemm(P * np.concatenate([da, db]), P, np.zeros((N1, N1)), 0, 0, alpha=0.5, reps=7)
        row["wsyrk_alone"] = {"n": N1, "panel_widths": [N2, N1], "wsyrk_ms": ms_w, "gemm_nt_prescaled_ms": ms_g,
                              "max_abs_difference": float(np.abs(C - G).max())}
        print(json.dumps(row), flush=True)
        rows.append(row)
        ctx.close()
    out = a.out or os.path.join(ROOT, "profiles", "kgpr_time_%s.json" % "_".join(a.shapes.split(",")))
    with open(out, "w") as f:
        json.dump({"factors": "K1 RBF (lengthscale 1.5), K2 Matern32 (lengthscale 1.0), sorted uniform 1-D inputs on [0, 10], noise 0.1",
                   "ms": "medians of 7 after 2 warm-ups, HIP events; keys as KgprContext.MS_NAMES",
                   "unmeasured": "no CPU or torch baseline of the whole model; no other shapes; the host-side kernel builds (kern.K, "
                                 "update_gradients_full) are outside these figures", "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
