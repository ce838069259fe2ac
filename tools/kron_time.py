"""Time of grid regression on G x G x G grids: one evaluation (mi355gp_kron_solve + mi355gp_kron_quadforms for the D + 2 = 5
parameters) and one mode product alone, by HIP events on the context's stream (the library records them around the mode products
and the scaling kernel; the two-stage sums and their read-backs are outside the events and inside the wall clock, which is given
next to them).  Two warm-ups, then the median of `--reps`.  The host's share -- K_d, derivative factors, `numpy.linalg.eigh` and
the gammas -- is timed separately.  Each mode product is set against 16 N bytes at the HBM copy rate and 2 N G flops at the fp64
MFMA rate that csrc/peaks.hip measures on the same device in the same run.  Records, not pass / fail bars; nothing is tuned.

    python tools/kron_time.py --sizes 128 256 --out profiles
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gpy_amd import _lib as L  # noqa: E402
import kron_ld as KR  # noqa: E402


def host_inputs(xg, variance, ls):
    Kds, factors = KR.grid_factors(xg, variance, ls, np.float64)
    e = [np.linalg.eigh(Kd) for Kd in Kds]
    Qs, lams = [q for _, q in e], [lam for lam, _ in e]
    return Qs, lams, factors, KR.gammas_of(Qs, factors, np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="directory for kron_time_g<G>.json")
    a = ap.parse_args()
    peaks = L.dbg_peaks()
    for G in a.sizes:
        rng = np.random.default_rng(G)
        D, N = 3, G ** 3
        xg = [np.sort(rng.random(G)) * 0.25 * G for _ in range(D)]
        ls, variance, noise = np.array([1.1, 1.6, 0.9]), 1.3, 0.1
        y = rng.standard_normal(N)
        host_ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            Qs, lams, factors, gammas = host_inputs(xg, variance, ls)
            host_ms.append((time.perf_counter() - t0) * 1e3)
        ctx = L.KronContext()
        ctx.set_data([G] * D, y)
        ev, wall = [], []
        for rep in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            ctx.solve(Qs, lams, noise + 1e-8)
            ctx.quadforms(factors, gammas)
            w = (time.perf_counter() - t0) * 1e3
            if rep >= a.warmup:
                ev.append(ctx.last_ms())
                wall.append(w)
        x = rng.standard_normal((N // G, G))
        mode = []
        for rep in range(a.warmup + a.reps):
            ms = ctx.mode_probe(Qs[0], x)[1]
            if rep >= a.warmup:
                mode.append(ms)
        ctx.close()
        m = float(np.median(mode))
        n_products = 2 * D + (D + 1) * D           # Q^T and Q passes, D products for each non-identity parameter set
        out = {"grid": [G] * D, "N": N, "reps": a.reps, "warmup": a.warmup, "tuned": "not tuned",
               "clock": "HIP events on the context's stream around the mode products; wall clock around solve + quadforms",
               "host_Kd_eigh_factors_ms": float(np.median(host_ms)), "evaluation_event_ms": float(np.median(ev)),
               "evaluation_wall_ms": float(np.median(wall)), "mode_products_per_evaluation": n_products,
               "mode_product_ms": m, "mode_product_GBs_of_16N": 16.0 * N / (m * 1e-3) / 1e9,
               "mode_product_TFs_of_2NG": 2.0 * N * G / (m * 1e-3) / 1e12,
               "peaks_hbm_copy_GBs": float(peaks["hbm_copy_gbs"]), "peaks_mfma_f64_TFs": float(peaks["mfma_f64_tflops"]),
               "all": {"evaluation_event_ms": ev, "evaluation_wall_ms": wall, "mode_product_ms": mode}}
        out["mode_product_share_of_hbm_rate"] = out["mode_product_GBs_of_16N"] / out["peaks_hbm_copy_GBs"]
        out["mode_product_share_of_mfma_rate"] = out["mode_product_TFs_of_2NG"] / out["peaks_mfma_f64_TFs"]
        print(json.dumps(out), flush=True)
        if a.out:
            with open(os.path.join(a.out, "kron_time_g%d.json" % G), "w") as f:
                json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
