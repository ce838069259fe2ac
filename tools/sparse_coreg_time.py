"""Times VarDTC with an ICM kernel (stationary x Coregionalize) on the MI355X next to its neighbours, in one run:
`mi355gp_vardtc_inference_sum` by HIP events on the launching stream (the entry point's own `stage_ms`: pass 1, M x M, pass 2,
total) for

    rbf_hom     one RBF ARD part over all D columns with ONE noise variance (the fused single-part passes; the evaluation
                profiles/sparse_lin_time_*.json has as `rbf`)
    rbf         the same with the per-point noise vector the other rows use
    rbf*bias    RBF ARD x Bias: the product route with a second factor that costs nothing to evaluate -- the other factor's
                K-build, `form_times`, the gradient kernel with H written, the column reduction, per factor
    icm_rbf     RBF ARD on the D - 1 spatial columns x Coregionalize on the last (P = 4 outputs, rows sorted by output, W of rank
                1) through k_grad_cols_icm: both factors' gradients from one pass over the chunk's weights
    icm_rbf_product   the same kernel with the context's fused passes off (`mi355gp_dbg_sparse_set_fuse_cols`): the product
                route with the lookup build and the bucketed pass as the second factor's kernels

at N = 200000, M = 2048, D = 16, Dy = 1 (the sparse configuration of BASELINE.json) and N = 8192, M = 256, with one noise
variance per output handed over by point, as MixedNoise does.  Medians of 7 after 2 warm-ups.  A record, no gate.

    python tools/sparse_coreg_time.py [--reps 7] [--out profiles]     (needs the GPU; writes profiles/sparse_coreg_time_<shape>.json)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gpy_amd import _lib  # noqa: E402

SHAPES = [dict(name="n200000_m2048_d16", N=200000, M=2048, D=16), dict(name="n8192_m256_d16", N=8192, M=256, D=16)]
STAGES = ("pass1", "mxm", "pass2", "total")
P = 4


def inputs(sh, seed=0):
    rng = np.random.default_rng(seed)
    N, M, D = sh["N"], sh["M"], sh["D"]
    X = rng.uniform(-0.5, 0.5, (N, D))
    X[:, D - 1] = np.sort(np.arange(N) % P)                     # rows sorted by output, as build_XY stacks them
    idx = X[:, D - 1].astype(int)
    Y = np.sin(X[:, :3].sum(1) + 0.5 * idx)[:, None] + X[:, :1] + 0.1 * rng.standard_normal((N, 1))
    Z = X[np.sort(rng.permutation(N)[:M])].copy()
    allq, sp = np.arange(D, dtype=np.int32), np.arange(D - 1, dtype=np.int32)
    W = np.array([0.6, 0.4, -0.3, 0.5])
    B = np.outer(W, W) + np.diag([0.5, 0.6, 0.7, 0.8])
    kernels = {"rbf": [("rbf", 1, np.concatenate([[1.0], np.full(D, 1.5)]), allq, 0)],
               "rbf*bias": [("rbf", 1, np.concatenate([[1.0], np.full(D, 1.5)]), allq, 1), ("bias", 0, np.array([1.0]), allq, 1)],
               "icm_rbf": [("rbf", 1, np.concatenate([[1.0], np.full(D - 1, 1.5)]), sp, 1),
                           ("coregionalize", P, B.ravel(), np.array([D - 1], dtype=np.int32), 1)]}
    noise = (0.01 + 0.002 * np.arange(P))[idx]
    return X, Y, Z, kernels, noise


def run(sh, reps, warmup=2):
    X, Y, Z, kernels, noise = inputs(sh)
    ctx = _lib.SparseContext(0)
    ctx.set_coregionalize(True)
    ctx.set_data(X, Y)
    res = dict(shape=dict((k, sh[k]) for k in ("N", "M", "D")), P=P, Dy=1, reps=reps, warmup=warmup, noise="one variance per output, by point")
    runs = [("rbf_hom", kernels["rbf"], 0.01, True)] + [(k, v, noise, True) for k, v in kernels.items()]
    runs.append(("icm_rbf_product", kernels["icm_rbf"], noise, False))
    for name, specs, nz, fuse in runs:
        ts = []
        ctx.set_fuse_cols(fuse)
        for it in range(warmup + reps):
            info, r = ctx.vardtc_sum(specs, Z, nz, extra_jitter=1e-5, want_stage_ms=True)   # one fixed rung: Z is drawn from X
            assert info == 0, "Kmm or B not positive definite at the timing shape (%s, info %d)" % (name, info)
            if it >= warmup:
                ts.append(r["stage_ms"])
        for k in STAGES:
            res["%s_%s_ms" % (name, k)] = float(np.median([s[k] for s in ts]))
        res["%s_total_ms_min_max" % name] = [min(s["total"] for s in ts), max(s["total"] for s in ts)]
        res["%s_log_marginal" % name] = float(r["lml"])
    res["pass2_ms_over_rbf"] = dict((k, res[k + "_pass2_ms"] - res["rbf_pass2_ms"]) for k in ("rbf*bias", "icm_rbf", "icm_rbf_product"))
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    _lib.require_device(0)
    os.makedirs(a.out, exist_ok=True)
    for sh in SHAPES:
        res = run(sh, a.reps)
        with open(os.path.join(a.out, "sparse_coreg_time_%s.json" % sh["name"]), "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
        print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
