"""Times the Linear / Bias psi-statistics on the MI355X, in one run, by HIP events on the launching stream (the entry points' own
`stage_ms`: pass 1, M x M, pass 2, total).  Medians of 7 after 2 warm-ups.  A record, no gate.

    n200000_m2048_d16        Linear ARD + Bias + White, Dy = 1: `mi355gp_vardtc_inference_uncertain` (inputs N(mu, diag S)) next to
                             the certain-input `mi355gp_vardtc_inference_sum` of the same expression at X = mu.  By arithmetic
                             the uncertain evaluation adds one more read of each chunk's weights (k_grad_rows_lin: N M doubles)
                             and N D-sized passes to the 3 N M^2 flops of the two Gram products.
    n8192_m256_q8_dy12       uncertain RBF ARD + Bias next to uncertain RBF ARD (the Bias parts add M-sized work per chunk).
    row kernel               k_grad_rows_lin alone (`mi355gp_dbg_psi_lin_rows`, weights formed on the fly from W and a rank
                             term with Dy = 1) at 32768 x 2048, D = 16: bytes of one read of W and one read / write of the rows
                             over its time (the median of 7 launches timed one by one after 2 warm-ups), next to the copy figure of
                             peaks.hip (`mi355gp_dbg_peaks`).

    python tools/psi_lin_time.py [--reps 7] [--out profiles]     (needs the GPU; writes profiles/psi_lin_time_<shape>.json)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gpy_amd import _lib  # noqa: E402

STAGES = ("pass1", "mxm", "pass2", "total")


def _median_stages(res, name, ts):
    for k in STAGES:
        res["%s_%s_ms" % (name, k)] = float(np.median([s[k] for s in ts]))
    res["%s_total_ms_min_max" % name] = [min(s["total"] for s in ts), max(s["total"] for s in ts)]


def linear_shape(reps, warmup, N=200000, M=2048, D=16):
    rng = np.random.default_rng(0)
    mu, S = rng.uniform(-0.5, 0.5, (N, D)), rng.uniform(0.01, 0.05, (N, D))
    Y = mu @ (rng.standard_normal((D, 1)) / np.sqrt(D)) + 0.3 + 0.1 * rng.standard_normal((N, 1))
    Z = mu[rng.permutation(N)[:M]].copy()
    w = 1.0 + 0.5 * np.arange(D)
    specs = [("linear", 1, w / w.sum(), None, 0), ("bias", 0, np.array([0.5]), None, 0), ("white", 0, np.array([0.05]), None, 0)]
    ctx = _lib.SparseContext(0)
    ctx.set_psi_lin_bias(True)
    ctx.set_data(mu, Y)
    ctx.set_input_variance(S)
    res = dict(shape=dict(N=N, M=M, D=D), Dy=1, reps=reps, warmup=warmup, kernel="linear_ard+bias+white")
    for name, call in (("certain", lambda: ctx.vardtc_sum(specs, Z, 0.01, want_stage_ms=True)),
                       ("uncertain", lambda: ctx.vardtc_uncertain(specs, Z, 0.01, want_stage_ms=True))):
        ts = []
        for it in range(warmup + reps):
            info, r = call()
            assert info == 0, "Kmm or B not positive definite at the timing shape (%s, info %d)" % (name, info)
            if it >= warmup:
                ts.append(r["stage_ms"])
        _median_stages(res, name, ts)
        res["%s_log_marginal" % name] = float(r["lml"])
    res["uncertain_over_certain"] = res["uncertain_total_ms"] / res["certain_total_ms"]
    ctx.close()
    return "n%d_m%d_d%d" % (N, M, D), res


def rbf_shape(reps, warmup, N=8192, M=256, Q=8, Dy=12):
    rng = np.random.default_rng(1)
    mu, S = rng.uniform(-2, 2, (N, Q)), rng.uniform(0.05, 0.5, (N, Q))
    Y = np.sin(mu.sum(1, keepdims=True) / np.sqrt(Q) + np.arange(Dy)[None, :]) + 0.3 + 0.1 * rng.standard_normal((N, Dy))
    Z = mu[rng.permutation(N)[:M]].copy()
    rbf = ("rbf", 1, np.concatenate([[1.3], np.full(Q, 2.5)]), None, 0)
    ctx = _lib.SparseContext(0)
    ctx.set_psi_lin_bias(True)
    ctx.set_data(mu, Y)
    ctx.set_input_variance(S)
    res = dict(shape=dict(N=N, M=M, Q=Q), Dy=Dy, reps=reps, warmup=warmup)
    for name, specs in (("rbf", [rbf]), ("rbf+bias", [rbf, ("bias", 0, np.array([0.5]), None, 0)])):
        ts = []
        for it in range(warmup + reps):
            info, r = ctx.vardtc_uncertain(specs, Z, 0.05, extra_jitter=1e-5, want_stage_ms=True)   # one fixed rung: Z is drawn from mu
            assert info == 0, "Kmm or B not positive definite at the timing shape (%s, info %d)" % (name, info)
            if it >= warmup:
                ts.append(r["stage_ms"])
        _median_stages(res, name, ts)
        res["%s_log_marginal" % name] = float(r["lml"])
    res["bias_over_plain"] = res["rbf+bias_total_ms"] / res["rbf_total_ms"]
    ctx.close()
    return "n%d_m%d_q%d_dy%d" % (N, M, Q, Dy), res


def row_kernel(reps, warmup=2, rows=32768, M=2048, D=16):
    rng = np.random.default_rng(2)
    W, X, Z = rng.standard_normal((rows, M)), rng.standard_normal((rows, D)), rng.standard_normal((M, D))
    Y, V = rng.standard_normal((rows, 1)), rng.standard_normal((M, 1))
    _, each = _lib.psi_lin_rows_probe(W, X, Z, np.full(D, 0.7), c0=-1.0, Y=Y, V=V, rowscale=np.full(rows, 2.0), beta=1.0, gscale=2.0,
                                      fused=True, time_reps=warmup + reps)
    ms = float(np.median(each[warmup:]))
    nbytes = 8.0 * (rows * M + 2 * rows * D + rows * 2)
    peaks = _lib.dbg_peaks(0)
    gbs = nbytes / (ms * 1e-3) / 1e9
    return dict(rows=rows, M=M, D=D, ms=ms, ms_min_max=[float(each[warmup:].min()), float(each[warmup:].max())], reps=reps,
                warmup=warmup, bytes=nbytes, gb_per_s=gbs, hbm_copy_gbs=float(peaks["hbm_copy_gbs"]),
                fraction_of_copy=gbs / float(peaks["hbm_copy_gbs"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    _lib.require_device(0)
    os.makedirs(a.out, exist_ok=True)
    rk = row_kernel(a.reps)
    for name, res in (linear_shape(a.reps, 2), rbf_shape(a.reps, 2)):
        if "D" in res["shape"]:
            res["row_kernel"] = rk
        with open(os.path.join(a.out, "psi_lin_time_%s.json" % name), "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
        print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
