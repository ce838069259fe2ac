"""Times one FITC / PEP evaluation on the MI355X: `mi355gp_pep_inference` by HIP events on the launching stream (the entry
point's own `stage_ms`: pass 1, M x M, pass 2, total; first event after Z is enqueued, last one before the results are copied
back), and in the same run `mi355gp_vardtc_inference_sum` at the same shape for comparison.  A record, no gate.

Shapes: N = 200000, M = 2048, D = 16, Dy = 1 with one RBF ARD part (the sparse configuration of BASELINE.json) and a small one,
N = 8192, M = 256.  Medians of 7 after 2 warm-ups.  The N M^2 products of the arrangement, counted here from the shapes
(2 flops a multiply-add; `chunks` = row chunks of the context, a single chunk keeps W for pass 2):
    pass 1   W = Kfu Xm^T (full tile GEMM: 2 N M^2), the split-K Gram of the lower tiles (N M^2)
    pass 2   W again when there are several chunks (2 N M^2), C1 = W (A^-1 Xm) and C2 = W Xm (2 N M^2 each), the signed weighted
             Gram C2^T diag(dL_dR) C2 as a full GEMM (2 N M^2)
against VarDTC's Gram (N M^2) and T = Kfu dL_dpsi2 (2 N M^2).

    python tools/pep_time.py [--reps 7] [--alpha 1.0] [--out profiles]     (needs the GPU; writes profiles/pep_time_<shape>.json)
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
CHUNK_MAX = 262144                      # rows per chunk of the sparse context (csrc/sparse.hip)


def inputs(sh, seed=0):
    rng = np.random.default_rng(seed)
    N, M, D = sh["N"], sh["M"], sh["D"]
    X = rng.uniform(0.0, 1.0, (N, D))
    Y = np.sin(X[:, :3].sum(1))[:, None] + 0.1 * rng.standard_normal((N, 1))
    Z = X[rng.permutation(N)[:M]].copy()
    specs = [("rbf", 1, np.concatenate([[1.0], np.full(D, 1.5)]), None, 0)]
    return X, Y, Z, specs


def flops(N, M):
    """algorithmic N M^2 flops of one PEP and one VarDTC evaluation"""
    nm2 = float(N) * M * M
    chunks = -(-N // CHUNK_MAX)
    pep = (2.0 + 1.0) * nm2 + ((2.0 if chunks > 1 else 0.0) + 2.0 + 2.0 + 2.0) * nm2
    return pep, 3.0 * nm2


def median(v):
    return float(np.median(v))


def run(sh, reps, alpha, warmup=2):
    X, Y, Z, specs = inputs(sh)
    ctx = _lib.SparseContext(0)
    ctx.set_data(X, Y)
    noise, jitter = 0.01, 1e-6 + 1e-5         # const_jitter and one fixed rung of the ladder (Z is drawn from X), the same every repetition
    pt, vt = [], []
    for it in range(warmup + reps):
        info, r = ctx.pep(specs, Z, noise, alpha, jitter, want_stage_ms=True)
        assert info == 0, "Kmm or A not positive definite at the timing shape (info %d)" % info
        if it >= warmup:
            pt.append(r["stage_ms"])
    lml = float(r["lml"])
    for it in range(warmup + reps):
        info, r = ctx.vardtc_sum(specs, Z, noise, extra_jitter=1e-5, want_stage_ms=True)
        assert info == 0
        if it >= warmup:
            vt.append(r["stage_ms"])
    ctx.close()
    fp, fv = flops(sh["N"], sh["M"])
    res = dict(shape=dict((k, sh[k]) for k in ("N", "M", "D")), Dy=1, alpha=alpha, reps=reps, warmup=warmup, log_marginal=lml,
               algorithmic_flops=fp, vardtc_algorithmic_flops=fv)
    for k in ("pass1", "mxm", "pass2", "total"):
        res["pep_%s_ms" % k] = median([s[k] for s in pt])
        res["vardtc_%s_ms" % k] = median([s[k] for s in vt])
    res["pep_total_ms_min_max"] = [min(s["total"] for s in pt), max(s["total"] for s in pt)]
    res["vardtc_total_ms_min_max"] = [min(s["total"] for s in vt), max(s["total"] for s in vt)]
    res["algorithmic_tflops_over_device_time"] = fp / (res["pep_total_ms"] * 1e-3) / 1e12
    res["pep_over_vardtc_time"] = res["pep_total_ms"] / res["vardtc_total_ms"]
    res["pep_over_vardtc_flops"] = fp / fv
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--alpha", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    _lib.require_device(0)
    os.makedirs(a.out, exist_ok=True)
    for sh in SHAPES:
        res = run(sh, a.reps, a.alpha)
        path = os.path.join(a.out, "pep_time_%s.json" % sh["name"])
        with open(path, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
        print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
