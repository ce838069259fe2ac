"""Times VarDTC with a Linear part on the MI355X next to its stationary neighbours, in one run: `mi355gp_vardtc_inference_sum`
by HIP events on the launching stream (the entry point's own `stage_ms`: pass 1, M x M, pass 2, total) for

    rbf            one RBF ARD part (the fused single-part passes)
    rbf+matern32   two stationary ARD parts: the fair two-part comparison (pass 1 unfused, two gradient passes)
    rbf+linear     RBF ARD + Linear ARD: pass 1 unfused, k_grad_cols_mfma for the RBF part and k_grad_cols_lin for the Linear one

at N = 200000, M = 2048, D = 16, Dy = 1 (the sparse configuration of BASELINE.json) and N = 8192, M = 256.  Medians of 7 after 2
warm-ups.  A record, no gate.

What the second part's gradient pass costs is the difference of pass 2 against `rbf` (pass 2 of a two-part sum = the T product,
both parts' gradient passes and their reductions); the two differences are reported side by side.  The per-point-diagonal
kernels (kern_diag.hip) run inside the `rbf+linear` total; on their own they are timed through `mi355gp_sparse_kdiag` with
weights, by the host's clock around the call -- which therefore includes the upload of the N weights, the copy of kd back and
the synchronisation (the entry point has no event pair of its own).

    python tools/sparse_lin_time.py [--reps 7] [--out profiles]     (needs the GPU; writes profiles/sparse_lin_time_<shape>.json)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gpy_amd import _lib  # noqa: E402

SHAPES = [dict(name="n200000_m2048_d16", N=200000, M=2048, D=16), dict(name="n8192_m256_d16", N=8192, M=256, D=16)]
STAGES = ("pass1", "mxm", "pass2", "total")


def inputs(sh, seed=0):
    rng = np.random.default_rng(seed)
    N, M, D = sh["N"], sh["M"], sh["D"]
    X = rng.uniform(-0.5, 0.5, (N, D))
    Y = np.sin(X[:, :3].sum(1))[:, None] + X[:, :1] + 0.1 * rng.standard_normal((N, 1))
    Z = X[rng.permutation(N)[:M]].copy()
    allq = np.arange(D, dtype=np.int32)
    rbf = ("rbf", 1, np.concatenate([[1.0], np.full(D, 1.5)]), allq, 0)
    w = 1.0 + 0.5 * np.arange(D)
    kernels = {"rbf": [rbf],
               "rbf+matern32": [rbf, ("matern32", 1, np.concatenate([[0.5], np.full(D, 2.0)]), allq, 0)],
               "rbf+linear": [rbf, ("linear", 1, w / w.sum(), allq, 0)]}
    return X, Y, Z, kernels


def run(sh, reps, warmup=2):
    X, Y, Z, kernels = inputs(sh)
    ctx = _lib.SparseContext(0)
    ctx.set_linear(True)
    ctx.set_data(X, Y)
    res = dict(shape=dict((k, sh[k]) for k in ("N", "M", "D")), Dy=1, reps=reps, warmup=warmup)
    for name, specs in kernels.items():
        ts = []
        for it in range(warmup + reps):
            info, r = ctx.vardtc_sum(specs, Z, 0.01, extra_jitter=1e-5, want_stage_ms=True)   # one fixed rung: Z is drawn from X
            assert info == 0, "Kmm or B not positive definite at the timing shape (%s, info %d)" % (name, info)
            if it >= warmup:
                ts.append(r["stage_ms"])
        for k in STAGES:
            res["%s_%s_ms" % (name, k)] = float(np.median([s[k] for s in ts]))
        res["%s_total_ms_min_max" % name] = [min(s["total"] for s in ts), max(s["total"] for s in ts)]
        res["%s_log_marginal" % name] = float(r["lml"])
    res["second_part_pass2_ms"] = {"matern32": res["rbf+matern32_pass2_ms"] - res["rbf_pass2_ms"],
                                   "linear": res["rbf+linear_pass2_ms"] - res["rbf_pass2_ms"]}
    w = np.cos(np.arange(sh["N"]))
    tk = []
    for it in range(warmup + reps):
        t0 = time.perf_counter()
        ctx.kdiag(kernels["rbf+linear"], w=w)
        tk.append((time.perf_counter() - t0) * 1e3)
    res["kdiag_entry_host_ms"] = float(np.median(tk[warmup:]))
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
        with open(os.path.join(a.out, "sparse_lin_time_%s.json" % sh["name"]), "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
        print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
