"""Times the spike-and-slab psi-statistics on the MI355X, in one run.  Medians of 7 after 2 warm-ups.  A record, no gate.

    n8192_m256_q8_dy12   RBF ARD + White: one `mi355gp_vardtc_inference_ss` evaluation with its pass split (HIP events on the
                         launching stream, the entry point's own `stage_ms`: pass 1, M x M, pass 2, total) next to
                         `mi355gp_vardtc_inference_uncertain` on the same context with gamma cleared (Gaussian inputs N(mu, diag S)).
                         By instruction count the psi passes cost about Q times the Gaussian ones in exponentials (one per
                         factor where the Gaussian kernels have one per element; the gradient kernels evaluate the group's
                         factors a second time for their shares).
    stateless            `mi355gp_ssrbf_psi` (psi2 alone) and `mi355gp_ssrbf_psi_grad` (dL_dpsi2 alone) at the same shape: WALL time
                         of the calls, uploads and downloads included (they have no event hooks), next to the Gaussian pair.

    python tools/psi_ss_time.py [--reps 7] [--out profiles]     (needs the GPU; writes profiles/psi_ss_time_<shape>.json)
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

STAGES = ("pass1", "mxm", "pass2", "total")


def _wall(fn, reps, warmup):
    ts = []
    for it in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        if it >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return dict(wall_ms=float(np.median(ts)), wall_ms_min_max=[min(ts), max(ts)])


def run(reps, warmup, N=8192, M=256, Q=8, Dy=12):
    rng = np.random.default_rng(1)
    mu, S, gam = rng.uniform(-2, 2, (N, Q)), rng.uniform(0.05, 0.5, (N, Q)), rng.uniform(0.05, 0.95, (N, Q))
    Y = np.sin(mu.sum(1, keepdims=True) / np.sqrt(Q) + np.arange(Dy)[None, :]) + 0.3 + 0.1 * rng.standard_normal((N, Dy))
    Z = mu[rng.permutation(N)[:M]].copy()
    ls = np.full(Q, 2.5)
    specs = [("rbf", 1, np.concatenate([[1.3], ls]), None, 0), ("white", 0, np.array([0.05]), None, 0)]
    ctx = _lib.SparseContext(0)
    ctx.set_data(mu, Y)
    ctx.set_input_variance(S)
    res = dict(shape=dict(N=N, M=M, Q=Q), Dy=Dy, reps=reps, warmup=warmup, kernel="rbf_ard+white")
    for name, call in (("gaussian", ctx.vardtc_uncertain), ("spike_and_slab", ctx.vardtc_ss)):
        if name == "spike_and_slab":
            ctx.set_binary_prob(gam)
        ts = []
        for it in range(warmup + reps):
            info, r = call(specs, Z, 0.05, extra_jitter=1e-5, want_stage_ms=True)      # one fixed rung: Z is drawn from mu
            assert info == 0, "Kmm or B not positive definite at the timing shape (%s, info %d)" % (name, info)
            if it >= warmup:
                ts.append(r["stage_ms"])
        for k in STAGES:
            res["%s_%s_ms" % (name, k)] = float(np.median([s[k] for s in ts]))
        res["%s_total_ms_min_max" % name] = [min(s["total"] for s in ts), max(s["total"] for s in ts)]
        res["%s_log_marginal" % name] = float(r["lml"])
    for k in ("pass1", "pass2", "total"):
        res["spike_and_slab_over_gaussian_%s" % k] = res["spike_and_slab_%s_ms" % k] / res["gaussian_%s_ms" % k]
    ctx.close()
    A = rng.standard_normal((M, M))
    dL2 = A + A.T
    a = (1.3, ls, True, Z, mu, S)
    res["stateless"] = {
        "ss_psi2": _wall(lambda: _lib.ssrbf_psi(*a, gam, want_psi1=False), reps, warmup),
        "ss_psi2_grad": _wall(lambda: _lib.ssrbf_psi_grad(*a, gam, dL_dpsi2=dL2), reps, warmup),
        "gaussian_psi2": _wall(lambda: _lib.rbf_psi(*a, want_psi1=False), reps, warmup),
        "gaussian_psi2_grad": _wall(lambda: _lib.rbf_psi_grad(*a, dL_dpsi2=dL2), reps, warmup),
        "exponentials_psi2": float(N) * (M * (M + 1) // 2) * Q,
    }
    return "n%d_m%d_q%d_dy%d" % (N, M, Q, Dy), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    _lib.require_device(0)
    os.makedirs(a.out, exist_ok=True)
    name, res = run(a.reps, 2)
    with open(os.path.join(a.out, "psi_ss_time_%s.json" % name), "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
