"""Times the gradient phase of an exact-GP evaluation with latent inputs on the MI355X, in one run and one process, by the HIP
events of the entries' own `stage_ms["grad"]` (the gradient phase alone).  Medians of 7 after 2 warm-ups.  A record, no gate.

Per case (N in 4096, 8192; (Q, Dy) in (2, 12), (8, 64); RBF ARD + Bias):
    latent_grad_ms   `mi355gp_latent_inference_sum`: one pass over Ky^-1 and alpha, dL/dX and the theta sums (csrc/latent.hip)
    exact_grad_ms    `mi355gp_exact_inference_sum` on the same data: the theta sums alone, alpha alpha^T by a scalar loop over Dy
    fetch_gradx_ms   what a caller could do before: fetch dL_dK (N x N over PCIe) and call the stateless `mi355gp_gradients_X`,
                     wall clock (transfers and host work are the point of that figure)
The solve stage (alpha with Dy right-hand sides, untouched) is recorded next to them.

    python tools/latent_time.py [--reps 7] [--out profiles]     (needs the GPU; writes profiles/latent_time_<shape>.json)
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


def one_shape(N, Q, Dy, reps, warmup):
    rng = np.random.default_rng(N + Q)
    X = rng.standard_normal((N, Q))
    Y = np.tanh(X @ rng.standard_normal((Q, Dy))) + 0.1 * rng.standard_normal((N, Dy))
    theta = np.r_[1.0, np.full(Q, 1.5)]
    specs = [("rbf", 1, theta, None, 0), ("bias", 0, np.array([np.exp(-2.0)]), None, 0)]
    ctx = _lib.Context(0)
    ctx.set_data(X, Y)
    res = dict(shape=dict(N=N, Q=Q, Dy=Dy), reps=reps, warmup=warmup, kernel="rbf_ard+bias")
    for name, call in (("latent", lambda: ctx.latent_inference_sum(specs, 0.1, want_stage_ms=True)),
                       ("exact", lambda: ctx.exact_inference_sum(specs, 0.1, want_stage_ms=True))):
        ts = []
        for it in range(warmup + reps):
            info, r = call()
            assert info == 0
            if it >= warmup:
                ts.append(r["stage_ms"])
        for k in ("grad", "solve", "total"):
            res["%s_%s_ms" % (name, k)] = float(np.median([s[k] for s in ts]))
        res["%s_grad_ms_min_max" % name] = [min(s["grad"] for s in ts), max(s["grad"] for s in ts)]
    ts = []
    for it in range(warmup + reps):
        t0 = time.perf_counter()
        G = ctx.fetch(_lib.FETCH_DLDK)
        _lib.gradients_X("rbf", 1, theta, G, X)
        ts.append((time.perf_counter() - t0) * 1e3)
    res["fetch_gradx_ms"] = float(np.median(ts[warmup:]))
    res["latent_over_exact_grad"] = res["latent_grad_ms"] / res["exact_grad_ms"]
    ctx.close()
    return "n%d_q%d_dy%d" % (N, Q, Dy), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--sizes", type=int, nargs="*", default=[4096, 8192])
    a = ap.parse_args()
    for N in a.sizes:
        for Q, Dy in ((2, 12), (8, 64)):
            name, res = one_shape(N, Q, Dy, a.reps, a.warmup)
            with open(os.path.join(a.out, "latent_time_%s.json" % name), "w") as f:
                json.dump(res, f, indent=1, sort_keys=True)
            print(name, json.dumps({k: v for k, v in res.items() if k.endswith("_ms") or k == "latent_over_exact_grad"}), flush=True)


if __name__ == "__main__":
    main()
