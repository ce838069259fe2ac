"""Times one Bayesian GPLVM evaluation and one prediction at uncertain points on the MI355X.  A record, no gate.

Shape: N = 8192, M = 256, Q = 8, Dy = 12, an ARD RBF kernel.  One model evaluation is an upload of the inputs followed by
`mi355gp_vardtc_inference_uncertain`; it is timed with the upload a GPLVM step needs, `mi355gp_sparse_set_inputs` (means and
variances, Y stays resident), and with the one it needed before, `mi355gp_sparse_set_data` + `mi355gp_sparse_set_input_variance`
(which takes Y along and frees / reallocates every buffer).  The fit's time is the entry point's own `stage_ms` (HIP events on the
launching stream); the uploads are synchronous host calls and are timed by the wall clock, as is the whole evaluation.
`mi355gp_sparse_predict_uncertain` at Mn = 8192 is timed by HIP events on the launching stream around its chunks (uploads of the
chunk, psi1, the thin product, k_psi2n_contract, the copies back: `mi355gp_sparse_get_predict_ms`) and by the wall clock.
Medians of `--reps` (7) after 2 warm-ups.  Neither path has been profiled or tuned.

    python tools/bgplvm_time.py [--reps 7] [--out profiles]        (needs the GPU; writes profiles/bgplvm_time_<shape>.json)
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

SHAPE = dict(name="n8192_m256_q8_dy12", N=8192, M=256, Q=8, Dy=12, Mn=8192)


def median(v):
    return float(np.median(v))


def run(sh, reps, warmup=2):
    r = np.random.default_rng(0)
    N, M, Q, Dy, Mn = (sh[k] for k in ("N", "M", "Q", "Dy", "Mn"))
    mu, S = r.uniform(-3, 3, (N, Q)), r.uniform(0.05, 1.0, (N, Q))
    Y = np.sin(mu[:, :2].sum(1, keepdims=True) + 0.7 * np.arange(Dy)[None, :]) + 0.1 * r.standard_normal((N, Dy))
    Z = mu[r.permutation(N)[:M]].copy()
    specs = [("rbf", True, np.concatenate([[1.3], r.uniform(0.8, 1.8, Q) * np.sqrt(Q)]), None, 0)]
    mu_new, S_new = r.uniform(-3, 3, (Mn, Q)), r.uniform(0.05, 1.0, (Mn, Q))
    ctx = _lib.SparseContext(0)
    ctx.set_data(mu, Y)
    ctx.set_input_variance(S)
    res = dict(shape=dict((k, sh[k]) for k in ("N", "M", "Q", "Dy", "Mn")), reps=reps, warmup=warmup)
    for mode in ("set_inputs", "set_data"):
        up, fit, wall = [], [], []
        for it in range(warmup + reps):
            mu_it = mu + 1e-3 * (it + 1)                               # a step changes every mean and variance
            S_it = S * (1.0 + 1e-3 * (it + 1))
            t0 = time.perf_counter()
            if mode == "set_inputs":
                ctx.set_inputs(mu_it, S_it)
            else:
                ctx.set_data(mu_it, Y)
                ctx.set_input_variance(S_it)
            t1 = time.perf_counter()
            info, out = ctx.vardtc_uncertain(specs, Z, 0.05, want_stage_ms=True)
            t2 = time.perf_counter()
            assert info == 0, "Kmm not positive definite at the timing shape (info %d)" % info
            if it >= warmup:
                up.append(1e3 * (t1 - t0))
                fit.append(out["stage_ms"]["total"])
                wall.append(1e3 * (t2 - t0))
        res["evaluation_with_" + mode] = dict(upload_wall_ms=median(up), fit_device_ms=median(fit), evaluation_wall_ms=median(wall),
                                              evaluation_wall_ms_min_max=[min(wall), max(wall)])
    dev, wall = [], []
    for it in range(warmup + reps):
        t0 = time.perf_counter()
        ctx.predict_uncertain(specs, mu_new, S_new)
        t1 = time.perf_counter()
        if it >= warmup:
            dev.append(ctx.predict_ms())
            wall.append(1e3 * (t1 - t0))
    res["predict_uncertain"] = dict(stream_ms=median(dev), stream_ms_min_max=[min(dev), max(dev)], wall_ms=median(wall),
                                    psi2n_values=float(Mn) * M * (M + 1) / 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    _lib.require_device(0)
    os.makedirs(a.out, exist_ok=True)
    res = run(SHAPE, a.reps)
    with open(os.path.join(a.out, "bgplvm_time_%s.json" % SHAPE["name"]), "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
