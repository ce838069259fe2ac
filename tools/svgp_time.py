"""Times the SVGP device session on the MI355X: `mi355gp_svgp_forward` and `mi355gp_svgp_backward` separately, by HIP events on
the launching stream (the entry points' own `stage_ms`, first event after the uploads are enqueued, last one before the results
are copied back), and in the same run `mi355gp_vardtc_inference_sum` at the first shape for comparison.  A record, no gate.

Shapes: N = 200000, M = 2048, D = 16, L = 1 (the sparse configuration of BASELINE.json) and a minibatch of N = 1024, M = 512.
By arithmetic SVGP does about (4 + 4 L) N M^2 flops an evaluation against VarDTC's 3 N M^2.  The likelihood's quadrature runs on
the host between the two calls and is not in these times; the wall-clock time of a whole evaluation (uploads, quadrature and
copies included) is reported next to them.

    python tools/svgp_time.py [--reps 7] [--out profiles]        (needs the GPU; writes profiles/svgp_time_<shape>.json)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gpy_amd  # noqa: E402
from gpy_amd import _lib  # noqa: E402

SHAPES = [dict(name="n200000_m2048_d16_l1", N=200000, M=2048, D=16, L=1, vardtc=True),
          dict(name="n1024_m512_d16_l1", N=1024, M=512, D=16, L=1, vardtc=False)]


def inputs(sh, seed=0):
    rng = np.random.default_rng(seed)
    N, M, D, L = sh["N"], sh["M"], sh["D"], sh["L"]
    X = rng.uniform(0.0, 1.0, (N, D))
    Y = np.sin(X[:, :3].sum(1))[:, None] + 0.1 * rng.standard_normal((N, L))
    Z = X[rng.permutation(N)[:M]].copy()
    specs = [("rbf", 1, np.concatenate([[1.0], np.full(D, 1.5)]), None, 0)]
    q_mean = 0.1 * rng.standard_normal((M, L))
    q_L = np.stack([np.eye(M) + 0.1 * np.tril(rng.standard_normal((M, M))) / np.sqrt(M) for _ in range(L)])
    return X, Y, Z, specs, q_mean, q_L


def median(v):
    return float(np.median(v))


def run(sh, reps, warmup=2):
    X, Y, Z, specs, q_mean, q_L = inputs(sh)
    lik = gpy_amd.Gaussian(variance=0.01)
    ctx = _lib.SparseContext(0)
    ctx.set_data(X, Y)
    jit = 1e-6                                                    # (no 1e-8 on Kmm in SVGP: a fixed ladder rung, the same every repetition)
    fwd, bwd, wall = [], [], []
    for it in range(warmup + reps):
        t0 = time.perf_counter()
        info, fw = ctx.svgp_forward(specs, Z, q_mean, q_L, extra_jitter=jit, want_stage_ms=True)
        assert info == 0, "Kmm not positive definite at the timing shape (info %d)" % info
        _, dFm, dFv, _ = lik.variational_expectations(Y, fw["mu"], fw["v"])
        bw = ctx.svgp_backward(dFm, dFv, want_stage_ms=True)
        t1 = time.perf_counter()
        if it >= warmup:
            fwd.append(fw["stage_ms"])
            bwd.append(bw["stage_ms"])
            wall.append(1e3 * (t1 - t0))
    N, M, L = sh["N"], sh["M"], sh["L"]
    flops = (4.0 + 4.0 * L) * N * M * M
    res = dict(shape=dict((k, sh[k]) for k in ("N", "M", "D", "L")), reps=reps, warmup=warmup,
               forward_ms=median([f["total"] for f in fwd]), forward_mxm_ms=median([f["mxm"] for f in fwd]),
               forward_rows_ms=median([f["rows"] for f in fwd]), backward_ms=median([b["total"] for b in bwd]),
               backward_rows_ms=median([b["rows"] for b in bwd]), backward_mxm_ms=median([b["mxm"] for b in bwd]),
               forward_ms_min_max=[min(f["total"] for f in fwd), max(f["total"] for f in fwd)],
               backward_ms_min_max=[min(b["total"] for b in bwd), max(b["total"] for b in bwd)],
               wall_ms_whole_evaluation=median(wall), algorithmic_flops=flops)
    dev = res["forward_ms"] + res["backward_ms"]
    res["device_ms"] = dev
    res["algorithmic_tflops_over_device_time"] = flops / (dev * 1e-3) / 1e12
    if sh["vardtc"]:
        vt = []
        for it in range(warmup + reps):
            info, r = ctx.vardtc_sum(specs, Z, 0.01, want_stage_ms=True)
            assert info == 0
            if it >= warmup:
                vt.append(r["stage_ms"]["total"])
        res["vardtc_ms"] = median(vt)
        res["vardtc_ms_min_max"] = [min(vt), max(vt)]
        res["vardtc_algorithmic_flops"] = 3.0 * N * M * M
        res["svgp_over_vardtc_time"] = dev / res["vardtc_ms"]
        res["svgp_over_vardtc_flops"] = flops / res["vardtc_algorithmic_flops"]
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
        path = os.path.join(a.out, "svgp_time_%s.json" % sh["name"])
        with open(path, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
        print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
