"""Times EPDTC on the MI355X by HIP events on the launching stream: one `mi355gp_epdtc_recompute`, one `mi355gp_epdtc_sweep`
(each from a fresh recompute of the same sites) and the final `mi355gp_epdtc_inference`, and in the same run
`mi355gp_vardtc_inference_sum` at the same shape for comparison.  A record, no gate.

Shapes: N = 200000, M = 2048, D = 16 with one RBF ARD part (the sparse configuration of BASELINE.json) and a small one,
N = 8192, M = 256.  Medians of 7 after 2 warm-ups.  Algorithmic flops, counted from the shapes (2 a multiply-add):
    recompute   the row-weighted Gram (N M^2) and V = Kfu L^-T (2 N M^2)
    sweep       A0 = K_b P and P -= W1^T diag(c) W1 per block of 64 sites (2 N M^2 each: 4 N M^2)
    inference   VarDTC's (3 N M^2)
The sweep's tile GEMMs run on 128-row tiles, of which a block fills 64 rows, so the device does twice the sweep's count.
`sweep_floor_ms` is the same sweep with ONE inducing point: the site-block launches and the launch overhead of the blocks with
next to no GEMM work under them.  The site block is 64 (two 64 x 64 fp64 matrices in LDS); 128 would need 256 KiB of LDS and does
not exist, so there is no second block size to run against.

    python tools/epdtc_time.py [--reps 7] [--out profiles]     (needs the GPU; writes profiles/epdtc_time_<shape>.json)
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
BLOCK = 64


def inputs(sh, seed=0):
    rng = np.random.default_rng(seed)
    N, M, D = sh["N"], sh["M"], sh["D"]
    X = rng.uniform(0.0, 1.0, (N, D))
    sign = np.where(np.sin(X[:, :3].sum(1)) + 0.3 * rng.standard_normal(N) > 0.7, 1.0, -1.0)
    Z = X[rng.permutation(N)[:M]].copy()
    specs = [("rbf", 1, np.concatenate([[1.0], np.full(D, 1.5)]), None, 0)]
    return X, sign, Z, specs, rng.permutation(N)


def median(v):
    return float(np.median(v))


def sweeps(ctx, order, sign, tau, v, reps, warmup):
    out = []
    for it in range(warmup + reps):
        assert ctx.epdtc_recompute(tau, v)[0] == 0
        r = ctx.epdtc_sweep(order, sign, tau, v, first=True, want_ms=True)
        if it >= warmup:
            out.append(r["ms"])
    return out, r


def run(sh, reps, warmup=2):
    X, sign, Z, specs, order = inputs(sh)
    N, M = sh["N"], sh["M"]
    jitter = 1e-5                              # one fixed rung of the ladder (Z is drawn from X), the same every repetition
    ctx = _lib.SparseContext(0)
    ctx.set_data(X, sign[:, None])
    assert ctx.epdtc_begin(specs, Z, jitter)[0] == 0
    tau, v = np.full(N, 0.3), 0.2 * sign
    rt = []
    for it in range(warmup + reps):
        info, mu, sd, ms = ctx.epdtc_recompute(tau, v, want_ms=True)
        assert info == 0
        if it >= warmup:
            rt.append(ms)
    st, r = sweeps(ctx, order, sign, tau, v, reps, warmup)
    it_, vt = [], []
    for it in range(warmup + reps):
        info, d = ctx.epdtc_inference(specs, Z, r["tau"], r["v"], jitter, want_stage_ms=True)
        assert info == 0, "B not positive definite at the timing shape (info %d)" % info
        if it >= warmup:
            it_.append(d["stage_ms"]["total"])
    for it in range(warmup + reps):
        info, d = ctx.vardtc_sum(specs, Z, 0.01, extra_jitter=jitter, want_stage_ms=True)
        assert info == 0
        if it >= warmup:
            vt.append(d["stage_ms"]["total"])
    # the floor: the same sites and order over ONE inducing point
    assert ctx.epdtc_begin(specs, Z[:1], jitter)[0] == 0
    ft, _ = sweeps(ctx, order, sign, tau, v, reps, warmup)
    ctx.close()
    nm2 = float(N) * M * M
    res = dict(shape=dict((k, sh[k]) for k in ("N", "M", "D")), reps=reps, warmup=warmup, block=BLOCK, blocks=-(-N // BLOCK),
               recompute_ms=median(rt), sweep_ms=median(st), sweep_ms_min_max=[min(st), max(st)], sweep_floor_ms=median(ft),
               inference_ms=median(it_), vardtc_ms=median(vt), sweep_algorithmic_flops=4.0 * nm2, vardtc_algorithmic_flops=3.0 * nm2)
    res["sweep_over_vardtc_time"] = res["sweep_ms"] / res["vardtc_ms"]
    res["sweep_over_vardtc_flops"] = 4.0 / 3.0
    res["sweep_floor_share"] = res["sweep_floor_ms"] / res["sweep_ms"]
    res["sweep_us_per_site"] = 1e3 * res["sweep_ms"] / N
    res["inference_over_vardtc_time"] = res["inference_ms"] / res["vardtc_ms"]
    res["sweep_algorithmic_tflops_over_device_time"] = 4.0 * nm2 / (res["sweep_ms"] * 1e-3) / 1e12
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
        with open(os.path.join(a.out, "epdtc_time_%s.json" % sh["name"]), "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
        print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
