"""Device time of one fused exact-GP evaluation with Cosine, Sinc and ExpQuadCosine next to RBF and RatQuad in the same run: the
context's own `stage_ms` (HIP events on the launching stream) -- K build (MI355GP_T_KBUILD), gradient pass (MI355GP_T_GRAD) and
the total -- at N = 8192 with D = 1 and D = 8 (isotropic; the oscillating kinds act on column 0 alone, where they are positive
definite, and are summed with a White part at every D so that the factorisation never fails).  Medians of 7 after 2 warm-ups (with the minimum and maximum of each, for A/B margins).
A record, no gate: the new kernels are not tuned.

    python tools/osc_time.py [--reps 7] [--out profiles]      (needs the GPU; writes profiles/osc_time_n8192.json)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gpy_amd import _lib  # noqa: E402

N = 8192
DIMS = (1, 8)


def parts(kind, D):
    """[the kind, White]: RBF / RatQuad over all D columns, the oscillating kinds over column 0"""
    cols = np.arange(D)
    ls = 0.3 * np.sqrt(D)
    theta = {"rbf": [1.0, ls], "ratquad": [1.0, ls, 1.7], "cosine": [1.0, 0.1], "sinc": [1.0, 0.3], "expquadcosine": [1.0, 2.0, 0.1]}[kind]
    dims = cols if kind in ("rbf", "ratquad") else cols[:1]
    return [(kind, 0, np.array(theta), dims, 0), ("white", 0, np.array([0.05]), cols, 0)]


def run(reps, warmup=2):
    res = dict(N=N, reps=reps, warmup=warmup, kinds={})
    ctx = _lib.Context(0)
    for D in DIMS:
        rng = np.random.default_rng(D)
        X = rng.uniform(-1.0, 1.0, (N, D))
        Y = np.sin(2 * np.pi * X[:, :1] / 0.35) + 0.1 * rng.standard_normal((N, 1))
        ctx.set_data(X, Y)
        for kind in ("rbf", "ratquad", "cosine", "sinc", "expquadcosine"):
            ms = []
            for it in range(warmup + reps):
                info, r = ctx.exact_inference_sum(parts(kind, D), 0.05, want_stage_ms=True)
                assert info == 0, (kind, D, info)
                if it >= warmup:
                    ms.append(r["stage_ms"])
            res["kinds"]["%s_d%d" % (kind, D)] = dict(
                kbuild_ms=float(np.median([m["kbuild"] for m in ms])), grad_ms=float(np.median([m["grad"] for m in ms])),
                kbuild_ms_min_max=[float(min(m["kbuild"] for m in ms)), float(max(m["kbuild"] for m in ms))],
                grad_ms_min_max=[float(min(m["grad"] for m in ms)), float(max(m["grad"] for m in ms))],
                total_ms=float(np.median([m["total"] for m in ms])),
                total_ms_min_max=[float(min(m["total"] for m in ms)), float(max(m["total"] for m in ms))], log_marginal=float(r["lml"]))
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    _lib.require_device(0)
    os.makedirs(a.out, exist_ok=True)
    res = run(a.reps)
    with open(os.path.join(a.out, "osc_time_n%d.json" % N), "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
