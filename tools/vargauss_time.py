"""Time of one VarGauss evaluation (mi355gp_vargauss_forward, mi355gp_vargauss_backward and _backward_exact) next to a Laplace finish + gradients on the
same context and data: wall clock around each synchronous C-ABI call (the N-vector uploads and read-backs included; they are
microseconds next to the N^3 work at these sizes).  Two warm-up rounds, then the median of `--reps` rounds.

    python tools/vargauss_time.py --sizes 4096 8192 --out profiles
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gpy_amd import _lib as L  # noqa: E402
import laplace_np as LP  # noqa: E402
import mlp_np as P  # noqa: E402


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 8192])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="directory for vargauss_time_n<N>.json")
    a = ap.parse_args()
    specs = [("rbf", 1, np.array([1.4, 1.1, 0.8, 1.5]), np.arange(3), 0), ("bias", 0, np.array([0.2]), np.arange(3), 0)]
    for N in a.sizes:
        rng = np.random.default_rng(N)
        X, Y = LP.two_class(N, 3, 170 + N)
        alpha, beta = 0.1 * rng.standard_normal(N), np.where(rng.random(N) < 0.3, -1.0, 1.0) * rng.uniform(0.3, 1.5, N)
        g, v = 0.5 * rng.standard_normal(N), -0.3 * np.abs(rng.standard_normal(N))
        W = beta ** 2
        ctx = L.Context()
        ctx.set_data(X, Y)
        ctx.laplace_begin(P.cabi_specs(specs))
        t = {"vargauss_forward_ms": [], "vargauss_backward_ms": [], "vargauss_backward_exact_ms": [], "laplace_finish_ms": [],
             "laplace_gradients_ms": []}
        for rep in range(a.warmup + a.reps):
            ms_f, r = timed(lambda: ctx.vargauss_forward(alpha, beta))
            assert r[0] == 0
            ms_b, _ = timed(lambda: ctx.vargauss_backward(g, v))
            assert ctx.vargauss_forward(alpha, beta)[0] == 0
            ms_e, _ = timed(lambda: ctx.vargauss_backward(g, v, exact=True))       # dF_dv <= 0 here: one Gram product
            ms_lf, r = timed(lambda: ctx.laplace_finish(W))
            assert r[0] == 0
            ms_lg, _ = timed(lambda: ctx.laplace_gradients(alpha, g))
            if rep >= a.warmup:
                for k, ms in zip(t, (ms_f, ms_b, ms_e, ms_lf, ms_lg)):
                    t[k].append(ms)
        ctx.close()
        out = {"N": N, "reps": a.reps, "warmup": a.warmup, "clock": "wall clock around the synchronous C-ABI call"}
        out.update((k, float(np.median(x))) for k, x in t.items())
        out["all"] = t
        print(json.dumps(out), flush=True)
        if a.out:
            with open(os.path.join(a.out, "vargauss_time_n%d.json" % N), "w") as f:
                json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
