"""Device time of one EP recompute and one EP sweep (HIP events around the enqueued work, returned by the C-ABI calls) next to
the NumPy restatement's sweep on the host.  One untimed warm-up call of each, then the median of `--reps` calls.

    python tools/ep_time.py --sizes 4096 8192 --host-size 4096
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
import ep_np as EP  # noqa: E402
import laplace_np as LP  # noqa: E402
import mlp_np as P  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 8192])
    ap.add_argument("--host-size", type=int, default=4096, help="size of the NumPy sweep (0: skip)")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    specs = [("rbf", 1, np.array([1.4, 1.1, 0.8, 1.5]), np.arange(3), 0), ("bias", 0, np.array([0.2]), np.arange(3), 0)]
    out = {}
    for N in a.sizes:
        X, Y = LP.two_class(N, 3, 170 + N)
        tau = 0.05 + 0.3 / (1.0 + X[:, 0] ** 2)
        v = EP.ysign(Y) * tau * (0.5 + 0.2 * np.cos(X[:, 1]))
        order = np.random.default_rng(N).permutation(N)
        ctx = L.Context()
        ctx.set_data(X, Y)
        ctx.laplace_begin(P.cabi_specs(specs))
        rec, rec_diag, swp = [], [], []
        for rep in range(a.reps + 1):
            info, _, _, _, ms = ctx.ep_recompute(tau, v, want_sigma=False, want_ms=True)
            assert info == 0
            rec_diag.append(ms)
            info, _, _, _, ms = ctx.ep_recompute(tau, v, add_diag=1e-7, want_sigma=True, want_ms=True)
            assert info == 0
            rec.append(ms)
            swp.append(ctx.ep_sweep(order, EP.ysign(Y), tau, v, want_ms=True)["ms"])
        out[str(N)] = {"recompute_ms": float(np.median(rec[1:])), "recompute_diag_only_ms": float(np.median(rec_diag[1:])),
                       "sweep_ms": float(np.median(swp[1:])), "sweep_all_ms": swp[1:]}
        if N == a.host_size:
            K = LP.expr(specs, X)[0]
            mu0, _, _, Sigma = EP.recompute(K, tau, v, 1e-7, True)
            t0 = time.perf_counter()
            EP.sweep(Sigma, mu0, order, EP.ysign(Y), 1.0, 1.0, tau, v)
            out[str(N)]["numpy_sweep_host_ms"] = (time.perf_counter() - t0) * 1e3
        ctx.close()
        print(json.dumps({str(N): out[str(N)]}), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
