"""Times the RBF psi-statistics and the uncertain-input sparse fit on the device:
    python tools/psi_time.py [--N 8192 --M 256 --Q 8 --reps 3 --host-rows 64]
`fit_*_ms` are HIP-event times on the launching stream of one `mi355gp_vardtc_inference_uncertain` call (its `stage_ms`):
pass 1 = Kmm's factorisation + psi1, psi1^T V and psi2 over all row chunks; mxm = the M x M phase; pass 2 = the psi1 and
psi2 gradient kernels with their reductions + the Kmm gradients; total = the whole evaluation on the device.
`*_call_ms` are wall times of whole stateless C-ABI calls (validation, allocation, upload, kernels, download).
`pyloop_*_ms_scaled` is the per-row Python loop of tests/psi_np.py (float64) timed on `--host-rows` rows and scaled to N: a
baseline for orientation, not an optimised host implementation.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=8192)
    ap.add_argument("--M", type=int, default=256)
    ap.add_argument("--Q", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-rows", type=int, default=64)
    a = ap.parse_args()
    import psi_np as P
    from gpy_amd import _lib
    p = P.problem(a.N, a.M, a.Q, 1)
    args = (p["var"], p["ls"], True, p["Z"], p["mu"], p["S"])

    def best(f):
        f()
        ts = []
        for _ in range(a.reps):
            t = time.perf_counter()
            f()
            ts.append(time.perf_counter() - t)
        return min(ts) * 1e3
    out = {"N": a.N, "M": a.M, "Q": a.Q,
           "psi2_call_ms": best(lambda: _lib.rbf_psi(*args, want_psi1=False)),
           "psi1_call_ms": best(lambda: _lib.rbf_psi(*args, want_psi2=False)),
           "grad_call_ms": best(lambda: _lib.rbf_psi_grad(*args, p["dL_dpsi0"], p["dL_dpsi1"], p["dL_dpsi2"]))}
    f = P.fit_problem(a.N, a.M, a.Q, 1, 1, True, [0.1])
    specs = [("rbf", True, np.concatenate([[f["var"]], f["ls"] * np.sqrt(a.Q)]), None, 0), ("white", False, np.array([0.1]), None, 0)]
    ctx = _lib.SparseContext(0)
    ctx.set_data(f["mu"], f["Y"])
    ctx.set_input_variance(f["S"])
    stages = []
    for _ in range(a.reps + 1):
        rc, r = ctx.vardtc_uncertain(specs, f["Z"], f["noise"], want_stage_ms=True)
        assert rc == 0
        stages.append(r["stage_ms"])
    for k in ("pass1", "mxm", "pass2", "total"):
        out["fit_%s_ms" % k] = min(s[k] for s in stages[1:])
    h = min(a.host_rows, a.N)
    t = time.perf_counter()
    P.psi_stats(p["var"], p["ls"], p["Z"], p["mu"][:h], p["S"][:h])
    out["pyloop_psi_ms_scaled"] = (time.perf_counter() - t) * 1e3 * a.N / h
    t = time.perf_counter()
    P.psi_grads(p["var"], p["ls"], True, p["Z"], p["mu"][:h], p["S"][:h], p["dL_dpsi0"][:h], p["dL_dpsi1"][:h], p["dL_dpsi2"])
    out["pyloop_grad_ms_scaled"] = (time.perf_counter() - t) * 1e3 * a.N / h
    print(json.dumps(out))


if __name__ == "__main__":
    main()
