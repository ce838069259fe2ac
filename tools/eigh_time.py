"""Time of the device eigensolver (`mi355gp_eigh`, csrc/eigh.hip) on an RBF covariance matrix at n = 512, 1024, 2048, 4096, next to
`numpy.linalg.eigh` on this box's CPUs and `torch.linalg.eigh` on the same GPU, all on the same matrix:

    python tools/eigh_time.py [--sizes 512,1024,2048,4096] [--out profiles/eigh_time_<sizes>.json]

Device time is by HIP events around the solver's own launches (the C-ABI's `ms`), median of 7 calls after 2 warm-ups, the sweep
count recorded; torch by `torch.cuda.Event`, the same 2 + 7; NumPy by `time.perf_counter`, median of 3.  A record, no bar."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gpy_amd import _lib  # noqa: E402


def rbf_matrix(n, seed=0):
    X = np.random.default_rng(seed).uniform(0.0, 10.0, (n, 2))
    d2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    return np.exp(-0.5 * d2 / 1.5 ** 2) + 1e-6 * np.eye(n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,1024,2048,4096")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    rows = []
    for n in sizes:
        A = rbf_matrix(n)
        dev = []
        for _ in range(9):
            w, V, info, sweeps, ms = _lib.eigh(A)
            dev.append(ms)
        res = float(np.abs(A @ V - V * w).max() / np.linalg.norm(A, 2))
        cpu = []
        for _ in range(3):
            t0 = time.perf_counter()
            np.linalg.eigh(A)
            cpu.append(1e3 * (time.perf_counter() - t0))
        row = {"n": n, "device_ms": float(np.median(dev[2:])), "sweeps": sweeps, "info": info, "residual_f64": res,
               "numpy_cpu_ms": float(np.median(cpu)), "cpus": os.cpu_count()}
        try:
            import torch
            At = torch.from_numpy(A).cuda()
            tt = []
            for _ in range(9):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                torch.linalg.eigh(At)
                e1.record()
                torch.cuda.synchronize()
                tt.append(e0.elapsed_time(e1))
            row["torch_gpu_ms"] = float(np.median(tt[2:]))
        except Exception as e:                                  # unmeasured, and the record says why
            row["torch_gpu_ms"] = None
            row["torch_unmeasured_because"] = repr(e)[:200]
        print(json.dumps(row), flush=True)
        rows.append(row)
    out = a.out or os.path.join(ROOT, "profiles", "eigh_time_%s.json" % "_".join(str(n) for n in sizes))
    with open(out, "w") as f:
        json.dump({"matrix": "RBF, 2-D uniform inputs on [0, 10]^2, lengthscale 1.5, + 1e-6 I",
                   "info": "0: converged; 1: the cap of %d sweeps was reached" % _lib.EIGH_MAX_SWEEPS, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
