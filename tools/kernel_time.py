"""Device time of fused exact-GP evaluations (`exact_inference_sum`, noise 0.1) of named kernel expressions at N = 16384, D = 32,
with the stage times of the library (kbuild, potrf, trtri, lauum, solve, grad, total: hipEvent timings, MI355GP_T_*).
Per expression the median over the timed evaluations after the warm-up ones (and their minimum and maximum); one JSON line.
MI355GP_LIB chooses the library; an expression that the library refuses (a kind it predates) reports null.  The kernels'
own times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/kernel_time.py ...`.

    python tools/kernel_time.py [NAME ...] [--n 16384] [--d 32] [--reps 5] [--warmup 3] [--shuffle] [--list]

Names: every kind alone with ARD (the default, `kinds`): rbf matern52 matern32 exponential white bias ratquad stdperiodic
coregionalize linear mlp poly; the sums rbf+linear+bias and rbf+mlp+bias; icm = Matern52 ARD x Coregionalize (P = 4, rows
sorted by output as build_XY stacks them, or in random order with --shuffle; per-output noise).  Groups: `kinds`, `linear`
(rbf linear rbf+linear+bias), `mlp` (rbf mlp poly rbf+mlp+bias), `coreg` (icm matern52).
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpy_amd import _lib as L  # noqa: E402

P = 4
KINDS = ["rbf", "matern52", "matern32", "exponential", "white", "bias", "ratquad", "stdperiodic", "coregionalize", "linear", "mlp",
         "poly"]
GROUPS = {"kinds": KINDS, "linear": ["rbf", "linear", "rbf+linear+bias"], "mlp": ["rbf", "mlp", "poly", "rbf+mlp+bias"],
          "coreg": ["icm", "matern52"]}


def expressions(D):
    """{name: [part, ...]}; a part is (kind, ard, theta, active_dims, product flag).  Column D of the inputs holds the output index."""
    dims = np.arange(D)
    ls = np.linspace(0.5, 2.0, D) * np.sqrt(D / 8.0)
    W = np.array([[0.9], [-0.5], [0.7], [0.3]])
    B = W @ W.T + np.diag([0.5, 0.4, 0.6, 0.3])
    part = {"white": ("white", 0, np.array([0.7]), dims, 0), "bias": ("bias", 0, np.array([0.5]), dims, 0),
            "ratquad": ("ratquad", 1, np.concatenate([[1.0], ls, [1.7]]), dims, 0),
            "stdperiodic": ("stdperiodic", 3, np.concatenate([[1.0], np.linspace(1.5, 3.0, D), ls]), dims, 0),
            "coregionalize": ("coregionalize", P, B.ravel(), np.array([D]), 0),
            "linear": ("linear", 1, np.linspace(0.5, 1.5, D) / D, dims, 0),
            "mlp": ("mlp", 1, np.concatenate([[1.0], np.linspace(0.5, 1.5, D) / D, [0.5]]), dims, 0),
            "poly": ("poly", 0, np.array([1.0, 1.0 / D, 1.0, 2.0]), dims, 0)}
    for k in ("rbf", "matern52", "matern32", "exponential"):
        part[k] = (k, 1, np.concatenate([[1.0], ls]), dims, 0)
    ex = {k: [v] for k, v in part.items()}
    ex["rbf+linear+bias"] = [part["rbf"], part["linear"], part["bias"]]
    ex["rbf+mlp+bias"] = [part["rbf"], part["mlp"], part["bias"]]
    ex["icm"] = [("matern52", 1, np.concatenate([[1.0], np.linspace(2.0, 6.0, D)]), dims, 1), part["coregionalize"][:4] + (1,)]
    return ex


def stage_stats(ctx, specs, noise, reps, warmup):
    runs = []
    for r in range(warmup + reps):
        info, res = ctx.exact_inference_sum(specs, noise, want_stage_ms=True)
        assert info == 0, info
        if r >= warmup:
            runs.append(res["stage_ms"])
    return {f: {k: float(fn([m[k] for m in runs])) for k in runs[0]} for f, fn in (("median", np.median), ("min", min), ("max", max))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("names", nargs="*", default=["kinds"])
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shuffle", action="store_true", help="rows in random output order (many output pairs per tile)")
    ap.add_argument("--list", action="store_true")
    a = ap.parse_args()
    ex = expressions(a.d)
    if a.list:
        print("\n".join(sorted(ex) + ["group " + g + ": " + " ".join(v) for g, v in sorted(GROUPS.items())]))
        return
    names = [n for arg in a.names for n in GROUPS.get(arg, [arg])]
    names = list(dict.fromkeys(names))
    unknown = [n for n in names if n not in ex]
    if unknown:
        ap.error("unknown expression(s) %s; --list shows the names" % unknown)
    n, D = a.n, a.d
    rng = np.random.default_rng(n)
    idx = np.sort(rng.integers(0, P, n))
    if a.shuffle:
        idx = rng.permutation(idx)
    X = rng.standard_normal((n, D))
    y = X @ (rng.standard_normal(D) / np.sqrt(D)) + np.sin(X[:, 0]) * (1.0 + 0.2 * idx) + 0.1 * rng.standard_normal(n)
    XI = np.hstack([X, idx[:, None].astype(float)])
    noises = np.array([0.1, 0.05, 0.2, 0.1])
    out = {"N": n, "D": D, "reps": a.reps, "warmup": a.warmup, "shuffled": bool(a.shuffle), "lib": L.LIB_PATH, "stage_ms": {},
           "stage_ms_min": {}, "stage_ms_max": {}}
    # the expressions on the plain inputs first, then those that read the output index in column D: one context at a time
    for indexed in (False, True):
        todo = [nm for nm in names if any(p[0] == "coregionalize" for p in ex[nm]) == indexed]
        if not todo:
            continue
        c = L.Context(0)
        try:
            c.set_data(XI if indexed else X, y[:, None])
            for nm in todo:
                try:
                    st = stage_stats(c, ex[nm], noises[idx] if nm == "icm" else 0.1, a.reps, a.warmup)
                except L.MI355GPError:                     # MI355GP_LIB points at a library that predates the kind
                    st = {"median": None, "min": None, "max": None}
                out["stage_ms"][nm], out["stage_ms_min"][nm], out["stage_ms_max"][nm] = st["median"], st["min"], st["max"]
        finally:
            c.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
