"""Times the group-batched psi2 kernels (csrc/psi_missing.hip) next to the route they replace on the MI355X.  A record with ONE
condition: at G = PSI_GB groups each batched kernel must beat PSI_GB launches of the single-mask kernel (`faster` in the output).

Shape: N = 8192, M = 256, Q = 8, an ARD RBF kernel, Dy = 12 output columns with 20 % of the entries missing, arranged as G = 1, 4,
PSI_GB and 12 row masks.  For pass 1's psi2 (`mi355gp_rbf_psi2_groups`) and for the psi2 gradient (`mi355gp_rbf_psi_grad_groups`)
the calls report the stream time of their psi2 kernels alone (HIP events around the launches on the launching stream, summed
over the 2048-row chunks): `multi` is the batched kernel, ceil(G / PSI_GB) launches a chunk; `loop` is k_psi2 / k_psi2_grad once
per group with weights w_g (the diagnostic entries of include/mi355gp_debug_sparse_missing.h).  `evaluation`: the pass split of one
whole missing-data evaluation at G = 1, 4 and 12 next to the complete-data uncertain evaluation (`evaluation_split`).  Medians of
`--reps` (7) after 2 warm-ups.  Neither kernel has been tuned.

    python tools/missing_time.py [--reps 7] [--out profiles]        (needs the GPU; writes profiles/missing_time_<shape>.json)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gpy_amd import _lib  # noqa: E402

SHAPE = dict(name="n8192_m256_q8_dy12", N=8192, M=256, Q=8, Dy=12, missing=0.2)


def masks(N, G, missing, r):
    """N x G 0/1: every group drops `missing` of the rows, its own draw"""
    return (r.uniform(size=(N, G)) >= missing).astype(np.float64)


def evaluation_split(sh, reps, warmup, r, mu, S, Z, var, ls):
    """the pass split (`stage_ms`: pass 1, the M x M phase, pass 2, total; HIP events on the launching stream) of one
    `mi355gp_vardtc_inference_missing` with the Dy columns arranged as G = 1, 4 and 12 groups, next to the complete-data
    `mi355gp_vardtc_inference_uncertain` on the same inputs in the same run"""
    N, Dy = sh["N"], sh["Dy"]
    Yfull = np.sin(mu[:, :2].sum(1, keepdims=True) + 0.7 * np.arange(Dy)[None, :]) + 0.1 * r.standard_normal((N, Dy))
    specs = [("rbf", True, np.concatenate([[var], ls]), None, 0)]
    med = lambda runs: dict((k, float(np.median([x[k] for x in runs]))) for k in runs[0])
    rows = []
    ctx = _lib.SparseContext(0)
    ctx.set_data(mu, Yfull)
    ctx.set_input_variance(S)
    runs = [ctx.vardtc_uncertain(specs, Z, 0.05, want_stage_ms=True)[1]["stage_ms"] for _ in range(warmup + reps)][warmup:]
    rows.append(dict(entry="uncertain (complete data)", G=0, **med(runs)))
    print(json.dumps(rows[-1]))
    for G in (1, 4, 12):
        W = masks(N, G, sh["missing"], r)
        Y = np.where(W[:, np.arange(Dy) % G] > 0, Yfull, np.nan)
        gof, Wg, Y0 = _lib.output_groups(Y)
        ctx.set_data(mu, Y0)
        ctx.set_input_variance(S)
        ctx.set_output_groups(gof, Wg)
        runs = [ctx.vardtc_missing(specs, Z, 0.05, want_stage_ms=True)[1]["stage_ms"] for _ in range(warmup + reps)][warmup:]
        rows.append(dict(entry="missing", G=int(Wg.shape[1]), **med(runs)))
        print(json.dumps(rows[-1]))
    return rows


def run(sh, reps, warmup=2):
    r = np.random.default_rng(0)
    N, M, Q = sh["N"], sh["M"], sh["Q"]
    mu, S = r.uniform(-3, 3, (N, Q)), r.uniform(0.05, 1.0, (N, Q))
    Z = mu[r.permutation(N)[:M]].copy()
    var, ls = 1.3, r.uniform(0.8, 1.8, Q) * np.sqrt(Q)
    GB = _lib.psi_groups_batch()
    out = dict(shape=sh, reps=reps, warmup=warmup, groups_per_launch=GB, rows=[])
    for G in (1, 4, GB, 12):
        W, dL = masks(N, G, sh["missing"], r), r.standard_normal((G, M, M))
        row = dict(G=G)
        for loop in (False, True):
            t2, tg = [], []
            for i in range(warmup + reps):
                _, a = _lib.rbf_psi2_groups(var, ls, True, Z, mu, S, W, loop=loop, want_ms=True)
                b = _lib.rbf_psi_grad_groups(var, ls, True, Z, mu, S, W, dL, loop=loop, want_ms=True)[-1]
                if i >= warmup:
                    t2.append(a), tg.append(b)
            k = "loop" if loop else "multi"
            row["psi2_%s_ms" % k], row["psi2_grad_%s_ms" % k] = float(np.median(t2)), float(np.median(tg))
        out["rows"].append(row)
        print(json.dumps(row))
    out["evaluation"] = evaluation_split(sh, reps, warmup, r, mu, S, Z, var, ls)
    at = next(x for x in out["rows"] if x["G"] == GB)
    out["faster"] = dict(psi2=at["psi2_multi_ms"] < at["psi2_loop_ms"], psi2_grad=at["psi2_grad_multi_ms"] < at["psi2_grad_loop_ms"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    _lib.require_device(0)
    res = run(SHAPE, a.reps)
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "missing_time_%s.json" % SHAPE["name"])
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print("faster:", res["faster"], "->", path)


if __name__ == "__main__":
    main()
