"""Bit-for-bit record of what the sparse inference families that existed before FITC / PEP compute, for comparing two builds of
the library (MI355GP_LIB chooses it): one seeded evaluation each of VarDTC, SVGP and VarDTC with uncertain inputs at N = 4097,
M = 129, D = 3 (two output columns; an RBF ARD part and a White part), on one context in that order.

    python tools/pep_bits.py --out FILE.npz      store the raw fp64 outputs: vardtc_sum (dL_dm included), the six
                                                 mi355gp_sparse_fetch matrices, a dL_dKnm block, sparse_predict; svgp forward,
                                                 backward, Woodbury quantities, predict; vardtc_uncertain with dmu and dS
    python tools/pep_bits.py --compare A B       name every array whose bytes differ; exit status 1 if any does

The dumps are device results: compare two of the same machine, keep none as a fixture.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]
N, M, D, DY = 4097, 129, 3, 2


def dump(path):
    from gpy_amd import _lib as L
    rng = np.random.default_rng(4097)
    X = rng.uniform(0.0, 1.0, (N, D))
    Y = np.sin(2.0 * np.pi * X @ rng.uniform(1.0, 3.0, (D, DY))) + 0.2 * rng.standard_normal((N, DY))
    Z = X[rng.permutation(N)[:M]] + 0.01 * rng.standard_normal((M, D))
    S = rng.uniform(0.001, 0.01, (N, D))
    Xs = rng.uniform(0.0, 1.0, (65, D))
    specs = [("rbf", 1, np.array([1.3, 0.3, 0.4, 0.5]), None, 0), ("white", 0, np.array([0.05]), None, 0)]
    q_mean = 0.5 * rng.standard_normal((M, DY))
    q_L = np.stack([np.eye(M) + 0.1 * np.tril(rng.standard_normal((M, M))) / np.sqrt(M) for _ in range(DY)])
    dFm, dFv = rng.standard_normal((N, DY)), rng.standard_normal((N, DY)) - 0.5
    out = {}

    def put(name, value):
        if isinstance(value, dict):
            for k in sorted(value):
                put(name + "/" + k, value[k])
        elif isinstance(value, (float, np.floating, np.ndarray)):
            out[name] = np.ascontiguousarray(np.asarray(value, dtype=np.float64))

    ctx = L.SparseContext(0)
    ctx.set_data(X, Y)
    info, r = ctx.vardtc_sum(specs, Z, 0.04, want_dL_dm=True)
    assert info == 0
    put("vardtc/result", r)
    for which in range(6):
        put("vardtc/fetch%d" % which, ctx.fetch(which))
    put("vardtc/dL_dKnm_block", ctx.fetch_dL_dKnm(2000, 300))
    mu, var = ctx.predict(specs, Xs)
    put("vardtc/predict", {"mu": mu, "var": var, "cov": ctx.predict(specs, Xs, full_cov=True)[1]})
    info, fw = ctx.svgp_forward(specs, Z, q_mean, q_L, extra_jitter=1e-6)
    assert info == 0
    put("svgp/forward", fw)
    put("svgp/backward", ctx.svgp_backward(dFm, dFv))
    wv, wi = ctx.svgp_woodbury()
    mu, var = ctx.svgp_predict(specs, Xs)
    put("svgp/predict", {"wv": wv, "winv": wi, "mu": mu, "var": var, "cov": ctx.svgp_predict(specs, Xs, full_cov=True)[1]})
    ctx.set_input_variance(S)
    info, r = ctx.vardtc_uncertain(specs, Z, 0.04)
    assert info == 0
    put("uncertain/result", r)
    put("uncertain/fetch0", ctx.fetch(0))
    ctx.close()
    np.savez(path, **out)
    print("pep_bits: %d arrays, %d doubles -> %s (library %s)" % (len(out), sum(a.size for a in out.values()), path, L.LIB_PATH))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.compare:
        from sparse_bits import compare
        return compare(*a.compare)
    if not a.out:
        ap.error("--out FILE or --compare A B")
    dump(a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
