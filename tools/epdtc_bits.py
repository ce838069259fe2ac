"""Bit-for-bit record of what the sparse inference families that existed before EPDTC compute, for comparing two builds of the
library (MI355GP_LIB chooses it).  EPDTC's final evaluation runs through the VarDTC evaluation of sparse.hip, which was split
into its C-ABI wrapper and a body that takes the precisions and Kmm's jitter as they are; this holds VarDTC, VarDTC with
uncertain inputs, SVGP, the row-sharded mode, FITC / PEP and the exact path's EP (whose probit helper moved into a header)
to the parent's bytes.

    python tools/epdtc_bits.py --out FILE.npz     store the raw fp64 outputs of
        everything tools/sparse_bits.py stores  (VarDTC over tests/sparse_ld.py's cases with its fetches and predictions, the
                                                 uncertain-input fits, SVGP over tests/svgp_np.py's cases, two loopback ranks)
        pep/NAME      every fixture of tests/golden/pep through mi355gp_pep_inference, the four fetch matrices a PEP result
                      has, a dL_dKnm block and the prediction
        ep/NAME       one recompute and one sweep of the exact path's EP at two fixtures of tests/golden/ep
    python tools/epdtc_bits.py --compare A B      name every array whose bytes differ; exit status 1 if any does

The dumps are device results (device libm included): compare two of the same machine, keep none as a fixture.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]


def dump(path):
    import ep_np as EP
    import mlp_np as MP
    import pep_np as P
    import sparse_bits
    from gpy_amd import _lib as L

    sparse_bits.dump(path)
    out = dict(np.load(path))

    def put(name, value):
        out[name] = np.ascontiguousarray(np.asarray(value, dtype=np.float64))

    ctx = L.SparseContext(0)
    for name in P.FIXTURES:
        fx = P.load_fixture(name)
        ctx.set_data(fx["X"], fx["Y"])
        info, r = ctx.pep(fx["specs"], fx["Z"], float(fx["noise"]), float(fx["alpha"]), P.JITTER)
        assert info == 0, (name, info)
        for q, v in r.items():
            if isinstance(v, (float, np.floating, np.ndarray)):
                put("pep/%s/%s" % (name, q), v)
        for which in range(4):
            put("pep/%s/fetch%d" % (name, which), ctx.fetch(which))
        put("pep/%s/dL_dKnm_block" % name, ctx.fetch_dL_dKnm(5, 64))
        mu, var = ctx.predict(fx["specs"], fx["Xs"])
        put("pep/%s/mu" % name, mu)
        put("pep/%s/var" % name, var)
    ctx.close()

    ex = L.Context(0)
    for name in EP.CASES[:2]:
        g = EP.load(name)
        ex.set_data(g["X"], g["Y"])
        ex.laplace_begin(MP.cabi_specs(g["specs"]))
        n = g["X"].shape[0]
        info, mu, sd, _ = ex.ep_recompute(np.zeros(n), np.zeros(n), 0.0, 1e-7)
        assert info == 0
        r = ex.ep_sweep(g["orders"][0], EP.ysign(g["Y"]), np.zeros(n), np.zeros(n), g["eta"], g["delta"])
        put("ep/%s/mu0" % name, mu)
        for q in ("tau", "v", "cav_tau", "cav_v", "log_Z_hat", "mu", "Sigma_diag"):
            put("ep/%s/%s" % (name, q), r[q])
    ex.close()
    np.savez(path, **out)
    print("epdtc_bits: %d arrays, %d doubles -> %s (library %s)" % (len(out), sum(a.size for a in out.values()), path, L.LIB_PATH))


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
