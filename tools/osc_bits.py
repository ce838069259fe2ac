"""Bit-for-bit record of what the twelve covariance kinds that existed before Cosine / Sinc / ExpQuadCosine compute, for comparing
two builds of the library (MI355GP_LIB chooses it): every variant of tests/kern_ld.py (all twelve kinds, iso and ARD) at two
shapes of its sweep, 65 / 63 / 33 / 1 (tile + 1, second ARD group) and 129 / 130 / 5 / 4 (128-row padding + 1, active_dims a
strict subset), through

    the stateless entry points   kern_K symmetric and cross, update_gradients_full square and rectangular, gradients_X (not Poly)
    the fused calls              exact_inference_sum of the kind next to a White (lml, dnoise, alpha, dtheta, diag dL_dK), the
                                 fetched K and predict_sum with the diagonal and the full covariance

    python tools/osc_bits.py --out FILE.npz      store the raw fp64 outputs
    python tools/osc_bits.py --compare A B       name every array whose bytes differ; exit status 1 if any does

The dumps are device results (device libm included): compare two of the same machine, keep none as a fixture.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]
SHAPES = [(65, 63, 33, 1), (129, 130, 5, 4)]


def dump(path):
    import kern_ld as KL
    from gpy_amd import _lib as L

    out = {}

    def put(name, value):
        out[name] = np.ascontiguousarray(np.asarray(value, dtype=np.float64))

    ctx = L.Context(0)
    for variant in KL.VARIANTS:
        for shape in SHAPES:
            c = KL.make_case(variant, shape)
            tag = KL.case_id(variant, shape)
            kind, ard, th, dims, _ = KL.cabi_specs([c["spec"]])[0]
            Xa, Xb = np.ascontiguousarray(c["X"][:, dims]), np.ascontiguousarray(c["X2"][:, dims])
            if kind not in ("white", "bias"):                           # (static kinds: host arithmetic, parts of a sum only)
                put(tag + "/K", L.kern_K(kind, ard, th, Xa))
                put(tag + "/Kx", L.kern_K(kind, ard, th, Xa, Xb))
                put(tag + "/dtheta", L.update_gradients_full(kind, ard, th, c["G"], Xa, None))
                put(tag + "/dtheta_x", L.update_gradients_full(kind, ard, th, c["G2"], Xa, Xb))
            if kind not in ("poly", "coregionalize", "white", "bias"):
                put(tag + "/gradX", L.gradients_X(kind, ard, th, c["G"], Xa, None))
                put(tag + "/gradX_x", L.gradients_X(kind, ard, th, c["G2"], Xa, Xb))
            label, specs, X, Xs = KL.fused_exprs(c)[1]                  # next to a White
            dev = KL.cabi_specs(specs)
            ctx.set_data(X, c["Y"])
            info, r = ctx.exact_inference_sum(dev, c["noise"], want_diag=True)
            assert info == 0, (tag, info)
            for k in ("lml", "dnoise", "alpha", "dtheta", "diag_dL_dK"):
                put(tag + "/fused/" + k, r[k])
            put(tag + "/fused/K", ctx.fetch(L.FETCH_K))
            mu, var = ctx.predict_sum(dev, Xs)
            put(tag + "/fused/mu", mu)
            put(tag + "/fused/var", var)
            put(tag + "/fused/cov", ctx.predict_sum(dev, Xs, full_cov=True)[1])
    ctx.close()
    np.savez(path, **out)
    print("osc_bits: %d arrays, %d doubles -> %s (library %s)" % (len(out), sum(a.size for a in out.values()), path, L.LIB_PATH))


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
