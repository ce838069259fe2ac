"""Bit-for-bit record of what the covariance kernels compute, for comparing two builds of the library (MI355GP_LIB chooses it).

    python tools/kern_bits.py --out FILE.npz     walk tests/kern_ld.py's VARIANTS x SHAPES (every kind, iso / ARD, N / M / D at
                                                 the tile, chunk and padding edges) on make_case inputs and store the raw fp64
                                                 arrays of: K(X), K(X, X2), Kdiag, update_gradients_full rectangular and square,
                                                 gradients_X where the kind has it; per fused_exprs expression (alone, plus
                                                 White, times RBF) exact_inference_sum (lml, alpha, dtheta, dnoise, fetched K)
                                                 and predict_sum with and without full_cov; and the six (D, Dy) sparse
                                                 dispatch cases of tests/test_gpu_kernel_shapes.py (vardtc_sum, dL_dKnm).
    python tools/kern_bits.py --compare A B      name every array whose bytes differ; exit status 1 if any does

The dumps are device results (device libm included): compare two of the same machine, keep none as a fixture.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def dump(path):
    import kern_ld as KL
    from gpy_amd import _lib as L
    from oracle import gp_oracle as O
    from oracle import sparse_oracle as S
    import test_gpu_kernel_shapes as T

    out = {}

    def put(name, value):
        if isinstance(value, dict):
            for k in sorted(value):
                put(name + "/" + k, value[k])
        elif value is not None:
            out[name] = np.ascontiguousarray(np.asarray(value, dtype=np.float64))

    ctx = L.Context(0)
    for variant in KL.VARIANTS:
        for shape in KL.SHAPES:
            c = KL.make_case(variant, shape)
            tag = KL.case_id(variant, shape)
            spec, X, X2, G, G2 = c["spec"], c["X"], c["X2"], c["G"], c["G2"]
            k = T.kernel(spec)
            put(tag + "/K", k.K(X))
            put(tag + "/K_cross", k.K(X, X2))
            put(tag + "/Kdiag", k.Kdiag(X))
            k.update_gradients_full(G2, X, X2)
            put(tag + "/dtheta_rect", np.atleast_1d(k.gradient).copy())
            k.update_gradients_full(G, X)
            put(tag + "/dtheta_square", np.atleast_1d(k.gradient).copy())
            if spec[0] != "poly":
                put(tag + "/gradX_rect", k.gradients_X(G2, X, X2))
                put(tag + "/gradX_square", k.gradients_X(G, X))
            for label, specs, Xe, Xs in KL.fused_exprs(c):
                dev = KL.cabi_specs(specs)
                ctx.set_data(Xe, c["Y"])
                info, r = ctx.exact_inference_sum(dev, c["noise"])
                assert info == 0, (tag, label, info)
                put(tag + "/" + label + "/exact", {q: r[q] for q in ("lml", "alpha", "dtheta", "dnoise")})
                put(tag + "/" + label + "/K_fetched", ctx.fetch(L.FETCH_K))
                mu, var = ctx.predict_sum(dev, Xs)
                _, cov = ctx.predict_sum(dev, Xs, full_cov=True)
                put(tag + "/" + label + "/predict", {"mu": mu, "var": var, "cov": cov})
    ctx.close()

    sctx = L.SparseContext(0)
    for kern in sorted(T.SPARSE_KERNELS):
        for D, Dy in [(16, 4), (16, 5), (17, 1), (32, 4), (32, 5), (33, 1)]:
            N, M = 193, 65
            X, Y = O.synthetic(N, D, seed=D * 10 + Dy, Dy=Dy)
            Z = S.synthetic_Z(X, M, D)
            parts = T.SPARSE_KERNELS[kern](D, np.random.default_rng(D))
            specs = [(p[0], p[1], L.theta_vec(p[2], p[3], p[1], D) if p[3] is not None else np.array([p[2]]),
                      np.asarray(p[4], np.int32), 0) for p in parts]
            sctx.set_data(X, Y)
            info, r = sctx.vardtc_sum(specs, Z, 0.07)
            assert info == 0, (kern, D, Dy, info)
            tag = "sparse_%s_d%d_dy%d" % (kern, D, Dy)
            put(tag + "/vardtc", {q: v for q, v in r.items() if isinstance(v, (float, np.floating, np.ndarray))})
            put(tag + "/dL_dKnm", sctx.fetch_dL_dKnm(0, N))
    sctx.close()
    np.savez(path, **out)
    print("kern_bits: %d arrays, %d doubles -> %s (library %s)" % (len(out), sum(a.size for a in out.values()), path, L.LIB_PATH))


def compare(pa, pb):
    A, B = np.load(pa), np.load(pb)
    names = sorted(set(A.files) | set(B.files))
    bad = []
    for n in names:
        if n not in A.files or n not in B.files:
            bad.append(n + " (in one dump only)")
        elif A[n].shape != B[n].shape or A[n].tobytes() != B[n].tobytes():
            a, b = A[n], B[n]
            d = float(np.nanmax(np.abs(a - b))) if a.shape == b.shape and a.size else float("nan")
            bad.append("%s (max |a - b| = %.3e)" % (n, d))
    for n in bad:
        print("DIFFERS: " + n)
    print("kern_bits compare: %d arrays, %d doubles, %d differing" % (len(names), sum(A[n].size for n in A.files), len(bad)))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.compare:
        return compare(*a.compare)
    if not a.out:
        ap.error("--out FILE or --compare A B")
    dump(a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
