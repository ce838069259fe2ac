"""Bit-for-bit record of what the exact-GP context computes, for comparing two builds of the library (MI355GP_LIB chooses it).

    python tools/exact_bits.py --out FILE.npz   store the raw fp64 outputs of
        seq/ID/callK     six (lookahead: eight) consecutive exact_inference calls on one context at N = 300 -- with graphs on:
                         plain, capture, replay ... -- for ID in: plain; stage_ms4 (call 4 asks for the stage times: it runs on
                         launches, the graph stays); graph0 (option "graph" = 0); lookahead (option toggled between calls: the
                         graph is dropped and captured again)
        shape/ID         N in {100, 128, 129, 700} x Dy in {1, 3}, RBF iso (D = 3) and Matern52 ARD with D = 40 (two gradient
                         groups), scalar noise and an N-vector of noise
        expr/ID          RBF + White + Bias; RBF x Matern32; RatQuad; Coregionalize x RBF; Linear + RBF
        studentt         the Student-t process, nu = 5, N = 129
        given_K          inference_given_K, N = 129
        npd              the not-positive-definite case of tests/test_gpu_linalg.py (jitter = -1e-3): its info code, then the
                         evaluation that follows it on the same context
        calib/callK      the nine calls at N = 2304 in which a context settles on a schedule (not the schedule: it is timed)
        fetch/ID         K, L, LINV, KINV, DLDK after the Gaussian, the product and the Student-t evaluation
        predict/...      at M in {1, 128, 130}: predict_sum with the diagonal variance and full_cov (RBF; Linear + RBF, whose
                         diagonal depends on the point), predictive_gradients (RBF, Linear + RBF, StdPeriodic, MLP; Dy = 2),
                         covariance_between_points
        dense/N          potrf and pdinv_full at N in {100, 129, 700}: L, Linv, Ainv, logdet
      -- per evaluation: info, lml, logdet, dnoise, alpha, dtheta, diag_dL_dK where the entry point returns it
    python tools/exact_bits.py --compare A B    name every array whose bytes differ; exit status 1 if any does

Stage times and the calibrated schedule are not stored.  The dumps are device results (device libm included): compare two of the
same machine, keep none as a fixture.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

FETCH_LINV = 100


def dump(path):
    from gpy_amd import _lib as L
    from oracle import gp_oracle as O

    out = {}

    def put(name, value):
        out[name] = np.ascontiguousarray(np.asarray(value, dtype=np.float64))

    def record(tag, info, r, expect=0):
        assert info == expect, (tag, info)
        put(tag + "/info", [info])
        for k in ("lml", "logdet", "datafit", "dnoise", "trKinv", "beta", "scale", "alpha", "dtheta", "diag_dL_dK"):
            if r.get(k) is not None:
                put(tag + "/" + k, r[k])

    def fetch_all(tag, c, with_K=True):
        names = [("L", L.FETCH_L), ("LINV", FETCH_LINV), ("KINV", L.FETCH_KINV), ("DLDK", L.FETCH_DLDK)]
        for name, which in names + ([("K", L.FETCH_K)] if with_K else []):
            put(tag + "/" + name, c.fetch(which))

    def iso(kind, D):
        var, ls, noise = O.default_theta(D, False)
        return (kind, 0, L.theta_vec(var, ls, False, D), None), noise

    c = L.Context(0)
    try:
        # ---- evaluation sequences on one context
        X, Y = O.synthetic(300, 3, seed=300)
        (kind, _, th, _), noise = iso("rbf", 3)
        for tag, ncalls in (("plain", 6), ("stage_ms4", 6), ("graph0", 6), ("lookahead", 8)):
            c.set_data(X, Y)
            c.set_option("graph", 0 if tag == "graph0" else -1)
            la = 1
            for i in range(ncalls):
                want = (1, 1, 1, 0, 0, 1, 1, 1)[i] if tag == "lookahead" else la
                if want != la:
                    c.set_option("lookahead", want)
                    la = want
                info, r = c.exact_inference(kind, False, th, noise, want_diag=True, want_stage_ms=(tag == "stage_ms4" and i == 3))
                record("seq/%s/call%d" % (tag, i + 1), info, r)
        c.set_option("graph", -1)
        c.set_option("lookahead", -1)

        # ---- shapes
        for N in (100, 128, 129, 700):
            for Dy in (1, 3):
                for kind, ARD, D in (("rbf", False, 3), ("matern52", True, 40)):
                    X, Y = O.synthetic(N, D, seed=N + Dy, Dy=Dy)
                    var, ls, noise = O.default_theta(D, ARD)
                    c.set_data(X, Y)
                    for nname, nz in (("scalar", noise), ("vector", 0.05 + 0.1 * np.random.default_rng(N).random(N))):
                        info, r = c.exact_inference(kind, ARD, L.theta_vec(var, ls, ARD, D), nz, want_diag=True)
                        record("shape/%s_N%d_Dy%d_%s" % (kind, N, Dy, nname), info, r)

        # ---- expressions (N = 129, D = 4; the Coregionalize case reads the output index from a fifth column)
        N, D = 129, 4
        X, Y = O.synthetic(N, D, seed=129, Dy=2)
        rng = np.random.default_rng(7)
        Xc = np.hstack([X, rng.integers(0, 3, (N, 1)).astype(np.float64)])
        W = rng.uniform(-1.0, 1.0, (3, 2))
        B = W @ W.T + np.diag(rng.uniform(0.3, 0.9, 3))
        rbf = ("rbf", 0, np.array([1.3, 1.4]), None)
        lin = ("linear", 1, np.array([0.3, 0.2, 0.4, 0.25]), None)
        exprs = {
            "rbf_white_bias": (X, [rbf, ("white", 0, np.array([0.05]), None), ("bias", 0, np.array([0.3]), None)]),
            "rbf_x_matern32": (X, [("rbf", 1, np.array([1.1, 1.4, 0.8]), np.array([0, 1]), 1),
                                   ("matern32", 0, np.array([0.9, 1.2]), np.array([2, 3]), 1)]),
            "ratquad": (X, [("ratquad", 0, np.array([0.9, 1.5, 1.7]), None)]),
            "coreg_x_rbf": (Xc, [("coregionalize", 3, 0.5 * (B + B.T).ravel(), np.array([4]), 1),
                                 ("rbf", 0, np.array([1.3, 1.4]), np.array([0, 1, 2, 3]), 1)]),
            "linear_rbf": (X, [lin, rbf]),
        }
        for tag, (Xe, specs) in exprs.items():
            c.set_data(Xe, Y)
            info, r = c.exact_inference_sum(specs, 0.1, want_diag=True)
            record("expr/" + tag, info, r)
            if tag == "rbf_x_matern32":
                fetch_all("fetch/product", c)

        # ---- Student-t process, inference_given_K, fetch after the Gaussian evaluation
        c.set_data(X, Y)
        info, r = c.exact_studentt_sum([rbf], 5.0)
        record("studentt", info, r)
        fetch_all("fetch/studentt", c)
        info, r = c.exact_inference_sum([rbf], 0.1, want_diag=True)
        record("gaussian", info, r)
        fetch_all("fetch/gaussian", c)

        # ---- prediction from that factorisation
        Xs_all, _ = O.synthetic(130, D, seed=17)
        per = ("stdperiodic", 0, np.array([1.1, 2.5, 1.3]), None)
        mlp = ("mlp", 0, np.array([1.2, 0.3, 0.4]), None)
        for name, specs in (("rbf", [rbf]), ("linear_rbf", [lin, rbf]), ("stdperiodic", [per]), ("mlp", [mlp])):
            info, r = c.exact_inference_sum(specs, 0.1)
            assert info == 0, (name, info)
            for M in (1, 128, 130):
                Xs = Xs_all[:M]
                tag = "predict/%s_M%d" % (name, M)
                dmu, dvar = c.predictive_gradients(specs, Xs)
                put(tag + "/dmu", dmu)
                put(tag + "/dvar", dvar)
                if name in ("rbf", "linear_rbf"):
                    mu, var = c.predict_sum(specs, Xs)
                    _, cov = c.predict_sum(specs, Xs, full_cov=True)
                    put(tag + "/mu", mu)
                    put(tag + "/var", var)
                    put(tag + "/cov", cov)
                    put(tag + "/between", c.covariance_between_points(specs, Xs, Xs_all[:max(1, M - 2)]))

        info, r = c.inference_given_K(O.kern_K("rbf", X, None, 1.3, np.array([1.4]), False), 0.1, want_diag=True)
        record("given_K", info, r)
        fetch_all("fetch/given_K", c, with_K=False)

        # ---- not positive definite, then the evaluation that follows
        X, Y = O.synthetic(1500, 3, seed=5)
        (kind, _, th, _), noise = iso("rbf", 3)
        c.set_data(np.vstack([X[:700], X[:700], X[:100]]), Y)
        info, _ = c.exact_inference(kind, False, th, 0.0, jitter=-1e-3)
        assert info > 0, info
        put("npd/info", [info])
        info, r = c.exact_inference(kind, False, th, noise, want_diag=True)
        record("npd/next", info, r)

        # ---- the calibration sequence
        X, Y = O.synthetic(2304, 4, seed=11)
        (kind, _, th, _), noise = iso("rbf", 4)
        c.set_data(X, Y)
        for i in range(9):
            info, r = c.exact_inference(kind, False, th, noise, want_diag=True)
            record("calib/call%d" % (i + 1), info, r)
    finally:
        c.close()

    # ---- dense routines
    for N in (100, 129, 700):
        X, _ = O.synthetic(N, 3, seed=N)
        A = O.kern_K("matern52", X, None, 1.3, np.array([0.8, 1.1, 1.9]), True) + 0.5 * np.eye(N)
        Lf, info, _ = L.potrf(A)
        assert info == 0, (N, info)
        put("dense/N%d/potrf_L" % N, np.tril(Lf))
        Ai, Lf, Li, ld, info = L.pdinv_full(A)
        assert info == 0, (N, info)
        for k, v in (("L", Lf), ("Linv", Li), ("Ainv", Ai), ("logdet", [ld])):
            put("dense/N%d/%s" % (N, k), v)

    np.savez(path, **out)
    print("exact_bits: %d arrays, %d doubles -> %s (library %s)" % (len(out), sum(a.size for a in out.values()), path, L.LIB_PATH))


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
    print("exact_bits compare: %d arrays, %d doubles, %d differing" % (len(names), sum(A[n].size for n in A.files), len(bad)))
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
