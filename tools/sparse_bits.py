"""Bit-for-bit record of what the three sparse inference families compute on one context (VarDTC, VarDTC with uncertain
inputs, SVGP), for comparing two builds of the library (MI355GP_LIB chooses it).

    python tools/sparse_bits.py --out FILE.npz   store the raw fp64 outputs of
        vardtc/NAME      every tests/sparse_ld.py PLAIN case and the first BLOCKED one through vardtc_sum (per-point noise
                         rows and dL_dm included), the six mi355gp_sparse_fetch matrices, one fetch_dL_dKnm block and
                         sparse_predict with and without full_cov
        uncertain/ID     a fit at each shape of tests/test_gpu_psi.py CASES (psi_np.fit_problem; a White part where the case
                         has weights) through vardtc_uncertain, dmu and dS included
        svgp/NAME        every tests/svgp_np.py PLAIN case and the first BLOCKED one through forward, backward (seeded
                         dF_dmu, dF_dv of mixed sign) and predict: the Woodbury vector and inverses, diag and full variances
        loopback/rankR   one two-rank VarDTC evaluation over the loopback transport, scalar and per-point noise, set up as
                         test_row_sharded_mode_over_the_loopback_transport of tests/test_gpu_sparse.py
    python tools/sparse_bits.py --compare A B    name every array whose bytes differ; exit status 1 if any does

The dumps are device results (device libm included): compare two of the same machine, keep none as a fixture.
"""
import argparse
import os
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def dump(path):
    import psi_np as P
    import sparse_ld as SL
    import svgp_np as SV
    import test_gpu_psi as TP
    from gpy_amd import _lib as L
    from gpy_amd import grid as G
    from oracle import gp_oracle as O
    from oracle import sparse_oracle as S

    out = {}
    SC = L.SparseContext

    def put(name, value):
        if isinstance(value, dict):
            for k in sorted(value):
                put(name + "/" + k, value[k])
        elif value is not None:
            out[name] = np.ascontiguousarray(np.asarray(value, dtype=np.float64))

    def numeric(r):
        return {q: v for q, v in r.items() if isinstance(v, (float, np.floating, np.ndarray))}

    ctx = SC(0)
    for name in SL.PLAIN + SL.BLOCKED[:1]:
        c = SL.make_case(name)
        ctx.set_data(c["X"], c["R"])
        info, r = ctx.vardtc_sum(c["specs"], c["Z"], c["noise"], want_dL_dm=True)
        assert info == 0, (name, info)
        tag = "vardtc/" + name
        put(tag + "/result", numeric(r))
        for which in range(6):
            put(tag + "/fetch%d" % which, ctx.fetch(which))
        r0, nr = c["block"]
        put(tag + "/dL_dKnm_block", ctx.fetch_dL_dKnm(r0, max(min(nr, 300), 1)))
        mu, var = ctx.predict(c["specs"], c["Xs129"])
        put(tag + "/predict", {"mu": mu, "var": var, "cov": ctx.predict(c["specs"], c["Xs129"], full_cov=True)[1]})
    ctx.close()

    for N, M, Q, ARD, w in TP.CASES:
        p = P.fit_problem(N, M, Q, 2, 100 + N + M + Q, ARD, [0.3] if w else [])
        specs = [("rbf", ARD, np.concatenate([[p["var"]], p["ls"]]), None, 0)] + [("white", False, np.array([v]), None, 0) for v in p["white"]]
        ctx = SC(0)
        ctx.set_data(p["mu"], p["Y"])
        ctx.set_input_variance(p["S"])
        info, r = ctx.vardtc_uncertain(specs, p["Z"], p["noise"])
        assert info == 0, ((N, M, Q, ARD, w), info)
        put("uncertain/N%d_M%d_Q%d_%d%d" % (N, M, Q, ARD, w), numeric(r))
        ctx.close()

    ctx = SC(0)
    for name in SV.PLAIN + SV.BLOCKED[:1]:
        c = SV.make_case(name)
        rng = np.random.default_rng(c["N"] + 7 * c["M"])
        dFm, dFv = rng.standard_normal((c["N"], c["L"])), rng.standard_normal((c["N"], c["L"])) - 0.5
        ctx.set_data(c["X"], c["Y"])
        info, fw = ctx.svgp_forward(c["specs"], c["Z"], c["q_mean"], c["q_L"])
        assert info == 0, (name, info)
        tag = "svgp/" + name
        put(tag + "/forward", numeric(fw))
        put(tag + "/backward", numeric(ctx.svgp_backward(dFm, dFv)))
        wv, wi = ctx.svgp_woodbury()
        mu, var = ctx.svgp_predict(c["specs"], c["Xs"]["129"])
        put(tag + "/predict", {"wv": wv, "winv": wi, "mu": mu, "var": var,
                               "cov": ctx.svgp_predict(c["specs"], c["Xs"]["129"], full_cov=True)[1]})
    ctx.close()

    N, M, D, world = 5000, 96, 4, 2
    X, Y = O.synthetic(N, D, seed=5)
    Z = S.synthetic_Z(X, M, 0)
    specs = [("rbf", True, np.array([1.1, 0.7, 1.0, 1.3, 1.6]), None, 0), ("bias", False, np.array([0.2]), None, 0)]
    for tag, noise in (("hom", 0.1), ("het", 0.05 + 0.1 * np.random.default_rng(1).random(N))):
        res, errs = [None] * world, []

        def work(rank):
            try:
                c = SC(0)
                try:
                    lo, hi = G.shard_rows(N, rank, world)
                    c.attach_loopback(rank, world, group_key=7000 + (1 if np.ndim(noise) else 0))
                    c.set_data(X[lo:hi], Y[lo:hi])
                    info, r = c.vardtc_sum(specs, Z, noise[lo:hi] if np.ndim(noise) else noise)
                    assert info == 0
                    res[rank] = numeric(r)
                finally:
                    c.close()
            except Exception as e:      # noqa: BLE001
                errs.append(e)
        ts = [threading.Thread(target=work, args=(r,)) for r in range(world)]
        [t.start() for t in ts]
        [t.join(timeout=120) for t in ts]
        assert not errs, errs
        for rank in range(world):
            put("loopback/%s/rank%d" % (tag, rank), res[rank])
    np.savez(path, **out)
    print("sparse_bits: %d arrays, %d doubles -> %s (library %s)" % (len(out), sum(a.size for a in out.values()), path, L.LIB_PATH))


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
    print("sparse_bits compare: %d arrays, %d doubles, %d differing" % (len(names), sum(A[n].size for n in A.files), len(bad)))
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
