"""Bit-for-bit record of what the 2D block-cyclic grid mode computes, for comparing two builds of the library (MI355GP_LIB
chooses it).

    python tools/grid_bits.py --out FILE.npz   store the raw fp64 outputs of
        loopback/ID      every entry of CASES in tests/test_gpu_grid.py over the loopback transport
        options/ID       the 2 x 4, nb = 128, N = 1150 shape of test_two_level_blocking_options under every (G, GW, lookahead)
                         triple of BLOCKING_OPTIONS, on one context as the test runs them
        het              the heteroscedastic 2 x 3 case
                         -- for each of these: lml, logdet, dnoise, alpha, dtheta, diag_dL_dK, fetch(FETCH_L), fetch(FETCH_LINV)
                            and coll_log(r) of every rank (not on the degenerate 1 x 1 grid, which keeps no log)
        npd              the two info codes of the not-positive-definite case
        rccl1            the RCCL transport at world size 1 (test_rccl_transport_world_size_one): the same outputs and its log
        generic1x1       only with the diagnostics library and MI355GP_GRID_FORCE_GENERIC=1: the 1 x 1 grid on the generic code
                         (the 1 x 1 entries of CASES then run it as well)
    python tools/grid_bits.py --compare A B    name every array whose bytes differ; exit status 1 if any does

Stage times are not stored.  The dumps are device results (device libm included): compare two of the same machine, keep none
as a fixture.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def dump(path):
    import test_gpu_grid as TG
    from gpy_amd import _lib as L
    from gpy_amd import grid as G
    from oracle import gp_oracle as O

    out = {}
    generic = bool(int(os.environ.get("MI355GP_GRID_FORCE_GENERIC") or 0)) and "diag" in os.path.basename(L.LIB_PATH)

    def put(name, value):
        out[name] = np.ascontiguousarray(np.asarray(value, dtype=np.float64))

    def record(tag, g, info, res, ranks):
        assert info == 0, (tag, info)
        for k in ("lml", "logdet", "dnoise", "alpha", "dtheta", "diag_dL_dK"):
            put(tag + "/" + k, res[k])
        put(tag + "/L", g.fetch(G.FETCH_L))
        put(tag + "/Linv", g.fetch(G.FETCH_LINV))
        for r in range(ranks):
            log = g.coll_log(r)
            put(tag + "/coll_log/rank%d" % r, [[log[c][0], log[c][1] >> 32, log[c][1] & 0xffffffff] for c in ("world", "row", "col")])

    def loopback(tag, kind, ARD, N, D, Dy, Pr, Pc, nb):
        X, Y = O.synthetic(N, D, seed=N + Pr, Dy=Dy)
        var, ls, noise = O.default_theta(D, ARD)
        g = G.GridContext.loopback(Pr, Pc, nb)
        try:
            g.set_data(X, Y)
            info, res = g.exact_inference(kind, ARD, L.theta_vec(var, ls, ARD, D), noise, want_diag=True)
            record(tag, g, info, res, Pr * Pc if (Pr * Pc > 1 or generic) else 0)
        finally:
            g.close()

    for kind, ARD, N, D, Dy, Pr, Pc, nb in TG.CASES:
        loopback("loopback/%s_%d_N%d_D%d_Dy%d_%dx%d_nb%d" % (kind, ARD, N, D, Dy, Pr, Pc, nb), kind, ARD, N, D, Dy, Pr, Pc, nb)
    if generic:
        loopback("generic1x1", "rbf", False, 300, 3, 1, 1, 1, 128)

    Pr, Pc, nb, N = 2, 4, 128, 1150                      # _blocking_options_case
    kind, ARD, D = "matern52", True, 4
    X, Y = O.synthetic(N, D, seed=N + 3, Dy=2)
    var, ls, noise = O.default_theta(D, ARD)
    g = G.GridContext.loopback(Pr, Pc, nb)
    try:
        g.set_data(X, Y)
        for Gs, GW, la in TG.BLOCKING_OPTIONS:
            g.set_option("G", Gs)
            g.set_option("GW", GW)
            g.set_option("lookahead", la)
            info, res = g.exact_inference(kind, ARD, L.theta_vec(var, ls, ARD, D), noise, want_diag=True)
            record("options/G%d_GW%d_la%d" % (Gs, GW, la), g, info, res, Pr * Pc)
    finally:
        g.close()

    N, D = 1100, 6                                       # test_grid_agrees_with_single_gpu_path_and_heteroscedastic_noise
    X, Y = O.synthetic(N, D, seed=5)
    var, ls, _ = O.default_theta(D, True)
    noise = 0.05 + 0.1 * np.random.default_rng(1).random(N)
    g = G.GridContext.loopback(2, 3, 256)
    try:
        g.set_data(X, Y)
        info, res = g.exact_inference("matern52", True, L.theta_vec(var, ls, True, D), noise, want_diag=True)
        record("het", g, info, res, 6)
    finally:
        g.close()

    N, D = 400, 2                                        # test_grid_reports_not_positive_definite_on_every_rank
    X, Y = O.synthetic(N, D, seed=3)
    X[200:] = X[:200]
    g = G.GridContext.loopback(2, 2, 128)
    try:
        g.set_data(X, Y)
        th = L.theta_vec(1.0, 1.0, False, D)
        put("npd/info", [g.exact_inference("rbf", False, th, 0.0, jitter=0.0)[0],
                         g.exact_inference("rbf", False, th, 0.0, jitter=0.0, extra_jitter=1e-4)[0]])
    finally:
        g.close()

    N, D = 600, 3                                        # test_rccl_transport_world_size_one
    X, Y = O.synthetic(N, D, seed=9)
    var, ls, noise = O.default_theta(D, False)
    g = G.GridContext(0, 0, 1, 1, 1, 256, G.unique_id())
    try:
        g.set_data(X, Y)
        info, res = g.exact_inference("rbf", False, L.theta_vec(var, ls, False, D), noise, want_diag=True)
        record("rccl1", g, info, res, 1)
    finally:
        g.close()

    np.savez(path, **out)
    print("grid_bits: %d arrays, %d doubles -> %s (library %s%s)" % (
        len(out), sum(a.size for a in out.values()), path, L.LIB_PATH, ", generic 1 x 1" if generic else ""))


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
    print("grid_bits compare: %d arrays, %d doubles, %d differing" % (len(names), sum(A[n].size for n in A.files), len(bad)))
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
