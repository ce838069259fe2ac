"""Cases, long-double reference and judge of the 2D block-cyclic grid evaluation (gpy_amd/csrc/grid.hip, grid_comm.hip,
gpy_amd/grid.py) at the edges of its layout, shared by tests/test_oracle_grid_ld.py (CPU) and tests/test_gpu_grid_shapes.py (GPU).

Reference: `kern_ld.exact` (80-bit kernels, column-oriented Cholesky, triangular solves, explicit-sum products) on the inputs of
`oracle.gp_oracle.synthetic` with the parameters of `default_theta`, jitter 1e-8; from it

    lml, logdet, alpha, dtheta (with its cond), L, Linv = L^-1,  datafit = sum alpha o Y,  trKinv = tr Ky^-1,
    diag_dL_dK = diag((alpha alpha^T - Dy Ky^-1) / 2),  dnoise = its sum (one noise variance) or the vector itself (one per point),

and the same call with dt = float64 as the fp64 restatement.  A reference is keyed by (kind, ARD, N, D, Dy, noise tag, seed) --
never by the layout: every process grid, tile edge and option triple at one N is held against the same numbers (one reference at
N = 513, about 9 s of long-double Cholesky, serves 33 cases).

Judge: the project's rule (tests/sparse_ld.py `rel_err` / `bound`, tests/kern_ld.py `grad_tol`), nothing new:

    err(q) = max |got - q_ld| / max |q_ld|  <=  max(32 e64(q), 256 eps64 kappa)     q in QUANTITIES
    |dtheta_k - dtheta_k_ld|                <=  max(32 e64_k, 256 eps64 cond_k)     every entry

with e64 the distance of the fp64 restatement from long double on the same input (never a device figure) and kappa = cond2 of the
fp64 K + noise + jitter, at most 1e4 in every case (KAPPA_MAX; asserted on the CPU), so that the kappa arm stays below 6e-10.
The fetched factors are judged by tests/dense_ld.py as in tests/test_gpu_dense_ld.py: |A - L L^T| <= gamma_{n+1} |L| |L^T| + 1e-13 v
elementwise over the lower triangle (A = the long-double K rounded to fp64, plus noise and jitter; 1e-13 x variance is what the
project allows a device covariance entry), in fp64 at twice the bound and in long double at the bound; the figures of Linv
(|Linv L - I|, |L Linv - I| over n u |.||.|, with the SAME L) at most 8 times the larger of LAPACK's dtrtri and the 128-block
transcription on that L; both strict upper triangles exactly zero; no NaN anywhere.

Families (default: Matern-5/2 ARD, D = 3, Dy = 2, one noise variance; T = ceil(N / nb) tiles a side):

    n_edge   2 x 2, nb = 128, N = 1 | 2 | 127 | 128 (T = 1: three ranks without a tile), 129 | 255 | 256 (T = 2: rank (0, 1) holds only
             the tile above the diagonal; a last tile with one real row; an exact multiple), 257 | 385 | 513 (T = 3, 4, 5)
    layout   nb = 128, N = 257 (T = 3) and 513 (T = 5) on 1x2, 2x1, 1x3, 3x1, 3x2, 2x3, 3x3, 2x4, 4x2, 1x7: T < P (empty process
             rows / columns), T == P, wrap-around
    subtile  nb = 256 (q = 2 sub-tiles a side) on 2x2 and 3x2, N = 128 (the second sub-tile all padding) | 129 | 255 | 256 | 257 |
             513; nb = 384 (q = 3) on 2x2 at N = 385
    d_edge   D = 1 | 32 | 33 | 65, ARD and iso, N = 257: one, two, three ARD groups of 32 dimensions
    dy       Dy = 1 | 4 | 5, N = 257: one reduction per output column
    kinds    RBF, Matern-3/2, Exponential, iso and ARD, on 3x2 at N = 257
    noise    one variance per point, uniform in [0.05, 0.15]: N = 257 at nb = 256, N = 129 at nb = 128 (the padding next to it)
    options  every (G, GW, lookahead) of test_gpu_grid.BLOCKING_OPTIONS at N = 513 (T = 5: G not dividing T, 2 G > T) on 2x2 and 4x2

plus STALE (the data sets one context is walked through), GENERIC (the 1 x 1 grid on the generic code) and DETERMINISM."""
import numpy as np

import dense_ld as DL
import kern_ld as KL
import sparse_ld as SL
from gpy_amd import grid as G
from oracle import gp_oracle as O
from predict_ld import figures_line  # noqa: F401  (the FIG line of the GPU tests)
from test_gpu_grid import BLOCKING_OPTIONS

LD = KL.LD
EPS64 = KL.EPS64
JITTER = 1e-8
MAX_N = 513
KAPPA_MAX = 1e4
K_TOL = 1e-13                     # x variance: the project's tolerance of one device covariance entry (kern_ld.k_ok)
INV_FACTOR = 8.0                  # tests/test_gpu_dense_ld.py
QUANTITIES = ("lml", "logdet", "datafit", "dnoise", "trKinv", "alpha", "diag_dL_dK", "dtheta")
FAMILIES = ("n_edge", "layout", "subtile", "d_edge", "dy", "kinds", "noise", "options")
LAYOUTS = ((1, 2), (2, 1), (1, 3), (3, 1), (3, 2), (2, 3), (3, 3), (2, 4), (4, 2), (1, 7))

rel_err = SL.rel_err
bound = SL.bound


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def _case(family, N, Pr, Pc, nb, kind="matern52", ARD=True, D=3, Dy=2, het=False, options=None):
    name = "%s-%s_%s-n%d_d%d_dy%d_%s-%dx%d_nb%d" % (family, kind, "ard" if ARD else "iso", N, D, Dy, "het" if het else "hom", Pr, Pc, nb)
    if options is not None:
        name += "-G%d_GW%d_la%d" % tuple(options)
    return dict(name=name, family=family, N=N, Pr=Pr, Pc=Pc, nb=nb, kind=kind, ARD=ARD, D=D, Dy=Dy, het=het, options=options)


def _cases():
    out = [_case("n_edge", N, 2, 2, 128) for N in (1, 2, 127, 128, 129, 255, 256, 257, 385, 513)]
    out += [_case("layout", N, Pr, Pc, 128) for Pr, Pc in LAYOUTS for N in (257, 513)]
    out += [_case("subtile", N, Pr, 2, 256) for Pr in (2, 3) for N in (128, 129, 255, 256, 257, 513)]
    out += [_case("subtile", 385, 2, 2, 384)]
    out += [_case("d_edge", 257, 2, 2, 128, D=D, ARD=ARD) for D in (1, 32, 33, 65) for ARD in (True, False)]
    out += [_case("dy", 257, 2, 2, 128, Dy=Dy) for Dy in (1, 4, 5)]
    out += [_case("kinds", 257, 3, 2, 128, kind=k, ARD=ARD) for k in ("rbf", "matern32", "exponential") for ARD in (False, True)]
    out += [_case("noise", 257, 2, 2, 256, het=True), _case("noise", 129, 2, 2, 128, het=True)]
    out += [_case("options", 513, Pr, 2, 128, options=o) for Pr in (2, 4) for o in BLOCKING_OPTIONS]
    return out


CASES = _cases()
NAMES = [c["name"] for c in CASES]
BY_NAME = dict((c["name"], c) for c in CASES)
assert len(BY_NAME) == len(CASES)
# one 2 x 2 context, nb = 128, new data at every step
STALE = [_case("stale", 513, 2, 2, 128), _case("stale", 1, 2, 2, 128), _case("stale", 257, 2, 2, 128),
         _case("stale", 129, 2, 2, 128, D=33, Dy=5)]
# the 1 x 1 grid on the generic code (MI355GP_GRID_FORCE_GENERIC=1, diagnostics library)
GENERIC = [_case("generic", N, 1, 1, 128) for N in (1, 129, 257)] + [_case("generic", 257, 1, 1, 256)]
DETERMINISM = _case("determinism", 385, 3, 2, 128)
FAULT_CASE = "n_edge-matern52_ard-n257_d3_dy2_hom-2x2_nb128"
FAULT_CASE_D33 = "d_edge-matern52_ard-n257_d33_dy2_hom-2x2_nb128"
FAULT_CASE_HET = "noise-matern52_ard-n257_d3_dy2_het-2x2_nb256"
ACCEPT_513 = "n_edge-matern52_ard-n513_d3_dy2_hom-2x2_nb128"


def by_family(family):
    return [c["name"] for c in CASES if c["family"] == family]


def _get(case):
    return BY_NAME[case] if isinstance(case, str) else case


def seed_of(c):
    return 7919 + c["N"] + 31 * c["D"] + c["Dy"]


def ref_key(case):
    """what a reference depends on: never the layout, the tile edge or the options"""
    c = _get(case)
    return (c["kind"], bool(c["ARD"]), c["N"], c["D"], c["Dy"], "het" if c["het"] else "hom", seed_of(c))


def shapes():
    """every (N, nb, Pr, Pc) of the table"""
    return sorted(set((c["N"], c["nb"], c["Pr"], c["Pc"]) for c in CASES + STALE + GENERIC + [DETERMINISM]))


def make_inputs(case):
    """dict(X, Y, var, ls, theta (as the device takes it), noise (a float, or N of them), specs (as kern_ld takes them))"""
    c = _get(case)
    N, D = c["N"], c["D"]
    X, Y = O.synthetic(N, D, seed=seed_of(c), Dy=c["Dy"])
    var, ls, noise = O.default_theta(D, c["ARD"])
    if c["het"]:
        noise = 0.05 + 0.1 * np.random.default_rng(seed_of(c)).random(N)
    theta = np.concatenate([[var], np.atleast_1d(ls)])
    specs = [(c["kind"], int(c["ARD"]), theta, np.arange(D), 0)]
    return dict(X=X, Y=Y, var=var, ls=ls, theta=theta, noise=noise, specs=specs)


# ---- the reference -----------------------------------------------------------------------------------------------------------
def evaluate(specs, X, Y, noise, dt=LD, het_as_scalar=False):
    """the judged quantities (and L, Linv, Ki_diag, dtheta_cond) of one exact-GP evaluation in the working type; noise: one variance
    or N of them -- then dnoise is the vector diag(dL_dK) and dnoise_sum its sum"""
    noise = np.asarray(noise, dtype=np.float64)
    ex = KL.exact(specs, X, Y, noise if noise.ndim else float(noise), jitter=JITTER, dt=dt, max_n=MAX_N)
    Yt = KL._a(Y, dt)
    diag = np.diag(ex["dL_dK"]).copy()
    out = dict(lml=ex["lml"], logdet=ex["logdet"], datafit=np.sum(ex["alpha"] * Yt), trKinv=np.sum(np.diag(ex["Ki"])),
               alpha=ex["alpha"], diag_dL_dK=diag, dtheta=ex["dtheta"], dtheta_cond=ex["dtheta_cond"], L=ex["L"], Linv=ex["Linv"],
               Ki_diag=np.diag(ex["Ki"]).copy(), dnoise=ex["dnoise"])
    if noise.ndim:
        out["dnoise"], out["dnoise_sum"] = diag, ex["dnoise"]
    return out


_MEMO, _KAPPA = {}, {}


def gram64(case):
    """A = the long-double K rounded to fp64, plus noise plus jitter (what the device factorises, up to K_TOL x variance an entry)"""
    inp = make_inputs(case)
    A = KL.f64(KL.K(inp["specs"], inp["X"], None, LD if KL.HAVE_LD else np.float64))
    n = A.shape[0]
    A[np.arange(n), np.arange(n)] += inp["noise"] + JITTER
    return A


def kappa_of(case):
    """cond2(K + noise + jitter) in fp64, once per reference key"""
    key = ref_key(case)
    if key not in _KAPPA:
        inp = make_inputs(case)
        Ky = np.array(KL.K(inp["specs"], inp["X"], None, np.float64), dtype=np.float64)
        n = Ky.shape[0]
        Ky[np.arange(n), np.arange(n)] += inp["noise"] + JITTER
        _KAPPA[key] = float(np.linalg.cond(Ky))
    return _KAPPA[key]


def reference(case):
    """(inputs, long-double reference, the same in fp64, kappa, A) of a case: computed once per reference key and process, shared by
    every layout and option triple, and not to be modified"""
    key = ref_key(case)
    if key not in _MEMO:
        KL.require_ld()
        inp = make_inputs(case)
        args = (inp["specs"], inp["X"], inp["Y"], inp["noise"])
        ref, r64 = evaluate(*args, dt=LD), evaluate(*args, dt=np.float64)
        A = gram64(case)
        for d in (ref, r64, inp):
            for v in d.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        A.setflags(write=False)
        _MEMO[key] = (inp, ref, r64, kappa_of(case), A)
    return _MEMO[key]


def lapack_result(case):
    """the fp64 restatement as a device result would come back: the judged quantities in fp64, LAPACK's L of A and dtrtri's
    inverse of it (a fresh copy: the fault planters write into it)"""
    inp, ref, r64, kappa, A = reference(case)
    got = dict((q, np.array(KL.f64(r64[q]))) for q in QUANTITIES)
    if "dnoise_sum" in r64:
        got["dnoise_sum"] = np.array(KL.f64(r64["dnoise_sum"]))
    got["L"] = np.linalg.cholesky(A)
    got["Linv"] = DL.trtri_lapack(got["L"])
    return got


# ---- the judge ---------------------------------------------------------------------------------------------------------------
def chol_figures(A, L, slack):
    """dense_ld.chol_figures with `slack` added to every element's bound: (fp64 BLAS figure over every element of the lower
    triangle against twice the bound, long-double figure against the bound)"""
    if slack == 0.0:
        return DL.chol_figures(A, L)
    n = A.shape[0]
    low = np.tril(np.ones((n, n), dtype=bool))
    bnd = DL.gamma(n + 1) * (np.abs(L) @ np.abs(L.T)) + slack
    f64 = DL._worst(np.abs(A - L @ L.T), 2.0 * bnd, low)
    if not KL.HAVE_LD:
        return f64, None
    return f64, max(DL._worst(e, bnd[ix], low[ix]) for e, ix in DL._ld_parts(L, L.T, "lu", A))


def judge_factors(Lg, Li, A, variance):
    """the fetched L and L^-1 against the matrix they factorise: ({name: (figure, limit)}, [what failed])"""
    figs, bad = {}, []
    n = A.shape[0]
    if np.shape(Lg) != (n, n) or np.shape(Li) != (n, n):
        return figs, ["L / Linv: shape %s / %s, not %s" % (np.shape(Lg), np.shape(Li), (n, n))]
    if np.isnan(Lg).any() or np.isnan(Li).any():
        return figs, ["NaN in L or Linv"]
    for name, M in (("L", Lg), ("Linv", Li)):
        if np.any(np.triu(M, 1) != 0.0):
            bad.append("%s: the strict upper triangle is not exactly zero" % name)
    f64, ld = chol_figures(A, Lg, K_TOL * float(variance))
    figs["chol64"] = (f64, 1.0)
    if ld is not None:
        figs["chol"] = (ld, 1.0)
    if not (f64 <= 1.0 and (ld is None or ld <= 1.0)):
        bad.append("|A - L L^T|: %.3f of twice the bound against fp64 BLAS, %s of the bound in long double" % (f64, ld))
    inv = DL.inv_figures(Lg, Li)
    refs = (DL.inv_figures(Lg, DL.trtri_lapack(Lg)), DL.inv_figures(Lg, DL.trtri_blocked(Lg)))
    for side, name in ((0, "LinvL"), (1, "LLinv")):
        lim = INV_FACTOR * max(refs[0][side], refs[1][side])
        figs[name] = (inv[side], lim)
        if not inv[side] <= lim:
            bad.append("%s - I: figure %.4f, references %.4f (dtrtri) %.4f (transcription)" % (name, inv[side], refs[0][side], refs[1][side]))
    return figs, bad


def judge(got, ref_ld, ref_64, kappa, A=None, variance=1.0):
    """Hold every quantity of QUANTITIES to err(q) <= bound(q), every dtheta entry to its own grad_tol, `dnoise_sum` (per-point
    noise: the scalar the device reports next to the vector) to the same rule, and -- where `got` has L and Linv -- the factors to
    the dense figures.  Nothing may be NaN or missing.  Returns ({q: (err, bound)}, [what failed])."""
    figs, bad = {}, []
    for q in QUANTITIES + (("dnoise_sum",) if "dnoise_sum" in ref_ld else ()):
        if got.get(q) is None:
            bad.append("%s is missing" % q)
            continue
        if np.isnan(np.asarray(got[q], dtype=np.float64)).any():
            bad.append("%s has a NaN" % q)
            continue
        e, b = rel_err(got[q], ref_ld[q]), bound(q, ref_ld, ref_64, kappa)
        figs[q] = (e, b)
        if not e <= b:
            bad.append("%s: %.3e > %.3e" % (q, e, b))
    if got.get("dtheta") is not None and not KL.grad_ok(got["dtheta"], ref_ld["dtheta"],
                                                         KL.grad_tol(ref_ld["dtheta"], ref_64["dtheta"], ref_ld["dtheta_cond"])):
        bad.append("dtheta: an entry outside max(32 e64, 256 eps64 cond): worst %.1f eps64 cond"
                   % KL.grad_figure(got["dtheta"], ref_ld["dtheta"], ref_ld["dtheta_cond"]))
    if "L" in got or "Linv" in got:
        assert A is not None
        f2, b2 = judge_factors(got.get("L"), got.get("Linv"), A, variance)
        figs.update(f2)
        bad += b2
    return figs, bad


# ---- planted faults (test_oracle_grid_ld.py): each takes (case, inputs, fp64 reference, a correct result) and returns a faulty copy
def _copy(got):
    return dict((k, np.array(v)) for k, v in got.items())


def _sums(bad, inp, Dy):
    """the scalars the host derives from alpha and diag Ky^-1, as grid_assemble does"""
    a2 = np.sum(np.square(bad["alpha"]), axis=1)
    bad["datafit"] = np.sum(bad["alpha"] * inp["Y"])
    bad["lml"] = 0.5 * (-bad["alpha"].size * np.log(2.0 * np.pi) - Dy * bad["logdet"] - bad["datafit"])
    return a2


def fault_missing_kinv_tile(c, inp, r64, got):
    """the second nb-tile of diag Ky^-1 never arrives: trKinv, diag_dL_dK and dnoise are formed without it"""
    bad = _copy(got)
    nb, Dy = c["nb"], c["Dy"]
    kd = np.array(KL.f64(r64["Ki_diag"]))
    kd[nb:2 * nb] = 0.0
    a2 = np.sum(np.square(bad["alpha"]), axis=1)
    bad["trKinv"] = kd.sum()
    bad["diag_dL_dK"] = 0.5 * (a2 - Dy * kd)
    bad["dnoise"] = bad["diag_dL_dK"].sum()
    return bad


def fault_padding_pivot(c, inp, r64, got):
    """one padding row enters the log-determinant with the pivot of a real row (noise + jitter instead of 1)"""
    bad = _copy(got)
    bad["logdet"] = bad["logdet"] + np.log(np.min(inp["noise"]) + JITTER)
    _sums(bad, inp, c["Dy"])
    return bad


def fault_alpha_partial(c, inp, r64, got, rank=3):
    """alpha = X^T y without the partial sum of one rank: the rows and columns of its tiles, from grid.local_tiles"""
    bad = _copy(got)
    N, nb, Pr, Pc = c["N"], c["nb"], c["Pr"], c["Pc"]
    T = -(-N // nb)
    pr, pc = G.rank_coords(rank, Pc)
    rows = [i for I in G.local_tiles(T, pr, Pr) for i in range(I * nb, min((I + 1) * nb, N))]
    cols = [j for J in G.local_tiles(T, pc, Pc) for j in range(J * nb, min((J + 1) * nb, N))]
    assert rows and cols and all(G.tile_owner(i // nb, j // nb, Pr, Pc) == rank for i in rows[::nb] for j in cols[::nb])
    Li = got["Linv"]
    y = Li @ inp["Y"]
    bad["alpha"][cols] -= Li[np.ix_(rows, cols)].T @ y[rows]
    _sums(bad, inp, c["Dy"])
    return bad


def fault_ard_group(c, inp, r64, got):
    """the second ARD group (dimensions 32 ..) never reaches dtheta"""
    assert c["ARD"] and c["D"] > 32
    bad = _copy(got)
    bad["dtheta"][1 + 32:] = 0.0
    return bad


def fault_noise0(c, inp, r64, got):
    """noise[0] on every row of a per-point noise case"""
    assert c["het"]
    r = evaluate(inp["specs"], inp["X"], inp["Y"], np.full(c["N"], inp["noise"][0]), dt=np.float64)
    bad = dict((q, np.array(KL.f64(r[q]))) for q in QUANTITIES + ("dnoise_sum", "L", "Linv"))
    return bad


def fault_missing_slab(c, inp, r64, got):
    """one 16-term k-slab missing from the update of one 128 x 128 tile of L (the last tile row, the tile before the diagonal)"""
    bad = _copy(got)
    n = c["N"]
    ti, tj = (n - 1) // 128, (n - 1) // 128 - 1
    assert tj >= 1
    r, s = slice(ti * 128, min((ti + 1) * 128, n)), slice(tj * 128, (tj + 1) * 128)
    k0 = 16 * (tj * 128 // 32)
    Lf = got["L"]
    lost = Lf[r, k0:k0 + 16] @ Lf[s, k0:k0 + 16].T                          # what the trailing update did not subtract
    bad["L"][r, s] += np.linalg.solve(Lf[s, s], lost.T).T                  # ... through the panel solve L_ik = A_ik L_kk^-T
    return bad


FAULTS = {"one nb-tile of Ki missing from trKinv / diag_dL_dK": (FAULT_CASE, fault_missing_kinv_tile),
          "one padding row counted in logdet": (FAULT_CASE, fault_padding_pivot),
          "alpha without one rank's partial sum": (FAULT_CASE, fault_alpha_partial),
          "one ARD group dropped from dtheta": (FAULT_CASE_D33, fault_ard_group),
          "noise[0] on every row": (FAULT_CASE_HET, fault_noise0),
          "one 16-term k-slab missing from one tile of L": (FAULT_CASE, fault_missing_slab)}
