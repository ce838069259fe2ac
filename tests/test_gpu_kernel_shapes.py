"""GPU (-m gpu): every kernel kind of the exact-GP device path at tile, chunk and column edges, judged against the long-double
restatement tests/kern_ld.py (80-bit, eps 1.08e-19), and the sparse path on its dispatch boundaries.

Shapes (N, M, D, Dy) = kern_ld.SHAPES: 1/1/1/1, 2/3/3/1, 63/1/2/1 (one partial 64 x 64 tile, a one-column block), 64/65/32/2
(exact tile, exact 32-dimension chunk), 65/63/33/1 (tile + 1, second ARD group), 65/64/65/5 (three chunks / groups, more than
four output columns), 129/130/5/4 (128-row padding + 1; active_dims a strict subset).  Inputs: kern_ld.make_case (row 1 of X
equals row 0, one row of X2 equals a row of X, an all-zero row for Linear / MLP / Poly, a pair exactly one period apart for
StdPeriodic).  Variants: kern_ld.VARIANTS (all twelve kinds, iso and ARD, Coregionalize rank 1 / 2 with P = 3, Poly order 1 / 3).

(a) stateless entry points through the kernel classes: |K - K_ld| <= 1e-13 x scale (scale = max Kdiag), K(X, X) bitwise
    symmetric, and every gradient entry within max(32 e64, 256 eps64 cond) of the long-double value: e64 = what the same formulas
    give in fp64 on the same input (never the device's figure), cond = the sum of the absolute terms of that entry.
(b) fused calls (exact_inference_sum alone / next to a White / times an RBF on two further columns, predict_sum, and
    exact_studentt_sum at 65/63/33/1) against the long-double Cholesky: the standing LML 1e-10, alpha 1e-9, prediction 1e-9,
    gradients 1e-8 of the largest entry, and every dtheta entry within max(10 x floor, 256) eps64 cond, floor = the figure of an
    fp64 SciPy pipeline for that case (tests/golden/kernel_shapes/floor.npz, tools/make_golden_kernel_shapes.py).
(c) what an entry point refuses by design is asserted by its message.
(d) vardtc_inference_sum, dL_dKnm and the Z gradients at N = 193, M = 65 on the (D, Dy) boundaries of the sparse dispatch
    (D = 16 | 17, 32 | 33, Dy = 4 | 5) against oracle/sparse_oracle.py with the tolerances of tests/test_gpu_sparse.py.

Measured on an MI355X (worst over the shapes; K in eps64 x scale, gradients in eps64 x cond; "stateless" = (a); "fused" = the
dtheta entries of (b), whose floor from the fp64 SciPy pipeline reaches 72.7):

    variant                 K  stateless      fused
    rbf_iso              1.48      12.65       9.59
    rbf_ard              1.46       4.51      20.02
    matern52_iso         1.88      22.53      21.65
    matern52_ard         1.82      20.57       9.29
    matern32_iso         1.50       8.50      16.46
    matern32_ard         1.64      22.20      11.48
    exponential_iso      0.92       3.27      97.85
    exponential_ard      0.80       8.24      10.27
    ratquad_iso          1.34      13.87       7.15
    ratquad_ard          1.18      64.17       3.97
    stdperiodic_iso      1.50       5.01      14.59
    stdperiodic_ard      1.20       1.63       6.21
    linear_iso           2.21       1.31      15.22
    linear_ard           1.36       1.02      12.13
    mlp_iso              1.89       2.89      11.90
    mlp_ard              1.62       1.95      22.06
    poly_o1              1.12       0.53       3.34
    poly_o3              2.39       1.52       5.86
    white                0.00       0.24       2.63
    bias                 0.00       0.46       3.85
    coreg_r1             0.39       0.51       7.79
    coreg_r2             0.42       0.45       7.91

The whole file: 324 cases, 16 s wall.  (d): LML within 9e-14, gradients within 2e-12, dZ / dL_dKnm within 9e-12, relative.

One case needed a kernel fix: `gradients_X(dL_dK, X)` (the X2-is-None form) at N = 2 / D = 3 for RBF, Matern52, Matern32 and
RatQuad, iso and ARD.  Both rows of X coincide there, so every pair has r = 0 and the reference returns exactly 0 (`_inv_dist`,
stationary.py:225-232); the device returned entries of 1e-17 ... 5e-16 (RBF iso: [[0, 4.6e-17, -2.3e-17], [-2.3e-17, -4.6e-17,
0]]).  `mi355gp_gradients_X` forms x_iq sum_j H_ij - sum_j H_ij x_jq from the column reduction H^T [X2~ | 1] with
H = dL_dK dK/dr / r, and for these kinds dK/dr / r stays finite at r = 0 (-K for RBF), so a coincident pair was not masked but
left to cancel, which it does only to rounding (the Exponential kernel, masked at r = 0 of necessity, was exact).  `k_grad` and
`k_grad_ext` (csrc/kern_ext.hip) now store H_ij = 0 where r_ij = 0.
"""
import os

import numpy as np
import pytest

import gpy_amd
from gpy_amd import _lib as L
from oracle import gp_oracle as O
from oracle import sparse_oracle as S

import kern_ld as KL
from test_oracle_sparse import check_sparse2

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not KL.HAVE_LD, reason="np.longdouble is not an extended format on this host")]
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [(v, s) for v in KL.VARIANTS for s in KL.SHAPES]
IDS = [KL.case_id(v, s) for v, s in CASES]
TOL_LML, TOL_ALPHA, TOL_GRAD, TOL_PRED = 1e-10, 1e-9, 1e-8, 1e-9
EPS = KL.EPS64


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def sctx():
    c = L.SparseContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def floors():
    z = np.load(os.path.join(HERE, "golden", "kernel_shapes", "floor.npz"))
    return dict(zip([str(n) for n in z["names"]], [float(f) for f in z["figures"]])), float(z["nu"])


def kernel(spec):
    """the gpy_amd kernel of one part"""
    kind, ard, th, dims, _ = spec
    nd = len(dims)
    cls = {"rbf": gpy_amd.RBF, "matern52": gpy_amd.Matern52, "matern32": gpy_amd.Matern32, "exponential": gpy_amd.Exponential}
    if kind in cls:
        return cls[kind](nd, th[0], th[1:], ARD=bool(ard), active_dims=dims)
    if kind == "ratquad":
        return gpy_amd.RatQuad(nd, th[0], th[1:-1], th[-1], ARD=bool(ard), active_dims=dims)
    if kind == "stdperiodic":
        npr = nd if ard & 1 else 1
        return gpy_amd.StdPeriodic(nd, th[0], th[1:1 + npr], th[1 + npr:], ARD1=bool(ard & 1), ARD2=bool(ard & 2), active_dims=dims)
    if kind == "linear":
        return gpy_amd.Linear(nd, th, ARD=bool(ard), active_dims=dims)
    if kind == "mlp":
        return gpy_amd.MLP(nd, th[0], th[1:-1] if ard else th[1], th[-1], ARD=bool(ard), active_dims=dims)
    if kind == "poly":
        return gpy_amd.Poly(nd, th[0], th[1], th[2], order=th[3], active_dims=dims)
    if kind == "white":
        return gpy_amd.White(nd, th[0], active_dims=dims)
    if kind == "bias":
        return gpy_amd.Bias(nd, th[0], active_dims=dims)
    P, r = ard % 100, ard // 100
    return gpy_amd.Coregionalize(1, P, rank=r, W=th[:P * r].reshape(P, r).copy(), kappa=th[P * r:].copy(), active_dims=dims)


def _judge(what, got, ref, ref64, worst):
    """print the figure of a gradient, then hold every entry to max(32 e64, 256 eps64 cond)"""
    val, cond = ref
    fig = KL.grad_figure(got, val, cond)
    worst.append(fig)
    print("    %s: %.2f eps x cond" % (what, fig))
    assert KL.grad_ok(got, val, KL.grad_tol(val, ref64, cond)), what


# ---- (a) stateless entry points ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,shape", CASES, ids=IDS)
def test_stateless_entry_points(variant, shape):
    c = KL.make_case(variant, shape)
    spec, X, X2, G, G2, scale = c["spec"], c["X"], c["X2"], c["G"], c["G2"], c["scale"]
    specs = [spec]
    k = kernel(spec)
    lv_s, lv_r = KL.leaves(specs, X), KL.leaves(specs, X, X2)
    f64 = dict(dt=np.float64)
    Ks, Kr = k.K(X), k.K(X, X2)
    Ks_ld, Kr_ld = KL.K(specs, X, lv=lv_s), KL.K(specs, X, X2, lv=lv_r)
    kd = k.Kdiag(X)
    fk = max(KL.k_figure(Ks, Ks_ld, scale), KL.k_figure(Kr, Kr_ld, scale), KL.k_figure(kd, KL.Kdiag(specs, X), scale))
    print("FIG %s K %.2f eps x scale" % (c["name"], fk))
    assert KL.k_ok(Ks, Ks_ld, scale) and KL.k_ok(Kr, Kr_ld, scale) and KL.k_ok(kd, KL.Kdiag(specs, X), scale)
    assert np.array_equal(Ks, Ks.T)
    worst = []
    k.update_gradients_full(G2, X, X2)                              # a non-symmetric rectangular dL_dK
    _judge("dtheta rectangular", np.atleast_1d(k.gradient).copy(), KL.dtheta(specs, G2, X, X2, lv=lv_r),
           KL.dtheta(specs, G2, X, X2, **f64)[0], worst)
    k.update_gradients_full(G, X)                                   # square, not symmetric
    _judge("dtheta square", np.atleast_1d(k.gradient).copy(), KL.dtheta(specs, G, X, lv=lv_s), KL.dtheta(specs, G, X, **f64)[0],
           worst)
    if spec[0] == "poly":                                           # (c) refused by design (poly.py:47-48), class and C-ABI
        with pytest.raises(NotImplementedError, match="Poly has no gradients_X"):
            k.gradients_X(G2, X, X2)
        with pytest.raises(L.MI355GPError, match="Poly .kind 11. has no gradients_X"):
            L.gradients_X("poly", 0, spec[2], G, np.ascontiguousarray(X[:, spec[3]]), None)
    else:
        _judge("gradients_X rectangular", k.gradients_X(G2, X, X2), KL.gradients_X(specs, G2, X, X2, lv=lv_r),
               KL.gradients_X(specs, G2, X, X2, **f64)[0], worst)
        _judge("gradients_X square", k.gradients_X(G, X), KL.gradients_X(specs, G, X, lv=lv_s),
               KL.gradients_X(specs, G, X, **f64)[0], worst)
    print("FIG %s grad %.2f eps x cond" % (c["name"], max(worst)))


# ---- (b) fused calls --------------------------------------------------------------------------------------------------------
def _check_fused(tag, specs, r, ex, floor, Y):
    dth = KL.chain_coreg(specs, r["dtheta"])
    lml, alpha, ref = float(ex["lml"]), KL.f64(ex["alpha"]), KL.f64(ex["dtheta"])
    fig = KL.grad_figure(dth, ex["dtheta"], ex["dtheta_cond"])
    print("FIG %s fused %.2f eps x cond (fp64 pipeline %.2f); lml %.2e alpha %.2e dtheta %.2e" % (
        tag, fig, floor, abs(r["lml"] - lml) / abs(lml), np.linalg.norm(r["alpha"] - alpha) / np.linalg.norm(alpha),
        np.abs(dth - ref).max() / np.abs(ref).max()))
    assert abs(r["lml"] - lml) <= TOL_LML * abs(lml)
    assert np.linalg.norm(r["alpha"] - alpha) <= TOL_ALPHA * np.linalg.norm(alpha)
    assert np.abs(dth - ref).max() <= TOL_GRAD * np.abs(ref).max()
    tol = KL.LD(max(10.0 * floor, 256.0) * EPS) * ex["dtheta_cond"]
    assert KL.grad_ok(dth, ex["dtheta"], tol), "dtheta per entry"


@pytest.mark.parametrize("variant,shape", CASES, ids=IDS)
def test_fused_calls(variant, shape, ctx, floors):
    floor, nu = floors
    c = KL.make_case(variant, shape)
    for label, specs, X, Xs in KL.fused_exprs(c):
        tag = KL.case_id(variant, shape) + "-" + label
        dev = KL.cabi_specs(specs)
        ctx.set_data(X, c["Y"])
        info, r = ctx.exact_inference_sum(dev, c["noise"])
        assert info == 0
        ex = KL.exact(specs, X, c["Y"], c["noise"])
        _check_fused(tag, specs, r, ex, floor[tag], c["Y"])
        assert abs(r["dnoise"] - float(ex["dnoise"])) <= TOL_GRAD * abs(float(ex["dnoise"]))
        scale = float(np.max(KL.Kdiag(specs, np.vstack([X, Xs]))))
        Kd = ctx.fetch(L.FETCH_K)
        assert KL.k_ok(Kd, KL.K(specs, X), scale) and np.array_equal(Kd, Kd.T)
        mu_ld, var_ld, cov_ld = KL.predict(specs, X, ex, Xs)
        mu, var = ctx.predict_sum(dev, Xs)
        _, cov = ctx.predict_sum(dev, Xs, full_cov=True)
        print("    prediction: mu %.2e var %.2e cov %.2e" % (np.abs(mu - KL.f64(mu_ld)).max(), np.abs(var - KL.f64(var_ld)).max(),
                                                             np.abs(cov - KL.f64(cov_ld)).max()))
        assert np.abs(mu - KL.f64(mu_ld)).max() <= TOL_PRED and np.abs(var - KL.f64(var_ld)).max() <= TOL_PRED
        assert np.abs(cov - KL.f64(cov_ld)).max() <= TOL_PRED
        if label == "plus_white" and tuple(shape) == KL.STUDENTT_SHAPE:
            info, r = ctx.exact_studentt_sum(dev, nu)
            assert info == 0
            _check_fused(tag[:-len(label)] + "studentt", specs, r, KL.exact(specs, X, c["Y"], 0.0, nu),
                         floor[tag[:-len(label)] + "studentt"], c["Y"])


# ---- (c) refusals by design --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,cls,theta", [("linear", "Linear", [1.0]), ("mlp", "MLP", [1.0, 1.0, 1.0]), ("poly", "Poly", [1.0, 1.0, 1.0, 2.0])])
def test_kern_Kdiag_of_the_c_abi_refuses_point_dependent_diagonals(kind, cls, theta):
    with pytest.raises(L.MI355GPError, match="diagonal of a %s .* depends on the points" % cls):
        L.kern_Kdiag(kind, np.array(theta), 4)


def test_coregionalize_above_the_output_limit_is_refused(ctx):
    X = np.zeros((4, 1))
    with pytest.raises(L.MI355GPError, match="number of outputs .ard. must be between 1 and 16, got 17"):
        L.kern_K("coregionalize", 17, np.eye(17).ravel(), X)
    with pytest.raises(L.MI355GPError, match="between 1 and 16, got 17"):
        L.update_gradients_full("coregionalize", 17, np.eye(17).ravel(), np.ones((4, 4)), X)
    ctx.set_data(X, np.ones((4, 1)))
    with pytest.raises(L.MI355GPError, match="between 1 and 16, got 17"):
        ctx.exact_inference_sum([("coregionalize", 17, np.eye(17).ravel(), np.array([0]), 0)], 0.1)
    with pytest.raises(L.MI355GPError, match="mi355gp_gradients_X: covariance kind 8 .* is not supported here"):   # no gradients_X of the kind in the C-ABI: zero on the host class
        L.gradients_X("coregionalize", 3, np.eye(3).ravel(), np.ones((4, 4)), X)


# ---- (d) the (D, Dy) boundaries of the sparse dispatch -----------------------------------------------------------------------
SPARSE_KERNELS = {"rbf_ard": lambda D, rng: [("rbf", True, 1.3, np.sqrt(D) * rng.uniform(0.8, 1.6, D), list(range(D)))],
                  "matern32_white": lambda D, rng: [("matern32", False, 0.9, np.array([1.2 * np.sqrt(D)]), list(range(D))),
                                                    ("white", False, 0.05, None, list(range(D)))]}


@pytest.mark.parametrize("kern", sorted(SPARSE_KERNELS))
@pytest.mark.parametrize("D,Dy", [(16, 4), (16, 5), (17, 1), (32, 4), (32, 5), (33, 1)])
def test_sparse_dispatch_boundaries(D, Dy, kern, sctx):
    N, M = 193, 65
    X, Y = O.synthetic(N, D, seed=D * 10 + Dy, Dy=Dy)
    Z = S.synthetic_Z(X, M, D)
    parts = SPARSE_KERNELS[kern](D, np.random.default_rng(D))
    ref = S.vardtc_general(parts, X, Z, Y, 0.07)
    specs = [(p[0], p[1], L.theta_vec(p[2], p[3], p[1], D) if p[3] is not None else np.array([p[2]]), np.asarray(p[4], np.int32), 0)
             for p in parts]
    sctx.set_data(X, Y)
    info, r = sctx.vardtc_sum(specs, Z, 0.07)
    assert info == 0
    B = sctx.fetch_dL_dKnm(0, N)
    rel = lambda a, b: np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max()
    print("sparse %s D=%d Dy=%d: lml %.2e dtheta %.2e dnoise %.2e dZ %.2e dL_dKnm %.2e" % (
        kern, D, Dy, abs(r["lml"] - ref["lml"]) / abs(ref["lml"]), rel(r["dtheta"], ref["dtheta"]), rel(r["dnoise"], ref["dnoise"]),
        rel(r["dZ"], ref["dZ"]), rel(B, ref["dL_dKnm"])))
    check_sparse2(r, ref)
    assert rel(B, ref["dL_dKnm"]) <= 1e-6
