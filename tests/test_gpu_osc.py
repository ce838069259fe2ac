"""GPU (-m gpu): Cosine, Sinc and ExpQuadCosine (C-ABI kinds 12 / 13 / 14) on the exact-GP device path, judged against the
long-double restatement tests/osc_ld.py (on the leaf machinery of tests/kern_ld.py) and against fixtures from the reference's own
code (tests/golden/osc, tools/make_golden_osc.py).

(a) K-level sweep, six variants (iso and ARD of each kind) x kern_ld.SHAPES, the kind over every column (no definiteness is
    needed): kern_K symmetric and cross and kern_Kdiag within 1e-13 x scale of long double (`kern_ld.k_ok`), K(X, X) bitwise
    symmetric with the variance exactly on its diagonal, and every entry of update_gradients_full (square and rectangular) and
    of gradients_X within max(32 e64, 256 eps64 cond): e64 = what the same formulas give in fp64 on the same input, cond = the
    sum of the absolute terms of that entry (`kern_ld.grad_tol`, as tests/test_gpu_kernel_shapes.py).
(b) fused calls at the same shapes with the kind on ONE column (the kinds are positive definite over one dimension only;
    tests/test_oracle_osc.py checks every case's Ky: cond_2 <= 1e5), alone / next to a White / times an RBF on two further
    columns, through exact_inference_sum and predict_sum against the long-double Cholesky: LML 1e-10, alpha 1e-9, prediction
    1e-9, gradients 1e-8 of the largest entry and every dtheta entry within max(10 x floor, 256) eps64 cond -- the bounds
    tests/test_gpu_kernel_shapes.py applies to RatQuad; floor = the figure of the restatement evaluated in fp64 on that case.
(c) one shape each: the Student-t process, predict with one new point, predictive_gradients, covariance_between_points and the
    Laplace session's kernel gradients from its resident dL_dK.
(d) the reference's fixtures at LML 1e-10, alpha 1e-9, gradients 1e-8, K 1e-13 x variance, prediction 1e-9, through the C-ABI
    and through GPRegression / the kernel classes.
(e) one fused case twice in fresh contexts: identical bytes.  The example's fit at reduced size reaches the reference's optimum.
    ExpQuadCosine + ExpQuadCosine fits and predicts through GPRegression and GPClassification with Laplace and EP.

Measured on an MI355X (worst over the shapes; K in eps64 x scale, bound 450; gradients in eps64 x cond, bound max(32 e64, 256);
"fused" = the dtheta entries of (b) and of the Student-t run, whose fp64 floor reaches 12.2):

    variant          K  stateless      fused
    cosine_iso    3.72      56.21       7.58
    cosine_ard    4.19      24.83       5.55
    sinc_iso      2.57      92.37      12.92
    sinc_ard      2.43     187.30      13.25
    eqc_iso       1.76      11.93       6.32
    eqc_ard       1.72      50.02      13.70

The stateless maxima all come from `gradients_X(dL_dK, X, X2)` at 63 / 1 / 2 / 1, where every output row is ONE term (M = 1) and
the device forms x_iq sum_j H_ij - sum_j H_ij x_jq instead of H_ij (x_iq - x_jq) (as for the other stationary kinds: RatQuad ARD
sits at 64 there); at every other shape the figures are below 21.  The whole file: 131 cases, 5 s."""
import importlib.util
import os

import numpy as np
import pytest

import gpy_amd
from gpy_amd import _lib as L

import kern_ld as KL
import osc_ld as OS

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not KL.HAVE_LD, reason="np.longdouble is not an extended format on this host")]
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [(v, s) for v in OS.VARIANTS for s in OS.SHAPES]
IDS = [OS.case_id(v, s) for v, s in CASES]
VIDS = [v[0] for v in OS.VARIANTS]
TOL_LML, TOL_ALPHA, TOL_GRAD, TOL_K, TOL_PRED = OS.TOL_LML, OS.TOL_ALPHA, OS.TOL_GRAD, OS.TOL_K, OS.TOL_PRED
EPS = KL.EPS64
NU = 5.0
F64 = dict(dt=np.float64)


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


def kernel(spec):
    """the gpy_amd kernel of one part"""
    kind, ard, th, dims, _ = spec
    nd = len(dims)
    nl = nd if ard else 1
    if kind == "cosine":
        return gpy_amd.Cosine(nd, th[0], th[1:1 + nl], ARD=bool(ard), active_dims=dims)
    if kind == "sinc":
        return gpy_amd.Sinc(nd, th[0], th[1:1 + nl], ARD=bool(ard), active_dims=dims)
    if kind == "expquadcosine":
        return gpy_amd.ExpQuadCosine(nd, th[0], th[1:1 + nl], th[1 + nl], ARD=bool(ard), active_dims=dims)
    if kind == "rbf":
        return gpy_amd.RBF(nd, th[0], th[1:], ARD=bool(ard), active_dims=dims)
    if kind == "bias":
        return gpy_amd.Bias(nd, th[0], active_dims=dims)
    assert kind == "white"
    return gpy_amd.White(nd, th[0], active_dims=dims)


def expression(specs):
    summands = []
    for t in KL.terms(specs):
        k = kernel(specs[t[0]])
        for i in t[1:]:
            k = k * kernel(specs[i])
        summands.append(k)
    k = summands[0]
    for s in summands[1:]:
        k = k + s
    return k


def _judge(what, got, ref, ref64, worst):
    """print the figure of a gradient, then hold every entry to max(32 e64, 256 eps64 cond)"""
    val, cond = ref
    fig = KL.grad_figure(got, val, cond)
    worst.append(fig)
    print("    %s: %.2f eps x cond" % (what, fig))
    assert KL.grad_ok(got, val, KL.grad_tol(val, ref64, cond)), what


# ---- (a) the K-level sweep ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,shape", CASES, ids=IDS)
def test_stateless_entry_points(variant, shape):
    c = OS.make_case(variant, shape)
    spec, X, X2, G, G2, scale = c["spec"], c["X"], c["X2"], c["G"], c["G2"], c["scale"]
    specs = [spec]
    k = kernel(spec)
    lv_s, lv_r = KL.leaves(specs, X), KL.leaves(specs, X, X2)
    Ks, Kr = k.K(X), k.K(X, X2)
    Ks_ld, Kr_ld = KL.K(specs, X, lv=lv_s), KL.K(specs, X, X2, lv=lv_r)
    kd = k.Kdiag(X)
    fk = max(KL.k_figure(Ks, Ks_ld, scale), KL.k_figure(Kr, Kr_ld, scale), KL.k_figure(kd, KL.Kdiag(specs, X), scale))
    print("FIG %s K %.2f eps x scale" % (c["name"], fk))
    assert KL.k_ok(Ks, Ks_ld, scale) and KL.k_ok(Kr, Kr_ld, scale) and KL.k_ok(kd, KL.Kdiag(specs, X), scale)
    assert np.array_equal(Ks, Ks.T)                                  # bitwise symmetric
    assert np.all(np.diag(Ks) == spec[2][0]) and np.all(kd == spec[2][0])        # r = 0: exactly the variance
    if shape[0] >= 2:
        assert Ks[0, 1] == spec[2][0] and Kr[-1, 0] == spec[2][0]    # the coincident pairs as well
    worst = []
    k.update_gradients_full(G2, X, X2)                               # a non-symmetric rectangular dL_dK
    _judge("dtheta rectangular", np.atleast_1d(k.gradient).copy(), KL.dtheta(specs, G2, X, X2, lv=lv_r),
           KL.dtheta(specs, G2, X, X2, **F64)[0], worst)
    k.update_gradients_full(G, X)                                    # square, not symmetric
    _judge("dtheta square", np.atleast_1d(k.gradient).copy(), KL.dtheta(specs, G, X, lv=lv_s), KL.dtheta(specs, G, X, **F64)[0],
           worst)
    _judge("gradients_X rectangular", k.gradients_X(G2, X, X2), KL.gradients_X(specs, G2, X, X2, lv=lv_r),
           KL.gradients_X(specs, G2, X, X2, **F64)[0], worst)
    _judge("gradients_X square", k.gradients_X(G, X), KL.gradients_X(specs, G, X, lv=lv_s),
           KL.gradients_X(specs, G, X, **F64)[0], worst)
    assert np.array_equal(k.gradients_X_diag(np.ones(shape[0]), X), np.zeros(X.shape))
    print("FIG %s grad %.2f eps x cond" % (c["name"], max(worst)))


# ---- (b) fused calls ---------------------------------------------------------------------------------------------------------
def _check_fused(tag, r, ex, floor):
    dth = np.asarray(r["dtheta"])
    lml, alpha, ref = float(ex["lml"]), KL.f64(ex["alpha"]), KL.f64(ex["dtheta"])
    fig = KL.grad_figure(dth, ex["dtheta"], ex["dtheta_cond"])
    print("FIG %s fused %.2f eps x cond (fp64 restatement %.2f); lml %.2e alpha %.2e dtheta %.2e" % (
        tag, fig, floor, abs(r["lml"] - lml) / abs(lml), np.linalg.norm(r["alpha"] - alpha) / np.linalg.norm(alpha),
        np.abs(dth - ref).max() / np.abs(ref).max()))
    assert abs(r["lml"] - lml) <= TOL_LML * abs(lml)
    assert np.linalg.norm(r["alpha"] - alpha) <= TOL_ALPHA * np.linalg.norm(alpha)
    assert np.abs(dth - ref).max() <= TOL_GRAD * np.abs(ref).max()
    tol = KL.LD(max(10.0 * floor, 256.0) * EPS) * ex["dtheta_cond"]
    assert KL.grad_ok(dth, ex["dtheta"], tol), "dtheta per entry"


@pytest.mark.parametrize("variant,shape", CASES, ids=IDS)
def test_fused_calls(variant, shape, ctx):
    c = OS.make_fused_case(variant, shape)
    for label, specs, X, Xs in KL.fused_exprs(c):
        tag = OS.case_id(variant, shape) + "-" + label
        ctx.set_data(X, c["Y"])
        info, r = ctx.exact_inference_sum(specs, c["noise"])
        assert info == 0
        ex = KL.exact(specs, X, c["Y"], c["noise"])
        _check_fused(tag, r, ex, OS.fp64_floor(specs, X, c["Y"], c["noise"], ex))
        assert abs(r["dnoise"] - float(ex["dnoise"])) <= TOL_GRAD * abs(float(ex["dnoise"]))
        scale = float(np.max(KL.Kdiag(specs, np.vstack([X, Xs]))))
        Kd = ctx.fetch(L.FETCH_K)
        assert KL.k_ok(Kd, KL.K(specs, X), scale) and np.array_equal(Kd, Kd.T)
        mu_ld, var_ld, cov_ld = KL.predict(specs, X, ex, Xs)
        mu, var = ctx.predict_sum(specs, Xs)
        _, cov = ctx.predict_sum(specs, Xs, full_cov=True)
        print("    prediction: mu %.2e var %.2e cov %.2e" % (np.abs(mu - KL.f64(mu_ld)).max(), np.abs(var - KL.f64(var_ld)).max(),
                                                             np.abs(cov - KL.f64(cov_ld)).max()))
        assert np.abs(mu - KL.f64(mu_ld)).max() <= TOL_PRED and np.abs(var - KL.f64(var_ld)).max() <= TOL_PRED
        assert np.abs(cov - KL.f64(cov_ld)).max() <= TOL_PRED


# ---- (c) one shape each ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_shape():
    """the long-double answers of the one-shape runs, computed once per (variant, shape, expression) and shared"""
    cache = {}

    def get(variant, shape, label, nu=None):
        key = (variant[0], tuple(shape), label, nu)
        if key not in cache:
            c = OS.make_fused_case(variant, shape)
            specs, X, Xs = [(s, x, xs) for lb, s, x, xs in KL.fused_exprs(c) if lb == label][0]
            ex = KL.exact(specs, X, c["Y"], 0.0 if nu else c["noise"], nu)
            cache[key] = (c, specs, X, Xs, ex)
        return cache[key]
    return get


@pytest.mark.parametrize("variant", OS.VARIANTS, ids=VIDS)
def test_student_t_process(variant, ctx, one_shape):
    c, specs, X, Xs, ex = one_shape(variant, KL.STUDENTT_SHAPE, "plus_white", NU)
    ctx.set_data(X, c["Y"])
    info, r = ctx.exact_studentt_sum(specs, NU)
    assert info == 0
    _check_fused(variant[0] + "-studentt", r, ex, OS.fp64_floor(specs, X, c["Y"], 0.0, ex, NU))


@pytest.mark.parametrize("variant", OS.VARIANTS, ids=VIDS)
def test_predict_one_new_point(variant, ctx, one_shape):
    """M = 1 at 63 / 1 / 2 / 1: a one-column block of the cross-covariance, mean, variance and the 1 x 1 full covariance"""
    c, specs, X, Xs, ex = one_shape(variant, (63, 1, 2, 1), "times_rbf")
    assert Xs.shape[0] == 1
    ctx.set_data(X, c["Y"])
    info, r = ctx.exact_inference_sum(specs, c["noise"])
    assert info == 0
    mu_ld, var_ld, cov_ld = KL.predict(specs, X, ex, Xs)
    mu, var = ctx.predict_sum(specs, Xs)
    _, cov = ctx.predict_sum(specs, Xs, full_cov=True)
    assert np.abs(mu - KL.f64(mu_ld)).max() <= TOL_PRED and np.abs(var - KL.f64(var_ld)).max() <= TOL_PRED
    assert cov.shape == (1, 1) and np.abs(cov - KL.f64(cov_ld)).max() <= TOL_PRED


@pytest.mark.parametrize("variant", OS.VARIANTS, ids=VIDS)
def test_predictive_gradients_against_the_restatement(variant, ctx, one_shape):
    """dmu / dX* and dvar / dX* (core/gp.py:418-474) at the subset shape (the kind on column 2, next to a White), M = 130:
    dmu_d = gradients_X(1 alpha_d^T, X*, X), dvar = gradients_X(-2 K(X*, X) Ky^-1, X*, X) in long double (Kdiag is constant)"""
    c, specs, X, Xs, ex = one_shape(variant, KL.SUBSET_SHAPE, "plus_white")
    ctx.set_data(X, c["Y"])
    info, r = ctx.exact_inference_sum(specs, c["noise"])
    assert info == 0
    dmu, dvar = ctx.predictive_gradients(specs, Xs)
    M, D = Xs.shape
    assert dmu.shape == (M, D, c["Y"].shape[1]) and dvar.shape == (M, D)
    for d in range(c["Y"].shape[1]):
        ref = KL.f64(KL.gradients_X(specs, np.ones((M, 1), dtype=KL.LD) * ex["alpha"][:, d][None, :], Xs, X)[0])
        assert np.abs(dmu[:, :, d] - ref).max() <= TOL_GRAD * np.abs(ref).max()
    a2 = -2 * KL.matmul(KL.K(specs, Xs, X), ex["Ki"])
    ref = KL.f64(KL.gradients_X(specs, a2, Xs, X)[0])
    assert np.abs(dvar - ref).max() <= TOL_GRAD * np.abs(ref).max()
    col = OS.fused_column(KL.SUBSET_SHAPE)
    assert np.all(np.delete(dmu, col, axis=1) == 0) and np.all(np.delete(dvar, col, axis=1) == 0)     # one active column


@pytest.mark.parametrize("variant", OS.VARIANTS, ids=VIDS)
def test_covariance_between_points(variant, ctx, one_shape):
    c, specs, X, Xs, ex = one_shape(variant, (65, 63, 33, 1), "times_rbf")
    ctx.set_data(X, c["Y"])
    info, r = ctx.exact_inference_sum(specs, c["noise"])
    assert info == 0
    X1, X2 = Xs[:40], Xs[21:]
    T1, T2 = KL.solve_lower(ex["L"], KL.K(specs, X, X1)), KL.solve_lower(ex["L"], KL.K(specs, X, X2))
    ref = KL.f64(KL.K(specs, X1, X2) - KL.matmul(T1.T, T2))
    got = ctx.covariance_between_points(specs, X1, X2)
    assert got.shape == ref.shape and np.abs(got - ref).max() <= TOL_PRED


@pytest.mark.parametrize("variant", OS.VARIANTS, ids=VIDS)
def test_laplace_session_kernel_gradients(variant, ctx):
    """laplace_gradients reduces the session's resident dL_dK against every part's dK/dtheta: the device's gradients against
    the long-double contraction of the dL_dK it holds (fetched), entry by entry as in (a)"""
    c = OS.make_fused_case(variant, (65, 63, 33, 1))
    _, specs, X, _ = KL.fused_exprs(c)[2]                            # times an RBF
    rng = np.random.default_rng(11)
    N = X.shape[0]
    W, b, Ki_f, s = rng.uniform(0.1, 0.5, N), rng.standard_normal(N), rng.standard_normal(N), 0.1 * rng.standard_normal(N)
    ctx.set_data(X, c["Y"])
    ctx.laplace_begin(specs)
    info = ctx.laplace_newton(W, b)[0]
    assert info == 0
    info = ctx.laplace_finish(W)[0]
    assert info == 0
    dth = ctx.laplace_gradients(Ki_f, s)
    G = ctx.fetch(L.FETCH_DLDK)
    assert np.array_equal(G, G.T) and np.isfinite(G).all()
    val, cond = KL.dtheta(specs, G, X)
    fig = KL.grad_figure(dth, val, cond)
    print("FIG %s laplace dtheta %.2f eps x cond" % (variant[0], fig))
    assert KL.grad_ok(dth, val, KL.grad_tol(val, KL.dtheta(specs, G, X, **F64)[0], cond))
    Xs = np.hstack([c["X2"], c["E2"]])                               # laplace_predict: the mean is K(X*, X) Ki_f
    mu, var = ctx.laplace_predict(specs, Xs, Ki_f)
    ref = KL.f64(KL.matmul(KL.K(specs, X, Xs).T, np.asarray(Ki_f, KL.LD)[:, None]))
    assert np.abs(mu - ref).max() <= TOL_PRED * max(1.0, np.abs(ref).max()) and np.isfinite(var).all()


# ---- (d) the reference's fixtures --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", OS.INFERENCE_FIXTURES)
def test_golden_through_the_c_abi(name):
    g = OS.load_fixture(name)
    specs = g["specs"]
    c = L.Context(0)
    try:
        c.set_data(g["X"], g["Y"])
        if g["nu"] is None:
            info, r = c.exact_inference_sum(specs, g["noise"], want_diag=True)
            assert abs(r["dnoise"] - g["dnoise"]) <= TOL_GRAD * abs(g["dnoise"])
        else:
            info, r = c.exact_studentt_sum(specs, g["nu"])
        assert info == 0
        print(name, "lml %.2e alpha %.2e dtheta %.2e" % (abs(r["lml"] - g["lml"]) / abs(g["lml"]),
                                                       np.linalg.norm(r["alpha"] - g["alpha"]) / np.linalg.norm(g["alpha"]),
                                                       np.abs(r["dtheta"] - g["dtheta"]).max() / np.abs(g["dtheta"]).max()))
        assert abs(r["lml"] - g["lml"]) <= TOL_LML * abs(g["lml"])
        assert np.linalg.norm(r["alpha"] - g["alpha"]) <= TOL_ALPHA * np.linalg.norm(g["alpha"])
        assert np.abs(r["dtheta"] - g["dtheta"]).max() <= TOL_GRAD * np.abs(g["dtheta"]).max()
        K = c.fetch(L.FETCH_K)
        var = max(float(s[2][0]) for s in specs)
        assert np.abs(K[0] - g["K_row0"]).max() <= TOL_K * var
        if g["nu"] is None:
            mu, v = c.predict_sum(specs, g["Xs"])
            assert np.abs(mu - g["pred_mu"]).max() <= TOL_PRED and np.abs(v - g["pred_var"]).max() <= TOL_PRED
            _, cov = c.predict_sum(specs, g["Xs"], full_cov=True)
            assert np.abs(cov - g["pred_cov"]).max() <= TOL_PRED
    finally:
        c.close()


@pytest.mark.parametrize("name", [n for n in OS.INFERENCE_FIXTURES if not n.startswith("studentt")])
def test_golden_through_gpregression(name):
    g = OS.load_fixture(name)
    k = expression(g["specs"])
    m = gpy_amd.GPRegression(g["X"], g["Y"], k, noise_var=float(g["noise"]))
    assert abs(m.log_likelihood() - g["lml"]) <= TOL_LML * abs(g["lml"])
    gref = np.concatenate([g["dtheta"], [g["dnoise"]]])
    assert np.abs(m.gradient - gref).max() <= TOL_GRAD * np.abs(gref).max()
    mu, var = m.predict_noiseless(g["Xs"])
    assert np.abs(mu - g["pred_mu"]).max() <= TOL_PRED and np.abs(var - g["pred_var"]).max() <= TOL_PRED
    gx = k.gradients_X(g["G"], g["X"])
    assert np.abs(gx - g["gradX"]).max() <= TOL_GRAD * np.abs(g["gradX"]).max()
    gx2 = k.gradients_X(g["G2"], g["X"], g["Xs"])
    assert np.abs(gx2 - g["gradX2"]).max() <= TOL_GRAD * np.abs(g["gradX2"]).max()


def test_golden_kernels_with_ard():
    g = OS.load_fixture("kernels_ard_n90_m70_d3")
    X, X2 = g["X"], g["X2"]
    for spec in g["specs"]:
        kind, k = spec[0], kernel(spec)
        assert np.abs(k.K(X) - g[kind + "_K"]).max() <= TOL_K * spec[2][0]
        assert np.abs(k.K(X, X2) - g[kind + "_Kx"]).max() <= TOL_K * spec[2][0]
        assert np.all(k.Kdiag(X) == spec[2][0])
        for G, B, key in ((g["G"], None, ""), (g["G2"], X2, "_x")):
            k.update_gradients_full(G, X, B)
            ref = g[kind + "_dtheta" + key]
            assert k.gradient.shape == ref.shape and np.abs(k.gradient - ref).max() <= TOL_GRAD * np.abs(ref).max(), (kind, key)
        assert np.abs(k.gradients_X(g["G"], X) - g[kind + "_gradX"]).max() <= TOL_GRAD * np.abs(g[kind + "_gradX"]).max()
        assert np.abs(k.gradients_X(g["G2"], X, X2) - g[kind + "_gradX2"]).max() <= TOL_GRAD * np.abs(g[kind + "_gradX2"]).max()


# ---- (e) determinism, the example, the models ------------------------------------------------------------------------------
def test_a_fused_case_twice_in_fresh_contexts_gives_identical_bytes():
    c = OS.make_fused_case(("eqc_ard", "expquadcosine", 1), (129, 130, 5, 4))
    _, specs, X, Xs = KL.fused_exprs(c)[2]
    runs = []
    for _ in range(2):
        cx = L.Context(0)
        try:
            cx.set_data(X, c["Y"])
            info, r = cx.exact_inference_sum(specs, c["noise"], want_diag=True)
            assert info == 0
            mu, var = cx.predict_sum(specs, Xs)
            runs.append([np.float64(r["lml"]), np.float64(r["dnoise"]), r["alpha"], r["dtheta"], r["diag_dL_dK"],
                         cx.fetch(L.FETCH_K), mu, var])
        finally:
            cx.close()
    for a, b in zip(*runs):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()


def _example():
    path = os.path.join(os.path.dirname(HERE), "examples", "spectral_mixture_regression.py")
    spec = importlib.util.spec_from_file_location("spectral_mixture_regression", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_example_fit_reaches_the_reference_optimum():
    """the example's model on the toy fixture's 120 points: the start matches the reference's log marginal, `optimize()` over the
    same number of L-BFGS-B iterations ends at least at the reference's value minus 1e-3 of its size (the tolerance of the other
    toy-optimisation tests), and the two learned periods are the signal's (1 and sqrt 7)"""
    t = OS.load_fixture("toy_sm_optimize")
    ex = _example()
    assert np.array_equal(ex.THETA0, t["theta0"])
    m = ex.build_model(t["X"], t["Y"])
    l0 = m.log_likelihood()
    assert abs(l0 - float(t["lml_start"])) <= TOL_LML * abs(float(t["lml_start"]))
    m.optimize(max_iters=int(t["maxiter"]))
    l1 = m.log_likelihood()
    periods = ex.learned_periods(m.kern)
    print("toy: log marginal %.6f -> %.6f (reference %.6f -> %.6f), periods %s" % (l0, l1, float(t["lml_start"]), float(t["lml_end"]),
                                                                                  periods))
    assert l1 > l0
    assert l1 >= float(t["lml_end"]) - 1e-3 * abs(float(t["lml_end"]))
    assert np.abs(np.sort(periods)[:2] - [1.0, np.sqrt(7.0)]).max() <= 0.02


def test_a_sum_of_two_fits_and_predicts_through_the_models():
    rng = np.random.default_rng(2)
    X = np.sort(rng.uniform(-3.0, 3.0, (60, 1)), axis=0)
    f = np.sin(2 * np.pi * X / 1.5) + 0.5 * np.sin(2 * np.pi * X / 0.7)
    Y = f + 0.1 * rng.standard_normal(X.shape)
    Xs = np.linspace(-3.0, 3.0, 17)[:, None]
    make = lambda: gpy_amd.kern.ExpQuadCosine(1, lengthscale=10.0, period=0.15) + gpy_amd.kern.ExpQuadCosine(1, lengthscale=8.0, period=0.09)
    m = gpy_amd.GPRegression(X, Y, make())
    l0 = m.log_likelihood()
    m.optimize(max_iters=30)
    assert m.log_likelihood() > l0
    mu, var = m.predict(Xs)
    assert mu.shape == (17, 1) and np.isfinite(mu).all() and np.all(var > 0)
    for inf in (gpy_amd.Laplace(), gpy_amd.EP()):
        mc = gpy_amd.GPClassification(X, (f > 0).astype(float), kernel=make(), inference_method=inf)
        l0 = mc.log_likelihood()
        mc.optimize(max_iters=10)
        assert np.isfinite(mc.log_likelihood()) and mc.log_likelihood() >= l0 - 1e-6 * abs(l0)
        p, _ = mc.predict(Xs)
        assert p.shape == (17, 1) and np.all((p >= 0) & (p <= 1))
        acc = float(np.mean((mc.predict(X)[0] > 0.5) == (f > 0)))
        assert acc >= 0.8, acc
