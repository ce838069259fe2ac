"""CPU: the restatement of Cosine, Sinc and ExpQuadCosine (tests/osc_ld.py, C-ABI kinds 12 / 13 / 14) against the fixtures from
the reference's own code (tests/golden/osc) and against central differences; what the host classes send to the device for
them (a recording context in the manner of tests/test_host_routing.py) and how they install gradients; the refusals of the
sparse, grid, SVGP, PEP / FITC and uncertain-input paths by class name; and the conditions under which the GPU sweep
(tests/test_gpu_osc.py) judges the device:

    the kinds are positive definite over one input dimension only, so every inference-level case puts the kind on one active
    column, alone, next to a White or times an RBF on two further columns; Ky = K + 0.1 x scale I of every such case factors in
    long double and has cond_2 <= 1e5; the fp64 evaluation of the restatement's K lies within 1e-14 x scale of the long-double
    one on every case of the sweep: ten times inside the device's bound of 1e-13 x scale, which therefore tests the device and
    not the inputs."""
import numpy as np
import pytest

import gpy_amd
from gpy_amd import _lib
from gpy_amd.inference import ExactGaussianInference
from gpy_amd.sparse import VarDTC

import kern_ld as KL
import osc_ld as OS
from test_host_routing import Rec, RecSparse, Recorded, part, rec  # noqa: F401  (rec: the recording-context fixture)

needs_ld = pytest.mark.skipif(not KL.HAVE_LD, reason="np.longdouble is not an extended format on this host")
CASES = [(v, s) for v in OS.VARIANTS for s in OS.SHAPES]
IDS = [OS.case_id(v, s) for v, s in CASES]
F64 = dict(dt=np.float64)


def test_the_ids_are_12_13_14():
    assert [_lib.KIND_IDS[k] for k in OS.KINDS] == [12, 13, 14] and OS.KIND_IDS == {k: _lib.KIND_IDS[k] for k in OS.KINDS}
    from gpy_amd.kern import EXACT_ONLY_KINDS, KERNEL_CLASSES
    for kind in OS.KINDS:
        assert kind in EXACT_ONLY_KINDS and KERNEL_CLASSES[kind].__name__ == OS.CLASS_NAMES[kind]
        assert KERNEL_CLASSES[kind].kind == kind and issubclass(KERNEL_CLASSES[kind], gpy_amd.Stationary)
    assert gpy_amd.kern.Cosine is gpy_amd.Cosine and gpy_amd.kern.Sinc is gpy_amd.Sinc
    assert gpy_amd.kern.ExpQuadCosine is gpy_amd.ExpQuadCosine


# ---- the fp64 restatement meets every fixture --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", OS.INFERENCE_FIXTURES)
def test_fp64_restatement_meets_the_inference_fixtures(name):
    g = OS.load_fixture(name)
    specs, X, Y = g["specs"], g["X"], g["Y"]
    ex = KL.exact(specs, X, Y, float(g["noise"]), g["nu"], max_n=256, **F64)
    var = max(float(s[2][0]) for s in specs)
    print(name, "lml %.2e alpha %.2e dtheta %.2e" % (abs(ex["lml"] - g["lml"]) / abs(g["lml"]),
                                                   np.linalg.norm(ex["alpha"] - g["alpha"]) / np.linalg.norm(g["alpha"]),
                                                   np.abs(ex["dtheta"] - g["dtheta"]).max() / np.abs(g["dtheta"]).max()))
    assert abs(ex["lml"] - g["lml"]) <= OS.TOL_LML * abs(g["lml"])
    assert np.linalg.norm(ex["alpha"] - g["alpha"]) <= OS.TOL_ALPHA * np.linalg.norm(g["alpha"])
    assert np.abs(ex["dtheta"] - g["dtheta"]).max() <= OS.TOL_GRAD * np.abs(g["dtheta"]).max()
    assert np.abs(KL.K(specs, X, **F64)[0] - g["K_row0"]).max() <= OS.TOL_K * var
    if g["nu"] is None:
        assert abs(ex["dnoise"] - g["dnoise"]) <= OS.TOL_GRAD * abs(g["dnoise"])
        mu, v, cov = KL.predict(specs, X, ex, g["Xs"], **F64)
        assert np.abs(mu - g["pred_mu"]).max() <= OS.TOL_PRED and np.abs(v - g["pred_var"]).max() <= OS.TOL_PRED
        assert np.abs(cov - g["pred_cov"]).max() <= OS.TOL_PRED
    gx = KL.gradients_X(specs, g["G"], X, **F64)[0]
    gx2 = KL.gradients_X(specs, g["G2"], X, g["Xs"], **F64)[0]
    assert np.abs(gx - g["gradX"]).max() <= OS.TOL_GRAD * np.abs(g["gradX"]).max()
    assert np.abs(gx2 - g["gradX2"]).max() <= OS.TOL_GRAD * np.abs(g["gradX2"]).max()


def test_fp64_restatement_meets_the_kernel_fixture():
    g = OS.load_fixture("kernels_ard_n90_m70_d3")
    X, X2 = g["X"], g["X2"]
    for spec in g["specs"]:
        kind, specs = spec[0], [spec]
        assert np.abs(KL.K(specs, X, **F64) - g[kind + "_K"]).max() <= OS.TOL_K * spec[2][0]
        assert np.abs(KL.K(specs, X, X2, **F64) - g[kind + "_Kx"]).max() <= OS.TOL_K * spec[2][0]
        assert np.all(KL.Kdiag(specs, X, **F64) == spec[2][0])
        for G, B, key in ((g["G"], None, ""), (g["G2"], X2, "_x")):
            dth = KL.dtheta(specs, G, X, B, **F64)[0]
            ref = g[kind + "_dtheta" + key]
            assert dth.shape == ref.shape and np.abs(dth - ref).max() <= OS.TOL_GRAD * np.abs(ref).max(), (kind, key)
        gx, gx2 = KL.gradients_X(specs, g["G"], X, **F64)[0], KL.gradients_X(specs, g["G2"], X, X2, **F64)[0]
        assert np.abs(gx - g[kind + "_gradX"]).max() <= OS.TOL_GRAD * np.abs(g[kind + "_gradX"]).max()
        assert np.abs(gx2 - g[kind + "_gradX2"]).max() <= OS.TOL_GRAD * np.abs(g[kind + "_gradX2"]).max()


def test_fp64_restatement_meets_the_toy_fixture():
    t = OS.load_fixture("toy_sm_optimize")
    for th, key in ((t["theta0"], "lml_start"), (t["theta_end"], "lml_end")):
        ex = KL.exact(OS.toy_specs(th), t["X"], t["Y"], float(th[10]), max_n=256, **F64)
        assert abs(ex["lml"] - float(t[key])) <= 1e-9 * abs(float(t[key])), key
    assert float(t["lml_end"]) > float(t["lml_start"])
    periods = np.sort(t["theta_end"][1:9:3] * t["theta_end"][2:9:3])[:2]          # in input units: lengthscale x period
    assert np.abs(periods - [1.0, np.sqrt(7.0)]).max() <= 0.02


# ---- long double and fp64 against central differences ------------------------------------------------------------------------
@needs_ld
@pytest.mark.parametrize("variant", OS.VARIANTS, ids=lambda v: v[0])
@pytest.mark.parametrize("dt,h,tol", [(KL.LD, 1e-7, 1e-10), (np.float64, 1e-5, 1e-7)], ids=["long_double", "fp64"])
def test_derivatives_agree_with_central_differences(variant, dt, h, tol):
    """every dK/dtheta_k and dK/dX_iq of a 6 x 5 x 3 case against (K(+h) - K(-h)) / 2h in the same type; the coincident pair
    is left out of the lengthscale and X derivatives (`_inv_dist` sets them to 0 there, the differences see the one-sided
    slope)"""
    rng = np.random.default_rng(7)
    N, M, D = 6, 5, 3
    X, X2 = rng.standard_normal((N, D)), rng.standard_normal((M, D))
    X2[0] = X[N - 1]
    th = OS._theta(variant[1], variant[2], D, rng)
    th[1:1 + (D if variant[2] else 1)] /= np.sqrt(D)                             # a few oscillations across the points
    mask = np.ones((N, M), dtype=bool)
    mask[N - 1, 0] = False
    Kof = lambda t, A: KL.K([(variant[1], variant[2], t, np.arange(D), 0)], A, X2, dt=dt)
    lf = KL.leaves([(variant[1], variant[2], th, np.arange(D), 0)], X, X2, dt)[0]
    scale = th[0]
    for k in range(lf.np_):
        e = np.zeros(th.size, dtype=dt)
        e[k] = dt(h) * dt(th[k])
        fd = (Kof(np.asarray(th, dt) + e, X) - Kof(np.asarray(th, dt) - e, X)) / (2 * e[k])
        err = np.abs(fd - lf.dparam(k))[mask].max() * dt(th[k])
        assert err <= tol * scale, (k, float(err))
    for q in range(D):
        e = np.zeros((N, D), dtype=dt)
        e[:, q] = dt(h)
        fd = (Kof(th, np.asarray(X, dt) + e) - Kof(th, np.asarray(X, dt) - e)) / (2 * dt(h))
        err = np.abs(fd - lf.dx(q))[mask].max()
        assert err <= tol * scale * float(np.abs(lf.dx(q)).max() / scale + 1), (q, float(err))


@needs_ld
@pytest.mark.parametrize("kind", OS.KINDS)
def test_coincident_points_contribute_nothing_to_a_gradient(kind):
    c = OS.make_case((kind, kind, 1), (65, 63, 33, 1))
    specs = [c["spec"]]
    G2 = np.zeros((65, 63))
    G2[64, 0] = 1.5                                               # X2[0] == X[64]
    G = np.zeros((65, 65))
    G[0, 1], G[1, 0], G[5, 5] = 0.7, -0.2, 1.0                    # X[1] == X[0]
    for Gm, B in ((G2, c["X2"]), (G, None)):
        val, _ = KL.dtheta(specs, Gm, c["X"], B)
        assert np.all(val[1:] == 0) and val[0] != 0               # lengthscales and the period: r = 0
        assert np.all(KL.gradients_X(specs, Gm, c["X"], B)[0] == 0)
    assert np.all(np.diag(KL.K(specs, c["X"])) == KL.LD(c["spec"][2][0]))        # the diagonal is the variance, exactly


# ---- the conditions of the GPU sweep --------------------------------------------------------------------------------------
def test_the_kinds_are_positive_definite_over_one_dimension_only():
    """cos |x - x'| over the four corners of a square of side pi / sqrt 2 has a negative eigenvalue; over one column every
    sweep kind is positive semi-definite"""
    a = np.pi / np.sqrt(2.0)
    sq = np.array([[0.0, 0.0], [a, 0.0], [0.0, a], [a, a]])
    spec = ("cosine", 0, np.array([1.0, 1.0]), np.arange(2), 0)
    assert np.linalg.eigvalsh(KL.K([spec], sq, **F64)).min() < -0.1
    x = np.random.default_rng(3).standard_normal((40, 1))
    for kind, th in (("cosine", [1.0, 0.7]), ("sinc", [1.0, 0.7]), ("expquadcosine", [1.0, 4.0, 0.3])):
        w = np.linalg.eigvalsh(KL.K([(kind, 0, np.array(th), np.arange(1), 0)], x, **F64))
        assert w.min() >= -1e-12 * w.max(), kind


@needs_ld
@pytest.mark.parametrize("variant,shape", CASES, ids=IDS)
def test_the_inference_cases_of_the_sweep_are_well_conditioned(variant, shape):
    c = OS.make_fused_case(variant, shape)
    assert len(c["spec"][3]) == 1                                                 # one active column
    for label, specs, X, Xs in KL.fused_exprs(c):
        scale = float(np.max(KL.Kdiag(specs, np.vstack([X, Xs]))))
        K_ld = KL.K(specs, X)
        Ky = np.array(K_ld)
        n = Ky.shape[0]
        Ky[np.arange(n), np.arange(n)] += KL.LD(c["noise"]) + KL.LD(1e-8)
        KL.cholesky(Ky)                                                           # asserts every pivot > 0
        w = np.linalg.eigvalsh(KL.f64(Ky))
        fig = KL.k_figure(KL.K(specs, X, **F64), K_ld, scale)
        print("%s-%s: cond_2 %.3g, fp64 K %.2f eps x scale" % (OS.case_id(variant, shape), label, w.max() / w.min(), fig))
        assert w.min() > 0 and w.max() / w.min() <= 1e5
        assert KL.k_ok(KL.K(specs, X, **F64), K_ld, scale, tol=1e-14)
        assert KL.k_ok(KL.K(specs, X, Xs, **F64), KL.K(specs, X, Xs), scale, tol=1e-14)


@needs_ld
@pytest.mark.parametrize("variant,shape", CASES, ids=IDS)
def test_the_kernel_cases_of_the_sweep_in_fp64(variant, shape):
    """K of the K-level cases (every column) within 1e-14 x scale, the gradients within 16 eps64 x cond, in fp64; and the
    ExpQuadCosine envelope keeps its mass (asserted inside make_case: median off-diagonal >= 0.1)"""
    c = OS.make_case(variant, shape)
    specs, X, X2 = [c["spec"]], c["X"], c["X2"]
    assert KL.k_ok(KL.K(specs, X, **F64), KL.K(specs, X), c["scale"], tol=1e-14)
    assert KL.k_ok(KL.K(specs, X, X2, **F64), KL.K(specs, X, X2), c["scale"], tol=1e-14)
    fg = KL.grad_figure(KL.dtheta(specs, c["G2"], X, X2, **F64)[0], *KL.dtheta(specs, c["G2"], X, X2))
    fx = KL.grad_figure(KL.gradients_X(specs, c["G"], X, **F64)[0], *KL.gradients_X(specs, c["G"], X))
    print("%s: dtheta %.2f gradients_X %.2f eps x cond" % (OS.case_id(variant, shape), fg, fx))
    assert fg <= 16 and fx <= 16
    if variant[1] == "expquadcosine" and shape[0] >= 2:
        assert OS.envelope_median(c["spec"], X) >= OS.MIN_ENVELOPE
        assert 0.5 <= c["spec"][2][-1] <= 2.0


# ---- what the host classes send to the device ---------------------------------------------------------------------------------
def _data():
    rng = np.random.default_rng(5)
    X = rng.standard_normal((12, 3))
    return X, rng.standard_normal((12, 1)), X[:5] + 0.25


HOST = {
    # name: (kernel, columns of X on the device (None: all), the parts, the parameter names in link order)
    "cosine": (lambda: gpy_amd.Cosine(1, 1.3, 0.7, active_dims=[1]), [1], [part("cosine", 0, [1.3, 0.7], None, 0)]),
    "sinc_ard": (lambda: gpy_amd.Sinc(2, 0.9, [0.7, 1.1], ARD=True, active_dims=[2, 0]), [2, 0],
                 [part("sinc", 1, [0.9, 0.7, 1.1], None, 0)]),
    "eqc": (lambda: gpy_amd.ExpQuadCosine(1, 1.1, 6.0, 0.25, active_dims=[0]), [0],
            [part("expquadcosine", 0, [1.1, 6.0, 0.25], None, 0)]),
    "eqc+eqc+bias": (lambda: gpy_amd.ExpQuadCosine(1, 1.1, 6.0, 0.25, active_dims=[0])
                     + gpy_amd.ExpQuadCosine(1, 0.4, 9.0, 0.5, active_dims=[0]) + gpy_amd.Bias(3, 0.3), None,
                     [part("expquadcosine", 0, [1.1, 6.0, 0.25], (0,), 0), part("expquadcosine", 0, [0.4, 9.0, 0.5], (0,), 0),
                      part("bias", 0, [0.3], (0, 1, 2), 0)]),
    "rbf*cosine": (lambda: gpy_amd.RBF(2, 1.3, 0.7, active_dims=[0, 2]) * gpy_amd.Cosine(1, 0.8, 0.4, active_dims=[1]), None,
                   [part("rbf", 0, [1.3, 0.7], (0, 2), 1), part("cosine", 0, [0.8, 0.4], (1,), 1)]),
}


@pytest.mark.parametrize("name", list(HOST))
def test_host_classes_emit_the_parts_and_install_gradients(rec, name):  # noqa: F811
    make, cols, parts = HOST[name]
    X, Y, Xs = _data()
    k = make()
    post, lml, grads = ExactGaussianInference().inference(k, X, gpy_amd.Gaussian(0.1), Y)
    ctx, = rec.made
    assert np.array_equal(ctx.X, X if cols is None else X[:, cols])
    assert ctx.log == [("exact_inference_sum", parts)]
    assert grads["dL_dK"].matches_kernel(k)
    k.update_gradients_full(grads["dL_dK"], X)                     # the recording context answers dtheta = 1, 2, 3, ...
    assert np.array_equal(k.gradient, np.arange(1.0, 1.0 + k.size))
    i = 1.0
    for leaf in k.leaves():                                        # the reference's parameter order: variance, lengthscale, period
        names = ["variance", "lengthscale"] + (["period"] if isinstance(leaf, gpy_amd.ExpQuadCosine) else [])
        if isinstance(leaf, gpy_amd.Bias):
            names = ["variance"]
        assert [p.name for p in leaf.parameters] == names
        for n in names:
            g = np.atleast_1d(getattr(leaf, n).gradient)
            assert np.array_equal(g, np.arange(i, i + g.size)), (name, n)
            i += g.size
    post._raw_predict(k, Xs, X)
    assert ctx.log[-1] == ("predict_sum", parts)


def test_expquadcosine_follows_the_reference_signature():
    k = gpy_amd.ExpQuadCosine(2, variance=1.5, lengthscale=[2.0, 3.0], period=0.4, ARD=True, active_dims=[1, 2])
    assert k.name == "ExpQuadCosine" and gpy_amd.Cosine(1).name == "Cosine" and gpy_amd.Sinc(1).name == "Sinc"
    assert np.array_equal(k._theta(), [1.5, 2.0, 3.0, 0.4]) and float(gpy_amd.ExpQuadCosine(1).period.values[0]) == 1.0
    d = k.to_dict()
    assert d["class"] == "GPy.kern.ExpQuadCosine" and d["period"] == [0.4] and d["lengthscale"] == [2.0, 3.0]
    X = np.zeros((4, 3))
    k.period.gradient = 7.0
    k.update_gradients_diag(np.ones(4), X)                         # stationary.py:711-713
    assert k.period.gradient == 0.0 and float(np.ravel(k.variance.gradient)[0]) == 4.0
    k.period.gradient = 7.0
    k.reset_gradients()
    assert k.period.gradient == 0.0
    assert np.array_equal(k.gradients_X_diag(np.ones(4), X), np.zeros((4, 3)))


# ---- the refusals name the class -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", OS.KINDS)
def test_sparse_grid_svgp_pep_and_psi_refuse_by_class_name(rec, kind):  # noqa: F811
    cls = getattr(gpy_amd, OS.CLASS_NAMES[kind])
    name = OS.CLASS_NAMES[kind]
    X, Y, _ = _data()
    Z, lik = X[::3].copy(), gpy_amd.Gaussian(0.1)
    msg = "the MI355X sparse path does not evaluate %s kernels" % name
    for k in (cls(3), gpy_amd.RBF(2, active_dims=[0, 1]) * cls(1, active_dims=[2]), gpy_amd.RBF(3) + cls(1, active_dims=[0])):
        with pytest.raises(NotImplementedError, match=msg):
            VarDTC().inference(k, X, Z, lik, Y)
    for inf in (gpy_amd.FITC(), gpy_amd.PEP(0.5)):
        with pytest.raises(NotImplementedError, match=msg):
            inf.inference(cls(3), X, Z, lik, Y)
    with pytest.raises(NotImplementedError, match=r"\(%s\) has no psi-statistics" % name):     # uncertain inputs
        VarDTC().inference(cls(3), gpy_amd.NormalPosterior(X, np.full(X.shape, 0.1)), Z, lik, Y)
    with pytest.raises(NotImplementedError, match=msg):
        gpy_amd.SparseGPRegression(X, Y, kernel=cls(3), num_inducing=4)
    M = Z.shape[0]
    from gpy_amd.svgp import SVGP as SVGPInference
    with pytest.raises(NotImplementedError, match=msg):
        SVGPInference().inference(np.zeros((M, 1)), np.zeros((M * (M + 1) // 2, 1)), cls(3), X, Z, lik, Y)
    from gpy_amd.grid import GridContext
    with pytest.raises(NotImplementedError, match="grid path evaluates RBF / Matern / Exponential kernels, not %s" % name):
        GridContext.exact_inference(None, kind, False, cls(3)._theta(), 0.1)
    assert all(c.log == [] for c in rec.made)                         # nothing reached a device context
