"""CPU: grid regression (GaussianGridInference, GpGrid, GPRegressionGrid) without a device.

1. The long-double restatement tests/kron_ld.py against fixtures of the reference's OWN `GaussianGridInference.inference`
   (tests/golden/kron/*.npz, written by tools/make_golden_kron.py through oracle/ref_loader.py): D = 1, 2, 3 and 4, a dimension
   of size 1, unequal sizes, ARD lengthscales; integer-valued coordinates.  The restatement takes the reference's eigenvectors and
   eigenvalues as given.  Bound: 1000 eps64 kappa, kappa = (max V + noise) / (min V + noise) the condition of Ky: the reference
   works in float64 from an `np.linalg.eig` whose backward error is O(G eps ||K_d||), which alpha sees amplified by kappa.
2. The restatement against the DENSE restatement (Cholesky of the N x N covariance, long double) on NON-integer grids, where the
   reference itself is wrong (hash order of `set`): same bound, the eigenvectors being float64 `numpy.linalg.eigh` of float64 K_d.
3. `gpy_amd.kern.GridRBF`: the derivative factors against central differences of the Kronecker product of its `K`.
4. The host classes over a recording context that answers from the float64 restatement: call order, what is uploaded, gradient
   installation, lazy `alpha`, every refusal by message, the model against the fixtures, pickling.
5. `_lib.KRON_ABI` against the prototypes of include/mi355gp_kron.h."""
import inspect
import os
import pickle

import numpy as np
import pytest

import gpy_amd
from gpy_amd import _lib
from gpy_amd import kron as K

import kron_ld as KR
from test_abi import _prototypes, _type_class

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = KR.LD
needs_ld = pytest.mark.skipif(not KR.HAVE_LD, reason="np.longdouble is not an extended format on this host")
EPS = np.finfo(np.float64).eps


def kappa(lams, noise):
    V = KR.kron_vec(lams, np.float64)
    return float((V.max() + noise) / (V.min() + noise))


def fixture_restated(g, dt=LD):
    """the restatement on a fixture's inputs, from the reference's Q and lam: dict(alpha, lml, grad (D + 2), mu, var)"""
    xg = [np.unique(g["X"][:, d]) for d in range(g["X"].shape[1])]
    D = len(xg)
    ls = g["lengthscale"] if g["lengthscale"].size == D else np.full(D, g["lengthscale"][0])
    _, factors = KR.grid_factors(xg, g["variance"], ls, dt)
    gammas = KR.gammas_of(g["Qs"], factors, dt)
    noise = dt(float(g["noise"])) + dt(1e-8)
    r = KR.evaluate(g["Qs"], g["lams"], g["Y"], noise, factors, gammas, dt)
    kx = KR.cross_blocks(xg, g["Xs"], g["variance"], ls, dt)
    bx = [np.dot(k, np.asarray(Q, dtype=dt)) for k, Q in zip(kx, g["Qs"])]
    mu, red = KR.predict(r["alpha"], g["lams"], kx, bx, float(g["noise"]), dt)
    return dict(alpha=r["alpha"].reshape(-1, 1), lml=KR.lml_of(r, g["X"].shape[0], dt), grad=KR.grad_of(r, dt), mu=mu.reshape(-1, 1),
                var=(dt(float(g["variance"])) - red).reshape(-1, 1), V=r["V"])


def fixture_figures(g, got):
    """rel_err of (alpha, lml, grad, mu, var) against the fixture"""
    ref = dict(alpha=g["alpha"], lml=g["lml"], grad=np.concatenate([g["dL_dLen"], [g["dL_dVar"]], [g["dL_dthetaL"]]]),
               mu=g["pred_mu"], var=g["pred_var"])
    return dict((q, KR.rel_err(np.asarray(got[q]).reshape(np.shape(ref[q])), ref[q])) for q in ref)


def test_the_fixtures_are_the_six_of_the_issue():
    assert len(KR.FIXTURES) == 6 and sorted(os.listdir(KR.GOLDEN)) == sorted(n + ".npz" for n in KR.FIXTURES)
    Gs = [tuple(int(v) for v in KR.load_fixture(n)["G"]) for n in KR.FIXTURES]
    assert sorted(len(G) for G in Gs) == [1, 2, 2, 3, 3, 4]
    assert any(1 in G for G in Gs) and (5, 4, 3) in Gs
    for n in KR.FIXTURES:
        g = KR.load_fixture(n)
        assert np.array_equal(g["X"], np.round(g["X"])) and g["Y"].shape == (g["X"].shape[0], 1)
        assert abs(g["lml"] - g["lml_dense"]) <= 1e-13 * abs(g["lml_dense"])
        assert g["noise"] >= 0.05 * g["variance"] and os.path.getsize(os.path.join(KR.GOLDEN, n + ".npz")) < 64 * 1024


@needs_ld
@pytest.mark.parametrize("name", KR.FIXTURES)
def test_restatement_against_the_reference(name):
    g = KR.load_fixture(name)
    figs = fixture_figures(g, fixture_restated(g))
    tol = 1000 * EPS * kappa(g["lams"], float(g["noise"]))
    print(name, "  ".join("%s %.1e" % kv for kv in figs.items()), "bound %.1e" % tol)
    for q, e in figs.items():
        assert e <= tol, (q, e, tol)
    assert KR.rel_err(KR.kron_vec(g["lams"], np.float64), g["V_kron"]) == 0.0


NONINT = [([0.0, 0.7, 1.1, 2.0],), ([0.0, 0.7, 1.1, 2.0, 2.6], [-1.3, 0.2, 0.9]), ([0.1, 0.9, 1.4, 2.2, 3.1, 3.3], [0.0, 0.7, 1.1, 2.0, 2.9], [-0.5, 0.3, 1.2, 1.9]),
          ([0.3, 1.0], [2.5], [0.0, 0.45, 1.3])]


def nonint_case(i):
    xg = [np.array(x) for x in NONINT[i]]
    D = len(xg)
    rng = np.random.default_rng(100 + i)
    X = KR.grid_of(xg)
    Y = np.cos(X.sum(1))[:, None] + 0.2 * rng.standard_normal((X.shape[0], 1))
    ls = 0.8 + 0.9 * rng.random(D)
    Xs = X.min(0) + (X.max(0) - X.min(0)) * rng.random((7, D))
    return xg, X, Y, 1.4, ls, 0.11, Xs


def eig_inputs(xg, variance, ls):
    """float64 K_d, numpy.linalg.eigh of it, and the float64 derivative factors and gammas: what the host hands the device"""
    Kds, factors = KR.grid_factors(xg, variance, ls, np.float64)
    e = [np.linalg.eigh(Kd) for Kd in Kds]
    Qs, lams = [q for _, q in e], [lam for lam, _ in e]
    return Qs, lams, factors, KR.gammas_of(Qs, factors, np.float64)


@needs_ld
@pytest.mark.parametrize("i", range(len(NONINT)))
def test_restatement_against_the_dense_restatement_on_non_integer_grids(i):
    xg, X, Y, variance, ls, noise, Xs = nonint_case(i)
    Qs, lams, factors, gammas = eig_inputs(xg, variance, ls)
    r = KR.evaluate(Qs, lams, Y, noise, factors, gammas, LD)
    kx = KR.cross_blocks(xg, Xs, variance, ls, LD)
    mu, red = KR.predict(r["alpha"], lams, kx, [np.dot(k, Q.astype(LD)) for k, Q in zip(kx, Qs)], noise, LD)
    d = KR.dense(xg, variance, ls, Y, noise, Xs=Xs, dt=LD)
    tol = 1000 * EPS * kappa(lams, noise)
    figs = dict(alpha=KR.rel_err(r["alpha"], d["alpha"]), lml=KR.rel_err(KR.lml_of(r, X.shape[0]), d["lml"]),
                grad=KR.rel_err(KR.grad_of(r), d["grad"]), mu=KR.rel_err(mu, d["mu"]), red=KR.rel_err(red, d["red"]))
    print(i, "  ".join("%s %.1e" % kv for kv in figs.items()), "bound %.1e" % tol)
    for q, e in figs.items():
        assert e <= tol, (q, e, tol)


def test_grid_values_are_sorted_where_set_order_is_not():
    """the first deviation from the reference: hash order of a set of generic reals is not ascending"""
    x = np.array([0.0, 0.7, 1.1, 2.0, 2.6, 3.3])
    assert list(set(x)) != sorted(x)
    assert np.array_equal(K.grid_values(x[:, None])[0], x)


def test_gridrbf_derivative_factors_against_central_differences():
    xg = [np.array([0.0, 0.7, 1.1, 2.0]), np.array([-1.0, 0.4, 0.9]), np.array([0.3, 1.0])]
    D, variance, ls = 3, 1.7, np.array([0.9, 1.3, 0.6])

    def full_K(variance, ls):
        k = gpy_amd.RBF(D, variance=variance, lengthscale=ls, ARD=True).get_one_dimensional_kernel(D)
        out = np.ones((1, 1))
        for d in range(D):
            k.lengthscale = ls[d]
            out = np.kron(out, k.K(xg[d][:, None]))
        return out
    k = gpy_amd.RBF(D, variance=variance, lengthscale=ls, ARD=True).get_one_dimensional_kernel(D)
    assert isinstance(k, gpy_amd.kern.GridRBF) and k.originalDimensions == D
    h = 1e-5
    for t in range(D + 1):
        A = np.ones((1, 1))
        for d in range(D):
            k.lengthscale = ls[d]
            A = np.kron(A, k.dKd_dLen(xg[d][:, None], t == d, lengthscale=ls[t]) if t < D else k.dKd_dVar(xg[d][:, None]))
        if t < D:
            e = np.zeros(D)
            e[t] = h
            num = (full_K(variance, ls + e) - full_K(variance, ls - e)) / (2 * h)
        else:
            num = (full_K(variance + h, ls) - full_K(variance - h, ls)) / (2 * h)
        assert np.abs(A - num).max() <= 1e-8 * max(1.0, np.abs(num).max()), (t, np.abs(A - num).max())
    # the Kronecker product of the factors is the reference's RBF on the grid, the variance carried once
    X = KR.grid_of(xg)
    r2 = (((X[:, None, :] - X[None, :, :]) / ls) ** 2).sum(-1)
    assert np.abs(full_K(variance, ls) - variance * np.exp(-0.5 * r2)).max() <= 8 * EPS * variance


class RecordingKron(object):
    """stands where `_lib.KronContext` stands and answers from the float64 restatement"""
    log = []

    def __init__(self, device=0):
        self.device, self.G, self.N = device, (), 0
        type(self).log.append(("create", device))

    def set_data(self, G, y):
        self.G, self.y, self.N = tuple(int(g) for g in G), np.array(y, dtype=np.float64).ravel(), int(np.prod(G))
        type(self).log.append(("set_data", self.G, self.y.copy()))

    def solve(self, Qs, lams, noise):
        self.Qs, self.lams, self.noise = [np.array(q) for q in Qs], [np.array(v) for v in lams], noise
        self.r = KR.evaluate(self.Qs, self.lams, self.y, noise, dt=np.float64)
        type(self).log.append(("solve", noise))
        return float(self.r["yTa"]), float(self.r["sumlog"])

    def quadforms(self, factors, gammas):
        r = KR.evaluate(self.Qs, self.lams, self.y, self.noise, factors, gammas, dt=np.float64)
        type(self).log.append(("quadforms", len(factors), [[np.array(a) for a in A] for A in factors]))
        return r["q"], r["s"]

    def predict(self, kx, bx, noise_pred, want_var=True):
        type(self).log.append(("predict", noise_pred, np.shape(kx[0])[0]))
        return KR.predict(self.r["alpha"], self.lams, kx, bx, noise_pred, np.float64)

    def fetch_alpha(self):
        type(self).log.append(("fetch_alpha",))
        return self.r["alpha"].copy()


@pytest.fixture
def recording(monkeypatch):
    RecordingKron.log = []
    monkeypatch.setattr(_lib, "KronContext", RecordingKron)
    return RecordingKron


def model_of(g, cls=None):
    D = g["X"].shape[1]
    k = gpy_amd.RBF(D, variance=float(g["variance"]), lengthscale=g["lengthscale"], ARD=bool(g["ARD"]))
    m = (cls or gpy_amd.GPRegressionGrid)(g["X"], g["Y"], k)
    m.likelihood.variance[:] = float(g["noise"])
    m.parameters_changed()
    return m


def model_results(m, g):
    mu, var = m.predict_noiseless(g["Xs"])
    return dict(alpha=m.posterior.alpha, lml=m.log_likelihood(), grad=np.concatenate([m.kern.lengthscale.gradient.ravel(),
                m.kern.variance.gradient.ravel(), m.likelihood.variance.gradient.ravel()]), mu=mu, var=var)


@needs_ld
@pytest.mark.parametrize("name", KR.FIXTURES)
def test_model_over_the_recording_context_against_the_fixtures(recording, name):
    """the host classes (own sorted grid values, own eigh) with float64 device answers: ten times the long-double restatement's
    own distance from the fixture, the bound tests/test_gpu_kron.py holds the device to"""
    g = KR.load_fixture(name)
    own = fixture_figures(g, fixture_restated(g))
    figs = fixture_figures(g, model_results(model_of(g), g))
    print(name, "  ".join("%s %.1e (%.1e)" % (q, figs[q], own[q]) for q in figs))
    tol = 1000 * EPS * kappa(g["lams"], float(g["noise"]))             # here: the bound of the fixtures themselves
    for q, e in figs.items():
        assert e <= tol, (q, e, tol)


def test_call_order_uploads_and_gradient_installation(recording):
    g = KR.load_fixture("d3_5x4x3_ard")
    m = model_of(g)
    names = [c[0] for c in recording.log]
    # construction (default noise 1) and one explicit parameters_changed: one context, y uploaded once, no fetch yet
    assert names == ["create", "set_data", "solve", "quadforms", "solve", "quadforms"], names
    assert recording.log[1][1] == (5, 4, 3) and np.array_equal(recording.log[1][2], g["Y"].ravel())
    assert recording.log[2][1] == 1.0 + 1e-8 and recording.log[4][1] == float(g["noise"]) + 1e-8
    nmat, factors = recording.log[5][1:]
    assert nmat == 5 and all(np.array_equal(a, np.eye(a.shape[0])) for a in factors[4])
    assert set(m.grad_dict) == {"dL_dLen", "dL_dVar", "dL_dthetaL"} and m.grad_dict["dL_dLen"].shape == (3,)
    assert np.array_equal(m.kern.lengthscale.gradient, m.grad_dict["dL_dLen"])
    assert float(m.kern.variance.gradient[0]) == m.grad_dict["dL_dVar"]
    assert float(m.likelihood.variance.gradient[0]) == m.grad_dict["dL_dthetaL"]
    assert m.gradient.shape == (5,) and m.parameter_names()[-1].endswith("variance")
    # alpha and V_kron are lazy: one fetch, then cached
    a = m.posterior.alpha
    assert a.shape == (60, 1) and m.posterior.alpha is a and [c[0] for c in recording.log].count("fetch_alpha") == 1
    assert m.posterior.V_kron.shape == (60, 1) and len(m.posterior.Qs) == 3 and np.array_equal(m.posterior.QTs[1], m.posterior.Qs[1].T)
    # predict: the likelihood variance WITHOUT 1e-8, and added to the variance by predict but not by predict_noiseless
    mu, var = m.predict(g["Xs"])
    assert recording.log[-1] == ("predict", float(g["noise"]), 13)
    mu0, var0 = m.predict_noiseless(g["Xs"])
    assert np.array_equal(mu, mu0) and np.allclose(var - var0, float(g["noise"]), rtol=0, atol=1e-15)
    # a stale posterior refuses to fetch
    post = m.posterior
    post2 = gpy_amd.GaussianGridInference.inference(m.inference_method, m.kern, m.X, m.likelihood, m.Y)[0]
    fresh = K.GridPosterior(alpha_kron=post2._alpha_kron, QTs=post.QTs, Qs=post.Qs, V_kron=post.V_kron)
    assert fresh.alpha.shape == (60, 1)
    with pytest.raises(RuntimeError, match="not the device's latest"):
        m.predict(g["Xs"])
    with pytest.raises(ValueError, match="insufficient information"):
        K.GridPosterior(alpha_kron=a, QTs=post.QTs, Qs=post.Qs)


def test_same_X_is_validated_once_and_new_Y_is_uploaded(recording, monkeypatch):
    g = KR.load_fixture("d2_6x5_ard")
    calls = []
    real = K.grid_values
    monkeypatch.setattr(K, "grid_values", lambda X: calls.append(1) or real(X))
    m = model_of(g)
    n0 = len(calls)                                   # the constructor's check and the session's
    m.kern.variance[:] = 2.0
    m.parameters_changed()
    assert len(calls) == n0 == 2
    m.set_Y(g["Y"] * 2.0)
    assert len(calls) == n0 and [c[0] for c in recording.log].count("set_data") == 2
    m.set_XY(g["X"] + 1.0, g["Y"])
    assert len(calls) == n0 + 1 and [c[0] for c in recording.log].count("set_data") == 3


def test_one_lengthscale_for_several_dimensions_sums_the_gradients(recording):
    g = KR.load_fixture("d2_6x5_ard")
    ard = gpy_amd.GPRegressionGrid(g["X"], g["Y"], gpy_amd.RBF(2, variance=1.2, lengthscale=[1.5, 1.5], ARD=True))
    iso = gpy_amd.GPRegressionGrid(g["X"], g["Y"], gpy_amd.RBF(2, variance=1.2, lengthscale=1.5))
    assert iso.log_likelihood() == ard.log_likelihood()
    assert iso.kern.lengthscale.gradient.shape == (1,)
    assert iso.kern.lengthscale.gradient[0] == ard.kern.lengthscale.gradient.sum()
    assert iso.checkgrad() and ard.checkgrad()


def test_normalizer_and_pickling(recording):
    g = KR.load_fixture("d2_6x5_ard")
    k = gpy_amd.RBF(2, variance=1.2, lengthscale=[1.5, 1.1], ARD=True)
    m = gpy_amd.GPRegressionGrid(g["X"], 3.0 * g["Y"] + 5.0, k, normalizer=True)
    plain = gpy_amd.GPRegressionGrid(g["X"], m.Y_normalized, gpy_amd.RBF(2, variance=1.2, lengthscale=[1.5, 1.1], ARD=True))
    assert m.log_likelihood() == plain.log_likelihood()
    mu, var = m.predict(g["Xs"])
    mu0, var0 = plain.predict(g["Xs"])
    assert np.allclose(mu, mu0 * m.normalizer.std + m.normalizer.mean, rtol=1e-14) and np.allclose(var, var0 * m.normalizer.std ** 2, rtol=1e-14)
    m2 = pickle.loads(pickle.dumps(m))
    assert m2.inference_method._state is None and m2.posterior._state is None
    assert np.array_equal(m2.posterior.alpha, m.posterior.alpha) and m2.log_likelihood() == m.log_likelihood()
    m2.parameters_changed()                            # a fresh context
    assert np.array_equal(m2.predict(g["Xs"])[0], mu)


def test_every_refusal_by_message(recording):
    g = KR.load_fixture("d2_6x5_ard")
    X, Y = g["X"], g["Y"]
    rbf = lambda **kw: gpy_amd.RBF(2, ARD=True, **kw)                                  # noqa: E731
    G = gpy_amd.GPRegressionGrid
    cases = [
        (lambda: G(X, Y, gpy_amd.Matern52(2, ARD=True)), NotImplementedError, "one RBF kernel.*not Matern52"),
        (lambda: G(X, Y, rbf() + gpy_amd.White(2)), NotImplementedError, "one RBF kernel.*not Add"),
        (lambda: G(X, Y, gpy_amd.RBF(2, inv_l=True)), NotImplementedError, "inv_l=True"),
        (lambda: G(X, Y, gpy_amd.RBF(1, active_dims=[1])), NotImplementedError, r"all 2 input columns.*active_dims \[1\]"),
        (lambda: G(X, Y), NotImplementedError, r"all 2 input columns.*active_dims \[0\]"),
        (lambda: G(X, np.hstack([Y, Y]), rbf()), NotImplementedError, r"one output column, Y has shape \(30, 2\)"),
        (lambda: gpy_amd.GpGrid(X, Y, rbf(), gpy_amd.Bernoulli()), NotImplementedError, "Gaussian likelihood, not Bernoulli"),
        (lambda: gpy_amd.GpGrid(X, Y, rbf(), gpy_amd.Gaussian(), mean_function=object()), NotImplementedError, "mean function"),
        (lambda: G(X[:-1], Y[:-1], rbf()), ValueError, r"6 x 5 distinct values, a full grid of them has 30 points, X has 29 rows"),
        (lambda: G(X[::-1], Y, rbf()), ValueError, r"row 0 is \(5, 6\), the grid expects \(0, 2\)"),
        (lambda: G(np.vstack([X[:7], X[6:7], X[8:]]), Y, rbf()), ValueError, r"row 7 is \(1, 3\), the grid expects \(1, 4\)"),
        (lambda: G(np.where(np.arange(30)[:, None] == 3, np.nan, X), Y, rbf()), ValueError, "not finite"),
    ]
    for call, exc, msg in cases:
        with pytest.raises(exc, match=msg):
            call()
    assert recording.log == [], "a refusal reached the device"
    m = G(X, Y, rbf())
    Xs = g["Xs"]
    for call, msg in [(lambda: m.predict(Xs, full_cov=True), "full_cov=True"),
                      (lambda: m.predict_noiseless(Xs, full_cov=True), "full_cov=True"),
                      (lambda: m.predictive_gradients(Xs), "predictive_gradients"),
                      (lambda: m.posterior_samples_f(Xs), "posterior_samples_f"),
                      (lambda: m.posterior_samples(Xs), "posterior_samples"),
                      (lambda: m.posterior_covariance_between_points(Xs, Xs), "posterior_covariance_between_points"),
                      (lambda: m.predict(Xs, kern=rbf()), "another kernel")]:
        with pytest.raises(NotImplementedError, match=msg):
            call()
    with pytest.raises(ValueError, match=r"Xnew must be M x 2"):
        m.predict(Xs[:, :1])
    q = m.predict_quantiles(Xs)
    assert len(q) == 2 and q[0].shape == (13, 1) and (q[0] < q[1]).all()                 # comes free of `GP`
    for name in ("SSGPLVM", "MRD", "GPLVM", "SparseGPLVM"):
        with pytest.raises(NotImplementedError):
            getattr(gpy_amd.models, name)


def test_the_names_a_gpy_user_types():
    GPy = gpy_amd
    assert GPy.models.GPRegressionGrid is GPy.GPRegressionGrid is K.GPRegressionGrid
    assert GPy.core.GpGrid is K.GpGrid and issubclass(K.GPRegressionGrid, K.GpGrid) and issubclass(K.GpGrid, GPy.core.GP)
    lfi = GPy.inference.latent_function_inference
    assert lfi.GaussianGridInference is lfi.gaussian_grid_inference.GaussianGridInference is K.GaussianGridInference
    assert lfi.grid_posterior.GridPosterior is lfi.GridPosterior is K.GridPosterior
    sig = inspect.signature(K.GPRegressionGrid.__init__)
    assert list(sig.parameters) == ["self", "X", "Y", "kernel", "Y_metadata", "normalizer", "device"]
    assert K.GaussianGridInference().to_dict()["class"].endswith("gaussian_grid_inference.GaussianGridInference")


def test_host_kron_mvprod_is_the_reference_order():
    rng = np.random.default_rng(3)
    As = [rng.standard_normal((g, g)) for g in (3, 2, 4)]
    b = rng.standard_normal(24)
    full = np.kron(np.kron(As[0], As[1]), As[2])
    got = K.GaussianGridInference().kron_mvprod(As, b[:, None])
    assert got.shape == (24, 1) and np.allclose(got.ravel(), full.dot(b), rtol=0, atol=1e-13)
    assert np.allclose(KR.kron_mv(As, b, np.float64), full.dot(b), rtol=0, atol=1e-13)


def test_the_binding_table_states_the_prototypes_of_the_kron_header():
    protos = _prototypes("mi355gp_kron.h")
    assert [p[0] for p in protos] == list(_lib.KRON_ABI) and len(protos) == 9 and all(p[1] == "int" for p in protos)
    others = set(_lib.ABI) | set(_lib.DEBUG_LAUUM_ABI) | set(_lib.DEBUG_TILEOPS_ABI) | set(_lib.EPDTC_ABI) | set(_lib.VARGAUSS_ABI)
    assert not set(_lib.KRON_ABI) & others and all(n.startswith("mi355gp_kron_") for n in _lib.KRON_ABI)
    for name, _, types in protos:
        bound = _lib.KRON_ABI[name]
        assert len(bound) == len(types), name
        for i, (c, b) in enumerate(zip(types, bound)):
            assert _type_class(c, b), (name, i, c, b)
    assert "KRON_ABI" in inspect.getsource(_lib.lib)
    assert "mi355gp_kron.h" in inspect.getsource(_lib.build)
    mk = open(os.path.join(ROOT, "gpy_amd", "csrc", "Makefile")).read()
    assert "mi355gp_kron.h" in mk and "kron.hip" in mk
    header = open(os.path.join(ROOT, "include", "mi355gp.h")).read()
    assert "kron" not in header.lower()                            # the drop-in header and its 84 prototypes are as they were
    assert set(_lib.KRON_ABI).isdisjoint(_lib.EXPORTED)
