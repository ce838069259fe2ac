"""CPU: `BayesianGPLVM` and what it stands on -- the NumPy restatement of tests/bgplvm_np.py (KL term, bound, q(X) gradients,
prediction at uncertain points) against the reference's own values in tests/golden/bgplvm/*.npz (tools/make_golden_bgplvm.py),
the latent initialisation, and the model's routing and refusals over a recording context (no device).

Measured here (|mu|, |z| <= 3, S in [0.05, 1]):
  prediction at uncertain points GIVEN woodbury_vector and woodbury_inv (the sums k_psi2n_contract makes), relative to psi0*,
  worst over the eleven shapes of bgplvm_np.EDGE_CASES (fits with a White part or few inducing points, so |woodbury_inv| <= 3.3):
  float64 restatement against long-double restatement
    mean 4.2e-16   variance 1.3e-15
  Times ten for a different summation order on the device, these bound tests/test_gpu_bgplvm.py: 4.2e-15 and 1.3e-14.
  Restatement (float64 and long double alike) against the reference's float64 fixture values, the reference's own
  woodbury_vector and woodbury_inv given, worst over the seven fixtures: mean 3.3e-15, variance 1.5e-12 relative to psi0*
  (without a White part Kmm + 1e-8 I is ill conditioned, woodbury_inv reaches 1e4 and the terms of the variance cancel that
  far); KL 3.6e-16, its gradients 1.1e-16.
The whole evaluation (bound, gradients, prediction from its own posterior) is held to the sparse path's tolerances as in
tests/test_oracle_psi.py: 1e-9 for the bound, 1e-6 for gradients and means, 1e-5 for variances.
"""
import glob
import os

import numpy as np
import pytest

import bgplvm_np as B
import psi_np as P

LD = np.longdouble
F64_PRED_MEAN, F64_PRED_VAR = 4.2e-16, 1.3e-15     # the measured figures above, rounded up in the last digit
REF_PRED_MEAN, REF_PRED_VAR, REF_KL, REF_DKL = 3.3e-15, 1.5e-12, 3.6e-16, 1.1e-16
TOL_LML, TOL_FIT, TOL_VAR = 1e-9, 1e-6, 1e-5       # the sparse path's tolerances (tests/test_gpu_sparse.py)
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(f for f in glob.glob(os.path.join(HERE, "golden", "bgplvm", "*.npz")) if not os.path.basename(f).startswith("pca_"))
PCA_FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "bgplvm", "pca_*.npz")))
FIX_IDS = [os.path.basename(f)[:-4] for f in FIXTURES]


def fixture_args(g):
    """(variance, lengthscale, ARD, white, Z, mu, S) on the kernel's active columns"""
    d = g["dims"]
    return float(g["variance"]), g["ls"], bool(g["ARD"]), list(g["white"]), g["Z"][:, d], g["mu"][:, d], g["S"][:, d]


def _rel(x, ref, scale=None):
    ref = np.asarray(ref, dtype=LD)
    return float(np.abs(np.asarray(x, dtype=LD) - ref).max() / (np.abs(ref).max() if scale is None else scale))


def test_the_fixture_set_covers_the_cases_it_was_asked_for():
    seen = [np.load(f) for f in FIXTURES]
    assert len(seen) >= 4
    assert {bool(g["ARD"]) for g in seen} == {True, False} and {len(g["dims"]) for g in seen} == {1, 2, 3}
    assert {g["Y"].shape[1] for g in seen} == {1, 3, 12} and any(len(g["white"]) for g in seen)
    assert any(len(g["dims"]) < g["mu"].shape[1] for g in seen)
    assert all(g["mu"].shape[0] <= 200 for g in seen)
    for g in seen:
        for m, s in ((g["mu"], g["S"]), (g["Xs"], g["Ss"])):
            assert np.abs(m).max() <= 3 and 0.05 <= s.min() and s.max() <= 1
        # no predictive variance sits at the 1e-15 clip of posterior.py:268
        assert g["upred_var"].min() > 1e-3 and g["pred_var"].min() > 1e-6
        assert g["upred_var"].shape == g["upred_mu"].shape == (g["Xs"].shape[0], g["Y"].shape[1])


@pytest.mark.parametrize("path", FIXTURES, ids=FIX_IDS)
def test_restated_kl_and_uncertain_prediction_match_the_reference(path):
    g = np.load(path)
    var, ls, ARD, white, Z, mu, S = fixture_args(g)
    d = g["dims"]
    figs = {}
    for dt in (np.float64, LD):
        k, gm, gs = B.kl(mu, S, dt)
        figs["KL", dt] = abs(float(k) - float(g["KL"])) / float(g["KL"])
        figs["dKL", dt] = max(_rel(g["Xmean_grad"], g["dmu"].astype(LD) - gm), _rel(g["Xvar_grad"], g["dS"].astype(LD) - gs))
        pm, pv, psi0 = B.predict_uncertain(var, ls, white, Z, g["woodbury_vector"], g["woodbury_inv"], g["Xs"][:, d], g["Ss"][:, d], dt)
        figs["mean", dt] = _rel(g["upred_mu"], pm, scale=psi0)
        figs["var", dt] = _rel(g["upred_var"], pv, scale=psi0)
    print(os.path.basename(path), {"%s/%s" % (k[0], "ld" if k[1] is LD else "f64"): "%.2e" % v for k, v in figs.items()})
    for dt in (np.float64, LD):
        assert figs["KL", dt] <= REF_KL and figs["dKL", dt] <= REF_DKL
        assert figs["mean", dt] <= REF_PRED_MEAN and figs["var", dt] <= REF_PRED_VAR


@pytest.mark.parametrize("path", FIXTURES, ids=FIX_IDS)
def test_restated_bound_and_gradients_match_the_reference(path):
    g = np.load(path)
    var, ls, ARD, white, Z, mu, S = fixture_args(g)
    v = B.bound(var, ls, ARD, white, Z, mu, S, g["Y"], float(g["noise"]), dtype=LD)
    assert abs(g["bound"] - v["bound"]) <= TOL_LML * abs(v["bound"]) and abs(g["KL"] - v["KL"]) <= 1e-14 * abs(v["KL"])
    dtheta = np.concatenate([[v["dvar"]], v["dl"], v["dwhite"]]).astype(LD)
    for name, x, y in (("woodbury_vector", g["woodbury_vector"], v["woodbury_vector"]), ("woodbury_inv", g["woodbury_inv"], v["woodbury_inv"]),
                       ("dtheta", g["dtheta"], dtheta), ("dnoise", g["dnoise"], np.atleast_1d(v["dnoise"])), ("dZ", g["dZ"], v["dZ"]),
                       ("Xmean_grad", g["Xmean_grad"], v["Xmean_grad"]), ("Xvar_grad", g["Xvar_grad"], v["Xvar_grad"])):
        assert _rel(x, np.asarray(y)) <= (1e-4 if name == "woodbury_inv" else TOL_FIT), name
    d = g["dims"]
    pm, pv, psi0 = B.predict_uncertain(var, ls, white, Z, v["woodbury_vector"], v["woodbury_inv"], g["Xs"][:, d], g["Ss"][:, d], LD)
    assert _rel(g["upred_mu"], pm) <= TOL_FIT and _rel(g["upred_var"], pv) <= TOL_VAR


_edge = {}


def edge_reference(c):
    """the float64 fit of an edge case (woodbury_vector, woodbury_inv) and the long-double prediction GIVEN them, once"""
    if c not in _edge:
        p = B.edge_problem(c)
        a = (p["var"], p["ls"], p["white"], p["Z"])
        wv = P.vardtc_uncertain(p["var"], p["ls"], True, p["white"], p["Z"], p["mu"], p["S"], p["Y"], p["noise"], want_grads=False)["woodbury_vector"]
        Wi = B.woodbury_inv(*a, p["mu"], p["S"], p["noise"])
        _edge[c] = (p, wv, Wi, B.predict_uncertain(*a, wv, Wi, p["mu_new"], p["S_new"], LD))
    return _edge[c]


@pytest.mark.parametrize("c", B.EDGE_CASES, ids=B.edge_id)
def test_float64_prediction_is_within_its_measured_distance_of_long_double(c):
    p, wv, Wi, (mean, var, psi0) = edge_reference(c)
    m64, v64, _ = B.predict_uncertain(p["var"], p["ls"], p["white"], p["Z"], wv, Wi, p["mu_new"], p["S_new"])
    e = (_rel(m64, mean, scale=psi0), _rel(v64, var, scale=psi0))
    print(B.edge_id(c), "float64 against long double, relative to psi0*: mean %.2e  variance %.2e   (min variance %.3e)"
          % (e + (float(var.min()),)))
    assert var.min() > 1e-6                                            # far from the clip
    assert e[0] <= F64_PRED_MEAN and e[1] <= F64_PRED_VAR


@pytest.mark.parametrize("path", PCA_FIXTURES, ids=[os.path.basename(f)[:-4] for f in PCA_FIXTURES])
def test_initialize_latent_reproduces_the_references_pca(path):
    from gpy_amd.util.initialization import initialize_latent
    g = np.load(path)
    X, fracs = initialize_latent("PCA", int(g["Q"]), g["Y"])
    assert X.shape == g["X"].shape and np.allclose(fracs, g["fracs"], rtol=1e-9, atol=1e-12)
    sign = np.sign((X * g["X"]).sum(0))                                # an eigenvector's sign is arbitrary
    assert np.all(sign != 0) and np.allclose(X * sign, g["X"], rtol=1e-8, atol=1e-9)
    assert np.allclose(X.mean(0), 0, atol=1e-12) and np.allclose(X.std(0), 1)


def test_initialize_latent_random_and_refusal_and_pca_class():
    import gpy_amd
    from gpy_amd.util.initialization import initialize_latent
    from gpy_amd.util.pca import PCA
    assert gpy_amd.util.initialization.initialize_latent is initialize_latent
    Y = np.random.default_rng(0).standard_normal((20, 4))
    X, fracs = initialize_latent("random", 3, Y)
    assert X.shape == (20, 3) and fracs.shape == (3,) and fracs.max() == 1.0 and np.allclose(X.std(0), 1)
    with pytest.raises(ValueError, match="empirical_samples"):
        initialize_latent("empirical_samples", 3, Y)
    p = PCA(Y)
    assert p.Q == 4 and np.isclose(p.fracs.sum(), 1) and np.all(np.diff(p.eigvals) <= 0)
    assert np.allclose(p.eigvectors.T @ p.eigvectors, np.eye(4), atol=1e-12)
    assert p.project(Y, 2).shape == (20, 2)
    with pytest.raises(IndexError):
        p.project(Y, 5)


def test_normal_posterior_is_parameterized_and_the_prior_restates_the_reference():
    import gpy_amd
    from gpy_amd.variational import NormalPosterior, NormalPrior
    assert gpy_amd.NormalPrior is NormalPrior and gpy_amd.core.parameterization.variational.NormalPrior is NormalPrior
    r = np.random.default_rng(1)
    m, v = r.standard_normal((4, 3)), r.uniform(0.1, 2.0, (4, 3))
    q = NormalPosterior(m, v)
    assert [p.name for p in q.parameters] == ["mean", "variance"] and not q.mean.positive and q.variance.positive
    assert np.array_equal(q.param_array, np.concatenate([m.ravel(), v.ravel()])) and q.gradient.shape == (24,)
    q.set_gradients((np.ones((4, 3)), np.full((4, 3), 2.0)))
    assert np.array_equal(q.mean.gradient, np.ones((4, 3))) and np.array_equal(q.variance.gradient, np.full((4, 3), 2.0))
    prior = NormalPrior()
    k, gm, gs = B.kl(m, v)
    assert np.isclose(prior.KL_divergence(q), k, rtol=1e-14)
    prior.update_gradients_KL(q)
    assert np.allclose(q.mean.gradient, 1.0 - gm, rtol=1e-15) and np.allclose(q.variance.gradient, 2.0 - gs, rtol=1e-15)
    other = NormalPosterior(np.zeros((4, 3)), np.ones((4, 3)))
    assert np.isclose(q.KL(other), k, rtol=1e-13) and abs(q.KL(q)) < 1e-14
    x = q.param_array.copy()
    q.param_array = x + 0.5
    assert np.allclose(q.mean, m + 0.5) and np.allclose(q.variance, v + 0.5)


# ---- the model over a recording context: no device ----------------------------------------------------------------------------
class RecSparse(object):
    FETCH_DLDKMM, FETCH_WOODBURY_INV, FETCH_LM, FETCH_KMM, FETCH_PSI2, FETCH_DLDPSI2_BETA = range(6)
    sharded = False

    def __init__(self, device=0):
        self.log = []

    def set_data(self, X, Y):
        self.log.append(("set_data", np.array(X), np.array(Y)))
        self.N, self.D, self.Dy = X.shape[0], X.shape[1], Y.shape[1]

    def set_input_variance(self, S):
        self.log.append(("set_input_variance", np.array(S)))

    def set_inputs(self, X, S=None):
        self.log.append(("set_inputs", np.array(X), None if S is None else np.array(S)))

    def _res(self, specs, Z):
        nth = sum(np.size(s[2]) for s in specs)
        self.M = Z.shape[0]
        return 0, dict(lml=-1.0, dnoise=0.5, dtheta=np.arange(1.0, 1.0 + nth), dZ=np.full(Z.shape, 3.0),
                       woodbury_vector=np.ones((Z.shape[0], self.Dy)), dL_dm=None, dmu=np.full((self.N, self.D), 4.0),
                       dS=np.full((self.N, self.D), 5.0))

    def vardtc_sum(self, specs, Z, noise, **kw):
        self.log.append(("vardtc_sum", [s[0] for s in specs]))
        return self._res(specs, Z)

    def vardtc_uncertain(self, specs, Z, noise, **kw):
        self.log.append(("vardtc_uncertain", [s[0] for s in specs], np.array(Z), np.array(noise)))
        return self._res(specs, Z)

    def fetch(self, which):
        return np.full((self.M, self.M), 0.01 * (1 + which))

    def predict(self, specs, Xnew, full_cov=False, want_var=True):
        self.log.append(("sparse_predict", np.array(Xnew)))
        return np.zeros((Xnew.shape[0], self.Dy)), np.ones((Xnew.shape[0], 1))

    def predict_uncertain(self, specs, mu, S, want_var=True):
        self.log.append(("predict_uncertain", [s[0] for s in specs], np.array(mu), np.array(S)))
        return np.zeros((mu.shape[0], self.Dy)), np.ones((mu.shape[0], self.Dy))


@pytest.fixture
def rec(monkeypatch):
    from gpy_amd import _lib
    made = []

    class Ctx(RecSparse):
        def __init__(self, device=0):
            RecSparse.__init__(self, device)
            made.append(self)
    monkeypatch.setattr(_lib, "SparseContext", Ctx)
    return made


def _problem(N=12, Q=3, Dy=4, M=5, seed=4):
    r = np.random.default_rng(seed)
    return (r.standard_normal((N, Dy)), r.uniform(-2, 2, (N, Q)), r.uniform(0.1, 0.5, (N, Q)), r.uniform(-2, 2, (M, Q)))


def test_model_parameters_uploads_objective_and_gradients_over_a_recording_context(rec):
    import gpy_amd
    import gpy_amd as GPy
    assert GPy.models.BayesianGPLVM is gpy_amd.BayesianGPLVM and issubclass(gpy_amd.BayesianGPLVM, gpy_amd.SparseGP)
    Y, X, S, Z = _problem()
    N, Q, M = X.shape[0], X.shape[1], Z.shape[0]
    m = gpy_amd.BayesianGPLVM(Y, Q, X=X, X_variance=S, Z=Z)
    assert m.name == "bayesian gplvm" and isinstance(m.X, gpy_amd.NormalPosterior) and m.has_uncertain_inputs()
    assert isinstance(m.kern, gpy_amd.RBF) and m.kern.ARD and isinstance(m.likelihood, gpy_amd.Gaussian)
    assert isinstance(m.variational_prior, gpy_amd.NormalPrior)
    # flat order [X.mean, X.variance, Z, kernel, noise] and names
    assert m.parameters[0] is m.X and m.parameters[1] is m.Z
    assert [p.name for p in m.flattened_parameters()][:3] == ["mean", "variance", "inducing inputs"]
    names = m.parameter_names()
    assert names[0] == "latent space.mean[0]" and names[N * Q] == "latent space.variance[0]" and names[2 * N * Q] == "inducing inputs[0]"
    assert m.param_array.size == 2 * N * Q + M * Q + (1 + Q) + 1 == len(names)
    pa = m.param_array
    assert np.array_equal(pa[:N * Q], X.ravel()) and np.array_equal(pa[N * Q:2 * N * Q], S.ravel())
    assert np.array_equal(pa[2 * N * Q:2 * N * Q + M * Q], Z.ravel())
    log = rec[0].log
    assert [c[0] for c in log] == ["set_data", "set_input_variance", "vardtc_uncertain"]
    assert np.array_equal(log[0][1], X) and np.array_equal(log[0][2], Y) and np.array_equal(log[1][1], S)
    # objective = -(lml - KL); X gradients = dmu - mean, dS - (1 - 1/S)/2
    k, gm, gs = B.kl(X, S)
    assert np.isclose(m.objective_function(), -(-1.0 - k), rtol=1e-14) and np.isclose(m.log_likelihood(), -1.0 - k, rtol=1e-14)
    assert np.allclose(m.X.mean.gradient, 4.0 - X, rtol=1e-15) and np.allclose(m.X.variance.gradient, 5.0 - 0.5 * (1 - 1 / S), rtol=1e-15)
    assert np.array_equal(m._Xgrad, m.X.gradient) and np.array_equal(m.gradient[:2 * N * Q], m._Xgrad)
    assert m.get_X_gradients(m.X)[0] is m.X.mean.gradient
    m.set_X_gradients(m.X, (np.zeros(X.shape), np.ones(X.shape)))
    assert not m.X.mean.gradient.any() and np.all(m.X.variance.gradient == 1.0)
    # an unchanged evaluation uploads nothing; a step in X and S goes through set_inputs, and Y is not uploaded again
    m.parameters_changed()
    assert [c[0] for c in log][3:] == ["vardtc_uncertain"]
    new = pa.copy()
    new[:N * Q] += 0.25
    new[N * Q:2 * N * Q] *= 1.5
    m.param_array = new
    assert [c[0] for c in log][4:] == ["set_inputs", "vardtc_uncertain"]
    assert np.array_equal(log[4][1], X + 0.25) and np.array_equal(log[4][2], S * 1.5)
    assert np.array_equal(m.param_array, new)                          # round trip
    new[2 * N * Q] += 1.0                                              # Z alone: no upload at all
    m.param_array = new
    assert [c[0] for c in log][6:] == ["vardtc_uncertain"] and log[-1][2][0, 0] == Z[0, 0] + 1.0
    # prediction at certain and at uncertain points
    mu, var = m.predict(X[:5])
    assert log[-1][0] == "sparse_predict" and mu.shape == (5, Y.shape[1])
    qn = gpy_amd.NormalPosterior(X[:5], S[:5])
    mu, var = m.predict(qn)
    assert log[-1][0] == "predict_uncertain" and log[-1][1] == ["rbf"] and np.array_equal(log[-1][2], X[:5]) and np.array_equal(log[-1][3], S[:5])
    assert mu.shape == var.shape == (5, Y.shape[1]) and np.allclose(var, 1.0 + float(m.likelihood.variance.values[0]))
    mu, var = m.predict_noiseless(qn)
    assert np.allclose(var, 1.0)
    with pytest.raises(NotImplementedError, match="Full covariance"):
        m.predict(qn, full_cov=True)


def test_model_defaults_follow_the_reference(rec):
    import gpy_amd
    Y = B.example_data(seed=3, n_per=6, Dy=7)[0]
    np.random.seed(0)
    m = gpy_amd.BayesianGPLVM(Y, 3, num_inducing=4)
    from gpy_amd.util.initialization import initialize_latent
    X, fracs = initialize_latent("PCA", 3, Y)
    assert np.allclose(m.X.mean, X) and m.X.variance.max() <= 0.1 and m.X.variance.min() > 0
    assert m.Z.shape == (4, 3) and all(any(np.allclose(z, x) for x in X) for z in m.Z.values)
    assert np.allclose(m.kern.lengthscale.values, 1.0 / fracs) and m.init == "PCA"
    m2 = gpy_amd.BayesianGPLVM(Y, 2, init="random", num_inducing=3)
    assert m2.X.shape == (18, 2) and np.allclose(m2.X.mean.values.std(0), 1)
    # active_dims a strict subset: the device's gradients come back on the active columns and are scattered to full width
    k = gpy_amd.RBF(2, ARD=True, active_dims=[2, 0])
    m3 = gpy_amd.BayesianGPLVM(Y, 3, X=X, X_variance=np.full(X.shape, 0.5), Z=X[:4], kernel=k)
    assert rec[-1].log[0][1].shape == (18, 2)
    g = m3.X.mean.gradient
    assert np.allclose(g[:, [2, 0]], 4.0 - X[:, [2, 0]]) and np.allclose(g[:, 1], -X[:, 1])
    assert np.allclose(m3.X.variance.gradient[:, 1], -0.5 * (1 - 1 / 0.5))


def test_refusals_name_what_they_refuse(rec):
    import gpy_amd
    import gpy_amd as GPy
    Y, X, S, Z = _problem()
    kw = dict(X=X, X_variance=S, Z=Z)
    for arg, value in (("mpi_comm", object()), ("normalizer", True), ("missing_data", True), ("stochastic", True), ("batchsize", 10)):
        with pytest.raises(NotImplementedError, match=arg):
            gpy_amd.BayesianGPLVM(Y, 3, **dict(kw, **{arg: value}))
    assert not rec                                                     # nothing reached a context
    with pytest.raises(ValueError, match="empirical_samples"):
        gpy_amd.BayesianGPLVM(Y, 3, init="empirical_samples")
    with pytest.raises(ValueError, match="Z must have 3 columns"):
        gpy_amd.BayesianGPLVM(Y, 3, X=X, X_variance=S, Z=Z[:, :2])
    with pytest.raises(ValueError, match="X must be 12 x 3"):
        gpy_amd.BayesianGPLVM(Y, 3, X=X[:5])
    # kernels: refused by the code that refuses them for every uncertain-input fit
    for k, pat in ((gpy_amd.RBF(3) + gpy_amd.Bias(3), "bias.*Bias"), (gpy_amd.Matern52(3), "Mat52"), (gpy_amd.Linear(3), "Linear"),
                   (gpy_amd.RBF(3) + gpy_amd.RBF(3, name="other"), "exactly one RBF"), (gpy_amd.RBF(3) * gpy_amd.RBF(3, name="o"), "Prod")):
        with pytest.raises(NotImplementedError, match=pat):
            gpy_amd.BayesianGPLVM(Y, 3, kernel=k, **kw)
    m = gpy_amd.BayesianGPLVM(Y, 3, kernel=gpy_amd.RBF(3, ARD=True) + gpy_amd.White(3, variance=0.1), **kw)
    assert rec[-1].log[-1][1] == ["rbf", "white"]
    with pytest.raises(NotImplementedError, match="infer_newX"):
        m.infer_newX(Y[:2])
    for name in ("SSGPLVM", "MRD", "GPLVM", "SparseGPLVM"):
        with pytest.raises(NotImplementedError, match=name):
            getattr(GPy.models, name)
    # SparseGPRegression keeps X as data and keeps refusing uncertain new points
    s = gpy_amd.SparseGPRegression(X, Y, Z=Z, X_variance=S)
    assert s.param_array.size == Z.size + 2 + 1
    with pytest.raises(NotImplementedError, match="uncertain new points"):
        s.predict(gpy_amd.NormalPosterior(X[:2], S[:2]))


def test_host_fallback_of_uncertain_prediction_matches_the_restatement(rec, monkeypatch):
    """a posterior that is no longer the context's latest result predicts from kern.psi0 / psi1 / psi2n on the host; those need
    the device, so they are patched to the restatement here"""
    import gpy_amd
    g = np.load(FIXTURES[1])
    var, ls, ARD, white, Z, mu, S = fixture_args(g)
    k = gpy_amd.RBF(Z.shape[1], variance=var, lengthscale=ls, ARD=ARD)
    monkeypatch.setattr(gpy_amd.RBF, "psi1", lambda self, Z, q: P.psi_stats(var, ls, Z, q.mean, q.variance)[1])
    monkeypatch.setattr(gpy_amd.RBF, "psi2n", lambda self, Z, q: P.psi_stats(var, ls, Z, q.mean, q.variance, want_psi2n=True)[3])
    from gpy_amd.sparse import SparsePosterior
    post = SparsePosterior(g["woodbury_inv"], g["woodbury_vector"], None, None, device=None)
    d = g["dims"]
    qn = gpy_amd.NormalPosterior(g["Xs"][:, d], g["Ss"][:, d])
    pm, pv = post._raw_predict(k, qn, Z)
    rm, rv, psi0 = B.predict_uncertain(var, ls, white, Z, g["woodbury_vector"], g["woodbury_inv"], qn.mean, qn.variance, LD)
    # (a fixture without a White part: the bounds of the fixtures' regime, see the module docstring)
    assert _rel(pm, rm, scale=psi0) <= REF_PRED_MEAN and _rel(pv, rv, scale=psi0) <= REF_PRED_VAR
    assert _rel(pm, g["upred_mu"], scale=psi0) <= REF_PRED_MEAN and _rel(pv, g["upred_var"], scale=psi0) <= REF_PRED_VAR
    # in row blocks: a block of one row gives the same numbers
    assert np.allclose(post._raw_predict(k, qn[:1], Z)[1], pv[:1], rtol=1e-12)
    with pytest.raises(NotImplementedError, match="Full covariance"):
        post._raw_predict(k, qn, Z, full_cov=True)
    # a live posterior goes to the device call; one overwritten by a later fit does not
    Y, X, S2, Z2 = _problem()
    m = gpy_amd.BayesianGPLVM(Y, 3, X=X, X_variance=S2, Z=Z2)
    stale = m.posterior
    m.parameters_changed()
    assert stale._device["owner"]._token != stale._device["token"]
