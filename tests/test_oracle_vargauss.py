"""CPU: VarGauss inference and GPVariationalGaussianApproximation without a device.

1. The long-double restatement tests/vargauss_ld.py against fixtures of the reference's OWN `VarGauss.inference`
   (tests/golden/vargauss/*.npz, written by tools/make_golden_vargauss.py through oracle/ref_loader.py): Bernoulli on RBF iso,
   Matern52-ARD, RBF + Linear + Bias and StdPeriodic at D = 1; Gaussian, StudentT and Poisson on RBF; one fixture with mixed-sign
   beta; every part list carries a White part so that cond2(K) <= 1516 and the reference's K^-1 posterior can be a fixture too.
   Distances found, max |restatement - fixture| / max |fixture| over the eight fixtures:
       m 1.5e-15   var 1.2e-14   lml 2.2e-16   dalpha 6.6e-16   dbeta 3.9e-14   dL_dK_sym 7.0e-15   dL_dthetaL 5.4e-16
       dtheta 5.6e-16   pred_mu 1.1e-15   pred_var 2.7e-14   pred_cov 2.7e-14
   The bound (vargauss_ld.FIXTURE_TOL) is ten times each, and tests/test_gpu_vargauss.py holds the device to the same.
2. Every case of the shape sweep keeps cond2(A) <= 1e4 (checked here, before any device sees it).
3. `VarGauss.inference` and the model end to end over a recording context that answers from the restatement: the call order, the
   upload of the signed beta, the results against the fixtures, the refusals by message, parameter order, names and `to_dict`.
4. `_lib.VARGAUSS_ABI` against the prototypes of include/mi355gp_vargauss.h.
5. Which form of dL_dK is the gradient of the bound: central differences of the restated bound in the kernel parameters agree with
   T diag(dF_dv) T^T (the package's default) and not with the reference's row-scaled (T o dF_dv) T^T (var_gauss.py:65)."""
import inspect
import os

import numpy as np
import pytest

import gpy_amd
from gpy_amd import _lib

import kern_ld as KL
import vargauss_ld as VL
from test_abi import _prototypes, _type_class

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_ld = pytest.mark.skipif(not KL.HAVE_LD, reason="np.longdouble is not an extended format on this host")


def _rel(got, want):
    return VL.SL.rel_err(np.asarray(got, float).reshape(np.shape(want)), np.asarray(want, float))


def test_the_fixtures_are_the_eight_of_the_issue():
    assert len(VL.FIXTURES) == 8
    liks = sorted(VL.load_fixture(n)["lik"] for n in VL.FIXTURES)
    assert liks == ["bernoulli"] * 5 + ["gaussian", "poisson", "studentt"]
    for n in VL.FIXTURES:
        g = VL.load_fixture(n)
        assert 120 <= g["X"].shape[0] <= 160 and float(g["condK"]) <= 1e4 and float(g["condA"]) <= 1e4
        assert os.path.getsize(os.path.join(VL.GOLDEN, n + ".npz")) < 400 * 1024
    assert (VL.load_fixture("bernoulli_rbf_iso_mixed_signs_n120_d2")["beta"] < 0).sum() > 30


@needs_ld
@pytest.mark.parametrize("name", VL.FIXTURES)
def test_restatement_against_the_reference(name):
    g = VL.load_fixture(name)
    r = VL.restate_fixture(g)
    figs = dict((q, _rel(KL.f64(r[q]), g[q])) for q in VL.FIXTURE_Q)
    print(name, "  ".join("%s %.1e" % kv for kv in figs.items()))
    for q, e in figs.items():
        assert e <= VL.FIXTURE_TOL[q], (q, e, VL.FIXTURE_TOL[q])
    assert np.array_equal(g["dL_dK_sym"], g["dL_dK_sym"].T)


def test_every_case_of_the_sweep_is_well_conditioned():
    assert VL.NAMES["n_edge"] == ["n_edge-rbf_ard+bias-n%d" % N for N in (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513)]
    assert len(VL.NAMES["signs"]) == 10 and len(VL.NAMES["kernels"]) == 9 and VL.BY_NAME[VL.NAMES["points"][0]]["Ms"] == (1, 127, 128, 129, 257)
    worst = 0.0
    for name in VL.BY_NAME:
        c = VL.make_case(name)
        K = KL.f64(KL.K(c["specs"], c["X"], None, np.float64)) + np.zeros((c["N"], c["N"]))
        b = c["beta"]
        kappa = float(np.linalg.cond(np.eye(c["N"]) + b[:, None] * K * b[None, :]))
        worst = max(worst, kappa)
        assert kappa <= 1e4, (name, kappa)
        assert np.abs(b).max() <= 7.0 and np.abs(b).min() > 0
        if c["variant"] == "big":
            assert np.abs(b).max() == 7.0
        if c["variant"] == "small":
            assert (np.abs(b) == 1e-2).sum() == max(c["N"] // 10, 1)
        if c["variant"] == "dfdv":
            assert (c["dF_dv"] == 0).sum() == max(c["N"] // 10, 1) and (c["dF_dv"] > 0).any() and (c["dF_dv"] < 0).any()
        if c["variant"] in ("mixed", "small", "big", "dfdv"):
            assert (b < 0).any() and (b > 0).any()
    print("worst cond2(A) of the sweep: %.1f" % worst)


@needs_ld
def test_the_restatement_states_the_reference_formulas():
    """the reference's lines in plain NumPy (with its cancelling Sigma) next to the restatement, on a small mixed-sign case"""
    c, ref, r64, kappa = VL.reference("kernels-rbf_x_coreg_r1-n65")
    K, b, al, g, v, n = KL.f64(ref["K"]), c["beta"], c["alpha"], c["dF_dm"], c["dF_dv"], c["N"]
    Ai = np.linalg.inv(np.eye(n) + b[:, None] * K * b[None, :])
    Sigma = np.diag(b ** -2.) - Ai / b[:, None] / b[None, :]
    A_A2 = Ai - Ai.dot(Ai)
    tmp = Ai * b[:, None] / b[None, :]
    dL = np.outer(al, g) + np.dot(tmp * v[:, None], tmp.T) - 0.5 * (np.outer(al, al) + np.outer(b, b) * A_A2)
    want = dict(var=np.diag(Sigma), dbeta=-2 * np.sum(Sigma ** 2 * (v[:, None] * b), 0) - np.diag((K * b[:, None]).T.dot(A_A2)),
                dL_dK=0.5 * (dL + dL.T), trAi=np.trace(Ai), dalpha=K.dot(g) - K.dot(al),
                woodbury_inv=b[:, None] * Ai * b[None, :])
    for q, w in want.items():
        assert _rel(w, KL.f64(ref[q])) <= 1e-12, q


@needs_ld
def test_which_form_of_dL_dK_is_the_gradient_of_the_bound():
    """Central differences of the restated bound in the kernel parameters, on a Bernoulli fixture (dF_dv differs from point to
    point): the exact form T diag(dF_dv) T^T agrees to 1e-7, the reference's row-scaled (T o dF_dv) T^T (var_gauss.py:65) does not
    (it is off by more than 1e-4 of the gradient); on the Gaussian fixture, where dF_dv is constant, the two forms are the same."""
    g = VL.load_fixture("bernoulli_rbf_iso_mixed_signs_n120_d2")

    def bound(specs):
        return float(VL.restate_fixture(dict(g, specs=specs))["lml"])
    exact, ref = KL.f64(VL.restate_fixture(g, exact=True)["dtheta"]), KL.f64(VL.restate_fixture(g)["dtheta"])
    num, k = [], 0
    for i, sp in enumerate(g["specs"]):
        for j in range(len(sp[2])):
            h = 1e-5 * sp[2][j]
            up, dn = [list(x) for x in g["specs"]], [list(x) for x in g["specs"]]
            up[i][2], dn[i][2] = np.array(sp[2], float), np.array(sp[2], float)
            up[i][2][j] += h
            dn[i][2][j] -= h
            num.append((bound([tuple(x) for x in up]) - bound([tuple(x) for x in dn])) / (2 * h))
            k += 1
    num = np.array(num)
    print("central differences", num, "exact", exact, "reference", ref)
    scale = np.abs(num).max()
    assert np.abs(exact - num).max() <= 1e-7 * scale
    assert np.abs(ref - num).max() >= 1e-4 * scale
    gg = VL.load_fixture("gaussian_rbf_iso_n150_d1")
    a, b = VL.restate_fixture(gg, exact=True), VL.restate_fixture(gg)
    assert _rel(KL.f64(a["dL_dK_sym"]), KL.f64(b["dL_dK_sym"])) <= 1e-14 and _rel(KL.f64(a["dtheta"]), KL.f64(b["dtheta"])) <= 1e-13


# ---- the host class over a recording context -------------------------------------------------------------------------------
class RecordingContext(object):
    """Stands in for `_lib.Context`: records the calls and answers them from the restatement (long double, rounded once)."""
    made = []

    def __init__(self, device=0):
        self.log, self.uploads, self.jitters = [], {}, []
        self.fail_first = 0
        RecordingContext.made.append(self)

    def set_data(self, X, R):
        self.log.append("set_data")
        self.X, self.N = np.array(X), X.shape[0]

    def set_targets(self, R):
        self.log.append("set_targets")

    def laplace_begin(self, specs):
        self.log.append("laplace_begin")
        self.specs = [(s[0], s[1], np.asarray(s[2], float), np.arange(self.X.shape[1]) if s[3] is None else np.asarray(s[3]), s[4])
                      for s in specs]
        self.K = KL.K(self.specs, self.X, None, VL.LD) + np.zeros((self.N, self.N), dtype=VL.LD)

    def vargauss_forward(self, alpha, beta, extra_jitter=0.0):
        self.log.append("vargauss_forward")
        self.jitters.append(extra_jitter)
        self.uploads["alpha"], self.uploads["beta"] = np.array(alpha), np.array(beta)
        if len(self.jitters) <= self.fail_first:
            return 3, None, None, 0.0, 0.0, 0.0
        self.fw = VL.forward(self.K, np.ravel(alpha), np.ravel(beta))
        f = self.fw
        return 0, KL.f64(f["m"]), KL.f64(f["var"]), float(f["logdet"]), float(f["trAi"]), float(f["ma"])

    def vargauss_backward(self, dF_dm, dF_dv, exact=False):
        self.log.append("vargauss_backward_exact" if exact else "vargauss_backward")
        self.bw = VL.backward(self.specs, self.X, self.K, np.ravel(self.uploads["alpha"]), np.ravel(self.uploads["beta"]), self.fw,
                              np.ravel(dF_dm), np.ravel(dF_dv), exact=exact)
        return KL.f64(self.bw["dalpha"]), KL.f64(self.bw["dbeta"]), KL.f64(self.bw["dtheta"])

    def laplace_predict(self, specs, Xnew, wv, full_cov=False, want_var=True):
        self.log.append("laplace_predict")
        mu, var = VL.predict(self.specs, self.X, Xnew, np.ravel(wv), np.ravel(self.uploads["beta"]), self.fw["L"], full_cov)
        return KL.f64(mu), KL.f64(var)

    def fetch(self, which, fortran_order=False):
        self.log.append("fetch%d" % which)
        return KL.f64({_lib.FETCH_K: self.K, _lib.FETCH_KINV: self.bw["woodbury_inv"], _lib.FETCH_DLDK: self.bw["dL_dK"]}[which])


@pytest.fixture
def rec(monkeypatch):
    RecordingContext.made = []
    monkeypatch.setattr(_lib, "Context", RecordingContext)
    return RecordingContext


def _model(g):
    """the model at the fixture's alpha and beta, with the reference's form of the kernel gradient (what the fixtures hold)"""
    m = gpy_amd.GPVariationalGaussianApproximation(g["X"], g["Y"], VL.fixture_kernel(g["specs"]), VL.fixture_likelihood(g))
    m.inference_method.reference_gradient = True
    n = g["X"].shape[0]
    x = m.param_array
    x[-2 * n:-n], x[-n:] = g["alpha"][:, 0], g["beta"]
    m.param_array = x
    return m


def check_model_against_fixture(m, g):
    """({quantity: distance}, the model) of a model set to the fixture's alpha and beta; shared with tests/test_gpu_vargauss.py"""
    n = g["X"].shape[0]
    mu, var = m._raw_predict(g["Xs"])
    _, cov = m._raw_predict(g["Xs"], full_cov=True)
    nk = m.kern.size
    got = dict(m=m.posterior.mean, var=np.diag(np.asarray(m.posterior.covariance)), lml=m.log_likelihood(), dalpha=m.alpha.gradient,
               dbeta=m.beta.gradient, dL_dK_sym=np.asarray(m.grad_dict["dL_dK"]), dL_dthetaL=m.grad_dict["dL_dthetaL"],
               dtheta=m.gradient[:nk], pred_mu=mu, pred_var=var, pred_cov=cov)
    assert m.gradient.size == nk + m.likelihood.size + 2 * n
    return dict((q, _rel(got[q], g[q])) for q in VL.FIXTURE_Q)


@needs_ld
@pytest.mark.parametrize("name", ["bernoulli_rbf_iso_mixed_signs_n120_d2", "studentt_rbf_iso_n140_d2"])
def test_inference_end_to_end_over_a_recording_context(rec, name):
    g = VL.load_fixture(name)
    m = _model(g)
    ctx = rec.made[-1]
    assert len(rec.made) == 1
    one = ["laplace_begin", "vargauss_forward", "vargauss_backward"]
    assert ctx.log == ["set_data"] + one[:2] + ["vargauss_backward_exact"] + one   # the default is the exact form                   # the data are uploaded once, K is rebuilt per evaluation
    assert ctx.uploads["beta"].tobytes() == g["beta"].tobytes() and ctx.uploads["alpha"].tobytes() == g["alpha"][:, 0].tobytes()
    assert set(ctx.jitters) == {0.0}
    figs = check_model_against_fixture(m, g)
    assert ctx.log[7:] == ["laplace_predict", "laplace_predict", "fetch%d" % _lib.FETCH_K, "fetch%d" % _lib.FETCH_KINV,
                           "fetch%d" % _lib.FETCH_DLDK]
    for q, e in figs.items():
        assert e <= VL.FIXTURE_TOL[q], (q, e)
    gd = m.grad_dict
    assert sorted(gd) == ["dL_dK", "dL_dthetaL", "fused"] and gd["dL_dK"].matches_kernel(m.kern)
    assert np.array_equal(gd["fused"], gd["dL_dK"].fused_dtheta)
    post = m.posterior
    assert post.woodbury_chol is None and np.array_equal(post.woodbury_vector, g["alpha"])
    with pytest.raises(NotImplementedError, match="predictive_gradients is not implemented"):
        post.predictive_gradients(m.kern, g["Xs"])
    with pytest.raises(NotImplementedError, match="covariance_between_points is not implemented"):
        post.covariance_between_points(m.kern, g["X"], g["Xs"], g["Xs"])
    # the jitter ladder: an info code on the plain attempt is answered with mean(Kdiag) * 1e-6
    ctx.fail_first = len(ctx.jitters) + 1
    m.param_array = m.param_array
    assert ctx.jitters[-2] == 0.0 and abs(ctx.jitters[-1] - 1e-6 * np.mean(m.kern.Kdiag(g["X"]))) < 1e-18


def test_refusals_by_name(rec):
    g = VL.load_fixture("bernoulli_rbf_iso_n150_d2")
    X, Y, n = g["X"], g["Y"], g["X"].shape[0]
    al, be = gpy_amd.param.Param("alpha", np.zeros((n, 1)), positive=False), gpy_amd.param.Param("beta", np.ones(n), positive=False)
    inf = gpy_amd.VarGauss(al, be)
    k = gpy_amd.RBF(2)
    with pytest.raises(NotImplementedError, match="VarGauss inference with a mean function is not implemented"):
        inf.inference(k, X, gpy_amd.Bernoulli(), Y, mean_function=object())
    with pytest.raises(NotImplementedError, match="VarGauss inference on the MI355X path takes one output column"):
        inf.inference(k, X, gpy_amd.Bernoulli(), np.hstack([Y, Y]))
    with pytest.raises(NotImplementedError, match="the MI355X VarGauss path evaluates gpy_amd kernels on the device"):
        inf.inference(gpy_amd.White(2), X, gpy_amd.Bernoulli(), Y)

    class NoVE(object):
        size = 0
    with pytest.raises(NotImplementedError, match="needs a likelihood with variational_expectations, NoVE has none"):
        inf.inference(k, X, NoVE(), Y)
    with pytest.raises(ValueError, match="alpha has 150 and beta 150 entries for 149 data points"):
        inf.inference(k, X[:-1], gpy_amd.Bernoulli(), Y[:-1])
    assert rec.made == []
    assert inf.to_dict() == {"class": "GPy.inference.latent_function_inference.var_gauss.VarGauss"}


@needs_ld
def test_model_parameters_names_and_to_dict(rec):
    g = VL.load_fixture("gaussian_rbf_iso_n150_d1")
    n = g["X"].shape[0]
    m = gpy_amd.GPVariationalGaussianApproximation(g["X"], g["Y"], VL.fixture_kernel(g["specs"]), VL.fixture_likelihood(g))
    assert m.name == "VarGP" and isinstance(m.inference_method, gpy_amd.VarGauss)
    assert m.inference_method.alpha is m.alpha and m.inference_method.beta is m.beta
    assert m.alpha.shape == (n, 1) and m.beta.shape == (n,) and not m.alpha.positive and not m.beta.positive
    assert np.array_equal(m.alpha, np.zeros((n, 1))) and np.array_equal(m.beta, np.ones(n))
    names = m.parameter_names()
    nk = m.kern.size
    assert m.parameters == [m.kern, m.likelihood, m.alpha, m.beta]
    assert len(names) == nk + 1 + 2 * n and names[nk] == "Gaussian_noise.variance"
    assert names[nk + 1] == "alpha[0]" and names[nk + 1 + n] == "beta[0]" and names[-1] == "beta[%d]" % (n - 1)
    d = m.to_dict()
    assert d["class"] == "GPy.models.GPVariationalGaussianApproximation" and d["name"] == "VarGP"
    assert d["inference_method"] == {"class": "GPy.inference.latent_function_inference.var_gauss.VarGauss"}
    assert gpy_amd.models.GPVariationalGaussianApproximation is gpy_amd.GPVariationalGaussianApproximation
    lfi = gpy_amd.inference.latent_function_inference
    assert lfi.VarGauss is gpy_amd.VarGauss and lfi.var_gauss.VarGauss is gpy_amd.VarGauss
    for call in (lambda: m.predictive_gradients(g["Xs"]), lambda: m.posterior_covariance_between_points(g["Xs"], g["Xs"])):
        with pytest.raises(NotImplementedError):
            call()
    mb = gpy_amd.GPVariationalGaussianApproximation(g["X"], (g["Y"] > 0).astype(float), gpy_amd.RBF(1), gpy_amd.Bernoulli())
    for call in (lambda: mb.predictive_gradients(g["Xs"]), lambda: mb.log_predictive_density(g["Xs"], g["Y"][:13]),
                 lambda: mb.predict_quantiles(g["Xs"]), lambda: mb.posterior_covariance_between_points(g["Xs"], g["Xs"])):
        with pytest.raises(NotImplementedError):
            call()


def test_the_binding_table_states_the_prototypes_of_the_vargauss_header():
    protos = _prototypes("mi355gp_vargauss.h")
    assert [p[0] for p in protos] == list(_lib.VARGAUSS_ABI) and len(protos) == 3 and all(p[1] == "int" for p in protos)
    assert not set(_lib.VARGAUSS_ABI) & (set(_lib.ABI) | set(_lib.DEBUG_LAUUM_ABI) | set(_lib.DEBUG_TILEOPS_ABI) | set(_lib.EPDTC_ABI))
    for name, _, types in protos:
        bound = _lib.VARGAUSS_ABI[name]
        assert len(bound) == len(types), name
        for i, (c, b) in enumerate(zip(types, bound)):
            assert _type_class(c, b), (name, i, c, b)
    assert "VARGAUSS_ABI" in inspect.getsource(_lib.lib)
    assert "mi355gp_vargauss.h" in inspect.getsource(_lib.build)
    assert "mi355gp_vargauss.h" in open(os.path.join(ROOT, "gpy_amd", "csrc", "Makefile")).read()
    header = open(os.path.join(ROOT, "include", "mi355gp.h")).read()
    assert "vargauss" not in header.lower()                       # the drop-in header and its 84 prototypes are as they were
    assert set(_lib.VARGAUSS_ABI).isdisjoint(_lib.EXPORTED)
