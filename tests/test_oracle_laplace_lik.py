"""CPU checks of the Student-t and Poisson likelihoods under the Laplace approximation: the likelihoods and links against values
stored from the reference (tools/make_golden_laplace_lik.py), `_laplace_gradients` against central differences, the NumPy
restatement of the likelihood-parameter gradient (tests/laplace_lik_np.py) against central differences of its own log marginal
and against every fixture, and the host bookkeeping that needs no device."""
import os

import numpy as np
import pytest

import gpy_amd
import laplace_np as LP
import laplace_lik_np as LL

VALUES = os.path.join(LL.GOLDEN, "likelihood_values.npz")


def _same(got, want, what):
    got, want = np.asarray(got, float), np.asarray(want, float)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    assert np.allclose(got[ok], want[ok], rtol=1e-13, atol=0.0), (what, np.abs(got[ok] - want[ok]).max())


def test_the_cases_are_there():
    assert len(LL.CASES) == 5
    for want in ("studentt_rbf_iso", "studentt_matern52_ard", "studentt_rbf_linear_bias", "poisson_rbf_iso", "poisson_stdperiodic"):
        assert any(c.startswith(want) for c in LL.CASES), want
    for f in os.listdir(LL.GOLDEN):
        assert f.endswith(".npz") and os.path.getsize(os.path.join(LL.GOLDEN, f)) < 1 << 19
    assert sum(not LL.load(c)["check_y_prediction"] for c in LL.CASES) <= 1          # at most one Poisson predictive check dropped


def test_student_t_against_values_stored_from_the_reference():
    z = np.load(VALUES)
    f = z["f"]
    for tag in "abc":
        s2, v = z["studentt_%s_theta" % tag]
        lik = gpy_amd.likelihoods.StudentT(deg_free=v, sigma2=s2)
        for yv in (-1.5, 0.25, 6.0):
            y = np.full_like(f, yv)
            key = "studentt_%s_y%g_" % (tag, yv)
            for m in ("logpdf", "dlogpdf_df", "d2logpdf_df2", "d3logpdf_df3", "dlogpdf_link_dvar", "dlogpdf_dlink_dvar",
                      "d2logpdf_dlink2_dvar", "dlogpdf_link_dv", "dlogpdf_dlink_dv", "d2logpdf_dlink2_dv"):
                _same(getattr(lik, m)(f, y), z[key + m], key + m)
            for m, a in zip(("dlogpdf_dtheta", "dlogpdf_df_dtheta", "d2logpdf_df2_dtheta"), lik._laplace_gradients(f, y)):
                _same(a, z[key + m], key + m)
        _same(lik.predictive_mean(f, z["studentt_%s_pm_var" % tag]), z["studentt_%s_predictive_mean" % tag], tag)
        _same(np.ravel(lik.conditional_variance(f)), z["studentt_%s_conditional_variance" % tag], tag)     # a constant
    low = gpy_amd.StudentT(deg_free=1.5, sigma2=1.0)
    _same(low.predictive_variance(f, np.ones_like(f)), z["studentt_low_predictive_variance"], "deg_free <= 2")
    assert low.log_concave is False and low.size == 2


def test_poisson_and_the_links_against_values_stored_from_the_reference():
    z = np.load(VALUES)
    f = z["poisson_f"]
    lik = gpy_amd.likelihoods.Poisson()
    for yv in (0, 1, 7, 250):
        y = np.full_like(f, float(yv))
        for m in ("logpdf", "dlogpdf_df", "d2logpdf_df2", "d3logpdf_df3"):
            with np.errstate(all="ignore"):
                _same(getattr(lik, m)(f, y), z["poisson_y%d_%s" % (yv, m)], (yv, m))
    _same(lik.conditional_mean(f), z["poisson_conditional_mean"], "conditional_mean")
    _same(lik.conditional_variance(f), z["poisson_conditional_variance"], "conditional_variance")
    assert lik.log_concave is True and lik.size == 0
    assert [a.shape for a in lik._laplace_gradients(f, f)] == [(0,) + f.shape] * 3
    fl = z["link_f"]
    assert fl.max() == 800.0
    for name, link in (("identity", gpy_amd.link_functions.Identity()), ("log", gpy_amd.link_functions.Log())):
        for m in ("transf", "dtransf_df", "d2transf_df2", "d3transf_df3"):
            _same(getattr(link, m)(fl), z["%s_%s" % (name, m)], (name, m))
    mu, v = np.array([[0.3], [-1.0]]), np.array([[0.5], [2.0]])
    E = np.exp(mu + v / 2)
    assert np.allclose(lik.predictive_mean(mu, v), E, rtol=1e-15)
    assert np.allclose(lik.predictive_variance(mu, v), E + (np.exp(v) - 1) * np.exp(2 * mu + v), rtol=1e-14)
    s = lik.samples(np.full((4, 1), -700.0))
    assert s.shape == (4, 1) and not s.any()


@pytest.mark.parametrize("which", [0, 1])
def test_laplace_gradients_against_central_differences(which):
    """each of the three stacked arrays, differenced in t_scale2 (0) and deg_free (1); the arrays are smooth in both, so a
    central difference with h = 1e-5 theta carries a relative error of about h^2 = 1e-10 plus rounding eps / h = 1e-11"""
    rng = np.random.default_rng(3)
    f, y = rng.standard_normal((40, 1)), 2.0 * rng.standard_normal((40, 1))
    theta = np.array([0.7, 4.5])
    ana = gpy_amd.StudentT(deg_free=theta[1], sigma2=theta[0])._laplace_gradients(f, y)
    h = 1e-5 * theta[which]
    vals = []
    for sign in (1.0, -1.0):
        th = theta.copy()
        th[which] += sign * h
        lik = gpy_amd.StudentT(deg_free=th[1], sigma2=th[0])
        vals.append((lik.logpdf(f, y), lik.dlogpdf_df(f, y), lik.d2logpdf_df2(f, y)))
    for a, p, m in zip(ana, vals[0], vals[1]):
        fd = (p - m) / (2 * h)
        assert np.abs(fd - a[which]).max() <= 1e-8 * max(1.0, np.abs(a[which]).max())


STUDENT_CASES = [c for c in LL.CASES if c.startswith("studentt")]


@pytest.mark.parametrize("name", LL.CASES)
def test_restatement_against_the_reference(name):
    g = LL.load(name)
    specs, X, Y, Xs = g["specs"], g["X"], g["Y"], g["Xs"]
    lik = LL.make_likelihood(g)
    r = LL.inference(specs, X, Y, lik)
    mu, var = LP.predict(specs, X, r, Xs)
    ymean, yvar = lik.predictive_values(mu, var)
    got = dict(lml=r["lml"], f_hat=r["f_hat"], Ki_fhat=r["Ki_fhat"], dtheta=r["dtheta"], pred_mu=mu, pred_var=var)
    if lik.size:
        got["dL_dthetaL"] = r["dL_dthetaL"]
    if g["check_y_prediction"]:
        got.update(pred_ymean=ymean, pred_yvar=yvar)
    fig = LL.figures(g, got)
    for q in fig:
        assert fig[q] <= g["tol"][q], (q, fig[q], g["tol"][q])
    s = LL.implicit_vector(r["K"], r["woodbury_inv"], r["dL_dfhat"])
    dg = lik._laplace_gradients(r["f_hat"], Y)[1]
    for i in range(lik.size):            # the identity the device entry rests on: s . g_i is the reference's implicit term
        want = r["dL_dfhat"] @ ((np.eye(X.shape[0]) - r["K"] @ r["woodbury_inv"]) @ (r["K"] @ dg[i][:, 0]))
        assert abs(s @ dg[i][:, 0] - want) <= 1e-11 * (np.abs(s) @ np.abs(dg[i][:, 0]))


@pytest.mark.parametrize("name", STUDENT_CASES)
def test_restatement_gradient_against_central_differences_of_its_log_marginal(name):
    """the mode re-found at 1e-12 (and polished by full Newton steps) on either side; step and bound of the kernel-gradient
    test of tests/test_oracle_laplace.py"""
    g = LL.load(name)
    specs, X, Y = g["specs"], g["X"], g["Y"]
    theta = np.asarray(g["lik_theta"], float)
    ana = LL.inference(specs, X, Y, LL.make_likelihood(g), tol=1e-12, polish=3)["dL_dthetaL"]
    fd = np.zeros(2)
    for j in range(2):
        h = 1e-6 * max(1.0, abs(theta[j]))
        lm = []
        for sign in (1.0, -1.0):
            th = theta.copy()
            th[j] += sign * h
            lm.append(LL.inference(specs, X, Y, gpy_amd.StudentT(deg_free=th[1], sigma2=th[0]), tol=1e-12, polish=3)["lml"])
        fd[j] = (lm[0] - lm[1]) / (2 * h)
    assert np.abs(fd - ana).max() <= 1e-5 * max(1.0, np.abs(ana).max()), (fd, ana)


def test_host_bookkeeping():
    import gpy_amd as GPy
    assert GPy.likelihoods.StudentT is gpy_amd.StudentT and GPy.likelihoods.Poisson is gpy_amd.Poisson
    assert GPy.likelihoods.link_functions.Identity is gpy_amd.link_functions.Identity
    assert GPy.likelihoods.link_functions.Log is gpy_amd.link_functions.Log
    assert "mi355gp_laplace_implicit" in gpy_amd._lib.EXPORTED
    lik = GPy.likelihoods.StudentT(deg_free=5, sigma2=2)
    assert lik.parameter_names() == ["t_scale2", "deg_free"] and lik.param_array.tolist() == [2.0, 5.0]
    assert isinstance(lik.gp_link, GPy.likelihoods.link_functions.Identity)
    lik.update_gradients(np.array([3.0, -4.0]))
    assert lik.gradient.tolist() == [3.0, -4.0]
    d = lik.to_dict()
    assert d["class"] == "GPy.likelihoods.StudentT" and d["gp_link_dict"]["class"] == "GPy.likelihoods.link_functions.Identity"
    assert d["deg_free"] == [5.0] and d["t_scale2"] == [2.0]
    p = GPy.likelihoods.Poisson()
    assert isinstance(p.gp_link, GPy.likelihoods.link_functions.Log)
    assert p.to_dict() == {"class": "GPy.likelihoods.Poisson", "name": "Poisson",
                           "gp_link_dict": {"class": "GPy.likelihoods.link_functions.Log"}}
    assert p.check_targets(np.array([[0.0], [3.0], [12.0]])).shape == (3, 1)
    for bad in ([[0.5]], [[-1.0]]):
        with pytest.raises(AssertionError, match=r"only with outputs in \{0, 1, 2, \.\.\.\}"):
            p.check_targets(np.array(bad))
    s = lik.samples(np.zeros((6, 1)))
    assert s.shape == (6, 1) and np.isfinite(s).all()
    assert gpy_amd.Bernoulli().to_dict()["class"] == "GPy.likelihoods.Bernoulli"


class _Ctx(object):
    """a context that records the session calls and answers with the dense NumPy of tests/laplace_np.py"""
    made = []

    def __init__(self, device=0):
        self.calls = []
        _Ctx.made.append(self)

    def set_data(self, X, Y):
        self.X, self.N = np.array(X), X.shape[0]

    set_targets = set_data

    def laplace_begin(self, specs):
        self.K = 1.3 * np.exp(-0.5 * (self.X - self.X.T) ** 2) + 1e-6 * np.eye(self.N)

    def laplace_newton(self, W, b, extra_jitter=0.0):
        return (0,) + LP.newton(self.K, np.ravel(W), np.ravel(b))

    def laplace_finish(self, W, extra_jitter=0.0):
        d, logdet, self.KWi = LP.finish(self.K, np.ravel(W))
        return 0, d, logdet

    def laplace_gradients(self, Ki_f, dL_dfhat):
        return np.zeros(2)

    def laplace_implicit(self, dL_dfhat):
        self.calls.append("laplace_implicit")
        return LL.implicit_vector(self.K, self.KWi, np.ravel(dL_dfhat))


def test_laplace_takes_a_parameterised_likelihood_and_calls_the_device_once(monkeypatch):
    """fails on the parent commit, where a likelihood with parameters raised NotImplementedError (and had no class)"""
    monkeypatch.setattr(gpy_amd._lib, "Context", _Ctx)
    _Ctx.made = []
    rng = np.random.default_rng(8)
    X = np.sort(rng.uniform(-2, 2, (30, 1)), 0)
    Y = np.sin(2 * X) + 0.1 * rng.standard_normal(X.shape)
    lik = gpy_amd.StudentT(deg_free=4.0, sigma2=0.5)
    inf = gpy_amd.Laplace()
    inf._mode_finding_tolerance = 1e-10
    post, lml, gd = inf.inference(gpy_amd.RBF(1, 1.3, 1.0), X, lik, Y)
    ctx = _Ctx.made[-1]
    assert ctx.calls == ["laplace_implicit"]
    y = Y[:, 0]
    f = inf.f_hat[:, 0]
    want = LL.dL_dthetaL(lik, ctx.K, f, y, inf.diag_Ki_W_i, ctx.KWi, -0.5 * inf.diag_Ki_W_i * (-lik.d3logpdf_df3(f, y)))
    assert gd["dL_dthetaL"].shape == (2,) and np.allclose(gd["dL_dthetaL"], want, rtol=1e-10, atol=0.0)
    lik.is_fixed = True
    assert inf.inference(gpy_amd.RBF(1, 1.3, 1.0), X, lik, Y)[2]["dL_dthetaL"].tolist() == [0.0, 0.0]
    for none in (gpy_amd.Poisson(), gpy_amd.Bernoulli()):          # no parameters: nothing new is launched
        Yc = (Y > 0).astype(float)
        inf2 = gpy_amd.Laplace()
        assert inf2.inference(gpy_amd.RBF(1, 1.3, 1.0), X, none, Yc)[2]["dL_dthetaL"].shape == (0,)
        assert _Ctx.made[-1].calls == []
