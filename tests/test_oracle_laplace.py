"""CPU checks of the Laplace approximation: the NumPy restatement of the device split (tests/laplace_np.py) against every
fixture the reference's own `Laplace` + `Bernoulli` produced (tools/make_golden_laplace.py), its gradients against central
differences of its own log marginal, the Bernoulli likelihood against values stored from the reference, and the host
bookkeeping that needs no device."""
import os

import numpy as np
import pytest

import gpy_amd
import laplace_np as LP
import mlp_np as P


def test_the_cases_the_issue_names_are_there():
    assert len(LP.CASES) == 7
    for want in ("rbf_iso", "matern52_ard", "rbf_linear_bias", "mlp0_x_rbf12", "stdperiodic", "separated", "overlapping"):
        assert any(c.startswith(want) for c in LP.CASES), want
    for f in os.listdir(LP.GOLDEN):
        assert os.path.getsize(os.path.join(LP.GOLDEN, f)) < 1 << 19
    for c in LP.CASES:
        assert 120 <= LP.load(c)["X"].shape[0] <= 300


@pytest.mark.parametrize("name", LP.CASES)
def test_restatement_against_the_reference(name):
    g = LP.load(name)
    specs, X, Y, Xs = g["specs"], g["X"], g["Y"], g["Xs"]
    r = LP.inference(specs, X, Y)
    mu, var = LP.predict(specs, X, r, Xs)
    _, cov = LP.predict(specs, X, r, Xs, full_cov=True)
    got = dict(r, pred_mu=mu, pred_var=var, pred_cov=cov, pred_p=gpy_amd.Bernoulli().predictive_mean(mu, var))
    ref = dict(g, dL_dK=0.5 * (g["dL_dK"] + g["dL_dK"].T))          # the reference's dL_dK is not symmetric; its gradients see the symmetric part
    fig = {q: (abs(got[q] - ref[q]) / abs(ref[q]) if q == "lml" else LP.rel(got[q], ref[q])) for q in LP.STANDING}
    print(name, {q: "%.1e (tol %.1e)" % (fig[q], g["tol"][q]) for q in fig})
    for q in LP.STANDING:
        assert fig[q] <= g["tol"][q], (q, fig[q], g["tol"][q])


@pytest.mark.parametrize("name", LP.CASES)
def test_gradients_against_central_differences_of_the_log_marginal(name):
    g = LP.load(name)
    specs, X, Y = g["specs"], g["X"], g["Y"]
    dth = LP.inference(specs, X, Y, polish=True)["dtheta"]
    fd, k = np.zeros_like(dth), 0
    for i, s in enumerate(specs):
        for j in range(P.n_params(s)):
            h = 1e-6 * max(1.0, abs(s[2][j]))
            lm = []
            for sign in (1.0, -1.0):
                th = s[2].copy()
                th[j] += sign * h
                sp = list(specs)
                sp[i] = (s[0], s[1], th, s[3], s[4])
                lm.append(LP.inference(sp, X, Y, polish=True)["lml"])
            fd[k] = (lm[0] - lm[1]) / (2 * h)
            k += 1
    assert k == dth.size
    assert np.abs(fd - dth).max() <= 1e-5 * max(1.0, np.abs(dth).max())        # step and bound of tests/test_oracle_mlp.py


def test_bernoulli_against_values_stored_from_the_reference():
    z = np.load(os.path.join(LP.GOLDEN, "bernoulli_values.npz"))
    lik = gpy_amd.likelihoods.Bernoulli()
    f = z["f"]
    assert f.min() == -40.0 and f.max() == 40.0
    for yv in (0, 1):
        y = np.full_like(f, float(yv))
        for name in ("logpdf", "dlogpdf_df", "d2logpdf_df2", "d3logpdf_df3"):
            with np.errstate(all="ignore"):
                got = getattr(lik, name)(f, y)
            want = z["%s_y%d" % (name, yv)]
            assert np.array_equal(np.isnan(got), np.isnan(want)), (name, yv)
            ok = ~np.isnan(want)
            assert np.allclose(got[ok], want[ok], rtol=1e-13, atol=0.0), (name, yv, np.abs(got[ok] - want[ok]).max())
    assert np.allclose(lik.predictive_mean(f, z["pm_var"]), z["predictive_mean"], rtol=1e-14, atol=0.0)
    assert lik.log_concave is True and lik.size == 0
    assert np.isnan(lik.predictive_variance(f, z["pm_var"]))
    s = lik.samples(np.array([[-40.0], [40.0]]))
    assert s.tolist() == [[0], [1]]


def test_host_bookkeeping():
    X, Y = LP.two_class(30, 2, 1)
    with pytest.raises(NotImplementedError, match=r"EP.*inference_method=gpy_amd\.Laplace\(\)"):
        gpy_amd.GPClassification(X, Y)
    with pytest.raises(AssertionError, match="only with outputs in \\{0, 1\\}"):
        gpy_amd.GPClassification(X, 2.0 * Y - 1.0, inference_method=gpy_amd.Laplace())
    with pytest.raises(AssertionError, match="only with outputs in \\{0, 1\\}"):
        gpy_amd.Bernoulli.check_targets(np.array([[0.0], [0.5]]))
    inf = gpy_amd.Laplace()
    assert inf._mode_finding_tolerance == 1e-4 and inf._mode_finding_max_iter == 30
    with pytest.raises(AssertionError, match="mean function not implemented"):
        inf.inference(gpy_amd.RBF(2), X, gpy_amd.Bernoulli(), Y, mean_function=object())
    with pytest.raises(NotImplementedError, match="one output column"):
        inf.inference(gpy_amd.RBF(2), X, gpy_amd.Bernoulli(), np.hstack([Y, Y]))
    assert inf.to_dict()["class"] == "GPy.inference.latent_function_inference.laplace.Laplace"
    assert gpy_amd.Bernoulli().to_dict()["class"] == "GPy.likelihoods.Bernoulli"
    assert gpy_amd.Bernoulli().to_dict()["gp_link_dict"]["class"] == "GPy.likelihoods.link_functions.Probit"


def test_gpy_style_import_paths_of_the_new_names():
    import gpy_amd as GPy
    assert GPy.models.GPClassification is gpy_amd.GPClassification
    assert GPy.likelihoods.Bernoulli is gpy_amd.Bernoulli
    assert isinstance(GPy.likelihoods.Bernoulli().gp_link, GPy.likelihoods.link_functions.Probit)
    assert GPy.inference.latent_function_inference.Laplace is gpy_amd.Laplace
    assert GPy.inference.latent_function_inference.laplace.Laplace is gpy_amd.Laplace
    for sym in ("mi355gp_laplace_begin", "mi355gp_laplace_newton", "mi355gp_laplace_finish", "mi355gp_laplace_gradients",
                "mi355gp_laplace_predict"):
        assert sym in gpy_amd._lib.EXPORTED
