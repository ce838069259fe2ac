"""CPU checks of expectation propagation: the NumPy restatement of the device split (tests/ep_np.py) against every fixture the
reference's own `EP` + `Bernoulli` produced (tools/make_golden_ep.py), following the stored update orders; its kernel gradients
against central differences of its own log marginal at EP's fixed point; `Bernoulli.moments_match_ep` against values stored from
the reference; and the host bookkeeping that needs no device."""
import os

import numpy as np
import pytest

import gpy_amd
import ep_np as EP
import laplace_np as LP
import mlp_np as P


def test_the_cases_the_issue_names_are_there():
    seq = [c for c in EP.CASES if not EP.load(c)["parallel_updates"]]
    par = [c for c in EP.CASES if EP.load(c)["parallel_updates"]]
    for want in ("rbf_iso", "matern52_ard", "rbf_linear_bias", "mlp0_x_rbf12", "stdperiodic", "separated", "overlapping"):
        assert any(c.startswith(want) for c in seq), want
    assert len(par) >= 2
    assert any(EP.load(c)["eta"] == 0.9 and EP.load(c)["delta"] == 0.8 for c in EP.CASES)
    assert sum(1 for c in seq if not EP.load(c)["clamped"]) >= 5
    for f in os.listdir(EP.GOLDEN):
        assert os.path.getsize(os.path.join(EP.GOLDEN, f)) < 1 << 19
    for c in EP.CASES:
        g = EP.load(c)
        assert 120 <= g["X"].shape[0] <= 300 and 2 <= g["sweeps"] <= 100 and g["orders"].shape == (g["sweeps"], g["X"].shape[0])


@pytest.mark.parametrize("name", EP.CASES)
def test_restatement_against_the_reference(name):
    g = EP.load(name)
    specs, X, Y, Xs = g["specs"], g["X"], g["Y"], g["Xs"]
    r = EP.inference(specs, X, Y, orders=g["orders"], parallel=g["parallel_updates"], eta=g["eta"], delta=g["delta"],
                     epsilon=g["epsilon"])
    assert r["sweeps"] == g["sweeps"]
    mu, var = EP.predict(specs, X, r, Xs)
    _, cov = EP.predict(specs, X, r, Xs, full_cov=True)
    got = dict(r, pred_mu=mu, pred_var=var, pred_cov=cov, pred_p=gpy_amd.Bernoulli().predictive_mean(mu, var))
    fig = EP.figures(g, got)
    assert set(fig) == set(EP.STANDING)
    for q in fig:
        assert fig[q] <= g["tol"][q], (q, fig[q], g["tol"][q])


def _fixed_point(specs, X, Y):
    """EP run until the sites stop moving (parallel updates, damped so that every case settles): at the fixed point the
    derivative of the log marginal with the sites held fixed is its total derivative"""
    K, dKs = LP.expr(specs, X)
    e = EP.run(K, Y, parallel=True, delta=0.7, epsilon=1e-27, max_iters=2000)
    assert e["converged"], "parallel EP did not reach its fixed point"
    again = EP.parallel_sweep(*EP.recompute(K, e["tau"], e["v"], 0.0, False)[:2], EP.ysign(Y), 1.0, 1.0, e["tau"], e["v"])
    assert np.abs(again["tau"] - e["tau"]).max() < 1e-12 and np.abs(again["v"] - e["v"]).max() < 1e-12
    return EP.final(K, dKs, e)


@pytest.mark.parametrize("name", [c for c in EP.CASES if not c.startswith(("parallel", "fractional"))])
def test_gradients_against_central_differences_of_the_log_marginal(name):
    g = EP.load(name)
    specs, X, Y = g["specs"], g["X"], g["Y"]
    dth = _fixed_point(specs, X, Y)["dtheta"]
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
                lm.append(_fixed_point(sp, X, Y)["lml"])
            fd[k] = (lm[0] - lm[1]) / (2 * h)
            k += 1
    assert k == dth.size
    err = np.abs(fd - dth).max() / max(1.0, np.abs(dth).max())
    print(name, "central differences against the fixed-point gradient: %.2e" % err)
    assert err <= 1e-5                                          # step and bound of tests/test_oracle_laplace.py


def test_moments_against_values_stored_from_the_reference():
    z = np.load(os.path.join(EP.GOLDEN, "bernoulli_ep_moments.npz"))
    lik = gpy_amd.Bernoulli()
    tau, v = z["tau"], z["v"]
    assert tau.min() == 1e-8 and tau.max() == 1e4 and (v / tau).min() <= -40.0 + 1e-9 and (v / tau).max() >= 40.0 - 1e-9
    for yv in (0, 1):
        got = dict(zip(("log_Z_hat", "mu_hat", "sigma2_hat"), lik.log_moments_match_ep(np.full(tau.shape, float(yv)), tau, v)))
        mine = dict(zip(("log_Z_hat", "mu_hat", "sigma2_hat"), EP.log_moments(1.0 if yv else -1.0, tau, v)))
        for q in got:
            want, bound = z["%s_y%d" % (q, yv)], 10.0 * float(z["ref_vs_scipy_" + q])
            assert np.isfinite(got[q]).all(), (q, yv)
            for name, a in (("gpy_amd", got[q]), ("ep_np", mine[q])):
                err = np.max(np.abs(a - want) / np.where(want != 0, np.abs(want), 1.0))
                print("%s %s y=%d: %.2e (bound %.2e)" % (name, q, yv, err, bound))
                assert err <= bound, (name, q, yv, err, bound)
    Z, mu_hat, s2 = lik.moments_match_ep(1, 2.0, 0.3)                   # scalars, as the reference's sweep calls it
    lz, mu2, s22 = lik.log_moments_match_ep(1, 2.0, 0.3)
    assert Z == np.exp(lz) and mu_hat == mu2 and s2 == s22 and 0.0 < Z < 1.0
    with pytest.raises(ValueError, match="bad value for Bernoulli observation"):
        lik.moments_match_ep(0.5, 1.0, 0.0)
    assert lik.ep_gradients(None, None, None, None).shape == (0,)


def test_host_bookkeeping():
    X, Y = LP.two_class(30, 2, 1)
    with pytest.raises(NotImplementedError) as e:
        gpy_amd.GPClassification(X, Y)
    msg = str(e.value)
    assert "inference_method=gpy_amd.EP()" in msg and "inference_method=gpy_amd.Laplace()" in msg and "explicit" in msg
    assert "does not implement" not in msg
    inf = gpy_amd.EP()
    assert (inf.epsilon, inf.eta, inf.delta, inf.always_reset, inf.max_iters, inf.ep_mode, inf.parallel_updates) == (
        1e-6, 1.0, 1.0, False, np.inf, "alternated", False)
    d = inf.to_dict()
    assert d["class"] == "GPy.inference.latent_function_inference.expectation_propagation.EP"
    assert d["ep_mode"] == "alternated" and "ga_approx_old" not in d and "_ep_approximation" not in d
    # reset / on_optimization_start / warm start bookkeeping on hand-made state
    from gpy_amd.ep import cavityParams, gaussianApproximation, posteriorParams
    ga = gaussianApproximation(np.arange(3.0), np.ones(3))
    cav = cavityParams(3)
    cav.tau[:], cav.v[:] = 1.0, 2.0
    inf.ga_approx_old = ga
    inf._ep_approximation = (posteriorParams(np.zeros(3), np.ones(3)), ga, cav, -1.5)
    d = inf.to_dict()
    assert d["ga_approx_old"] == {"tau": [1.0, 1.0, 1.0], "v": [0.0, 1.0, 2.0]}
    assert set(d["_ep_approximation"]["post_params"]) == {"mu", "Sigma_diag"}           # no N x N member
    assert d["_ep_approximation"]["log_Z_tilde"] == -1.5
    import json
    json.dumps(d)
    inf.on_optimization_start()
    assert inf._ep_approximation is None and inf.ga_approx_old is ga                   # the sites survive: warm start
    inf.reset()
    assert inf.ga_approx_old is None
    inf.ga_approx_old = gaussianApproximation(np.zeros(3), np.zeros(3))
    other = gaussianApproximation(np.full(3, 1e-4), np.zeros(3))
    inf.epsilon = 1e-6
    assert inf._stop_criteria(other) and not inf._stop_criteria(gaussianApproximation(np.ones(3), np.zeros(3)))
    # the sentences for what this path does not take (all raised before any device call)
    k, lik = gpy_amd.RBF(2), gpy_amd.Bernoulli()
    for kwargs, match in ((dict(mean_function=object()), "mean function"), (dict(precision=np.ones(30)), "precision="),
                          (dict(K=np.eye(30)), "K=")):
        with pytest.raises(NotImplementedError, match=match):
            gpy_amd.EP().inference(k, X, lik, Y, **kwargs)
    with pytest.raises(NotImplementedError, match="one output column"):
        gpy_amd.EP().inference(k, X, lik, np.hstack([Y, Y]))
    with pytest.raises(NotImplementedError, match="Bernoulli likelihood only"):
        gpy_amd.EP().inference(k, X, gpy_amd.Gaussian(), Y)

    other_link = gpy_amd.Bernoulli()
    other_link.gp_link = type("Heaviside", (), {})()
    with pytest.raises(NotImplementedError, match="probit link only"):
        gpy_amd.EP().inference(k, X, other_link, Y)
    with pytest.raises(ValueError, match="ep_mode value not valid"):
        gpy_amd.EP(ep_mode="sometimes").inference(k, X, lik, Y)


def test_gpy_style_import_paths_of_the_new_names():
    import gpy_amd as GPy
    assert GPy.inference.latent_function_inference.EP is gpy_amd.EP
    assert GPy.inference.latent_function_inference.expectation_propagation.EP is gpy_amd.EP
    assert GPy.inference.latent_function_inference.posterior.PosteriorEP is gpy_amd.PosteriorEP
    assert issubclass(gpy_amd.PosteriorEP, gpy_amd.PosteriorExact)
    for sym in ("mi355gp_ep_recompute", "mi355gp_ep_sweep"):
        assert sym in gpy_amd._lib.EXPORTED
    assert gpy_amd._lib.EP_BERNOULLI_PROBIT == 0
