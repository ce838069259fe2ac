"""GPU checks of expectation propagation (C-ABI mi355gp_ep_recompute / mi355gp_ep_sweep inside a Laplace session, gpy_amd.EP,
gpy_amd.GPClassification) against the fixtures the reference's own code produced (tools/make_golden_ep.py), following the
stored update orders, and against the NumPy restatement run live (tests/ep_np.py).

Tolerances against a fixture are max(standing tolerance, 10 x the reference's own rounding floor stored in it), as tests/ep_np.py
states them; the number of sweeps must be equal outright.  Against the restatement, which is driven through the very same
(tau, v) and order, one recompute and one sweep are compared at the standing tolerances."""
import os
import signal

import numpy as np
import pytest

import gpy_amd
from gpy_amd import _lib as L
import ep_np as EP
import laplace_np as LP
import mlp_np as P

pytestmark = pytest.mark.gpu
LIMIT_S = 420


@pytest.fixture(autouse=True)
def _time_limit():
    def stop(signum, frame):
        raise TimeoutError("test exceeded its %d s limit" % LIMIT_S)
    old = signal.signal(signal.SIGALRM, stop)
    signal.alarm(LIMIT_S)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def _session(ctx, specs, Y, orders=None, parallel=False, eta=1.0, delta=1.0, epsilon=1e-6, max_iters=100, seed=0):
    """`expectation_propagation` and the final pass through the raw session calls: the result dict of ep_np.final"""
    n = Y.shape[0]
    sign = EP.ysign(Y)
    rng = np.random.default_rng(seed)
    ctx.laplace_begin(P.cabi_specs(specs))
    tau, v = np.zeros(n), np.zeros(n)
    info, mu, sd, _ = ctx.ep_recompute(tau, v, add_diag=1e-7, want_sigma=not parallel)
    assert info == 0
    stop, it, old = False, 0, None
    while not stop and it < max_iters:
        if parallel:
            r = EP.parallel_sweep(mu, sd, sign, eta, delta, tau, v)
        else:
            r = ctx.ep_sweep(orders[it] if orders is not None else rng.permutation(n), sign, tau, v, eta, delta)
        tau, v = r["tau"], r["v"]
        info, mu, sd, _ = ctx.ep_recompute(tau, v, want_sigma=not parallel)
        assert info == 0
        if it > 0:
            stop = bool(np.mean(np.square(tau - old[0])) < epsilon and np.mean(np.square(v - old[1])) < epsilon)
        old = (tau.copy(), v.copy())
        it += 1
    lzt = EP.log_Z_tilde(r["log_Z_hat"], tau, v, r["cav_tau"], r["cav_v"])
    info, alpha, mu, logdet = ctx.laplace_newton(tau, v)
    assert info == 0
    lml = 0.5 * (-n * np.log(2 * np.pi) - logdet + np.dot(v, mu)) + lzt
    assert ctx.laplace_finish(tau)[0] == 0
    dtheta = ctx.laplace_gradients(alpha, np.zeros(n))
    return dict(lml=lml, log_Z_tilde=lzt, tau_tilde=tau, v_tilde=v, cav_tau=r["cav_tau"], cav_v=r["cav_v"], alpha=alpha[:, None],
                dtheta=dtheta, sweeps=it)


@pytest.mark.parametrize("name", EP.CASES)
def test_session_calls_against_the_reference(name):
    g = EP.load(name)
    specs, X, Y, Xs = g["specs"], g["X"], g["Y"], g["Xs"]
    ctx = L.Context()
    ctx.set_data(X, Y)
    r = _session(ctx, specs, Y, g["orders"], g["parallel_updates"], g["eta"], g["delta"], g["epsilon"])
    assert r["sweeps"] == g["sweeps"]
    mu, var = ctx.laplace_predict(P.cabi_specs(specs), Xs, r["alpha"])
    _, cov = ctx.laplace_predict(P.cabi_specs(specs), Xs, r["alpha"], full_cov=True)
    got = dict(r, dtheta=P.gpy_dtheta(specs, r["dtheta"]), dL_dK=ctx.fetch(L.FETCH_DLDK), Wi=ctx.fetch(L.FETCH_KINV), pred_mu=mu,
               pred_var=var, pred_cov=cov, pred_p=gpy_amd.Bernoulli().predictive_mean(mu, var))
    fig = EP.figures(g, got)
    assert set(fig) == set(EP.STANDING)
    for q in fig:
        assert fig[q] <= g["tol"][q], (q, fig[q], g["tol"][q])


class _StoredOrders(gpy_amd.EP):
    """feeds a fixture's update orders through the `update_order` hook of `_local_updates`"""
    orders = None

    def _local_updates(self, *args, **kwargs):
        kwargs["update_order"] = self.orders[self._k]
        self._k += 1
        return super(_StoredOrders, self)._local_updates(*args, **kwargs)

    def expectation_propagation(self, *args, **kwargs):
        self._k = 0
        return super(_StoredOrders, self).expectation_propagation(*args, **kwargs)


@pytest.mark.parametrize("name", EP.CASES)
def test_model_against_the_reference(name):
    g = EP.load(name)
    specs, X, Y, Xs = g["specs"], g["X"], g["Y"], g["Xs"]
    inf = _StoredOrders(epsilon=g["epsilon"], eta=g["eta"], delta=g["delta"], max_iters=100, parallel_updates=g["parallel_updates"])
    inf.orders = g["orders"]
    m = gpy_amd.GPClassification(X, Y, kernel=LP.gpy_amd_kernel(specs), inference_method=inf)
    assert inf.iterations == g["sweeps"]
    mu, var = m.predict_noiseless(Xs)
    p, _ = m.predict(Xs)
    _, cov = m._raw_predict(Xs, full_cov=True)
    _, ga, cav, lzt = inf._ep_approximation
    assert isinstance(m.posterior, gpy_amd.PosteriorEP) and m.grad_dict["dL_dthetaL"].shape == (0,)
    assert np.array_equal(m.grad_dict["dL_dm"], m.posterior.woodbury_vector)
    got = dict(lml=m.log_likelihood(), log_Z_tilde=lzt, tau_tilde=ga.tau, v_tilde=ga.v, cav_tau=cav.tau, cav_v=cav.v,
               alpha=m.posterior.woodbury_vector, dtheta=m.gradient, pred_mu=mu, pred_var=var, pred_cov=cov, pred_p=p,
               Wi=np.asarray(m.posterior.woodbury_inv), dL_dK=np.asarray(m.grad_dict["dL_dK"]))
    fig = EP.figures(g, got)
    assert set(fig) == set(EP.STANDING)
    for q in fig:
        assert fig[q] <= g["tol"][q], (q, fig[q], g["tol"][q])


def _nontrivial_sites(X, Y):
    """site parameters of the size EP reaches, away from the cold start"""
    tau = 0.05 + 0.3 / (1.0 + X[:, 0] ** 2)
    return tau, EP.ysign(Y) * tau * (0.5 + 0.2 * np.cos(X[:, 1]))


@pytest.mark.parametrize("N", [129, 1300, 4096, 6500])
def test_recompute_and_sweep_against_the_restatement_live(N):
    """padding (129, 1300, 6500) and both factorisation schedules (4096: persistent launch, 6500: launch per step): the same
    (tau, v) and the same order through the device and through NumPy; at 6500 the recompute alone"""
    X, Y = LP.two_class(N, 3, 170 + N)
    specs = [("rbf", 1, np.array([1.4, 1.1, 0.8, 1.5]), np.arange(3), 0), ("bias", 0, np.array([0.2]), np.arange(3), 0)]
    K = LP.expr(specs, X)[0]
    tau, v = _nontrivial_sites(X, Y)
    ctx = L.Context()
    ctx.set_data(X, Y)
    ctx.laplace_begin(P.cabi_specs(specs))
    info, mu, sd, logdet = ctx.ep_recompute(tau, v, add_diag=1e-7, want_sigma=True)
    mu0, sd0, logdet0, Sigma = EP.recompute(K, tau, v, 1e-7, True)
    assert info == 0
    fig = dict(mu=LP.rel(mu, mu0), sd=LP.rel(sd, sd0), logdet=abs(logdet - logdet0) / abs(logdet0))
    info, mu1, sd1, _ = ctx.ep_recompute(tau, v, add_diag=1e-7, want_sigma=False)          # the diagonal alone (colsumsq path)
    assert info == 0
    fig.update(mu_diag_only=LP.rel(mu1, mu0), sd_diag_only=LP.rel(sd1, sd0))
    if N <= 4096:
        assert ctx.ep_recompute(tau, v, add_diag=1e-7, want_sigma=True)[0] == 0
        order = np.random.default_rng(N).permutation(N)
        r = ctx.ep_sweep(order, EP.ysign(Y), tau, v, 0.9, 0.8)
        r0 = EP.sweep(Sigma, mu0, order, EP.ysign(Y), 0.9, 0.8, tau, v)
        fig.update({q: LP.rel(r[q], r0[q]) for q in r0})
        assert np.abs(r["tau"] - tau).max() > 1e-3                                        # the sweep moved the sites
    print(N, fig)
    assert fig.pop("logdet") <= 1e-10
    assert max(fig.values()) <= 1e-9, fig


def test_repeated_runs_give_the_same_bits_and_regression_is_untouched():
    X, Y = LP.two_class(700, 3, 9)
    Yr = np.sin(X[:, :1]) + 0.1 * X[:, 1:2]
    specs = [("rbf", 1, np.array([1.4, 1.1, 0.8, 1.5]), np.arange(3), 0)]
    ctx = L.Context()
    ctx.set_data(X, Yr)

    def regression():
        rc, r = ctx.exact_inference_sum(P.cabi_specs(specs), 0.1, want_diag=True)
        assert rc == 0
        return np.float64(r["lml"]).tobytes() + r["alpha"].tobytes() + r["dtheta"].tobytes()
    before = [regression() for _ in range(3)]
    ctx.set_targets(Y)
    runs = [_session(ctx, specs, Y, seed=5) for _ in range(3)]
    assert runs[0]["sweeps"] >= 2
    for r in runs[1:]:
        assert r["sweeps"] == runs[0]["sweeps"]
        for q in ("tau_tilde", "v_tilde", "cav_tau", "cav_v", "alpha", "dtheta"):
            assert r[q].tobytes() == runs[0][q].tobytes(), q
        assert np.float64(r["lml"]).tobytes() == np.float64(runs[0]["lml"]).tobytes()
    ctx.set_targets(Yr)
    after = [regression() for _ in range(3)]
    assert all(a == before[0] for a in before + after)


@pytest.mark.parametrize("name", [c for c in EP.CASES if not c.startswith(("parallel", "fractional"))])
def test_parallel_and_sequential_updates_agree_at_the_fixed_point(name):
    g = EP.load(name)
    specs, X, Y = g["specs"], g["X"], g["Y"]
    ctx = L.Context()
    ctx.set_data(X, Y)
    seq = _session(ctx, specs, Y, epsilon=1e-24, max_iters=300, seed=1)
    par = _session(ctx, specs, Y, parallel=True, delta=0.7, epsilon=1e-24, max_iters=2000)
    err = abs(seq["lml"] - par["lml"]) / abs(par["lml"])
    print(name, "sweeps %d / %d, log marginal %.15e / %.15e: %.1e (tol %.1e)" % (seq["sweeps"], par["sweeps"], seq["lml"], par["lml"],
                                                                                 err, g["tol"]["lml"]))
    assert seq["sweeps"] < 300 and par["sweeps"] < 2000
    assert err <= g["tol"]["lml"]


def test_optimize_on_the_example_data():
    z = np.load(os.path.join(EP.GOLDEN, "toy_1d_optimize.npz"))
    np.random.seed(2)
    m = gpy_amd.GPClassification(z["X"], z["Y"], inference_method=gpy_amd.EP(ep_mode="alternated"))
    start = m.log_likelihood()
    assert abs(start - float(z["lml_start"])) <= 1e-3 * abs(float(z["lml_start"]))     # shipped epsilon 1e-6, another order
    m.optimize()
    p, _ = m.predict(z["X"])
    acc = float(np.mean((p > 0.5) == (z["Y"] == 1)))
    print("lml %.6f -> %.6f (reference %.6f -> %.6f), accuracy %.4f (reference %.4f)" % (
        start, m.log_likelihood(), float(z["lml_start"]), float(z["lml_end"]), acc, float(z["accuracy"])))
    assert m.log_likelihood() > start
    assert acc >= float(z["accuracy"])
    f = m.posterior_samples_f(z["X"][:5], size=3)
    assert f.shape == (5, 1, 3) and np.isfinite(f).all()
    for call in (lambda: m.predictive_gradients(z["X"][:3]), lambda: m.log_predictive_density(z["X"][:3], z["Y"][:3]),
                 lambda: m.predict_quantiles(z["X"][:3]), lambda: m.posterior_covariance_between_points(z["X"][:3], z["X"][:3])):
        with pytest.raises(NotImplementedError):
            call()
    nested = gpy_amd.GPClassification(z["X"], z["Y"], inference_method=gpy_amd.EP(ep_mode="nested", parallel_updates=True, max_iters=50))
    assert abs(nested.log_likelihood() - float(z["lml_start"])) <= 1e-3 * abs(float(z["lml_start"]))


def test_error_paths_return_a_message():
    X, Y = LP.two_class(200, 2, 11)
    specs = P.cabi_specs([("rbf", 0, np.array([1.0, 1.0]), np.arange(2), 0)])
    ctx = L.Context()
    ctx.set_data(X, Y)
    tau, v, sign, order = np.full(200, 0.3), np.full(200, 0.1), EP.ysign(Y), np.arange(200)
    with pytest.raises(L.MI355GPError, match="mi355gp_laplace_begin first"):
        ctx.ep_recompute(tau, v)
    ctx.laplace_begin(specs)
    with pytest.raises(L.MI355GPError, match="mi355gp_ep_recompute with want_sigma first"):
        ctx.ep_sweep(order, sign, tau, v)
    assert ctx.ep_recompute(tau, v, want_sigma=False)[0] == 0
    with pytest.raises(L.MI355GPError, match="mi355gp_ep_recompute with want_sigma first"):
        ctx.ep_sweep(order, sign, tau, v)
    assert ctx.ep_recompute(tau, v, want_sigma=True)[0] == 0
    twice = order.copy()
    twice[5] = 6
    with pytest.raises(L.MI355GPError, match="not a permutation"):
        ctx.ep_sweep(twice, sign, tau, v)
    bad = tau.copy()
    bad[17] = np.nan
    with pytest.raises(L.MI355GPError, match="tau is NaN"):
        ctx.ep_sweep(order, sign, bad, v)
    with pytest.raises(L.MI355GPError, match="tau is NaN"):
        ctx.ep_recompute(bad, v)
    assert ctx.ep_recompute(tau, v, want_sigma=True)[0] == 0
    with pytest.raises(L.MI355GPError, match="unknown likelihood 7"):
        ctx.ep_sweep(order, sign, tau, v, lik=7)
    r = ctx.ep_sweep(order, sign, tau, v)                                                  # the session is still usable
    assert np.isfinite(r["tau"]).all() and np.isfinite(r["mu"]).all()
    assert ctx.laplace_newton(tau, v)[0] == 0
    with pytest.raises(L.MI355GPError, match="mi355gp_ep_recompute with want_sigma first"):   # newton overwrote Sigma
        ctx.ep_sweep(order, sign, tau, v)
