"""GPU checks of the Laplace session (C-ABI mi355gp_laplace_*, gpy_amd.Laplace, gpy_amd.GPClassification) against the fixtures
the reference's own code produced (tools/make_golden_laplace.py) and against the NumPy restatement run live (tests/laplace_np.py).

Tolerances against a fixture are max(standing tolerance, 10 x the reference's own convergence floor stored in it), as
tests/laplace_np.py states them.  Against the restatement, which is driven through the very same W and b, one Newton step is
compared at the standing tolerances."""
import os
import signal

import numpy as np
import pytest

import gpy_amd
from gpy_amd import _lib as L
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


def _session(ctx, specs, Y, tol=1e-10, max_iter=100):
    """the mode search of gpy_amd.Laplace through the raw session calls: (f_hat, Ki_fhat, lml, dtheta, iterations)"""
    lik = gpy_amd.Bernoulli()
    ctx.laplace_begin(P.cabi_specs(specs))
    y = Y[:, 0]
    Ki_f, f = np.zeros_like(y), np.zeros_like(y)

    def obj(Ki_f, f):
        return -0.5 * np.dot(Ki_f, f) + np.sum(lik.logpdf(f, y))
    diff, it = np.inf, 0
    while diff > tol and it < max_iter:
        W = -lik.d2logpdf_df2(f, y)
        info, a, Ka, _ = ctx.laplace_newton(W, W * f + lik.dlogpdf_df(f, y))
        assert info == 0
        dKi_f, Kd = a - Ki_f, Ka - f
        s = LP.line_step(obj, Ki_f, f, dKi_f, Kd)
        new = (Ki_f + s * dKi_f, f + s * Kd)
        diff = abs(obj(*new) - obj(Ki_f, f))
        Ki_f, f = new
        it += 1
    W = -lik.d2logpdf_df2(f, y)
    info, d, logdet = ctx.laplace_finish(W)
    assert info == 0
    lml = -0.5 * np.dot(Ki_f, f) + np.sum(lik.logpdf(f, y)) - 0.5 * logdet
    dtheta = ctx.laplace_gradients(Ki_f, -0.5 * d * (-lik.d3logpdf_df3(f, y)))
    return f[:, None], Ki_f[:, None], lml, dtheta, it


def _figures(g, got):
    ref = dict(g, dL_dK=0.5 * (g["dL_dK"] + g["dL_dK"].T))
    fig = {q: (abs(got[q] - ref[q]) / abs(ref[q]) if q == "lml" else LP.rel(got[q], ref[q])) for q in got}
    print({q: "%.1e (tol %.1e)" % (fig[q], g["tol"][q]) for q in fig})
    return fig


@pytest.mark.parametrize("name", LP.CASES)
def test_session_calls_against_the_reference(name):
    g = LP.load(name)
    specs, X, Y, Xs = g["specs"], g["X"], g["Y"], g["Xs"]
    ctx = L.Context()
    ctx.set_data(X, Y)
    f, Ki_f, lml, dtheta, _ = _session(ctx, specs, Y)
    mu, var = ctx.laplace_predict(P.cabi_specs(specs), Xs, Ki_f)
    _, cov = ctx.laplace_predict(P.cabi_specs(specs), Xs, Ki_f, full_cov=True)
    got = dict(lml=lml, f_hat=f, Ki_fhat=Ki_f, dtheta=P.gpy_dtheta(specs, dtheta), dL_dK=ctx.fetch(L.FETCH_DLDK),
               woodbury_inv=ctx.fetch(L.FETCH_KINV), pred_mu=mu, pred_var=var, pred_cov=cov,
               pred_p=gpy_amd.Bernoulli().predictive_mean(mu, var))
    assert np.abs(ctx.fetch(L.FETCH_K) - LP.expr(specs, X)[0]).max() <= 1e-13 * LP.Kdiag(specs, X).max()
    fig = _figures(g, got)
    for q in fig:
        assert fig[q] <= g["tol"][q], (q, fig[q], g["tol"][q])


@pytest.mark.parametrize("name", LP.CASES)
def test_model_against_the_reference(name):
    g = LP.load(name)
    specs, X, Y, Xs = g["specs"], g["X"], g["Y"], g["Xs"]
    inf = gpy_amd.Laplace()
    inf._mode_finding_tolerance, inf._mode_finding_max_iter = 1e-10, 100
    m = gpy_amd.GPClassification(X, Y, kernel=LP.gpy_amd_kernel(specs), inference_method=inf)
    mu, var = m.predict_noiseless(Xs)
    p, _ = m.predict(Xs)
    _, cov = m._raw_predict(Xs, full_cov=True)
    got = dict(lml=m.log_likelihood(), f_hat=inf.f_hat, Ki_fhat=m.posterior.woodbury_vector, dtheta=m.gradient, pred_mu=mu,
               pred_var=var, pred_cov=cov, pred_p=p, woodbury_inv=np.asarray(m.posterior.woodbury_inv),
               dL_dK=np.asarray(m.grad_dict["dL_dK"]))
    fig = _figures(g, got)
    for q in fig:
        assert fig[q] <= g["tol"][q], (q, fig[q], g["tol"][q])


@pytest.mark.parametrize("N", [129, 1300, 4096, 6500])
def test_one_session_against_the_restatement_live(N):
    """padding (129, 1300, 6500) and both factorisation schedules (4096: persistent launch, 6500: launch per step): the same W, b
    through the device and through NumPy"""
    X, Y = LP.two_class(N, 3, 70 + N)
    specs = [("rbf", 1, np.array([1.4, 1.1, 0.8, 1.5]), np.arange(3), 0), ("bias", 0, np.array([0.2]), np.arange(3), 0)]
    lik, y = gpy_amd.Bernoulli(), Y[:, 0]
    K, dKs = LP.expr(specs, X)
    ctx = L.Context()
    ctx.set_data(X, Y)
    ctx.laplace_begin(P.cabi_specs(specs))
    f = 0.3 * np.sin(X[:, 0])
    W = -lik.d2logpdf_df2(f, y)
    b = W * f + lik.dlogpdf_df(f, y)
    info, a, Ka, logdet = ctx.laplace_newton(W, b)
    a0, Ka0, logdet0 = LP.newton(K, W, b)
    assert info == 0
    fig = dict(a=LP.rel(a, a0), Ka=LP.rel(Ka, Ka0), logdet=abs(logdet - logdet0) / abs(logdet0))
    info, d, ld2 = ctx.laplace_finish(W)
    d0, ld0, KWi = LP.finish(K, W)
    s = -0.5 * d0 * (-lik.d3logpdf_df3(f, y))
    dth = ctx.laplace_gradients(a0, s)
    G0 = LP.dL_dK_sym(K, a0, s, KWi)
    dth0 = np.array([np.sum(G0 * dK) for dK in dKs])
    fig.update(diag=LP.rel(d, d0), logdet2=abs(ld2 - ld0) / abs(ld0), dtheta=np.abs(dth - dth0).max() / np.abs(dth0).max())
    if N <= 1300:
        fig.update(dLdK=LP.rel(ctx.fetch(L.FETCH_DLDK), G0), KWi=LP.rel(ctx.fetch(L.FETCH_KINV), KWi))
    print(N, fig)
    assert info == 0
    assert max(fig["a"], fig["Ka"], fig["diag"], fig.get("KWi", 0.0)) <= 1e-9
    assert max(fig["logdet"], fig["logdet2"]) <= 1e-10
    assert max(fig["dtheta"], fig.get("dLdK", 0.0)) <= 1e-8


def test_checkgrad_of_a_three_part_kernel():
    X, Y = LP.two_class(300, 2, 5)
    k = gpy_amd.RBF(2, 1.3, 0.9) + gpy_amd.Linear(2, 0.4) + gpy_amd.Bias(2, 0.3)
    inf = gpy_amd.Laplace()
    inf._mode_finding_tolerance, inf._mode_finding_max_iter = 1e-12, 100
    m = gpy_amd.GPClassification(X, Y, kernel=k, inference_method=inf)
    np.random.seed(3)
    assert m.checkgrad(verbose=True, step=1e-4)


def test_repeated_calls_give_the_same_bits_and_regression_is_untouched():
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
    runs = [_session(ctx, specs, Y) for _ in range(3)]
    for r in runs[1:]:
        assert r[4] == runs[0][4]
        assert r[0].tobytes() == runs[0][0].tobytes() and r[1].tobytes() == runs[0][1].tobytes()
        assert np.float64(r[2]).tobytes() == np.float64(runs[0][2]).tobytes() and r[3].tobytes() == runs[0][3].tobytes()
    ctx.set_targets(Yr)
    after = [regression() for _ in range(3)]
    assert all(a == before[0] for a in before + after)


def test_optimize_on_the_example_data():
    z = np.load(os.path.join(LP.GOLDEN, "toy_1d_optimize.npz"))
    m = gpy_amd.GPClassification(z["X"], z["Y"], inference_method=gpy_amd.Laplace())
    start = m.log_likelihood()
    assert abs(start - float(z["lml_start"])) <= 1e-3 * abs(float(z["lml_start"]))     # shipped mode tolerance 1e-4 on both sides
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
                 lambda: m.predict_quantiles(z["X"][:3])):
        with pytest.raises(NotImplementedError):
            call()


def test_error_paths_return_a_message():
    X, Y = LP.two_class(200, 2, 11)
    specs = P.cabi_specs([("rbf", 0, np.array([1.0, 1.0]), np.arange(2), 0)])
    ctx = L.Context()
    ctx.set_data(X, Y)
    W = np.full(200, 0.3)
    with pytest.raises(L.MI355GPError, match="mi355gp_laplace_begin first"):
        ctx.laplace_newton(W, W)
    ctx.laplace_begin(specs)
    bad = W.copy()
    bad[17] = np.nan
    with pytest.raises(L.MI355GPError, match="W is NaN"):
        ctx.laplace_newton(bad, W)
    with pytest.raises(L.MI355GPError, match="mi355gp_laplace_finish first"):
        ctx.laplace_gradients(W, W)
    with pytest.raises(L.MI355GPError, match="not available at this stage"):
        ctx.fetch(L.FETCH_L)
    assert ctx.laplace_newton(W, W)[0] == 0                       # the session is still usable
    ctx2 = L.Context()
    ctx2.set_data(X, np.hstack([Y, Y]))
    with pytest.raises(L.MI355GPError, match="one output column"):
        ctx2.laplace_begin(specs)
    with pytest.raises(ValueError, match=r"One or more element\(s\) of W is NaN"):
        class NaNLik(gpy_amd.Bernoulli):
            def d2logpdf_df2(self, f, y, Y_metadata=None):
                return np.full_like(f, np.nan)
        gpy_amd.Laplace().inference(gpy_amd.RBF(2), X, NaNLik(), Y)
