"""GPU checks of the Student-t and Poisson likelihoods under the Laplace approximation (gpy_amd.StudentT, gpy_amd.Poisson,
C-ABI mi355gp_laplace_implicit) against the fixtures the reference's own code produced (tools/make_golden_laplace_lik.py) and
against the dense NumPy restatement (tests/laplace_lik_np.py).

Tolerances against a fixture are those of tests/laplace_lik_np.py: max(standing tolerance of tests/test_gpu_laplace.py, 10 x the
reference's own floor stored in the fixture); dL_dthetaL and the Poisson predictive moments as explained there."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gpy_amd
from gpy_amd import _lib as L
import laplace_np as LP
import laplace_lik_np as LL
import mlp_np as P

pytestmark = pytest.mark.gpu
RBF = [("rbf", 0, np.array([1.3, 0.8]), np.arange(2), 0)]


def _data(N, seed=0):
    rng = np.random.default_rng(100 + N + seed)
    X = rng.standard_normal((N, 2))
    return X, (np.sin(X[:, :1]) + 0.3 * rng.standard_normal((N, 1)))


def _implicit(N, twice=True):
    """(s from the device, the dense s, its scale) for an RBF K, a Student-t W at a trial f and a random dL_dfhat"""
    X, Y = _data(N)
    lik = gpy_amd.StudentT(deg_free=6.0, sigma2=8.0)            # W > 0 for residuals below sqrt(48)
    f, y = 0.3 * np.sin(X[:, 0]), Y[:, 0]
    W = -lik.d2logpdf_df2(f, y)
    assert W.min() > 0
    u = np.random.default_rng(N).standard_normal(N)
    ctx = L.Context()
    ctx.set_data(X, Y)
    ctx.laplace_begin(P.cabi_specs(RBF))
    info, _, _ = ctx.laplace_finish(W)
    assert info == 0
    s = ctx.laplace_implicit(u)
    if twice:
        assert ctx.laplace_implicit(u).tobytes() == s.tobytes()
        ctx.laplace_gradients(u, u)                           # dL_dK resident: the vector is the same afterwards
        assert ctx.laplace_implicit(u).tobytes() == s.tobytes()
    K = LP.expr(RBF, X)[0]
    KWi = LP.finish(K, W)[2]
    Ku = K @ u
    scale = np.abs(K) @ (np.abs(u) + np.abs(KWi) @ np.abs(Ku))    # sum of the absolute values of the terms of each entry
    return s, LL.implicit_vector(K, KWi, u), scale


@pytest.mark.parametrize("N", [1, 63, 127, 128, 129, 257])
def test_implicit_vector_at_padding_edges(N):
    """against the dense K (u - K_Wi_i K u); an entry is a sum of about 3 N products, so it may differ from the dense one by
    3 N eps times the sum of the absolute values of its terms (10 x that is allowed, and never less than the 1e-9 of the
    session's other vectors)"""
    s, s0, scale = _implicit(N)
    err = np.abs(s - s0)
    print(N, "max err %.2e, relative to the norm %.2e" % (err.max(), LP.rel(s, s0)))
    assert np.all(err <= 10 * 3 * N * 2.0 ** -53 * scale)
    assert LP.rel(s, s0) <= 1e-9


def test_implicit_vector_under_both_factorisation_schedules():
    """the session's factorisation takes its schedule from the process default (MI355GP_PERSIST): a child process with the
    persistent launch switched off must return the bytes this process gets with it on"""
    s, s0, _ = _implicit(257, twice=False)
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_laplace_lik as T; "
            "sys.stdout.write(T._implicit(257, twice=False)[0].tobytes().hex())" % (here, os.path.dirname(here)))
    env = dict(os.environ, MI355GP_PERSIST="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == s.tobytes().hex()
    assert LP.rel(s, s0) <= 1e-9


def _model(g, tol=1e-10):
    inf = gpy_amd.Laplace()
    inf._mode_finding_tolerance, inf._mode_finding_max_iter = tol, 100
    m = gpy_amd.GP(g["X"], g["Y"], kernel=LP.gpy_amd_kernel(g["specs"]), likelihood=LL.make_likelihood(g), inference_method=inf)
    return m, inf


@pytest.mark.parametrize("name", LL.CASES)
def test_model_against_the_reference(name):
    g = LL.load(name)
    m, inf = _model(g)
    mu, var = m.predict_noiseless(g["Xs"])
    ymean, yvar = m.predict(g["Xs"])
    nk = m.kern.size
    got = dict(lml=m.log_likelihood(), f_hat=inf.f_hat, Ki_fhat=m.posterior.woodbury_vector, dtheta=m.gradient[:nk], pred_mu=mu,
               pred_var=var)
    if m.likelihood.size:
        got["dL_dthetaL"] = m.gradient[nk:]
        assert m.parameter_names()[-2:] == ["Student_T.t_scale2", "Student_T.deg_free"]
    if g["check_y_prediction"]:
        got.update(pred_ymean=ymean, pred_yvar=yvar)
    fig = LL.figures(g, got)
    for q in fig:
        assert fig[q] <= g["tol"][q], (q, fig[q], g["tol"][q])
    fs = m.posterior_samples_f(g["Xs"][:5], size=3)
    assert fs.shape == (5, 1, 3) and np.isfinite(fs).all()
    with pytest.raises(NotImplementedError):
        m.predictive_gradients(g["Xs"][:3])


def test_checkgrad_student_t_and_poisson():
    g = LL.load("studentt_rbf_iso_n150_d1")
    m, _ = _model(g, tol=1e-12)
    assert m.X.shape[0] == 150 and m.param_array.size == 4
    np.random.seed(3)
    assert m.checkgrad(verbose=True, step=1e-4)
    g = LL.load("poisson_rbf_iso_n150_d2")
    m, _ = _model(g, tol=1e-12)
    np.random.seed(4)
    assert m.checkgrad(verbose=True, step=1e-4)


def test_optimize_on_the_outlier_data():
    z = np.load(os.path.join(LL.GOLDEN, "robust_toy_optimize.npz"))
    X, Y, Xt, ft = z["X"], z["Y"], z["Xt"], z["ft"]
    mg = gpy_amd.GPRegression(X, Y, gpy_amd.RBF(1))
    mg.optimize(max_iters=20)
    m = gpy_amd.GP(X, Y, kernel=gpy_amd.RBF(1), likelihood=gpy_amd.StudentT(deg_free=5, sigma2=2), inference_method=gpy_amd.Laplace())
    start = m.log_likelihood()
    m.optimize(max_iters=20)
    rmse = [float(np.sqrt(np.mean(np.square(mm.predict_noiseless(Xt)[0] - ft)))) for mm in (mg, m)]
    print("Student-t lml %.4f -> %.4f (reference %.4f -> %.4f); rmse Gaussian %.4f, Student-t %.4f (reference %.4f, %.4f)" % (
        start, m.log_likelihood(), float(z["studentt_lml_start"]), float(z["studentt_lml_end"]), rmse[0], rmse[1],
        float(z["gaussian_rmse"]), float(z["studentt_rmse"])))
    assert float(z["studentt_rmse"]) < float(z["gaussian_rmse"])          # what the generator confirmed on the reference
    assert m.log_likelihood() > start
    assert rmse[1] < rmse[0]


def test_classification_is_unchanged_around_a_student_t_run(monkeypatch):
    """Bernoulli Laplace and EP on one context before and after a Student-t run on it: the same bytes; and a likelihood without
    parameters never reaches laplace_implicit (counted on the Python side)"""
    X, Y = _data(300, seed=1)
    Yc = (Y > 0).astype(float)
    calls = []
    real = L.Context.laplace_implicit
    monkeypatch.setattr(L.Context, "laplace_implicit", lambda self, d: (calls.append(1), real(self, d))[1])
    inf_l, inf_e, inf_t = gpy_amd.Laplace(), gpy_amd.EP(), gpy_amd.Laplace()

    def run(inf, lik, Yv):
        post, lml, gd = inf.inference(gpy_amd.RBF(2, 1.3, 0.8), X, lik, Yv)
        return np.float64(lml).tobytes() + np.asarray(post.woodbury_vector).tobytes() + np.asarray(gd["dL_dK"].fused_dtheta).tobytes()
    first = run(inf_l, gpy_amd.Bernoulli(), Yc)
    inf_e._state = inf_t._state = inf_l._state                       # one context for the three of them
    before = [first, run(inf_e, gpy_amd.Bernoulli(), Yc), run(inf_l, gpy_amd.Bernoulli(), Yc)]
    assert before[2] == first and calls == []
    run(inf_t, gpy_amd.StudentT(deg_free=6.0, sigma2=8.0), Y)
    assert calls == [1]
    after = [run(inf_l, gpy_amd.Bernoulli(), Yc), run(inf_e, gpy_amd.Bernoulli(), Yc), run(inf_l, gpy_amd.Bernoulli(), Yc)]
    assert calls == [1]
    assert before == after


def test_error_paths_return_a_message():
    X, Y = _data(200)
    ctx = L.Context()
    ctx.set_data(X, Y)
    W = np.full(200, 0.3)
    ctx.laplace_begin(P.cabi_specs(RBF))
    with pytest.raises(L.MI355GPError, match="mi355gp_laplace_finish first"):
        ctx.laplace_implicit(W)
    assert ctx.laplace_newton(W, W)[0] == 0
    with pytest.raises(L.MI355GPError, match="mi355gp_laplace_finish first"):
        ctx.laplace_implicit(W)
    assert ctx.laplace_finish(W)[0] == 0
    bad = W.copy()
    bad[17] = np.nan
    with pytest.raises(L.MI355GPError, match=r"dL_dfhat\[17\] = nan is not finite"):
        ctx.laplace_implicit(bad)
    assert np.isfinite(ctx.laplace_implicit(W)).all()                # the session is still usable
