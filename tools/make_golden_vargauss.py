"""Fixtures tests/golden/vargauss/*.npz FROM THE REFERENCE'S OWN CODE: `VarGauss.inference`
(GPy/inference/latent_function_inference/var_gauss.py) with the reference's kernels, likelihoods (their
`variational_expectations`), `update_gradients_full` and `Posterior._raw_predict`, executed through oracle/ref_loader.py
(imported, unchanged).  Only data goes into the fixtures.

Each fixture holds the inputs (X, Y, Xs, the part list, the likelihood and its parameters, alpha, beta -- seeded vectors, not an
optimum: the judged map is one evaluation) and the reference's m, var, log marginal, both variational gradients,
(dL_dK + dL_dK^T) / 2, dL_dthetaL, the kernel gradient and the latent prediction at 13 new points.

The reference builds its posterior by inverting K (`posterior.py`), so its prediction is only as good as K is conditioned: every
part list carries a White part and a case whose cond2(K) exceeds 1e4 is REFUSED, not written.  cond2(K) and cond2(A) are stored.

`toy_1d_optimize.npz`: the 1-D two-class data of tests/golden/laplace/toy_1d_optimize.npz; the reference's bound at the default
start and after its own L-BFGS-B run (at most 100 iterations) over [log variance, log lengthscale, alpha, beta].

    python tools/make_golden_vargauss.py
"""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from oracle import ref_loader  # noqa: E402
import make_golden_mlp as mlp  # noqa: E402
import make_golden_laplace as G  # noqa: E402  (leaf of Matern52 / StdPeriodic, two_class)
import make_golden_laplace_lik as GL  # noqa: E402  (student_t, robust_data, count_data)

OUT = os.path.join(ROOT, "tests", "golden", "vargauss")
NAMES = dict(G.NAMES, White=("variance",))
COND_MAX = 1e4


def leaf(ns, spec):
    if spec[0] == "white":
        return ns.White(len(spec[3]), variance=float(spec[2][0]), active_dims=spec[3])
    return G.leaf(ns, spec)


def grads(k):
    return np.concatenate([np.atleast_1d(np.asarray(getattr(k, n).gradient, float)).ravel() for n in NAMES[type(k).__name__]])


def make_lik(ns, lik, theta):
    if lik == "bernoulli":
        return ns.Bernoulli()
    if lik == "gaussian":
        return ns.Gaussian(variance=theta[0])
    if lik == "studentt":
        return GL.student_t(ns, theta[1], theta[0])
    return ns.Poisson()


def case(ns, name, lik_name, lik_theta, X, Y, specs, seed, signs="pos"):
    rng = np.random.default_rng(seed + 7)
    N = X.shape[0]
    lo, hi = X.min(0), X.max(0)
    Xs = lo + (hi - lo) * rng.random((13, X.shape[1]))
    alpha = 0.3 * rng.standard_normal((N, 1))
    beta = rng.uniform(0.4, 1.2, N)
    if signs == "mixed":
        beta = np.where(rng.random(N) < 0.5, -beta, beta)
    k, leaves = mlp.assemble(ns, specs)
    K = np.asarray(k.K(X), float)
    condK = float(np.linalg.cond(K))
    if condK > COND_MAX:
        raise RuntimeError("%s REFUSED: cond2(K) = %.2e exceeds %.0e, the reference's K^-1 posterior is not trustworthy" % (name, condK, COND_MAX))
    condA = float(np.linalg.cond(np.eye(N) + beta[:, None] * K * beta[None, :]))
    lik = make_lik(ns, lik_name, lik_theta)
    a, b = ns.Param("alpha", alpha.copy()), ns.Param("beta", beta.copy())
    post, lml, gd = ns.VarGauss(a, b).inference(k, X, lik, Y)
    k.update_gradients_full(gd["dL_dK"], X)
    dL = np.asarray(gd["dL_dK"], float)
    mu, var = post._raw_predict(k, Xs, pred_var=X, full_cov=False)
    _, cov = post._raw_predict(k, Xs, pred_var=X, full_cov=True)
    spec_json = json.dumps([[s[0], int(s[1]), [float(v) for v in s[2]], [int(d) for d in s[3]], int(s[4])] for s in specs])
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, X=X, Y=Y, Xs=Xs, specs=spec_json, lik=lik_name, lik_theta=np.asarray(lik_theta, float), alpha=alpha,
                        beta=beta, m=np.asarray(post.mean, float), var=np.diag(np.asarray(post.covariance, float)).copy(),
                        lml=float(lml), dalpha=np.asarray(a.gradient, float), dbeta=np.asarray(b.gradient, float),
                        dL_dK_sym=0.5 * (dL + dL.T), dL_dthetaL=np.asarray(gd["dL_dthetaL"], float).ravel(),
                        dtheta=np.concatenate([grads(p) for p in leaves]), pred_mu=np.asarray(mu, float), pred_var=np.asarray(var, float),
                        pred_cov=np.asarray(cov, float), condK=condK, condA=condA)
    print("%-40s N %d  cond K %.1f  cond A %.1f  lml % .12e  %d bytes" % (name, N, condK, condA, float(lml), os.path.getsize(path)))


def toy_1d(ns):
    from scipy.optimize import minimize
    z = np.load(os.path.join(ROOT, "tests", "golden", "laplace", "toy_1d_optimize.npz"))
    X, Y = z["X"], z["Y"]
    N = X.shape[0]

    def evaluate(p):
        k = ns.RBF(1, variance=np.exp(p[0]), lengthscale=np.exp(p[1]))
        lik = ns.Bernoulli()
        a, b = ns.Param("alpha", p[2:2 + N][:, None].copy()), ns.Param("beta", p[2 + N:].copy())
        post, lml, gd = ns.VarGauss(a, b).inference(k, X, lik, Y)
        k.update_gradients_full(gd["dL_dK"], X)
        g = np.concatenate([np.array([float(k.variance.gradient), float(k.lengthscale.gradient)]) * np.exp(p[:2]),
                            np.asarray(a.gradient, float).ravel(), np.asarray(b.gradient, float).ravel()])
        return k, lik, post, float(lml), g
    p0 = np.concatenate([np.zeros(2), np.zeros(N), np.ones(N)])
    lml0 = evaluate(p0)[3]
    res = minimize(lambda p: (lambda r: (-r[3], -r[4]))(evaluate(p)), p0, jac=True, method="L-BFGS-B", options={"maxiter": 100})
    k, lik, post, lml1, _ = evaluate(res.x)
    mu, var = post._raw_predict(k, X, pred_var=X)
    prob = lik.predictive_values(mu, var)[0]
    acc = float(np.mean((prob > 0.5) == (Y == 1)))
    np.savez_compressed(os.path.join(OUT, "toy_1d_optimize.npz"), X=X, Y=Y, lml_start=lml0, lml_end=lml1, accuracy=acc,
                        theta_end=np.exp(res.x[:2]), iterations=int(res.nit))
    print("toy_1d_optimize: bound %.6f -> %.6f in %d iterations, training accuracy %.4f, theta %s" % (lml0, lml1, res.nit, acc, np.exp(res.x[:2])))


def main():
    ns = ref_loader.load_sum_kernels(ref_loader.load())
    ns.Linear = importlib.import_module("GPy.kern.src.linear").Linear
    ns.StdPeriodic = importlib.import_module("GPy.kern.src.standard_periodic").StdPeriodic
    ns.Bernoulli = importlib.import_module("GPy.likelihoods.bernoulli").Bernoulli
    ns.StudentTClass = importlib.import_module("GPy.likelihoods.student_t").StudentT
    ns.Poisson = importlib.import_module("GPy.likelihoods.poisson").Poisson
    ns.VarGauss = importlib.import_module("GPy.inference.latent_function_inference.var_gauss").VarGauss
    ns.Param = importlib.import_module("GPy.core.parameterization.param").Param
    G._leaf, mlp.leaf = mlp.leaf, leaf
    os.makedirs(OUT, exist_ok=True)
    d1, d2, d3 = [0], [0, 1], [0, 1, 2]
    w = lambda dims, v=0.1: ("white", 0, [v], dims, 0)                 # noqa: E731
    X1, Y1 = G.two_class(130, 1, 51, 2.0)
    X2, Y2 = G.two_class(150, 2, 52, 2.0)
    X3, Y3 = G.two_class(140, 3, 53, 2.5)
    case(ns, "bernoulli_rbf_iso_n150_d2", "bernoulli", [], X2, Y2, [("rbf", 0, [1.3, 0.9], d2, 0), w(d2)], 0)
    case(ns, "bernoulli_matern52_ard_n140_d3", "bernoulli", [], X3, Y3, [("matern52", 1, [1.5, 1.2, 0.8, 1.6], d3, 0), w(d3)], 1)
    case(ns, "bernoulli_rbf_linear_bias_n140_d3", "bernoulli", [], X3, Y3,
         [("rbf", 0, [1.2, 0.9], d3, 0), ("linear", 0, [0.4], d3, 0), ("bias", 0, [0.3], d3, 0), w(d3)], 2)
    case(ns, "bernoulli_stdperiodic_n130_d1", "bernoulli", [], X1, Y1, [("stdperiodic", 0, [1.3, 5.0, 0.9], d1, 0), w(d1)], 3)
    case(ns, "bernoulli_rbf_iso_mixed_signs_n120_d2", "bernoulli", [], *G.two_class(120, 2, 54, 2.0),
         specs=[("rbf", 0, [1.0, 0.7], d2, 0), w(d2)], seed=4, signs="mixed")
    Xg, Yg = GL.robust_data(150, 1, 61)
    case(ns, "gaussian_rbf_iso_n150_d1", "gaussian", [0.3], Xg, Yg, [("rbf", 0, [1.5, 0.9], d1, 0), w(d1)], 5)
    Xt, Yt = GL.robust_data(140, 2, 62, outliers=0.05)
    case(ns, "studentt_rbf_iso_n140_d2", "studentt", [0.5, 5.0], Xt, Yt, [("rbf", 0, [1.2, 0.8], d2, 0), w(d2)], 6)
    Xp, Yp = GL.count_data(150, 2, 63)
    case(ns, "poisson_rbf_iso_n150_d2", "poisson", [], Xp, Yp, [("rbf", 0, [1.0, 0.7], d2, 0), w(d2)], 7)
    toy_1d(ns)


if __name__ == "__main__":
    main()
