"""Fixtures tests/golden/osc/*.npz FROM THE REFERENCE'S OWN CODE: `Cosine`, `Sinc` and `ExpQuadCosine`
(GPy/kern/src/stationary.py:664-743), `Add` / `Prod`, `ExactGaussianInference`, `ExactStudentTInference`,
`update_gradients_full`, `gradients_X` and `PosteriorExact._raw_predict`, executed through oracle/ref_loader.py (imported,
unchanged).  Only the arrays below are stored; the layout of the inference fixtures is that of tools/make_golden_periodic.py.

specs entries are [kind, ard, theta (GPy link order), active_dims, term]; parts sharing a non-zero term id are the factors of
one `Prod` (the C-ABI's `mi355gp_part`).  theta of ExpQuadCosine is [variance, lengthscale(s), period] (:692-695).

Inputs are centred at the origin: the reference forms r^2 = x^2 + x'^2 - 2 x x' (stationary.py `_unscaled_dist`), which loses
digits away from it.  The three kinds are positive definite over one input dimension only, so every inference fixture puts
them on one column.

    kernels_ard_n90_m70_d3   K(X, X), K(X, X2), update_gradients_full on seeded dL_dK (square and rectangular) and gradients_X
                             of the three kinds with ARD over three columns; no inference
    toy_sm_optimize          a 1-D signal with two incommensurate periods under a slow trend, three ExpQuadCosine parts plus
                             Bias: the reference's log marginal at the start and after `maxiter` L-BFGS-B iterations over the
                             log-parameters (what `GPRegression.optimize` runs), with the parameters it reached

    python tools/make_golden_osc.py
"""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "osc")
PARAMS = {"Cosine": ("variance", "lengthscale"), "Sinc": ("variance", "lengthscale"),
          "ExpQuadCosine": ("variance", "lengthscale", "period"), "RBF": ("variance", "lengthscale"), "White": ("variance",),
          "Bias": ("variance",)}


def leaf(ns, spec):
    kind, ard, th, dims, _ = spec
    th = np.asarray(th, dtype=float)
    nd = len(dims)
    nl = nd if ard else 1
    if kind == "cosine":
        return ns.Cosine(nd, variance=th[0], lengthscale=th[1:1 + nl], ARD=bool(ard), active_dims=dims)
    if kind == "sinc":
        return ns.Sinc(nd, variance=th[0], lengthscale=th[1:1 + nl], ARD=bool(ard), active_dims=dims)
    if kind == "expquadcosine":
        return ns.ExpQuadCosine(nd, variance=th[0], lengthscale=th[1:1 + nl], period=th[1 + nl], ARD=bool(ard), active_dims=dims)
    if kind == "rbf":
        return ns.RBF(nd, variance=th[0], lengthscale=th[1:], ARD=bool(ard), active_dims=dims)
    if kind == "white":
        return ns.White(nd, variance=th[0], active_dims=dims)
    if kind == "bias":
        return ns.Bias(nd, variance=th[0], active_dims=dims)
    raise ValueError(kind)


def grads(k):
    return np.concatenate([np.atleast_1d(np.asarray(getattr(k, n).gradient, float)) for n in PARAMS[type(k).__name__]])


def assemble(ns, specs):
    leaves = [leaf(ns, s) for s in specs]
    groups, seen = [], {}
    for s, k in zip(specs, leaves):
        t = s[4]
        if t == 0:
            groups.append([k])
        elif t in seen:
            seen[t].append(k)
        else:
            seen[t] = [k]
            groups.append(seen[t])
    tops = [g[0] if len(g) == 1 else ns.Prod(g) for g in groups]
    top = tops[0] if len(tops) == 1 else ns.Add(tops)

    def walk(k):                                   # Add / Prod copy their parts: the linked copies, in order
        return [q for p in k.parts for q in walk(p)] if hasattr(k, "parts") else [k]
    return top, walk(top)


def seeded_dL_dK(seed, N, M):
    """the dL_dK (N x N) and dL_dK against Xs (N x M) the gradient fixtures were made with"""
    rng = np.random.default_rng(1000 + seed)
    return rng.standard_normal((N, N)), rng.standard_normal((N, M))


def spec_json(specs):
    return json.dumps([[s[0], int(s[1]), [float(v) for v in s[2]], [int(d) for d in s[3]], int(s[4])] for s in specs])


def centred(N, D, seed):
    """seeded inputs centred at the origin and a smooth target with two oscillations of the first column"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (N, D))
    X -= X.mean(0)
    f = np.sin(2 * np.pi * X[:, 0] / 1.3) + 0.5 * np.cos(2 * np.pi * X[:, 0] / 0.45) + 0.3 * X.sum(1)
    Y = (f + 0.1 * rng.standard_normal(N))[:, None]
    return np.ascontiguousarray(X), np.ascontiguousarray(Y)


def case(ns, name, X, Y, specs, noise=0.1, nu=None, seed=0):
    k, leaves = assemble(ns, specs)
    rng = np.random.default_rng(seed + 7)
    if nu is None:
        lik = ns.Gaussian(variance=noise)
        post, lml, gd = ns.ExactGaussianInference().inference(k, X, lik, Y)
        lik.update_gradients(gd["dL_dthetaL"])
        dnoise = float(np.asarray(lik.variance.gradient).ravel()[0])
    else:
        post, lml, gd = ns.studentt.ExactStudentTInference().inference(k, X, Y, nu)
        dnoise = float(gd["dL_dnu"])
    k.update_gradients_full(gd["dL_dK"], X)
    dtheta = np.concatenate([grads(p) for p in leaves])
    lo, hi = X.min(0), X.max(0)
    Xs = lo + (hi - lo) * rng.random((13, X.shape[1]))
    mu, var = post._raw_predict(k, Xs, pred_var=X, full_cov=False)
    _, cov = post._raw_predict(k, Xs, pred_var=X, full_cov=True)
    G, G2 = seeded_dL_dK(seed, X.shape[0], Xs.shape[0])
    np.savez_compressed(os.path.join(OUT, name + ".npz"), X=X, Y=Y, noise=noise, nu=-1.0 if nu is None else nu,
                        specs=spec_json(specs), lml=float(lml), alpha=np.asarray(post.woodbury_vector), dtheta=dtheta,
                        dnoise=dnoise, K_row0=np.asarray(k.K(X))[0], Xs=Xs, pred_mu=np.asarray(mu),
                        pred_var=np.asarray(var), pred_cov=np.asarray(cov), gseed=seed, gradX=np.asarray(k.gradients_X(G, X)),
                        gradX2=np.asarray(k.gradients_X(G2, X, Xs)))
    print("%-36s lml=% .12e" % (name, lml))


def kernels_ard(ns):
    rng = np.random.default_rng(41)
    X, X2 = rng.uniform(-1.5, 1.5, (90, 3)), rng.uniform(-1.5, 1.5, (70, 3))
    X -= X.mean(0)
    G, G2 = seeded_dL_dK(41, 90, 70)
    specs = [("cosine", 1, [1.2, 1.9, 2.6, 1.4], [0, 1, 2], 0), ("sinc", 1, [0.8, 2.2, 1.7, 3.1], [0, 1, 2], 0),
             ("expquadcosine", 1, [1.1, 9.0, 12.5, 7.0, 0.3], [0, 1, 2], 0)]
    out = dict(X=X, X2=X2, gseed=41, specs=spec_json(specs))
    for s in specs:
        k = leaf(ns, s)
        out[s[0] + "_K"] = np.asarray(k.K(X))
        out[s[0] + "_Kx"] = np.asarray(k.K(X, X2))
        k.update_gradients_full(G, X)
        out[s[0] + "_dtheta"] = grads(k)
        k.update_gradients_full(G2, X, X2)
        out[s[0] + "_dtheta_x"] = grads(k)
        out[s[0] + "_gradX"] = np.asarray(k.gradients_X(G, X))
        out[s[0] + "_gradX2"] = np.asarray(k.gradients_X(G2, X, X2))
    np.savez_compressed(os.path.join(OUT, "kernels_ard_n90_m70_d3.npz"), **out)
    print("kernels_ard_n90_m70_d3")


def toy_signal(N, half_width, seed):
    """the example's signal (examples/spectral_mixture_regression.py): periods 1 and sqrt 7 under a slow trend, centred inputs"""
    rng = np.random.default_rng(seed)
    x = np.sort(rng.uniform(-half_width, half_width, N))
    y = np.sin(2 * np.pi * x) + 0.6 * np.sin(2 * np.pi * x / np.sqrt(7.0) + 0.4) + 0.15 * x + 0.1 * rng.standard_normal(N)
    return x[:, None], y[:, None]


# the example's start: [variance, lengthscale, period] of the three parts (period in input units = lengthscale x period),
# Bias variance, noise variance
TOY_THETA0 = np.array([0.5, 30.0, 1.1 / 30.0, 0.3, 40.0, 2.4 / 40.0, 0.5, 60.0, 5.0, 0.1, 0.05])


def toy_sm(ns, N=120, half_width=6.0, maxiter=200):
    from scipy.optimize import minimize
    X, Y = toy_signal(N, half_width, 5)

    def evaluate(z):
        th = np.exp(z)
        specs = [("expquadcosine", 0, th[3 * i:3 * i + 3], [0], 0) for i in range(3)] + [("bias", 0, th[9:10], [0], 0)]
        k, leaves = assemble(ns, specs)
        lik = ns.Gaussian(variance=th[10])
        post, lml, gd = ns.ExactGaussianInference().inference(k, X, lik, Y)
        lik.update_gradients(gd["dL_dthetaL"])
        k.update_gradients_full(gd["dL_dK"], X)
        g = np.concatenate([grads(p) for p in leaves] + [np.atleast_1d(np.asarray(lik.variance.gradient, float)).ravel()])
        return float(lml), g * th
    z0 = np.log(TOY_THETA0)
    lml0 = evaluate(z0)[0]
    res = minimize(lambda z: (lambda r: (-r[0], -r[1]))(evaluate(z)), z0, jac=True, method="L-BFGS-B",
                   options={"maxiter": maxiter, "gtol": 1e-6})
    lml1 = evaluate(res.x)[0]
    th = np.exp(res.x)
    np.savez_compressed(os.path.join(OUT, "toy_sm_optimize.npz"), X=X, Y=Y, theta0=TOY_THETA0, lml_start=lml0, lml_end=lml1,
                        theta_end=th, maxiter=maxiter)
    print("toy_sm_optimize: lml %.6f -> %.6f after %d iterations; periods %s" % (lml0, lml1, res.nit, th[1:9:3] * th[2:9:3]))


def main():
    ns = ref_loader.load_sum_kernels(ref_loader.load())
    ns.Cosine, ns.Sinc, ns.ExpQuadCosine = ns.stationary.Cosine, ns.stationary.Sinc, ns.stationary.ExpQuadCosine
    importlib.import_module("GPy.inference.latent_function_inference.posterior")
    ns.studentt = importlib.import_module("GPy.inference.latent_function_inference.exact_studentt_inference")
    os.makedirs(OUT, exist_ok=True)
    X1, Y1 = centred(160, 1, 21)
    X1b, Y1b = centred(180, 1, 22)
    X2, Y2 = centred(180, 2, 23)
    X2b, Y2b = centred(160, 2, 24)
    X3, Y3 = centred(160, 3, 25)
    Xs, Ys = centred(200, 1, 26)
    case(ns, "cosine_iso_n160_d1", X1, Y1, [("cosine", 0, [1.2, 0.4], [0], 0)])
    case(ns, "rbf0_x_cosine1_n180_d2", X2, Y2, [("rbf", 0, [1.2, 1.5], [0], 1), ("cosine", 0, [0.9, 0.3], [1], 1)], seed=1)
    case(ns, "sinc_iso_n160_d1", X1, Y1, [("sinc", 0, [0.8, 1.6], [0], 0)], seed=2)
    case(ns, "sinc1_plus_rbfard_n160_d3", X3, Y3, [("sinc", 0, [0.7, 1.9], [1], 0), ("rbf", 1, [1.1, 1.3, 0.9, 1.7], [0, 1, 2], 0)],
         seed=3)
    case(ns, "eqc_iso_n180_d1", X1b, Y1b, [("expquadcosine", 0, [1.1, 6.0, 0.2], [0], 0)], seed=4)
    case(ns, "sm3_bias_n200_d1", Xs, Ys,
         [("expquadcosine", 0, [0.6, 8.0, 1.3 / 8.0], [0], 0), ("expquadcosine", 0, [0.3, 5.0, 0.45 / 5.0], [0], 0),
          ("expquadcosine", 0, [0.4, 20.0, 4.0], [0], 0), ("bias", 0, [0.2], [0], 0)], noise=0.02, seed=5)
    case(ns, "studentt_eqc1_plus_rbf_n160_d2", X2b, Y2b,
         [("expquadcosine", 0, [0.8, 7.0, 0.25], [1], 0), ("rbf", 0, [1.0, 1.4], [0, 1], 0), ("white", 0, [0.05], [0, 1], 0)],
         nu=4.0, seed=6)           # (the Student-t process has no noise term: the White part keeps Ky well conditioned)
    kernels_ard(ns)
    toy_sm(ns)


if __name__ == "__main__":
    main()
