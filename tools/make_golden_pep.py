"""Fixtures tests/golden/pep/*.npz FROM THE REFERENCE'S OWN CODE: `FITC.inference`
(GPy/inference/latent_function_inference/fitc.py) and `PEP.inference` (.../pep.py), the kernels' `update_gradients_diag` /
`update_gradients_full` / `gradients_X` assembled as GPy/core/sparse_gp.py:108-119 does (certain inputs), and
`Posterior._raw_predict` at 7 new points with `full_cov` both ways, executed through oracle/ref_loader.py (imported, unchanged).
Only data goes into the fixtures.

Inputs as tools/make_golden_svgp.py draws them: Z on a jittered regular grid over the first (at most two) active dimensions with
lengthscales of 0.75 grid spacings there, in the unit cube centred at the origin.  With Z drawn at random cond(Kmm + 1e-6 I) is
of order 1e6 or more and the reference's own numbers are no yardstick.  The D = 1 case has M = 10: with 20 grid cells on a line
the reference's r^2 = |x|^2 + |z|^2 - 2 x.z (scaled coordinates up to 13) is itself 1.3e-12 from long double in dL_dKmm, twice
the bound its kappa = 12 gives.

`pep_alpha1_*` repeats a FITC case through `PEP(1.0)`.  The reference's two results are NOT the same bits: sigma_star is summed
in another order (fitc.py:43 against pep.py:45); the generator asserts agreement to 64 eps of each quantity's largest entry and
prints the figure.
`toy_fitc.npz`: a 1-D regression problem; the reference's FITC log marginal before and after 40 L-BFGS-B iterations over
(Z, log kernel parameters, log noise variance), the flat order of the package's `SparseGP`.

    python tools/make_golden_pep.py
"""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import ref_loader  # noqa: E402
from make_golden_svgp import assemble, grads, grid_Z  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "pep")


def evaluate(ns, method, alpha, specs, noise, X, Y, Z, Xs=None):
    """one FITC / PEP inference + the gradient assembly of core/sparse_gp.py:108-119 (+ predictions at Xs)"""
    k, leaves = assemble(ns, specs)
    lik = ns.Gaussian(variance=noise)
    # GPy's Gaussian.exact_inference_gradients returns dL_dKdiag.sum(), a NumPy scalar, which pep.py:87 then adds a (1,) array to
    # in place; a 0-d array in its place cannot take that `+=`, so the sum is handed over as the scalar GPy produces
    lik.exact_inference_gradients = lambda dL_dKdiag, Y_metadata=None: np.float64(np.sum(dL_dKdiag))
    inf = ns.FITC() if method == "fitc" else ns.PEP(alpha)
    post, lml, gd = inf.inference(k, X, Z, lik, Y)
    k.update_gradients_diag(gd["dL_dKdiag"], X)
    g = grads(leaves)
    k.update_gradients_full(gd["dL_dKnm"], X, Z)
    g = g + grads(leaves)
    k.update_gradients_full(gd["dL_dKmm"], Z, None)
    g = g + grads(leaves)
    dZ = k.gradients_X(gd["dL_dKmm"], Z) + k.gradients_X(gd["dL_dKnm"].T, Z, X)
    out = dict(lml=float(np.squeeze(lml)), dtheta=g, dZ=np.asarray(dZ, float), dL_dKmm=np.asarray(gd["dL_dKmm"], float),
               dL_dKnm=np.asarray(gd["dL_dKnm"], float), dL_dKdiag=np.asarray(gd["dL_dKdiag"], float).ravel(),
               dL_dthetaL=np.atleast_1d(np.asarray(gd["dL_dthetaL"], float)).ravel(),
               woodbury_vector=np.asarray(post.woodbury_vector, float), woodbury_inv=np.asarray(post.woodbury_inv, float))
    if Xs is not None:
        mu, var = post._raw_predict(k, Xs, pred_var=Z, full_cov=False)
        _, cov = post._raw_predict(k, Xs, pred_var=Z, full_cov=True)
        out.update(pred_mu=np.asarray(mu, float), pred_var=np.asarray(var, float), pred_cov=np.asarray(cov, float))
    return out


def inputs(N, M, D, kern, seed):
    rng = np.random.default_rng(seed)
    allq = list(range(D))
    gdims = [2, 0] if kern == "rbf_ard_subset" else allq[:2]
    Z, g = grid_Z(M, D, gdims, rng)
    X = rng.uniform(0.0, 1.0, (N, D))

    def ls(dims, ard):
        v = np.array([0.75 / g * rng.uniform(0.9, 1.1) if q in gdims else 4.0 * np.sqrt(D) for q in dims])
        return list(v if ard else v[:1])
    if kern == "rbf_iso":
        specs = [("rbf", 0, [1.2] + ls(allq, 0), allq, 0)]
    elif kern == "rbf_ard":
        specs = [("rbf", 1, [1.3] + ls(allq, 1), allq, 0)]
    elif kern == "matern52_ard":
        specs = [("matern52", 1, [0.9] + ls(allq, 1), allq, 0)]
    elif kern == "rbf+white+bias":
        specs = [("rbf", 0, [1.2] + ls(allq, 0), allq, 0), ("white", 0, [0.05], allq, 0), ("bias", 0, [0.2], allq, 0)]
    elif kern == "rbf*matern32":
        specs = [("rbf", 0, [1.3] + ls(allq, 0), allq, 1), ("matern32", 0, [0.8] + ls(allq, 0), allq, 1)]
    else:                                          # RBF ARD on active_dims = [2, 0] of a 3-column X: column 1 is seen by no part
        assert kern == "rbf_ard_subset" and D == 3
        specs = [("rbf", 1, [1.1] + ls([2, 0], 1), [2, 0], 0)]
    w = rng.uniform(1.0, 3.0, (min(D, 3), 1))
    Y = np.sin(2.0 * np.pi * X[:, :w.shape[0]] @ w / w.shape[0]) + 0.2 * rng.standard_normal((N, 1))
    Xs = rng.uniform(0.0, 1.0, (7, D))
    # the unit cube centred at the origin: the reference forms r^2 as |x|^2 + |z|^2 - 2 x.z in scaled coordinates, whose rounding
    # grows with their squares (up to 27^2 for 20 grid cells of 0.75 lengthscales in [0, 1]); centring quarters that, as
    # tests/sparse_ld.make_case does for D = 1, so that the reference's own numbers are a yardstick to its kappa
    return specs, X - 0.5, Y, Z - 0.5, Xs - 0.5


def case(ns, name, method, alpha, noise, N, M, D, kern, seed):
    specs, X, Y, Z, Xs = inputs(N, M, D, kern, seed)
    r = evaluate(ns, method, alpha, specs, noise, X, Y, Z, Xs)
    k, _ = assemble(ns, specs)
    kappa = float(np.linalg.cond(np.asarray(k.K(Z)) + 1e-6 * np.eye(M)))
    spec_json = json.dumps([[s[0], int(s[1]), [float(v) for v in s[2]], [int(d) for d in s[3]], int(s[4])] for s in specs])
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, X=X, Y=Y, Z=Z, Xs=Xs, specs=spec_json, method=method, alpha=float(alpha), noise=float(noise),
                        cond_Kmm=kappa, **r)
    print("%-36s lml % .10e  cond(Kmm + 1e-6 I) %.1e  %d bytes" % (name, r["lml"], kappa, os.path.getsize(path)))
    return r


def toy_fitc(ns):
    from scipy.optimize import minimize
    rng = np.random.default_rng(9)
    N, M = 120, 10
    X = np.sort(rng.uniform(0.0, 1.0, (N, 1)), 0)
    Y = np.sin(2.0 * np.pi * X) + 0.3 * np.cos(9.0 * X) + 0.15 * rng.standard_normal((N, 1))
    Z0 = ((np.arange(M) + 0.5) / M)[:, None]

    # flat order of the package's model: Z, kern.variance, kern.lengthscale, noise variance; positive parameters in log space
    def f(x):
        Z, var, ls, s2 = x[:M].reshape(M, 1), np.exp(x[M]), np.exp(x[M + 1]), np.exp(x[M + 2])
        r = evaluate(ns, "fitc", 1.0, [("rbf", 0, [var, ls], [0], 0)], s2, X, Y, Z)
        g = np.concatenate([r["dZ"].ravel(), r["dtheta"] * np.array([var, ls]), r["dL_dthetaL"] * s2])
        return -r["lml"], -g
    theta0 = np.array([1.0, 0.1, 0.1])
    x0 = np.concatenate([Z0.ravel(), np.log(theta0)])
    l0 = -f(x0)[0]
    res = minimize(f, x0, jac=True, method="L-BFGS-B", options={"maxiter": 40})
    l1 = -f(res.x)[0]
    np.savez_compressed(os.path.join(OUT, "toy_fitc.npz"), X=X, Y=Y, Z0=Z0, theta0=theta0, lml_start=l0, lml_end=l1, maxiter=40)
    print("toy_fitc: log marginal %.6f -> %.6f" % (l0, l1))


def main():
    ns = ref_loader.load_sum_kernels(ref_loader.load())
    ns.FITC = importlib.import_module("GPy.inference.latent_function_inference.fitc").FITC
    ns.PEP = importlib.import_module("GPy.inference.latent_function_inference.pep").PEP
    os.makedirs(OUT, exist_ok=True)
    case(ns, "fitc_rbf_iso_n200_m10_d1", "fitc", 1.0, 0.04, 200, 10, 1, "rbf_iso", 1)
    r1 = case(ns, "fitc_matern52_ard_n250_m36_d3", "fitc", 1.0, 0.05, 250, 36, 3, "matern52_ard", 2)
    case(ns, "fitc_rbf_white_bias_n180_m30_d2", "fitc", 1.0, 0.04, 180, 30, 2, "rbf+white+bias", 3)
    case(ns, "fitc_rbf_x_matern32_n220_m25_d2", "fitc", 1.0, 0.05, 220, 25, 2, "rbf*matern32", 4)
    case(ns, "fitc_rbf_ard_subset_n300_m40_d3", "fitc", 1.0, 0.04, 300, 40, 3, "rbf_ard_subset", 5)
    r2 = case(ns, "pep_alpha1_matern52_ard_n250_m36_d3", "pep", 1.0, 0.05, 250, 36, 3, "matern52_ard", 2)
    # PEP(alpha = 1) is FITC in the reference up to the order of ONE sum: sigma_star = Knn + sigma_n - q (fitc.py:43) against
    # sigma_n + 1 (Knn - q) (pep.py:45).  The two roundings differ in the last bit of some sigma_star, so the results are not the
    # same bits; they agree to a few ulps of each quantity's largest entry, which is what is asserted (and printed) here.
    worst = 0.0
    for q in r1:
        a, b = np.asarray(r1[q], float), np.asarray(r2[q], float)
        worst = max(worst, float(np.max(np.abs(a - b)) / np.max(np.abs(a))))
        assert a.shape == b.shape and np.max(np.abs(a - b)) <= 64 * np.finfo(float).eps * np.max(np.abs(a)), q
    print("PEP(1.0) against FITC in the reference: worst relative difference %.2e (not bit-identical: %s)"
          % (worst, ", ".join(q for q in r1 if not np.array_equal(np.asarray(r1[q]), np.asarray(r2[q])))))
    case(ns, "pep_alpha05_rbf_ard_n240_m32_d3", "pep", 0.5, 0.05, 240, 32, 3, "rbf_ard", 6)
    case(ns, "pep_alpha01_rbf_white_bias_n160_m24_d2", "pep", 0.1, 0.04, 160, 24, 2, "rbf+white+bias", 7)
    toy_fitc(ns)


if __name__ == "__main__":
    main()
