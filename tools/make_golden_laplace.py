"""Fixtures tests/golden/laplace/*.npz FROM THE REFERENCE'S OWN CODE: `Laplace` (GPy/inference/latent_function_inference/
laplace.py), `Bernoulli` with the `Probit` link, the kernels, `update_gradients_full` and `Posterior._raw_predict`, executed
through oracle/ref_loader.py (imported, unchanged).  Only data goes into the fixtures.

The reference stops its mode search when the objective moves by less than `_mode_finding_tolerance` (1e-4 as shipped), which
leaves every result converged to a few digits only.  Each case is therefore run with the tolerance set to 1e-10 (100 iterations
allowed) -- that run is stored -- and a second time with 1e-8; the largest relative difference between the two runs, per
quantity, is the reference's own convergence floor and is stored as `ref_floor_<quantity>`.  The stored run must itself be
at the mode (`case` explains how that is checked on the reference alone and what happens where it is not).  A test compares at
max(standing tolerance, 10 x floor): the factor 10 covers two implementations stopping on either side of the mode.  The
standing tolerances are those of the other kernel fixtures (LML 1e-10, vectors 1e-9, gradients 1e-8, prediction 1e-9).

The reference's line search, `optimize.brent(inner_obj, tol=1e-4, maxiter=12)`, returns the step to 1e-4 only, so the iterate at
which the reference stops lies 1e-4 of its last step away from the mode WHATEVER the mode tolerance: with plain SciPy the stored
f_hat was 2e-9 .. 2e-8 off the mode (stationarity residual 4e-9 .. 6e-7 over a scan of variances), and the difference between the
two runs did not show it, because both stop at the same iterate.  SciPy >= 1.11 also raises BracketError from `brent` when the
line is flat to rounding, which is what the search meets one iteration after the mode is reached.  A fixture that is not the
mode cannot pin an implementation to 1e-9, so `flat_line_brent` stands in for `brent` in the reference's module (the reference's
files are unchanged): it calls SciPy, and where the full Newton step is as good as SciPy's answer to rounding (1e-12 of the
objective) -- or SciPy found no bracket -- it returns the full step.  Steps that really beat the full step (the first
iterations) are SciPy's.  `case` then checks on the reference's own numbers that the stored run is stationary.

`bernoulli_values.npz` holds the reference's logpdf, its three derivatives in f and predictive_mean over f in [-40, 40];
`toy_1d_optimize.npz` the example's data with the reference's training accuracy after its own optimisation from the same start.

    python tools/make_golden_laplace.py
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
import make_golden_mlp as mlp  # noqa: E402  (leaves of every kind but the two below, assemble, grads)

OUT = os.path.join(ROOT, "tests", "golden", "laplace")
STANDING = {"lml": 1e-10, "f_hat": 1e-9, "Ki_fhat": 1e-9, "dtheta": 1e-8, "dL_dK": 1e-8, "woodbury_inv": 1e-9,
            "pred_mu": 1e-9, "pred_var": 1e-9, "pred_cov": 1e-9, "pred_p": 1e-9}


NAMES = dict(mlp.NAMES, Matern52=("variance", "lengthscale"), StdPeriodic=("variance", "period", "lengthscale"))


def grads(k):
    return np.concatenate([np.atleast_1d(np.asarray(getattr(k, n).gradient, float)).ravel() for n in NAMES[type(k).__name__]])


def flat_line_brent(func, **kw):
    """`scipy.optimize.brent` for the reference's line search, made exact where SciPy's answer is not: see the module docstring"""
    from scipy import optimize
    try:
        s = optimize.brent(func, **kw)
    except Exception as e:
        if type(e).__name__ != "BracketError":
            raise
        s = 0.0
    f0, fs, f1 = func(0.0), func(s), func(1.0)
    if f1 > fs + 1e-12 * max(1.0, abs(fs)):
        return s                                   # the search found something better than the full step: keep it
    # the full Newton step is as good to rounding; the reference raises if its objective comes out below the old one, so the
    # nearest step that does not do that by a rounding error
    for j in range(0, 21):
        for c in ((1.0,) if j == 0 else (1.0 + j * 1e-6, 1.0 - j * 1e-6)):
            if func(c) <= f0:
                return c
    return s if fs <= f0 else 0.0


def leaf(ns, spec):
    kind, ard, th, dims, _ = spec
    th = np.asarray(th, dtype=float)
    nd = len(dims)
    if kind == "matern52":
        return ns.Matern52(nd, variance=th[0], lengthscale=th[1:] if ard else th[1], ARD=bool(ard), active_dims=dims)
    if kind == "stdperiodic":
        return ns.StdPeriodic(nd, variance=th[0], period=th[1], lengthscale=th[2], active_dims=dims)
    return _leaf(ns, spec)


def two_class(N, D, seed, sep):
    """two Gaussian blobs `sep` apart along the first axis, labels 0 / 1"""
    rng = np.random.default_rng(seed)
    y = (rng.random(N) < 0.5).astype(float)
    X = rng.standard_normal((N, D))
    X[:, 0] += sep * (y - 0.5)
    return np.ascontiguousarray(X), y[:, None].copy()


def run(ns, specs, X, Y, tol, Xs):
    k, leaves = mlp.assemble(ns, specs)
    lik = ns.Bernoulli()
    inf = ns.Laplace()
    inf._mode_finding_tolerance, inf._mode_finding_max_iter = tol, 100
    post, lml, gd = inf.inference(k, X, lik, Y)
    k.update_gradients_full(gd["dL_dK"], X)
    mu, var = post._raw_predict(k, Xs, pred_var=X, full_cov=False)
    _, cov = post._raw_predict(k, Xs, pred_var=X, full_cov=True)
    f_hat, Ki = np.asarray(inf.f_hat), np.asarray(post.woodbury_vector)
    resid = float(np.abs(np.asarray(k.K(X)) @ (np.asarray(lik.dlogpdf_df(f_hat, Y)) - Ki)).max() / np.abs(f_hat).max())
    return dict(ref_mode_residual=resid, lml=float(lml), f_hat=np.asarray(inf.f_hat), Ki_fhat=np.asarray(post.woodbury_vector),
                dtheta=np.concatenate([grads(p) for p in leaves]), dL_dK=np.asarray(gd["dL_dK"]),
                woodbury_inv=np.asarray(post.woodbury_inv), pred_mu=np.asarray(mu), pred_var=np.asarray(var),
                pred_cov=np.asarray(cov), pred_p=np.asarray(lik.predictive_values(mu, var)[0]), W=np.asarray(inf.W))


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


def case(ns, name, X, Y, specs, seed=0):
    rng = np.random.default_rng(seed + 7)
    lo, hi = X.min(0), X.max(0)
    Xs = lo + (hi - lo) * rng.random((13, X.shape[1]))
    # The stored run has to BE the mode.  The reference's own stationarity residual says whether it is:
    #   max |K (dlogpdf_df(f_hat) - Ki_fhat)| / max |f_hat|   (zero at the mode, where f = K dlogpdf_df(f))
    r = run(ns, specs, X, Y, 1e-10, Xs)
    if r["ref_mode_residual"] > 1e-10:
        raise RuntimeError("%s: the reference stopped short of the mode (residual %.1e)" % (name, r["ref_mode_residual"]))
    r2 = run(ns, specs, X, Y, 1e-8, Xs)
    r2.pop("ref_mode_residual")
    floors = {"ref_floor_" + q: rel(r2[q], r[q]) for q in STANDING}
    spec_json = json.dumps([[s[0], int(s[1]), [float(v) for v in s[2]], [int(d) for d in s[3]], int(s[4])] for s in specs])
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, X=X, Y=Y, Xs=Xs, specs=spec_json, **r, **floors)
    print("%-30s residual %.1e  lml=% .12e  min W=%.1e  %d bytes" % (name, r["ref_mode_residual"], r["lml"], r["W"].min(), os.path.getsize(path)))
    for q in STANDING:
        f = floors["ref_floor_" + q]
        print("    %-13s floor %.2e -> tolerance %.1e" % (q, f, max(STANDING[q], 10 * f)))


def bernoulli_values(ns):
    lik = ns.Bernoulli()
    f = np.concatenate([np.linspace(-40, 40, 161), [-8.3, -5.7, -0.66, 0.66, 5.7, 8.3]])[:, None]
    out = {"f": f}
    for yv in (0, 1):
        y = np.full_like(f, float(yv))
        out["logpdf_y%d" % yv] = np.asarray(lik.logpdf(f, y))
        out["dlogpdf_df_y%d" % yv] = np.asarray(lik.dlogpdf_df(f, y))
        out["d2logpdf_df2_y%d" % yv] = np.asarray(lik.d2logpdf_df2(f, y))
        out["d3logpdf_df3_y%d" % yv] = np.asarray(lik.d3logpdf_df3(f, y))
    v = np.linspace(0.0, 30.0, f.size)[:, None]
    out["pm_var"] = v
    out["predictive_mean"] = np.asarray(lik.predictive_mean(f, v))
    np.savez_compressed(os.path.join(OUT, "bernoulli_values.npz"), **out)


def toy_1d(ns):
    """the shape of the reference example's data (`GPy/examples/classification.py:96-126`: pods' toy_linear_1d_classification is
    not available offline): two 1-D Gaussian classes; the reference's own L-BFGS-B optimisation from the default start"""
    from scipy.optimize import minimize
    rng = np.random.default_rng(4)
    X = np.concatenate([rng.normal(-1.5, 1.0, 30), rng.normal(1.5, 1.0, 30)])[:, None]
    Y = np.concatenate([np.zeros(30), np.ones(30)])[:, None]

    def evaluate(z):
        k = ns.RBF(1, variance=np.exp(z[0]), lengthscale=np.exp(z[1]))
        lik, inf = ns.Bernoulli(), ns.Laplace()
        post, lml, gd = inf.inference(k, X, lik, Y)
        k.update_gradients_full(gd["dL_dK"], X)
        g = np.array([float(k.variance.gradient), float(k.lengthscale.gradient)]) * np.exp(z)
        return k, lik, post, float(lml), g
    lml0 = evaluate(np.zeros(2))[3]
    res = minimize(lambda z: (lambda r: (-r[3], -r[4]))(evaluate(z)), np.zeros(2), jac=True, method="L-BFGS-B")
    k, lik, post, lml1, _ = evaluate(res.x)
    mu, var = post._raw_predict(k, X, pred_var=X)
    p = lik.predictive_values(mu, var)[0]
    acc = float(np.mean((p > 0.5) == (Y == 1)))
    np.savez_compressed(os.path.join(OUT, "toy_1d_optimize.npz"), X=X, Y=Y, lml_start=lml0, lml_end=lml1, accuracy=acc,
                        theta_end=np.exp(res.x))
    print("toy_1d_optimize: lml %.6f -> %.6f, training accuracy %.4f, theta %s" % (lml0, lml1, acc, np.exp(res.x)))


def main():
    global _leaf
    ns = ref_loader.load_sum_kernels(ref_loader.load())
    ns.Linear = importlib.import_module("GPy.kern.src.linear").Linear
    ns.MLP = importlib.import_module("GPy.kern.src.mlp").MLP
    ns.Poly = importlib.import_module("GPy.kern.src.poly").Poly
    ns.Coregionalize = importlib.import_module("GPy.kern.src.coregionalize").Coregionalize
    ns.StdPeriodic = importlib.import_module("GPy.kern.src.standard_periodic").StdPeriodic
    ns.Bernoulli = importlib.import_module("GPy.likelihoods.bernoulli").Bernoulli
    lap = importlib.import_module("GPy.inference.latent_function_inference.laplace")
    ns.Laplace = lap.Laplace
    import types
    lap.optimize = types.SimpleNamespace(brent=flat_line_brent)      # the module's own name for scipy.optimize
    _leaf, mlp.leaf = mlp.leaf, leaf
    os.makedirs(OUT, exist_ok=True)
    X1, Y1 = two_class(130, 1, 51, 2.0)
    X2, Y2 = two_class(150, 2, 52, 2.0)
    X3, Y3 = two_class(140, 3, 53, 2.5)
    Xw, Yw = two_class(120, 2, 54, 9.0)          # well separated: W underflows towards 0 in the tails
    Xo, Yo = two_class(160, 2, 55, 0.4)          # strongly overlapping
    d2, d3 = [0, 1], [0, 1, 2]
    case(ns, "rbf_iso_n150_d2", X2, Y2, [("rbf", 0, [1.5, 1.1], d2, 0)])
    case(ns, "matern52_ard_n140_d3", X3, Y3, [("matern52", 1, [2.0, 1.2, 0.8, 1.6], d3, 0)], seed=1)
    case(ns, "rbf_linear_bias_n140_d3", X3, Y3,
         [("rbf", 0, [1.2, 0.9], d3, 0), ("linear", 0, [0.4], d3, 0), ("bias", 0, [0.3], d3, 0)], seed=2)
    case(ns, "mlp0_x_rbf12_n140_d3", X3, Y3, [("mlp", 0, [1.5, 0.9, 0.7], [0], 1), ("rbf", 1, [1.2, 0.8, 1.4], [1, 2], 1)], seed=3)
    case(ns, "stdperiodic_n130_d1", X1, Y1, [("stdperiodic", 0, [1.3, 5.0, 0.9], [0], 0)], seed=4)
    case(ns, "separated_rbf_n120_d2", Xw, Yw, [("rbf", 0, [6.0, 1.5], d2, 0)], seed=5)
    case(ns, "overlapping_rbf_n160_d2", Xo, Yo, [("rbf", 0, [1.0, 1.0], d2, 0)], seed=6)
    bernoulli_values(ns)
    toy_1d(ns)


if __name__ == "__main__":
    main()
