"""Fixtures tests/golden/laplace_lik/*.npz FROM THE REFERENCE'S OWN CODE: `Laplace` with the reference's `StudentT` and
`Poisson` likelihoods (GPy/likelihoods/student_t.py, poisson.py, link_functions.py), the kernels, `update_gradients_full` and
`Posterior._raw_predict`, executed through oracle/ref_loader.py (imported, unchanged).  Only data goes into the fixtures.

The conventions are those of tools/make_golden_laplace.py, whose helpers are imported: each case runs at a mode tolerance of
1e-10 (stored) and again at 1e-8; the largest relative difference between the two, per quantity, is the reference's own
convergence floor, stored as `ref_floor_<quantity>`, and a test compares at max(standing tolerance, 10 x floor) -- for
dL_dthetaL, which has no standing tolerance, at 10 x floor.  `flat_line_brent` stands in for `brent` in the reference's module
exactly as there.  A run that is not stationary by the reference's own residual is refused; each case takes the first data seed
of a fixed list whose run is accepted.

With that line search the reference's Newton iteration converges quadratically and its runs at 1e-10 and 1e-8 stop at the same
iterate in every Student-t case tried (20 seeds): the stored floor of dL_dthetaL is then exactly 0, and 10 x 0 is a tolerance no
second floating-point evaluation of the same sums can meet.  The fixture therefore also stores `ref_rounding_dL_dthetaL`, the
forward rounding-error bound of the reference's own evaluation of dL_dthetaL (4 N accumulations at unit roundoff 2^-53 times the
sum of the absolute values of the terms, relative to the result), and a test compares dL_dthetaL at 10 x max(floor, that bound).

The reference integrates a likelihood's predictive mean and variance numerically (`likelihood.py:413-497`); the package uses
closed forms.  For the Poisson cases the fixture stores the reference's values, and `closed_form_diff_<quantity>` = the relative
difference between the closed form (evaluated here, in NumPy, on the reference's latent mean and variance) and the reference.
Where that exceeds 1e-6 the case's predictive check is dropped and `note` says so (at most one Poisson case).  One of the three
integrals of the reference's predictive variance runs over an empty interval; `missing_term` says what is stored for it.

`likelihood_values.npz`: every method of the two likelihoods and of the `Identity` and `Log` links on a grid of f.
`robust_toy_optimize.npz`: a sine with corrupted points; the reference's Gaussian and Student-t (Laplace) fits after 20
L-BFGS-B iterations from the default start and their errors against the clean function.

    python tools/make_golden_laplace_lik.py
"""
import importlib
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from oracle import ref_loader  # noqa: E402
import make_golden_mlp as mlp  # noqa: E402
import make_golden_laplace as G  # noqa: E402  (flat_line_brent, leaf, grads, rel: the conventions of the Bernoulli fixtures)

OUT = os.path.join(ROOT, "tests", "golden", "laplace_lik")
STANDING = {"lml": 1e-10, "f_hat": 1e-9, "Ki_fhat": 1e-9, "dtheta": 1e-8, "pred_mu": 1e-9, "pred_var": 1e-9,
            "pred_ymean": 1e-9, "pred_yvar": 1e-9, "dL_dthetaL": 0.0}


def student_t(ns, deg_free, sigma2):
    """the reference's StudentT; paramz resolves a linked parameter by its name (`self.deg_free`, student_t.py:290,303), which
    the parameter stub of oracle/ does not do, so the name is set here on the object"""
    lik = ns.StudentTClass(deg_free=deg_free, sigma2=sigma2)
    lik.deg_free = lik.v
    return lik


def make_lik(ns, lik, theta):
    return ns.StudentT(deg_free=theta[1], sigma2=theta[0]) if lik == "studentt" else ns.Poisson()


def missing_term(lik, mu, var):
    """E[E(y* | f*)^2] over f* ~ N(mu, var), the third integral of the reference's `predictive_variance`.  The reference
    integrates it from +inf to +inf (`likelihood.py:456,490`: `fmin_m = np.inf`), so it comes out 0 and the reference returns
    E[V(y* | f*)] - E(y*)^2, which is negative wherever the mean is large.  The term is restored here with the reference's own
    integrand (its `conditional_mean`, its cut of the density below 1e-10) and the same `quad` over the whole line; the
    fixtures store the sum as `pred_yvar` and what the reference returns as `pred_yvar_reference_as_is`."""
    from scipy.integrate import quad

    def integrand(f, m, v):
        p = np.exp(-(0.5 / v) * np.square(f - m))
        return 0.0 if p < 1e-10 else float(np.ravel(lik.conditional_mean(f))[0]) ** 2 * p
    vals = [quad(integrand, -np.inf, np.inf, args=(float(m), float(v)))[0] for m, v in zip(mu[:, 0], var[:, 0])]
    return np.array(vals)[:, None] / np.sqrt(2 * np.pi * var)


def run(ns, lik_name, lik_theta, specs, X, Y, tol, Xs):
    k, leaves = mlp.assemble(ns, specs)
    lik = make_lik(ns, lik_name, lik_theta)
    inf = ns.Laplace()
    inf._mode_finding_tolerance, inf._mode_finding_max_iter = tol, 100
    post, lml, gd = inf.inference(k, X, lik, Y)
    k.update_gradients_full(gd["dL_dK"], X)
    mu, var = post._raw_predict(k, Xs, pred_var=X, full_cov=False)
    ymean, yvar_raw = lik.predictive_values(mu, var)
    yvar = np.asarray(yvar_raw, float) + missing_term(lik, np.asarray(mu), np.asarray(var))
    f_hat, Ki = np.asarray(inf.f_hat), np.asarray(post.woodbury_vector)
    resid = float(np.abs(np.asarray(k.K(X)) @ (np.asarray(lik.dlogpdf_df(f_hat, Y)) - Ki)).max() / np.abs(f_hat).max())
    rounding = 0.0
    if lik.size:
        # forward rounding-error bound of the reference's own dL_dthetaL (`laplace.py:285-296`): sums and products of N terms
        # nested four deep, so n = 4 N accumulations at unit roundoff 2^-53 times the sum of the absolute values of the terms
        Kd, KWi, d = np.abs(np.asarray(k.K(X))), np.abs(np.asarray(post.woodbury_inv)), np.diag(np.asarray(inf.Ki_W_i))
        u = np.abs(-0.5 * d[:, None] * -np.asarray(lik.d3logpdf_df3(f_hat, Y)))
        s_abs = Kd @ (u + KWi @ (Kd @ u))
        dl, dg, dh = lik._laplace_gradients(f_hat, Y)
        A = np.array([np.abs(dl[i]).sum() + 0.5 * np.abs(d * dh[i][:, 0]).sum() + float(s_abs[:, 0] @ np.abs(dg[i][:, 0]))
                      for i in range(lik.size)])
        rounding = float(np.linalg.norm(4 * X.shape[0] * 2.0 ** -53 * A) / np.linalg.norm(np.asarray(gd["dL_dthetaL"], float)))
    return dict(ref_rounding_dL_dthetaL=rounding, ref_mode_residual=resid, lml=float(lml), f_hat=f_hat, Ki_fhat=Ki, dtheta=np.concatenate([G.grads(p) for p in leaves]),
                dL_dthetaL=np.asarray(gd["dL_dthetaL"], float), pred_mu=np.asarray(mu), pred_var=np.asarray(var),
                pred_ymean=np.asarray(ymean, float), pred_yvar=np.asarray(yvar, float), pred_yvar_reference_as_is=np.asarray(yvar_raw, float), W=np.asarray(inf.W))


def case(ns, name, lik_name, lik_theta, X, Y, specs, seed=0, dropped=[]):
    rng = np.random.default_rng(seed + 7)
    lo, hi = X.min(0), X.max(0)
    Xs = lo + (hi - lo) * rng.random((25, X.shape[1]))
    r = run(ns, lik_name, lik_theta, specs, X, Y, 1e-10, Xs)
    if r["ref_mode_residual"] > 1e-10:
        print("%s REFUSED: the reference stopped short of the mode (residual %.1e)" % (name, r["ref_mode_residual"]))
        return False
    r2 = run(ns, lik_name, lik_theta, specs, X, Y, 1e-8, Xs)
    floors = {"ref_floor_" + q: (G.rel(r2[q], r[q]) if np.size(r[q]) else 0.0) for q in STANDING}
    extra, note = {}, ""
    if lik_name == "poisson":
        mu, v = r["pred_mu"], r["pred_var"]
        closed = {"pred_ymean": np.exp(mu + 0.5 * v), "pred_yvar": np.exp(mu + 0.5 * v) + np.expm1(v) * np.exp(2.0 * mu + v)}
        for q in closed:
            extra["closed_form_diff_" + q] = G.rel(closed[q], r[q])
        worst = max(extra.values())
        if worst > 1e-6:
            if dropped:
                raise RuntimeError("%s: a second Poisson case whose closed form is %.1e from the reference" % (name, worst))
            dropped.append(name)
            note = "predictive check dropped: closed form and the reference's quadrature differ by %.1e (relative)" % worst
    spec_json = json.dumps([[s[0], int(s[1]), [float(v) for v in s[2]], [int(d) for d in s[3]], int(s[4])] for s in specs])
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, X=X, Y=Y, Xs=Xs, specs=spec_json, lik=lik_name, lik_theta=np.asarray(lik_theta, float), note=note,
                        **r, **floors, **extra)
    print("%-36s residual %.1e  lml=% .12e  min W=%.1e  %d bytes %s" % (name, r["ref_mode_residual"], r["lml"], r["W"].min(),
                                                                     os.path.getsize(path), note))
    print("    dL_dthetaL", r["dL_dthetaL"], {k: "%.1e" % v for k, v in extra.items()})
    for q in STANDING:
        f = floors["ref_floor_" + q]
        print("    %-13s floor %.2e -> tolerance %.1e" % (q, f, max(STANDING[q], 10 * f)))
    print("    rounding bound of dL_dthetaL %.2e" % r["ref_rounding_dL_dthetaL"])
    return True


def first_accepted(ns, name, lik_name, lik_theta, data, specs, seeds, seed=0):
    """the first data seed of a fixed list whose run `case` accepts (stationary by the reference's own residual, floors measured)"""
    for sd in seeds:
        X, Y = data(sd)
        if case(ns, name, lik_name, lik_theta, X, Y, specs, seed=seed):
            return
    raise RuntimeError("%s: no seed of %r gave a run the generator accepts" % (name, list(seeds)))


def smooth(X, seed):
    """a smooth function of the inputs with unit-order amplitude"""
    w = np.random.default_rng(seed).standard_normal(X.shape[1])
    return np.sin(X @ w) + 0.3 * np.cos(2.0 * X[:, 0])


def robust_data(N, D, seed, outliers=0.0):
    """smooth function + Gaussian noise (0.2); a share `outliers` of the rows shifted by +-5"""
    rng = np.random.default_rng(seed)
    X = np.sort(rng.uniform(-3.0, 3.0, (N, 1)), 0) if D == 1 else rng.standard_normal((N, D))
    Y = smooth(X, seed) + 0.2 * rng.standard_normal(N)
    idx = rng.choice(N, int(round(outliers * N)), replace=False)
    Y[idx] += 5.0 * np.where(rng.random(idx.size) < 0.5, -1.0, 1.0)
    return np.ascontiguousarray(X), Y[:, None].copy()


def count_data(N, D, seed):
    rng = np.random.default_rng(seed)
    X = np.sort(rng.uniform(-3.0, 3.0, (N, 1)), 0) if D == 1 else rng.standard_normal((N, D))
    return np.ascontiguousarray(X), rng.poisson(np.exp(0.5 + 0.7 * smooth(X, seed)))[:, None].astype(float)


def likelihood_values(ns):
    out = {}
    f = np.concatenate([np.linspace(-12, 12, 97), [-8.3, -0.66, 0.0, 0.66, 5.7]])[:, None]
    out["f"] = f
    for tag, (s2, v) in (("a", (2.0, 5.0)), ("b", (0.3, 2.5)), ("c", (4.5, 40.0))):
        lik = ns.StudentT(deg_free=v, sigma2=s2)
        out["studentt_%s_theta" % tag] = np.array([s2, v])
        for yv in (-1.5, 0.25, 6.0):
            y = np.full_like(f, yv)
            key = "studentt_%s_y%g_" % (tag, yv)
            for m in ("logpdf", "dlogpdf_df", "d2logpdf_df2", "d3logpdf_df3", "dlogpdf_link_dvar", "dlogpdf_dlink_dvar",
                      "d2logpdf_dlink2_dvar", "dlogpdf_link_dv", "dlogpdf_dlink_dv", "d2logpdf_dlink2_dv"):
                out[key + m] = np.asarray(getattr(lik, m)(f, y), float)
            for m, a in zip(("dlogpdf_dtheta", "dlogpdf_df_dtheta", "d2logpdf_df2_dtheta"), lik._laplace_gradients(f, y)):
                out[key + m] = np.asarray(a, float)
        var = np.linspace(0.01, 9.0, f.size)[:, None]
        out["studentt_%s_pm_var" % tag] = var
        out["studentt_%s_predictive_mean" % tag] = np.asarray(lik.predictive_mean(f, var), float)
        out["studentt_%s_conditional_variance" % tag] = np.asarray(lik.conditional_variance(f), float)
    lik = ns.StudentT(deg_free=1.5, sigma2=1.0)
    out["studentt_low_predictive_variance"] = np.asarray(lik.predictive_variance(f, np.ones_like(f)), float)
    fp = np.concatenate([np.linspace(-30, 30, 121), [-700.0, -0.66, 0.66, 5.7]])[:, None]
    out["poisson_f"] = fp
    lik = ns.Poisson()
    for yv in (0, 1, 7, 250):
        y = np.full_like(fp, float(yv))
        with np.errstate(all="ignore"):
            for m in ("logpdf", "dlogpdf_df", "d2logpdf_df2", "d3logpdf_df3"):
                out["poisson_y%d_%s" % (yv, m)] = np.asarray(getattr(lik, m)(fp, y), float)
    out["poisson_conditional_mean"] = np.asarray(lik.conditional_mean(fp), float)
    out["poisson_conditional_variance"] = np.asarray(lik.conditional_variance(fp), float)
    fl = np.concatenate([np.linspace(-50, 50, 41), [-745.0, 709.0, 710.0, 800.0]])[:, None]
    out["link_f"] = fl
    for name, link in (("identity", ns.Identity()), ("log", ns.Log())):
        for m in ("transf", "dtransf_df", "d2transf_df2", "d3transf_df3"):
            out["%s_%s" % (name, m)] = np.asarray(getattr(link, m)(fl), float)
    np.savez_compressed(os.path.join(OUT, "likelihood_values.npz"), **out)
    print("likelihood_values.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(os.path.join(OUT, "likelihood_values.npz"))))


def robust_toy(ns):
    """the reference example's shape (`GPy/examples/regression.py`, toy Student-t regression: a sine, a few corrupted points):
    both models optimised by L-BFGS-B over log-parameters for 20 iterations from the default start"""
    from scipy.optimize import minimize
    rng = np.random.default_rng(12)
    X = np.sort(rng.uniform(0.0, 10.0, (150, 1)), 0)
    Y = np.sin(X) + 0.1 * rng.standard_normal(X.shape)
    idx = rng.choice(150, 15, replace=False)
    Y[idx, 0] += 5.0 * np.where(rng.random(15) < 0.5, -1.0, 1.0)
    Xt = np.linspace(0.2, 9.8, 60)[:, None]
    ft = np.sin(Xt)

    def evaluate(z, student):
        k = ns.RBF(1, variance=np.exp(z[0]), lengthscale=np.exp(z[1]))
        if student:
            lik, inf = ns.StudentT(deg_free=np.exp(z[3]), sigma2=np.exp(z[2])), ns.Laplace()
        else:
            lik, inf = ns.Gaussian(variance=np.exp(z[2])), ns.ExactGaussianInference()
        post, lml, gd = inf.inference(k, X, lik, Y)
        k.update_gradients_full(gd["dL_dK"], X)
        gl = np.atleast_1d(np.asarray(gd["dL_dthetaL"], float)).ravel()
        g = np.concatenate([[float(k.variance.gradient), float(k.lengthscale.gradient)], gl]) * np.exp(z)
        return k, post, float(lml), g
    out = dict(X=X, Y=Y, Xt=Xt, ft=ft)
    for student, z0 in ((False, np.zeros(3)), (True, np.log([1.0, 1.0, 2.0, 5.0]))):
        tag = "studentt" if student else "gaussian"
        lml0 = evaluate(z0, student)[2]
        res = minimize(lambda z: (lambda r: (-r[2], -r[3]))(evaluate(z, student)), z0, jac=True, method="L-BFGS-B",
                       options={"maxiter": 20})
        k, post, lml1, _ = evaluate(res.x, student)
        mu, _ = post._raw_predict(k, Xt, pred_var=X)
        err = float(np.sqrt(np.mean(np.square(np.asarray(mu) - ft))))
        out.update({tag + "_lml_start": lml0, tag + "_lml_end": lml1, tag + "_rmse": err, tag + "_theta_end": np.exp(res.x)})
        print("robust_toy %-8s lml %.6f -> %.6f, rmse to the clean function %.4f, theta %s" % (tag, lml0, lml1, err, np.exp(res.x)))
    if not (out["studentt_lml_end"] > out["studentt_lml_start"] and out["studentt_rmse"] < out["gaussian_rmse"]):
        raise RuntimeError("the reference itself does not show the Student-t fit closer to the clean function for this seed")
    np.savez_compressed(os.path.join(OUT, "robust_toy_optimize.npz"), **out)


def main():
    ns = ref_loader.load_sum_kernels(ref_loader.load())
    ns.Linear = importlib.import_module("GPy.kern.src.linear").Linear
    ns.StdPeriodic = importlib.import_module("GPy.kern.src.standard_periodic").StdPeriodic
    ns.StudentTClass = importlib.import_module("GPy.likelihoods.student_t").StudentT
    ns.StudentT = lambda deg_free, sigma2: student_t(ns, deg_free, sigma2)
    ns.Poisson = importlib.import_module("GPy.likelihoods.poisson").Poisson
    links = importlib.import_module("GPy.likelihoods.link_functions")
    ns.Identity, ns.Log = links.Identity, links.Log
    lap = importlib.import_module("GPy.inference.latent_function_inference.laplace")
    ns.Laplace = lap.Laplace
    lap.optimize = types.SimpleNamespace(brent=G.flat_line_brent)     # the module's own name for scipy.optimize
    G._leaf, mlp.leaf = mlp.leaf, G.leaf
    os.makedirs(OUT, exist_ok=True)
    d2, d3 = [0, 1], [0, 1, 2]
    # Where a W is negative the reference clips it inside the B statistics only (`laplace.py:319-321`) while b = W f + grad keeps
    # the unclipped one (`:191-193`), so its iteration settles away from the mode and the residual check of `case` refuses the
    # run (seen here: residual 0.9 with t_scale2 = 0.5, deg_free = 4 on the outlier data).  The outlier case therefore takes a
    # scale at which every W at the mode is positive (deg_free t_scale2 = 48 > the largest squared residual, about 31)
    first_accepted(ns, "studentt_rbf_iso_n150_d1", "studentt", [8.0, 6.0], lambda sd: robust_data(150, 1, sd, outliers=0.10),
                   [("rbf", 0, [1.5, 0.9], [0], 0)], range(61, 81))
    first_accepted(ns, "studentt_matern52_ard_n140_d3", "studentt", [0.3, 5.0], lambda sd: robust_data(140, 3, sd),
                   [("matern52", 1, [2.0, 1.2, 0.8, 1.6], d3, 0)], range(62, 82), seed=1)
    first_accepted(ns, "studentt_rbf_linear_bias_n140_d3", "studentt", [2.0, 3.5], lambda sd: robust_data(140, 3, sd),
                   [("rbf", 0, [1.2, 0.9], d3, 0), ("linear", 0, [0.4], d3, 0), ("bias", 0, [0.3], d3, 0)], range(62, 82), seed=2)
    first_accepted(ns, "poisson_rbf_iso_n150_d2", "poisson", [], lambda sd: count_data(150, 2, sd), [("rbf", 0, [1.0, 0.7], d2, 0)],
                   range(63, 83), seed=3)
    first_accepted(ns, "poisson_stdperiodic_n130_d1", "poisson", [], lambda sd: count_data(130, 1, sd),
                   [("stdperiodic", 0, [1.3, 5.0, 0.9], [0], 0)], range(64, 84), seed=4)
    likelihood_values(ns)
    robust_toy(ns)


if __name__ == "__main__":
    main()
