"""Fixtures tests/golden/ep/*.npz FROM THE REFERENCE'S OWN CODE: `EP` (GPy/inference/latent_function_inference/
expectation_propagation.py), `Bernoulli` with the `Probit` link, the kernels, `update_gradients_full` and
`PosteriorEP._raw_predict`, executed through oracle/ref_loader.py (imported, unchanged).  Only data goes into the fixtures.

The reference's `EP` is subclassed for one purpose: `_local_updates` draws each sweep's permutation here, passes it as
`update_order` (the reference's own hook) and records it, so that an implementation can follow the same trajectory.  With the
same orders and the same stopping rule there is no convergence floor; what limits agreement is how EP amplifies rounding.
That is measured on the reference alone: every case is run a second time with the same orders and `K=` perturbed
symmetrically by a relative 2^-52 random factor, and the relative change of every quantity is stored as
`ref_floor_<quantity>`.  A test compares at max(standing tolerance, 10 x floor); the standing tolerances are those of the
Laplace fixtures (scalars 1e-10, vectors 1e-9 -- the site parameters among them --, gradients 1e-8, prediction 1e-9).

Enforced on the reference alone (RuntimeError otherwise): every case converges (`_stop_criteria`) within 100 sweeps, the
perturbed run takes the same number of sweeps, and at least five cases never had a site's tau clamped.

`bernoulli_ep_moments.npz`: the reference's moment matching for both labels over tau in [1e-8, 1e4] and v / tau in [-40, 40],
stored as log Z_hat, mu_hat, sigma2_hat, with the largest relative difference between the reference's helper and the same
formulas (bernoulli.py:74-79) evaluated with scipy.special, per quantity.  `toy_1d_optimize.npz`: the toy data of the Laplace
fixtures with the reference's own EP run ("alternated") optimised by L-BFGS-B from the default start.

    python tools/make_golden_ep.py
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
import make_golden_laplace as gl  # noqa: E402  (leaf, two_class, grads, rel)

OUT = os.path.join(ROOT, "tests", "golden", "ep")
STANDING = {"lml": 1e-10, "log_Z_tilde": 1e-10, "tau_tilde": 1e-9, "v_tilde": 1e-9, "cav_tau": 1e-9, "cav_v": 1e-9, "alpha": 1e-9,
            "Wi": 1e-9, "dL_dK": 1e-8, "dtheta": 1e-8, "pred_mu": 1e-9, "pred_var": 1e-9, "pred_cov": 1e-9, "pred_p": 1e-9}
EPS = np.finfo(float).eps


def recording_ep(EP):
    class RecordingEP(EP):
        """the reference's EP; the permutation of every sweep is drawn (or replayed) here and handed to the reference's hook"""
        rng = None
        replay = None

        def _local_updates(self, num_data, cav_params, post_params, marg_moments, ga_approx, likelihood, Y, Y_metadata,
                           update_order=None):
            k = len(self.orders)
            order = self.replay[k] if self.replay is not None else self.rng.permutation(num_data)
            self.orders.append(np.asarray(order, dtype=np.int64))
            super(RecordingEP, self)._local_updates(num_data, cav_params, post_params, marg_moments, ga_approx, likelihood, Y,
                                                    Y_metadata, update_order=order)
            self.clamped = self.clamped or bool(np.any(ga_approx.tau <= EPS))

        def _stop_criteria(self, ga_approx):
            self.last_stop = bool(super(RecordingEP, self)._stop_criteria(ga_approx))
            return self.last_stop
    return RecordingEP


def bernoulli(ns):
    lik = ns.Bernoulli()
    lik.num_params = 0           # paramz's count of parameters, which the test-only paramz stand-in does not keep (likelihood.py:308)
    return lik


def run(ns, specs, X, Y, Xs, seed, opts, replay=None, perturb=None):
    k, leaves = mlp.assemble(ns, specs)
    lik = bernoulli(ns)
    inf = ns.RecordingEP(max_iters=100, **opts)
    inf.rng, inf.replay, inf.orders, inf.clamped, inf.last_stop = np.random.default_rng(seed), replay, [], False, False
    K = None
    if perturb is not None:
        K = np.asarray(k.K(X)).copy()
        R = np.random.default_rng(perturb).uniform(-1.0, 1.0, K.shape)
        K *= 1.0 + 2.0 ** -52 * np.triu(R) + 2.0 ** -52 * np.triu(R, 1).T
    post, lml, gd = inf.inference(k, ns.ObsAr(X), lik, ns.ObsAr(Y), K=K)
    if not inf.last_stop:
        raise RuntimeError("the reference's EP did not converge within 100 sweeps")
    k.update_gradients_full(gd["dL_dK"], X)
    mu, var = post._raw_predict(k, Xs, pred_var=X, full_cov=False)
    _, cov = post._raw_predict(k, Xs, pred_var=X, full_cov=True)
    _, ga, cav, lz = inf._ep_approximation
    r = dict(lml=float(lml), log_Z_tilde=float(lz), tau_tilde=np.asarray(ga.tau), v_tilde=np.asarray(ga.v), cav_tau=np.asarray(cav.tau),
             cav_v=np.asarray(cav.v), alpha=np.asarray(post.woodbury_vector), Wi=np.asarray(post.woodbury_inv),
             dL_dK=np.asarray(gd["dL_dK"]), dtheta=np.concatenate([gl.grads(p) for p in leaves]), pred_mu=np.asarray(mu),
             pred_var=np.asarray(var), pred_cov=np.asarray(cov), pred_p=np.asarray(lik.predictive_values(mu, var)[0]))
    return r, inf


def change(a, b, scalar):
    return abs(a - b) / abs(b) if scalar else gl.rel(a, b)


def case(ns, name, X, Y, specs, seed=0, **opts):
    rng = np.random.default_rng(seed + 7)
    lo, hi = X.min(0), X.max(0)
    Xs = lo + (hi - lo) * rng.random((13, X.shape[1]))
    r, inf = run(ns, specs, X, Y, Xs, seed + 100, opts)
    r2, inf2 = run(ns, specs, X, Y, Xs, seed + 100, opts, replay=inf.orders, perturb=seed + 200)
    if len(inf2.orders) != len(inf.orders):
        raise RuntimeError("%s: a 2^-52 perturbation of K changed the number of sweeps (%d -> %d)" % (name, len(inf.orders), len(inf2.orders)))
    floors = {"ref_floor_" + q: change(r2[q], r[q], q in ("lml", "log_Z_tilde")) for q in STANDING}
    spec_json = json.dumps([[s[0], int(s[1]), [float(v) for v in s[2]], [int(d) for d in s[3]], int(s[4])] for s in specs])
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, X=X, Y=Y, Xs=Xs, specs=spec_json, orders=np.array(inf.orders), sweeps=len(inf.orders),
                        clamped=inf.clamped, parallel_updates=bool(opts.get("parallel_updates", False)),
                        eta=float(opts.get("eta", 1.0)), delta=float(opts.get("delta", 1.0)), epsilon=float(inf.epsilon), **r, **floors)
    print("%-40s sweeps %3d  clamped %d  lml=% .12e  %d bytes" % (name, len(inf.orders), inf.clamped, r["lml"], os.path.getsize(path)))
    for q in STANDING:
        f = floors["ref_floor_" + q]
        print("    %-12s floor %.2e -> tolerance %.1e" % (q, f, max(STANDING[q], 10 * f)))
    return inf.clamped


def moments(ns):
    from scipy import special
    lik = ns.Bernoulli()
    ug = importlib.import_module("GPy.util.univariate_Gaussian")
    tau = np.logspace(-8, 4, 25)
    ratio = np.concatenate([np.linspace(-40, 40, 33), [-8.3, -0.66, 0.66, 5.7]])
    T, Rr = [a.ravel() for a in np.meshgrid(tau, ratio, indexing="ij")]
    V = T * Rr
    out, worst = {"tau": T, "v": V}, {"log_Z_hat": 0.0, "mu_hat": 0.0, "sigma2_hat": 0.0}
    for yv in (0, 1):
        sign = 1.0 if yv == 1 else -1.0
        got = np.array([lik.moments_match_ep(yv, t, v)[1:] for t, v in zip(T, V)])
        z = sign * V / np.sqrt(T ** 2 + T)
        lz = np.array([ug.logCdfNormal(zi) for zi in z])            # the log Z_hat that moments_match_ep exponentiates
        out["log_Z_hat_y%d" % yv], out["mu_hat_y%d" % yv], out["sigma2_hat_y%d" % yv] = lz, got[:, 0], got[:, 1]
        # the same formulas (bernoulli.py:74-79) with scipy.special in place of the reference's helper
        s_lz = special.log_ndtr(z)
        s_r = np.exp(-0.5 * z * z - 0.5 * np.log(2 * np.pi) - s_lz)
        s_mu = V / T + sign * s_r / np.sqrt(T ** 2 + T)
        s_s2 = 1.0 / T - (s_r / (T ** 2 + T)) * (z + s_r)
        for q, a, b in (("log_Z_hat", lz, s_lz), ("mu_hat", got[:, 0], s_mu), ("sigma2_hat", got[:, 1], s_s2)):
            worst[q] = max(worst[q], float(np.max(np.abs(a - b) / np.where(b != 0, np.abs(b), 1.0))))
    for q in worst:
        out["ref_vs_scipy_" + q] = worst[q]
    np.savez_compressed(os.path.join(OUT, "bernoulli_ep_moments.npz"), **out)
    print("bernoulli_ep_moments: %d points per label, reference's helper against scipy.special: %s" % (T.size, worst))


def toy_1d(ns):
    """the toy data of tests/golden/laplace/toy_1d_optimize.npz; the reference's own EP in "alternated" mode, L-BFGS-B on the
    log parameters from the default start, EP rerun at the start of every optimisation round (three rounds)"""
    from scipy.optimize import minimize
    z0 = np.load(os.path.join(ROOT, "tests", "golden", "laplace", "toy_1d_optimize.npz"))
    X, Y = z0["X"], z0["Y"]
    inf = ns.RecordingEP(max_iters=100)
    inf.rng, inf.replay, inf.orders, inf.clamped, inf.last_stop = np.random.default_rng(11), None, [], False, False
    lik = bernoulli(ns)

    def evaluate(z):
        k = ns.RBF(1, variance=np.exp(z[0]), lengthscale=np.exp(z[1]))
        post, lml, gd = inf.inference(k, ns.ObsAr(X), lik, ns.ObsAr(Y))
        k.update_gradients_full(gd["dL_dK"], X)
        g = np.array([np.ravel(k.variance.gradient)[0], np.ravel(k.lengthscale.gradient)[0]], dtype=float) * np.exp(z)
        return k, post, float(lml), g
    z = np.zeros(2)
    lml0 = evaluate(z)[2]
    inf.on_optimization_start()
    res = minimize(lambda zz: (lambda r: (-r[2], -r[3]))(evaluate(zz)), z, jac=True, method="L-BFGS-B")
    k, post, lml1, _ = evaluate(res.x)
    mu, var = post._raw_predict(k, X, pred_var=X)
    p = lik.predictive_values(mu, var)[0]
    acc = float(np.mean((p > 0.5) == (Y == 1)))
    np.savez_compressed(os.path.join(OUT, "toy_1d_optimize.npz"), X=X, Y=Y, lml_start=lml0, lml_end=lml1, accuracy=acc,
                        theta_end=np.exp(res.x))
    print("toy_1d_optimize: lml %.6f -> %.6f, training accuracy %.4f, theta %s" % (lml0, lml1, acc, np.exp(res.x)))


def main():
    ns = ref_loader.load_sum_kernels(ref_loader.load())
    ns.Linear = importlib.import_module("GPy.kern.src.linear").Linear
    ns.MLP = importlib.import_module("GPy.kern.src.mlp").MLP
    ns.Poly = importlib.import_module("GPy.kern.src.poly").Poly
    ns.Coregionalize = importlib.import_module("GPy.kern.src.coregionalize").Coregionalize
    ns.StdPeriodic = importlib.import_module("GPy.kern.src.standard_periodic").StdPeriodic
    ns.Bernoulli = importlib.import_module("GPy.likelihoods.bernoulli").Bernoulli
    # names the reference's EP module imports from packages that are stubs here
    lfi, liks = sys.modules["GPy.inference.latent_function_inference"], sys.modules["GPy.likelihoods"]
    lfi.ExactGaussianInference = ns.ExactGaussianInference
    lfi.VarDTC = type("VarDTC", (), {})
    liks.Gaussian = ns.Gaussian
    ns.ObsAr = importlib.import_module("paramz").ObsAr
    ns.RecordingEP = recording_ep(importlib.import_module("GPy.inference.latent_function_inference.expectation_propagation").EP)
    gl._leaf, mlp.leaf = mlp.leaf, gl.leaf
    os.makedirs(OUT, exist_ok=True)
    X1, Y1 = gl.two_class(130, 1, 51, 2.0)
    X2, Y2 = gl.two_class(150, 2, 52, 2.0)
    X3, Y3 = gl.two_class(140, 3, 53, 2.5)
    Xw, Yw = gl.two_class(120, 2, 54, 9.0)
    Xo, Yo = gl.two_class(160, 2, 55, 0.4)
    d2, d3 = [0, 1], [0, 1, 2]
    rbf = [("rbf", 0, [1.5, 1.1], d2, 0)]
    mat = [("matern52", 1, [2.0, 1.2, 0.8, 1.6], d3, 0)]
    clamped = [
        case(ns, "rbf_iso_n150_d2", X2, Y2, rbf),
        case(ns, "matern52_ard_n140_d3", X3, Y3, mat, seed=1),
        case(ns, "rbf_linear_bias_n140_d3", X3, Y3,
             [("rbf", 0, [1.2, 0.9], d3, 0), ("linear", 0, [0.4], d3, 0), ("bias", 0, [0.3], d3, 0)], seed=2),
        case(ns, "mlp0_x_rbf12_n140_d3", X3, Y3, [("mlp", 0, [1.5, 0.9, 0.7], [0], 1), ("rbf", 1, [1.2, 0.8, 1.4], [1, 2], 1)], seed=3),
        case(ns, "stdperiodic_n130_d1", X1, Y1, [("stdperiodic", 0, [1.3, 5.0, 0.9], [0], 0)], seed=4),
        case(ns, "separated_rbf_n120_d2", Xw, Yw, [("rbf", 0, [6.0, 1.5], d2, 0)], seed=5),
        case(ns, "overlapping_rbf_n160_d2", Xo, Yo, [("rbf", 0, [1.0, 1.0], d2, 0)], seed=6),
    ]
    if clamped.count(False) < 5:
        raise RuntimeError("a site's tau was clamped in %d of the seven sequential cases" % clamped.count(True))
    case(ns, "parallel_rbf_iso_n150_d2", X2, Y2, rbf, seed=7, parallel_updates=True)
    case(ns, "parallel_matern52_ard_n140_d3", X3, Y3, mat, seed=8, parallel_updates=True)
    case(ns, "fractional_rbf_iso_n150_d2", X2, Y2, rbf, seed=9, eta=0.9, delta=0.8)
    moments(ns)
    toy_1d(ns)


if __name__ == "__main__":
    main()
