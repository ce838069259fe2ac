"""Fixtures tests/golden/epdtc/*.npz FROM THE REFERENCE'S OWN CODE: `EPDTC` (GPy/inference/latent_function_inference/
expectation_propagation.py:436-578) over `VarDTC`, `Bernoulli` with the `Probit` link, the kernels' `update_gradients_diag` /
`update_gradients_full` / `gradients_X` assembled as GPy/core/sparse_gp.py:108-119 does, and `Posterior._raw_predict` at 13 new
points, executed through oracle/ref_loader.py (imported, unchanged).  Only data goes into the fixtures.

The reference's `EPDTC` is subclassed for one purpose: `_local_updates` draws each sweep's permutation here, passes it as
`update_order` (the reference's own hook) and records it, as tools/make_golden_ep.py does for `EP`.

Inputs: two-class data in the unit cube centred at the origin and Z on a jittered regular grid with lengthscales of 0.75 grid
spacings (tools/make_golden_svgp.py's recipe), so that cond(Kmm) stays far below 1e6.  While a case runs, every call of the
reference's `jitchol` is watched: a fixture whose run entered the jitter ladder (a second `jitchol` attempt) is REFUSED -- the
reference's numbers with added jitter are no fixture -- and so is one whose EP did not converge within 100 sweeps.

`toy_1d_optimize.npz`: the 1-D toy problem; the reference's bound before and after L-BFGS-B over (Z, log kernel parameters), the
flat order of the package's `SparseGP`, with EP in "alternated" mode rerun at the start of the optimisation.

    python tools/make_golden_epdtc.py
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

OUT = os.path.join(ROOT, "tests", "golden", "epdtc")
EPS = np.finfo(float).eps
LADDER = {"entered": False}


def recording_epdtc(EPDTC):
    class RecordingEPDTC(EPDTC):
        rng = None
        replay = None

        def _local_updates(self, num_data, LLT0, LLT, Kmn, cav_params, post_params, marg_moments, ga_approx, likelihood, Y,
                           Y_metadata, update_order=None):
            k = len(self.orders)
            order = self.replay[k] if self.replay is not None else self.rng.permutation(num_data)
            self.orders.append(np.asarray(order, dtype=np.int64))
            super(RecordingEPDTC, self)._local_updates(num_data, LLT0, LLT, Kmn, cav_params, post_params, marg_moments, ga_approx,
                                                       likelihood, Y, Y_metadata, update_order=order)
            self.cav = cav_params
            self.log_Z_hat = np.log(marg_moments.Z_hat)
            self.clamped = self.clamped or bool(np.any(ga_approx.tau <= EPS))

        def _stop_criteria(self, ga_approx):
            self.last_stop = bool(super(RecordingEPDTC, self)._stop_criteria(ga_approx))
            return self.last_stop
    return RecordingEPDTC


def watch_jitchol():
    """wraps the reference's jitter ladder where its modules look it up: a run that gets past the plain attempt is marked"""
    la = importlib.import_module("GPy.util.linalg")
    plain = la.jitchol

    def jitchol(A, maxtries=5):
        L, info = la.lapack.dpotrf(np.ascontiguousarray(A), lower=1)          # jitchol's own first attempt (util/linalg.py:62-65)
        if info == 0:
            return L
        LADDER["entered"] = True
        return plain(A, maxtries)
    for mod in ("GPy.util.linalg", "GPy.inference.latent_function_inference.expectation_propagation",
                "GPy.inference.latent_function_inference.var_dtc"):
        m = sys.modules.get(mod)
        if m is not None and hasattr(m, "jitchol"):
            m.jitchol = jitchol


def bernoulli(ns):
    lik = ns.Bernoulli()
    lik.num_params = 0           # paramz's count of parameters, which the test-only paramz stand-in does not keep
    lik.exact_inference_gradients = lambda dL_dKdiag, Y_metadata=None: np.zeros(0)
    return lik


def new_inf(ns, seed, opts, replay=None):
    inf = ns.RecordingEPDTC(max_iters=100, **opts)
    inf.rng, inf.replay, inf.orders, inf.clamped, inf.last_stop = np.random.default_rng(seed), replay, [], False, False
    return inf


def evaluate(ns, inf, specs, X, Y, Z, Xs=None):
    """one EPDTC.inference + the gradient assembly of core/sparse_gp.py:108-119 (+ predictions at Xs)"""
    k, leaves = assemble(ns, specs)
    lik = bernoulli(ns)
    post, lml, gd = inf.inference(k, X, Z, lik, ns.ObsAr(Y))
    k.update_gradients_diag(gd["dL_dKdiag"], X)
    g = grads(leaves)
    k.update_gradients_full(gd["dL_dKnm"], X, Z)
    g = g + grads(leaves)
    k.update_gradients_full(gd["dL_dKmm"], Z, None)
    g = g + grads(leaves)
    dZ = k.gradients_X(gd["dL_dKmm"], Z) + k.gradients_X(gd["dL_dKnm"].T, Z, X)
    _, ga, lz = inf._ep_approximation
    out = dict(lml=float(np.squeeze(lml)), log_Z_tilde=float(lz), tau_tilde=np.asarray(ga.tau, float), v_tilde=np.asarray(ga.v, float),
               cav_tau=np.asarray(inf.cav.tau, float), cav_v=np.asarray(inf.cav.v, float), log_Z_hat=np.asarray(inf.log_Z_hat, float),
               dtheta=g, dZ=np.asarray(dZ, float), woodbury_vector=np.asarray(post.woodbury_vector, float),
               woodbury_inv=np.asarray(post.woodbury_inv, float), dL_dKmm=np.asarray(gd["dL_dKmm"], float))
    if Xs is not None:
        mu, var = post._raw_predict(k, Xs, pred_var=Z, full_cov=False)
        out.update(pred_mu=np.asarray(mu, float), pred_var=np.asarray(var, float),
                   pred_p=np.asarray(lik.predictive_values(mu, var)[0], float))
    return out


def two_class(N, D, seed, sharp):
    """labels from a smooth function of X in the centred unit cube; `sharp` scales it against the label noise"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-0.5, 0.5, (N, D))
    w = rng.uniform(1.0, 3.0, D)
    f = np.sin(2.0 * np.pi * X @ w / D) + 0.4 * X[:, 0]
    Y = (sharp * f + rng.standard_normal(N) > 0).astype(float)[:, None]
    return X, Y


def inputs(N, M, D, kern, seed, sharp=2.0):
    rng = np.random.default_rng(seed)
    allq = list(range(D))
    gdims = allq[:2]
    Z, g = grid_Z(M, D, gdims, rng)
    X, Y = two_class(N, D, seed + 50, sharp)

    def ls(ard):
        v = np.array([0.75 / g * rng.uniform(0.9, 1.1) if q in gdims else 4.0 * np.sqrt(D) for q in allq])
        return list(v if ard else v[:1])
    specs = {"rbf_iso": lambda: [("rbf", 0, [1.5] + ls(0), allq, 0)],
             "separated": lambda: [("rbf", 0, [40.0] + ls(0), allq, 0)],
             "matern52_ard": lambda: [("matern52", 1, [2.0] + ls(1), allq, 0)],
             "rbf+white": lambda: [("rbf", 0, [1.2] + ls(0), allq, 0), ("white", 0, [0.05], allq, 0)],
             "rbf*matern32": lambda: [("rbf", 0, [1.3] + ls(0), allq, 1), ("matern32", 0, [1.1] + ls(0), allq, 1)]}[kern]()
    Xs = rng.uniform(-0.5, 0.5, (13, D))
    return specs, X, Y, Z - 0.5, Xs


def spec_json(specs):
    return json.dumps([[s[0], int(s[1]), [float(v) for v in s[2]], [int(d) for d in s[3]], int(s[4])] for s in specs])


def case(ns, name, N, M, D, kern, seed, sharp=2.0, warm_from=None, **opts):
    specs, X, Y, Z, Xs = inputs(N, M, D, kern, seed, sharp)
    LADDER["entered"] = False
    inf = new_inf(ns, seed + 100, opts)
    extra = {}
    if warm_from is not None:
        # a warm start across a change of kernel parameters ("alternated"): EP at the first parameters, then forgotten as
        # on_optimization_start forgets it, then EP again at the fixture's parameters from the sites of the first run
        specs0 = [(s[0], s[1], [v * warm_from for v in s[2]], s[3], s[4]) for s in specs]
        evaluate(ns, inf, specs0, X, Y, Z)
        extra = dict(warm_specs=spec_json(specs0), warm_orders=np.array(inf.orders), warm_tau=np.array(inf.ga_approx_old.tau, float),
                     warm_v=np.array(inf.ga_approx_old.v, float))      # (copies: the second run updates these arrays in place)
        inf.orders = []
        inf.on_optimization_start()
    r = evaluate(ns, inf, specs, X, Y, Z, Xs)
    k, _ = assemble(ns, specs)
    kappa = float(np.linalg.cond(np.asarray(k.K(Z))))
    if LADDER["entered"]:
        raise RuntimeError("%s: the reference entered jitchol's ladder (cond(Kmm) %.1e): no fixture is written" % (name, kappa))
    if not inf.last_stop:
        raise RuntimeError("%s: the reference's EPDTC did not converge within 100 sweeps" % name)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, X=X, Y=Y, Z=Z, Xs=Xs, specs=spec_json(specs), orders=np.array(inf.orders), sweeps=len(inf.orders),
                        clamped=inf.clamped, parallel_updates=bool(opts.get("parallel_updates", False)),
                        eta=float(opts.get("eta", 1.0)), delta=float(opts.get("delta", 1.0)), epsilon=float(inf.epsilon),
                        cond_Kmm=kappa, **extra, **r)
    print("%-40s sweeps %3d  clamped %d  lml=% .12e  cond(Kmm) %.1e  max tau %.2e  %d bytes"
          % (name, len(inf.orders), inf.clamped, r["lml"], kappa, r["tau_tilde"].max(), os.path.getsize(path)))


def toy_1d(ns):
    from scipy.optimize import minimize
    rng = np.random.default_rng(12)
    N, M = 120, 10
    X = np.sort(rng.uniform(-0.5, 0.5, (N, 1)), 0)
    Y = (np.sin(2.0 * np.pi * X[:, 0]) * 2.5 + rng.standard_normal(N) > 0).astype(float)[:, None]
    Z0 = ((np.arange(M) + 0.5) / M)[:, None] - 0.5
    inf = new_inf(ns, 13, {})
    LADDER["entered"] = False

    def f(x):
        Z, var, ls = x[:M].reshape(M, 1), np.exp(x[M]), np.exp(x[M + 1])
        r = evaluate(ns, inf, [("rbf", 0, [var, ls], [0], 0)], X, Y, Z)
        return -r["lml"], -np.concatenate([r["dZ"].ravel(), r["dtheta"] * np.array([var, ls])])
    theta0 = np.array([1.0, 0.1])
    x0 = np.concatenate([Z0.ravel(), np.log(theta0)])
    l0 = -f(x0)[0]
    inf.on_optimization_start()
    res = minimize(f, x0, jac=True, method="L-BFGS-B", options={"maxiter": 100})
    l1 = -f(res.x)[0]
    if LADDER["entered"]:
        raise RuntimeError("toy_1d_optimize: the reference entered jitchol's ladder: no fixture is written")
    np.savez_compressed(os.path.join(OUT, "toy_1d_optimize.npz"), X=X, Y=Y, Z0=Z0, theta0=theta0, lml_start=l0, lml_end=l1,
                        theta_end=np.exp(res.x[M:]), Z_end=res.x[:M].reshape(M, 1))
    print("toy_1d_optimize: bound %.6f -> %.6f, theta %s" % (l0, l1, np.exp(res.x[M:])))


def main():
    ns = ref_loader.load_sum_kernels(ref_loader.load())
    ns.Bernoulli = importlib.import_module("GPy.likelihoods.bernoulli").Bernoulli
    # names the reference's EP module imports from packages that are stubs here
    lfi, liks = sys.modules["GPy.inference.latent_function_inference"], sys.modules["GPy.likelihoods"]
    lfi.ExactGaussianInference = ns.ExactGaussianInference
    lfi.VarDTC = importlib.import_module("GPy.inference.latent_function_inference.var_dtc").VarDTC
    liks.Gaussian = ns.Gaussian
    ns.ObsAr = importlib.import_module("paramz").ObsAr
    ns.RecordingEPDTC = recording_epdtc(
        importlib.import_module("GPy.inference.latent_function_inference.expectation_propagation").EPDTC)
    watch_jitchol()
    os.makedirs(OUT, exist_ok=True)
    case(ns, "rbf_iso_n150_m16_d2", 150, 16, 2, "rbf_iso", 1)
    case(ns, "matern52_ard_n140_m25_d3", 140, 25, 3, "matern52_ard", 2)
    case(ns, "rbf_white_n130_m16_d2", 130, 16, 2, "rbf+white", 3)
    case(ns, "rbf_x_matern32_n140_m20_d2", 140, 20, 2, "rbf*matern32", 4)
    case(ns, "parallel_rbf_iso_n150_m16_d2", 150, 16, 2, "rbf_iso", 1, parallel_updates=True)
    case(ns, "fractional_rbf_iso_n150_m16_d2", 150, 16, 2, "rbf_iso", 1, eta=0.9, delta=0.8)
    case(ns, "warm_rbf_iso_n150_m16_d2", 150, 16, 2, "rbf_iso", 5, warm_from=1.3)
    case(ns, "separated_rbf_n120_m12_d2", 120, 12, 2, "separated", 6, sharp=40.0)
    toy_1d(ns)


if __name__ == "__main__":
    main()
