"""Fixtures tests/golden/mlp/*.npz FROM THE REFERENCE'S OWN CODE: `MLP` (GPy/kern/src/mlp.py), `Poly` (GPy/kern/src/poly.py),
`Linear`, `RBF`, `Bias`, `Coregionalize`, `Add` / `Prod`, `ExactGaussianInference`, `ExactStudentTInference`,
`update_gradients_full`, `gradients_X`, `Kdiag` and `PosteriorExact._raw_predict`, executed through oracle/ref_loader.py
(imported, unchanged).  The fixtures live in a subdirectory so that the parametrisations over tests/golden/*.npz do not pick
them up.  Only data goes into them.

specs entries are [kind, ard, theta (GPy link order), active_dims, term] as in tools/make_golden_linear.py.  An MLP entry's
theta is [variance, weight_variance (1, or one per active dimension with ard = 1), bias_variance]; a Poly entry's is [variance,
scale, bias, order] -- the order is no parameter, so `dtheta` holds three numbers for it.  `gradX` / `gradX2` are absent for
cases with a Poly leaf (the reference raises NotImplementedError).  The lone-MLP cases also carry the reference's
`update_gradients_diag` (`diag_dtheta`) and `gradients_X_diag` (`gradXdiag`) for the seeded dL_dKdiag of `seeded_dL_dKdiag`.

    python tools/make_golden_mlp.py
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
from oracle.gp_oracle import synthetic  # noqa: E402
import make_golden_linear as base  # noqa: E402  (leaf of the older kinds, the seeded dL_dK, the two-output data)

OUT = os.path.join(ROOT, "tests", "golden", "mlp")
NAMES = {"MLP": ("variance", "weight_variance", "bias_variance"), "Poly": ("variance", "scale", "bias"),
         "Linear": ("variances",), "RBF": ("variance", "lengthscale"), "Bias": ("variance",), "Coregionalize": ("W", "kappa")}


def leaf(ns, spec):
    kind, ard, th, dims, _ = spec
    th = np.asarray(th, dtype=float)
    nd = len(dims)
    if kind == "mlp":
        return ns.MLP(nd, variance=th[0], weight_variance=th[1:-1] if ard else th[1], bias_variance=th[-1], ARD=bool(ard),
                      active_dims=dims)
    if kind == "poly":
        return ns.Poly(nd, variance=th[0], scale=th[1], bias=th[2], order=th[3], active_dims=dims)
    return base.leaf(ns, spec)


def grads(k):
    return np.concatenate([np.atleast_1d(np.asarray(getattr(k, n).gradient, float)).ravel() for n in NAMES[type(k).__name__]])


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
    out = walk(top)
    for k in out:
        if type(k).__name__ == "Coregionalize":
            k.parameters_changed()                 # B = W W^T + diag(kappa) on the copies that evaluate
    return top, out


def seeded_dL_dKdiag(seed, N):
    """the dL_dKdiag (N) the diagonal-gradient fixtures of the lone-MLP cases were made with"""
    return np.random.default_rng(2000 + seed).standard_normal(N)


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
    for s in specs:                                # new points of a multi-output model carry an output index
        if s[0] == "coregionalize":
            Xs[:, s[3][0]] = rng.integers(0, s[1] % 100, 13)
    mu, var = post._raw_predict(k, Xs, pred_var=X, full_cov=False)
    _, cov = post._raw_predict(k, Xs, pred_var=X, full_cov=True)
    extra = {}
    if not any(s[0] == "poly" for s in specs):
        G, G2 = base.seeded_dL_dK(seed, X.shape[0], Xs.shape[0])
        extra["gradX"] = np.asarray(k.gradients_X(G, X))
        extra["gradX2"] = np.asarray(k.gradients_X(G2, X, Xs))
    if len(specs) == 1 and specs[0][0] == "mlp":
        gdiag = seeded_dL_dKdiag(seed, X.shape[0])
        k.update_gradients_diag(gdiag, X)
        extra["diag_dtheta"] = grads(k)
        extra["gradXdiag"] = np.asarray(k.gradients_X_diag(gdiag, X))
    K = np.asarray(k.K(X))
    spec_json = json.dumps([[s[0], int(s[1]), [float(v) for v in s[2]], [int(d) for d in s[3]], int(s[4])] for s in specs])
    np.savez_compressed(os.path.join(OUT, name + ".npz"), X=X, Y=Y, noise=noise, nu=-1.0 if nu is None else nu,
                        specs=spec_json, lml=float(lml), alpha=np.asarray(post.woodbury_vector), dtheta=dtheta,
                        dnoise=dnoise, K_row0=K[0], Kdiag_Xs=np.asarray(k.Kdiag(Xs)), Xs=Xs,
                        pred_mu=np.asarray(mu), pred_var=np.asarray(var), pred_cov=np.asarray(cov), gseed=seed, **extra)
    Ky = K + (noise if nu is None else 0.0) * np.eye(X.shape[0]) + 1e-8 * np.eye(X.shape[0])
    print("%-28s lml=% .12e  cond(Ky)=%.1e  %d bytes" % (name, lml, np.linalg.cond(Ky),
                                                         os.path.getsize(os.path.join(OUT, name + ".npz"))))


def main():
    ns = ref_loader.load_sum_kernels(ref_loader.load())
    ns.Linear = importlib.import_module("GPy.kern.src.linear").Linear
    ns.MLP = importlib.import_module("GPy.kern.src.mlp").MLP
    ns.Poly = importlib.import_module("GPy.kern.src.poly").Poly
    ns.Coregionalize = importlib.import_module("GPy.kern.src.coregionalize").Coregionalize
    importlib.import_module("GPy.inference.latent_function_inference.posterior")
    ns.studentt = importlib.import_module("GPy.inference.latent_function_inference.exact_studentt_inference")
    os.makedirs(OUT, exist_ok=True)
    X2, Y2 = synthetic(180, 2, seed=41)
    X3, Y3 = synthetic(160, 3, seed=42)
    X40, Y40 = synthetic(200, 40, seed=43)
    d3 = [0, 1, 2]
    ard3 = ("mlp", 1, [1.3, 0.7, 1.5, 0.3, 0.4], d3, 0)
    case(ns, "mlp_iso_n180_d2", X2, Y2, [("mlp", 0, [1.2, 0.8, 0.5], [0, 1], 0)])
    case(ns, "mlp_ard_active_n160_d3", X3, Y3, [("mlp", 1, [1.1, 0.7, 1.6, 0.6], [0, 2], 0)], seed=1)
    case(ns, "mlp_ard_n200_d40", X40, Y40,
         [("mlp", 1, [1.4] + list(np.linspace(0.02, 0.08, 40)) + [0.3], list(range(40)), 0)], seed=2)
    case(ns, "mlpard_rbf_bias_n160_d3", X3, Y3, [ard3, ("rbf", 0, [1.1, 0.9], d3, 0), ("bias", 0, [0.6], d3, 0)], seed=3)
    case(ns, "mlp0_x_rbf12_n160_d3", X3, Y3, [("mlp", 0, [1.5, 0.9, 0.7], [0], 1), ("rbf", 1, [1.2, 0.8, 1.4], [1, 2], 1)], seed=4)
    case(ns, "lin0_x_mlp12_n160_d3", X3, Y3, [("linear", 0, [0.7], [0], 1), ("mlp", 1, [1.6, 1.1, 0.6, 0.5], [1, 2], 1)], seed=5)
    case(ns, "mlp_ard_x20_n160_d3", 20.0 * X3, Y3, [ard3], seed=6)
    # (no noise term in the Student-t process: short lengthscales keep Ky = K + 1e-8 I well conditioned)
    case(ns, "studentt_mlp_rbf_n160_d3", X3, Y3,
         [("mlp", 0, [0.8, 0.9, 0.5], d3, 0), ("rbf", 1, [1.0, 0.3, 0.25, 0.35], d3, 0)], nu=4.0, seed=7)
    Xm, Ym = base.two_outputs([80, 70], seed=44)
    case(ns, "icm_mlpard_p2_n150", Xm, Ym,
         [("mlp", 1, [1.2, 0.8, 1.3, 0.4], [0, 1], 1), ("coregionalize", 102, [0.9, -0.4, 0.3, 0.5], [2], 1)], seed=8)
    case(ns, "poly_o3_n160_d3", X3, Y3, [("poly", 0, [0.6, 0.25, 1.1, 3.0], d3, 0)], seed=9)
    case(ns, "poly_o2_rbf_bias_n160_d3", X3, Y3,
         [("poly", 0, [0.5, 0.4, 0.8, 2.0], d3, 0), ("rbf", 0, [1.1, 0.9], d3, 0), ("bias", 0, [0.6], d3, 0)], seed=10)
    case(ns, "poly0_x_rbf12_n160_d3", X3, Y3,
         [("poly", 0, [0.7, 0.5, 0.9, 2.0], [0], 1), ("rbf", 1, [1.2, 0.8, 1.4], [1, 2], 1)], seed=11)


if __name__ == "__main__":
    main()
