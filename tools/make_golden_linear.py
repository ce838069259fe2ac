"""Fixtures tests/golden/linear/*.npz FROM THE REFERENCE'S OWN CODE: `Linear` (GPy/kern/src/linear.py), `RBF`, `Bias`,
`Coregionalize`, `Add` / `Prod`, `ExactGaussianInference`, `ExactStudentTInference`, `update_gradients_full`, `gradients_X`,
`Kdiag` and `PosteriorExact._raw_predict`, executed through oracle/ref_loader.py (imported, unchanged).  The fixtures live in
a subdirectory so that the parametrisations over tests/golden/*.npz do not pick them up.

specs entries are [kind, ard, theta (GPy link order), active_dims, term]; parts sharing a non-zero term id are the factors of
one `Prod` (the C-ABI's `mi355gp_part`).  A Linear entry's theta is its variances.  A Coregionalize entry is written as in
tools/make_golden_coreg.py: theta = [W (P x rank, row-major) | kappa (P)], ard = rank * 100 + P; dtheta is in GPy order (W,
then kappa).  The multi-output case uses one Gaussian noise for all outputs.

    python tools/make_golden_linear.py
"""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader  # noqa: E402
from oracle.gp_oracle import synthetic  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "linear")


def leaf(ns, spec):
    kind, ard, th, dims, _ = spec
    th = np.asarray(th, dtype=float)
    nd = len(dims)
    if kind == "linear":
        return ns.Linear(nd, variances=th, ARD=bool(ard), active_dims=dims)
    if kind == "rbf":
        return ns.RBF(nd, variance=th[0], lengthscale=th[1:], ARD=bool(ard), active_dims=dims)
    if kind == "bias":
        return ns.Bias(nd, variance=th[0], active_dims=dims)
    if kind == "coregionalize":
        P, rank = ard % 100, ard // 100
        return ns.Coregionalize(1, P, rank=rank, W=th[:P * rank].reshape(P, rank), kappa=th[P * rank:], active_dims=dims,
                                name="B")
    raise ValueError(kind)


def grads(k):
    names = {"Linear": ("variances",), "RBF": ("variance", "lengthscale"), "Bias": ("variance",),
             "Coregionalize": ("W", "kappa")}[type(k).__name__]
    return np.concatenate([np.atleast_1d(np.asarray(getattr(k, n).gradient, float)).ravel() for n in names])


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


def seeded_dL_dK(seed, N, M):
    """the dL_dK (N x N) and dL_dK against Xs (N x M) the gradients_X fixtures were made with"""
    rng = np.random.default_rng(1000 + seed)
    return rng.standard_normal((N, N)), rng.standard_normal((N, M))


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
    G, G2 = seeded_dL_dK(seed, X.shape[0], Xs.shape[0])
    gx = k.gradients_X(G, X)
    gx2 = k.gradients_X(G2, X, Xs)
    spec_json = json.dumps([[s[0], int(s[1]), [float(v) for v in s[2]], [int(d) for d in s[3]], int(s[4])] for s in specs])
    np.savez_compressed(os.path.join(OUT, name + ".npz"), X=X, Y=Y, noise=noise, nu=-1.0 if nu is None else nu,
                        specs=spec_json, lml=float(lml), alpha=np.asarray(post.woodbury_vector), dtheta=dtheta,
                        dnoise=dnoise, K_row0=np.asarray(k.K(X))[0], Kdiag_Xs=np.asarray(k.Kdiag(Xs)), Xs=Xs,
                        pred_mu=np.asarray(mu), pred_var=np.asarray(var), pred_cov=np.asarray(cov), gseed=seed,
                        gradX=np.asarray(gx), gradX2=np.asarray(gx2))
    print("%-36s lml=% .12e" % (name, lml))


def two_outputs(n_per, seed):
    """two correlated outputs with a linear trend over two inputs, stacked with the index column last"""
    rng = np.random.default_rng(seed)
    Xs, Ys = [], []
    for p, n in enumerate(n_per):
        x = rng.standard_normal((n, 2))
        f = (0.8 + 0.4 * p) * x[:, 0] - 0.5 * x[:, 1] + 0.2 * p
        Xs.append(np.hstack([x, np.full((n, 1), float(p))]))
        Ys.append((f + 0.1 * rng.standard_normal(n))[:, None])
    return np.ascontiguousarray(np.vstack(Xs)), np.ascontiguousarray(np.vstack(Ys))


def main():
    ns = ref_loader.load_sum_kernels(ref_loader.load())
    ns.Linear = importlib.import_module("GPy.kern.src.linear").Linear
    ns.Coregionalize = importlib.import_module("GPy.kern.src.coregionalize").Coregionalize
    importlib.import_module("GPy.inference.latent_function_inference.posterior")
    ns.studentt = importlib.import_module("GPy.inference.latent_function_inference.exact_studentt_inference")
    os.makedirs(OUT, exist_ok=True)
    X2, Y2 = synthetic(180, 2, seed=31)
    X3, Y3 = synthetic(160, 3, seed=32)
    sum3 = [("linear", 1, [0.5, 1.2, 0.8], [0, 1, 2], 0), ("rbf", 0, [1.1, 0.9], [0, 1, 2], 0),
            ("bias", 0, [0.6], [0, 1, 2], 0)]
    case(ns, "linear_iso_n180_d2", X2, Y2, [("linear", 0, [0.8], [0, 1], 0)])
    case(ns, "linear_ard_active_n160_d3", X3, Y3, [("linear", 1, [0.7, 1.6], [0, 2], 0)], seed=1)
    case(ns, "linard_rbf_bias_n160_d3", X3, Y3, sum3, seed=2)
    case(ns, "lin0_x_rbf12_n160_d3", X3, Y3, [("linear", 0, [0.9], [0], 1), ("rbf", 1, [1.2, 0.8, 1.4], [1, 2], 1)], seed=3)
    case(ns, "lin0_x_lin12_n160_d3", X3, Y3, [("linear", 0, [0.7], [0], 1), ("linear", 1, [1.1, 0.6], [1, 2], 1)], seed=4)
    case(ns, "linard_rbf_bias_shift50_n160_d3", X3 + 50.0, Y3, sum3, seed=5)
    # (no noise term in the Student-t process: short lengthscales keep Ky = K + 1e-8 I at a condition number of ~3e3)
    case(ns, "studentt_lin_rbf_n160_d3", X3, Y3,
         [("linear", 0, [0.6], [0, 1, 2], 0), ("rbf", 1, [1.0, 0.3, 0.25, 0.35], [0, 1, 2], 0)], nu=4.0, seed=6)
    Xm, Ym = two_outputs([80, 70], seed=33)
    case(ns, "icm_linard_p2_n150", Xm, Ym,
         [("linear", 1, [0.8, 1.3], [0, 1], 1), ("coregionalize", 102, [0.9, -0.4, 0.3, 0.5], [2], 1)], seed=7)


if __name__ == "__main__":
    main()
