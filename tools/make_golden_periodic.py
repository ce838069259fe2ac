"""Fixtures tests/golden/periodic/*.npz FROM THE REFERENCE'S OWN CODE: `RatQuad` (GPy/kern/src/stationary.py),
`StdPeriodic` (GPy/kern/src/standard_periodic.py), `Add` / `Prod`, `ExactGaussianInference`, `ExactStudentTInference`,
`update_gradients_full`, `gradients_X` and `PosteriorExact._raw_predict`, executed through oracle/ref_loader.py (imported,
unchanged).  The fixtures live in a subdirectory so that the parametrisations over tests/golden/*.npz do not pick them up.

specs entries are [kind, ard, theta (GPy link order), active_dims, term]; parts sharing a non-zero term id are the
factors of one `Prod` (the C-ABI's `mi355gp_part`).  StdPeriodic's ard is the bitmask ARD1 | ARD2 << 1.

    python tools/make_golden_periodic.py
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

OUT = os.path.join(ROOT, "tests", "golden", "periodic")


def leaf(ns, spec):
    kind, ard, th, dims, _ = spec
    th = np.asarray(th, dtype=float)
    nd = len(dims)
    if kind == "ratquad":
        nl = nd if ard else 1
        return ns.RatQuad(nd, variance=th[0], lengthscale=th[1:1 + nl], power=th[1 + nl], ARD=bool(ard), active_dims=dims)
    if kind == "stdperiodic":
        npr = nd if ard & 1 else 1
        return ns.StdPeriodic(nd, variance=th[0], period=th[1:1 + npr], lengthscale=th[1 + npr:], ARD1=bool(ard & 1),
                              ARD2=bool(ard & 2), active_dims=dims)
    if kind == "rbf":
        return ns.RBF(nd, variance=th[0], lengthscale=th[1:], ARD=bool(ard), active_dims=dims)
    if kind == "white":
        return ns.White(nd, variance=th[0], active_dims=dims)
    raise ValueError(kind)


def grads(k):
    names = {"RatQuad": ("variance", "lengthscale", "power"), "StdPeriodic": ("variance", "period", "lengthscale"),
             "RBF": ("variance", "lengthscale"), "White": ("variance",)}[type(k).__name__]
    return np.concatenate([np.atleast_1d(np.asarray(getattr(k, n).gradient, float)) for n in names])


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
    mu, var = post._raw_predict(k, Xs, pred_var=X, full_cov=False)
    _, cov = post._raw_predict(k, Xs, pred_var=X, full_cov=True)
    G, G2 = seeded_dL_dK(seed, X.shape[0], Xs.shape[0])
    gx = k.gradients_X(G, X)
    gx2 = k.gradients_X(G2, X, Xs)
    spec_json = json.dumps([[s[0], int(s[1]), [float(v) for v in s[2]], [int(d) for d in s[3]], int(s[4])] for s in specs])
    np.savez_compressed(os.path.join(OUT, name + ".npz"), X=X, Y=Y, noise=noise, nu=-1.0 if nu is None else nu,
                        specs=spec_json, lml=float(lml), alpha=np.asarray(post.woodbury_vector), dtheta=dtheta,
                        dnoise=dnoise, K_row0=np.asarray(k.K(X))[0], Xs=Xs, pred_mu=np.asarray(mu),
                        pred_var=np.asarray(var), pred_cov=np.asarray(cov), gseed=seed, gradX=np.asarray(gx),
                        gradX2=np.asarray(gx2))
    print("%-36s lml=% .12e" % (name, lml))


def mauna_loa_like(N, seed):
    """calendar-year inputs (1958 .. 2020): trend + annual cycle + noise, standardised"""
    rng = np.random.default_rng(seed)
    x = np.sort(1958.0 + 62.0 * rng.random(N))
    y = 0.02 * (x - 1958.0) ** 1.4 + 0.6 * np.sin(2 * np.pi * x) + 0.1 * rng.standard_normal(N)
    y = (y - y.mean()) / y.std()
    return np.ascontiguousarray(x[:, None]), np.ascontiguousarray(y[:, None])


def main():
    ns = ref_loader.load_sum_kernels(ref_loader.load())
    ns.RatQuad = ns.stationary.RatQuad
    ns.StdPeriodic = importlib.import_module("GPy.kern.src.standard_periodic").StdPeriodic
    importlib.import_module("GPy.inference.latent_function_inference.posterior")
    ns.studentt = importlib.import_module("GPy.inference.latent_function_inference.exact_studentt_inference")
    os.makedirs(OUT, exist_ok=True)
    X2, Y2 = synthetic(180, 2, seed=11)
    X3, Y3 = synthetic(160, 3, seed=12)
    case(ns, "ratquad_iso_n180_d2", X2, Y2, [("ratquad", 0, [1.3, 0.8, 1.7], [0, 1], 0)])
    case(ns, "ratquad_ard_active_n160_d3", X3, Y3, [("ratquad", 1, [0.9, 0.7, 1.4, 2.5], [0, 2], 0)], seed=1)
    case(ns, "stdper_iso_n160_d3", X3, Y3, [("stdperiodic", 0, [1.1, 1.3, 0.9], [0, 1, 2], 0)], seed=2)
    case(ns, "stdper_ard1_n160_d3", X3, Y3, [("stdperiodic", 1, [1.1, 1.3, 2.1, 0.8, 0.9], [0, 1, 2], 0)], seed=3)
    case(ns, "stdper_ard2_n160_d3", X3, Y3, [("stdperiodic", 2, [0.9, 1.6, 0.7, 1.2, 1.9], [0, 1, 2], 0)], seed=4)
    case(ns, "stdper_ard12_n160_d3", X3, Y3, [("stdperiodic", 3, [1.2, 1.3, 2.1, 0.8, 0.7, 1.2, 1.9], [0, 1, 2], 0)],
         seed=5)
    case(ns, "rbf0_x_stdper1_n180_d2", X2, Y2, [("rbf", 0, [1.2, 1.5], [0], 1), ("stdperiodic", 0, [0.8, 0.7, 1.1], [1], 1)],
         seed=6)
    Xm, Ym = mauna_loa_like(300, seed=13)
    case(ns, "maunaloa_years_n300_d1", Xm, Ym,
         [("rbf", 0, [1.0, 30.0], [0], 0), ("rbf", 0, [0.3, 60.0], [0], 1), ("stdperiodic", 0, [1.0, 1.0, 1.2], [0], 1),
          ("ratquad", 0, [0.2, 1.5, 0.8], [0], 0), ("white", 0, [0.02], [0], 0)], noise=0.01, seed=7)
    case(ns, "studentt_stdper_plus_rq_n160_d3", X3, Y3,
         [("stdperiodic", 0, [1.1, 1.3, 0.9], [0, 1, 2], 0), ("ratquad", 1, [0.5, 1.1, 0.9, 1.6, 1.2], [0, 1, 2], 0)],
         nu=4.0, seed=8)


if __name__ == "__main__":
    main()
