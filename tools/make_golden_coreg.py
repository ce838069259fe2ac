"""Fixtures tests/golden/coreg/*.npz FROM THE REFERENCE'S OWN CODE: `Coregionalize` (GPy/kern/src/coregionalize.py), `RBF` /
`Matern52`, `Add` / `Prod`, `MixedNoise` (GPy/likelihoods/mixed_noise.py), `ExactGaussianInference`, `ExactStudentTInference`,
`update_gradients_full` and `PosteriorExact._raw_predict`, executed through oracle/ref_loader.py (imported, unchanged).  The
fixtures live in a subdirectory so that the parametrisations over tests/golden/*.npz do not pick them up.

The loader's stub `Parameterized` does not call `parameters_changed` at construction and `Prod` copies its parts, so B is
formed by calling `parameters_changed()` on the linked copies, and the gradients are read from them.

specs entries are [kind, ard, theta, active_dims, term] as the C-ABI's part list, except that a Coregionalize entry carries
[W (P x rank, row-major) | kappa (P)] as theta and ard = rank * 100 + P (the tests form B = W W^T + diag(kappa)).
dtheta is in GPy order: every leaf's parameters in link order (Coregionalize: W, then kappa).

    python tools/make_golden_coreg.py
"""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "coreg")


def leaf(ns, spec):
    kind, ard, th, dims, _ = spec
    th = np.asarray(th, dtype=float)
    nd = len(dims)
    if kind == "coregionalize":
        P, rank = ard % 100, ard // 100
        return ns.Coregionalize(1, P, rank=rank, W=th[:P * rank].reshape(P, rank), kappa=th[P * rank:], active_dims=dims,
                                name="B")
    if kind == "white":
        return ns.White(nd, variance=th[0], active_dims=dims)
    cls = {"rbf": ns.RBF, "matern52": ns.Matern52}[kind]
    return cls(nd, variance=th[0], lengthscale=th[1:], ARD=bool(ard), active_dims=dims)


def grads(k):
    names = {"Coregionalize": ("W", "kappa"), "White": ("variance",)}.get(type(k).__name__, ("variance", "lengthscale"))
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


def data(P, n_per, D, seed, shuffle=False):
    """per-output inputs / outputs of correlated functions, stacked with the index column as build_XY does"""
    rng = np.random.default_rng(seed)
    Xs, Ys = [], []
    for p in range(P):
        x = rng.random((n_per[p], D)) * 4.0
        f = np.sin(x @ np.linspace(1.0, 0.4, D)) * (1.0 + 0.3 * p) + 0.2 * p * np.cos(2 * x[:, 0])
        Xs.append(x)
        Ys.append((f + 0.05 * rng.standard_normal(n_per[p]))[:, None])
    I = np.hstack([np.repeat(j, n) for j, n in enumerate(n_per)])
    X = np.hstack([np.vstack(Xs), I[:, None].astype(float)])
    Y = np.vstack(Ys)
    if shuffle:
        perm = rng.permutation(X.shape[0])
        X, Y = X[perm], Y[perm]
    return np.ascontiguousarray(X), np.ascontiguousarray(Y)


def seeded_dL_dK(seed, N, M):
    """the asymmetric dL_dK (N x N) and dL_dK against Xs (N x M) of the lone-Coregionalize gradient fixtures"""
    rng = np.random.default_rng(1000 + seed)
    return rng.standard_normal((N, N)), rng.standard_normal((N, M))


def case(ns, name, X, Y, specs, noises, nu=None, seed=0):
    k, leaves = assemble(ns, specs)
    rng = np.random.default_rng(seed + 7)
    P_all = [s[1] % 100 for s in specs if s[0] == "coregionalize"]
    P = P_all[0]
    meta = {"output_index": X[:, -1:].astype(int)}
    if nu is None:
        lik = ns.MixedNoise([ns.Gaussian(variance=v, name="Gaussian_noise_%d" % j) for j, v in enumerate(noises)])
        post, lml, gd = ns.ExactGaussianInference().inference(k, X, lik, Y, Y_metadata=meta)
        dnoise = np.asarray(gd["dL_dthetaL"], float).ravel()
    else:
        post, lml, gd = ns.studentt.ExactStudentTInference().inference(k, X, Y, nu)
        dnoise = np.array([float(gd["dL_dnu"])])
    k.update_gradients_full(gd["dL_dK"], X)
    dtheta = np.concatenate([grads(p) for p in leaves])
    D = X.shape[1] - 1
    lo, hi = X[:, :D].min(0), X[:, :D].max(0)
    Xs = np.hstack([lo + (hi - lo) * rng.random((13, D)), rng.integers(0, P, (13, 1)).astype(float)])
    mu, var = post._raw_predict(k, Xs, pred_var=X, full_cov=False)
    _, cov = post._raw_predict(k, Xs, pred_var=X, full_cov=True)
    # update_gradients_full of the lone Coregionalize (the first one) against seeded asymmetric dL_dK, against X and X2
    cg = [p for p in leaves if type(p).__name__ == "Coregionalize"][0]
    G, G2 = seeded_dL_dK(seed, X.shape[0], Xs.shape[0])
    cg.update_gradients_full(G, X)
    ug = grads(cg)
    cg.update_gradients_full(G2, X, Xs)
    ug2 = grads(cg)
    spec_json = json.dumps([[s[0], int(s[1]), [float(v) for v in s[2]], [int(d) for d in s[3]], int(s[4])] for s in specs])
    np.savez_compressed(os.path.join(OUT, name + ".npz"), X=X, Y=Y, noises=np.asarray(noises, float),
                        nu=-1.0 if nu is None else nu, specs=spec_json, lml=float(lml), alpha=np.asarray(post.woodbury_vector),
                        dtheta=dtheta, dnoise=dnoise, K_row0=np.asarray(k.K(X))[0], Xs=Xs, pred_mu=np.asarray(mu),
                        pred_var=np.asarray(var), pred_cov=np.asarray(cov), gseed=seed, ug=ug, ug2=ug2)
    print("%-30s N=%4d lml=% .12e" % (name, X.shape[0], lml))


def main():
    ns = ref_loader.load_sum_kernels(ref_loader.load())
    ns.Coregionalize = importlib.import_module("GPy.kern.src.coregionalize").Coregionalize
    ns.MixedNoise = importlib.import_module("GPy.likelihoods.mixed_noise").MixedNoise
    importlib.import_module("GPy.inference.latent_function_inference.posterior")
    ns.studentt = importlib.import_module("GPy.inference.latent_function_inference.exact_studentt_inference")
    os.makedirs(OUT, exist_ok=True)
    W3 = [0.9, -0.4, 0.7]
    X, Y = data(3, [50, 40, 45], 2, seed=21)
    case(ns, "icm_rbfard_p3_r1_n135", X, Y,
         [("rbf", 1, [1.1, 1.3, 0.8], [0, 1], 1), ("coregionalize", 103, W3 + [0.3, 0.5, 0.2], [2], 1)],
         [0.1, 0.1, 0.1], seed=1)
    case(ns, "icm_rbfard_p3_noises_n135", X, Y,
         [("rbf", 1, [1.1, 1.3, 0.8], [0, 1], 1), ("coregionalize", 103, W3 + [0.3, 0.5, 0.2], [2], 1)],
         [0.05, 0.2, 0.01], seed=2)
    X, Y = data(2, [60, 50], 2, seed=22)
    case(ns, "lcm_m52_rbf_p2_r2_n110", X, Y,
         [("matern52", 1, [0.9, 1.4, 0.7], [0, 1], 1), ("coregionalize", 202, [0.8, 0.3, -0.5, 0.6, 0.4, 0.3], [2], 1),
          ("rbf", 0, [0.6, 0.9], [0, 1], 2), ("coregionalize", 202, [0.2, -0.7, 0.5, 0.1, 0.2, 0.6], [2], 2)],
         [0.08, 0.12], seed=3)
    X, Y = data(5, [30, 25, 40, 35, 30], 1, seed=23, shuffle=True)
    case(ns, "icm_rbf_p5_shuffled_n160", X, Y,
         [("rbf", 0, [1.0, 0.8], [0], 1), ("coregionalize", 105, [0.9, -0.3, 0.6, 0.2, -0.8, 0.4, 0.3, 0.5, 0.2, 0.6], [1], 1)],
         [0.1, 0.05, 0.15, 0.1, 0.08], seed=4)
    X, Y = data(1, [80], 2, seed=24)
    case(ns, "icm_m52_p1_n80", X, Y,
         [("matern52", 0, [1.2, 0.9], [0, 1], 1), ("coregionalize", 101, [0.7, 0.4], [2], 1)], [0.1], seed=5)
    X, Y = data(3, [40, 45, 35], 2, seed=25)
    case(ns, "studentt_icm_m52_p3_n120", X, Y,
         [("matern52", 1, [1.0, 1.1, 0.9], [0, 1], 1), ("coregionalize", 103, [0.6, -0.5, 0.8, 0.4, 0.3, 0.6], [2], 1),
          ("white", 0, [0.05], [0, 1], 0)], [0.0, 0.0, 0.0], nu=5.0, seed=6)


if __name__ == "__main__":
    main()
