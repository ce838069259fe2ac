"""Fixtures tests/golden/svgp/*.npz FROM THE REFERENCE'S OWN CODE: `SVGP.inference`
(GPy/inference/latent_function_inference/svgp.py), the likelihoods' `variational_expectations`, the kernels'
`update_gradients_full` / `update_gradients_diag` / `gradients_X` assembled as GPy/core/svgp.py:58-65 does, and
`Posterior._raw_predict`, executed through oracle/ref_loader.py (imported, unchanged; `choleskies` falls back to its pure-Python
form).  Only data goes into the fixtures.

Inputs: SVGP adds no 1e-8 to Kmm (svgp.py:37), so Z lies on a jittered regular grid over the first (at most two) active
dimensions with lengthscales of 0.75 grid spacings there, as tests/sparse_ld.make_case does; with Z drawn at random cond(Kmm) is
about 5e7 and the bound about -5e7, which is no fixture.  L_d = I + 0.1 tril(randn) / sqrt(M) keeps cond(S_d) below 2.

`toy_classification.npz`: a 1-D two-class problem; the reference's bound before and after 60 L-BFGS-B iterations over (Z, log
kernel parameters, q_u_chol, q_u_mean) from the default start, and the training accuracy it reaches.

    python tools/make_golden_svgp.py
"""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "svgp")
NAMES = {"RBF": ("variance", "lengthscale"), "Matern52": ("variance", "lengthscale"), "Matern32": ("variance", "lengthscale"),
         "Exponential": ("variance", "lengthscale"), "White": ("variance",), "Bias": ("variance",)}


def leaf(ns, spec):
    kind, ard, th, dims, _ = spec
    th, nd = np.asarray(th, dtype=float), len(dims)
    if kind in ("white", "bias"):
        return {"white": ns.White, "bias": ns.Bias}[kind](nd, variance=th[0], active_dims=dims)
    cls = {"rbf": ns.RBF, "matern52": ns.Matern52, "matern32": ns.Matern32, "exponential": ns.Exponential}[kind]
    return cls(nd, variance=th[0], lengthscale=th[1:] if ard else th[1], ARD=bool(ard), active_dims=dims)


def assemble(ns, specs):
    groups, seen = [], {}
    for s in specs:
        k, t = leaf(ns, s), s[4]
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


def grads(leaves):
    return np.concatenate([np.atleast_1d(np.asarray(getattr(k, n).gradient, float)).ravel() for k in leaves
                           for n in NAMES[type(k).__name__]])


def make_lik(ns, name, theta):
    if name == "gaussian":
        return ns.Gaussian(variance=theta[0])
    if name == "bernoulli":
        return ns.Bernoulli()
    if name == "studentt":
        lik = ns.StudentT(deg_free=theta[1], sigma2=theta[0])
        lik.deg_free = lik.v                       # (the parameter stub does not resolve a linked parameter by its name)
        return lik
    return ns.Poisson()


def grid_Z(M, D, gdims, rng):
    """M of the g^nd cell centres of a regular grid over `gdims` of the unit cube, jittered by +-0.2 / g; uniform elsewhere"""
    g = 1
    while g ** len(gdims) < M:
        g += 1
    Z = rng.uniform(0.0, 1.0, (M, D))
    sites = rng.permutation(g ** len(gdims))[:M]
    for a, q in enumerate(gdims):
        Z[:, q] = ((sites // g ** a) % g + 0.5 + rng.uniform(-0.2, 0.2, M)) / g
    return Z, g


def evaluate(ns, specs, lik, X, Y, Z, q_mean, q_chol, batch_scale, Xs=None):
    """one SVGP.inference + the gradient assembly of core/svgp.py:58-65 (+ predictions at Xs)"""
    k, leaves = assemble(ns, specs)
    rec = {}
    ve = lik.variational_expectations

    def recording(Y_, m, v, **kw):
        r = ve(Y_, m, v, **kw)
        rec.update(mu=np.array(m), v=np.array(v), F=np.array(r[0]), dF_dmu=np.array(r[1]), dF_dv=np.array(r[2]),
                   dF_dtheta=np.zeros((0,) + np.shape(m)) if r[3] is None else np.array(r[3], dtype=float))
        return r
    lik.variational_expectations = recording
    post, bound, gd = ns.SVGP().inference(q_mean, q_chol, k, X, Z, lik, Y, batch_scale=batch_scale)
    k.update_gradients_full(gd["dL_dKmm"], Z)
    g = grads(leaves)
    k.update_gradients_full(gd["dL_dKmn"], Z, X)
    g = g + grads(leaves)
    k.update_gradients_diag(gd["dL_dKdiag"], X)
    g = g + grads(leaves)
    dZ = k.gradients_X(gd["dL_dKmm"], Z) + k.gradients_X(gd["dL_dKmn"], Z, X)
    out = dict(bound=float(bound), dtheta=g, dZ=np.asarray(dZ, float), dL_dm=np.asarray(gd["dL_dm"], float),
               dL_dchol=np.asarray(gd["dL_dchol"], float), dL_dKmm=np.asarray(gd["dL_dKmm"], float),
               dL_dKmn=np.asarray(gd["dL_dKmn"], float), dL_dKdiag=np.asarray(gd["dL_dKdiag"], float),
               dL_dthetaL=np.zeros(0) if gd["dL_dthetaL"] is None else np.atleast_1d(np.asarray(gd["dL_dthetaL"], float)), **rec)
    if Xs is not None:
        mu, var = post._raw_predict(k, Xs, pred_var=Z, full_cov=False)
        _, cov = post._raw_predict(k, Xs, pred_var=Z, full_cov=True)
        out.update(pred_mu=np.asarray(mu, float), pred_var=np.asarray(var, float), pred_cov=np.asarray(cov, float),
                   woodbury_vector=np.asarray(post.woodbury_vector, float), woodbury_inv=np.asarray(post.woodbury_inv, float))
    return out


def targets(lik_name, X, L, rng):
    w = rng.uniform(1.0, 3.0, (min(X.shape[1], 3), L))
    f = np.sin(2.0 * np.pi * X[:, :w.shape[0]] @ w / w.shape[0])
    if lik_name == "bernoulli":
        return (rng.random(f.shape) < 0.5 * (1.0 + np.tanh(2.0 * f))).astype(float)
    if lik_name == "poisson":
        return rng.poisson(np.exp(0.5 + 0.8 * f)).astype(float)
    Y = f + 0.2 * rng.standard_normal(f.shape)
    if lik_name == "studentt":
        idx = rng.choice(X.shape[0], X.shape[0] // 10, replace=False)
        Y[idx] += 4.0 * np.where(rng.random((idx.size, L)) < 0.5, -1.0, 1.0)
    return Y


def case(ns, name, lik_name, lik_theta, N, M, D, L, kern, batch_scale, seed):
    rng = np.random.default_rng(seed)
    allq = list(range(D))
    gdims = [0, 2] if kern == "prod_subset" else allq[:2]
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
    elif kern == "matern32_iso":
        specs = [("matern32", 0, [1.1] + ls(allq, 0), allq, 0)]
    elif kern == "rbf+white":
        specs = [("rbf", 0, [1.2] + ls(allq, 0), allq, 0), ("white", 0, [0.05], allq, 0)]
    else:                                          # rbf[0] x matern32[2] + bias on a 4-column X: column 1 and 3 are seen by no part
        assert kern == "prod_subset" and D == 4
        specs = [("rbf", 0, [1.3] + ls([0], 0), [0], 1), ("matern32", 0, [0.8] + ls([2], 0), [2], 1), ("bias", 0, [0.2], allq, 0)]
    Y = targets(lik_name, X, L, rng)
    q_mean = 0.5 * rng.standard_normal((M, L))
    Ls = np.stack([np.eye(M) + 0.1 * np.tril(rng.standard_normal((M, M))) / np.sqrt(M) for _ in range(L)])
    q_chol = ns.choleskies.triang_to_flat(Ls)
    Xs = rng.uniform(0.0, 1.0, (17, D))
    r = evaluate(ns, specs, make_lik(ns, lik_name, lik_theta), X, Y, Z, q_mean, q_chol, batch_scale, Xs)
    k, _ = assemble(ns, specs)
    kappa = float(np.linalg.cond(np.asarray(k.K(Z))))
    spec_json = json.dumps([[s[0], int(s[1]), [float(v) for v in s[2]], [int(d) for d in s[3]], int(s[4])] for s in specs])
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, X=X, Y=Y, Z=Z, Xs=Xs, q_mean=q_mean, q_chol=q_chol, specs=spec_json, lik=lik_name,
                        lik_theta=np.asarray(lik_theta, float), batch_scale=float(batch_scale), cond_Kmm=kappa, **r)
    print("%-34s bound % .10e  cond(Kmm) %.1e  %d bytes" % (name, r["bound"], kappa, os.path.getsize(path)))


def toy_classification(ns):
    from scipy.optimize import minimize
    rng = np.random.default_rng(5)
    N, M = 200, 8
    X = np.sort(rng.uniform(0.0, 1.0, (N, 1)), 0)
    p = 0.5 * (1.0 + np.tanh(3.0 * np.sin(2.0 * np.pi * X[:, 0])))
    Y = (rng.random(N) < p).astype(float)[:, None]
    Z0 = ((np.arange(M) + 0.5) / M)[:, None]
    nt = M * (M + 1) // 2
    chol0 = ns.choleskies.triang_to_flat(np.eye(M)[None])
    lik = ns.Bernoulli()

    # flat order of the package's model: Z, kern.variance, kern.lengthscale, q_u_chol, q_u_mean; kernel parameters in log space
    def unpack(x):
        return x[:M].reshape(M, 1), np.exp(x[M]), np.exp(x[M + 1]), x[M + 2:M + 2 + nt].reshape(nt, 1), x[M + 2 + nt:].reshape(M, 1)

    def f(x):
        Z, var, ls, chol, m = unpack(x)
        r = evaluate(ns, [("rbf", 0, [var, ls], [0], 0)], lik, X, Y, Z, m, chol, 1.0)
        g = np.concatenate([r["dZ"].ravel(), r["dtheta"] * np.array([var, ls]), r["dL_dchol"].ravel(), r["dL_dm"].ravel()])
        return -r["bound"], -g
    x0 = np.concatenate([Z0.ravel(), np.log([1.0, 0.1]), chol0.ravel(), np.zeros(M)])
    b0 = -f(x0)[0]
    res = minimize(f, x0, jac=True, method="L-BFGS-B", options={"maxiter": 60})
    Z, var, ls, chol, m = unpack(res.x)
    r = evaluate(ns, [("rbf", 0, [var, ls], [0], 0)], lik, X, Y, Z, m, chol, 1.0, Xs=X)
    acc = float(np.mean((r["pred_mu"][:, 0] > 0) == (Y[:, 0] == 1)))
    np.savez_compressed(os.path.join(OUT, "toy_classification.npz"), X=X, Y=Y, Z0=Z0, theta0=np.array([1.0, 0.1]), bound_start=b0,
                        bound_end=r["bound"], accuracy=acc, maxiter=60)
    print("toy_classification: bound %.6f -> %.6f, training accuracy %.4f" % (b0, r["bound"], acc))


def main():
    ns = ref_loader.load_sum_kernels(ref_loader.load())
    ns.SVGP = importlib.import_module("GPy.inference.latent_function_inference.svgp").SVGP
    ns.choleskies = importlib.import_module("GPy.util.choleskies")
    ns.Bernoulli = importlib.import_module("GPy.likelihoods.bernoulli").Bernoulli
    ns.StudentT = importlib.import_module("GPy.likelihoods.student_t").StudentT
    ns.Poisson = importlib.import_module("GPy.likelihoods.poisson").Poisson
    os.makedirs(OUT, exist_ok=True)
    case(ns, "gauss_rbf_iso_l1_n200_m30_d2", "gaussian", [0.04], 200, 30, 2, 1, "rbf_iso", 1.0, 1)
    case(ns, "gauss_rbf_ard_l2_n150_m40_d3_bs3", "gaussian", [0.05], 150, 40, 3, 2, "rbf_ard", 3.0, 2)
    case(ns, "gauss_rbf_white_l1_n180_m36_d2", "gaussian", [0.04], 180, 36, 2, 1, "rbf+white", 1.0, 3)
    case(ns, "bern_rbf_iso_l1_n300_m70_d2", "bernoulli", [], 300, 70, 2, 1, "rbf_iso", 1.0, 4)
    case(ns, "bern_matern52_ard_l2_n160_m25_d3_bs3", "bernoulli", [], 160, 25, 3, 2, "matern52_ard", 3.0, 5)
    case(ns, "bern_prod_subset_l1_n170_m30_d4", "bernoulli", [], 170, 30, 4, 1, "prod_subset", 1.0, 6)
    case(ns, "studentt_rbf_iso_l1_n150_m25_d1", "studentt", [0.3, 4.0], 150, 25, 1, 1, "rbf_iso", 1.0, 7)
    case(ns, "poisson_matern32_iso_l1_n140_m20_d2_bs3", "poisson", [], 140, 20, 2, 1, "matern32_iso", 3.0, 8)
    toy_classification(ns)


if __name__ == "__main__":
    main()
