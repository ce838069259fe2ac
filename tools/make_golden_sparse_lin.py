"""Fixtures tests/golden/sparse_lin/*.npz FROM THE REFERENCE'S OWN CODE for expressions with a Linear part on the sparse path:
`VarDTC.inference` (GPy/inference/latent_function_inference/var_dtc.py), `FITC.inference`, `PEP.inference`, `SVGP.inference` and
one `EPDTC.inference` with its recorded update orders (the recording subclass, inputs and refusals of tools/make_golden_epdtc.py),
the kernels' `update_gradients_diag` / `update_gradients_full` / `gradients_X` assembled as GPy/core/sparse_gp.py:108-119 (and
core/svgp.py:58-65) do for certain inputs, and `Posterior._raw_predict` at 7 new points with `full_cov` both ways, executed
through oracle/ref_loader.py (imported, unchanged).  Only data goes into the fixtures.

Inputs as tools/make_golden_pep.py draws them (Z on a jittered regular grid over the first two active dimensions, lengthscales
0.75 grid spacings there, the unit cube centred at the origin), N <= 60, M <= 12.  A fixture is REFUSED when
cond2(Kmm + jitter I) exceeds 1e3, and when the run would have entered jitchol's ladder: `jitchol` is replaced by a plain
Cholesky factorisation for the run, which raises instead of adding jitter.

    python tools/make_golden_sparse_lin.py
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
import make_golden_epdtc as GE  # noqa: E402
import make_golden_pep as GP  # noqa: E402
import make_golden_svgp as GS  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "sparse_lin")      # (a directory: tests/golden/sparse_*.npz is another family's glob)
COND_CAP = 1e3
GS.NAMES["Linear"] = ("variances",)
_leaf = GS.leaf


def leaf(ns, spec):
    kind, ard, th, dims, _ = spec
    if kind == "linear":
        return ns.Linear(len(dims), variances=np.asarray(th, dtype=float), ARD=bool(ard), active_dims=dims)
    return _leaf(ns, spec)


GS.leaf = leaf


class NoiseModel(object):
    """what VarDTC.inference reads of a likelihood: the noise variance(s) and the pass-through of dL_dR"""

    size = 1                                       # (var_dtc.py:238: a likelihood with parameters)

    def __init__(self, variance):
        self.v = np.atleast_1d(np.asarray(variance, dtype=float))

    def gaussian_variance(self, Y_metadata=None):
        return self.v if self.v.size > 1 else self.v[0]

    def exact_inference_gradients(self, dL_dR, Y_metadata=None):
        return np.asarray(dL_dR, dtype=float)


def strict_jitchol(A, maxtries=5):
    return np.linalg.cholesky(np.asarray(A, dtype=float))          # raises where jitchol would have climbed its ladder


def vardtc(ns, specs, noise, X, Y, Z, Xs):
    k, leaves = GS.assemble(ns, specs)
    post, lml, gd = ns.VarDTC(limit=1).inference(k, X, Z, NoiseModel(noise), Y)
    k.update_gradients_diag(gd["dL_dKdiag"], X)
    g = GS.grads(leaves)
    k.update_gradients_full(gd["dL_dKnm"], X, Z)
    g = g + GS.grads(leaves)
    k.update_gradients_full(gd["dL_dKmm"], Z, None)
    g = g + GS.grads(leaves)
    dZ = k.gradients_X(gd["dL_dKmm"], Z) + k.gradients_X(gd["dL_dKnm"].T, Z, X)
    mu, var = post._raw_predict(k, Xs, pred_var=Z, full_cov=False)
    _, cov = post._raw_predict(k, Xs, pred_var=Z, full_cov=True)
    return dict(lml=float(np.squeeze(lml)), dtheta=g, dZ=np.asarray(dZ, float), dL_dKmm=np.asarray(gd["dL_dKmm"], float),
                dL_dKnm=np.asarray(gd["dL_dKnm"], float), dL_dKdiag=np.asarray(gd["dL_dKdiag"], float).ravel(),
                dL_dthetaL=np.asarray(gd["dL_dthetaL"], float), woodbury_vector=np.asarray(post.woodbury_vector, float),
                woodbury_inv=np.asarray(post.woodbury_inv, float), pred_mu=np.asarray(mu, float), pred_var=np.asarray(var, float),
                pred_cov=np.asarray(cov, float))


def inputs(N, M, D, kern, Dy, seed):
    rng = np.random.default_rng(seed)
    allq = list(range(D))
    gdims = allq[:2]
    Z, g = GS.grid_Z(M, D, gdims, rng)
    X = rng.uniform(0.0, 1.0, (N, D))

    def ls(dims, ard):
        v = np.array([0.75 / g * rng.uniform(0.9, 1.1) if q in gdims else 4.0 * np.sqrt(D) for q in dims])
        return list(v if ard else v[:1])

    def lin(dims, ard, term=0):
        w = 1.0 + 0.5 * np.arange(len(dims))
        return ("linear", int(ard), list(w / w.sum()) if ard else [1.0 / len(dims)], list(dims), term)
    if kern == "rbf+linear":
        specs = [("rbf", 0, [1.2] + ls(allq, 0), allq, 0), lin(allq, 0)]
    elif kern == "rbf+linear_ard+white":
        specs = [("rbf", 1, [1.3] + ls(allq, 1), allq, 0), lin(allq, 1), ("white", 0, [0.05], allq, 0)]
    elif kern == "linear_ard*rbf+bias":
        specs = [lin(allq, 1, 1), ("rbf", 0, [1.3] + ls(allq, 0), allq, 1), ("bias", 0, [0.2], allq, 0)]
    else:                                          # Linear on columns (0, 2) of three, RBF on all of them
        assert kern == "rbf+linear_subset" and D == 3
        specs = [("rbf", 1, [1.1] + ls(allq, 1), allq, 0), lin([0, 2], 1)]
    w = rng.uniform(1.0, 3.0, (min(D, 3), Dy))
    Y = np.sin(2.0 * np.pi * X[:, :w.shape[0]] @ w / w.shape[0]) + X[:, :1] + 0.2 * rng.standard_normal((N, Dy))
    Xs = rng.uniform(0.0, 1.0, (7, D))
    return specs, X - 0.5, Y, Z - 0.5, Xs - 0.5, rng


def save(ns, name, specs, jitter, arrays, **meta):
    k, _ = GS.assemble(ns, specs)
    Z = meta["Z"]
    kappa = float(np.linalg.cond(np.asarray(k.K(Z)) + jitter * np.eye(Z.shape[0])))
    assert kappa <= COND_CAP, "%s refused: cond2(Kmm + %g I) = %.3g exceeds %g" % (name, jitter, kappa, COND_CAP)
    spec_json = json.dumps([[s[0], int(s[1]), [float(v) for v in s[2]], [int(d) for d in s[3]], int(s[4])] for s in specs])
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, specs=spec_json, cond_Kmm=kappa, **dict(arrays, **meta))
    print("%-44s cond(Kmm + %g I) %.1f  %d bytes" % (name, jitter, kappa, os.path.getsize(path)))


def epdtc_case(ns, name, N, M, D, seed):
    """RBF + Linear through make_golden_epdtc.case (two-class data, recorded orders, refused if the run entered jitchol's ladder or
    did not converge), then held to this file's cond cap and marked with its family"""
    sys.modules["GPy.inference.latent_function_inference"].ExactGaussianInference = ns.ExactGaussianInference
    sys.modules["GPy.inference.latent_function_inference"].VarDTC = ns.VarDTC
    sys.modules["GPy.likelihoods"].Gaussian = ns.Gaussian
    ns.Bernoulli = importlib.import_module("GPy.likelihoods.bernoulli").Bernoulli
    ns.ObsAr = importlib.import_module("paramz").ObsAr
    ns.RecordingEPDTC = GE.recording_epdtc(
        importlib.import_module("GPy.inference.latent_function_inference.expectation_propagation").EPDTC)
    GE.watch_jitchol()
    plain = GE.inputs

    def with_linear(N, M, D, kern, seed, sharp=2.0):
        specs, X, Y, Z, Xs = plain(N, M, D, "rbf_iso", seed, sharp)
        return specs + [("linear", 0, [1.0 / D], list(range(D)), 0)], X, Y, Z, Xs
    GE.inputs, GE.OUT = with_linear, OUT
    try:
        GE.case(ns, name, N, M, D, "rbf+linear", seed)
    finally:
        GE.inputs = plain
    path = os.path.join(OUT, name + ".npz")
    fx = dict(np.load(path, allow_pickle=False))
    if float(fx["cond_Kmm"]) > COND_CAP:
        os.remove(path)
        raise RuntimeError("%s refused: cond2(Kmm) = %.3g exceeds %g" % (name, float(fx["cond_Kmm"]), COND_CAP))
    np.savez_compressed(path, family="epdtc", **fx)


def main():
    ns = ref_loader.load_sum_kernels(ref_loader.load())
    ns.Linear = importlib.import_module("GPy.kern.src.linear").Linear
    mods = {n: importlib.import_module("GPy.inference.latent_function_inference." + n) for n in ("var_dtc", "fitc", "pep", "svgp")}
    ns.VarDTC, ns.FITC, ns.PEP, ns.SVGP = mods["var_dtc"].VarDTC, mods["fitc"].FITC, mods["pep"].PEP, mods["svgp"].SVGP
    ns.choleskies = importlib.import_module("GPy.util.choleskies")
    for m in mods.values():                        # a run that would have added jitter raises instead
        if hasattr(m, "jitchol"):
            m.jitchol = strict_jitchol
    os.makedirs(OUT, exist_ok=True)
    for name, kern, N, M, D, Dy, het, seed in (("vardtc_rbf_linear_n50_m9_d2", "rbf+linear", 50, 9, 2, 1, False, 1),
                                               ("vardtc_rbf_linard_white_n60_m12_d3", "rbf+linear_ard+white", 60, 12, 3, 1, False, 2),
                                               ("vardtc_linard_x_rbf_bias_n56_m10_d2", "linear_ard*rbf+bias", 56, 10, 2, 1, False, 3),
                                               ("vardtc_rbf_linear_subset_n60_m12_d3", "rbf+linear_subset", 60, 12, 3, 1, False, 4),
                                               ("vardtc_het_rbf_linard_white_n48_m9_d2", "rbf+linear_ard+white", 48, 9, 2, 1, True, 5),
                                               ("vardtc_dy2_rbf_linear_n52_m10_d2", "rbf+linear", 52, 10, 2, 2, False, 6)):
        specs, X, Y, Z, Xs, rng = inputs(N, M, D, kern, Dy, seed)
        noise = 0.03 + 0.1 * rng.uniform(0.0, 1.0, N) if het else 0.05
        save(ns, name, specs, 1e-8, vardtc(ns, specs, noise, X, Y, Z, Xs), family="vardtc", X=X, Y=Y, Z=Z, Xs=Xs, noise=noise)
    for name, method, alpha, kern, N, M, D, seed in (("fitc_rbf_linard_white_n60_m12_d3", "fitc", 1.0, "rbf+linear_ard+white", 60, 12, 3, 7),
                                                    ("pep_alpha05_rbf_linear_n50_m9_d2", "pep", 0.5, "rbf+linear", 50, 9, 2, 8)):
        specs, X, Y, Z, Xs, rng = inputs(N, M, D, kern, 1, seed)
        save(ns, name, specs, 1e-6, GP.evaluate(ns, method, alpha, specs, 0.05, X, Y, Z, Xs), family="pep", method=method,
             alpha=float(alpha), X=X, Y=Y, Z=Z, Xs=Xs, noise=0.05)
    specs, X, Y, Z, Xs, rng = inputs(60, 10, 2, "rbf+linear_ard+white", 2, 9)
    M, L = 10, 2
    q_mean = 0.5 * rng.standard_normal((M, L))
    chol = np.stack([0.3 * np.eye(M) + 0.05 * np.tril(rng.standard_normal((M, M)), -1) for _ in range(L)])
    q_chol = ns.choleskies.triang_to_flat(chol)
    r = GS.evaluate(ns, specs, GS.make_lik(ns, "gaussian", [0.05]), X, Y, Z, q_mean, q_chol, 1.0, Xs)
    save(ns, "svgp_gauss_rbf_linard_white_l2_n60_m10_d2", specs, 0.0, r, family="svgp", X=X, Y=Y, Z=Z, Xs=Xs, noise=0.05,
         q_mean=q_mean, q_chol=q_chol, q_L=chol)
    epdtc_case(ns, "epdtc_rbf_linear_n60_m12_d2", 60, 12, 2, 11)


if __name__ == "__main__":
    main()
