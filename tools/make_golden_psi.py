"""Fixtures tests/golden/psi/*.npz FROM THE REFERENCE'S OWN CODE: `VarDTC.inference` with a `NormalPosterior` X
(GPy/inference/latent_function_inference/var_dtc.py), `RBF.psi0 / psi1 / psi2` (GPy/kern/src/psi_comp/rbf_psi_comp.py),
`update_gradients_expectations`, `gradients_Z_expectations`, `gradients_qX_expectations`, the Kmm gradients of
`SparseGP._update_gradients` (GPy/core/sparse_gp.py:88-107) and `Posterior._raw_predict`, executed through
oracle/ref_loader.py (imported, unchanged).

The test-only paramz stand-in cannot slice the reference's `NormalPosterior`, so the generator hands the reference a small
subclass that returns itself from `__getitem__` and carries `parameters`; kernels with `active_dims` a strict subset are
therefore given inputs that already have only the active columns, and the fixture stores the full-width arrays with the
inactive columns filled from the seed.  |mu| <= 3 and S in [0.05, 1]: the range in which the reference's expanded psi2
exponent (rbf_psi_comp.py:48) keeps its digits.

    python tools/make_golden_psi.py
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader  # noqa: E402
from oracle.make_golden_sparse2 import _Lik  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "psi")


def g1(p):
    return np.atleast_1d(np.asarray(p.gradient, float)).ravel().copy()


def case(ns, name, N, M, D, dims, ARD, Dy, white, seed):
    vd = importlib.import_module("GPy.inference.latent_function_inference.var_dtc")
    var = importlib.import_module("GPy.core.parameterization.variational")

    class Q(var.NormalPosterior):
        ndim = 2

        def __getitem__(self, s):
            return self

    r = np.random.default_rng(seed)
    Q_ = len(dims)
    mu, S, Z = r.uniform(-3, 3, (N, D)), r.uniform(0.05, 1.0, (N, D)), r.uniform(-3, 3, (M, D))
    Y = np.sin(mu[:, dims].sum(1, keepdims=True) + np.arange(Dy)[None, :]) + 0.1 * r.standard_normal((N, Dy))
    variance, ls = 1.3, r.uniform(0.8, 1.8, Q_ if ARD else 1)
    noise = 0.05
    rbf = ns.RBF(Q_, variance=variance, lengthscale=ls, ARD=ARD)
    parts = [rbf] + [ns.White(Q_, variance=w) for w in white]
    k = parts[0] if len(parts) == 1 else ns.Add(parts)
    leaves = k.parts if len(parts) > 1 else [k]
    qX = Q(mu[:, dims].copy(), S[:, dims].copy())
    qX.parameters = [qX.mean, qX.variance]
    Za = Z[:, dims].copy()

    def grads():
        out = []
        for p in leaves:
            out.append(g1(p.variance))
            if hasattr(p, "lengthscale"):
                out.append(g1(p.lengthscale))
        return np.concatenate(out)
    post, lml, gd = vd.VarDTC(limit=1).inference(k, qX, Za, _Lik(noise), Y)
    a = dict(dL_dpsi0=gd["dL_dpsi0"], dL_dpsi1=gd["dL_dpsi1"], dL_dpsi2=gd["dL_dpsi2"])
    k.update_gradients_expectations(variational_posterior=qX, Z=Za, **a)            # sparse_gp.py:90-96
    g = grads().copy()
    k.update_gradients_full(gd["dL_dKmm"], Za, None)
    g += grads()
    dZ = k.gradients_X(gd["dL_dKmm"], Za) + k.gradients_Z_expectations(a["dL_dpsi0"], a["dL_dpsi1"], a["dL_dpsi2"], Z=Za,
                                                                       variational_posterior=qX)
    dmu, dS = k.gradients_qX_expectations(variational_posterior=qX, Z=Za, **a)
    Xs = r.uniform(-3, 3, (17, D))
    pm, pv = post._raw_predict(k, Xs[:, dims], Za, full_cov=False)
    # the RBF part's own statistics and chain rule, for the kernel-level comparisons
    r2 = np.random.default_rng(seed + 50)
    d0, d1, d2 = r2.standard_normal(N), r2.standard_normal((N, M)), r2.standard_normal((M, M))
    rbf2 = ns.RBF(Q_, variance=variance, lengthscale=ls, ARD=ARD)
    rbf2.update_gradients_expectations(d0, d1, d2, Za, qX)
    kg = np.concatenate([g1(rbf2.variance), g1(rbf2.lengthscale)])
    kZ = rbf2.gradients_Z_expectations(d0, d1, d2, Za, qX)
    kmu, kS = rbf2.gradients_qX_expectations(d0, d1, d2, Za, qX)
    np.savez_compressed(
        os.path.join(OUT, name + ".npz"), mu=mu, S=S, Z=Z, Y=Y, dims=np.asarray(dims, int), ARD=bool(ARD), variance=variance,
        ls=ls, white=np.asarray(white, float), noise=noise, lml=float(np.asarray(lml).ravel()[0]),
        woodbury_vector=np.asarray(post.woodbury_vector), dtheta=g, dnoise=np.asarray(gd["dL_dthetaL"], float).ravel(),
        dZ=np.asarray(dZ), dmu=np.asarray(dmu), dS=np.asarray(dS), dL_dKmm=np.asarray(gd["dL_dKmm"]),
        dL_dpsi0=np.asarray(gd["dL_dpsi0"]), dL_dpsi1=np.asarray(gd["dL_dpsi1"]), dL_dpsi2=np.asarray(gd["dL_dpsi2"]),
        psi0=np.asarray(rbf2.psi0(Za, qX)), psi1=np.asarray(rbf2.psi1(Za, qX)), psi2=np.asarray(rbf2.psi2(Za, qX)),
        k_d0=d0, k_d1=d1, k_d2=d2, k_dtheta=kg, k_dZ=np.asarray(kZ), k_dmu=np.asarray(kmu), k_dS=np.asarray(kS),
        Xs=Xs, pred_mu=np.asarray(pm), pred_var=np.asarray(pv))
    print("%-40s lml=% .12e |dZ|=%.6e" % (name, float(np.asarray(lml).ravel()[0]), np.linalg.norm(dZ)))


def main():
    ns = ref_loader.load_sum_kernels(ref_loader.load())
    os.makedirs(OUT, exist_ok=True)
    case(ns, "iso_q1_dy1_n40_m7", 40, 7, 1, [0], False, 1, [], 1)
    case(ns, "ard_q2_dy3_n120_m12", 120, 12, 2, [0, 1], True, 3, [], 2)
    case(ns, "iso_q3_dy1_n90_m15", 90, 15, 3, [0, 1, 2], False, 1, [], 3)
    case(ns, "ard_active_q2of4_dy1_n200_m20", 200, 20, 4, [3, 1], True, 1, [], 4)
    case(ns, "ard_q2_white_dy1_n150_m10", 150, 10, 2, [0, 1], True, 1, [0.3], 5)
    case(ns, "iso_q1_white_dy3_n60_m9", 60, 9, 1, [0], False, 3, [0.2], 6)


if __name__ == "__main__":
    main()
