"""Fixtures tests/golden/bgplvm/*.npz FROM THE REFERENCE'S OWN CODE, by the route of tools/make_golden_psi.py:
oracle/ref_loader.py imported unchanged and the small `NormalPosterior` subclass whose `__getitem__` returns itself.

The reference's `BayesianGPLVM` class does not import under the test-only paramz stand-in, so its `parameters_changed`
(GPy/models/bayesian_gplvm.py:84-100) is composed from its pieces: `VarDTC.inference` with the `NormalPosterior`,
`NormalPrior.KL_divergence`, `kern.gradients_qX_expectations` followed by `NormalPrior.update_gradients_KL`, the kernel and
inducing-input gradients of `SparseGP._update_gradients` (GPy/core/sparse_gp.py:88-107), and `Posterior._raw_predict`
at certain and at uncertain new points.  `initialize_latent('PCA', Q, Y)` (GPy/util/initialization.py) is recorded on a
fixed Y.  Kernels with `active_dims` a strict subset are given inputs that already have only the active columns; the fixture
stores the full-width arrays.  |mu| <= 3 and S in [0.05, 1], as for tests/golden/psi.

    python tools/make_golden_bgplvm.py
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader  # noqa: E402
from oracle.make_golden_sparse2 import _Lik  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "bgplvm")


def g1(p):
    return np.atleast_1d(np.asarray(p.gradient, float)).ravel().copy()


def case(ns, name, N, M, D, dims, ARD, Dy, white, seed, Nnew=23):
    vd = importlib.import_module("GPy.inference.latent_function_inference.var_dtc")
    var = importlib.import_module("GPy.core.parameterization.variational")

    class Q(var.NormalPosterior):
        ndim = 2

        def __getitem__(self, s):
            return self

    def posterior(m, s):
        q = Q(m.copy(), s.copy())
        q.parameters = [q.mean, q.variance]
        return q

    r = np.random.default_rng(seed)
    Q_ = len(dims)
    mu, S, Z = r.uniform(-3, 3, (N, D)), r.uniform(0.05, 1.0, (N, D)), r.uniform(-3, 3, (M, D))
    Y = np.sin(mu[:, dims].sum(1, keepdims=True) + 0.7 * np.arange(Dy)[None, :]) + 0.1 * r.standard_normal((N, Dy))
    variance, ls = 1.3, r.uniform(0.8, 1.8, Q_ if ARD else 1)
    noise = 0.05
    rbf = ns.RBF(Q_, variance=variance, lengthscale=ls, ARD=ARD)
    parts = [rbf] + [ns.White(Q_, variance=w) for w in white]
    k = parts[0] if len(parts) == 1 else ns.Add(parts)
    leaves = k.parts if len(parts) > 1 else [k]
    qX = posterior(mu[:, dims], S[:, dims])
    Za = Z[:, dims].copy()

    def grads():
        out = []
        for p in leaves:
            out.append(g1(p.variance))
            if hasattr(p, "lengthscale"):
                out.append(g1(p.lengthscale))
        return np.concatenate(out)
    post, lml, gd = vd.VarDTC(limit=1).inference(k, qX, Za, _Lik(noise), Y)                # sparse_gp.py:77-81
    lml = float(np.asarray(lml).ravel()[0])
    prior = var.NormalPrior()
    KL = float(prior.KL_divergence(qX))                                                    # bayesian_gplvm.py:89-90
    a = dict(dL_dpsi0=gd["dL_dpsi0"], dL_dpsi1=gd["dL_dpsi1"], dL_dpsi2=gd["dL_dpsi2"])
    k.update_gradients_expectations(variational_posterior=qX, Z=Za, **a)                   # sparse_gp.py:90-96
    g = grads().copy()
    k.update_gradients_full(gd["dL_dKmm"], Za, None)
    g += grads()
    dZ = k.gradients_X(gd["dL_dKmm"], Za) + k.gradients_Z_expectations(a["dL_dpsi0"], a["dL_dpsi1"], a["dL_dpsi2"], Z=Za,
                                                                       variational_posterior=qX)
    dmu, dS = k.gradients_qX_expectations(variational_posterior=qX, Z=Za, **a)             # bayesian_gplvm.py:92-97
    dmu, dS = np.array(dmu, float), np.array(dS, float)
    qX.mean.gradient, qX.variance.gradient = dmu.copy(), dS.copy()
    prior.update_gradients_KL(qX)                                                          # bayesian_gplvm.py:99
    Xmean_grad, Xvar_grad = np.array(qX.mean.gradient, float), np.array(qX.variance.gradient, float)
    Xs = r.uniform(-3, 3, (Nnew, D))
    Ss = r.uniform(0.05, 1.0, (Nnew, D))
    pm, pv = post._raw_predict(k, Xs[:, dims], Za, full_cov=False)
    um, uv = post._raw_predict(k, posterior(Xs[:, dims], Ss[:, dims]), Za, full_cov=False)  # posterior.py:249-269
    np.savez_compressed(
        os.path.join(OUT, name + ".npz"), mu=mu, S=S, Z=Z, Y=Y, dims=np.asarray(dims, int), ARD=bool(ARD), variance=variance,
        ls=ls, white=np.asarray(white, float), noise=noise, lml=lml, KL=KL, bound=lml - KL,
        woodbury_vector=np.asarray(post.woodbury_vector), woodbury_inv=np.asarray(post.woodbury_inv), dtheta=g,
        dnoise=np.asarray(gd["dL_dthetaL"], float).ravel(), dZ=np.asarray(dZ), dmu=dmu, dS=dS, Xmean_grad=Xmean_grad,
        Xvar_grad=Xvar_grad, Xs=Xs, Ss=Ss, pred_mu=np.asarray(pm), pred_var=np.asarray(pv), upred_mu=np.asarray(um),
        upred_var=np.asarray(uv))
    print("%-40s bound=% .12e KL=%.6e min uncertain var=%.3e" % (name, lml - KL, KL, float(np.min(uv))))


def pca_case(name, N, Dy, Q, seed):
    ini = importlib.import_module("GPy.util.initialization")
    r = np.random.default_rng(seed)
    t = r.uniform(-2, 2, (N, 2))
    Y = np.tanh(t @ r.standard_normal((2, Dy))) + 0.3 * t[:, :1] * r.standard_normal((1, Dy)) + 0.05 * r.standard_normal((N, Dy))
    X, fracs = ini.initialize_latent("PCA", Q, Y)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), Y=Y, Q=Q, X=np.asarray(X), fracs=np.asarray(fracs))
    print("%-40s fracs=%s" % (name, np.asarray(fracs)))


def main():
    ns = ref_loader.load_sum_kernels(ref_loader.load())
    os.makedirs(OUT, exist_ok=True)
    case(ns, "iso_q1_dy1_n40_m7", 40, 7, 1, [0], False, 1, [], 11)
    case(ns, "ard_q2_dy3_n120_m12", 120, 12, 2, [0, 1], True, 3, [], 12)
    case(ns, "ard_q3_dy12_n90_m15", 90, 15, 3, [0, 1, 2], True, 12, [], 13)
    case(ns, "iso_q3_dy3_n60_m10", 60, 10, 3, [0, 1, 2], False, 3, [], 14)
    case(ns, "ard_active_q2of4_dy3_n200_m20", 200, 20, 4, [3, 1], True, 3, [], 15)
    case(ns, "ard_q2_white_dy12_n150_m10", 150, 10, 2, [0, 1], True, 12, [0.3], 16)
    case(ns, "iso_q1_white_dy1_n60_m9", 60, 9, 1, [0], False, 1, [0.2], 17)
    pca_case("pca_n50_dy12_q5", 50, 12, 5, 21)
    pca_case("pca_dual_n8_dy12_q3", 8, 12, 3, 22)


if __name__ == "__main__":
    main()
