"""Fixtures tests/golden/psi_lin/*.npz FROM THE REFERENCE'S OWN CODE, by the route of tools/make_golden_psi.py:
oracle/ref_loader.py imported unchanged and the small `NormalPosterior` subclass whose `__getitem__` returns itself.

One input-dependent part, `Linear` (GPy/kern/src/linear.py, psi_comp/linear_psi_comp.py) or `RBF`, with `Bias` and `White`
parts (static.py:133-189, the cross terms of add.py:147-266): `VarDTC.inference` with the `NormalPosterior`, the three
`*_expectations` gradients, the Kmm gradients of `SparseGP._update_gradients` (GPy/core/sparse_gp.py:88-107),
`Posterior._raw_predict` at certain and at uncertain new points, the KL pieces of one BayesianGPLVM composition
(bayesian_gplvm.py:84-100), and the kernel-level psi0 / psi1 / psi2 / psi2n of the input-dependent part, of a Bias part and of
the sum with their chain rule for random dL_dpsi*.  Kernels with `active_dims` a strict subset are given inputs that already
have only the active columns; the fixture stores the full-width arrays.

A fixture is refused, not written, if Kmm + 1e-8 I has no Cholesky factor without more jitter (jitchol's ladder would be
entered) or cond2(Kmm + 1e-8 I) exceeds 1e4: `Linear` alone with M > D has a rank-deficient Kmm and is no fixture.

    python tools/make_golden_psi_lin.py
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader  # noqa: E402
from oracle.make_golden_sparse2 import _Lik  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "psi_lin")
COND_MAX = 1e4


def g1(p):
    return np.atleast_1d(np.asarray(p.gradient, float)).ravel().copy()


def case(ns, name, P, N, M, D, dims, ARD, Dy, bias, white, seed, Nnew=11):
    vd = importlib.import_module("GPy.inference.latent_function_inference.var_dtc")
    var = importlib.import_module("GPy.core.parameterization.variational")
    Linear = importlib.import_module("GPy.kern.src.linear").Linear

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
    mu, S, Z = r.uniform(-2, 2, (N, D)), r.uniform(0.05, 0.5, (N, D)), r.uniform(-2, 2, (M, D))
    noise = 0.05
    if P == "linear":
        Y = mu[:, dims] @ (r.standard_normal((Q_, Dy)) / np.sqrt(Q_)) + 0.3 + 0.1 * r.standard_normal((N, Dy))
        theta = r.uniform(0.5, 1.5, Q_ if ARD else 1)

        def make():
            return Linear(Q_, variances=theta.copy(), ARD=ARD)
    else:
        Y = np.sin(mu[:, dims].sum(1, keepdims=True) / np.sqrt(Q_) + np.arange(Dy)[None, :]) + 0.3 + 0.1 * r.standard_normal((N, Dy))
        theta = np.concatenate([[1.3], r.uniform(0.9, 1.8, Q_ if ARD else 1)])

        def make():
            return ns.RBF(Q_, variance=theta[0], lengthscale=theta[1:].copy(), ARD=ARD)

    def expression():
        parts = [make()] + [ns.Bias(Q_, variance=b) for b in bias] + [ns.White(Q_, variance=w) for w in white]
        k = parts[0] if len(parts) == 1 else ns.Add(parts)
        return k, (k.parts if len(parts) > 1 else [k])

    def grads(leaves):
        out = []
        for p in leaves:
            out.append(g1(p.variances) if hasattr(p, "variances") else g1(p.variance))
            if hasattr(p, "lengthscale"):
                out.append(g1(p.lengthscale))
        return np.concatenate(out)
    k, leaves = expression()
    qX = posterior(mu[:, dims], S[:, dims])
    Za = Z[:, dims].copy()
    Kmm = np.asarray(k.K(Za)) + 1e-8 * np.eye(M)
    try:
        np.linalg.cholesky(Kmm)
    except np.linalg.LinAlgError:
        raise SystemExit("%s: Kmm + 1e-8 I is not positive definite (jitchol's ladder): no fixture" % name)
    cond = float(np.linalg.cond(Kmm))
    if cond > COND_MAX:
        raise SystemExit("%s: cond2(Kmm + 1e-8 I) = %.3g exceeds %g: no fixture" % (name, cond, COND_MAX))
    post, lml, gd = vd.VarDTC(limit=1).inference(k, qX, Za, _Lik(noise), Y)
    lml = float(np.asarray(lml).ravel()[0])
    a = dict(dL_dpsi0=gd["dL_dpsi0"], dL_dpsi1=gd["dL_dpsi1"], dL_dpsi2=gd["dL_dpsi2"])
    k.update_gradients_expectations(variational_posterior=qX, Z=Za, **a)                   # sparse_gp.py:90-96
    g = grads(leaves).copy()
    k.update_gradients_full(gd["dL_dKmm"], Za, None)
    g += grads(leaves)
    dZ = k.gradients_X(gd["dL_dKmm"], Za) + k.gradients_Z_expectations(a["dL_dpsi0"], a["dL_dpsi1"], a["dL_dpsi2"], Z=Za,
                                                                       variational_posterior=qX)
    dmu, dS = k.gradients_qX_expectations(variational_posterior=qX, Z=Za, **a)             # bayesian_gplvm.py:92-97
    dmu, dS = np.array(dmu, float), np.array(dS, float)
    prior = var.NormalPrior()
    KL = float(prior.KL_divergence(qX))                                                    # bayesian_gplvm.py:89-90
    qX.mean.gradient, qX.variance.gradient = dmu.copy(), dS.copy()
    prior.update_gradients_KL(qX)                                                          # bayesian_gplvm.py:99
    Xmean_grad, Xvar_grad = np.array(qX.mean.gradient, float), np.array(qX.variance.gradient, float)
    Xs, Ss = r.uniform(-2, 2, (Nnew, D)), r.uniform(0.05, 0.5, (Nnew, D))
    pm, pv = post._raw_predict(k, Xs[:, dims], Za, full_cov=False)
    um, uv = post._raw_predict(k, posterior(Xs[:, dims], Ss[:, dims]), Za, full_cov=False)  # posterior.py:249-269
    # the kernel-level statistics and chain rule for random dL_dpsi*: the input-dependent part alone, a Bias part alone, the sum
    r2 = np.random.default_rng(seed + 50)
    d0, d1, d2 = r2.standard_normal(N), r2.standard_normal((N, M)), r2.standard_normal((M, M))
    q4 = posterior(mu[:4, dims], S[:4, dims])

    def level(kern, lv):
        kern.update_gradients_expectations(d0, d1, d2, Za, qX)
        return dict(psi0=np.asarray(kern.psi0(Za, qX)), psi1=np.asarray(kern.psi1(Za, qX)), psi2=np.asarray(kern.psi2(Za, qX)),
                    psi2n=np.asarray(kern.psi2n(Za, q4)), dtheta=grads(lv),
                    dZ=np.asarray(kern.gradients_Z_expectations(d0, d1, d2, Za, qX)),
                    dmu=np.asarray(kern.gradients_qX_expectations(d0, d1, d2, Za, qX)[0]),
                    dS=np.asarray(kern.gradients_qX_expectations(d0, d1, d2, Za, qX)[1]))
    lone = make()
    levels = {"p": level(lone, [lone]), "s": level(*expression())}
    bk = ns.Bias(Q_, variance=0.6)
    levels["b"] = level(bk, [bk])
    flat = dict(("k%s_%s" % (t, n), v) for t, d in levels.items() for n, v in d.items())
    np.savez_compressed(
        os.path.join(OUT, name + ".npz"), P=P, mu=mu, S=S, Z=Z, Y=Y, dims=np.asarray(dims, int), ARD=bool(ARD), theta=theta,
        bias=np.asarray(bias, float), white=np.asarray(white, float), noise=noise, cond=cond, lml=lml, KL=KL, bound=lml - KL,
        woodbury_vector=np.asarray(post.woodbury_vector), woodbury_inv=np.asarray(post.woodbury_inv), dtheta=g,
        dnoise=np.asarray(gd["dL_dthetaL"], float).ravel(), dZ=np.asarray(dZ), dmu=dmu, dS=dS, Xmean_grad=Xmean_grad,
        Xvar_grad=Xvar_grad, dL_dKmm=np.asarray(gd["dL_dKmm"]), dL_dpsi0=np.asarray(gd["dL_dpsi0"]),
        dL_dpsi1=np.asarray(gd["dL_dpsi1"]), dL_dpsi2=np.asarray(gd["dL_dpsi2"]), k_d0=d0, k_d1=d1, k_d2=d2, kb_variance=0.6,
        Xs=Xs, Ss=Ss, pred_mu=np.asarray(pm), pred_var=np.asarray(pv), upred_mu=np.asarray(um), upred_var=np.asarray(uv), **flat)
    print("%-44s lml=% .12e cond=%.3g |dmu|=%.6e" % (name, lml, cond, np.linalg.norm(dmu)))


def main():
    ns = ref_loader.load_sum_kernels(ref_loader.load())
    os.makedirs(OUT, exist_ok=True)
    case(ns, "linard_bias_white_dy1_n60_m8_d3", "linear", 60, 8, 3, [0, 1, 2], True, 1, [0.7], [0.2], 31)
    case(ns, "liniso_white_dy3_n50_m7_d2", "linear", 50, 7, 2, [0, 1], False, 3, [], [0.2], 32)
    case(ns, "linard_alone_dy1_n40_m3_d4", "linear", 40, 3, 4, [0, 1, 2, 3], True, 1, [], [], 33)
    case(ns, "linard_active_q2of4_bias_white_dy3_n70_m9", "linear", 70, 9, 4, [3, 1], True, 3, [0.5], [0.3], 34)
    case(ns, "rbfard_bias_dy1_n60_m6_d2", "rbf", 60, 6, 2, [0, 1], True, 1, [0.7], [], 35)
    case(ns, "rbfiso_bias_white_dy3_n80_m9_d2", "rbf", 80, 9, 2, [0, 1], False, 3, [0.4], [0.2], 36)
    case(ns, "rbfard_bias_white_dy1_n50_m8_d3", "rbf", 50, 8, 3, [0, 1, 2], True, 1, [0.5], [0.2], 37)
    case(ns, "linard_bias_white_dy3_n45_m10_d3", "linear", 45, 10, 3, [0, 1, 2], True, 3, [0.5], [0.2], 38)
    # (two Bias parts are no fixture: the reference leaves its exact psi-statistics for Gauss-Hermite quadrature as soon as a sum
    #  holds more than one Bias or more than one White part, add.py:33-44; tests/psi_lin_ld.py covers them in long double)


if __name__ == "__main__":
    main()
