"""Fixtures tests/golden/psi_ss/*.npz FROM THE REFERENCE'S OWN CODE, by the route of tools/make_golden_bgplvm.py:
oracle/ref_loader.py imported unchanged, then the NumPy branch of GPy/kern/src/psi_comp/ssrbf_psi_comp.py (`psicomputations`,
`psiDerivativecomputations`; the branch the module takes when `scipy.weave` is absent) on a posterior that is a plain
namespace of arrays, and `SpikeAndSlabPrior.KL_divergence` / `update_gradients_KL` of
GPy/core/parameterization/variational.py:39-96 on the same arrays.

The `fit_*` fixtures hold one whole SSGPLVM evaluation each, composed from the reference's pieces (`fit_case`), with prediction at
certain and at Gaussian new points; a fit that would enter jitchol's ladder or whose cond2(Kmm + 1e-8 I) exceeds 1e4 is refused.

dL_dpsi2 is symmetric in every fixture: the reference's dZ assumes it.  Kernels with `active_dims` a strict subset are given
inputs that already have only the active columns; the fixture stores the full-width arrays and the subset.  Two rows of gamma
sit at 1e-9 and 1 - 1e-9.  The case `far` has one inducing point 60 lengthscales from everything.

    python tools/make_golden_psi_ss.py
"""
import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "psi_ss")


def case(ss, var_mod, name, N, M, D, dims, ARD, seed, far=False, pi=0.5, prior_variance=1.0):
    r = np.random.default_rng(seed)
    Q = len(dims)
    mu, S, Z = r.uniform(-3, 3, (N, D)), r.uniform(0.05, 1.0, (N, D)), r.uniform(-3, 3, (M, D))
    gamma = r.uniform(0.05, 0.95, (N, D))
    gamma[0], gamma[1] = 1e-9, 1 - 1e-9
    variance, ls = 1.3, r.uniform(0.8, 1.8, Q if ARD else 1)
    if far:
        Z[M // 2] = 60.0 * np.max(ls) + 5.0
    dL0, dL1 = r.standard_normal(N), r.standard_normal((N, M))
    A = r.standard_normal((M, M))
    dL2 = A + A.T
    q = types.SimpleNamespace(mean=mu[:, dims].copy(), variance=S[:, dims].copy(), binary_prob=gamma[:, dims].copy())
    Za = Z[:, dims].copy()
    psi0, psi1, psi2 = ss.psicomputations(variance, ls, Za, q)
    dvar, dl, dZ, dmu, dS, dgamma = ss.psiDerivativecomputations(dL0, dL1, dL2, variance, ls, Za, q)
    out = dict(N=N, M=M, D=D, dims=np.asarray(dims), ARD=int(ARD), variance=variance, lengthscale=ls, Z=Z, mu=mu, S=S,
               gamma=gamma, dL0=dL0, dL1=dL1, dL2=dL2, psi0=psi0, psi1=psi1, psi2=psi2, dvar=np.float64(dvar),
               dl=np.atleast_1d(np.asarray(dl, float)), dZ=dZ, dmu=dmu, dS=dS, dgamma=dgamma)
    # the prior on the full-width posterior
    prior = var_mod.SpikeAndSlabPrior(pi=np.asarray(pi, float), variance=prior_variance)
    P = importlib.import_module("GPy.core.parameterization").Param
    qq = types.SimpleNamespace(mean=P("mean", mu.copy()), variance=P("variance", S.copy()), binary_prob=P("binary_prob", gamma.copy()))
    qq.gamma = qq.binary_prob
    qq.num_data = N
    for p in (qq.mean, qq.variance, qq.binary_prob):
        p.gradient = np.zeros((N, D))
    out["KL"] = np.float64(prior.KL_divergence(qq))
    prior.update_gradients_KL(qq)
    out.update(pi=np.asarray(pi, float), prior_variance=prior_variance, kl_dmu=-np.asarray(qq.mean.gradient, float),
               kl_dS=-np.asarray(qq.variance.gradient, float), kl_dgamma=-np.asarray(qq.binary_prob.gradient, float))
    for k, v in out.items():
        if isinstance(v, np.ndarray) and not np.all(np.isfinite(v)):
            raise RuntimeError("%s: %s is not finite" % (name, k))
    os.makedirs(OUT, exist_ok=True)
    np.savez(os.path.join(OUT, name + ".npz"), **out)
    print("%-12s N=%d M=%d Q=%d ARD=%d  psi2 max %.3e" % (name, N, M, Q, ARD, np.abs(psi2).max()))


COND_MAX = 1e4


def g1(p):
    return np.atleast_1d(np.asarray(p.gradient, float)).ravel().copy()


def fit_case(ns, var_mod, name, N, M, D, dims, ARD, Dy, white, seed, pi=0.5, Nnew=23):
    """One SSGPLVM evaluation composed from the reference's pieces, as `parameters_changed` of GPy/models/ss_gplvm.py:256-270
    composes it: `VarDTC.inference` with a `SpikeAndSlabPosterior` (the kernel's psicomp then takes ssrbf_psi_comp),
    `SpikeAndSlabPrior.KL_divergence`, the kernel and inducing-input gradients of `SparseGP._update_gradients`
    (GPy/core/sparse_gp.py:88-107), `gradients_qX_expectations` followed by `update_gradients_KL`, and `Posterior._raw_predict`
    at certain and at Gaussian new points.  Z on a jittered lattice 1.3 lengthscales apart; refused, not written, if
    Kmm + 1e-8 I has no Cholesky factor without more jitter (jitchol's ladder) or cond2(Kmm + 1e-8 I) exceeds 1e4."""
    vd = importlib.import_module("GPy.inference.latent_function_inference.var_dtc")
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from make_golden_sparse2 import _Lik

    class Q(var_mod.SpikeAndSlabPosterior):
        ndim = 2
        binary_prob = property(lambda self: self.gamma)               # (paramz finds a linked Param by its name)

        def __getitem__(self, s):
            return self

    class QN(var_mod.NormalPosterior):
        ndim = 2

        def __getitem__(self, s):
            return self

    def posterior(m, s, g):
        q = Q(m.copy(), s.copy(), g.copy())
        q.parameters = [q.mean, q.variance, q.binary_prob]
        return q
    r = np.random.default_rng(seed)
    Qa = len(dims)
    ls = r.uniform(0.9, 1.1, Qa if ARD else 1)
    nd = min(Qa, 3)
    side = int(np.ceil(M ** (1.0 / nd)))
    grid = np.stack(np.meshgrid(*[np.arange(side)] * nd, indexing="ij"), -1).reshape(-1, nd)[:M]
    Z = r.uniform(-0.5, 0.5, (M, D))
    Z[:, dims[:nd]] = 1.3 * grid + r.uniform(-0.1, 0.1, grid.shape)
    lo, hi = Z.min(0), Z.max(0)
    mu, S = r.uniform(lo - 0.5, hi + 0.5, (N, D)), r.uniform(0.05, 0.5, (N, D))
    gamma = r.uniform(0.05, 0.95, (N, D))
    gamma[0], gamma[1] = 1e-9, 1 - 1e-9
    Y = np.sin(mu[:, dims].sum(1, keepdims=True) + 0.7 * np.arange(Dy)[None, :]) + 0.1 * r.standard_normal((N, Dy))
    variance, noise = 1.3, 0.05
    rbf = ns.RBF(Qa, variance=variance, lengthscale=ls, ARD=ARD)
    parts = [rbf] + [ns.White(Qa, variance=w) for w in white]
    k = parts[0] if len(parts) == 1 else ns.Add(parts)
    leaves = k.parts if len(parts) > 1 else [k]
    qX = posterior(mu[:, dims], S[:, dims], gamma[:, dims])
    Za = Z[:, dims].copy()
    Kmm = np.asarray(k.K(Za)) + 1e-8 * np.eye(M)
    try:
        np.linalg.cholesky(Kmm)
    except np.linalg.LinAlgError:
        raise SystemExit("%s: Kmm + 1e-8 I is not positive definite (jitchol's ladder): no fixture" % name)
    cond = float(np.linalg.cond(Kmm))
    if cond > COND_MAX:
        raise SystemExit("%s: cond2(Kmm + 1e-8 I) = %.3g exceeds %g: no fixture" % (name, cond, COND_MAX))

    def grads():
        out = []
        for p in leaves:
            out.append(g1(p.variance))
            if hasattr(p, "lengthscale"):
                out.append(g1(p.lengthscale))
        return np.concatenate(out)
    post, lml, gd = vd.VarDTC(limit=1).inference(k, qX, Za, _Lik(noise), Y)                # sparse_gp.py:77-81
    lml = float(np.asarray(lml).ravel()[0])
    a = dict(dL_dpsi0=gd["dL_dpsi0"], dL_dpsi1=gd["dL_dpsi1"], dL_dpsi2=gd["dL_dpsi2"])
    if not np.array_equal(np.asarray(a["dL_dpsi2"]), np.asarray(a["dL_dpsi2"]).T):         # the reference's dZ assumes symmetry
        a["dL_dpsi2"] = 0.5 * (np.asarray(a["dL_dpsi2"]) + np.asarray(a["dL_dpsi2"]).T)
    k.update_gradients_expectations(variational_posterior=qX, Z=Za, **a)                   # sparse_gp.py:90-96
    g = grads().copy()
    k.update_gradients_full(gd["dL_dKmm"], Za, None)
    g += grads()
    dZ = k.gradients_X(gd["dL_dKmm"], Za) + k.gradients_Z_expectations(a["dL_dpsi0"], a["dL_dpsi1"], a["dL_dpsi2"], Z=Za,
                                                                       variational_posterior=qX)
    dmu, dS, dg = (np.array(x, float) for x in k.gradients_qX_expectations(variational_posterior=qX, Z=Za, **a))   # ss_gplvm.py:266
    # the prior on the full-width posterior (the dimensions the kernel does not see have zero fit gradients)
    full = lambda x: (lambda o: (o.__setitem__((slice(None), dims), x), o)[1])(np.zeros((N, D)))
    qF = posterior(mu, S, gamma)
    prior = var_mod.SpikeAndSlabPrior(pi=np.full(D, float(pi)), variance=1.0)
    KL = float(prior.KL_divergence(qF))                                                    # ss_gplvm.py:264
    qF.mean.gradient, qF.variance.gradient, qF.binary_prob.gradient = full(dmu), full(dS), full(dg)
    prior.update_gradients_KL(qF)                                                          # ss_gplvm.py:269
    Xs = r.uniform(lo - 0.5, hi + 0.5, (Nnew, D))
    Ss = r.uniform(0.05, 0.5, (Nnew, D))
    pm, pv = post._raw_predict(k, Xs[:, dims], Za, full_cov=False)
    qn = QN(Xs[:, dims].copy(), Ss[:, dims].copy())
    qn.parameters = [qn.mean, qn.variance]
    um, uv = post._raw_predict(k, qn, Za, full_cov=False)                                  # posterior.py:249-269
    out = dict(mu=mu, S=S, gamma=gamma, Z=Z, Y=Y, dims=np.asarray(dims, int), ARD=bool(ARD), variance=variance, ls=ls,
               white=np.asarray(white, float), noise=noise, pi=float(pi), cond=cond, lml=lml, KL=KL, bound=lml - KL,
               woodbury_vector=np.asarray(post.woodbury_vector), woodbury_inv=np.asarray(post.woodbury_inv), dtheta=g,
               dnoise=np.asarray(gd["dL_dthetaL"], float).ravel(), dZ=np.asarray(dZ), dmu=dmu, dS=dS, dgamma=dg,
               Xmean_grad=np.array(qF.mean.gradient, float), Xvar_grad=np.array(qF.variance.gradient, float),
               Xgamma_grad=np.array(qF.binary_prob.gradient, float), Xs=Xs, Ss=Ss, pred_mu=np.asarray(pm), pred_var=np.asarray(pv),
               upred_mu=np.asarray(um), upred_var=np.asarray(uv))
    for key, v in out.items():
        if isinstance(v, np.ndarray) and v.dtype.kind == "f" and not np.all(np.isfinite(v)):
            raise SystemExit("%s: %s is not finite: no fixture" % (name, key))
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print("%-34s bound=% .12e KL=%.6e cond=%.3g min uncertain var=%.3e" % (name, lml - KL, KL, cond, float(np.min(uv))))


def main():
    ns = ref_loader.load_sum_kernels(ref_loader.load())
    ss = importlib.import_module("GPy.kern.src.psi_comp.ssrbf_psi_comp")
    var_mod = importlib.import_module("GPy.core.parameterization.variational")
    case(ss, var_mod, "ard", 37, 11, 3, [0, 1, 2], True, 1)
    case(ss, var_mod, "iso", 41, 19, 4, [0, 1, 2, 3], False, 2, pi=[0.3, 0.5, 0.6, 0.8], prior_variance=1.7)
    case(ss, var_mod, "subset", 29, 13, 5, [0, 2, 3], True, 3)
    case(ss, var_mod, "far", 23, 9, 2, [0, 1], True, 4, far=True)
    fit_case(ns, var_mod, "fit_ard_q2_dy3_n60_m9", 60, 9, 2, [0, 1], True, 3, [], 31)
    fit_case(ns, var_mod, "fit_iso_q3_white_dy1_n50_m8", 50, 8, 3, [0, 1, 2], False, 1, [0.2], 32, pi=0.3)
    fit_case(ns, var_mod, "fit_ard_active_q3of5_white_dy4_n70_m16", 70, 16, 5, [0, 2, 3], True, 4, [0.3], 33)


if __name__ == "__main__":
    main()
