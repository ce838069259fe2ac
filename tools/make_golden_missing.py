"""Fixtures tests/golden/missing/*.npz FROM THE REFERENCE'S OWN CODE, by the route of tools/make_golden_bgplvm.py:
oracle/ref_loader.py imported unchanged and the small `NormalPosterior` subclass whose `__getitem__` returns itself.

The reference's `BayesianGPLVMMiniBatch` / `SparseGPMiniBatch` do not import under the test-only paramz stand-in, so the loop of
GPy/models/sparse_gp_minibatch.py:228-286 is composed from its pieces, literally:
    grouping        stochastics.py:57-79 (`SparseGPMissing`: columns with the same NaN rows, in order of their first column)
    statistics      `kern.psi0 / psi1 / psi2n` of the whole q(X), once (sparse_gp_minibatch.py:318-322)
    per group       `VarDTC.inference(kern, X[ninan], Z, lik, Y[ninan][:, d], psi0=psi0[ninan], psi1=psi1[ninan],
                    psi2=psi2n[ninan])`; `full_values[key][ninan] += grad_dict[key]` with an N x M x M `dL_dpsi2`;
                    `woodbury_inv[:, :, d]`, `woodbury_vector[:, d]`; the log marginal likelihoods added up
    gradients       `update_gradients_full(dL_dKmm)` + `update_gradients_expectations`, `gradients_X(dL_dKmm)` +
                    `gradients_Z_expectations` (sparse_gp_minibatch.py:169-188) and `gradients_qX_expectations`, all with the
                    N x M x M `dL_dpsi2`; `NormalPrior.KL_divergence` / `update_gradients_KL` with kl_factr = 1
                    (bayesian_gplvm_minibatch.py:100-126); dL_dthetaL added over the groups
    prediction      `Posterior(woodbury_inv (M x M x Dy), woodbury_vector, K, K_chol)._raw_predict` at certain and at
                    `NormalPosterior` new points (posterior.py:231-268)
Inputs as for tests/golden/psi (|mu| <= 3, S in [0.05, 1]) with Z on a jittered lattice.  A case is refused, not written, if any
call of the reference's `jitchol` gets past its plain attempt (the jitter ladder) or cond2(Kmm + 1e-8 I) exceeds 1e4.

    python tools/make_golden_missing.py
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader  # noqa: E402
from oracle.make_golden_sparse2 import _Lik  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "missing")
COND_MAX = 1e4
LADDER = {"entered": False}


def g1(p):
    return np.atleast_1d(np.asarray(p.gradient, float)).ravel().copy()


def watch_jitchol():
    """wraps the reference's jitter ladder where its modules look it up: a run that gets past the plain attempt is marked"""
    la = importlib.import_module("GPy.util.linalg")
    plain = la.jitchol

    def jitchol(A, maxtries=5):
        L, info = la.lapack.dpotrf(np.ascontiguousarray(A), lower=1)          # jitchol's own first attempt (util/linalg.py:62-65)
        if info == 0:
            return L
        LADDER["entered"] = True
        return plain(A, maxtries)
    for mod in ("GPy.util.linalg", "GPy.inference.latent_function_inference.var_dtc"):
        m = sys.modules.get(mod)
        if m is not None and hasattr(m, "jitchol"):
            m.jitchol = jitchol


def groups(Y):
    """stochastics.py:57-79: [(columns d, observed rows ninan)] in order of first appearance"""
    bdict, order = {}, []
    for d in range(Y.shape[1]):
        inan = np.isnan(Y)[:, d]
        key = inan.tobytes()
        if key not in bdict:
            bdict[key] = [[d], ~inan]
            order.append(key)
        else:
            bdict[key][0].append(d)
    return [bdict[k] for k in order]


def case(ns, name, N, M, Q, ARD, Dy, patterns, white, seed, frac=0.3, Nnew=11):
    vd = importlib.import_module("GPy.inference.latent_function_inference.var_dtc")
    var = importlib.import_module("GPy.core.parameterization.variational")
    pm_ = importlib.import_module("GPy.inference.latent_function_inference.posterior")

    class QX(var.NormalPosterior):
        ndim = 2

        def __getitem__(self, s):
            return self

    def posterior(m, s):
        q = QX(m.copy(), s.copy())
        q.parameters = [q.mean, q.variance]
        return q

    r = np.random.default_rng(seed)
    ls = r.uniform(0.9, 1.1, Q if ARD else 1)
    nd = min(Q, 3)
    side = int(np.ceil(M ** (1.0 / nd)))
    grid = np.stack(np.meshgrid(*[np.arange(side)] * nd, indexing="ij"), -1).reshape(-1, nd)[:M]
    Z = r.uniform(-0.5, 0.5, (M, Q))
    Z[:, :nd] = 1.3 * grid + r.uniform(-0.1, 0.1, grid.shape)
    Z -= Z.mean(0)
    lo, hi = np.maximum(Z.min(0) - 0.5, -3.0), np.minimum(Z.max(0) + 0.5, 3.0)
    mu, S = r.uniform(lo, hi, (N, Q)), r.uniform(0.05, 1.0, (N, Q))
    Yfull = np.sin(mu.sum(1, keepdims=True) + 0.7 * np.arange(Dy)[None, :]) + 0.1 * r.standard_normal((N, Dy))
    # output d follows pattern d % patterns: pattern 0 observes every row but row 1, which NOTHING observes; the last pattern
    # observes ONE row only (row N - 1); the others drop each row with probability frac
    Y = Yfull.copy()
    for k in range(patterns):
        drop = (r.uniform(size=N) < frac) if k else np.zeros(N, dtype=bool)
        if k and k == patterns - 1:
            drop[:] = True
            drop[N - 1] = False
        drop[1] = True
        Y[np.ix_(drop, np.arange(Dy) % patterns == k)] = np.nan
    variance, noise = 1.3, 0.05
    rbf = ns.RBF(Q, variance=variance, lengthscale=ls, ARD=ARD)
    parts = [rbf] + [ns.White(Q, variance=w) for w in white]
    k = parts[0] if len(parts) == 1 else ns.Add(parts)
    leaves = k.parts if len(parts) > 1 else [k]
    qX = posterior(mu, S)
    cond = float(np.linalg.cond(np.asarray(k.K(Z)) + 1e-8 * np.eye(M)))
    if cond > COND_MAX:
        raise SystemExit("%s: cond2(Kmm + 1e-8 I) = %.3g exceeds %g: no fixture" % (name, cond, COND_MAX))

    def grads():
        out = []
        for p in leaves:
            out.append(g1(p.variance))
            if hasattr(p, "lengthscale"):
                out.append(g1(p.lengthscale))
        return np.concatenate(out)
    LADDER["entered"] = False
    psi0, psi1, psi2n = np.asarray(k.psi0(Z, qX)), np.asarray(k.psi1(Z, qX)), np.asarray(k.psi2n(Z, qX))
    full = dict(dL_dKmm=np.zeros((M, M)), dL_dpsi0=np.zeros(N), dL_dpsi1=np.zeros((N, M)), dL_dpsi2=np.zeros((N, M, M)))
    woodbury_inv, woodbury_vector = np.zeros((M, M, Dy)), np.zeros((M, Dy))
    lml, dthetaL, lml_g, gof, W = 0.0, 0.0, [], np.zeros(Dy, int), []
    inf = vd.VarDTC(limit=1)
    for g, (d, ninan) in enumerate(groups(Y)):                                              # sparse_gp_minibatch.py:247-276
        post, l, gd = inf.inference(k, qX, Z, _Lik(noise), Y[ninan][:, d], None, Lm=None, dL_dKmm=None,
                                    psi0=psi0[ninan], psi1=psi1[ninan], psi2=psi2n[ninan])
        full["dL_dKmm"] += gd["dL_dKmm"]
        for key in ("dL_dpsi0", "dL_dpsi1", "dL_dpsi2"):
            full[key][ninan] += gd[key]
        dthetaL = dthetaL + np.asarray(gd["dL_dthetaL"], float)
        woodbury_inv[:, :, d] = np.asarray(post.woodbury_inv)[:, :, None]
        woodbury_vector[:, d] = post.woodbury_vector
        lml += float(np.asarray(l).ravel()[0])
        lml_g.append(float(np.asarray(l).ravel()[0]))
        gof[d] = g
        W.append(ninan.astype(float))
    if LADDER["entered"]:
        raise SystemExit("%s: the reference's jitchol entered its jitter ladder: no fixture" % name)
    a = dict(dL_dpsi0=full["dL_dpsi0"], dL_dpsi1=full["dL_dpsi1"], dL_dpsi2=full["dL_dpsi2"])
    k.update_gradients_full(full["dL_dKmm"], Z, None)                                       # sparse_gp_minibatch.py:171-179
    gk = grads().copy()
    k.update_gradients_expectations(variational_posterior=qX, Z=Z, **a)
    gk += grads()
    dZ = k.gradients_X(full["dL_dKmm"], Z) + k.gradients_Z_expectations(variational_posterior=qX, Z=Z, **a)
    dmu, dS = (np.array(x, float) for x in k.gradients_qX_expectations(variational_posterior=qX, Z=Z, **a))
    prior = var.NormalPrior()
    KL = float(prior.KL_divergence(qX))                                                     # kl_factr = 1
    qX.mean.gradient, qX.variance.gradient = dmu.copy(), dS.copy()
    prior.update_gradients_KL(qX)
    Kmm = np.asarray(k.K(Z)) + 1e-8 * np.eye(M)
    P = pm_.Posterior(woodbury_inv=woodbury_inv, woodbury_vector=woodbury_vector, K=Kmm, mean=None, cov=None,
                      K_chol=np.linalg.cholesky(Kmm))                                       # sparse_gp_minibatch.py:281-283
    Xs, Ss = r.uniform(lo, hi, (Nnew, Q)), r.uniform(0.05, 1.0, (Nnew, Q))
    pmu, pv = P._raw_predict(k, Xs, Z, full_cov=False)
    um, uv = P._raw_predict(k, posterior(Xs, Ss), Z, full_cov=False)
    out = dict(mu=mu, S=S, Z=Z, Y=Y, ARD=bool(ARD), variance=variance, ls=ls, white=np.asarray(white, float), noise=noise, cond=cond,
               group_of_output=gof, W=np.stack(W, 1), lml=lml, lml_g=np.asarray(lml_g), KL=KL, bound=lml - KL,
               woodbury_vector=woodbury_vector, woodbury_inv=woodbury_inv, dL_dKmm=full["dL_dKmm"], dL_dpsi0=full["dL_dpsi0"],
               dtheta=gk, dnoise=np.asarray(dthetaL, float).ravel(), dZ=np.asarray(dZ), dmu=dmu, dS=dS,
               Xmean_grad=np.array(qX.mean.gradient, float), Xvar_grad=np.array(qX.variance.gradient, float), Xs=Xs, Ss=Ss,
               pred_mu=np.asarray(pmu), pred_var=np.asarray(pv), upred_mu=np.asarray(um), upred_var=np.asarray(uv))
    for key, v in out.items():
        if isinstance(v, np.ndarray) and v.dtype.kind == "f" and key != "Y" and not np.all(np.isfinite(v)):
            raise SystemExit("%s: %s is not finite: no fixture" % (name, key))
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print("%-34s bound=% .12e KL=%.6e cond=%.3g groups=%d min uncertain var=%.3e" % (name, lml - KL, KL, cond, len(W), float(np.min(uv))))


def main():
    ns = ref_loader.load_sum_kernels(ref_loader.load())
    importlib.import_module("GPy.inference.latent_function_inference.var_dtc")
    watch_jitchol()
    os.makedirs(OUT, exist_ok=True)
    case(ns, "ard_q2_dy5_g3_n40_m9", 40, 9, 2, True, 5, 3, [], 31)
    case(ns, "iso_q3_dy6_g3_n50_m12", 50, 12, 3, False, 6, 3, [], 32)
    case(ns, "ard_q2_white_dy12_g4_n60_m16", 60, 16, 2, True, 12, 4, [0.2], 33)
    case(ns, "iso_q1_white_dy4_g2_n30_m7", 30, 7, 1, False, 4, 2, [0.3], 34)
    case(ns, "ard_q3_dy12_g9_n70_m17", 70, 17, 3, True, 12, 9, [], 35)


if __name__ == "__main__":
    main()
