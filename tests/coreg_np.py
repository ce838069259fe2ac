"""NumPy restatement of the Coregionalize covariance (GPy/kern/src/coregionalize.py:82-157) in sums of products with RBF /
Matern52 factors, the MixedNoise likelihood (GPy/likelihoods/mixed_noise.py) and the exact-GP quantities: K, S, the W /
kappa chain rule, LML, alpha, gradients and prediction.  Written from the formulas; shared by the CPU and GPU tests of
the kernel.  specs: [(kind, ard, theta, active_dims, term)] as in tools/make_golden_coreg.py (a Coregionalize entry: theta =
[W | kappa], ard = rank * 100 + P)."""
import json

import numpy as np
from scipy.special import gammaln


def load_specs(s):
    return [(k, int(a), np.asarray(t, float), np.asarray(d, int), int(term)) for k, a, t, d, term in json.loads(str(s))]


def coreg_WkB(spec):
    """(W, kappa, B) of a Coregionalize spec"""
    _, ard, th, _, _ = spec
    P, r = ard % 100, ard // 100
    W, kappa = th[:P * r].reshape(P, r), th[P * r:]
    return W, kappa, W @ W.T + np.diag(kappa)


def terms(specs):
    out, ids = [], {}
    for i, s in enumerate(specs):
        t = s[4]
        if t == 0:
            out.append([i])
        elif t in ids:
            out[ids[t]].append(i)
        else:
            ids[t] = len(out)
            out.append([i])
    return out


def leaf_K(spec, X, X2=None):
    """(K, [dK/dtheta_k] of the kernel parameters; for Coregionalize: None)"""
    kind, ard, th, dims, _ = spec
    if kind == "white":
        K = th[0] * np.eye(X.shape[0]) if X2 is None else np.zeros((X.shape[0], X2.shape[0]))
        return K, [K / th[0]]
    X2 = X if X2 is None else X2
    if kind in ("coregionalize", "coregionalize_B"):          # "coregionalize_B": theta is B itself (P x P), ard = P
        B = coreg_WkB(spec)[2] if kind == "coregionalize" else th.reshape(ard, ard)
        return B[X[:, dims[0]].astype(int)][:, X2[:, dims[0]].astype(int)], None
    ls = np.broadcast_to(th[1:], (len(dims),))
    diff = X[:, None, dims] - X2[None, :, dims]
    r2 = np.sum((diff / ls) ** 2, -1)
    if kind == "rbf":
        K = th[0] * np.exp(-0.5 * r2)
        dk_or = -K
    else:
        r = np.sqrt(r2)
        e = th[0] * np.exp(-np.sqrt(5.0) * r)
        K = (1.0 + np.sqrt(5.0) * r + 5.0 / 3.0 * r2) * e
        dk_or = -5.0 / 3.0 * (1.0 + np.sqrt(5.0) * r) * e
    per_dim = [-dk_or * diff[..., q] ** 2 / ls[q] ** 3 for q in range(len(dims))]
    return K, [K / th[0]] + (per_dim if ard else [sum(per_dim)])


def expr_K(specs, X, X2=None):
    K = 0.0
    for t in terms(specs):
        Kt = 1.0
        for i in t:
            Kt = Kt * leaf_K(specs[i], X, X2)[0]
        K = K + Kt
    return K


def expr_Kdiag(specs, X):
    kd = np.zeros(X.shape[0])
    for t in terms(specs):
        v = np.ones(X.shape[0])
        for i in t:
            kind, _, th, dims, _ = specs[i]
            if kind == "coregionalize":
                v = v * np.diag(coreg_WkB(specs[i])[2])[X[:, dims[0]].astype(int)]
            else:
                v = v * th[0]
        kd += v
    return kd


def bucket_S(Wm, idx, idx2, P):
    """S[a][b] = sum of Wm over rows with idx = a and columns with idx2 = b"""
    Ea, Eb = np.eye(P)[idx], np.eye(P)[idx2]
    return Ea.T @ Wm @ Eb


def chain_W_kappa(S, W):
    """S -> (dW, dkappa) (coregionalize.py:123-128)"""
    return (S + S.T) @ W, np.diag(S).copy()


def leaf_grads(specs, X, dL_dK):
    """per leaf, in spec order: S (Coregionalize) or the kernel-parameter gradients, from dL_dK of the whole expression"""
    out = [None] * len(specs)
    for t in terms(specs):
        Ks = {i: leaf_K(specs[i], X) for i in t}
        for i in t:
            Wm = dL_dK.copy()
            for j in t:
                if j != i:
                    Wm = Wm * Ks[j][0]
            kind, ard, th, dims, _ = specs[i]
            if kind == "coregionalize":
                idx = X[:, dims[0]].astype(int)
                out[i] = bucket_S(Wm, idx, idx, ard % 100)
            else:
                out[i] = np.array([np.sum(Wm * g) for g in Ks[i][1]])
    return out


def gpy_dtheta(specs, X, dL_dK):
    """dtheta in GPy order (leaves in link order; Coregionalize: W, then kappa)"""
    out = []
    for spec, g in zip(specs, leaf_grads(specs, X, dL_dK)):
        if spec[0] == "coregionalize":
            dW, dk = chain_W_kappa(g, coreg_WkB(spec)[0])
            out += [dW.ravel(), dk]
        else:
            out.append(g)
    return np.concatenate(out)


def noise_vector(noises, X):
    return np.asarray(noises, float)[X[:, -1].astype(int)]


def exact(specs, X, Y, noises=None, nu=None, jitter=1e-8):
    """(lml, alpha, dL_dK, Kyinv, dnoise per output) of the Gaussian (MixedNoise) or Student-t process"""
    N = X.shape[0]
    K = expr_K(specs, X)
    nv = noise_vector(noises, X) if nu is None else np.zeros(N)
    Ky = K + np.diag(nv + jitter)
    L = np.linalg.cholesky(Ky)
    Ki = np.linalg.inv(Ky)
    alpha = Ki @ Y
    logdet = 2 * np.sum(np.log(np.diag(L)))
    Dy = Y.shape[1]
    if nu is None:
        lml = 0.5 * (-N * Dy * np.log(2 * np.pi) - Dy * logdet - np.sum(alpha * Y))
        dL_dK = 0.5 * (alpha @ alpha.T - Dy * Ki)
        P = len(noises)
        dnoise = np.bincount(X[:, -1].astype(int), weights=np.diag(dL_dK), minlength=P)
        return lml, alpha, dL_dK, Ki, dnoise
    beta = float(np.sum(alpha * Y))
    lml = (0.5 * (-N * np.log((nu - 2.0) * np.pi) - logdet - (nu + N) * np.log(1.0 + beta / (nu - 2.0)))
           + gammaln(0.5 * (nu + N)) - gammaln(0.5 * nu))
    dL_dK = 0.5 * ((nu + N) / (nu + beta - 2.0) * alpha @ alpha.T - Ki)
    return lml, alpha, dL_dK, Ki, None


def predict(specs, X, alpha, Kyinv, Xs, full_cov=False, nu=None):
    """latent mean / variance; Student-t process: the variance scaled by (nu + beta - 2) / (nu + N - 2), beta = alpha^T K alpha
    (StudentTPosterior._raw_predict, posterior.py:344-360)"""
    Kx = expr_K(specs, X, Xs)
    mu = Kx.T @ alpha
    sc = 1.0
    if nu is not None:
        beta = float(np.sum(alpha * (expr_K(specs, X) @ alpha)))
        sc = (nu + beta - 2.0) / (nu + X.shape[0] - 2.0)
    if full_cov:
        return mu, sc * (expr_K(specs, Xs) - Kx.T @ Kyinv @ Kx)
    return mu, sc * (expr_Kdiag(specs, Xs) - np.sum(Kx * (Kyinv @ Kx), 0))[:, None]
