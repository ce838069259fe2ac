"""NumPy restatement of the RatQuad and StdPeriodic covariances (GPy/kern/src/stationary.py:747-802,
GPy/kern/src/standard_periodic.py:15-580) and of sums / products of them with RBF and White parts: K, dK/dtheta in link
order, gradients_X and the exact-GP quantities.  Written from the formulas; shared by the CPU and GPU tests of the two
kernels.  specs: [(kind, ard, theta, active_dims, term)] as the C-ABI's part list."""
import json

import numpy as np


def load_specs(s):
    return [(k, int(a), np.asarray(t, float), np.asarray(d, int), int(term)) for k, a, t, d, term in json.loads(str(s))]


def _split(kind, ard, th, nd):
    """per-dimension parameter vectors of a leaf"""
    if kind == "ratquad":
        nl = nd if ard else 1
        return dict(var=th[0], ls=np.broadcast_to(th[1:1 + nl], (nd,)), power=th[1 + nl])
    if kind == "stdperiodic":
        npr = nd if ard & 1 else 1
        return dict(var=th[0], T=np.broadcast_to(th[1:1 + npr], (nd,)), ls=np.broadcast_to(th[1 + npr:], (nd,)))
    if kind == "rbf":
        return dict(var=th[0], ls=np.broadcast_to(th[1:], (nd,)))
    return dict(var=th[0])


def leaf_parts(spec, X, X2=None):
    """(K, [dK/dtheta_k in theta order], dK/dx1 per dimension of X (N x M x D, zeros outside active_dims))"""
    kind, ard, th, dims, _ = spec
    sym = X2 is None
    X2 = X if sym else X2
    A, B = X[:, dims], X2[:, dims]
    p = _split(kind, ard, th, len(dims))
    diff = A[:, None, :] - B[None, :, :]                         # N x M x d
    dX = np.zeros((X.shape[0], X2.shape[0], X.shape[1]))
    if kind == "white":
        K = p["var"] * np.eye(X.shape[0]) if sym else np.zeros((X.shape[0], X2.shape[0]))
        return K, [K / p["var"]], dX
    if kind in ("rbf", "ratquad"):
        r2 = np.sum((diff / p["ls"]) ** 2, -1)
        if kind == "rbf":
            K = p["var"] * np.exp(-0.5 * r2)
            dk_or = -K                                           # dK/dr / r
        else:
            K = p["var"] * np.exp(-p["power"] * np.log1p(0.5 * r2))
            dk_or = -p["power"] * K / (1.0 + 0.5 * r2)
        g = [K / p["var"]]
        per_dim = [-dk_or * diff[..., q] ** 2 / p["ls"][q] ** 3 for q in range(len(dims))]   # dK/dl_q
        g += per_dim if ard else [sum(per_dim)]
        if kind == "ratquad":
            g.append(-K * np.log1p(0.5 * r2))
        for a, q in enumerate(dims):
            dX[..., q] = dk_or * diff[..., a] / p["ls"][a] ** 2
        return K, g, dX
    base = np.pi * diff / p["T"]
    sn, cs = np.sin(base), np.cos(base)
    K = p["var"] * np.exp(-0.5 * np.sum((sn / p["ls"]) ** 2, -1))
    g = [K / p["var"]]
    dT = [K * sn[..., q] * cs[..., q] * base[..., q] / (p["T"][q] * p["ls"][q] ** 2) for q in range(len(dims))]
    dL = [K * sn[..., q] ** 2 / p["ls"][q] ** 3 for q in range(len(dims))]
    g += dT if ard & 1 else [sum(dT)]
    g += dL if ard & 2 else [sum(dL)]
    for a, q in enumerate(dims):
        dX[..., q] = -np.pi / (2 * p["T"][a] * p["ls"][a] ** 2) * np.sin(2 * base[..., a]) * K
    return K, g, dX


def terms(specs):
    out, seen = [], {}
    for i, s in enumerate(specs):
        t = s[4]
        if t == 0:
            out.append([i])
        elif t in seen:
            seen[t].append(i)
        else:
            seen[t] = [i]
            out.append(seen[t])
    return out


def expr(specs, X, X2=None):
    """(K, [dK/dtheta over all leaves in spec order], dK/dx1 (N x M x D))"""
    leaves = [leaf_parts(s, X, X2) for s in specs]
    K = 0.0
    dX = 0.0
    grads = [None] * len(specs)
    for t in terms(specs):
        prod = np.prod([leaves[i][0] for i in t], axis=0)
        K = K + prod
        for i in t:
            others = np.prod([leaves[j][0] for j in t if j != i], axis=0) if len(t) > 1 else 1.0
            grads[i] = [gk * others for gk in leaves[i][1]]
            dX = dX + leaves[i][2] * (others[..., None] if len(t) > 1 else 1.0)
    return K, [g for gl in grads for g in gl], dX


def gradients_X(specs, G, X, X2=None):
    """kern.gradients_X(G, X, X2): sum_j G_ij dK(x_i, x2_j)/dx_i  (X2 None: G + G^T against X)"""
    _, _, dX = expr(specs, X, X2)
    W = G + G.T if X2 is None else G
    return np.einsum("ij,ijq->iq", W, dX)


def exact(specs, X, Y, noise, nu=None):
    """(lml, alpha, dtheta, dnoise or dL_dnu) of ExactGaussianInference (or the Student-t process for nu)"""
    K, dK, _ = expr(specs, X)
    N, Dy = Y.shape
    Ky = K + (noise if nu is None else 0.0) * np.eye(N) + 1e-8 * np.eye(N)
    L = np.linalg.cholesky(Ky)
    Ki = np.linalg.inv(Ky)
    alpha = Ki @ Y
    logdet = 2 * np.sum(np.log(np.diag(L)))
    if nu is None:
        lml = 0.5 * (-N * Dy * np.log(2 * np.pi) - Dy * logdet - np.sum(alpha * Y))
        dL_dK = 0.5 * (alpha @ alpha.T - Dy * Ki)
        dn = np.trace(dL_dK)
    else:
        from scipy.special import gammaln
        beta = np.sum(alpha * Y)
        lml = 0.5 * (-N * np.log((nu - 2) * np.pi) - logdet - (nu + N) * np.log(1 + beta / (nu - 2))) + \
            gammaln(0.5 * (nu + N)) - gammaln(0.5 * nu)
        dL_dK = 0.5 * ((nu + N) / (nu + beta - 2) * alpha @ alpha.T - Ki)
        dn = None
    return lml, alpha, np.array([np.sum(dL_dK * g) for g in dK]), dn
