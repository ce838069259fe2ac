"""NumPy restatement of the RBF psi-statistics for Gaussian inputs q(x_n) = N(mu_n, diag S_n) and of their gradients
(reference `GPy/kern/src/psi_comp/rbf_psi_comp.py:22-50,70-133`, restated from the formulas, row by row, with every squared
difference evaluated directly).  `dtype=np.longdouble` gives the reference the device kernels are judged against.

    psi0[n]    = var
    psi1[n,m]  = var   exp(-1/2 sum_q [log(S/l^2 + 1) + (mu - z_m)^2 / (S + l^2)])
    psi2n[m,o] = var^2 exp(-1/2 sum_q log(2S/l^2 + 1) - sum_q (z_m - z_o)^2 / (4 l^2) - sum_q (mu - (z_m+z_o)/2)^2 / (2S + l^2))
"""
import numpy as np


def _prep(var, ls, Z, mu, S, dtype):
    Z, mu, S = (np.asarray(a, dtype=dtype) for a in (Z, mu, S))
    l2 = np.broadcast_to(np.asarray(ls, dtype=dtype).ravel() ** 2, (Z.shape[1],)).astype(dtype)
    return dtype(var), l2, Z, mu, S


def psi1_row(var, l2, Z, mu_n, S_n):
    d = mu_n[None, :] - Z                                              # M x Q
    return var * np.exp(-0.5 * (np.log(S_n / l2 + 1).sum() + (d * d / (S_n + l2)[None, :]).sum(1)))


def psi2_row(var, l2, Z, mu_n, S_n):
    dz = Z[:, None, :] - Z[None, :, :]                                 # M x M x Q
    db = mu_n[None, None, :] - 0.5 * (Z[:, None, :] + Z[None, :, :])
    e = -0.5 * np.log(2 * S_n / l2 + 1).sum() - (dz * dz / (4 * l2)).sum(-1) - (db * db / (2 * S_n + l2)).sum(-1)
    return var * var * np.exp(e)


def psi_stats(var, ls, Z, mu, S, weights=None, dtype=np.float64, want_psi2n=False):
    """(psi0 (N), psi1 (N x M), psi2 = sum_n w_n psi2n (M x M)[, psi2n (N x M x M)])"""
    var, l2, Z, mu, S = _prep(var, ls, Z, mu, S, dtype)
    N, M = mu.shape[0], Z.shape[0]
    w = np.ones(N, dtype=dtype) if weights is None else np.asarray(weights, dtype=dtype)
    psi1 = np.empty((N, M), dtype=dtype)
    psi2 = np.zeros((M, M), dtype=dtype)
    rows = []
    for n in range(N):
        psi1[n] = psi1_row(var, l2, Z, mu[n], S[n])
        p2 = psi2_row(var, l2, Z, mu[n], S[n])
        psi2 += w[n] * p2
        if want_psi2n:
            rows.append(p2)
    out = (np.full(N, var, dtype=dtype), psi1, psi2)
    return out + (np.stack(rows),) if want_psi2n else out


def psi_grads(var, ls, ARD, Z, mu, S, dL_dpsi0=None, dL_dpsi1=None, dL_dpsi2=None, weights=None, dtype=np.float64):
    """(dvar, dl (Q if ARD else 1), dZ, dmu, dS) of  sum dL_dpsi0 psi0 + sum dL_dpsi1 * psi1 + sum dL_dpsi2 * psi2."""
    var, l2, Z, mu, S = _prep(var, ls, Z, mu, S, dtype)
    N, Q = mu.shape
    M = Z.shape[0]
    w = np.ones(N, dtype=dtype) if weights is None else np.asarray(weights, dtype=dtype)
    l = np.sqrt(l2)
    dvar = dtype(0)
    dl = np.zeros(Q, dtype=dtype)
    dZ = np.zeros((M, Q), dtype=dtype)
    dmu = np.zeros((N, Q), dtype=dtype)
    dS = np.zeros((N, Q), dtype=dtype)
    if dL_dpsi0 is not None:
        dvar += np.asarray(dL_dpsi0, dtype=dtype).sum()
    G1 = None if dL_dpsi1 is None else np.asarray(dL_dpsi1, dtype=dtype)
    G2 = None if dL_dpsi2 is None else np.asarray(dL_dpsi2, dtype=dtype)
    for n in range(N):
        if G1 is not None:
            L = G1[n] * psi1_row(var, l2, Z, mu[n], S[n])              # M
            d = mu[n][None, :] - Z                                      # M x Q
            den = S[n] + l2                                             # Q
            dvar += L.sum() / var
            dmu[n] += -(L[:, None] * d / den).sum(0)
            dZ += L[:, None] * d / den
            dS[n] += (L[:, None] * 0.5 * (d * d / den ** 2 - 1 / den)).sum(0)
            # d/dl of -1/2 [log(S/l^2 + 1) + d^2/(S + l^2)] = S / (l (S + l^2)) + l d^2 / (S + l^2)^2
            dl += (L[:, None] * (S[n] / (l * den) + l * d * d / den ** 2)).sum(0)
        if G2 is not None:
            L = w[n] * G2 * psi2_row(var, l2, Z, mu[n], S[n])          # M x M
            dz = Z[:, None, :] - Z[None, :, :]
            db = mu[n][None, None, :] - 0.5 * (Z[:, None, :] + Z[None, :, :])
            den = 2 * S[n] + l2
            dvar += 2 * L.sum() / var
            dmu[n] += -(L[:, :, None] * 2 * db / den).sum((0, 1))
            dS[n] += (L[:, :, None] * (2 * db * db / den ** 2 - 1 / den)).sum((0, 1))
            gz = L[:, :, None] * (-dz / (2 * l2) + db / den)            # derivative w.r.t. the FIRST index's z
            dZ += gz.sum(1)
            gz = L[:, :, None] * (dz / (2 * l2) + db / den)             # ... and the second index's
            dZ += gz.sum(0)
            # d/dl of -1/2 log(2S/l^2 + 1) - dz^2/(4 l^2) - db^2/(2S + l^2) = 2S/(l den) + dz^2/(2 l^3) + 2 l db^2/den^2
            dl += (L[:, :, None] * (2 * S[n] / (l * den) + dz * dz / (2 * l ** 3) + 2 * l * db * db / den ** 2)).sum((0, 1))
    return dvar, (dl if ARD else dl.sum(keepdims=True)), dZ, dmu, dS


def objective(var, ls, Z, mu, S, dL_dpsi0, dL_dpsi1, dL_dpsi2, weights=None, dtype=np.float64):
    p0, p1, p2 = psi_stats(var, ls, Z, mu, S, weights, dtype)
    return (np.asarray(dL_dpsi0, dtype=dtype) * p0).sum() + (np.asarray(dL_dpsi1, dtype=dtype) * p1).sum() + \
        (np.asarray(dL_dpsi2, dtype=dtype) * p2).sum()


def problem(N, M, Q, seed, ARD=True, weights=False):
    """seeded inputs in the range the psi-statistics are used in: |mu|, |z| <= 3, S in [0.05, 1], lengthscales in [0.7, 2]"""
    r = np.random.default_rng(seed)
    p = dict(var=1.7, ls=r.uniform(0.7, 2.0, Q if ARD else 1), ARD=ARD, Z=r.uniform(-3, 3, (M, Q)), mu=r.uniform(-3, 3, (N, Q)),
             S=r.uniform(0.05, 1.0, (N, Q)), dL_dpsi0=r.standard_normal(N), dL_dpsi1=r.standard_normal((N, M)),
             dL_dpsi2=r.standard_normal((M, M)), weights=r.uniform(0.2, 2.0, N) if weights else None)
    if Q > 8:       # many dimensions: longer lengthscales keep the statistics away from underflow
        p["ls"] = p["ls"] * np.sqrt(Q)
    return p


# ---- the whole uncertain-input VarDTC evaluation (reference `var_dtc.py:66-276` with psi statistics) -------------------
def _rbf_K(var, l2, Z):
    dz = Z[:, None, :] - Z[None, :, :]
    return var * np.exp(-0.5 * (dz * dz / l2).sum(-1))


def _chol(A):
    """lower Cholesky factor in A's dtype (long double has no LAPACK)"""
    if A.dtype == np.float64:
        return np.linalg.cholesky(A)
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        L[j, j] = np.sqrt(A[j, j] - (L[j, :j] ** 2).sum())
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _tri_inv(L):
    n = L.shape[0]
    X = np.zeros_like(L)
    for j in range(n):
        X[j, j] = 1 / L[j, j]
        for i in range(j + 1, n):
            X[i, j] = -(L[i, j:i] @ X[j:i, j]) / L[i, i]
    return X


def vardtc_uncertain(var, ls, ARD, white, Z, mu, S, Y, noise, dtype=np.float64, want_grads=True):
    """RBF(var, ls) + sum of White variances `white` (a list, may be empty), inputs N(mu, diag S), one noise variance.
    dict(lml, woodbury_vector, dL_dKmm, dL_dpsi0/1/2, dnoise, dvar, dl, dwhite (one entry per White part), dZ, dmu, dS)"""
    v, l2, Zd, mud, Sd = _prep(var, ls, Z, mu, S, dtype)
    Y = np.asarray(Y, dtype=dtype)
    N, Dy = Y.shape
    M = Zd.shape[0]
    wsum = dtype(sum(white))
    beta = 1 / max(dtype(noise), dtype(1e-8))
    psi0, psi1, psi2 = psi_stats(var, ls, Z, mu, S, None, dtype)
    psi0 = psi0 + wsum
    I = np.eye(M, dtype=dtype)
    Kmm = _rbf_K(v, l2, Zd) + (wsum + dtype(1e-8)) * I
    Lmi = _tri_inv(_chol(Kmm))
    A = Lmi @ (beta * psi2) @ Lmi.T
    B = I + A
    LB = _chol(B)
    LBi = _tri_inv(LB)
    c = LBi @ (Lmi @ (psi1.T @ (beta * Y)))
    wv = Lmi.T @ (LBi.T @ c)
    delit = c @ c.T
    data_fit = np.trace(delit)
    P = LBi.T @ (Dy * I + delit) @ LBi
    trYYT = (Y * Y).sum()
    lml = (-0.5 * N * Dy * (np.log(2 * dtype(np.pi)) - np.log(beta)) - 0.5 * beta * trYYT
           - 0.5 * Dy * (psi0.sum() * beta - np.trace(A)) - Dy * np.log(np.diag(LB)).sum() + 0.5 * data_fit)
    out = dict(lml=lml, woodbury_vector=wv)
    if not want_grads:
        return out
    dL_dKmm = Lmi.T @ (-0.5 * P - 0.5 * Dy * B + Dy * I) @ Lmi
    dL_dpsi0 = -0.5 * Dy * beta * np.ones(N, dtype=dtype)
    dL_dpsi1 = (beta * Y) @ wv.T
    dL_dpsi2 = beta * 0.5 * (Lmi.T @ (Dy * I - P) @ Lmi)
    dL_dR = (-0.5 * N * Dy * beta + 0.5 * trYYT * beta ** 2 + 0.5 * Dy * (psi0.sum() * beta ** 2 - np.trace(A) * beta)
             + beta * (0.5 * (A * P).sum() - data_fit))
    sym2 = 0.5 * (dL_dpsi2 + dL_dpsi2.T)                               # rbf_psi_comp.py:109
    dvar, dl, dZ, dmu, dS = psi_grads(var, ls, True, Z, mu, S, dL_dpsi0, dL_dpsi1, sym2, None, dtype)
    # the Kmm part: update_gradients_full(dL_dKmm, Z) and gradients_X(dL_dKmm, Z)
    Kr = _rbf_K(v, l2, Zd)
    G = dL_dKmm * Kr
    dz = Zd[:, None, :] - Zd[None, :, :]
    l = np.sqrt(l2)
    dvar = dvar + G.sum() / v
    dl = dl + (G[:, :, None] * dz * dz).sum((0, 1)) / l ** 3
    Gs = G + G.T
    dZ = dZ - (Gs[:, :, None] * dz).sum(1) / l2
    dwhite = [np.trace(dL_dKmm) + dL_dpsi0.sum() for _ in white]
    out.update(dL_dKmm=dL_dKmm, dL_dpsi0=dL_dpsi0, dL_dpsi1=dL_dpsi1, dL_dpsi2=dL_dpsi2, dnoise=dL_dR, dvar=dvar,
               dl=(dl if ARD else dl.sum(keepdims=True)), dwhite=dwhite, dZ=dZ, dmu=dmu, dS=dS)
    return out


def fit_problem(N, M, Q, Dy, seed, ARD=True, white=()):
    """a seeded regression problem with uncertain inputs in the fixtures' range (|mu| <= 3, S in [0.05, 1])"""
    r = np.random.default_rng(seed)
    mu = r.uniform(-3, 3, (N, Q))
    Y = np.sin(mu.sum(1, keepdims=True) + np.arange(Dy)[None, :]) + 0.1 * r.standard_normal((N, Dy))
    return dict(var=1.3, ls=r.uniform(0.8, 1.8, Q if ARD else 1), ARD=ARD, white=list(white), Z=r.uniform(-3, 3, (M, Q)), mu=mu,
                S=r.uniform(0.05, 1.0, (N, Q)), Y=Y, noise=0.05)
