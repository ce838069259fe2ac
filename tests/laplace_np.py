"""NumPy restatement of the Laplace approximation the way the device path splits it (include/mi355gp.h, mi355gp_laplace_*),
written from the formulas of the reference's `laplace.py:122-353` (Rasmussen & Williams, algorithms 3.1 and 5.1):

  newton(K, W, b)        one mode-search iteration through a Cholesky factor of B = I + W^1/2 K W^1/2: (a, K a, logdet B)
  line search            f_trial = f + s K dKi_f is linear in the step s, so the search never touches K
  finish(K, W)           diag(Ki_W_i) = Kdiag - colsumsq(L_B^-1 W^1/2 K), logdet B, K_Wi_i = W^1/2 B^-1 W^1/2
  dL_dK(...)             0.5 (a a^T - K_Wi_i) + 0.5 (a u^T + u a^T), u = dL_dfhat - K_Wi_i K dL_dfhat (the symmetrised form)

Kernels come from mlp_np.expr (every kind and product terms).  Shared by the CPU and the GPU tests."""
import json
import os

import numpy as np
from scipy import optimize
from scipy.linalg import cholesky, solve_triangular

import mlp_np as P
import periodic_np as PN
from gpy_amd.likelihoods import Bernoulli

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "laplace")
# standing tolerances of the kernel fixtures (tests/test_gpu_mlp.py, tests/test_gpu_linear.py): LML 1e-10, vectors 1e-9,
# gradients 1e-8, prediction 1e-9; a case compares at max(standing, 10 x the reference's own convergence floor)
STANDING = {"lml": 1e-10, "f_hat": 1e-9, "Ki_fhat": 1e-9, "dtheta": 1e-8, "dL_dK": 1e-8, "woodbury_inv": 1e-9,
            "pred_mu": 1e-9, "pred_var": 1e-9, "pred_cov": 1e-9, "pred_p": 1e-9}
CASES = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz") and f not in ("bernoulli_values.npz", "toy_1d_optimize.npz"))


def leaf_parts(spec, X, X2=None):
    """mlp_np.leaf_parts plus Matern52 (stationary.py:563-590): K = v (1 + sqrt5 r + 5/3 r^2) exp(-sqrt5 r)"""
    kind, ard, th, dims, _ = spec
    if kind == "stdperiodic":
        return PN.leaf_parts(spec, X, X2)
    if kind != "matern52":
        return P.leaf_parts(spec, X, X2)
    ls = np.broadcast_to(th[1:], (len(dims),))
    A = X[:, dims] / ls
    B = A if X2 is None else X2[:, dims] / ls
    d2 = (A[:, None, :] - B[None, :, :]) ** 2                      # per-dimension squared scaled distances
    r = np.sqrt(d2.sum(-1))
    e = np.exp(-np.sqrt(5.0) * r)
    K = th[0] * (1.0 + np.sqrt(5.0) * r + 5.0 / 3.0 * r * r) * e
    dK_dr_over_r = -th[0] * (5.0 / 3.0) * (1.0 + np.sqrt(5.0) * r) * e   # (dK/dr) / r, finite at r = 0
    per_dim = [-dK_dr_over_r * d2[..., q] / ls[q] for q in range(len(dims))]
    return K, [K / th[0]] + (per_dim if ard else [sum(per_dim)]), None


def leaf_Kdiag(spec, X):
    return np.full(X.shape[0], spec[2][0]) if spec[0] in ("matern52", "stdperiodic") else P.leaf_Kdiag(spec, X)


def expr(specs, X, X2=None):
    """(K, [dK/dtheta over all leaves in spec order]) of the sum of products (add.py:58-72, prod.py:58-99)"""
    leaves = [leaf_parts(s, X, X2) for s in specs]
    K, grads = 0.0, [None] * len(specs)
    for t in P.terms(specs):
        K = K + np.prod([leaves[i][0] for i in t], axis=0)
        for i in t:
            others = np.prod([leaves[j][0] for j in t if j != i], axis=0) if len(t) > 1 else 1.0
            grads[i] = [gk * others for gk in leaves[i][1]]
    return K, [g for gl in grads for g in gl]


def Kdiag(specs, X):
    return sum(np.prod([leaf_Kdiag(specs[i], X) for i in t], axis=0) for t in P.terms(specs))


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    g = {k: z[k] for k in z.files}
    g["specs"] = P.load_specs(g["specs"])
    g["tol"] = {q: max(STANDING[q], 10.0 * float(g["ref_floor_" + q])) for q in STANDING}
    return g


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


def _factor(K, W):
    sw = np.sqrt(W)
    L = cholesky(np.eye(K.shape[0]) + sw[:, None] * K * sw[None, :], lower=True)
    return sw, L


def _Binv(L, v):
    return solve_triangular(L, solve_triangular(L, v, lower=True), lower=True, trans=1)


def newton(K, W, b):
    sw, L = _factor(K, W)
    a = b - sw * _Binv(L, sw * (K @ b))
    return a, K @ a, 2.0 * np.sum(np.log(np.diag(L)))


def line_step(obj, Ki_f, f, dKi_f, Kd):
    """Brent on the step size (tolerance 1e-4 on the step, as the reference), then the full Newton step in its place wherever
    that is as good to rounding (1e-12 of the objective): Brent's step carries an error of 1e-4, which would leave 1e-4 of the
    distance to the mode behind, while the two objectives cannot be told apart.  A line that is flat to rounding (SciPy raises
    BracketError there) is the same situation with no Brent step to compare with."""
    def inner(s):
        return -obj(Ki_f + s * dKi_f, f + s * Kd)
    try:
        s = optimize.brent(inner, tol=1e-4, maxiter=12)
    except Exception as e:
        if type(e).__name__ != "BracketError":
            raise
        s = 0.0
    fs, f1 = inner(s), inner(1.0)
    return 1.0 if f1 <= fs + 1e-12 * max(1.0, abs(fs)) else s


def find_mode(K, Y, lik, tol=1e-10, max_iter=100, polish=False):
    """polish: three full Newton steps after the search (the central-difference test wants the mode to rounding)"""
    y = Y[:, 0]
    Ki_f, f = np.zeros_like(y), np.zeros_like(y)

    def obj(Ki_f, f):
        return -0.5 * np.dot(Ki_f, f) + np.sum(lik.logpdf(f, y))
    diff, it = np.inf, 0
    while diff > tol and it < max_iter:
        W = -lik.d2logpdf_df2(f, y)
        b = W * f + lik.dlogpdf_df(f, y)
        a, Ka, _ = newton(K, W, b)
        dKi_f, Kd = a - Ki_f, Ka - f
        s = line_step(obj, Ki_f, f, dKi_f, Kd)
        new = (Ki_f + s * dKi_f, f + s * Kd)
        diff = abs(obj(*new) - obj(Ki_f, f))
        Ki_f, f = new
        it += 1
    for _ in range(3 if polish else 0):
        W = -lik.d2logpdf_df2(f, y)
        Ki_f, f, _ = newton(K, W, W * f + lik.dlogpdf_df(f, y))
    return f, Ki_f, it


def finish(K, W):
    sw, L = _factor(K, W)
    C = solve_triangular(L, sw[:, None] * K, lower=True)
    LiW = solve_triangular(L, np.diag(sw), lower=True)
    return np.diag(K) - np.sum(C * C, 0), 2.0 * np.sum(np.log(np.diag(L))), LiW.T @ LiW


def dL_dK_sym(K, Ki_f, dL_dfhat, K_Wi_i):
    u = dL_dfhat - K_Wi_i @ (K @ dL_dfhat)
    return 0.5 * (np.outer(Ki_f, Ki_f) - K_Wi_i) + 0.5 * (np.outer(Ki_f, u) + np.outer(u, Ki_f))


def inference(specs, X, Y, tol=1e-10, max_iter=100, lik=None, polish=False):
    """dict(lml, f_hat, Ki_fhat, dtheta, dL_dK (symmetrised), woodbury_inv, W, iterations)"""
    lik = Bernoulli() if lik is None else lik
    K, dKs = expr(specs, X)
    y = Y[:, 0]
    f, Ki_f, it = find_mode(K, Y, lik, tol, max_iter, polish)
    W = -lik.d2logpdf_df2(f, y)
    dKiWi, logdet, K_Wi_i = finish(K, W)
    lml = -0.5 * np.dot(Ki_f, f) + np.sum(lik.logpdf(f, y)) - 0.5 * logdet
    dL_dfhat = -0.5 * dKiWi * (-lik.d3logpdf_df3(f, y))
    G = dL_dK_sym(K, Ki_f, dL_dfhat, K_Wi_i)
    return dict(lml=lml, f_hat=f[:, None], Ki_fhat=Ki_f[:, None], dL_dK=G, woodbury_inv=K_Wi_i, W=W, iterations=it,
                dtheta=np.array([np.sum(G * dK) for dK in dKs]), diag_Ki_W_i=dKiWi, dL_dfhat=dL_dfhat, K=K)


def predict(specs, X, r, Xs, full_cov=False):
    Kx = expr(specs, X, Xs)[0]
    mu = Kx.T @ r["Ki_fhat"]
    if full_cov:
        return mu, expr(specs, Xs)[0] - Kx.T @ r["woodbury_inv"] @ Kx
    return mu, (Kdiag(specs, Xs) - np.sum(Kx * (r["woodbury_inv"] @ Kx), 0))[:, None]


def gpy_amd_kernel(specs):
    """the gpy_amd kernel expression of a part list (with Matern52 and StdPeriodic leaves next to those of mlp_np)"""
    import gpy_amd

    def leaf(spec):
        kind, ard, th, dims, _ = spec
        if kind == "matern52":
            return gpy_amd.Matern52(len(dims), th[0], th[1:], ARD=bool(ard), active_dims=dims)
        if kind == "stdperiodic":
            return gpy_amd.StdPeriodic(len(dims), th[0], th[1], th[2], active_dims=dims)
        return P.gpy_amd_kernel([(kind, ard, th, dims, 0)])
    summands = []
    for t in P.terms(specs):
        k = leaf(specs[t[0]])
        for i in t[1:]:
            k = k * leaf(specs[i])
        summands.append(k)
    k = summands[0]
    for s in summands[1:]:
        k = k + s
    return k


def two_class(N, D, seed, sep=2.0):
    rng = np.random.default_rng(seed)
    y = (rng.random(N) < 0.5).astype(float)
    X = rng.standard_normal((N, D))
    X[:, 0] += sep * (y - 0.5)
    return np.ascontiguousarray(X), y[:, None].copy()
