"""NumPy restatement of expectation propagation the way the device path splits it (include/mi355gp.h, mi355gp_ep_*), written
from the formulas of the reference's `expectation_propagation.py:27-29,52-68,101-143,279-395` (Rasmussen & Williams, algorithm 3.5):

  recompute(K, tau, v)        B = I + S^1/2 K S^1/2 through its Cholesky factor: mu = K alpha, Sigma = K - V^T V (or its diagonal)
  sweep(Sigma, mu, order, ..) one sequential pass over the sites: cavity, moment matching, site update, rank-one update
  parallel_sweep(...)         the same with every site seeing the same q(f): whole-vector arithmetic
  run(K, Y, ...)              sweep, recompute, stop test, as `expectation_propagation` loops them
  final(...)                  the pass after convergence through the laplace_np functions with W = tau, b = v

Kernels come from laplace_np.expr.  Shared by the CPU and the GPU tests."""
import os

import numpy as np
from scipy import special
from scipy.linalg import cholesky, solve_triangular
from scipy.linalg.blas import dger

import laplace_np as LP
import mlp_np as P

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ep")
# the standing tolerances of tests/laplace_np.py by kind of quantity: scalars 1e-10, vectors (the site parameters among them) 1e-9,
# gradients 1e-8, prediction 1e-9; a case compares at max(standing, 10 x the reference's own rounding floor stored with it)
STANDING = {"lml": 1e-10, "log_Z_tilde": 1e-10, "tau_tilde": 1e-9, "v_tilde": 1e-9, "cav_tau": 1e-9, "cav_v": 1e-9, "alpha": 1e-9,
            "Wi": 1e-9, "dL_dK": 1e-8, "dtheta": 1e-8, "pred_mu": 1e-9, "pred_var": 1e-9, "pred_cov": 1e-9, "pred_p": 1e-9}
assert LP.STANDING["lml"] == 1e-10 and LP.STANDING["Ki_fhat"] == 1e-9 and LP.STANDING["dtheta"] == 1e-8 and LP.STANDING["pred_mu"] == 1e-9
OTHER = ("bernoulli_ep_moments.npz", "toy_1d_optimize.npz")
CASES = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz") and f not in OTHER)
EPS = np.finfo(float).eps


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    g = {k: z[k] for k in z.files}
    g["specs"] = P.load_specs(g["specs"])
    g["tol"] = {q: max(STANDING[q], 10.0 * float(g["ref_floor_" + q])) for q in STANDING}
    for k in ("sweeps", "parallel_updates", "eta", "delta", "epsilon", "clamped"):
        g[k] = g[k].item()
    return g


def ysign(Y):
    return np.where(np.asarray(Y)[:, 0] == 1, 1.0, -1.0)


def recompute(K, tau, v, add_diag=0.0, want_sigma=True):
    """(mu, diag(Sigma) + add_diag, log det B, Sigma + add_diag I or None)"""
    sw, L = LP._factor(K, tau)
    V = solve_triangular(L, sw[:, None] * K, lower=True)
    alpha = v - sw * LP._Binv(L, sw * (K @ v))
    logdet = 2.0 * np.sum(np.log(np.diag(L)))
    if not want_sigma:
        return K @ alpha, np.diag(K) - np.sum(V * V, 0) + add_diag, logdet, None
    Sigma = np.asfortranarray(K - V.T @ V)
    Sigma[np.diag_indices_from(Sigma)] += add_diag
    return K @ alpha, np.diag(Sigma).copy(), logdet, Sigma


def log_moments(sign, ct, cv):
    """(log Z_hat, mu_hat, sigma2_hat) of the probit site against the cavity N(cv / ct, 1 / ct) (bernoulli.py:73-79)"""
    q = ct * ct + ct
    z = sign * cv / np.sqrt(q)
    lz = special.log_ndtr(z)
    zn = np.minimum(z, 0.0)
    r = np.where(z < 0, np.sqrt(2.0 / np.pi) / special.erfcx(-zn / np.sqrt(2.0)),
                 np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi) / special.ndtr(np.maximum(z, 0.0)))
    return lz, cv / ct + sign * r / np.sqrt(q), 1.0 / ct - (r / q) * (z + r)


def sweep(Sigma, mu, order, sign, eta, delta, tau, v):
    """in place on Sigma (Fortran order, symmetric) and on copies of mu, tau, v: dict(tau, v, cav_tau, cav_v, log_Z_hat, mu, Sigma_diag)"""
    n = mu.size
    mu, tau, v = mu.copy(), tau.copy(), v.copy()
    ct, cv, lz = np.empty(n), np.empty(n), np.empty(n)
    for i in order:
        si = Sigma[:, i].copy()
        sii, mui = si[i], mu[i]
        ct[i] = 1.0 / sii - eta * tau[i]
        cv[i] = mui / sii - eta * v[i]
        lz[i], mu_hat, s2_hat = log_moments(sign[i], ct[i], cv[i])
        dtau = delta / eta * (1.0 / s2_hat - 1.0 / sii)
        dv = delta / eta * (mu_hat / s2_hat - mui / sii)
        prev = tau[i]
        tau[i] += dtau
        if tau[i] < EPS:
            tau[i] = EPS
            dtau = tau[i] - prev
        v[i] += dv
        ci = dtau / (1.0 + dtau * sii)
        mu -= (ci * (mui + sii * dv) - dv) * si
        if ci != 0.0:
            dger(-ci, si, si, a=Sigma, overwrite_a=1)
    return dict(tau=tau, v=v, cav_tau=ct, cav_v=cv, log_Z_hat=lz, mu=mu, Sigma_diag=np.diag(Sigma).copy())


def parallel_sweep(mu, sd, sign, eta, delta, tau, v):
    ct = 1.0 / sd - eta * tau
    cv = mu / sd - eta * v
    lz, mu_hat, s2_hat = log_moments(sign, ct, cv)
    dtau = delta / eta * (1.0 / s2_hat - 1.0 / sd)
    dv = delta / eta * (mu_hat / s2_hat - mu / sd)
    return dict(tau=np.maximum(tau + dtau, EPS), v=v + dv, cav_tau=ct, cav_v=cv, log_Z_hat=lz)


def log_Z_tilde(lz, tau, v, ct, cv):
    """(expectation_propagation.py:353-361)"""
    return np.sum(lz + 0.5 * np.log(2 * np.pi) + 0.5 * np.log(1 + tau / ct) - 0.5 * (v ** 2 / (ct + tau))
                  + 0.5 * (cv * ((tau / ct * cv - 2.0 * v) / (ct + tau))))


def run(K, Y, orders=None, parallel=False, eta=1.0, delta=1.0, epsilon=1e-6, max_iters=100, tau0=None, v0=None, seed=0):
    """`expectation_propagation` (:279-310): dict(tau, v, cav_tau, cav_v, log_Z_tilde, sweeps, converged)"""
    n = K.shape[0]
    sign = ysign(Y)
    rng = np.random.default_rng(seed)
    tau, v = (np.zeros(n), np.zeros(n)) if tau0 is None else (tau0.copy(), v0.copy())
    mu, sd, _, Sigma = recompute(K, tau, v, 1e-7, not parallel)
    stop, it, old = False, 0, None
    while not stop and it < max_iters:
        if parallel:
            r = parallel_sweep(mu, sd, sign, eta, delta, tau, v)
        else:
            r = sweep(Sigma, mu, orders[it] if orders is not None else rng.permutation(n), sign, eta, delta, tau, v)
        tau, v = r["tau"], r["v"]
        mu, sd, _, Sigma = recompute(K, tau, v, 0.0, not parallel)
        if it > 0:
            stop = bool(np.mean(np.square(tau - old[0])) < epsilon and np.mean(np.square(v - old[1])) < epsilon)
        old = (tau.copy(), v.copy())
        it += 1
    return dict(tau=tau, v=v, cav_tau=r["cav_tau"], cav_v=r["cav_v"], sweeps=it, converged=stop,
                log_Z_tilde=log_Z_tilde(r["log_Z_hat"], tau, v, r["cav_tau"], r["cav_v"]))


def final(K, dKs, e):
    """`_ep_marginal` and `_inference` (:363-395) through the Laplace restatement with W = tau, b = v"""
    tau, v = e["tau"], e["v"]
    alpha, mu, logdet = LP.newton(K, tau, v)
    lml = 0.5 * (-tau.size * np.log(2 * np.pi) - logdet + np.dot(v, mu)) + e["log_Z_tilde"]
    _, _, Wi = LP.finish(K, tau)
    G = LP.dL_dK_sym(K, alpha, np.zeros_like(alpha), Wi)
    return dict(lml=lml, log_Z_tilde=e["log_Z_tilde"], tau_tilde=tau, v_tilde=v, cav_tau=e["cav_tau"], cav_v=e["cav_v"],
                alpha=alpha[:, None], Wi=Wi, dL_dK=G, dtheta=np.array([np.sum(G * dK) for dK in dKs]), sweeps=e["sweeps"])


def inference(specs, X, Y, **kw):
    K, dKs = LP.expr(specs, X)
    return final(K, dKs, run(K, Y, **kw))


def predict(specs, X, r, Xs, full_cov=False):
    return LP.predict(specs, X, {"Ki_fhat": r["alpha"], "woodbury_inv": r["Wi"]}, Xs, full_cov)


def figures(g, got):
    """relative differences against a fixture, scalars as |a - b| / |b|"""
    fig = {q: (abs(got[q] - g[q]) / abs(g[q]) if q in ("lml", "log_Z_tilde") else LP.rel(got[q], g[q])) for q in got if q in STANDING}
    print({q: "%.1e (tol %.1e)" % (fig[q], g["tol"][q]) for q in fig})
    return fig
