"""Long-double (x86 80-bit) restatement of the Laplace / EP device session on the exact context (C-ABI mi355gp_laplace_* and
mi355gp_ep_*, csrc/laplace.hip with its session kernels and csrc/ep.hip), one function per device call,
and the shape sweep that tests/test_oracle_laplace_ld.py (CPU) and tests/test_gpu_laplace_shapes.py (GPU) share.  Written from
the formulas of the reference as laplace.hip and ep.hip cite them:

    newton(K, W, b)                               laplace.py:184-199, 333-334    a, K a, log det B
    finish(K, W)                                  laplace.py:333-351             diag(Ki_W_i), log det B, K_Wi_i = W^1/2 B^-1 W^1/2
    gradients(specs, X, K, K_Wi_i, Ki_f, dL_dfhat)  laplace.py:257-272           u, the symmetrised dL_dK, dtheta and its cond
    implicit(K, K_Wi_i, dL_dfhat)                 laplace.py:293-295             s = K (I - K_Wi_i K) dL_dfhat
    predict(specs, X, Xs, wv, W, L_B, full_cov)   posterior.py:198-262           mu, var or cov
    recompute(K, tau, v, add_diag, want_sigma)    expectation_propagation.py:129-143   mu, diag Sigma, log det B, Sigma
    sweep(Sigma, mu, order, ysign, eta, delta, tau, v)   expectation_propagation.py:27-29, 52-68, 101-105, 330-351,
                                                  bernoulli.py:73-79             one sequential pass over the sites

with B = I + W^1/2 K W^1/2 (W = tau for EP).  Everything kernel-shaped comes from tests/kern_ld.py: K, Kdiag, dtheta with its
per-entry cond, the column-oriented Cholesky, the triangular solves, the part format and the Coregionalize chain rule.  Every
function takes `dt`, np.longdouble or np.float64: the same formulas in double precision are the floor e64 that the judge
(sparse_ld.rel_err, sparse_ld.bound) measures a bound from -- never the device's figure.  No product goes through `@`.

log Phi and phi / Phi of the probit moments: in long double from mpmath at 40 digits, rounded once; in fp64 from SciPy
(log_ndtr, erfcx), as tests/ep_np.py.

Cost: N x N x N work is formed for N <= 513 only (a long-double Cholesky takes 0.5 s, a triangular solve of N columns 1.7 s
and a Gram product 2.4 s at N = 641).  N = 1025 restates what a Cholesky, one triangular solve per W and vector work give:
newton, diag(Ki_W_i) and log det B of finish, implicit, and recompute without Sigma.

Inputs (`make_case`): X and the labels from laplace_np.two_class, row 1 of X equal to row 0 (N >= 2); f = 0.3 sin(x_0), W and b
from the package's Bernoulli at f unless the family sets W; Ki_f and dL_dfhat seeded random vectors (the judged map is the
device call, not the mode search); EP sites tau = 0.05 + 0.3 / (1 + x_0^2), v = y tau (0.5 + 0.2 cos x_1), eta = 0.9,
delta = 0.8, a seeded permutation.  Every case must keep cond2(B) <= 1e4 (tests/test_oracle_laplace_ld.py)."""
import mpmath
import numpy as np
from scipy import special

import kern_ld as KL
import laplace_np as LP
import sparse_ld as SL
from gpy_amd.likelihoods import Bernoulli

LD = KL.LD
EPS64 = KL.EPS64
ETA, DELTA = 0.9, 0.8
FULL_MAX = 513                     # the largest N at which N x N x N products are formed
CHOL_MAX = 1025
POINTS_M = (1, 127, 128, 129, 257)


def _a(x, dt):
    return np.asarray(x, dtype=dt)


def _mv(A, x):
    return np.sum(A * x[None, :], axis=1)


def _gram(V):
    """V^T V, the lower half formed and mirrored: symmetric to the bit"""
    n = V.shape[1]
    out = np.zeros((n, n), dtype=V.dtype)
    for j in range(n):
        out[j:, j] = np.sum(V[:, j:] * V[:, j][:, None], axis=0)
        out[j, j:] = out[j:, j]
    return out


def _gram_lower(Li):
    """Li^T Li for a lower-triangular Li: row k contributes to the entries (i, j) with i, j <= k only"""
    n = Li.shape[0]
    out = np.zeros((n, n), dtype=Li.dtype)
    for j in range(n):
        out[:j + 1, j] = np.sum(Li[j:, :j + 1] * Li[j:, j][:, None], axis=0)
        out[j, :j + 1] = out[:j + 1, j]
    return out


def factor(K, W, dt=LD):
    """(W^1/2, the lower Cholesky factor of B = I + W^1/2 K W^1/2, B)  (laplace.py:333-334)"""
    sw = np.sqrt(_a(W, dt))
    B = sw[:, None] * _a(K, dt) * sw[None, :]
    B[np.arange(B.shape[0]), np.arange(B.shape[0])] += dt(1)
    return sw, KL.cholesky(B, CHOL_MAX), B


def _Binv(L, r):
    return KL.solve_upper_T(L, KL.solve_lower(L, r[:, None]))[:, 0]


def _logdet(L):
    return 2 * np.sum(np.log(np.diag(L)))


def newton(K, W, b, dt=LD, fac=None):
    """a = b - W^1/2 B^-1 W^1/2 K b, K a, log det B  (laplace.py:184-199)"""
    K, b = _a(K, dt), _a(b, dt)
    sw, L, _ = fac or factor(K, W, dt)
    a = b - sw * _Binv(L, sw * _mv(K, b))
    return a, _mv(K, a), _logdet(L)


def finish(K, W, dt=LD, fac=None, want_matrix=True):
    """diag(Ki_W_i) = Kdiag - colsumsq(L_B^-1 W^1/2 K)  (laplace.py:347-348), log det B, K_Wi_i = W^1/2 B^-1 W^1/2 (:338;
    None without `want_matrix`)"""
    K = _a(K, dt)
    sw, L, _ = fac or factor(K, W, dt)
    C = KL.solve_lower(L, sw[:, None] * K)
    d = np.diag(K) - np.sum(C * C, axis=0)
    if not want_matrix:
        return d, _logdet(L), None
    Li = KL.solve_lower(L, np.eye(K.shape[0], dtype=dt))
    return d, _logdet(L), sw[:, None] * _gram_lower(Li) * sw[None, :]


def _u(K, s, K_Wi_i=None, fac=None):
    """u = (I - K_Wi_i K) s, through the matrix or through the factor"""
    Ks = _mv(K, s)
    if K_Wi_i is not None:
        return s - _mv(K_Wi_i, Ks)
    sw, L, _ = fac
    return s - sw * _Binv(L, sw * Ks)


def gradients(specs, X, K, K_Wi_i, Ki_f, dL_dfhat, dt=LD):
    """u, dL_dK = (a a^T - K_Wi_i) / 2 + (a u^T + u a^T) / 2 with a = Ki_f (the symmetric part of laplace.py:257-270), and
    (dtheta, its per-entry cond) in link order (:272)"""
    K, KWi, a, s = _a(K, dt), _a(K_Wi_i, dt), _a(Ki_f, dt), _a(dL_dfhat, dt)
    u = _u(K, s, KWi)
    au = a[:, None] * u[None, :]
    G = (a[:, None] * a[None, :] - KWi) / 2 + (au + au.T) / 2
    val, cond = KL.dtheta(specs, G, X, None, dt)
    return u, G, val, cond


def implicit(K, K_Wi_i, dL_dfhat, dt=LD, fac=None):
    """s = K (dL_dfhat - K_Wi_i K dL_dfhat)  (laplace.py:293-295: dL_dfhat^T (I - K K_Wi_i) K g = s^T g)"""
    K = _a(K, dt)
    return _mv(K, _u(K, _a(dL_dfhat, dt), None if K_Wi_i is None else _a(K_Wi_i, dt), fac))


def predict(specs, X, Xs, wv, W, L_B, full_cov=False, dt=LD):
    """Posterior._raw_predict with woodbury_vector wv and woodbury_inv K_Wi_i (posterior.py:198-262):
    mu = Kx^T wv (M x 1), var = K** - colsumsq(L_B^-1 W^1/2 Kx) (M x 1) or the full covariance"""
    Kx = KL.K(specs, X, Xs, dt) + np.zeros((np.shape(X)[0], np.shape(Xs)[0]), dtype=dt)
    mu = np.sum(Kx * _a(wv, dt)[:, None], axis=0)[:, None]
    T = KL.solve_lower(_a(L_B, dt), np.sqrt(_a(W, dt))[:, None] * Kx)
    if full_cov:
        return mu, KL.K(specs, Xs, None, dt) - _gram(T)
    return mu, (KL.Kdiag(specs, Xs, dt) - np.sum(T * T, axis=0))[:, None]


def recompute(K, tau, v, add_diag=0.0, want_sigma=True, dt=LD, fac=None):
    """posteriorParams._recompute for a zero prior mean (expectation_propagation.py:129-143):
    (mu = K alpha, diag(Sigma) + add_diag, log det B, Sigma + add_diag I or None), alpha = v - S^1/2 B^-1 S^1/2 K v"""
    K, v = _a(K, dt), _a(v, dt)
    sw, L, _ = fac or factor(K, tau, dt)
    alpha = v - sw * _Binv(L, sw * _mv(K, v))
    mu = _mv(K, alpha)
    V = KL.solve_lower(L, sw[:, None] * K)
    if not want_sigma:
        return mu, np.diag(K) - np.sum(V * V, axis=0) + dt(add_diag), _logdet(L), None
    Sigma = K - _gram(V)
    Sigma[np.arange(K.shape[0]), np.arange(K.shape[0])] += dt(add_diag)
    return mu, np.diag(Sigma).copy(), _logdet(L), Sigma


# ---- the probit moments -----------------------------------------------------------------------------------------------------
def _mpf(x):
    """a long double as an mpf, exactly (two doubles)"""
    hi = float(x)
    return mpmath.mpf(hi) + mpmath.mpf(float(LD(x) - LD(hi)))


def _ld(x):
    """an mpf rounded to long double"""
    return LD(mpmath.nstr(x, 30, min_fixed=0, max_fixed=0))


def probit(z, dt=LD):
    """(log Phi(z), phi(z) / Phi(z)) of one z"""
    if dt is np.float64:
        z = float(z)
        lz = special.log_ndtr(z)
        r = (np.sqrt(2.0 / np.pi) / special.erfcx(-z / np.sqrt(2.0)) if z < 0
             else np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi) / special.ndtr(z))
        return np.float64(lz), np.float64(r)
    with mpmath.workdps(40):
        zz = _mpf(z)
        if zz < 0:
            Phi = mpmath.erfc(-zz / mpmath.sqrt(2)) / 2
            lz = mpmath.log(Phi)
        else:
            q = -mpmath.erfc(zz / mpmath.sqrt(2)) / 2               # Phi - 1
            Phi = 1 + q
            lz = mpmath.log1p(q)
        return _ld(lz), _ld(mpmath.npdf(zz) / Phi)


def moments(sign, ct, cv, dt=LD):
    """(log Z_hat, mu_hat, sigma2_hat, z) of the probit site against the cavity N(cv / ct, 1 / ct) (bernoulli.py:73-79); arrays
    or scalars"""
    sign, ct, cv = np.broadcast_arrays(_a(sign, dt), _a(ct, dt), _a(cv, dt))
    q = ct * ct + ct
    rq = np.sqrt(q)
    z = sign * cv / rq
    lz, r = np.empty(z.shape, dtype=dt), np.empty(z.shape, dtype=dt)
    for i in np.ndindex(z.shape):
        lz[i], r[i] = probit(z[i], dt)
    return lz, cv / ct + sign * r / rq, 1 / ct - (r / q) * (z + r), z


def sweep(Sigma, mu, order, ysign, eta, delta, tau, v, dt=LD):
    """One sequential pass of _local_updates (expectation_propagation.py:330-351) on copies: cavity (:52-68), moment matching,
    site update with the clamp of tau at eps64 (:27-29), rank-one update of Sigma and mu (:101-105).
    dict(tau, v, cav_tau, cav_v, log_Z_hat, mu, Sigma_diag, z, clamped)"""
    S, mu, tau, v, ys = np.array(Sigma, dtype=dt), np.array(mu, dtype=dt), np.array(tau, dtype=dt), np.array(v, dtype=dt), _a(ysign, dt)
    n = mu.size
    eta, delta, eps = dt(eta), dt(delta), dt(EPS64)
    ct, cv, lz, zs = (np.zeros(n, dtype=dt) for _ in range(4))
    clamped = []
    for i in [int(k) for k in order]:
        si = S[:, i].copy()
        sii, mui = si[i], mu[i]
        ct[i] = 1 / sii - eta * tau[i]
        cv[i] = mui / sii - eta * v[i]
        l, mu_hat, s2_hat, z = moments(ys[i], ct[i], cv[i], dt)
        lz[i], zs[i] = l, z
        dtau = delta / eta * (1 / s2_hat - 1 / sii)
        dv = delta / eta * (mu_hat / s2_hat - mui / sii)
        prev = tau[i]
        t = prev + dtau
        if t < eps:
            t = eps
            dtau = t - prev
            clamped.append(i)
        tau[i] = t
        v[i] = v[i] + dv
        ci = dtau / (1 + dtau * sii)
        mu = mu - (ci * (mui + sii * dv) - dv) * si
        if ci != 0:
            S = S - ci * (si[:, None] * si[None, :])
    return dict(tau=tau, v=v, cav_tau=ct, cav_v=cv, log_Z_hat=lz, mu=mu, Sigma_diag=np.diag(S).copy(), z=zs, clamped=clamped)


# ---- the judge ---------------------------------------------------------------------------------------------------------------
LAPLACE_Q = ("a", "Ka", "logdet_newton", "diag", "logdet_finish", "K", "K_Wi_i", "dL_dK", "s")
EP_Q = ("ep_mu", "ep_sd", "ep_logdet", "ep_mu_diag_only", "ep_sd_diag_only", "sw_tau", "sw_v", "sw_cav_tau", "sw_cav_v",
        "sw_log_Z_hat", "sw_mu", "sw_Sigma_diag", "again_mu", "again_sd")
SWEEP_KEYS = ("tau", "v", "cav_tau", "cav_v", "log_Z_hat", "mu", "Sigma_diag")
SYMMETRIC = ("K", "K_Wi_i", "dL_dK")


def pred_q(c):
    return tuple(q + str(M) for M in c["Ms"] for q in ("mu", "var", "cov"))


def judged(c):
    """the quantities one case is judged in (dtheta apart: it has a bound per entry)"""
    out = ()
    if c["laplace"]:
        out += tuple(q for q in LAPLACE_Q if c["full"] or q in ("a", "Ka", "logdet_newton", "diag", "logdet_finish", "s"))
        out += pred_q(c)
    if c["ep"]:
        out += tuple(q for q in EP_Q if (c["full"] or q in ("ep_logdet", "ep_mu_diag_only", "ep_sd_diag_only"))
                     and (judged_again(c) or not q.startswith("again_")))
    return out


def judge(c, got, ref, r64, kappa):
    """err(q) = max |got - q_ld| / max |q_ld| <= max(32 e64(q), 256 eps64 kappa) (sparse_ld.rel_err / bound; kappa = cond2(B)
    of the Laplace W or of the EP tau, by the quantity); every dtheta entry within kern_ld.grad_tol(ref_ld, ref_64, cond).
    Returns ({q: (err, bound)}, [what failed])."""
    figs, bad = {}, []
    for q in judged(c):
        if q not in got:
            bad.append("%s: missing" % q)
            continue
        k = kappa["ep" if q in EP_Q else "laplace"]
        e, b = SL.rel_err(got[q], ref[q]), SL.bound(q, ref, r64, k)
        figs[q] = (e, b)
        if not e <= b:
            bad.append("%s: %.3e > %.3e" % (q, e, b))
    if c["laplace"] and c["full"]:
        if "dtheta" not in got or np.shape(got["dtheta"]) != np.shape(ref["dtheta"]):
            bad.append("dtheta: missing or of another length")
        else:
            tol = KL.grad_tol(ref["dtheta"], r64["dtheta"], ref["dtheta_cond"])
            err = np.abs(_a(got["dtheta"], LD) - ref["dtheta"])
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(tol > 0, err / np.where(tol > 0, tol, 1), np.where(err > 0, np.inf, 0))
            k = int(np.argmax(ratio))
            figs["dtheta"] = (float(ratio[k]), 1.0)                # the worst entry in units of its own bound
            if not KL.grad_ok(got["dtheta"], ref["dtheta"], tol):
                bad.append("dtheta: entry %d off by %.3e, its bound %.3e" % (k, float(err[k]), float(tol[k])))
    return figs, bad


# ---- the shape sweep -------------------------------------------------------------------------------------------------------
FAMILIES = ("n_edge", "weights", "kernels", "points", "stale")
N_EDGE = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 512, 513, 1025)
WEIGHTS = ("zeros", "clip", "tauzero", "cold", "separated")
KERNELS = ("rbf_ard_d32", "rbf_ard_d33", "matern32_ard_subset", "stdperiodic_ard", "ratquad_ard", "linear+bias", "mlp_x_rbf", "poly_o3",
           "rbf_x_coreg_r1", "rbf_x_coreg_r2")
COREG_P = 3


def _case(family, kern, N, variant="", **kw):
    name = "%s-%s-n%d" % (family, kern, N) + ("-" + variant if variant else "")
    c = dict(name=name, family=family, kern=kern, N=N, variant=variant, laplace=True, ep=False, full=N <= FULL_MAX, Ms=(1, 129),
             add_diag=0.0)
    c.update(kw)
    return c


def _cases():
    out = [_case("n_edge", "rbf_ard+bias", N, ep=True) for N in N_EDGE]
    for N in (129, 257):
        out += [_case("weights", "rbf_iso", N, "zeros"), _case("weights", "rbf_iso", N, "clip"),
                _case("weights", "rbf_iso", N, "tauzero", laplace=False, ep=True),
                _case("weights", "rbf_iso", N, "cold", laplace=False, ep=True, add_diag=1e-7),
                _case("weights", "rbf_iso", N, "separated", laplace=False, ep=True)]
    out += [_case("kernels", k, 65 if "coreg" in k else 129) for k in KERNELS]
    out += [_case("points", k, 129, Ms=POINTS_M) for k in ("rbf+bias", "linear+bias")]
    # one context, no fresh context between the steps: set_data at N = 257, set_data at N = 129, set_targets and a product (the
    # product buffer is used), the first part list again, and the same once more after an exact_inference_sum on the context
    out += [_case("stale", "rbf_ard+bias", 257, "step1", ep=True, action="set_data"),
            _case("stale", "rbf_ard+bias", 129, "step2", ep=True, action="set_data"),
            _case("stale", "mlp_x_rbf", 129, "step3a", action="set_targets"),
            _case("stale", "rbf_ard+bias", 129, "step3b", ep=True, action=None),
            _case("stale", "rbf_ard+bias", 129, "step4", ep=True, action="exact_inference_sum")]
    return out


CASES = _cases()
BY_NAME = dict((c["name"], c) for c in CASES)
assert len(BY_NAME) == len(CASES)
NAMES = dict((f, [c["name"] for c in CASES if c["family"] == f]) for f in FAMILIES)
SCHEDULES = ["n_edge-rbf_ard+bias-n%d" % N for N in (129, 257, 513)]


def _specs(kern, rng):
    """(part list, D, the column of the output index or None)"""
    ar = lambda *d: np.array(d, dtype=np.int32)                  # noqa: E731
    allq = lambda D: np.arange(D, dtype=np.int32)                # noqa: E731
    if kern == "rbf_ard+bias":
        return [("rbf", 1, np.array([1.4, 1.1, 0.8, 1.5]), allq(3), 0), ("bias", 0, np.array([0.2]), allq(3), 0)], 3, None
    if kern == "rbf+bias":
        return [("rbf", 0, np.array([1.2, 1.3]), allq(3), 0), ("bias", 0, np.array([0.3]), allq(3), 0)], 3, None
    if kern == "rbf_iso":
        return [("rbf", 0, np.array([1.0, 1.0]), allq(2), 0)], 2, None
    if kern in ("rbf_ard_d32", "rbf_ard_d33"):
        D = int(kern[-2:])
        return [("rbf", 1, KL._theta("rbf", 1, D, rng), allq(D), 0)], D, None
    if kern == "matern32_ard_subset":
        return [("matern32", 1, KL._theta("matern32", 1, 3, rng), ar(0, 2, 3), 0)], 5, None
    if kern == "stdperiodic_ard":
        return [("stdperiodic", 3, KL._theta("stdperiodic", 3, 3, rng), allq(3), 0)], 3, None
    if kern == "ratquad_ard":
        return [("ratquad", 1, KL._theta("ratquad", 1, 3, rng), allq(3), 0)], 3, None
    if kern == "linear+bias":
        return [("linear", 1, KL._theta("linear", 1, 3, rng), allq(3), 0), ("bias", 0, np.array([0.3]), allq(3), 0)], 3, None
    if kern == "mlp_x_rbf":
        return [("mlp", 1, KL._theta("mlp", 1, 2, rng), ar(0, 1), 1), ("rbf", 1, np.array([1.1, 1.4, 0.8]), ar(2, 3), 1)], 4, None
    if kern == "poly_o3":
        return [("poly", 0, KL._theta("poly", 3, 3, rng), allq(3), 0)], 3, None
    assert kern in ("rbf_x_coreg_r1", "rbf_x_coreg_r2"), kern
    rank = int(kern[-1])
    W = rng.uniform(-1.0, 1.0, (COREG_P, rank))
    th = np.concatenate([W.ravel(), rng.uniform(0.3, 0.9, COREG_P)])
    return [("rbf", 1, np.array([1.2, 1.1, 0.9]), ar(0, 1), 1), ("coregionalize", rank * 100 + COREG_P, th, ar(2), 1)], 3, 2


def sites(X, Y):
    """site parameters of the size EP reaches, away from the cold start (`_nontrivial_sites` of tests/test_gpu_ep.py)"""
    tau = 0.05 + 0.3 / (1.0 + X[:, 0] ** 2)
    x1 = X[:, 1] if X.shape[1] > 1 else X[:, 0]
    return tau, np.where(Y[:, 0] == 1, 1.0, -1.0) * tau * (0.5 + 0.2 * np.cos(x1))


def make_case(name):
    """the seeded inputs of one case: dict(specs, X, Y, W, b, Ki_f, dL_dfhat, Xs{M}, tau, v, order, ysign, ...)"""
    c = dict(BY_NAME[name])
    N, kern, variant = c["N"], c["kern"], c["variant"]
    stale = c["family"] == "stale"
    # the members of `stale` from step 2 on share X; step 3a and later share the labels that set_targets brought
    seed = [FAMILIES.index(c["family"]), N] + ([] if stale else [CASES.index(BY_NAME[name])])
    rng = np.random.default_rng(seed)
    specs, D, icol = _specs(kern, np.random.default_rng([7, len(kern), N]))
    Dx = 4 if stale else D                                        # one X for both part lists of the family
    sep = 6.0 if variant == "separated" else 2.0
    X, Y = LP.two_class(N, Dx, int(rng.integers(1 << 30)), sep=sep)
    if stale and variant in ("step3a", "step3b", "step4"):
        Y = 1.0 - Y if N < 3 else np.roll(Y, 3, axis=0).copy()
    if icol is not None:
        X[:, icol] = rng.integers(0, COREG_P, N)
    if any(s[0] in ("linear", "mlp", "poly") for s in specs) and N >= 3 and not stale:
        X[N // 2, :icol] = 0.0                                    # an all-zero input row (kern_ld.make_case)
    if N >= 2:
        X[1] = X[0]
    y = Y[:, 0]
    ysign = np.where(y == 1, 1.0, -1.0)
    f = 0.3 * np.sin(X[:, 0])
    lik = Bernoulli()
    W = -lik.d2logpdf_df2(f, y)
    b = W * f + lik.dlogpdf_df(f, y)
    aux = np.random.default_rng(seed + [99])
    if variant == "zeros":                                        # 10 % exact zeros
        W = W.copy()
        W[aux.permutation(N)[:max(N // 10, 1)]] = 0.0
    elif variant == "clip":                                       # the Student-t clip (laplace.py:319-321) next to large curvature
        W = np.where(aux.random(N) < 0.5, 1e-6, aux.uniform(0.5, 50.0, N))
    tau, v = sites(X, Y)
    if variant == "tauzero":
        zero = aux.permutation(N)[:max(N // 10, 1)]
        tau, v = tau.copy(), v.copy()
        tau[zero] = 0.0
        v[zero] = 0.0
    elif variant == "cold":
        tau, v = np.zeros(N), np.zeros(N)
    elif variant == "separated":
        # strong sites that agree within each class; a few sites carry no information yet (tau = v = 0: their cavity is the
        # posterior of the others, z > 8, and the update of tau falls under eps64: the clamp), a few carry the label of the
        # other class in the sweep (z < -8)
        tau = np.full(N, 0.1)
        v = ysign * tau * 20.0
        pick = aux.permutation(N)
        tau[pick[:8]] = 0.0
        v[pick[:8]] = 0.0
        ysign = ysign.copy()
        ysign[pick[8:14]] *= -1.0
    c.update(specs=specs, dev_specs=KL.cabi_specs(specs), X=np.ascontiguousarray(X), Y=Y, W=W, b=b, f=f,
             Ki_f=aux.standard_normal(N), dL_dfhat=0.3 * aux.standard_normal(N), tau=tau, v=v, ysign=ysign,
             order=aux.permutation(N), eta=ETA, delta=DELTA)
    for M in c["Ms"]:
        Xs = aux.standard_normal((M, X.shape[1]))
        if icol is not None:
            Xs[:, icol] = aux.integers(0, COREG_P, M) if M > 1 else 1
        c["Xs%d" % M] = Xs
    return c


def evaluate(c, dt=LD):
    """every quantity of a case from the restatement in the working type (and "B": the fp64-rounded B matrices by session)"""
    specs, X = c["specs"], c["X"]
    full = c["full"]
    K = KL.K(specs, X, None, dt) + np.zeros((c["N"], c["N"]), dtype=dt)
    out, Bs = {}, {}
    if c["laplace"]:
        fac = factor(K, c["W"], dt)
        Bs["laplace"] = KL.f64(fac[2])
        out["a"], out["Ka"], out["logdet_newton"] = newton(K, c["W"], c["b"], dt, fac)
        out["diag"], out["logdet_finish"], KWi = finish(K, c["W"], dt, fac, want_matrix=full)
        out["s"] = implicit(K, KWi, c["dL_dfhat"], dt, fac)
        if full:
            out["K"], out["K_Wi_i"] = K, KWi
            out["u"], out["dL_dK"], out["dtheta"], out["dtheta_cond"] = gradients(specs, X, K, KWi, c["Ki_f"], c["dL_dfhat"], dt)
        for M in c["Ms"]:
            Xs = c["Xs%d" % M]
            out["mu%d" % M], out["var%d" % M] = predict(specs, X, Xs, c["Ki_f"], c["W"], fac[1], False, dt)
            out["cov%d" % M] = predict(specs, X, Xs, c["Ki_f"], c["W"], fac[1], True, dt)[1]
    if c["ep"]:
        fac = factor(K, c["tau"], dt)
        Bs["ep"] = KL.f64(fac[2])
        out["ep_mu_diag_only"], out["ep_sd_diag_only"], out["ep_logdet"], _ = recompute(K, c["tau"], c["v"], c["add_diag"], False, dt, fac)
        if full:
            out["ep_mu"], out["ep_sd"], _, Sigma = recompute(K, c["tau"], c["v"], c["add_diag"], True, dt, fac)
            r = sweep(Sigma, out["ep_mu"], c["order"], c["ysign"], c["eta"], c["delta"], c["tau"], c["v"], dt)
            for q in SWEEP_KEYS:
                out["sw_" + q] = r[q]
            out["sw_z"], out["sw_clamped"] = r["z"], r["clamped"]
            # a second recompute on the swept sites gives the swept mu and diag(Sigma) again (exact arithmetic, add_diag = 0)
            out["again_mu"], out["again_sd"] = r["mu"], r["Sigma_diag"]
    out["B"] = Bs
    return out


def judged_again(c):
    """whether the second recompute is judged: with add_diag on the diagonal Sigma is no posterior covariance of the sites"""
    return c["add_diag"] == 0.0


_MEMO = {}


def reference(name):
    """(case, long-double reference, fp64 restatement, {session: cond2(B) in fp64}) of a case, computed once per process and not
    to be modified"""
    if name not in _MEMO:
        KL.require_ld()
        c = make_case(name)
        ref, r64 = evaluate(c, LD), evaluate(c, np.float64)
        kappa = dict((k, float(np.linalg.cond(B))) for k, B in r64["B"].items())
        _MEMO[name] = (c, ref, r64, kappa)
    return _MEMO[name]
