"""Restatement of EPDTC (reference `expectation_propagation.py:145-185` posteriorParamsDTC, `:436-578` EPDTC) in float64 and in
long double (`dt`), the way the device path splits it (include/mi355gp_epdtc.h), shared by the CPU and the GPU tests:

  recompute(Kmm, Kmn, tau, v)       posteriorParamsDTC._recompute (:174-185): mu and diag(Sigma) from the factor of LLT
  ref_sweep(...)                    the reference's sequential sweep, literally: after every site LLT gets its rank-one term, is
                                    factored again and solved against all of Kmn (:149-156)
  blocked_sweep(..., b)             the same sweep in blocks of b sites from P = LLT^-1 and gamma = P Kmn v (gpy_amd/csrc/epdtc.hip)
  parallel_sweep(...)               parallel_updates=True: every site sees the same q(f)
  run(...)                          `expectation_propagation` (:494-512): sweep, recompute, stop test, warm start
  log_Z_tilde(...)                  (:514-520)
  final(...)                        the VarDTC evaluation of the converged sites through tests/sparse_ld.py with no jitter on Kmm

Kernels and the column-oriented factorisation come from tests/kern_ld.py, the probit moments from tests/laplace_ld.py."""
import os

import numpy as np

import kern_ld as KL
import laplace_ld as LL
import sparse_ld as SL

LD = KL.LD
EPS = np.finfo(np.float64).eps
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "epdtc")
SWEEP_KEYS = ("tau", "v", "cav_tau", "cav_v", "log_Z_hat", "mu_hat", "sigma2_hat")


def _a(x, dt):
    return np.asarray(x, dtype=dt)


def covariances(specs, X, Z, dt=LD):
    """(Kmm without jitter, Kmn)"""
    return _a(KL.K(specs, Z, None, dt), dt), _a(KL.K(specs, Z, X, dt), dt)


def _llt(Kmm, Kmn, tau):
    return Kmm + KL.matmul(Kmn * tau[None, :], Kmn.T.copy())


def recompute(Kmm, Kmn, tau, v, dt=LD):
    """(mu, Sigma_diag): V = L^-1 Kmn, Sigma = V^T V, mu = Sigma v (:174-185)"""
    Kmm, Kmn, tau, v = _a(Kmm, dt), _a(Kmn, dt), _a(tau, dt), _a(v, dt)
    V = KL.solve_lower(KL.cholesky(_llt(Kmm, Kmn, tau), 1 << 20), Kmn)
    return np.sum(V * (np.sum(V * v[None, :], axis=1))[:, None], axis=0), np.sum(V * V, axis=0)


def site(sign, S, m, tau_i, v_i, eta, delta, dt):
    """cavity (:27-29), moments (bernoulli.py:73-79), site update with tau clipped at eps64 (:52-68)"""
    ct = 1 / S - eta * tau_i
    cv = m / S - eta * v_i
    lz, mu_hat, s2_hat, _ = LL.moments(sign, ct, cv, dt)
    lz, mu_hat, s2_hat = lz[()], mu_hat[()], s2_hat[()]
    dtau = delta / eta * (1 / s2_hat - 1 / S)
    dv = delta / eta * (mu_hat / s2_hat - m / S)
    t = tau_i + dtau
    if t < dt(EPS):
        t = dt(EPS)
        dtau = t - tau_i
    return dict(tau=t, v=v_i + dv, cav_tau=ct, cav_v=cv, log_Z_hat=lz, mu_hat=mu_hat, sigma2_hat=s2_hat), dtau, dv


def _begin(order, sign, eta, delta, tau, v, dt):
    n = len(order)
    out = {k: np.zeros(n, dtype=dt) for k in SWEEP_KEYS}
    out["tau"], out["v"] = np.array(tau, dtype=dt), np.array(v, dtype=dt)
    return [int(i) for i in order], _a(sign, dt), dt(eta), dt(delta), out


def ref_sweep(Kmm, Kmn, order, sign, eta, delta, tau, v, first, dt=LD):
    """The reference's sweep, refactoring everything per site.  first: every Sigma_ii starts with 1e-8 added (:538, :547); the
    first rank-one update recomputes them all, so only the first site visited sees it."""
    Kmm, Kmn = _a(Kmm, dt), _a(Kmn, dt)
    order, sign, eta, delta, out = _begin(order, sign, eta, delta, tau, v, dt)
    LLT = _llt(Kmm, Kmn, out["tau"])
    mu, Sd = recompute(Kmm, Kmn, out["tau"], out["v"], dt)
    if first:
        Sd = Sd + dt(1e-8)
    for i in order:
        r, dtau, dv = site(sign[i], Sd[i], mu[i], out["tau"][i], out["v"][i], eta, delta, dt)
        for k in SWEEP_KEYS:
            out[k][i] = r[k]
        LLT = LLT + dtau * (Kmn[:, i][:, None] * Kmn[:, i][None, :])
        V = KL.solve_lower(KL.cholesky(LLT, 1 << 20), Kmn)
        Sd = np.maximum(np.sum(V * V, axis=0), dt(EPS))
        mu = mu + (dv - dtau * mu[i]) * np.sum(V * V[:, i][:, None], axis=0)
    return out


def blocked_sweep(Kmm, Kmn, order, sign, eta, delta, tau, v, first, b, dt=LD):
    """The sweep of gpy_amd/csrc/epdtc.hip: blocks of b sites from P = LLT^-1 and gamma = P Kmn v."""
    Kmm, Kmn = _a(Kmm, dt), _a(Kmn, dt)
    order, sign, eta, delta, out = _begin(order, sign, eta, delta, tau, v, dt)
    M = Kmm.shape[0]
    L = KL.cholesky(_llt(Kmm, Kmn, out["tau"]), 1 << 20)
    Li = KL.solve_lower(L, np.eye(M, dtype=dt))
    P = KL.matmul(Li.T.copy(), Li)
    gam = KL.matmul(P, KL.matmul(Kmn, out["v"][:, None]))[:, 0]
    for s0 in range(0, len(order), b):
        idx = order[s0:s0 + b]
        nb = len(idx)
        Kb = Kmn[:, idx]
        A0 = KL.matmul(P, Kb)
        G0 = KL.matmul(Kb.T.copy(), A0)
        G0 = (G0 + G0.T) / 2
        G, h = G0.copy(), KL.matmul(Kb.T.copy(), gam[:, None])[:, 0]
        R, gc = np.zeros((nb, nb), dtype=dt), np.zeros(nb, dtype=dt)
        for j, i in enumerate(idx):
            S, m = max(G[j, j], dt(EPS)), h[j]
            if first and s0 + j == 0:
                S = S + dt(1e-8)
            r, dtau, dv = site(sign[i], S, m, out["tau"][i], out["v"][i], eta, delta, dt)
            for k in SWEEP_KEYS:
                out[k][i] = r[k]
            c = dtau / (1 + dtau * G[j, j])
            kap = dv - c * (m + dv * G[j, j])
            rj = -np.sum(R * G0[:, j][None, :], axis=1)
            rj[j] += 1
            g = G[:, j].copy()
            R = R + c * (rj[:, None] * rj[None, :])
            gc = gc + kap * rj
            G = G - c * (g[:, None] * g[None, :])
            h = h + kap * g
        P = P - KL.matmul(A0, KL.matmul(R, A0.T.copy()))
        gam = gam + KL.matmul(A0, gc[:, None])[:, 0]
    return out


def parallel_sweep(mu, Sd, sign, eta, delta, tau, v, dt=LD):
    mu, Sd, sign, tau, v = (_a(x, dt) for x in (mu, Sd, sign, tau, v))
    ct = 1 / Sd - eta * tau
    cv = mu / Sd - eta * v
    lz, mu_hat, s2_hat, _ = LL.moments(sign, ct, cv, dt)
    dtau = delta / eta * (1 / s2_hat - 1 / Sd)
    dv = delta / eta * (mu_hat / s2_hat - mu / Sd)
    return dict(tau=np.maximum(tau + dtau, dt(EPS)), v=v + dv, cav_tau=ct, cav_v=cv, log_Z_hat=lz, mu_hat=mu_hat, sigma2_hat=s2_hat)


def log_Z_tilde(lz, tau, v, ct, cv):
    """(:514-520)"""
    mu_tilde, mu_cav, s2 = v / tau, cv / ct, 1 / ct + 1 / tau
    return np.sum(lz + np.log(2 * np.pi) / 2 + np.log(s2) / 2 + ((mu_cav - mu_tilde) ** 2) / s2 / 2)


def run(Kmm, Kmn, sign, orders=None, parallel=False, eta=1.0, delta=1.0, epsilon=1e-6, max_iters=100, tau0=None, v0=None,
        sweep=ref_sweep, dt=np.float64, **kw):
    """`expectation_propagation` (:494-512) from a cold (tau0 is None) or a warm start: dict(tau, v, cav_tau, cav_v, log_Z_hat,
    log_Z_tilde, sweeps, converged)"""
    n = Kmn.shape[1]
    tau, v = (np.zeros(n, dtype=dt), np.zeros(n, dtype=dt)) if tau0 is None else (_a(tau0, dt), _a(v0, dt))
    stop, it, old, r = False, 0, None, None
    if parallel:
        mu, Sd = recompute(Kmm, Kmn, tau, v, dt)
        Sd = Sd + dt(1e-8)
    while not stop and it < max_iters:
        if parallel:
            r = parallel_sweep(mu, Sd, sign, eta, delta, tau, v, dt)
        else:
            r = sweep(Kmm, Kmn, orders[it], sign, eta, delta, tau, v, it == 0, dt=dt, **kw)
        tau, v = r["tau"], r["v"]
        if parallel:
            mu, Sd = recompute(Kmm, Kmn, tau, v, dt)
            Sd = np.maximum(Sd, dt(EPS))
        if it > 0:
            stop = bool(np.mean(np.square(tau - old[0])) < epsilon and np.mean(np.square(v - old[1])) < epsilon)
        old = (tau.copy(), v.copy())
        it += 1
    return dict(r, sweeps=it, converged=stop, log_Z_tilde=log_Z_tilde(r["log_Z_hat"], tau, v, r["cav_tau"], r["cav_v"]))


def final(specs, X, Z, tau, v, lzt, dt=LD):
    """`EPDTC.inference` after EP (:482-492): VarDTC with targets v / tau, precisions tau and Lm = jitchol(K(Z)) passed in, so
    var_dtc.py:93 adds no jitter: tests/sparse_ld.py's evaluation with its jitter constant set to zero for the call"""
    tau, v = _a(tau, dt), _a(v, dt)
    keep = SL.JITTER
    SL.JITTER = 0.0
    try:
        r = SL.vardtc(specs, X, Z, np.asarray(v / tau, dtype=np.float64)[:, None], np.asarray(1 / tau, dtype=np.float64), dt=dt,
                      max_n=1 << 20)
    finally:
        SL.JITTER = keep
    r["lml"] = r["lml"] + lzt
    return r


def rel(got, ref):
    """max |got - ref| / max |ref|"""
    got, ref = np.asarray(got, dtype=LD), np.asarray(ref, dtype=LD)
    return float(np.max(np.abs(got - ref)) / max(float(np.max(np.abs(ref))), 1e-300))


# ---- the shapes the device sweep is held to (tests/test_gpu_epdtc.py) and the float64 restatement is measured at ----------------
B = 64                     # the device's block (EPB of epdtc.hip)
# (name, N, M, D): N on both sides of one and two blocks with M and D small; every tile / padding edge of M and every group edge
# of D once with the others small
SHAPES = [("n1", 1, 5, 2), ("n63", B - 1, 5, 2), ("n64", B, 5, 2), ("n65", B + 1, 5, 2), ("n129", 2 * B + 1, 6, 2),
          ("m1", 20, 1, 1), ("m63", 40, 63, 2), ("m65", 70, 65, 2), ("m129", 30, 129, 3), ("m257", 12, 257, 3),
          ("d17", 66, 9, 17), ("d33", 30, 7, 33)]


def make_case(name):
    """Inputs of a shape case: an RBF ARD kernel, Z on a jittered grid (sparse_ld's recipe: cond(Kmm) stays small), labels from a
    smooth function of X, the sites after one parallel sweep (tau of order one, so that every site is informative), an order."""
    N, M, D = next(s[1:] for s in SHAPES if s[0] == name)
    rng = np.random.default_rng(sum(map(ord, name)) * 7919 + 1)
    nd = min(D, 3 if M >= 27 else 2 if M >= 4 else 1)
    side = SL._grid_side(M, nd)
    grid = np.stack(np.meshgrid(*[np.arange(side)] * nd, indexing="ij"), -1).reshape(-1, nd)[:M] / float(side)
    Z = rng.uniform(0.2, 0.8, (M, D))
    Z[:, :nd] = grid + rng.uniform(-0.1, 0.1, (M, nd)) / side + 0.5 / side
    ls = np.full(D, 3.0)
    ls[:nd] = 0.75 / side
    X = rng.uniform(0, 1, (N, D))
    specs = [("rbf", 1, np.concatenate([[1.3], ls]), np.arange(D), 0)]
    sign = np.where(np.sin(5 * X[:, 0]) + 0.3 * rng.standard_normal(N) > 0, 1.0, -1.0)
    Kmm, Kmn = covariances(specs, X, Z, np.float64)
    mu, Sd = recompute(Kmm, Kmn, np.zeros(N), np.zeros(N), np.float64)
    p = parallel_sweep(mu, Sd + 1e-8, sign, 1.0, 1.0, np.zeros(N), np.zeros(N), np.float64)
    return dict(name=name, N=N, M=M, D=D, specs=specs, X=X, Z=Z, sign=sign, tau=np.asarray(p["tau"], np.float64),
                v=np.asarray(p["v"], np.float64), order=rng.permutation(N), eta=0.9, delta=0.8)


_MEMO = {}


def reference(name):
    """(case, long-double results): recompute of the case's sites, then one refactoring sweep from them"""
    if name not in _MEMO:
        c = make_case(name)
        Kmm, Kmn = covariances(c["specs"], c["X"], c["Z"], LD)
        mu, Sd = recompute(Kmm, Kmn, c["tau"], c["v"], LD)
        sw = ref_sweep(Kmm, Kmn, c["order"], c["sign"], c["eta"], c["delta"], c["tau"], c["v"], True, LD)
        _MEMO[name] = (c, dict(sw, mu=mu, Sigma_diag=Sd))
    return _MEMO[name]


# ---- the reference fixtures (tests/golden/epdtc, written by tools/make_golden_epdtc.py) -----------------------------------------
FIXTURES = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz") and f != "toy_1d_optimize.npz") if os.path.isdir(GOLDEN) else []
# the sparse path's tolerances against the reference's own evaluation (tests/test_gpu_sparse.py): log marginal 1e-9, gradients,
# Woodbury vector and predictive mean 1e-6, predictive variance 1e-5
DOWNSTREAM = {"lml": 1e-9, "log_Z_tilde": 1e-9, "dtheta": 1e-6, "dZ": 1e-6, "woodbury_vector": 1e-6, "pred_mu": 1e-6, "pred_var": 1e-5}


def _parse_specs(text):
    import json
    return [(s[0], int(s[1]), np.array(s[2], dtype=np.float64), np.array(s[3], dtype=np.int32), int(s[4])) for s in json.loads(str(text))]


def load(name):
    fx = dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))
    fx["name"] = name
    fx["specs"] = _parse_specs(fx["specs"])
    if "warm_specs" in fx:
        fx["warm_specs"] = _parse_specs(fx["warm_specs"])
    for k in ("sweeps", "parallel_updates", "eta", "delta", "epsilon", "clamped"):
        fx[k] = fx[k].item()
    return fx


def restate_fixture(fx, dt=np.float64, sweep=ref_sweep, **kw):
    """a fixture's whole trajectory with its recorded orders (for the warm case: the first run at the first parameters too):
    dict(tau_tilde, v_tilde, cav_tau, cav_v, log_Z_tilde, sweeps, lml, dtheta, dZ, woodbury_vector, pred_mu, pred_var)"""
    sign = np.where(fx["Y"][:, 0] == 1, 1.0, -1.0)
    opts = dict(parallel=fx["parallel_updates"], eta=fx["eta"], delta=fx["delta"], epsilon=fx["epsilon"], sweep=sweep, dt=dt, **kw)
    tau0 = v0 = None
    if "warm_specs" in fx:
        Kmm, Kmn = covariances(fx["warm_specs"], fx["X"], fx["Z"], dt)
        w = run(Kmm, Kmn, sign, orders=list(fx["warm_orders"]), **opts)
        tau0, v0 = w["tau"], w["v"]
    Kmm, Kmn = covariances(fx["specs"], fx["X"], fx["Z"], dt)
    e = run(Kmm, Kmn, sign, orders=list(fx["orders"]), tau0=tau0, v0=v0, **opts)
    r = final(fx["specs"], fx["X"], fx["Z"], e["tau"], e["v"], e["log_Z_tilde"], dt)
    mu, var = SL.predict(fx["specs"], fx["Z"], fx["Xs"], r, dt=dt)
    return dict(r, tau_tilde=e["tau"], v_tilde=e["v"], cav_tau=e["cav_tau"], cav_v=e["cav_v"], log_Z_tilde=e["log_Z_tilde"],
                sweeps=e["sweeps"], pred_mu=mu, pred_var=var)


class RestatementContext(object):
    """Stands for `_lib.SparseContext` in the CPU tests: the EPDTC calls answered by this restatement in fp64 (the sweep by the
    blocked one at the device's block), and a log of the calls.  Part lists arrive as the package sends them."""
    sharded = False
    FETCH_DLDKMM, FETCH_WOODBURY_INV, FETCH_LM, FETCH_KMM = 0, 1, 2, 3
    fail_begin = 0               # epdtc_begin answers this info while the jitter is zero

    def __init__(self, device=0):
        self.log, self.jitters = [], []
        self.res = None

    def set_data(self, X, Y):
        self.X, self.Y = np.array(X, dtype=np.float64), np.array(Y, dtype=np.float64)
        self.N, self.D = self.X.shape
        self.log.append(("set_data", self.X.shape, self.Y.shape))

    def _specs(self, specs):
        return [(s[0], int(bool(s[1])), np.asarray(s[2], np.float64), np.arange(self.D) if s[3] is None else np.asarray(s[3]),
                 int(s[4]) if len(s) > 4 else 0) for s in specs]

    def epdtc_begin(self, specs, Z, jitter=0.0):
        self.log.append(("epdtc_begin", np.shape(Z), float(jitter)))
        self.jitters.append(float(jitter))
        if self.fail_begin and jitter == 0.0:
            return self.fail_begin, {}
        self.specs, self.Z = self._specs(specs), np.array(Z, dtype=np.float64)
        self.Kmm, self.Kmn = covariances(self.specs, self.X, self.Z, np.float64)
        self.Kmm = self.Kmm + jitter * np.eye(self.Z.shape[0])
        return 0, {}

    def epdtc_recompute(self, tau, v, want_ms=False):
        self.log.append(("epdtc_recompute",))
        mu, sd = recompute(self.Kmm, self.Kmn, tau, v, np.float64)
        return 0, mu, sd

    def epdtc_sweep(self, order, ysign, tau, v, eta=1.0, delta=1.0, first=False, want_ms=False):
        self.log.append(("epdtc_sweep", bool(first), np.array(order)))
        return blocked_sweep(self.Kmm, self.Kmn, order, ysign, eta, delta, tau, v, first, B, np.float64)

    def epdtc_inference(self, specs, Z, tau, v, jitter=0.0, want_stage_ms=False):
        self.log.append(("epdtc_inference", np.shape(Z), float(jitter)))
        assert jitter == 0.0, "the restatement evaluates without jitter"
        r = final(self._specs(specs), self.X, Z, tau, v, 0.0, np.float64)
        self.res, self.M = r, np.shape(Z)[0]
        return 0, dict(lml=float(r["lml"]), dL_dR=r["dnoise"], dtheta=r["dtheta"], dZ=r["dZ"], woodbury_vector=r["woodbury_vector"])

    def predict(self, specs, Xnew, full_cov=False, want_var=True):
        self.log.append(("predict", np.shape(Xnew), bool(full_cov)))
        return SL.predict(self._specs(specs), self.Z, np.asarray(Xnew, np.float64), self.res, full_cov, np.float64)

    def fetch(self, which):
        return {0: self.res["dL_dKmm"], 1: self.res["woodbury_inv"], 2: self.res["Lm"], 3: self.res["Kmm"]}[which]

    def fetch_dL_dKnm(self, row0, nrows):
        return self.res["dL_dKnm"][row0:row0 + nrows]


# The float64 restatement's distance from long double, worst over SHAPES and over both sweeps (refactoring and blocked at B),
# relative to max |value| (measured by tests/test_oracle_epdtc.py, which holds the restatement to these figures), and the
# device's bound: ten times that.  tau is apart from the rest: 1 / sigma2_hat - 1 / Sigma_ii cancels (5.6e-12 at M = 257, N = 12).
FP64_DISTANCE = {"tau": 5.7e-12, "v": 9.5e-15, "cav_tau": 3.2e-15, "cav_v": 1.4e-14, "log_Z_hat": 3.5e-15, "mu_hat": 5.2e-15,
                 "sigma2_hat": 4.8e-15, "mu": 7.2e-16, "Sigma_diag": 1.5e-15}      # (each measured figure rounded up)
DEVICE_BOUND = {k: 10.0 * v for k, v in FP64_DISTANCE.items()}
