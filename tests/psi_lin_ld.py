"""NumPy restatement, in any dtype, of the uncertain-input VarDTC evaluation (reference `var_dtc.py:66-276` with psi
statistics) and of the prediction at uncertain points (`posterior.py:249-269`) for the expressions the `psi_lin_bias` path
covers: ONE input-dependent part P, Linear or RBF, plus Bias parts (b = the sum of their variances) and White parts (w).
`dtype=np.longdouble` gives the reference the device is judged against, `np.float64` the distance e64 of plain fp64.

With q(x_n) = N(mu_n, diag S_n), v_q the Linear variances (0 outside the part's active dimensions):

    Linear:  psi0_n = sum_q v_q (mu_nq^2 + S_nq)      psi1 = (mu v) Z^T      psi2_n = psi1_n psi1_n^T + Z diag(v^2 S_n) Z^T
    Bias:    psi0 = psi1 = b                           psi2_n = b^2
    sum:     psi2_n = psi2_n(P) + b (psi1_n 1^T + 1 psi1_n^T) + b^2         (psi1 of P alone on the right)

Everything is written from these formulas and differentiated by hand; `bound_only` evaluates the bound alone, for central
differences.  The kernel description `k` is a dict: P ("linear" / "rbf"), D, dims (active dimensions of P), ARD,
v (Linear: one variance or one per active dimension) or var / ls (RBF), bias (list), white (list).
"""
import numpy as np

from psi_np import _chol, _tri_inv, psi_grads, psi_stats

LD = np.longdouble


def _a(x, dt):
    return np.asarray(x, dtype=dt)


def lin_v(k, dt):
    """the D-vector of Linear variances, zero outside the active dimensions"""
    v = np.zeros(k["D"], dtype=dt)
    v[np.asarray(k["dims"])] = _a(k["v"], dt).ravel() * np.ones(len(k["dims"]), dtype=dt)
    return v


def rbf_ls(k, dt):
    """the D-vector of RBF lengthscales; a dimension the part does not see gets an infinite one"""
    ls = np.full(k["D"], np.inf, dtype=dt)
    ls[np.asarray(k["dims"])] = _a(k["ls"], dt).ravel() * np.ones(len(k["dims"]), dtype=dt)
    return ls


def part_stats(k, Z, mu, S, dt, want_psi2=True):
    """(psi0, psi1, psi2) of P alone"""
    if k["P"] == "linear":
        v = lin_v(k, dt)
        p1 = (mu * v) @ Z.T
        p2 = p1.T @ p1 + (Z * (v * v * S.sum(0))) @ Z.T if want_psi2 else None
        return ((np.square(mu) + S) * v).sum(1), p1, p2
    d = np.asarray(k["dims"])
    p0, p1, p2 = psi_stats(k["var"], rbf_ls(k, dt)[d], Z[:, d], mu[:, d], S[:, d], None, dt)
    return p0, p1, p2


def part_K(k, Z, dt):
    if k["P"] == "linear":
        return (Z * lin_v(k, dt)) @ Z.T
    d = np.asarray(k["dims"])
    dz = Z[:, None, d] - Z[None, :, d]
    return dt(k["var"]) * np.exp(-0.5 * (dz * dz / rbf_ls(k, dt)[d] ** 2).sum(-1))


def _algebra(k, Z, mu, S, Y, noise, dt, jitter=1e-8):
    Z, mu, S, Y = _a(Z, dt), _a(mu, dt), _a(S, dt), _a(Y, dt)
    N, Dy = Y.shape
    M = Z.shape[0]
    b, w = dt(sum(k.get("bias", ()))), dt(sum(k.get("white", ())))
    beta = 1 / max(dt(noise), dt(1e-8))
    p0, p1, p2 = part_stats(k, Z, mu, S, dt)
    c = p1.sum(0)
    psi0 = p0 + b + w
    psi1 = p1 + b
    psi2 = p2 + b * (c[:, None] + c[None, :]) + N * b * b
    I = np.eye(M, dtype=dt)
    Kmm = part_K(k, Z, dt) + b + (w + dt(jitter)) * I
    Lmi = _tri_inv(_chol(Kmm))
    A = Lmi @ (beta * psi2) @ Lmi.T
    B = I + A
    LB = _chol(B)
    LBi = _tri_inv(LB)
    cv = LBi @ (Lmi @ (psi1.T @ (beta * Y)))
    wv = Lmi.T @ (LBi.T @ cv)
    data_fit = (cv * cv).sum()
    trYYT = (Y * Y).sum()
    lml = (-0.5 * N * Dy * (np.log(2 * dt(np.pi)) - np.log(beta)) - 0.5 * beta * trYYT
           - 0.5 * Dy * (psi0.sum() * beta - np.trace(A)) - Dy * np.log(np.diag(LB)).sum() + 0.5 * data_fit)
    return dict(Z=Z, mu=mu, S=S, Y=Y, N=N, Dy=Dy, M=M, b=b, w=w, beta=beta, p1=p1, psi0=psi0, psi1=psi1, psi2=psi2, I=I,
                Kmm=Kmm, Lmi=Lmi, A=A, B=B, LBi=LBi, cv=cv, wv=wv, data_fit=data_fit, trYYT=trYYT, lml=lml)


def bound_only(k, Z, mu, S, Y, noise, dt=LD):
    return _algebra(k, Z, mu, S, Y, noise, dt)["lml"]


def evaluate(k, Z, mu, S, Y, noise, dt=LD):
    """dict(lml, woodbury_vector, woodbury_inv, psi2, dL_dKmm, dL_dpsi0/1/2, dnoise, dtheta (the parts' parameters in the
    order [P, bias..., white...]), dZ, dmu, dS, kappa = cond_2(Kmm + 1e-8 I))"""
    a = _algebra(k, Z, mu, S, Y, noise, dt)
    Z, mu, S, Y, N, Dy, M, b, beta, I, Lmi, LBi = (a[x] for x in ("Z", "mu", "S", "Y", "N", "Dy", "M", "b", "beta", "I", "Lmi", "LBi"))
    P = LBi.T @ (Dy * I + a["cv"] @ a["cv"].T) @ LBi
    dKmm = Lmi.T @ (-0.5 * P - 0.5 * Dy * a["B"] + Dy * I) @ Lmi
    d0 = -0.5 * Dy * beta * np.ones(N, dtype=dt)
    d1 = (beta * Y) @ a["wv"].T
    d2 = beta * 0.5 * (Lmi.T @ (Dy * I - P) @ Lmi)
    dnoise = (-0.5 * N * Dy * beta + 0.5 * a["trYYT"] * beta ** 2 + 0.5 * Dy * (a["psi0"].sum() * beta ** 2 - np.trace(a["A"]) * beta)
              + beta * (0.5 * (a["A"] * P).sum() - a["data_fit"]))
    E2 = d2 + d2.T
    t = E2.sum(0)
    d1P = d1 + b * t[None, :]                                          # what P sees: the Bias parts' psi1 times E2 on top
    Gs = dKmm + dKmm.T
    if k["P"] == "linear":
        v = lin_v(k, dt)
        T = d1P + ((mu * v) @ Z.T) @ E2
        TZ, EZ, s = T @ Z, E2 @ Z, S.sum(0)
        ze = 0.5 * (Z * EZ).sum(0)
        dv = d0 @ (np.square(mu) + S) + (mu * TZ).sum(0) + 2 * v * s * ze + (Z * (dKmm @ Z)).sum(0)
        dZ = T.T @ (mu * v) + v * v * s * EZ + (Gs @ Z) * v
        dmu = TZ * v + 2 * d0[:, None] * v * mu
        dS = v * v * ze + d0[:, None] * v + np.zeros_like(mu)
        dv = dv[np.asarray(k["dims"])]
        dP = dv if k["ARD"] else dv.sum(keepdims=True)
    else:
        d = np.asarray(k["dims"])
        ls = rbf_ls(k, dt)[d]
        dvar, dl, dZa, dmua, dSa = psi_grads(k["var"], ls, True, Z[:, d], mu[:, d], S[:, d], d0, d1P, 0.5 * E2, None, dt)
        Kr = part_K(k, Z, dt)
        G = dKmm * Kr
        dz = Z[:, None, d] - Z[None, :, d]
        dvar = dvar + G.sum() / dt(k["var"])
        dl = dl + (G[:, :, None] * dz * dz).sum((0, 1)) / ls ** 3
        dZa = dZa - ((G + G.T)[:, :, None] * dz).sum(1) / ls ** 2
        dZ, dmu, dS = np.zeros_like(Z), np.zeros_like(mu), np.zeros_like(mu)
        dZ[:, d], dmu[:, d], dS[:, d] = dZa, dmua, dSa
        dP = np.concatenate([[dvar], dl if k["ARD"] else dl.sum(keepdims=True)])
    db = dKmm.sum() + d0.sum() + d1.sum() + (a["p1"] @ E2).sum() + 2 * b * N * d2.sum()
    dw = np.trace(dKmm) + d0.sum()
    dtheta = np.concatenate([dP] + [[db] for _ in k.get("bias", ())] + [[dw] for _ in k.get("white", ())])
    Bi = LBi.T @ LBi
    Winv = Lmi.T @ (I - Bi) @ Lmi
    kappa = float(np.linalg.cond(np.asarray(a["Kmm"], dtype=np.float64)))
    return dict(lml=a["lml"], woodbury_vector=a["wv"], woodbury_inv=Winv, psi2=a["psi2"], dL_dKmm=dKmm, dL_dpsi0=d0,
                dL_dpsi1=d1, dL_dpsi2=d2, dnoise=dnoise, dtheta=dtheta, dZ=dZ, dmu=dmu, dS=dS, kappa=kappa)


def expectations(k, Z, mu, S, d0, d1, d2, dt=LD, rows=None):
    """The kernel-level statistics of the whole sum and the chain rule of  sum d0 psi0 + sum d1 * psi1 + sum d2 * psi2  (d2 any
    M x M matrix): dict(psi0, psi1, psi2, psi2n (the first `rows` points; None: all), dtheta in the order [P, bias..., white...],
    dZ, dmu, dS) -- what `Add.psi*(psi_lin_bias=True)` and its three gradient methods compute"""
    Z, mu, S, d0, d1, d2 = (_a(x, dt) for x in (Z, mu, S, d0, d1, d2))
    N = mu.shape[0]
    bs, b, w = [dt(x) for x in k.get("bias", ())], dt(sum(k.get("bias", ()))), dt(sum(k.get("white", ())))
    p0, p1, p2 = part_stats(k, Z, mu, S, dt)
    c = p1.sum(0)
    out = dict(psi0=p0 + b + w, psi1=p1 + b, psi2=p2 + b * (c[:, None] + c[None, :]) + N * b * b)
    n2 = N if rows is None else rows
    out["psi2n"] = np.stack([part_stats(k, Z, mu[i:i + 1], S[i:i + 1], dt)[2] + b * (p1[i][:, None] + p1[i][None, :]) + b * b
                             for i in range(n2)])
    E2 = d2 + d2.T
    d1P = d1 + b * E2.sum(0)[None, :]
    if k["P"] == "linear":
        v = lin_v(k, dt)
        T = d1P + ((mu * v) @ Z.T) @ E2
        TZ, EZ, s = T @ Z, E2 @ Z, S.sum(0)
        ze = 0.5 * (Z * EZ).sum(0)
        dv = (d0 @ (np.square(mu) + S) + (mu * TZ).sum(0) + 2 * v * s * ze)[np.asarray(k["dims"])]
        dP = dv if k["ARD"] else dv.sum(keepdims=True)
        dZ, dmu = T.T @ (mu * v) + v * v * s * EZ, TZ * v + 2 * d0[:, None] * v * mu
        dS = v * v * ze + d0[:, None] * v + np.zeros_like(mu)
    else:
        d = np.asarray(k["dims"])
        dvar, dl, dZa, dmua, dSa = psi_grads(k["var"], rbf_ls(k, dt)[d], True, Z[:, d], mu[:, d], S[:, d], d0, d1P, 0.5 * E2, None, dt)
        dZ, dmu, dS = np.zeros_like(Z), np.zeros_like(mu), np.zeros_like(mu)
        dZ[:, d], dmu[:, d], dS[:, d] = dZa, dmua, dSa
        dP = np.concatenate([[dvar], dl if k["ARD"] else dl.sum(keepdims=True)])
    db = d0.sum() + d1.sum() + (p1 @ E2).sum() + 2 * b * N * d2.sum()
    out.update(dtheta=np.concatenate([dP] + [[db] for _ in bs] + [[d0.sum()] for _ in k.get("white", ())]), dZ=dZ, dmu=dmu, dS=dS)
    return out


def expectations_objective(k, Z, mu, S, d0, d1, d2, dt=LD):
    """sum d0 psi0 + sum d1 * psi1 + sum d2 * psi2 of the whole sum, from the statistics alone (for central differences)"""
    Z, mu, S, d0, d1, d2 = (_a(x, dt) for x in (Z, mu, S, d0, d1, d2))
    b, w = dt(sum(k.get("bias", ()))), dt(sum(k.get("white", ())))
    p0, p1, p2 = part_stats(k, Z, mu, S, dt)
    c = p1.sum(0)
    return (d0 * (p0 + b + w)).sum() + (d1 * (p1 + b)).sum() + (d2 * (p2 + b * (c[:, None] + c[None, :]) + mu.shape[0] * b * b)).sum()


def predict(k, Z, res, mu_new, S_new, dt=LD):
    """(mean, var) at q(x*) = N(mu_new, diag S_new) from the definition: var[n, d] = psi0 + sum_mo psi2n[m, o] (lam_md lam_od
    - W_mo) - mean[n, d]^2, clipped at 1e-15, psi2n one row at a time"""
    Z, mu_new, S_new = _a(Z, dt), _a(mu_new, dt), _a(S_new, dt)
    la, W = _a(res["woodbury_vector"], dt), _a(res["woodbury_inv"], dt)
    b, w = dt(sum(k.get("bias", ()))), dt(sum(k.get("white", ())))
    n, Dy = mu_new.shape[0], la.shape[1]
    mean, var = np.empty((n, Dy), dtype=dt), np.empty((n, Dy), dtype=dt)
    for i in range(n):
        p0, p1, p2 = part_stats(k, Z, mu_new[i:i + 1], S_new[i:i + 1], dt)
        r = p1[0]
        p2n = p2 + b * (r[:, None] + r[None, :]) + b * b
        mean[i] = (r + b) @ la
        var[i] = p0[0] + b + w + np.einsum("mo,md,od->d", p2n, la, la) - (p2n * W).sum() - mean[i] ** 2
    return mean, np.maximum(var, dt(1e-15))


def predict_certain(k, Z, res, Xs, dt=LD):
    """(mean, var) at certain points: the same with S = 0"""
    Z, Xs = _a(Z, dt), _a(Xs, dt)
    la, W = _a(res["woodbury_vector"], dt), _a(res["woodbury_inv"], dt)
    b, w = dt(sum(k.get("bias", ()))), dt(sum(k.get("white", ())))
    if k["P"] == "linear":
        v = lin_v(k, dt)
        Kx, kd = (Xs * v) @ Z.T + b, (np.square(Xs) * v).sum(1) + b + w
    else:
        d = np.asarray(k["dims"])
        dz = Xs[:, None, d] - Z[None, :, d]
        Kx = dt(k["var"]) * np.exp(-0.5 * (dz * dz / rbf_ls(k, dt)[d] ** 2).sum(-1)) + b
        kd = np.full(Xs.shape[0], dt(k["var"]) + b + w, dtype=dt)
    return Kx @ la, np.maximum(kd - ((Kx @ W) * Kx).sum(1), dt(1e-15))[:, None]


def part_specs(k):
    """the C-ABI part list [(kind, ARD, theta, active_dims, term)] of the description"""
    dims = None if list(k["dims"]) == list(range(k["D"])) else np.asarray(k["dims"])
    if k["P"] == "linear":
        first = ("linear", bool(k["ARD"]), np.atleast_1d(np.asarray(k["v"], dtype=np.float64)).ravel(), dims, 0)
    else:
        first = ("rbf", bool(k["ARD"]), np.concatenate([[k["var"]], np.atleast_1d(np.asarray(k["ls"], dtype=np.float64)).ravel()]), dims, 0)
    return [first] + [("bias", False, np.array([float(x)]), None, 0) for x in k.get("bias", ())] + \
        [("white", False, np.array([float(x)]), None, 0) for x in k.get("white", ())]


def make_kernel(k):
    """the gpy_amd kernel object of the description"""
    import gpy_amd
    ad = None if list(k["dims"]) == list(range(k["D"])) else list(k["dims"])
    if k["P"] == "linear":
        P = gpy_amd.Linear(len(k["dims"]), variances=np.asarray(k["v"], dtype=float), ARD=bool(k["ARD"]), active_dims=ad)
    else:
        P = gpy_amd.RBF(len(k["dims"]), variance=float(k["var"]), lengthscale=np.asarray(k["ls"], dtype=float), ARD=bool(k["ARD"]),
                        active_dims=ad)
    parts = [P] + [gpy_amd.Bias(k["D"], variance=float(x), name="bias%d" % i) for i, x in enumerate(k.get("bias", ()))] + \
        [gpy_amd.White(k["D"], variance=float(x), name="white%d" % i) for i, x in enumerate(k.get("white", ()))]
    return P if len(parts) == 1 else gpy_amd.Add(parts)


def problem(P, N, M, D, Dy, seed, ARD=True, bias=(0.7,), white=(0.2,), dims=None):
    """a seeded problem in the fixtures' range: |mu|, |z| <= 2, S in [0.05, 0.5], Y linear (Linear) or sinusoidal (RBF) in mu"""
    r = np.random.default_rng(seed)
    dims = list(range(D)) if dims is None else list(dims)
    mu, S, Z = r.uniform(-2, 2, (N, D)), r.uniform(0.05, 0.5, (N, D)), r.uniform(-2, 2, (M, D))
    na = len(dims)
    if P == "linear":
        W = r.standard_normal((D, Dy)) / np.sqrt(D)
        Y = mu @ W + 0.3 + 0.1 * r.standard_normal((N, Dy))
        k = dict(P=P, D=D, dims=dims, ARD=ARD, v=r.uniform(0.5, 1.5, na if ARD else 1) / max(1.0, D / 4.0))
    else:
        Y = np.sin(mu[:, dims].sum(1, keepdims=True) / np.sqrt(na) + np.arange(Dy)[None, :]) + 0.3 + 0.1 * r.standard_normal((N, Dy))
        k = dict(P=P, D=D, dims=dims, ARD=ARD, var=1.3, ls=r.uniform(0.9, 1.8, na if ARD else 1) * np.sqrt(max(1.0, na / 2.0)))
    k.update(bias=list(bias), white=list(white))
    return dict(k=k, Z=Z, mu=mu, S=S, Y=Y, noise=0.05)
