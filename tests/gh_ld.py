"""Gauss-Hermite psi-statistics of a stationary kernel, their gradients and the VarDTC fit on them in a chosen float type (long
double by default), with loops over the nodes (reference `psi_comp/gaussherm.py:17-101`): t_i = sqrt(2) x_i, w_i = omega_i / sqrt(pi)
of hermgauss(H), X(i) = mu + t_i sqrt(S), the SAME node in every dimension.  Everything kernel-shaped is tests/kern_ld.py's, the
M x M phase tests/sparse_ld.py's.  Carries the cases of tests/test_gpu_psi_gh.py and the fp64 distances its tolerances come from."""
import numpy as np

import kern_ld as KL
import sparse_ld as SL

LD = KL.LD
QUANTITIES = ("psi0", "psi1", "psi2", "dtheta", "dZ", "dmu", "dS")
# max over CASES of the relative distance (max-abs norm) of this file in fp64 from this file in long double (`tolerance` uses it)
F64_DISTANCE = dict(psi0=1.2e-16, psi1=3.8e-16, psi2=2.3e-15, dtheta=7.1e-16, dZ=4.0e-16, dmu=8.4e-16, dS=4.6e-16)


def tolerance(q):
    return max(16.0 * F64_DISTANCE[q], 64.0 * float(np.finfo(np.float64).eps))


def ident(c):
    return "-".join(str(x) for x in c)


def _nodes(mu, S, H, dt):
    x, w = np.polynomial.hermite.hermgauss(int(H))
    t, w = np.asarray(x * np.sqrt(2.0), np.float64), np.asarray(w / np.sqrt(np.pi), np.float64)      # (fp64, as the device gets them)
    mu, rS = KL._a(mu, dt), np.sqrt(KL._a(S, dt))
    return [(dt(t[i]), dt(w[i]), mu + dt(t[i]) * rS) for i in range(len(t))], rS


def stats(spec, Z, mu, S, H=11, dt=LD):
    """(psi0 (N), psi1 (N x M), psi2 (M x M)) of one stationary part"""
    N, M = np.shape(mu)[0], np.shape(Z)[0]
    psi0, psi1, psi2 = np.zeros(N, dtype=dt), np.zeros((N, M), dtype=dt), np.zeros((M, M), dtype=dt)
    for t, w, Xi in _nodes(mu, S, H, dt)[0]:
        Ki = KL._a(KL.K([spec], Xi, Z, dt), dt)
        psi0 += w * KL.Kdiag([spec], Xi, dt)
        psi1 += w * Ki
        psi2 += w * KL.matmul(Ki.T, Ki)
    return psi0, psi1, psi2


def grads(spec, Z, mu, S, dL0=None, dL1=None, dL2=None, H=11, dt=LD):
    """dict(dtheta, dZ, dmu, dS) of sum dL0 psi0 + sum dL1 psi1 + sum dL2 psi2"""
    N, D = np.shape(mu)
    M = np.shape(Z)[0]
    dL1 = np.zeros((N, M), dtype=dt) if dL1 is None else KL._a(dL1, dt)
    D2 = np.zeros((M, M), dtype=dt) if dL2 is None else KL._a(dL2, dt) + KL._a(dL2, dt).T
    out = dict(dtheta=np.zeros(KL.n_params(spec), dtype=dt), dZ=np.zeros((M, D), dtype=dt), dmu=np.zeros((N, D), dtype=dt),
               dS=np.zeros((N, D), dtype=dt))
    nodes, rS = _nodes(mu, S, H, dt)
    for t, w, Xi in nodes:
        lv = KL.leaves([spec], Xi, Z, dt)
        G = w * (dL1 + KL.matmul(KL._a(lv[0].K, dt), D2))
        out["dtheta"] += KL.dtheta([spec], G, Xi, Z, dt, lv)[0]
        if dL0 is not None:
            out["dtheta"][0] += w * np.sum(KL._a(dL0, dt))       # update_gradients_diag: dKdiag / dvariance = 1
        dX = KL.gradients_X([spec], G, Xi, Z, dt, lv)[0]
        out["dZ"] += KL.gradients_X([spec], G.T, Z, Xi, dt)[0]
        out["dmu"] += dX
        out["dS"] += dX * t / (2 * rS)
    return out


def fit(specs, Z, mu, S, R, noise, H=11, dt=LD, max_n=257):
    """One SparseGP.parameters_changed with a NormalPosterior X: one stationary part and White parts, one noise variance
    (var_dtc.py:66-276 with the statistics above; the M x M phase as tests/sparse_ld.py:105-129)."""
    ist = [i for i, s in enumerate(specs) if s[0] != "white"]
    assert len(ist) == 1 and all(s[4] == 0 for s in specs)
    sp = specs[ist[0]]
    N, D = np.shape(mu)
    M, Dy = np.shape(Z)[0], np.shape(R)[1]
    R = KL._a(R, dt)
    beta = 1 / max(dt(noise), dt(SL.JITTER))
    wsum = sum(n[1] for n in _nodes(mu, S, H, dt)[0])
    psi0, psi1, psi2 = stats(sp, Z, mu, S, H, dt)
    psi0 = psi0 + wsum * sum(dt(s[2][0]) for s in specs if s[0] == "white")
    I = np.eye(M, dtype=dt)
    pi = KL._c(dt)["pi"]
    lvm = KL.leaves(specs, Z, None, dt)
    Kmm = KL.K(specs, Z, None, dt, lvm) + dt(SL.JITTER) * I
    Lm = KL.cholesky(Kmm, max_n)
    A = KL.solve_lower(Lm, KL.solve_lower(Lm, beta * psi2).T)
    A = (A + A.T) / 2
    B = I + A
    LB = KL.cholesky(B, max_n)
    c = KL.solve_lower(LB, KL.solve_lower(Lm, KL.matmul(psi1.T, beta * R)))
    wv = KL.solve_upper_T(Lm, KL.solve_upper_T(LB, c))
    data_fit = np.sum(c * c)
    P_ = SL._backsub(LB, Dy * I + KL.matmul(c, c.T))
    dL_dKmm = SL._backsub(Lm, -P_ / 2 - Dy * B / 2 + Dy * I)
    Q2 = SL._backsub(Lm, Dy * I - P_) / 2
    LBi = KL.solve_lower(LB, I)
    trA, YY = np.sum(np.diag(A)), np.sum(R * R)
    lml = (-N * Dy * np.log(2 * pi) + Dy * N * np.log(beta) - beta * YY) / 2 - Dy * (beta * np.sum(psi0) - trA) / 2 \
        - Dy * np.sum(np.log(np.diag(LB))) + data_fit / 2
    dnoise = -N * Dy * beta / 2 + beta * beta * YY / 2 + Dy * (beta * beta * np.sum(psi0) - trA * beta) / 2 \
        + beta * (np.sum(A * P_) / 2 - data_fit)
    dL0 = np.full(N, -Dy * beta / 2, dtype=dt)
    g = grads(sp, Z, mu, S, dL0, KL.matmul(beta * R, wv.T), beta * Q2, H, dt)
    first = np.cumsum([0] + [KL.n_params(s) for s in specs])
    dtheta = KL.dtheta(specs, dL_dKmm, Z, None, dt, lvm)[0]
    dtheta[first[ist[0]]:first[ist[0] + 1]] += g["dtheta"]
    for i, s in enumerate(specs):
        if s[0] == "white":
            dtheta[first[i]] += wsum * np.sum(dL0)
    return dict(lml=lml, dnoise=dnoise, dtheta=dtheta, dZ=KL.gradients_X(specs, dL_dKmm, Z, None, dt, lvm)[0] + g["dZ"], dmu=g["dmu"],
                dS=g["dS"], woodbury_vector=wv, woodbury_inv=SL._backsub(Lm, I - KL.matmul(LBi.T, LBi)), Kmm=Kmm,
                zero_cols=[q for q in range(D) if q not in set(int(d) for d in sp[3])])


# (kind, ARD, N, M, Q, H, a row of mu equals a row of Z).  The device tiles rows by 16, inducing points by 64 and chunks rows by
# 2048; at M = 321 (padded to 384) the gradient kernel's row-block operands leave LDS for its global scratch.
CASES = [("matern52", 1, 1, 1, 1, 1, False), ("exponential", 0, 15, 15, 3, 2, False), ("matern32", 1, 17, 17, 3, 11, False),
         ("matern52", 0, 17, 65, 33, 11, False), ("rbf", 1, 33, 64, 3, 11, True), ("exponential", 1, 16, 17, 1, 11, True),
         ("matern32", 0, 2049, 15, 3, 2, False), ("matern52", 1, 17, 321, 1, 2, False), ("matern52", 1, 130, 66, 2, 3, True)]


def make_case(c):
    kind, ARD, N, M, Q, H, coincide = c
    rng = np.random.default_rng([N, M, Q, H, int(ARD)])
    Z, mu = rng.uniform(0, 1, (M, Q)), rng.uniform(0, 1, (N, Q))
    if coincide:
        mu[N // 2] = Z[M // 2]
    ls = 0.6 * np.sqrt(Q) * rng.uniform(0.8, 1.25, Q if ARD else 1)
    spec = (kind, int(ARD), np.concatenate([[1.3], ls]), np.arange(Q, dtype=np.int32), 0)
    dL2 = rng.standard_normal((M, M)) / M
    return dict(spec=spec, Z=Z, mu=mu, S=rng.uniform(0.02, 0.3, (N, Q)), H=H, dL0=rng.standard_normal(N),
                dL1=rng.standard_normal((N, M)), dL2=dL2 + dL2.T, dL2_raw=dL2, R=rng.standard_normal((N, 2)),
                v=rng.standard_normal((M, 2)))


def all_quantities(c, dt=LD, dL=("dL0", "dL1", "dL2")):
    a = (c["spec"], c["Z"], c["mu"], c["S"])
    out = dict(zip(("psi0", "psi1", "psi2"), stats(*a, H=c["H"], dt=dt)))
    out.update(grads(*a, *(None if k is None else c[k] for k in dL), H=c["H"], dt=dt))
    return out


def rel(x, ref):
    ref = np.asarray(ref, dtype=LD)
    return float(np.abs(np.asarray(x, dtype=LD) - ref).max() / max(float(np.abs(ref).max()), 1e-300))


# The fit: (a case of tests/sparse_ld.py -- Z on a jittered grid, lengthscale 0.75 grid spacings --, the kind its stationary part
# is given here, White variance or None, H); its X are the means, the variances are drawn in units of the grid spacing
FIT_CASES = [("n_edge-matern52_iso-n127_m65_d3_dy2-hom", "matern52", None, 11), ("dispatch-matern32_ard-n193_m65_d1_dy1-hom", "matern32", 0.05, 11),
             ("n_edge-matern52_iso-n2_m65_d3_dy2-hom", "exponential", None, 3), ("subset-rbf_ard_subset-n257_m65_d3_dy2-hom", "matern52", None, 2)]


def make_fit_case(c):
    name, kind, white, H = c
    k = SL.make_case(name)
    specs = [(kind,) + k["specs"][0][1:]]                             # (the subset case keeps active_dims (0, 2) of D = 3)
    if white:
        specs.append(("white", 0, np.array([white]), np.arange(k["D"], dtype=np.int32), 0))
    g = SL._grid_side(k["M"], 2 if "subset" in name else min(k["D"], 3))
    S = np.random.default_rng(k["N"]).uniform(0.2, 1.0, k["X"].shape) / g ** 2
    return dict(specs=specs, Z=k["Z"], mu=k["X"], S=S, R=k["R"], noise=k["noise"], H=H)
