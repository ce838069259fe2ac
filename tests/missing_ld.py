"""NumPy restatement, in float64 or long double, of the reference's missing-data loop for a Bayesian GPLVM
(`GPy/models/sparse_gp_minibatch.py:228-286`, grouping of `inference/optimization/stochastics.py:57-79`, the 3-D `woodbury_inv`
branches of `inference/latent_function_inference/posterior.py:231-268`), restated from the formulas on top of tests/psi_np.py:

    for each group g of output columns d_g that share a NaN pattern (order: first output index), with its observed rows ninan:
        psi0[ninan], psi1[ninan], psi2n[ninan]  ->  VarDTC on Y[ninan][:, d_g]  (psi2 = the sum of psi2n over the observed rows)
        full dL_dpsi0[ninan] +=, dL_dpsi1[ninan] +=, dL_dpsi2[ninan] += (the group's M x M matrix on every observed row), dL_dKmm +=
        woodbury_inv[:, :, d] = the group's, woodbury_vector[:, d_g] = the group's

The stateless pair of include/mi355gp_sparse_missing.h is restated by `psi2_groups` and `psi_grad_groups`."""
import numpy as np

import psi_np as P

LD = np.longdouble


# ---- grouping -----------------------------------------------------------------------------------------------------------------
def groups_of(Y):
    """(group_of_output (Dy ints), W (N x G, 0/1)): outputs with the same NaN rows share a group; groups in order of their first output"""
    Y = np.asarray(Y)
    obs = ~np.isnan(Y)
    keys, gof = [], np.empty(Y.shape[1], dtype=np.int64)
    for d in range(Y.shape[1]):
        k = obs[:, d].tobytes()
        if k not in keys:
            keys.append(k)
        gof[d] = keys.index(k)
    W = np.stack([obs[:, list(gof).index(g)] for g in range(len(keys))], axis=1).astype(np.float64)
    return gof, W


# ---- the stateless pair -------------------------------------------------------------------------------------------------------
def psi2_groups(var, ls, Z, mu, S, W, dtype=np.float64):
    """G x M x M: psi2_g = sum_n W[n, g] psi2n, row by row"""
    v, l2, Zd, mud, Sd = P._prep(var, ls, Z, mu, S, dtype)
    W = np.asarray(W, dtype=dtype)
    out = np.zeros((W.shape[1], Zd.shape[0], Zd.shape[0]), dtype=dtype)
    for n in range(mud.shape[0]):
        p2 = P.psi2_row(v, l2, Zd, mud[n], Sd[n])
        for g in np.nonzero(W[n])[0]:
            out[g] += W[n, g] * p2
    return out


def psi_grad_groups(var, ls, ARD, Z, mu, S, W, dL, dtype=np.float64):
    """(dvar, dl, dZ, dmu, dS) of sum_g sum(sym(dL[g]) * psi2_g), as the reference forms it: a per-row
    dL_dpsi2[n] = sum_g W[n, g] sym(dL[g]) (its N x M x M array, a row at a time) through the chain rule of
    `psi_np.psi_grads` (rbf_psi_comp.py:70-133)"""
    v, l2, Zd, mud, Sd = P._prep(var, ls, Z, mu, S, dtype)
    W = np.asarray(W, dtype=dtype)
    sym = np.asarray(dL, dtype=dtype)
    sym = 0.5 * (sym + np.transpose(sym, (0, 2, 1)))
    N, Q = mud.shape
    M = Zd.shape[0]
    l = np.sqrt(l2)
    dvar, dl = dtype(0), np.zeros(Q, dtype=dtype)
    dZ, dmu, dS = np.zeros((M, Q), dtype=dtype), np.zeros((N, Q), dtype=dtype), np.zeros((N, Q), dtype=dtype)
    dz = Zd[:, None, :] - Zd[None, :, :]
    for n in range(N):
        gs = np.nonzero(W[n])[0]
        if not len(gs):
            continue
        L = (W[n, gs, None, None] * sym[gs]).sum(0) * P.psi2_row(v, l2, Zd, mud[n], Sd[n])       # M x M
        db = mud[n][None, None, :] - 0.5 * (Zd[:, None, :] + Zd[None, :, :])
        den = 2 * Sd[n] + l2
        dvar += 2 * L.sum() / v
        dmu[n] += -(L[:, :, None] * 2 * db / den).sum((0, 1))
        dS[n] += (L[:, :, None] * (2 * db * db / den ** 2 - 1 / den)).sum((0, 1))
        dZ += (L[:, :, None] * (-dz / (2 * l2) + db / den)).sum(1) + (L[:, :, None] * (dz / (2 * l2) + db / den)).sum(0)
        dl += (L[:, :, None] * (2 * Sd[n] / (l * den) + dz * dz / (2 * l ** 3) + 2 * l * db * db / den ** 2)).sum((0, 1))
    return dvar, (dl if ARD else dl.sum(keepdims=True)), dZ, dmu, dS


def group_problem(N, M, Q, G, seed, ARD=True, edge_masks=True):
    """the inputs of `psi_np.problem` with G 0/1 masks and G matrices dL.  With `edge_masks` (and room for them): group 0 observes
    every row, group 1 only the LAST row, and row 0 is in no group but group 0 -- unless G == 1, where group 0 drops row 0 too
    (a row in no group) when N > 1."""
    p = P.problem(N, M, Q, seed, ARD)
    r = np.random.default_rng(seed + 1000)
    W = (r.uniform(size=(N, G)) < 0.7).astype(np.float64)
    for g in range(G):
        if not W[:, g].any():
            W[r.integers(N), g] = 1.0
    if edge_masks:
        W[:, 0] = 1.0
        if G > 1:
            W[:, 1] = 0.0
            W[N - 1, 1] = 1.0
        if N > 1:
            W[0, 1:] = 0.0
            if G == 1:
                W[0, 0] = 0.0
    p["W"] = W
    p["dL"] = r.standard_normal((G, M, M))
    return p


# ---- the whole evaluation ---------------------------------------------------------------------------------------------------------
def _vardtc_group(v, l2, wsum, Zd, psi0, psi1, psi2, Y, beta, dtype):
    """VarDTC (var_dtc.py:66-276) from given statistics of the observed rows; psi2 already summed over them"""
    N, Dy = Y.shape
    M = Zd.shape[0]
    I = np.eye(M, dtype=dtype)
    Kmm = P._rbf_K(v, l2, Zd) + (wsum + dtype(1e-8)) * I
    Lmi = P._tri_inv(P._chol(Kmm))
    A = Lmi @ (beta * psi2) @ Lmi.T
    B = I + A
    LB = P._chol(B)
    LBi = P._tri_inv(LB)
    c = LBi @ (Lmi @ (psi1.T @ (beta * Y)))
    wv = Lmi.T @ (LBi.T @ c)
    delit = c @ c.T
    data_fit = np.trace(delit)
    Pm = LBi.T @ (Dy * I + delit) @ LBi
    trYYT = (Y * Y).sum()
    lml = (-0.5 * N * Dy * (np.log(2 * dtype(np.pi)) - np.log(beta)) - 0.5 * beta * trYYT
           - 0.5 * Dy * (psi0.sum() * beta - np.trace(A)) - Dy * np.log(np.diag(LB)).sum() + 0.5 * data_fit)
    dL_dKmm = Lmi.T @ (-0.5 * Pm - 0.5 * Dy * B + Dy * I) @ Lmi
    dL_dpsi2 = beta * 0.5 * (Lmi.T @ (Dy * I - Pm) @ Lmi)
    dL_dR = (-0.5 * N * Dy * beta + 0.5 * trYYT * beta ** 2 + 0.5 * Dy * (psi0.sum() * beta ** 2 - np.trace(A) * beta)
             + beta * (0.5 * (A * Pm).sum() - data_fit))
    Winv = Lmi.T @ (I - LBi.T @ LBi) @ Lmi
    return dict(lml=lml, wv=wv, Winv=Winv, dL_dKmm=dL_dKmm, dL_dpsi0=-0.5 * Dy * beta * np.ones(N, dtype=dtype),
                dL_dpsi1=(beta * Y) @ wv.T, dL_dpsi2=dL_dpsi2, dnoise=dL_dR, Kmm=Kmm)


def evaluate(var, ls, ARD, white, Z, mu, S, Y, noise, dtype=np.float64, kl=True):
    """The missing-data bound of RBF(var, ls) + White parts `white` for inputs N(mu, diag S), Y with NaN where unobserved, one noise
    variance.  dict(bound = sum of the groups' log marginal likelihoods (- KL to N(0, 1) with `kl`), lml (without KL), per-group
    lml_g / dnoise_g / woodbury_inv (G x M x M) / psi2 (G x M x M) / dL_dpsi2 (G x M x M), group_of_output, W, woodbury_vector
    (M x Dy), dL_dKmm, dL_dpsi0 (N), dL_dpsi1 (N x M), dnoise, dvar, dl, dwhite, dZ, dmu, dS (without KL), kl_dmu, kl_dS, kappa)"""
    v, l2, Zd, mud, Sd = P._prep(var, ls, Z, mu, S, dtype)
    Y = np.asarray(Y, dtype=np.float64)
    gof, W = groups_of(Y)
    N, Dy = Y.shape
    M, G = Zd.shape[0], W.shape[1]
    wsum = dtype(sum(white))
    beta = 1 / max(dtype(noise), dtype(1e-8))
    psi0, psi1, _, psi2n = P.psi_stats(var, ls, Z, mu, S, None, dtype, want_psi2n=True)
    psi0 = psi0 + wsum
    full = dict(dL_dKmm=np.zeros((M, M), dtype=dtype), dL_dpsi0=np.zeros(N, dtype=dtype), dL_dpsi1=np.zeros((N, M), dtype=dtype))
    wv = np.zeros((M, Dy), dtype=dtype)
    out = dict(lml_g=[], dnoise_g=[], woodbury_inv=[], psi2=[], dL_dpsi2=[])
    for g in range(G):
        ninan, d = W[:, g] > 0, np.nonzero(gof == g)[0]
        psi2g = psi2n[ninan].sum(0)
        r = _vardtc_group(v, l2, wsum, Zd, psi0[ninan], psi1[ninan], psi2g, np.asarray(Y[ninan][:, d], dtype=dtype), beta, dtype)
        full["dL_dKmm"] += r["dL_dKmm"]
        full["dL_dpsi0"][ninan] += r["dL_dpsi0"]
        full["dL_dpsi1"][ninan] += r["dL_dpsi1"]
        wv[:, d] = r["wv"]
        for k, q in (("lml_g", "lml"), ("dnoise_g", "dnoise"), ("woodbury_inv", "Winv"), ("psi2", "psi2g"), ("dL_dpsi2", "dL_dpsi2")):
            out[k].append(psi2g if q == "psi2g" else r[q])
        Kmm = r["Kmm"]
    out = dict((k, np.asarray(x, dtype=dtype)) for k, x in out.items())
    # the chain rule: psi0 and psi1 with the full arrays; psi2 with the per-row dL_dpsi2[n] = sum_g W[n, g] dL_dpsi2_g
    dvar, dl, dZ, dmu, dS = P.psi_grads(var, ls, True, Z, mu, S, full["dL_dpsi0"], full["dL_dpsi1"], None, None, dtype)
    g2 = psi_grad_groups(var, ls, True, Z, mu, S, W, out["dL_dpsi2"], dtype)
    dvar, dl, dZ, dmu, dS = dvar + g2[0], dl + g2[1], dZ + g2[2], dmu + g2[3], dS + g2[4]
    Kr = P._rbf_K(v, l2, Zd)
    Gk = full["dL_dKmm"] * Kr
    dz = Zd[:, None, :] - Zd[None, :, :]
    l = np.sqrt(l2)
    dvar = dvar + Gk.sum() / v
    dl = dl + (Gk[:, :, None] * dz * dz).sum((0, 1)) / l ** 3
    dZ = dZ - ((Gk + Gk.T)[:, :, None] * dz).sum(1) / l2
    dwhite = [np.trace(full["dL_dKmm"]) + full["dL_dpsi0"].sum() for _ in white]
    lml = out["lml_g"].sum()
    klv = 0.5 * (mud * mud + Sd - np.log(Sd) - 1).sum() if kl else dtype(0)
    out.update(full, bound=lml - klv, lml=lml, woodbury_vector=wv, dnoise=out["dnoise_g"].sum(), dvar=dvar,
               dl=(dl if ARD else dl.sum(keepdims=True)), dwhite=dwhite, dZ=dZ, dmu=dmu, dS=dS, kl_dmu=mud * (1 if kl else 0),
               kl_dS=0.5 * (1 - 1 / Sd) * (1 if kl else 0), group_of_output=gof, W=W,
               kappa=float(np.linalg.cond(np.asarray(Kmm, dtype=np.float64))))
    return out


def predict(var, ls, white, Z, r, Xs, Ss=None, dtype=np.float64):
    """(mean (N* x Dy), variance (N* x Dy)) from `evaluate`'s result with the 3-D woodbury_inv (posterior.py:240-248 at certain
    points, :250-269 at N(Xs, diag Ss))"""
    v, l2, Zd, Xd, _ = P._prep(var, ls, Z, Xs, Xs, dtype)
    wv, Winv, gof = r["woodbury_vector"], r["woodbury_inv"], r["group_of_output"]
    wsum = dtype(sum(white))
    if Ss is None:
        d = Xd[:, None, :] - Zd[None, :, :]
        Kx = v * np.exp(-0.5 * (d * d / l2).sum(-1))                     # N* x M
        mean = Kx @ wv
        var_ = np.stack([(v + wsum) - ((Kx @ Winv[gof[i]].T) * Kx).sum(1) for i in range(wv.shape[1])], axis=1)
    else:
        psi0, psi1, _, psi2n = P.psi_stats(var, ls, Z, Xs, Ss, None, dtype, want_psi2n=True)
        mean = psi1 @ wv
        tmp = psi2n - psi1[:, :, None] * psi1[:, None, :]
        var_ = np.einsum("nmo,md,od->nd", tmp, wv, wv) + (psi0 + wsum)[:, None]
        var_ = var_ - np.stack([(psi2n * Winv[gof[i]][None]).sum((1, 2)) for i in range(wv.shape[1])], axis=1)
    return mean, np.clip(var_, 1e-15, np.inf)


def mask_outputs(Y, patterns, seed, frac=0.3):
    """Y with NaNs: output d follows pattern d % patterns.  Pattern 0 observes every row, the others drop each row with probability
    `frac`; the LAST pattern, when patterns > 2, observes one row only (row N - 1); and with N > 2 row 1 is observed by NOTHING"""
    r = np.random.default_rng(seed + 77)
    Y = np.array(Y, dtype=np.float64)
    N, Dy = Y.shape
    for k in range(min(patterns, Dy)):
        drop = (r.uniform(size=N) < frac) if k else np.zeros(N, dtype=bool)
        if k and k == patterns - 1 and patterns > 2:
            drop[:] = True
            drop[N - 1] = False
        if N > 2:
            drop[1] = True
        if drop.all():
            drop[N - 1] = False
        Y[np.ix_(drop, np.arange(Dy) % patterns == k)] = np.nan
    return Y


def fit_problem(N, M, Q, Dy, seed, patterns=3, ARD=True, white=()):
    """`psi_np.fit_problem` with the NaNs of `mask_outputs`"""
    p = P.fit_problem(N, M, Q, Dy, seed, ARD, white)
    p["Y"] = mask_outputs(p["Y"], patterns, seed)
    return p


def lattice_problem(N, M, Q, Dy, seed, patterns=3, ARD=True, white=(0.2,)):
    """a well-conditioned fit (`psi_ss_ld.lattice_problem`: Z on a jittered lattice, cond_2(Kmm + 1e-8 I) <= 1e4) with the NaNs of
    `mask_outputs`, in `fit_problem`'s keys"""
    import psi_ss_ld
    c = psi_ss_ld.lattice_problem(N, M, Q, Dy, seed, ARD=ARD, white=white)
    return dict(var=c["k"]["var"], ls=c["k"]["ls"], ARD=ARD, white=list(white), Z=c["Z"], mu=c["mu"], S=c["S"],
                Y=mask_outputs(c["Y"], patterns, seed), noise=c["noise"], k=c["k"])


# (name, N, M, Q, Dy, patterns, ARD): the fit on the edges of the kernels (missing_ld's psi cases) with Dy in {1, 5, 12}, several
# columns per group across the four-columns-in-registers dispatch of the M x M phase, and 1 .. 12 groups
FIT_CASES = [
    ("n1_m1_q1_dy1_g1", 1, 1, 1, 1, 1, True),
    ("n15_m15_q3_dy5_g2", 15, 15, 3, 5, 2, False),
    ("n17_m17_q16_dy12_g3", 17, 17, 16, 12, 3, True),
    ("n63_m65_q2_dy5_g3", 63, 65, 2, 5, 3, True),
    ("n65_m17_q17_dy12_g9", 65, 17, 17, 12, 9, True),
    ("n257_m130_q2_dy12_g2", 257, 130, 2, 12, 2, True),
    ("n2049_m17_q3_dy5_g3", 2049, 17, 3, 5, 3, True),
    ("n63_m15_q33_dy5_g2", 63, 15, 33, 5, 2, True),
    ("n33_m9_q64_dy1_g1", 33, 9, 64, 1, 1, False),
    ("n17_m65_q1_dy12_g8", 17, 65, 1, 12, 8, True),
    ("n40_m16_q3_dy12_g12", 40, 16, 3, 12, 12, True),
]
