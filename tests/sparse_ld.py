"""Long-double (x86 80-bit) restatement of the sparse (VarDTC) evaluation for sums and products of stationary / White / Bias
parts, scalar or per-point noise and any number of output columns, and the shape sweep that tests/test_oracle_sparse_ld.py
(CPU) and tests/test_gpu_sparse_shapes.py (GPU) share.  Written from the formulas of the reference as oracle/sparse_oracle.py
cites them:

    var_dtc.py:66-215 (inference), :217-233 (dL_dpsi), :240-261 (dL_dR), :264-276 (log marginal likelihood),
    sparse_gp.py:108-119 (kernel and inducing-input gradients), posterior.py:220-262 (prediction).

Everything kernel-shaped comes from tests/kern_ld.py: K, Kdiag, the contractions with dK/dtheta, gradients_X, the part format
(kind, ard, theta, active_dims, term), and the column-oriented Cholesky, triangular solves and explicit-sum matrix product.

The evaluation is arranged in the two passes over the rows that the formulas allow: with k_n the row of Knm, b_n the precision
and V = b R,

    psi2 = sum_n b_n k_n k_n^T,  psi1V = Knm^T V                                            (pass 1)
    A = Lm^-1 psi2 Lm^-T  (:129-134),  B = I + A,  c = LB^-1 Lm^-1 psi1V  (:141-143),  v = Lm^-T LB^-T c  (:144-145)
    P = LB^-T (Dy I + c c^T) LB^-1  (:150-152),  dL_dKmm = Lm^-T (-P/2 - Dy B/2 + Dy I) Lm^-1  (:153-158)
    Q2 = Lm^-T (Dy I - P) Lm^-1 / 2,  dL_dKnm = V v^T + 2 diag(b) Knm Q2  (:219-233)          (pass 2)
    dL_dm = V - Knm v  (:148),  and per row q_n = k_n^T Kmm^-1 k_n, r_n = k_n^T Lm^-T B^-1 Lm^-1 k_n, s_n = k_n^T v for dL_dR.

`back-substitute both sides` is L^-T X L^-1 throughout.  In the plain mode both passes see all rows at once and every operation
is in the working type `dt`.  In the blocked mode (`block=4096`, meant for N above 262144, where N x M long-double arrays and
Python-level column loops are out of reach) the kernel blocks, their Gram, column and row products are formed per row block in
fp64 and rounded once; they are accumulated across blocks in long double, and everything M x M stays in long double.

Inputs of the sweep (`make_case`): Z on a jittered regular grid in the unit cube with the lengthscales of the gridded dimensions
0.75 grid spacings, so that cond2(Kmm + 1e-8 I) stays below 1e3 and an fp64 evaluation lies within 1e-11 of this one; the
seeded tests elsewhere draw Z from X with lengthscales of order one, where the fp64 oracle itself is only good to 1e-7.
"""
import numpy as np

import kern_ld as KL

LD = KL.LD
EPS64 = KL.EPS64
JITTER = 1e-8                       # var_dtc.py:24
LS_FACTOR = {1: 0.75, 2: 0.75, 3: 0.75}      # lengthscale of a gridded dimension in grid spacings, by the dimension of the grid
SUPPORTED = ("rbf", "matern52", "matern32", "exponential", "white", "bias")
JUDGED = ("lml", "dtheta", "dnoise", "dZ", "woodbury_vector", "dL_dm", "dL_dKnm", "dL_dKnm_block", "psi2", "dL_dKmm",
          "woodbury_inv", "mu1", "var1", "cov1", "mu129", "var129", "cov129")


def _backsub(L, X):
    """L^-T X L^-1"""
    return KL.solve_upper_T(L, KL.solve_upper_T(L, X).T).T


def _diag_weights(specs, X, dt):
    """per leaf: the product of the other factors' Kdiag (N,), what update_gradients_diag of a factor is weighted with
    (prod.py:67-71,101-113)"""
    out = [None] * len(specs)
    ones = np.ones(np.shape(X)[0], dtype=dt)
    for t in KL.terms(specs):
        for i in t:
            out[i] = KL._prod([ones] + [KL.leaf_Kdiag(specs[j], X, dt) for j in t if j != i])
    return out


def vardtc(specs, X, Z, R, noise, dt=LD, block=None, max_n=257, psi1_hook=None):
    """One SparseGP.parameters_changed.  noise: one variance or N of them.  Returns dict(lml, dtheta (concatenated in part
    order, with the update_gradients_diag term), dnoise (scalar; per-point noise: N, or N x Dy for Dy > 1), dZ,
    woodbury_vector, woodbury_inv, dL_dKmm, dL_dKnm, dL_dm, psi2 (Knm^T Knm for one noise variance, sum_n b_n k_n k_n^T for
    per-point noise), Kmm (with the 1e-8 on its diagonal), Lm, dZ_zero_cols).

    `psi1_hook(Knm block) -> Knm block` lets a test damage the cross-covariance on its way in."""
    assert all(s[0] in SUPPORTED for s in specs), "the sparse path takes stationary, White and Bias parts"
    X, Z, R = np.asarray(X, np.float64), np.asarray(Z, np.float64), np.asarray(R, np.float64)
    N, D = X.shape
    M, Dy = Z.shape[0], R.shape[1]
    bt = np.float64 if block else dt                             # the type of everything that has N rows
    mm = (lambda a, b: a @ b) if block else KL.matmul
    step = int(block) if block else max(N, 1)
    noise = np.atleast_1d(np.asarray(noise, np.float64)).ravel()
    het = noise.size > 1
    assert noise.size in (1, N)
    beta = 1 / np.maximum(KL._a(noise, dt), dt(JITTER))          # var_dtc.py:78-80
    I = np.eye(M, dtype=dt)
    pi = KL._c(dt)["pi"]

    def rows(r0):
        r1 = min(r0 + step, N)
        Xb = X[r0:r1]
        lv = KL.leaves(specs, Xb, Z, bt)
        P = KL._a(KL.K(specs, Xb, Z, bt, lv), bt) + np.zeros((r1 - r0, M), dtype=bt)
        if psi1_hook is not None:
            P = psi1_hook(P)
        b = KL._a(beta[r0:r1] if het else beta, bt)[:, None]     # (rows, 1) or (1, 1)
        Rb = KL._a(R[r0:r1], bt)
        return r1, Xb, lv, P, b, Rb, KL._a(KL.Kdiag(specs, Xb, bt), bt) + np.zeros(r1 - r0, dtype=bt)

    # ---- pass 1 ----------------------------------------------------------------------------------------------------------
    psi2, psi1V = np.zeros((M, M), dtype=dt), np.zeros((M, Dy), dtype=dt)
    sum_b_psi0 = sum_b2_psi0 = sum_bYY = sum_b2YY = dt(0)
    for r0 in range(0, N, step):
        r1, Xb, lv, P, b, Rb, psi0 = rows(r0)
        psi2 += KL._a(mm((P * b).T, P), dt)
        psi1V += KL._a(mm(P.T, b * Rb), dt)
        bl, yy = KL._a(b[:, 0], dt), np.sum(np.square(KL._a(Rb, dt)), axis=1)
        sum_b_psi0 += np.sum(bl * KL._a(psi0, dt))
        sum_b2_psi0 += np.sum(bl * bl * KL._a(psi0, dt))
        sum_bYY += np.sum(bl * yy)
        sum_b2YY += np.sum(bl * bl * yy)
    sum_logb = np.sum(np.log(beta)) if het else N * np.log(beta[0])
    # ---- the M x M phase -------------------------------------------------------------------------------------------------
    lvm = KL.leaves(specs, Z, None, dt)
    Kmm = KL.K(specs, Z, None, dt, lvm) + dt(JITTER) * I         # :93-94
    Lm = KL.cholesky(Kmm, max_n)
    A = KL.solve_lower(Lm, KL.solve_lower(Lm, psi2).T)           # Lm^-1 psi2 Lm^-T
    A = (A + A.T) / 2
    B = I + A
    LB = KL.cholesky(B, max_n)
    c = KL.solve_lower(LB, KL.solve_lower(Lm, psi1V))
    wv = KL.solve_upper_T(Lm, KL.solve_upper_T(LB, c))
    data_fit = np.sum(c * c)
    P_ = _backsub(LB, Dy * I + KL.matmul(c, c.T))
    dL_dKmm = _backsub(Lm, -P_ / 2 - Dy * B / 2 + Dy * I)
    Q2 = _backsub(Lm, Dy * I - P_) / 2
    LBi = KL.solve_lower(LB, I)
    Bi = KL.matmul(LBi.T, LBi)
    woodbury_inv = _backsub(Lm, I - Bi)                          # :198-214
    trA = np.sum(np.diag(A))
    lml = (-N * Dy * np.log(2 * pi) + Dy * sum_logb - sum_bYY) / 2 - Dy * (sum_b_psi0 - trA) / 2 \
        - Dy * np.sum(np.log(np.diag(LB))) + data_fit / 2        # :264-276
    if het:
        Kmmi, W2 = _backsub(Lm, I), _backsub(Lm, Bi)
        dnoise = np.zeros((N, Dy), dtype=dt)
    else:
        b0 = beta[0]                                             # :258-261
        dnoise = -N * Dy * b0 / 2 + sum_b2YY / 2 + Dy * (sum_b2_psi0 - trA * b0) / 2 + b0 * (np.sum(A * P_) / 2 - data_fit)
    # ---- pass 2 ----------------------------------------------------------------------------------------------------------
    wv_b, Q2_b = KL._a(wv, bt), KL._a(Q2, bt)
    dL_dKnm, dL_dm = np.zeros((N, M), dtype=bt), np.zeros((N, Dy), dtype=bt)
    npar = sum(KL.n_params(s) for s in specs)
    dtheta, dZ = np.zeros(npar, dtype=dt), np.zeros((M, D), dtype=dt)
    first = np.cumsum([0] + [KL.n_params(s) for s in specs])[:-1]
    for r0 in range(0, N, step):
        r1, Xb, lv, P, b, Rb, psi0 = rows(r0)
        V = b * Rb
        G = mm(V, wv_b.T) + 2 * mm(P * b, Q2_b)                  # :219,224-226,233
        dL_dKnm[r0:r1] = G
        s = mm(P, wv_b)
        dL_dm[r0:r1] = V - s                                     # :148
        if het:                                                  # :240-256
            q = np.sum(mm(P, KL._a(Kmmi, bt)) * P, axis=1)[:, None]
            r = np.sum(mm(P, KL._a(W2, bt)) * P, axis=1)[:, None]
            b2 = b * b
            dnoise[r0:r1] = KL._a(-b / 2 + V * V / 2 + Dy * (psi0[:, None] - q) * b2 / 2 + r * b2 / 2 - s * Rb * b2 + s * s * b2 / 2, dt)
        dtheta += KL._a(KL.dtheta(specs, G, Xb, Z, bt, lv)[0], dt)
        dZ += KL._a(KL.gradients_X(specs, G.T, Z, Xb, bt)[0], dt)
        w0 = -Dy * b[:, 0] / 2 + np.zeros(r1 - r0, dtype=bt)      # dL_dpsi0, update_gradients_diag (sparse_gp.py:110)
        for i, wd in enumerate(_diag_weights(specs, Xb, bt)):
            dtheta[first[i]] += np.sum(KL._a(w0 * wd, dt))
    dtheta += KL.dtheta(specs, dL_dKmm, Z, None, dt, lvm)[0]
    dZ += KL.gradients_X(specs, dL_dKmm, Z, None, dt, lvm)[0]
    active = set(int(d) for s in specs if s[0] not in ("white", "bias") for d in s[3])
    if het and Dy == 1:
        dnoise = dnoise[:, 0]
    return dict(lml=lml, dtheta=dtheta, dnoise=dnoise, dZ=dZ, woodbury_vector=wv, woodbury_inv=woodbury_inv, dL_dKmm=dL_dKmm,
                dL_dKnm=dL_dKnm, dL_dm=dL_dm, psi2=psi2 if het else psi2 / beta[0], Kmm=Kmm, Lm=Lm,
                dZ_zero_cols=[q for q in range(D) if q not in active])


def predict(specs, Z, Xs, res, full_cov=False, dt=LD):
    """(mu, var (M* x 1, clipped at 1e-15) or cov) of the sparse posterior at Xs (posterior.py:220-262) from the result of
    `vardtc`"""
    Kx = KL.K(specs, Z, Xs, dt)
    wv, Wi = KL._a(res["woodbury_vector"], dt), KL._a(res["woodbury_inv"], dt)
    mu = KL.matmul(Kx.T, wv)
    if full_cov:
        return mu, KL.K(specs, Xs, None, dt) - KL.matmul(Kx.T, KL.matmul(Wi, Kx))
    var = KL.Kdiag(specs, Xs, dt) - np.sum(KL.matmul(Wi.T, Kx) * Kx, axis=0)
    return mu, np.maximum(var, dt(1e-15))[:, None]


# ---- the judge ---------------------------------------------------------------------------------------------------------------
def rel_err(got, ref):
    """max |got - ref| / max |ref| (a scalar: |got - ref| / |ref|); inf where the shapes differ"""
    if np.shape(got) != np.shape(ref):
        return float("inf")
    wide = np.asarray(ref).dtype != np.float64                   # a blocked reference is fp64 where it has N rows
    got, ref = KL._a(got, LD if wide else np.float64), KL._a(ref, LD if wide else np.float64)
    if ref.size == 0:
        return 0.0
    den = np.max(np.abs(ref))
    num = np.max(np.abs(got - ref))
    return float(num / den) if den > 0 else (0.0 if num == 0 else float("inf"))


def bound(q, ref_ld, ref_64, kappa):
    """max(32 e64(q), 256 eps64 kappa): e64 = the distance of the fp64 oracle from the long-double value on the same input"""
    return max(32.0 * rel_err(ref_64[q], ref_ld[q]), 256.0 * EPS64 * float(kappa))


def judge(got, ref_ld, ref_64, kappa):
    """Hold every quantity of `got` that is in JUDGED to err(q) <= bound(q); the dZ columns outside every part's active_dims
    must be exactly zero.  Returns ({q: (err, bound)}, [what failed])."""
    figs, bad = {}, []
    for q in JUDGED:
        if q not in got or got[q] is None:
            continue
        e, b = rel_err(got[q], ref_ld[q]), bound(q, ref_ld, ref_64, kappa)
        figs[q] = (e, b)
        if not e <= b:
            bad.append("%s: %.3e > %.3e" % (q, e, b))
    if "dZ" in got:
        for col in ref_ld.get("dZ_zero_cols", []):
            if np.any(np.asarray(got["dZ"])[:, col] != 0):
                bad.append("dZ column %d is outside every part's active_dims and must be exactly 0" % col)
    return figs, bad


# ---- the shape sweep -------------------------------------------------------------------------------------------------------
KERNELS = ("rbf_ard", "matern52_iso", "matern32_ard", "exponential_iso", "rbf+white", "rbf_ard+bias", "prod", "rbf_ard_subset")
FAMILIES = ("m_edge", "n_edge", "noise", "subset", "dispatch", "stale", "chunks")


def _case(family, kern, N, M, D, Dy, het=False, variant=0):
    name = "%s-%s-n%d_m%d_d%d_dy%d-%s" % (family, kern, N, M, D, Dy, "het" if het else "hom") + ("-v%d" % variant if variant else "")
    return dict(name=name, family=family, kern=kern, N=N, M=M, D=D, Dy=Dy, het=het, variant=variant, blocked=family == "chunks")


def _cases():
    out = []
    # M edges: m < mp | m == mp (128) | the first persistent Kmm launch on the side stream (129) | three tiles (257)
    out += [_case("m_edge", "rbf_ard", 257, M, 2, 1) for M in (1, 127, 128, 129, 257)]
    out += [_case("m_edge", k, 257, M, 2, 1) for k in ("rbf+white", "prod") for M in (128, 129)]
    # N edges: the 128-row GEMM padding, the 256-row Gram rounding, the 2048-row chunk granule; N < M on purpose
    out += [_case("n_edge", k, N, 65, 3, 2) for k in ("matern52_iso", "rbf_ard+bias") for N in (1, 2, 127, 128, 129, 255, 256, 257, 2049)]
    # per-point noise, one and several output columns: fused single part, sum, product
    out += [_case("noise", k, N, M, 3, Dy, het=True) for N, M, single in ((257, 65, "rbf_ard"), (129, 128, "exponential_iso"))
            for Dy in (1, 3) for k in (single, "rbf+white", "prod")]
    out += [_case("subset", "rbf_ard_subset", 257, 65, 3, 2)]
    # the (D, Dy) boundaries of the dispatch: fused up to D = 16, ARD groups of 32 dimensions, four output columns in registers
    out += [_case("dispatch", k, 193, 65, D, Dy) for D, Dy in ((16, 4), (16, 5), (17, 1), (32, 4), (32, 5), (33, 1), (1, 1))
            for k in ("rbf_ard", "matern32_ard")]
    # stale state: one context, no set_data between the members (same X and R: the seed leaves M, the kernel and the noise out)
    out += [_case("stale", "prod", 257, 129, 3, 3, het=True), _case("stale", "rbf_ard", 257, 129, 3, 3),
            _case("stale", "rbf_ard", 257, 128, 3, 3), _case("stale", "rbf_ard", 257, 128, 3, 3, variant=1)]
    # several chunks (blocked reference)
    out += [_case("chunks", "rbf_ard", 262145, 128, 2, 1), _case("chunks", "rbf_ard+bias", 266240, 3, 2, 2, het=True),
            _case("chunks", "prod", 262145, 65, 3, 1)]
    return out


CASES = _cases()
BY_NAME = dict((c["name"], c) for c in CASES)
PLAIN = [c["name"] for c in CASES if not c["blocked"]]
BLOCKED = [c["name"] for c in CASES if c["blocked"]]
STALE = [c["name"] for c in CASES if c["family"] == "stale"]
DETERMINISM = "noise-prod-n257_m65_d3_dy3-het"
CHUNK_BLOCKS = {"chunks-rbf_ard+bias-n266240_m3_d2_dy2-het": (133000, 300)}       # across the chunk boundary at 133120


def _grid_side(M, nd):
    g = 1
    while g ** nd < M:
        g += 1
    return g


def _specs(kern, D, g, gdims, rng, variant):
    """the part list of one kernel variant: gridded dimensions get LS_FACTOR / g, the others 4 sqrt(D)"""
    scale = 1.0 + 0.2 * variant                                  # `variant`: the same case with other theta (and Z)
    allq = np.arange(D, dtype=np.int32)

    def ls(dims, ard):
        v = np.array([LS_FACTOR[len(gdims)] / g * rng.uniform(0.9, 1.1) if int(q) in gdims else 4.0 * np.sqrt(D) for q in dims])
        return scale * (v if ard else v[:1])
    if kern in ("rbf_ard", "rbf_ard+bias", "rbf_ard_subset"):
        dims = np.array(gdims, dtype=np.int32) if kern == "rbf_ard_subset" else allq
        out = [("rbf", 1, np.concatenate([[1.3 * scale], ls(dims, 1)]), dims, 0)]
        if kern == "rbf_ard+bias":
            out.append(("bias", 0, np.array([0.2]), allq, 0))
        return out
    if kern == "matern32_ard":
        return [("matern32", 1, np.concatenate([[0.9], ls(allq, 1)]), allq, 0)]
    if kern in ("matern52_iso", "exponential_iso"):
        return [(kern[:-4], 0, np.concatenate([[1.1 if kern[0] == "m" else 0.8], ls(allq, 0)]), allq, 0)]
    if kern == "rbf+white":
        return [("rbf", 0, np.concatenate([[1.2], ls(allq, 0)]), allq, 0), ("white", 0, np.array([0.05]), allq, 0)]
    assert kern == "prod" and D >= 2                             # rbf[0 .. D-2] x matern32[D-1] + white (D = 3: rbf[0,1] x matern32[2])
    return [("rbf", 0, np.concatenate([[1.3], ls(allq[:-1], 0)]), allq[:-1], 1),
            ("matern32", 0, np.concatenate([[0.8], ls(allq[-1:], 0)]), allq[-1:], 1), ("white", 0, np.array([0.03]), allq, 0)]


def oracle_parts(specs):
    """the part list as oracle/sparse_oracle.py takes it: (kind, ARD, variance, lengthscale, active_dims, term)"""
    return [(s[0], bool(s[1]), float(s[2][0]), np.array(s[2][1:]) if len(s[2]) > 1 else None, [int(d) for d in s[3]], int(s[4]))
            for s in specs]


def make_case(name):
    """the seeded inputs of one case: dict(specs, parts, X, Z, R, noise, Xs1, Xs129, ...).  Z on a jittered regular grid
    (g = ceil(M^(1/nd)) cells a side over the first nd <= 3 active dimensions, M of its g^nd cell centres, jitter +-0.2 / g),
    the other dimensions of Z and all of X uniform in the unit cube ([0, 1]^D; D = 1: [-1/2, 1/2]); targets a smooth function plus noise of variance
    0.05 x scale; per-point noise 0.03 + 0.1 u."""
    c = dict(BY_NAME[name])
    N, M, D, Dy, kern = c["N"], c["M"], c["D"], c["Dy"], c["kern"]
    gdims = [0, 2] if kern == "rbf_ard_subset" else list(range(min(D, 3)))
    g = _grid_side(M, len(gdims))
    data = np.random.default_rng([FAMILIES.index(c["family"]), N, D, Dy] + ([] if c["family"] == "stale" else [M, KERNELS.index(kern)]))
    X = data.uniform(0.0, 1.0, (N, D))
    freq = data.uniform(1.0, 3.0, (D, Dy))
    rng = np.random.default_rng([FAMILIES.index(c["family"]), N, M, D, Dy, KERNELS.index(kern), int(c["het"]), c["variant"]])
    Z = rng.uniform(0.0, 1.0, (M, D))
    sites = rng.permutation(g ** len(gdims))[:M]
    for a, q in enumerate(gdims):
        Z[:, q] = ((sites // g ** a) % g + 0.5 + rng.uniform(-0.2, 0.2, M)) / g
    specs = _specs(kern, D, g, gdims, rng, c["variant"])
    scale = float(np.max(KL.Kdiag(specs, X[:1], np.float64)))
    noise_var = 0.05 * scale
    nstd = np.sqrt(0.05 if c["family"] == "stale" else noise_var)          # stale: the members share X and R
    R = np.sin(2.0 * np.pi * X[:, :min(D, 3)] @ freq[:min(D, 3)]) + nstd * data.standard_normal((N, Dy))
    noise = 0.03 + 0.1 * rng.uniform(0.0, 1.0, N) if c["het"] else noise_var
    # D = 1: 65 cells of 0.75 lengthscales each put scaled coordinates of up to 87 into the oracle's |x|^2 + |z|^2 - 2 x.z, and
    # its fp64 distance from long double reaches 1.3e-11; the unit interval centred at the origin halves them (e64 2e-12)
    shift = 0.5 if D == 1 else 0.0
    c.update(specs=specs, parts=oracle_parts(specs), X=X - shift, Z=Z - shift, R=R, noise=noise, scale=scale,
             Xs1=rng.uniform(0.0, 1.0, (1, D)) - shift, Xs129=rng.uniform(0.0, 1.0, (129, D)) - shift,
             block=CHUNK_BLOCKS.get(name, (N // 3, N // 2)))
    return c


def _with_predictions(res, c, fn):
    for tag in ("1", "129"):
        res["mu" + tag], res["var" + tag] = fn(c["Xs" + tag], False)
        res["cov" + tag] = fn(c["Xs" + tag], True)[1]
    r0, nr = c["block"]
    res["dL_dKnm_block"] = res["dL_dKnm"][r0:r0 + nr]
    return res


def oracle64(c):
    """the fp64 oracle (oracle/sparse_oracle.py) on the inputs of a case, with the quantities the judge names"""
    from oracle import gp_oracle as O
    from oracle import sparse_oracle as S
    res = S.vardtc_general(c["parts"], c["X"], c["Z"], c["R"], c["noise"])
    psi1 = O.sum_kern_K(c["parts"], c["X"], c["Z"])
    res["psi2"] = (psi1 / np.fmax(c["noise"], JITTER)[:, None]).T @ psi1 if c["het"] else psi1.T @ psi1
    return _with_predictions(res, c, lambda Xs, full: S.sparse_predict(c["parts"], c["Z"], Xs, res["woodbury_vector"],
                                                                       res["woodbury_inv"], full_cov=full))


_MEMO = {}


def reference(name):
    """(case, long-double reference (blocked for the `chunks` family), fp64 oracle, kappa = cond2(Kmm + 1e-8 I) in fp64) of a
    case, computed once per process and not to be modified"""
    if name not in _MEMO:
        KL.require_ld()
        c = make_case(name)
        ref = vardtc(c["specs"], c["X"], c["Z"], c["R"], c["noise"], block=4096 if c["blocked"] else None)
        _with_predictions(ref, c, lambda Xs, full: predict(c["specs"], c["Z"], Xs, ref, full))
        kappa = float(np.linalg.cond(KL.f64(ref["Kmm"])))
        _MEMO[name] = (c, ref, oracle64(c), kappa)
    return _MEMO[name]
