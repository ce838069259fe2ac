"""Restatement of the FITC / power-EP (PEP) sparse evaluation, generic over the working type (float64 and x86 80-bit long
double), for sums and products of stationary / White / Bias parts, one noise variance and one output column; the fixtures of
tests/golden/pep, the stand-in device context of the CPU tests and the shape sweep that tests/test_oracle_pep.py (CPU) and
tests/test_gpu_pep.py (GPU) share.  Written from the formulas of the reference:

    pep.py:23-93 (fitc.py:21-88 is alpha = 1), sparse_gp.py:108-119 (kernel and inducing-input gradients, certain inputs),
    posterior.py:220-262 (prediction).

With U = K(X, Z), Kmm = K(Z) + jitter I (1e-6), L = chol(Kmm), s2 the noise variance and c = (1 - alpha) / alpha:

    q_n = |L^-1 k_n|^2,  sigma*_n = s2 + alpha (Knn_n - q_n),  beta*_n = 1 / sigma*_n                          (:44-46)
    A = I + (L^-1 U^T) diag(beta*) (L^-1 U^T)^T,  LA = chol(A),  b = LA^-1 L^-1 U^T (beta* y),  v = L^-T LA^-T b,
    P = L^-T LA^-T LA^-1 L^-1                                                                                   (:49-59)
    lml = -N/2 log 2 pi - sum log diag LA + (1 + c)/2 sum log beta* - 1/2 sum beta* y^2 + |b|^2/2 + c N/2 log s2  (:64-68)
    dL_dR_n = beta*^2 (k^T P k - (1 + c)/beta* + y^2 - 2 y k^T v + (k^T v)^2) / 2                                  (:70-72)
    dL_dKmm = (Kmm^-1 - v v^T - P)/2 + alpha Kmm^-1 U^T diag(dL_dR) U Kmm^-1                                     (:75-78)
    dL_dKnm[n] = beta*_n (y_n v^T - k_n^T (v v^T + P)) - 2 alpha dL_dR_n (Kmm^-1 k_n)^T                            (:81-84)
    dL_dKdiag = alpha dL_dR,  dL_dthetaL = sum dL_dR + c N / (2 s2),  woodbury_inv = Kmm^-1 - P,  woodbury_vector = v

Everything kernel-shaped comes from tests/kern_ld.py, the judge, the bound and the way inputs are drawn from tests/sparse_ld.py.
In the plain mode every operation is in the working type.  In the blocked mode (`block=4096`, for N above 262144) the kernel
blocks and the products that have a block's rows are formed in fp64 and rounded once, accumulated across blocks in long double,
and everything M x M stays in long double (`sparse_ld.vardtc(block=...)` is the model).
"""
import glob
import json
import os

import numpy as np

import kern_ld as KL
import sparse_ld as SL

LD = KL.LD
JITTER = 1e-6                       # pep.py:17, fitc.py:17
JUDGED = ("lml", "dtheta", "dnoise", "dZ", "woodbury_vector", "woodbury_inv", "dL_dKmm", "dL_dKnm_block", "mu1", "var1", "cov1",
          "mu129", "var129", "cov129")


def pep(specs, X, Z, Y, noise, alpha, dt=LD, block=None, max_n=257, jitter=JITTER):
    """One PEP.inference and the gradient assembly of sparse_gp.py:108-119.  Returns dict(lml, dtheta (concatenated in part order,
    with the update_gradients_diag term), dnoise (= dL_dthetaL), dZ, woodbury_vector (M x 1), woodbury_inv, dL_dKmm, dL_dKnm,
    dL_dR, dL_dKdiag, sigma_star, Kmm (with the jitter), Lm, dZ_zero_cols)."""
    assert all(s[0] in SL.SUPPORTED for s in specs), "the sparse path takes stationary, White and Bias parts"
    X, Z, Y = np.asarray(X, np.float64), np.asarray(Z, np.float64), np.asarray(Y, np.float64)
    N, D = X.shape
    M = Z.shape[0]
    assert Y.shape == (N, 1) and 0.0 < alpha <= 1.0
    bt = np.float64 if block else dt                             # the type of everything that has N rows
    mm = (lambda a, b: a @ b) if block else KL.matmul
    step = int(block) if block else max(N, 1)
    s2, al = dt(noise), dt(alpha)
    c = (1 - al) / al
    I = np.eye(M, dtype=dt)
    pi = KL._c(dt)["pi"]
    lvm = KL.leaves(specs, Z, None, dt)
    Kmm = KL.K(specs, Z, None, dt, lvm) + dt(jitter) * I         # :34,40
    Lm = KL.cholesky(Kmm, max_n)
    Li = KL.solve_lower(Lm, I)
    Kmmi = KL.matmul(Li.T, Li)
    Li_b, Kmmi_b = KL._a(Li, bt), KL._a(Kmmi, bt)

    def rows(r0):
        r1 = min(r0 + step, N)
        Xb = X[r0:r1]
        lv = KL.leaves(specs, Xb, Z, bt)
        U = KL._a(KL.K(specs, Xb, Z, bt, lv), bt) + np.zeros((r1 - r0, M), dtype=bt)
        knn = KL._a(KL.Kdiag(specs, Xb, bt), bt) + np.zeros(r1 - r0, dtype=bt)
        W = mm(U, Li_b.T)                                        # rows (L^-1 k_n)^T
        sig = bt(s2) + bt(al) * (knn - np.sum(W * W, axis=1))    # :45
        return r1, Xb, lv, U, W, sig, 1 / sig, KL._a(Y[r0:r1, 0], bt)

    # ---- pass 1 ----------------------------------------------------------------------------------------------------------
    G, r = np.zeros((M, M), dtype=dt), np.zeros(M, dtype=dt)
    sum_logb = sum_byy = dt(0)
    sigma_star = np.zeros(N, dtype=bt)
    for r0 in range(0, N, step):
        r1, Xb, lv, U, W, sig, b, y = rows(r0)
        sigma_star[r0:r1] = sig
        Ws = W * np.sqrt(b)[:, None]
        G += KL._a(mm(Ws.T, Ws), dt)                             # :49
        r += KL._a(mm(W.T, (b * y)[:, None])[:, 0], dt)          # :53-54
        sum_logb += np.sum(np.log(KL._a(b, dt)))
        sum_byy += np.sum(KL._a(b, dt) * np.square(KL._a(y, dt)))
    # ---- the M x M phase -------------------------------------------------------------------------------------------------
    G = (G + G.T) / 2
    A = I + G
    LA = KL.cholesky(A, max_n)
    bv = KL.solve_lower(LA, r[:, None])                          # :55
    v = KL.solve_upper_T(Lm, KL.solve_upper_T(LA, bv))           # :56-57
    LAi = KL.solve_lower(LA, I)
    Ai = KL.matmul(LAi.T, LAi)
    P = KL.matmul(Li.T, KL.matmul(Ai, Li))                       # :58-59
    woodbury_inv = KL.matmul(Li.T, KL.matmul(I - Ai, Li))        # Kmm^-1 - P (:91)
    lml = -N * np.log(2 * pi) / 2 - np.sum(np.log(np.diag(LA))) + (1 + c) * sum_logb / 2 - sum_byy / 2 \
        + np.sum(bv * bv) / 2 + c * N * np.log(s2) / 2           # :64-68
    # ---- pass 2 ----------------------------------------------------------------------------------------------------------
    v_b, P_b = KL._a(v, bt), KL._a(P, bt)
    dL_dKnm, dL_dR = np.zeros((N, M), dtype=bt), np.zeros(N, dtype=bt)
    npar = sum(KL.n_params(s) for s in specs)
    dtheta, dZ = np.zeros(npar, dtype=dt), np.zeros((M, D), dtype=dt)
    first = np.cumsum([0] + [KL.n_params(s) for s in specs])[:-1]
    S = np.zeros((M, M), dtype=dt)
    sum_dR = dt(0)
    for r0 in range(0, N, step):
        r1, Xb, lv, U, W, sig, b, y = rows(r0)
        Uv = mm(U, v_b)[:, 0]
        UP = mm(U, P_b)
        dR = (np.sum(U * UP, axis=1) - bt(1 + c) / b + y * y - 2 * Uv * y + Uv * Uv) * b * b / 2       # :70-72
        KiU = mm(U, Kmmi_b)                                      # rows (Kmm^-1 k_n)^T
        Gnm = b[:, None] * ((y - Uv)[:, None] * v_b[:, 0][None, :] - UP) - 2 * bt(al) * dR[:, None] * KiU   # :81-84
        dL_dKnm[r0:r1], dL_dR[r0:r1] = Gnm, dR
        S += KL._a(mm((KiU * dR[:, None]).T, KiU), dt)           # :77-78
        sum_dR += np.sum(KL._a(dR, dt))
        dtheta += KL._a(KL.dtheta(specs, Gnm, Xb, Z, bt, lv)[0], dt)
        dZ += KL._a(KL.gradients_X(specs, Gnm.T, Z, Xb, bt)[0], dt)
        w0 = bt(al) * dR                                         # dL_dKdiag, update_gradients_diag (sparse_gp.py:110)
        for i, wd in enumerate(SL._diag_weights(specs, Xb, bt)):
            dtheta[first[i]] += np.sum(KL._a(w0 * wd, dt))
    dL_dKmm = (Kmmi - KL.matmul(v, v.T) - P) / 2 + al * (S + S.T) / 2
    dtheta += KL.dtheta(specs, dL_dKmm, Z, None, dt, lvm)[0]
    dZ += KL.gradients_X(specs, dL_dKmm, Z, None, dt, lvm)[0]
    active = set(int(d) for s in specs if s[0] not in ("white", "bias") for d in s[3])
    return dict(lml=lml, dtheta=dtheta, dnoise=sum_dR + c * N / (2 * s2), dZ=dZ, woodbury_vector=v, woodbury_inv=woodbury_inv,
                dL_dKmm=dL_dKmm, dL_dKnm=dL_dKnm, dL_dR=dL_dR, dL_dKdiag=bt(al) * dL_dR, sigma_star=sigma_star, Kmm=Kmm, Lm=Lm,
                dZ_zero_cols=[q for q in range(D) if q not in active])


predict = SL.predict
rel_err = SL.rel_err
bound = SL.bound


def judge(got, ref_ld, ref_64, kappa):
    """`sparse_ld.judge` over this file's quantities: ({q: (err, bound)}, [what failed])"""
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


class RestatementContext(object):
    """Stands for `_lib.SparseContext` in the CPU tests: a PEP call answered by this restatement in fp64, and a log of the
    calls.  Part lists arrive as the package sends them ((kind, ARD, theta, active_dims or None, term))."""
    FETCH_DLDKMM, FETCH_WOODBURY_INV, FETCH_LM, FETCH_KMM = 0, 1, 2, 3
    sharded = False
    fail_infos = ()                  # info codes the next calls report before one succeeds (the jitter ladder)

    def __init__(self, device=0):
        self.log, self.jitters = [], []
        self.res = None
        self._fail = list(self.fail_infos)

    def set_data(self, X, Y):
        self.X, self.Y = np.array(X, dtype=np.float64), np.array(Y, dtype=np.float64)
        self.N, self.D = self.X.shape
        self.res = None
        self.log.append(("set_data", self.X.shape, self.Y.shape))

    def _specs(self, specs):
        return [(s[0], int(bool(s[1])), np.asarray(s[2], np.float64), np.arange(self.D) if s[3] is None else np.asarray(s[3]),
                 int(s[4]) if len(s) > 4 else 0) for s in specs]

    def pep(self, specs, Z, noise_variance, alpha, jitter, want_stage_ms=False):
        self.log.append(("pep", np.shape(Z), float(noise_variance), float(alpha)))
        self.jitters.append(float(jitter))
        if self._fail:
            return self._fail.pop(0), {}
        self.specs, self.Z = self._specs(specs), np.array(Z, dtype=np.float64)
        self.res = r = pep(self.specs, self.X, Z, self.Y, noise_variance, alpha, dt=np.float64, jitter=jitter)
        return 0, dict(lml=float(r["lml"]), dnoise=float(r["dnoise"]), sum_dL_dR=float(np.sum(r["dL_dR"])), dL_dR=r["dL_dR"],
                       dtheta=r["dtheta"], dZ=r["dZ"], woodbury_vector=r["woodbury_vector"])

    def fetch(self, which):
        self.log.append(("fetch", which))
        return self.res[{0: "dL_dKmm", 1: "woodbury_inv", 2: "Lm", 3: "Kmm"}[which]]

    def fetch_dL_dKnm(self, row0, nrows):
        self.log.append(("fetch_dL_dKnm", row0, nrows))
        return self.res["dL_dKnm"][row0:row0 + nrows]

    def predict(self, specs, Xnew, full_cov=False, want_var=True):
        self.log.append(("predict", np.shape(Xnew), bool(full_cov)))
        return predict(self._specs(specs), self.Z, np.asarray(Xnew, np.float64), self.res, full_cov, dt=np.float64)


# ---- the reference fixtures (tests/golden/pep, written by tools/make_golden_pep.py) -------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pep")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*_n*_m*_d*.npz")))
FIXTURE_QUANTITIES = ("lml", "dtheta", "dZ", "dL_dKmm", "dL_dKnm", "dL_dKdiag", "dL_dthetaL", "woodbury_vector", "woodbury_inv",
                      "pred_mu", "pred_var", "pred_cov")


def load_fixture(name):
    fx = dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))
    fx["name"] = name
    fx["specs"] = [(s[0], int(s[1]), np.array(s[2], dtype=np.float64), np.array(s[3], dtype=np.int32), int(s[4]))
                   for s in json.loads(str(fx["specs"]))]
    fx["method"], fx["alpha"], fx["noise"] = str(fx["method"]), float(fx["alpha"]), float(fx["noise"])
    return fx


def make_inference(fx, device=0):
    """the package's inference object of a fixture"""
    import gpy_amd
    return gpy_amd.FITC(device=device) if fx["method"] == "fitc" else gpy_amd.PEP(fx["alpha"], device=device)


def restate_fixture(fx, dt=np.float64):
    """the whole evaluation of a fixture by this restatement in `dt`, under the fixtures' names"""
    r = pep(fx["specs"], fx["X"], fx["Z"], fx["Y"], fx["noise"], fx["alpha"], dt=dt)
    mu, var = predict(fx["specs"], fx["Z"], fx["Xs"], r, False, dt=dt)
    return dict(lml=r["lml"], dtheta=r["dtheta"], dZ=r["dZ"], dL_dKmm=r["dL_dKmm"], dL_dKnm=r["dL_dKnm"], dL_dKdiag=r["dL_dKdiag"],
                dL_dthetaL=np.atleast_1d(r["dnoise"]), woodbury_vector=r["woodbury_vector"], woodbury_inv=r["woodbury_inv"],
                pred_mu=mu, pred_var=var, pred_cov=predict(fx["specs"], fx["Z"], fx["Xs"], r, True, dt=dt)[1], Kmm=r["Kmm"])


# ---- the shape sweep of tests/test_gpu_pep.py ---------------------------------------------------------------------------------
FAMILIES = ("m_edge", "n_edge", "d_edge", "alpha", "kernels", "stale", "chunks")


def _case(family, kern, N, M, D, alpha, variant=0):
    name = "%s-%s-n%d_m%d_d%d-a%g" % (family, kern, N, M, D, alpha) + ("-v%d" % variant if variant else "")
    return dict(name=name, family=family, kern=kern, N=N, M=M, D=D, Dy=1, alpha=alpha, het=False, variant=variant,
                blocked=family == "chunks")


def _cases():
    out = []
    # M edges: the tile padding | m == mp | the first persistent Kmm launch | three tiles
    out += [_case("m_edge", "rbf_ard", 257, M, 2, 1.0) for M in (1, 127, 128, 129, 257)]
    # N edges: the 128-row GEMM padding, the Gram rounding, the chunk granule; N < M on purpose
    out += [_case("n_edge", "matern52_iso", N, 65, 3, 0.5) for N in (1, 2, 127, 128, 129, 255, 256, 257, 2049)]
    # D: the fused gradient pass up to 16, the unfused one above, ARD groups of 32 dimensions
    out += [_case("d_edge", "rbf_ard", 193, 65, D, 1.0) for D in (1, 16, 17, 32, 33)]
    out += [_case("alpha", "matern32_ard", 257, 65, 3, a) for a in (1.0, 0.5, 0.05)]
    out += [_case("kernels", k, 257, 129, 3, 0.5) for k in ("rbf+white", "prod", "rbf_ard_subset")]
    # stale state: one context, no set_data between the members (the seed leaves M and the kernel out)
    out += [_case("stale", "rbf_ard", 257, 129, 3, 1.0), _case("stale", "rbf_ard", 257, 65, 3, 0.5)]
    # several chunks (blocked reference)
    out += [_case("chunks", "rbf_ard", 262145, 128, 2, 1.0), _case("chunks", "prod", 262145, 65, 3, 0.5)]
    return out


CASES = _cases()
BY_NAME = dict((c["name"], c) for c in CASES)
PLAIN = [c["name"] for c in CASES if not c["blocked"]]
BLOCKED = [c["name"] for c in CASES if c["blocked"]]
SWEEP = [c["name"] for c in CASES if c["family"] != "stale"]
STALE = [c["name"] for c in CASES if c["family"] == "stale"]
DETERMINISM = "kernels-prod-n257_m129_d3-a0.5"


def make_case(name):
    """the seeded inputs of one case, drawn as `sparse_ld.make_case` draws them (Z on a jittered regular grid over at most three
    active dimensions, lengthscales 0.75 grid spacings there, X uniform in the unit cube, D = 1 centred at the origin); one
    output column, one noise variance of 0.05 Kdiag"""
    c = dict(BY_NAME[name])
    N, M, D, kern = c["N"], c["M"], c["D"], c["kern"]
    gdims = [0, 2] if kern == "rbf_ard_subset" else list(range(min(D, 3)))
    g = SL._grid_side(M, len(gdims))
    fam, kix = FAMILIES.index(c["family"]), SL.KERNELS.index(kern)
    data = np.random.default_rng([101, fam, N, D] + ([] if c["family"] == "stale" else [M, kix]))
    X = data.uniform(0.0, 1.0, (N, D))
    freq = data.uniform(1.0, 3.0, (D, 1))
    rng = np.random.default_rng([101, fam, N, M, D, kix, int(round(1000 * c["alpha"])), c["variant"]])
    Z = rng.uniform(0.0, 1.0, (M, D))
    sites = rng.permutation(g ** len(gdims))[:M]
    for a, q in enumerate(gdims):
        Z[:, q] = ((sites // g ** a) % g + 0.5 + rng.uniform(-0.2, 0.2, M)) / g
    specs = SL._specs(kern, D, g, gdims, rng, c["variant"])
    scale = float(np.max(KL.Kdiag(specs, X[:1], np.float64)))
    noise = 0.05 * scale
    nstd = np.sqrt(0.05 if c["family"] == "stale" else noise)
    Y = np.sin(2.0 * np.pi * X[:, :min(D, 3)] @ freq[:min(D, 3)]) + nstd * data.standard_normal((N, 1))
    shift = 0.5 if D == 1 else 0.0
    c.update(specs=specs, parts=SL.oracle_parts(specs), X=X - shift, Z=Z - shift, Y=Y, noise=noise, scale=scale,
             Xs1=rng.uniform(0.0, 1.0, (1, D)) - shift, Xs129=rng.uniform(0.0, 1.0, (129, D)) - shift,
             block=(N // 3, min(N - N // 3, max(1, N // 2), 300)))
    if c["blocked"]:
        c["block"] = (131000, 300)                               # across the chunk boundary at 131072 + 128 k
    return c


def with_predictions(res, c, fn):
    for tag in ("1", "129"):
        res["mu" + tag], res["var" + tag] = fn(c["Xs" + tag], False)
        res["cov" + tag] = fn(c["Xs" + tag], True)[1]
    r0, nr = c["block"]
    res["dL_dKnm_block"] = res["dL_dKnm"][r0:r0 + nr]
    return res


_MEMO = {}


def reference(name):
    """(case, long-double reference (blocked for the `chunks` family), fp64 restatement, kappa = cond2(Kmm + 1e-6 I) in fp64) of
    a case, computed once per process and not to be modified"""
    if name not in _MEMO:
        KL.require_ld()
        c = make_case(name)
        ref = pep(c["specs"], c["X"], c["Z"], c["Y"], c["noise"], c["alpha"], block=4096 if c["blocked"] else None)
        with_predictions(ref, c, lambda Xs, full: predict(c["specs"], c["Z"], Xs, ref, full))
        r64 = pep(c["specs"], c["X"], c["Z"], c["Y"], c["noise"], c["alpha"], dt=np.float64, block=4096 if c["blocked"] else None)
        with_predictions(r64, c, lambda Xs, full: predict(c["specs"], c["Z"], Xs, r64, full, dt=np.float64))
        kappa = float(np.linalg.cond(KL.f64(ref["Kmm"])))
        _MEMO[name] = (c, ref, r64, kappa)
    return _MEMO[name]
