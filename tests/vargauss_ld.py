"""Long-double (x86 80-bit) restatement of one VarGauss evaluation on the exact context (C-ABI mi355gp_vargauss_forward /
mi355gp_vargauss_backward, csrc/vargauss.hip with its k_vg_* kernels) and the shape sweep that
tests/test_oracle_vargauss.py (CPU) and tests/test_gpu_vargauss.py (GPU) share.  Written from the formulas of the reference
(GPy/inference/latent_function_inference/var_gauss.py:34-65), not from the device's identities:

    A = I + diag(beta) K diag(beta), Ai = A^-1 from the Cholesky factor L_A, log det A, tr Ai                      :36-39
    m = K alpha                                                                                                     :35
    Sigma = K - (beta K)^T Ai (beta K) = (K^-1 + diag(beta^2))^-1, var = diag Sigma                                 :40-41
    dalpha = K dF_dm - m                                                                                            :48,55,59
    dF_db_j = -2 beta_j sum_i Sigma_ij^2 dF_dv_i;  dKL_db_j = sum_i beta_i K_ij (Ai - Ai Ai)_ij;  dbeta = dF_db - dKL_db   :51,56-60
    dL_dK = alpha dF_dm^T + (T o dF_dv) T^T - (alpha alpha^T + beta beta^T o (Ai - Ai Ai)) / 2,  T_ij = Ai_ij beta_i / beta_j   :63-65
    G = (dL_dK + dL_dK^T) / 2, dtheta = sum G o dK/dtheta (kern_ld.dtheta, with its per-entry cond)
    woodbury_inv = diag(beta) Ai diag(beta);  mu* = Kx^T alpha,  cov* = K** - (beta Kx)^T Ai (beta Kx)               posterior.py:198-262

Sigma is formed as K - V^T V with V = L_A^-1 diag(beta) K in BOTH working types, so the fp64 floor e64 of var and dbeta does not
carry the cancellation of the reference's beta^-2 - Ai_ii beta^-2 (which the device does not use either).  Every function takes
`dt`, np.longdouble or np.float64; the judge is the session's own (laplace_ld.judge's rule): err(q) = max |got - q_ld| / max |q_ld|
<= max(32 e64(q), 256 eps64 kappa), kappa = cond2(A) in fp64, every dtheta entry within kern_ld.grad_tol.  No product goes through `@`.

Inputs (`make_case`): X and the labels from laplace_np.two_class as laplace_ld seeds them (row 1 of X equal to row 0); alpha, dF_dm
and dF_dv seeded random vectors (the judged map is the device call, not a likelihood); beta by the variant:
    ""        |beta| in [0.3, 1.5], a third of the entries negative
    pos       beta in [0.3, 1.5]
    mixed     |beta| in [0.3, 1.5], half of the entries negative
    small     mixed, |beta| = 1e-2 on a tenth of the sites
    big       mixed, |beta| in [0.3, 7] (7 on one site)
    dfdv      mixed; dF_dv exactly zero on a tenth of the sites, of both signs on the rest
Every case must keep cond2(A) <= 1e4 (tests/test_oracle_vargauss.py asserts it on the CPU)."""
import numpy as np

import kern_ld as KL
import laplace_ld as LL
import laplace_np as LP
import osc_ld  # noqa: F401  (registers ExpQuadCosine on kern_ld)
import sparse_ld as SL

LD = KL.LD
EPS64 = KL.EPS64
POINTS_M = (1, 127, 128, 129, 257)
SYMMETRIC = ("K", "woodbury_inv", "dL_dK", "dL_dK_exact")
QUANT = ("m", "var", "logdet", "trAi", "dalpha", "dbeta", "K", "woodbury_inv", "dL_dK", "dL_dK_exact")

_a, _mv, _gram, _gram_lower = LL._a, LL._mv, LL._gram, LL._gram_lower


def forward(K, alpha, beta, dt=LD):
    """dict(m, var, logdet, trAi, ma, L, Ai, Sigma, A) of reference :34-41,54"""
    K, al, b = _a(K, dt), _a(alpha, dt), _a(beta, dt)
    n = K.shape[0]
    A = b[:, None] * K * b[None, :]
    A[np.arange(n), np.arange(n)] += dt(1)
    L = KL.cholesky(A, LL.CHOL_MAX)
    Ai = _gram_lower(KL.solve_lower(L, np.eye(n, dtype=dt)))
    V = KL.solve_lower(L, b[:, None] * K)
    Sigma = K - _gram(V)
    m = _mv(K, al)
    return dict(m=m, var=np.diag(Sigma).copy(), logdet=2 * np.sum(np.log(np.diag(L))), trAi=np.sum(np.diag(Ai)), ma=np.sum(m * al),
                L=L, Ai=Ai, Sigma=Sigma, A=A)


def backward(specs, X, K, alpha, beta, fw, dF_dm, dF_dv, dt=LD, exact=False):
    """dict(dalpha, dbeta, dL_dK (symmetrised), dtheta, dtheta_cond, woodbury_inv) of reference :48-65.  `exact`: the dF_dv term as
    the derivative of the bound, T diag(dF_dv) T^T (d var_i / dK = T[:, i] T[:, i]^T), where the reference has (T o dF_dv) T^T with
    dF_dv a column, i.e. the rows of T scaled (:65); `test_oracle_vargauss` shows by central differences which one is the gradient"""
    K, al, b, g, v = _a(K, dt), _a(alpha, dt), _a(beta, dt), _a(dF_dm, dt), _a(dF_dv, dt)
    Ai, Sigma = fw["Ai"], fw["Sigma"]
    dalpha = _mv(K, g) - fw["m"]
    dF_db = -2 * np.sum(Sigma * Sigma * (v[:, None] * b[None, :]), axis=0)
    A_A2 = Ai - KL.matmul(Ai, Ai)
    dKL_db = np.sum((K * b[:, None]) * A_A2, axis=0)
    T = Ai * b[:, None] / b[None, :]
    dF_dK = al[:, None] * g[None, :] + KL.matmul(T * (v[None, :] if exact else v[:, None]), T.T.copy())
    dKL_dK = (al[:, None] * al[None, :] + b[:, None] * b[None, :] * A_A2) / 2
    dL_dK = dF_dK - dKL_dK
    G = (dL_dK + dL_dK.T) / 2
    val, cond = KL.dtheta(specs, G, X, None, dt)
    return dict(dalpha=dalpha, dbeta=dF_db - dKL_db, dL_dK=G, dtheta=val, dtheta_cond=cond, woodbury_inv=b[:, None] * Ai * b[None, :])


def predict(specs, X, Xs, alpha, beta, L_A, full_cov=False, dt=LD):
    """Posterior._raw_predict with woodbury_vector alpha and woodbury_inv diag(beta) Ai diag(beta) (posterior.py:198-262)"""
    Kx = KL.K(specs, X, Xs, dt) + np.zeros((np.shape(X)[0], np.shape(Xs)[0]), dtype=dt)
    mu = np.sum(Kx * _a(alpha, dt)[:, None], axis=0)[:, None]
    T = KL.solve_lower(_a(L_A, dt), _a(beta, dt)[:, None] * Kx)
    if full_cov:
        return mu, KL.K(specs, Xs, None, dt) - _gram(T)
    return mu, (KL.Kdiag(specs, Xs, dt) - np.sum(T * T, axis=0))[:, None]


# ---- the judge ---------------------------------------------------------------------------------------------------------------
def pred_q(c):
    return tuple(q + str(M) for M in c["Ms"] for q in ("mu", "var", "cov"))


def judged(c):
    return QUANT + pred_q(c)


def judge(c, got, ref, r64, kappa):
    """laplace_ld.judge's rule on the quantities of a VarGauss case.  Returns ({q: (err, bound)}, [what failed])."""
    figs, bad = {}, []
    for q in judged(c):
        if q not in got:
            bad.append("%s: missing" % q)
            continue
        e, b = SL.rel_err(got[q], ref[q]), SL.bound(q, ref, r64, kappa)
        figs[q] = (e, b)
        if not e <= b:
            bad.append("%s: %.3e > %.3e" % (q, e, b))
    for q in ("dtheta", "dtheta_exact"):
        if q not in got or np.shape(got[q]) != np.shape(ref[q]):
            bad.append("%s: missing or of another length" % q)
            continue
        tol = KL.grad_tol(ref[q], r64[q], ref[q + "_cond"])
        err = np.abs(_a(got[q], LD) - ref[q])
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(tol > 0, err / np.where(tol > 0, tol, 1), np.where(err > 0, np.inf, 0))
        k = int(np.argmax(ratio))
        figs[q] = (float(ratio[k]), 1.0)                           # the worst entry in units of its own bound
        if not KL.grad_ok(got[q], ref[q], tol):
            bad.append("%s: entry %d off by %.3e, its bound %.3e" % (q, k, float(err[k]), float(tol[k])))
    return figs, bad


# ---- the shape sweep -------------------------------------------------------------------------------------------------------
FAMILIES = ("n_edge", "signs", "kernels", "points", "stale")
N_EDGE = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513)
SIGNS = ("pos", "mixed", "small", "big", "dfdv")
KERNELS = ("rbf_ard_d32", "rbf_ard_d33", "matern32_ard_subset", "stdperiodic_ard", "ratquad_ard", "linear+bias", "mlp_x_rbf",
           "expquadcosine_d1", "rbf_x_coreg_r1")


def _case(family, kern, N, variant="", **kw):
    name = "%s-%s-n%d" % (family, kern, N) + ("-" + variant if variant else "")
    c = dict(name=name, family=family, kern=kern, N=N, variant=variant, Ms=(1, 129))
    c.update(kw)
    return c


def _cases():
    out = [_case("n_edge", "rbf_ard+bias", N) for N in N_EDGE]
    out += [_case("signs", "rbf_iso", N, v) for N in (129, 257) for v in SIGNS]
    out += [_case("kernels", k, 65 if "coreg" in k else 129) for k in KERNELS]
    out += [_case("points", "rbf+bias", 129, Ms=POINTS_M)]
    # one context, no fresh one between the steps (tests/test_gpu_vargauss.py runs a Laplace round and an exact evaluation between them)
    out += [_case("stale", "rbf_ard+bias", 257, "step1"), _case("stale", "rbf_ard+bias", 129, "step2"),
            _case("stale", "rbf_ard+bias", 129, "step3"), _case("stale", "rbf_ard+bias", 129, "step4")]
    return out


CASES = _cases()
BY_NAME = dict((c["name"], c) for c in CASES)
assert len(BY_NAME) == len(CASES)
NAMES = dict((f, [c["name"] for c in CASES if c["family"] == f]) for f in FAMILIES)
DETERMINISM = "signs-rbf_iso-n257-small"


def _specs(kern, rng):
    if kern == "expquadcosine_d1":
        return [("expquadcosine", 0, np.array([1.3, 0.9, 1.7]), np.arange(1, dtype=np.int32), 0)], 1, None
    return LL._specs(kern, rng)


def make_case(name):
    """the seeded inputs of one case: dict(specs, dev_specs, X, Y, alpha, beta, dF_dm, dF_dv, Xs{M}, ...)"""
    c = dict(BY_NAME[name])
    N, kern, variant = c["N"], c["kern"], c["variant"]
    stale = c["family"] == "stale"
    seed = [40 + FAMILIES.index(c["family"]), N] + ([] if stale else [CASES.index(BY_NAME[name])])
    rng = np.random.default_rng(seed)
    specs, D, icol = _specs(kern, np.random.default_rng([7, len(kern), N]))
    X, Y = LP.two_class(N, D, int(rng.integers(1 << 30)), sep=2.0)
    if icol is not None:
        X[:, icol] = rng.integers(0, LL.COREG_P, N)
    if any(s[0] in ("linear", "mlp") for s in specs) and N >= 3:
        X[N // 2, :icol] = 0.0                                    # an all-zero input row (kern_ld.make_case)
    if N >= 2:
        X[1] = X[0]
    aux = np.random.default_rng(seed + [99] + ([CASES.index(BY_NAME[name])] if stale else []))
    mag = aux.uniform(0.3, 1.5, N)
    neg = aux.random(N) < (0.0 if variant == "pos" else 1.0 / 3.0 if variant in ("", "step1", "step2", "step3", "step4") else 0.5)
    if variant == "small":
        mag[aux.permutation(N)[:max(N // 10, 1)]] = 1e-2
    elif variant == "big":
        mag = aux.uniform(0.3, 7.0, N)
        mag[int(aux.integers(N))] = 7.0
    beta = np.where(neg, -mag, mag)
    dF_dv = -0.3 * np.abs(aux.standard_normal(N)) + 0.05 * aux.standard_normal(N)
    if variant == "dfdv":
        dF_dv = 0.3 * aux.standard_normal(N)
        dF_dv[aux.permutation(N)[:max(N // 10, 1)]] = 0.0
    c.update(specs=specs, dev_specs=KL.cabi_specs(specs), X=np.ascontiguousarray(X), Y=Y, alpha=0.4 * aux.standard_normal(N),
             beta=beta, dF_dm=0.5 * aux.standard_normal(N), dF_dv=dF_dv)
    for M in c["Ms"]:
        Xs = aux.standard_normal((M, X.shape[1]))
        if icol is not None:
            Xs[:, icol] = aux.integers(0, LL.COREG_P, M) if M > 1 else 1
        c["Xs%d" % M] = Xs
    return c


def evaluate(c, dt=LD):
    """every quantity of a case from the restatement in the working type (and "A": the matrix that was factored)"""
    specs, X = c["specs"], c["X"]
    K = KL.K(specs, X, None, dt) + np.zeros((c["N"], c["N"]), dtype=dt)
    fw = forward(K, c["alpha"], c["beta"], dt)
    out = dict((q, fw[q]) for q in ("m", "var", "logdet", "trAi", "ma"))
    out["K"], out["A"] = K, fw["A"]
    out.update(backward(specs, X, K, c["alpha"], c["beta"], fw, c["dF_dm"], c["dF_dv"], dt))
    ex = backward(specs, X, K, c["alpha"], c["beta"], fw, c["dF_dm"], c["dF_dv"], dt, exact=True)
    out.update(dL_dK_exact=ex["dL_dK"], dtheta_exact=ex["dtheta"], dtheta_exact_cond=ex["dtheta_cond"])
    for M in c["Ms"]:
        Xs = c["Xs%d" % M]
        out["mu%d" % M], out["var%d" % M] = predict(specs, X, Xs, c["alpha"], c["beta"], fw["L"], False, dt)
        out["cov%d" % M] = predict(specs, X, Xs, c["alpha"], c["beta"], fw["L"], True, dt)[1]
    return out


_MEMO = {}


def reference(name):
    """(case, long-double reference, fp64 restatement, cond2(A) in fp64) of a case, computed once per process, not to be modified"""
    if name not in _MEMO:
        KL.require_ld()
        c = make_case(name)
        ref, r64 = evaluate(c, LD), evaluate(c, np.float64)
        _MEMO[name] = (c, ref, r64, float(np.linalg.cond(KL.f64(r64["A"]))))
    return _MEMO[name]


# ---- the fixtures of the reference's own VarGauss.inference (tools/make_golden_vargauss.py) ---------------------------------
import os  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vargauss")
FIXTURES = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz") and f != "toy_1d_optimize.npz") if os.path.isdir(GOLDEN) else []
FIXTURE_Q = ("m", "var", "lml", "dalpha", "dbeta", "dL_dK_sym", "dL_dthetaL", "dtheta", "pred_mu", "pred_var", "pred_cov")
# max |restatement - fixture| / max |fixture| found over the eight fixtures, times ten (tests/test_oracle_vargauss.py)
FIXTURE_TOL = {"m": 1.5e-14, "var": 1.2e-13, "lml": 2.2e-15, "dalpha": 6.6e-15, "dbeta": 3.9e-13, "dL_dK_sym": 7.0e-14,
               "dL_dthetaL": 5.4e-15, "dtheta": 5.6e-15, "pred_mu": 1.1e-14, "pred_var": 2.7e-13, "pred_cov": 2.7e-13}


def load_fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    g = {k: z[k] for k in z.files}
    g["specs"] = LP.P.load_specs(g["specs"])
    g["lik"] = str(g["lik"])
    return g


def fixture_kernel(specs):
    """the gpy_amd kernel of a fixture's part list (a sum of single parts, the last one White)"""
    import gpy_amd
    k = None
    for s in specs:
        leaf = gpy_amd.White(len(s[3]), s[2][0], active_dims=s[3]) if s[0] == "white" else LP.gpy_amd_kernel([s])
        k = leaf if k is None else k + leaf
    return k


def fixture_likelihood(g):
    import gpy_amd
    th = g["lik_theta"]
    return {"bernoulli": lambda: gpy_amd.Bernoulli(), "gaussian": lambda: gpy_amd.Gaussian(variance=th[0]),
            "studentt": lambda: gpy_amd.StudentT(deg_free=th[1], sigma2=th[0]), "poisson": lambda: gpy_amd.Poisson()}[g["lik"]]()


def restate_fixture(g, dt=LD, exact=False):
    """the quantities of FIXTURE_Q from the restatement; the likelihood's variational expectations are the package's (fp64 host
    work on three N-vectors, the same in every working type)"""
    specs, X = g["specs"], g["X"]
    al, b = g["alpha"][:, 0], g["beta"]
    N = X.shape[0]
    K = KL.K(specs, X, None, dt) + np.zeros((N, N), dtype=dt)
    fw = forward(K, al, b, dt)
    F, dF_dm, dF_dv, dF_dth = fixture_likelihood(g).variational_expectations(g["Y"], KL.f64(fw["m"])[:, None], KL.f64(fw["var"])[:, None])
    bw = backward(specs, X, K, al, b, fw, dF_dm[:, 0], dF_dv[:, 0], dt, exact=exact)
    KLd = (fw["logdet"] + fw["trAi"] - N + fw["ma"]) / 2
    out = dict(m=fw["m"][:, None], var=fw["var"], lml=np.sum(_a(F, dt)) - KLd, dalpha=bw["dalpha"][:, None], dbeta=bw["dbeta"],
               dL_dK_sym=bw["dL_dK"], dtheta=bw["dtheta"], dL_dthetaL=dF_dth.sum(1).sum(1) if dF_dth is not None else np.zeros(0))
    out["pred_mu"], out["pred_var"] = predict(specs, X, g["Xs"], al, b, fw["L"], False, dt)
    out["pred_cov"] = predict(specs, X, g["Xs"], al, b, fw["L"], True, dt)[1]
    return out
