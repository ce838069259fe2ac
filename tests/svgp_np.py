"""NumPy restatement of the SVGP evaluation in the chunked order of the device (gpy_amd/csrc/svgp.hip), generic in the working
type so that it also runs in long double (x86 80-bit).  Written from the formulas of the reference:

    svgp.py:16-23 (q(u)), :37-42 (Kmm, its inverse), :45-51 (mu, v), :54-60 (KL and its gradients), :84-100 (dF terms),
    :111-117 (the sums, dL_dchol), core/svgp.py:57-65 (kernel and inducing-input gradients), posterior.py:190-248 (prediction).

Everything kernel-shaped comes from tests/kern_ld.py, as in tests/sparse_ld.py, whose judge and case format this module shares.
Two calls bracket the likelihood's quadrature, like the device's session:

    forward:   M x M: Kmm (no 1e-8 term), Lm, Kmmi, S_d = L_d L_d^T, S_d^-1, Kmmi m, KL
               rows : A^T = Kfu Kmmi, mu = A^T m, v_d = rowsum((A^T L_d)^2) + Kdiag - rowsum(A^T * Kfu)
    backward:  rows : A dF_dmu, AdvA_d = A diag(dF_dv_d) A^T, G = dF_dmu (Kmmi m)^T + sum_d diag(dF_dv_d) A^T tmp_d and its
                      theta / Z reductions;  M x M: dL_dKmm, dL_dm, dL_dchol

In the blocked mode (`block=4096`, for N above 262144) the row blocks and their products are formed in fp64 and accumulated
across blocks in long double; everything M x M stays in long double."""
import glob
import json
import os

import numpy as np

import kern_ld as KL
import sparse_ld as SLD
from sparse_ld import _diag_weights

LD = KL.LD
JUDGED = ("mu", "v", "KL", "dtheta", "dZ", "dL_dm", "dL_dchol", "woodbury_vector", "woodbury_inv", "mu1", "var1", "cov1", "mu129",
          "var129", "cov129")


def _inv_from_factor(L, I):
    Li = KL.solve_lower(L, I)
    return KL.matmul(Li.T, Li)


def forward(specs, X, Z, q_mean, q_L, dt=LD, block=None, max_n=257, jitter=0.0):
    """q_mean: M x L; q_L: L x M x M lower-triangular factors.  Returns the state dict: mu, v (N x L), KL, logdet_Kmm,
    logdet_S, Kmm, Kmmi, Kmmim (= woodbury_vector), S, Si, woodbury_inv (M x M x L) and what `backward` needs."""
    X, Z = np.asarray(X, np.float64), np.asarray(Z, np.float64)
    N, M, Lq = X.shape[0], Z.shape[0], np.shape(q_mean)[1]
    bt = np.float64 if block else dt
    mm = (lambda a, b: a @ b) if block else KL.matmul
    step = int(block) if block else max(N, 1)
    I = np.eye(M, dtype=dt)
    lvm = KL.leaves(specs, Z, None, dt)
    Kmm = KL.K(specs, Z, None, dt, lvm) + dt(jitter) * I                     # svgp.py:37: no 1e-8 term
    Lm = KL.cholesky(Kmm, max_n)
    Kmmi = _inv_from_factor(Lm, I)
    Kmmi = (Kmmi + Kmmi.T) / 2
    m = KL._a(q_mean, dt)
    Ls = [np.tril(KL._a(q_L[d], dt)) for d in range(Lq)]
    S = [KL.matmul(L, L.T) for L in Ls]
    Si = [_inv_from_factor(L, I) for L in Ls]
    logdetS = np.array([2 * np.sum(np.log(np.abs(np.diag(L)))) for L in Ls], dtype=dt)
    logdetKmm = 2 * np.sum(np.log(np.diag(Lm)))
    Kmmim = KL.matmul(Kmmi, m)
    KLs = [-logdetS[d] / 2 - dt(M) / 2 + logdetKmm / 2 + np.sum(Kmmi * S[d]) / 2 + np.sum(m[:, d] * Kmmim[:, d]) / 2
           for d in range(Lq)]
    mu, v = np.zeros((N, Lq), dtype=bt), np.zeros((N, Lq), dtype=bt)
    Kmmi_b, m_b, Ls_b = KL._a(Kmmi, bt), KL._a(m, bt), [KL._a(L, bt) for L in Ls]
    for r0 in range(0, N, step):
        r1 = min(r0 + step, N)
        Kfu = KL._a(KL.K(specs, X[r0:r1], Z, bt), bt) + np.zeros((r1 - r0, M), dtype=bt)
        At = mm(Kfu, Kmmi_b)
        mu[r0:r1] = mm(At, m_b)
        q = KL._a(KL.Kdiag(specs, X[r0:r1], bt), bt) - np.sum(At * Kfu, axis=1)
        for d in range(Lq):
            U = mm(At, Ls_b[d])
            v[r0:r1, d] = np.sum(U * U, axis=1) + q
    winv = np.dstack([Kmmi - KL.matmul(KL.matmul(Kmmi, S[d]), Kmmi) for d in range(Lq)])
    return dict(specs=specs, X=X, Z=Z, dt=dt, bt=bt, block=block, mm=mm, step=step, lvm=lvm, mu=mu, v=v, KL=sum(KLs), logdet_Kmm=logdetKmm,
                logdet_S=logdetS, Kmm=Kmm, Lm=Lm, Kmmi=Kmmi, Kmmim=Kmmim, woodbury_vector=Kmmim, woodbury_inv=winv, S=S, Si=Si, Ls=Ls,
                m=m)


def backward(st, dF_dmu, dF_dv):
    """dF_dmu, dF_dv: N x L, already times batch_scale.  dict(dtheta (concatenated in part order, with the
    update_gradients_diag term), dZ, dL_dm, dL_dchol (L x M x M, lower triangles), dL_dKmm, dL_dKnm (N x M, the transpose of
    the reference's dL_dKmn), dL_dKdiag, dZ_zero_cols)."""
    specs, X, Z, dt, bt, mm, step = st["specs"], st["X"], st["Z"], st["dt"], st["bt"], st["mm"], st["step"]
    N, D = X.shape
    M, Lq = st["m"].shape
    I = np.eye(M, dtype=dt)
    Kmmi, Kmmim, S, Si, Ls = st["Kmmi"], st["Kmmim"], st["S"], st["Si"], st["Ls"]
    dFm, dFv = KL._a(dF_dmu, bt), KL._a(dF_dv, bt)
    tmp = [2 * (KL.matmul(S[d], Kmmi) - I) for d in range(Lq)]                # svgp.py:92-93
    Kmmi_b, Kmmim_b, tmp_b = KL._a(Kmmi, bt), KL._a(Kmmim, bt), [KL._a(t, bt) for t in tmp]
    Admu = np.zeros((M, Lq), dtype=dt)
    AdvA = [np.zeros((M, M), dtype=dt) for _ in range(Lq)]
    npar = sum(KL.n_params(s) for s in specs)
    dtheta, dZ = np.zeros(npar, dtype=dt), np.zeros((M, D), dtype=dt)
    first = np.cumsum([0] + [KL.n_params(s) for s in specs])[:-1]
    G_all = np.zeros((N, M), dtype=bt)
    for r0 in range(0, N, step):
        r1 = min(r0 + step, N)
        Xb = X[r0:r1]
        lv = KL.leaves(specs, Xb, Z, bt)
        Kfu = KL._a(KL.K(specs, Xb, Z, bt, lv), bt) + np.zeros((r1 - r0, M), dtype=bt)
        At = mm(Kfu, Kmmi_b)
        Admu += KL._a(mm(At.T, dFm[r0:r1]), dt)                                # svgp.py:86
        G = mm(dFm[r0:r1], Kmmim_b.T)                                          # svgp.py:95 (as N x M)
        for d in range(Lq):
            U = At * dFv[r0:r1, d][:, None]                                    # Adv_d^T (svgp.py:85)
            AdvA[d] += KL._a(mm(At.T, U), dt)                                  # svgp.py:88
            G = G + mm(U, tmp_b[d])                                            # svgp.py:96-97
        G_all[r0:r1] = G
        dtheta += KL._a(KL.dtheta(specs, G, Xb, Z, bt, lv)[0], dt)
        dZ += KL._a(KL.gradients_X(specs, G.T, Z, Xb, bt)[0], dt)
        w0 = np.sum(dFv[r0:r1], axis=1)                                         # dL_dKdiag (svgp.py:117)
        for i, wd in enumerate(_diag_weights(specs, Xb, bt)):
            dtheta[first[i]] += np.sum(KL._a(w0 * wd, dt))
    # ---- M x M (svgp.py:58-60,88-91,112-115) -------------------------------------------------------------------------------
    sumA = sum(AdvA[1:], AdvA[0])
    t = KL.matmul(sum((KL.matmul(AdvA[d], S[d]) for d in range(1, Lq)), KL.matmul(AdvA[0], S[0])), Kmmi)
    dF_dKmm = -KL.matmul(Admu, Kmmim.T) + sumA - t - t.T
    dF_dKmm = (dF_dKmm + dF_dKmm.T) / 2
    sumS = sum(S[1:], S[0])
    dKL_dKmm = dt(Lq) * Kmmi / 2 - KL.matmul(KL.matmul(Kmmi, sumS), Kmmi) / 2 - KL.matmul(Kmmim, Kmmim.T) / 2
    dL_dKmm = dF_dKmm - dKL_dKmm
    dL_dm = Admu - Kmmim
    dL_dchol = np.stack([np.tril(2 * KL.matmul(AdvA[d] - (Kmmi - Si[d]) / 2, Ls[d])) for d in range(Lq)])
    dtheta += KL.dtheta(specs, dL_dKmm, Z, None, dt, st["lvm"])[0]
    dZ += KL.gradients_X(specs, dL_dKmm, Z, None, dt, st["lvm"])[0]
    active = set(int(d) for s in specs if s[0] not in ("white", "bias") for d in s[3])
    return dict(dtheta=dtheta, dZ=dZ, dL_dm=dL_dm, dL_dchol=dL_dchol, dL_dKmm=dL_dKmm, dL_dKnm=G_all, dL_dKdiag=np.sum(dFv, axis=1),
                dZ_zero_cols=[q for q in range(D) if q not in active])


def predict(st, Xs, full_cov=False):
    """(mu (M* x L), var (M* x L, clipped at 1e-15) or cov (M* x M* x L)) at Xs (posterior.py:220-248)"""
    specs, Z, dt = st["specs"], st["Z"], st["dt"]
    Kx = KL.K(specs, Z, Xs, dt)
    mu = KL.matmul(Kx.T, st["woodbury_vector"])
    Wi = st["woodbury_inv"]
    if full_cov:
        Kxx = KL.K(specs, Xs, None, dt)
        return mu, np.dstack([Kxx - KL.matmul(Kx.T, KL.matmul(Wi[:, :, d], Kx)) for d in range(Wi.shape[2])])
    kd = KL.Kdiag(specs, Xs, dt)
    var = np.stack([kd - np.sum(KL.matmul(Wi[:, :, d].T, Kx) * Kx, axis=0) for d in range(Wi.shape[2])], axis=1)
    return mu, np.maximum(var, dt(1e-15))


def evaluate(specs, X, Z, q_mean, q_L, dF, dt=LD, block=None, Xs=(), jitter=0.0):
    """forward, backward with the given (dF_dmu, dF_dv) and predictions at the point sets of `Xs` ({tag: points}) in one dict
    with the names of JUDGED"""
    st = forward(specs, X, Z, q_mean, q_L, dt=dt, block=block, jitter=jitter)
    out = dict(st)
    out.update(backward(st, dF[0], dF[1]))
    for tag, P in dict(Xs).items():
        out["mu" + tag], out["var" + tag] = predict(st, P, False)
        out["cov" + tag] = predict(st, P, True)[1]
    return out


class RestatementContext(object):
    """Stands for `_lib.SparseContext` in the CPU tests: the SVGP session answered by this restatement in fp64, and a log of
    the calls.  Part lists arrive as the package sends them ((kind, ARD, theta, active_dims or None, term))."""
    sharded = False
    fail_info = 0

    def __init__(self, device=0):
        self.log, self.jitters = [], []
        self.st = None

    def set_data(self, X, Y):
        self.X, self.Y = np.array(X, dtype=np.float64), np.array(Y, dtype=np.float64)
        self.N, self.D = self.X.shape
        self.st = None
        self.log.append(("set_data", self.X.shape))

    def _specs(self, specs):
        return [(s[0], int(bool(s[1])), np.asarray(s[2], np.float64), np.arange(self.D) if s[3] is None else np.asarray(s[3]),
                 int(s[4]) if len(s) > 4 else 0) for s in specs]

    def svgp_forward(self, specs, Z, q_mean, q_chol, extra_jitter=0.0, want_stage_ms=False):
        self.log.append(("svgp_forward", np.shape(Z), np.shape(q_mean), np.shape(q_chol)))
        self.jitters.append(float(extra_jitter))
        if self.fail_info:
            return self.fail_info, {}
        self.M = np.shape(Z)[0]
        self.st = forward(self._specs(specs), self.X, Z, q_mean, q_chol, dt=np.float64, jitter=extra_jitter)
        return 0, dict(mu=self.st["mu"], v=self.st["v"], KL=float(self.st["KL"]), logdet_Kmm=float(self.st["logdet_Kmm"]),
                       logdet_S=self.st["logdet_S"])

    def svgp_backward(self, dF_dmu, dF_dv, want_stage_ms=False):
        self.log.append(("svgp_backward", np.shape(dF_dmu), np.shape(dF_dv)))
        assert self.st is not None, "svgp_backward without svgp_forward"
        self.dF = (np.array(dF_dmu), np.array(dF_dv))
        r = backward(self.st, dF_dmu, dF_dv)
        return dict(dtheta=r["dtheta"], dZ=r["dZ"], dL_dm=r["dL_dm"], dL_dchol=r["dL_dchol"])

    def svgp_predict(self, specs, Xnew, full_cov=False, want_var=True):
        self.log.append(("svgp_predict", np.shape(Xnew), bool(full_cov)))
        return predict(self.st, np.asarray(Xnew, np.float64), full_cov)

    def svgp_woodbury(self, want_inv=True):
        return self.st["woodbury_vector"], self.st["woodbury_inv"] if want_inv else None


# ---- the reference fixtures (tests/golden/svgp, written by tools/make_golden_svgp.py) ----------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "svgp")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*_l[12]_*.npz")))
FIXTURE_QUANTITIES = ("bound", "mu", "v", "dtheta", "dZ", "dL_dm", "dL_dchol", "dL_dKmm", "dL_dKmn", "dL_dKdiag", "dL_dthetaL",
                      "woodbury_vector", "woodbury_inv", "pred_mu", "pred_var", "pred_cov")


def load_fixture(name):
    fx = dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))
    fx["name"] = name
    fx["specs"] = [(s[0], int(s[1]), np.array(s[2], dtype=np.float64), np.array(s[3], dtype=np.int32), int(s[4]))
                   for s in json.loads(str(fx["specs"]))]
    fx["lik"], fx["batch_scale"] = str(fx["lik"]), float(fx["batch_scale"])
    return fx


def make_likelihood(fx):
    """the package's likelihood of a fixture"""
    import gpy_amd
    th = fx["lik_theta"]
    return {"gaussian": lambda: gpy_amd.Gaussian(variance=th[0]), "bernoulli": gpy_amd.Bernoulli,
            "studentt": lambda: gpy_amd.StudentT(deg_free=th[1], sigma2=th[0]), "poisson": gpy_amd.Poisson}[fx["lik"]]()


def make_kernel(fx, device=0):
    """the package's kernel of a fixture's part list"""
    import gpy_amd
    cls = {"rbf": gpy_amd.RBF, "matern52": gpy_amd.Matern52, "matern32": gpy_amd.Matern32, "exponential": gpy_amd.Exponential}
    groups, seen = [], {}
    for kind, ard, th, dims, term in fx["specs"]:
        dims = [int(d) for d in dims]
        if kind in ("white", "bias"):
            k = {"white": gpy_amd.White, "bias": gpy_amd.Bias}[kind](len(dims), variance=th[0], active_dims=dims)
        else:
            k = cls[kind](len(dims), variance=th[0], lengthscale=th[1:] if ard else th[1], ARD=bool(ard), active_dims=dims)
        if term == 0:
            groups.append([k])
        elif term in seen:
            seen[term].append(k)
        else:
            seen[term] = [k]
            groups.append(seen[term])
    tops = [g[0] if len(g) == 1 else gpy_amd.Prod(g) for g in groups]
    return tops[0] if len(tops) == 1 else gpy_amd.Add(tops)


def restate_fixture(fx, dt=np.float64):
    """the whole evaluation of a fixture by this restatement in `dt`, with the package's likelihood for the quadrature (fp64),
    under the fixtures' names"""
    from gpy_amd.util import choleskies
    qL = choleskies.flat_to_triang(fx["q_chol"])
    st = forward(fx["specs"], fx["X"], fx["Z"], fx["q_mean"], qL, dt=dt)
    lik = make_likelihood(fx)
    F, dFm, dFv, dFt = lik.variational_expectations(fx["Y"], KL.f64(st["mu"]), KL.f64(st["v"]))
    bs = fx["batch_scale"]
    bw = backward(st, dFm * bs, dFv * bs)
    mu, var = predict(st, fx["Xs"], False)
    out = dict(bound=np.sum(KL._a(F, dt)) * dt(bs) - st["KL"], mu=st["mu"], v=st["v"], dtheta=bw["dtheta"], dZ=bw["dZ"], dL_dm=bw["dL_dm"],
               dL_dchol=choleskies.triang_to_flat(bw["dL_dchol"]), dL_dKmm=bw["dL_dKmm"], dL_dKmn=bw["dL_dKnm"].T,
               dL_dKdiag=bw["dL_dKdiag"], dL_dthetaL=np.zeros(0) if dFt is None else dFt.sum(1).sum(1) * bs,
               woodbury_vector=st["woodbury_vector"], woodbury_inv=st["woodbury_inv"], pred_mu=mu, pred_var=var,
               pred_cov=predict(st, fx["Xs"], True)[1], F=F, dF_dmu=dFm, dF_dv=dFv, dF_dtheta=dFt)
    return out


# ---- the shape sweep of tests/test_gpu_svgp.py -------------------------------------------------------------------------------
def _case(family, kern, N, M, D, L, lik="gaussian", variant=0):
    name = "%s-%s-n%d_m%d_d%d_l%d-%s" % (family, kern, N, M, D, L, lik) + ("-v%d" % variant if variant else "")
    return dict(name=name, family=family, kern=kern, N=N, M=M, D=D, L=L, lik=lik, variant=variant, blocked=family == "chunks")


def _cases():
    out = []
    # M edges: 64-wide covariance tiles, m < mp | m == mp (128) | the first padded second tile (129) | three tiles (257)
    out += [_case("m_edge", "rbf_ard", 257, M, 2, 1) for M in (1, 127, 128, 129, 257)]
    # N edges: the 128-row GEMM padding, one row, the 2048-row chunk granule; N < M on purpose
    out += [_case("n_edge", "matern52_iso", N, 65, 3, 2) for N in (1, 2, 127, 128, 129, 257, 2049)]
    # latent functions: the per-latent GEMMs and the register block of the row-reduction kernel (16 = its bound)
    out += [_case("latents", "rbf_ard", 129, 65, 2, L) for L in (3, 16)]
    # D: the fused gradient pass up to 16, the unfused one above, two 32-dimension record groups at 33
    out += [_case("dispatch", "rbf_ard", 193, 65, D, 1) for D in (1, 16, 17, 33)]
    # sums and products: rbf + white (unfused), rbf[0,1] x matern32[2] + white, rbf on columns 0 and 2 of three
    out += [_case("kernels", k, 257, 65, 3, 2) for k in ("rbf+white", "prod", "rbf_ard_subset")]
    # signed weights: Student-t's dF_dv changes sign over the rows
    out += [_case("signed", "rbf_ard", 257, 65, 2, 1, lik="studentt")]
    out += [_case("signed", "prod", 129, 65, 3, 2, lik="bernoulli")]
    # stale state: one context, no set_data between the members (the seed leaves M, L and the variant out of X)
    out += [_case("stale", "rbf_ard", 257, 129, 3, 2), _case("stale", "rbf_ard", 257, 128, 3, 1),
            _case("stale", "rbf_ard", 257, 128, 3, 1, variant=1)]
    # several chunks (blocked reference)
    out += [_case("chunks", "rbf_ard", 262145, 65, 2, 1)]
    return out


CASES = _cases()
BY_NAME = dict((c["name"], c) for c in CASES)
PLAIN = [c["name"] for c in CASES if c["family"] not in ("chunks", "stale")]
STALE = [c["name"] for c in CASES if c["family"] == "stale"]
BLOCKED = [c["name"] for c in CASES if c["blocked"]]
DETERMINISM = "kernels-prod-n257_m65_d3_l2-gaussian"
FAMILIES = ("m_edge", "n_edge", "latents", "dispatch", "kernels", "signed", "stale", "chunks")
LIKS = ("gaussian", "studentt", "bernoulli")


def make_case(name):
    """the seeded inputs of one case, in the manner of sparse_ld.make_case: Z on a jittered regular grid over the first (at most
    three) active dimensions with lengthscales of 0.75 grid spacings there (SVGP adds no 1e-8 to Kmm), X uniform in the unit
    cube, q_mean = 0.5 randn, L_d = I + 0.1 tril(randn) / sqrt(M) with one negative diagonal entry (the reference takes |.|)."""
    c = dict(BY_NAME[name])
    N, M, D, L, kern = c["N"], c["M"], c["D"], c["L"], c["kern"]
    gdims = [0, 2] if kern == "rbf_ard_subset" else list(range(min(D, 3)))
    g = SLD._grid_side(M, len(gdims))
    fam = FAMILIES.index(c["family"])
    data = np.random.default_rng([fam, N, D] + ([] if c["family"] == "stale" else [M, L, SLD.KERNELS.index(kern)]))
    X = data.uniform(0.0, 1.0, (N, D))
    rng = np.random.default_rng([fam, N, M, D, L, SLD.KERNELS.index(kern), LIKS.index(c["lik"]), c["variant"]])
    Z = rng.uniform(0.0, 1.0, (M, D))
    sites = rng.permutation(g ** len(gdims))[:M]
    for a, q in enumerate(gdims):
        Z[:, q] = ((sites // g ** a) % g + 0.5 + rng.uniform(-0.2, 0.2, M)) / g
    specs = SLD._specs(kern, D, g, gdims, rng, c["variant"])
    q_mean = 0.5 * rng.standard_normal((M, L))
    q_L = np.stack([np.eye(M) + 0.1 * np.tril(rng.standard_normal((M, M))) / np.sqrt(M) for _ in range(L)])
    q_L[0, M // 2, M // 2] *= -1.0
    freq = rng.uniform(1.0, 3.0, (min(D, 3), L))
    f = np.sin(2.0 * np.pi * X[:, :min(D, 3)] @ freq)
    if c["lik"] == "bernoulli":
        Y = (rng.random(f.shape) < 0.5 * (1.0 + np.tanh(2.0 * f))).astype(np.float64)
    else:
        Y = f + 0.3 * rng.standard_normal(f.shape)
        if c["lik"] == "studentt":                               # a tenth of the rows far out: there dF_dv is positive
            idx = rng.choice(N, max(N // 10, 1), replace=False)
            Y[idx] += 4.0
    shift = 0.5 if D == 1 else 0.0
    c.update(specs=specs, X=X - shift, Z=Z - shift, Y=Y, q_mean=q_mean, q_L=q_L, batch_scale=1.0 + 0.5 * (L % 2),
             Xs={"1": rng.uniform(0.0, 1.0, (1, D)) - shift, "129": rng.uniform(0.0, 1.0, (129, D)) - shift})
    return c


def case_likelihood(c):
    import gpy_amd
    return {"gaussian": lambda: gpy_amd.Gaussian(variance=0.09), "bernoulli": gpy_amd.Bernoulli,
            "studentt": lambda: gpy_amd.StudentT(deg_free=4.0, sigma2=0.09)}[c["lik"]]()


_MEMO = {}


def reference(name):
    """(case, (dF_dmu, dF_dv) times batch_scale, long-double evaluation (blocked for the `chunks` family), fp64 evaluation,
    kappa = cond2(Kmm) in fp64) of a case, computed once per process and not to be modified.  The dF come from the package's
    likelihood at the long-double mu and v rounded to fp64: all three evaluations, and the device, are given the same ones."""
    if name not in _MEMO:
        KL.require_ld()
        c = make_case(name)
        block = 4096 if c["blocked"] else None
        st = forward(c["specs"], c["X"], c["Z"], c["q_mean"], c["q_L"], dt=LD, block=block)
        _, dFm, dFv, _ = case_likelihood(c).variational_expectations(c["Y"], KL.f64(st["mu"]), KL.f64(st["v"]))
        dF = (np.ascontiguousarray(dFm * c["batch_scale"]), np.ascontiguousarray(dFv * c["batch_scale"]))
        ref = dict(st)
        ref.update(backward(st, dF[0], dF[1]))
        for tag, P in c["Xs"].items():
            ref["mu" + tag], ref["var" + tag] = predict(st, P, False)
            ref["cov" + tag] = predict(st, P, True)[1]
        r64 = evaluate(c["specs"], c["X"], c["Z"], c["q_mean"], c["q_L"], dF, dt=np.float64, block=block, Xs=c["Xs"])
        kappa = float(np.linalg.cond(KL.f64(ref["Kmm"])))
        _MEMO[name] = (c, dF, ref, r64, kappa)
    return _MEMO[name]


def judge(got, ref_ld, ref_64, kappa):
    """sparse_ld.judge over this module's JUDGED: err(q) = max |got - q_ld| / max |q_ld| <= max(32 e64(q), 256 eps64 kappa); the
    dZ columns outside every part's active_dims must be exactly zero.  Returns ({q: (err, bound)}, [what failed])."""
    figs, bad = {}, []
    for q in JUDGED:
        if q not in got or got[q] is None:
            continue
        e, b = SLD.rel_err(got[q], ref_ld[q]), SLD.bound(q, ref_ld, ref_64, kappa)
        figs[q] = (e, b)
        if not e <= b:
            bad.append("%s: %.3e > %.3e" % (q, e, b))
    if "dZ" in got:
        for col in ref_ld.get("dZ_zero_cols", []):
            if np.any(np.asarray(got["dZ"])[:, col] != 0):
                bad.append("dZ column %d is outside every part's active_dims and must be exactly 0" % col)
    return figs, bad
