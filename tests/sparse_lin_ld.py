"""Long-double restatement of the sparse evaluations (VarDTC, PEP / FITC, SVGP) for expressions with a Linear part, and the
shape sweep that tests/test_oracle_sparse_lin.py (CPU) and tests/test_gpu_sparse_lin.py (GPU) share.

tests/sparse_ld.py, pep_np.py and svgp_np.py are right for Linear in everything but one term: they give the whole
`update_gradients_diag` sum of a leaf to its FIRST parameter, which is the variance only where Kdiag is a variance.  For Linear,
Kdiag_n = sum_q variance_q x_nq^2 (linear.py:84-85) and the term is per variance (linear.py:100-105):

    d/dvariance_q  sum_n w_n (other factors)_n Kdiag_n  =  sum_n w_n (other factors)_n x_nq^2        (their sum for one variance)

So this helper runs those restatements with "linear" admitted and the Linear leaves' share of that term set to exactly zero,
and adds the term per kind itself (`linear_diag_term`), in the working type.  Kdiag by point (psi0 of VarDTC, Knn of PEP, the
marginal variance of SVGP, the predictive variance) is what kern_ld.Kdiag has given all along.

Inputs (`make_case`): sparse_ld.make_case's design -- Z on the jittered grid, gridded lengthscales 0.75 spacings -- centred about
the origin (x - 1/2), plus an ARD Linear part with unequal variances that sum to 1 (one variance: 1).  Centred, cond2(Kmm +
1e-8 I) stays below 1e3 for every case; `reference` asserts that cap.  The fp64 figure of the judge (`sparse_ld.bound`) is THIS
restatement run at dt = float64: oracle/sparse_oracle.py does not know Linear.
"""
import contextlib
import glob
import json
import os

import numpy as np

import kern_ld as KL
import pep_np as PN
import sparse_ld as SL
import svgp_np as SN

LD = KL.LD
EPS64 = KL.EPS64
KAPPA_CAP = 1e3
JUDGED = SL.JUDGED


@contextlib.contextmanager
def linear_admitted():
    """the three restatements take "linear"; a Linear leaf's share of their first-parameter diag term is exactly zero"""
    sup, dw = SL.SUPPORTED, SL._diag_weights

    def diag_weights(specs, X, dt):
        return [np.zeros_like(w) if specs[i][0] == "linear" else w for i, w in enumerate(dw(specs, X, dt))]
    SL.SUPPORTED = tuple(sup) + ("linear",)
    SL._diag_weights = SN._diag_weights = diag_weights
    try:
        yield
    finally:
        SL.SUPPORTED, SL._diag_weights, SN._diag_weights = sup, dw, dw


def linear_diag_term(specs, X, w, dt=LD):
    """update_gradients_diag(w, X) of the Linear leaves, concatenated in theta order (zero for every other leaf): per active
    dimension sum_n w_n (the other factors' Kdiag)_n x_nq^2, their sum over the dimensions for one shared variance"""
    X = np.asarray(X, np.float64)
    first = np.cumsum([0] + [KL.n_params(s) for s in specs])
    out = np.zeros(first[-1], dtype=dt)
    w = KL._a(np.asarray(w), dt).ravel()
    others = SL._diag_weights(specs, X, dt)
    for i, s in enumerate(specs):
        if s[0] != "linear":
            continue
        x2 = np.square(KL._a(X[:, np.asarray(s[3], dtype=int)], dt))
        g = np.sum((w * others[i])[:, None] * x2, axis=0)
        if s[1]:
            out[first[i]:first[i + 1]] = g
        else:
            out[first[i]] = np.sum(g)
    return out


def vardtc(specs, X, Z, R, noise, dt=LD, block=None, **kw):
    """`sparse_ld.vardtc` for expressions with Linear parts; dL_dKdiag_n = -Dy beta_n / 2 (sparse_gp.py:110)"""
    with linear_admitted():
        r = SL.vardtc(specs, X, Z, R, noise, dt=dt, block=block, **kw)
    N, Dy = np.shape(X)[0], np.shape(R)[1]
    beta = 1 / np.maximum(KL._a(np.atleast_1d(np.asarray(noise, np.float64)).ravel(), dt), dt(SL.JITTER))
    r["dL_dKdiag"] = -Dy * (beta + np.zeros(N, dtype=dt)) / 2
    r["dtheta"] = r["dtheta"] + linear_diag_term(specs, X, r["dL_dKdiag"], dt)
    return r


def pep(specs, X, Z, Y, noise, alpha, dt=LD, block=None, **kw):
    """`pep_np.pep` likewise; dL_dKdiag = alpha dL_dR (pep.py:85)"""
    with linear_admitted():
        r = PN.pep(specs, X, Z, Y, noise, alpha, dt=dt, block=block, **kw)
    r["dtheta"] = r["dtheta"] + linear_diag_term(specs, X, r["dL_dKdiag"], dt)
    return r


def svgp(specs, X, Z, q_mean, q_L, dF, dt=LD, Xs=(), jitter=0.0):
    """`svgp_np.evaluate` likewise; dL_dKdiag = dF_dv.sum(1) (svgp.py:117)"""
    with linear_admitted():
        r = SN.evaluate(specs, X, Z, q_mean, q_L, dF, dt=dt, Xs=Xs, jitter=jitter)
    r["dtheta"] = r["dtheta"] + linear_diag_term(specs, X, r["dL_dKdiag"], dt)
    return r


predict = SL.predict
rel_err = SL.rel_err
bound = SL.bound
judge = SL.judge


# ---- the shape sweep ---------------------------------------------------------------------------------------------------------
def linear_part(dims, ard, term=0):
    """an ARD Linear part with unequal variances that sum to 1 over `dims`, or one variance of 1 / len(dims) per dimension's
    worth (Kdiag of the same size either way)"""
    dims = np.asarray(dims, dtype=np.int32)
    w = 1.0 + 0.5 * np.arange(dims.size)
    return ("linear", 1, w / w.sum(), dims, term) if ard else ("linear", 0, np.array([1.0 / dims.size]), dims, term)


# form: what the expression is, around the base kernel of sparse_ld (None: no stationary part)
FORMS = ("rbf_ard+linear_ard", "rbf_ard+linear_iso", "matern32_ard+linear_ard", "matern32_ard+linear_iso", "linear_lone",
         "linear*rbf+white", "rbf_ard+linear*bias", "subset", "zero_row")
FAMILIES = ("m_edge", "n_edge", "dispatch", "forms", "noise", "families", "stale", "chunks", "kdiag")


def _case(family, form, N, M, D, Dy, het=False, variant=0):
    name = "%s-%s-n%d_m%d_d%d_dy%d-%s" % (family, form, N, M, D, Dy, "het" if het else "hom") + ("-v%d" % variant if variant else "")
    return dict(name=name, family=family, form=form, N=N, M=M, D=D, Dy=Dy, het=het, variant=variant, blocked=family == "chunks")


def _cases():
    out = []
    # the 64-column tiles of the Linear pass: one ragged | one short | one full | two | m == mp | three tiles
    out += [_case("m_edge", "rbf_ard+linear_ard", 257, M, 2, 1) for M in (1, 63, 64, 65, 128, 129, 257)]
    # a row tile, a row split, the chunk granule, N < M
    out += [_case("n_edge", "rbf_ard+linear_ard", N, 65, 3, 2) for N in (1, 2, 63, 64, 65, 129, 257, 2049)]
    # D = 16: the last shape of k_grad_cols_lin, the rank term in registers (Dy = 4) and per element (5); D = 17: the first with
    # the weights formed in memory; D = 33: two ARD groups
    out += [_case("dispatch", "matern32_ard+linear_%s" % a, 193, 65, D, Dy) for D, Dy in ((16, 4), (16, 5), (17, 1), (33, 1), (1, 1))
            for a in ("ard", "iso")]
    out += [_case("forms", "linear_lone", 129, 3, 4, 1), _case("forms", "linear*rbf+white", 257, 65, 3, 2),
            _case("forms", "rbf_ard+linear*bias", 257, 65, 3, 1), _case("forms", "subset", 257, 65, 3, 2),
            _case("forms", "zero_row", 129, 65, 2, 1)]
    out += [_case("noise", "rbf_ard+linear_ard", N, M, 3, Dy, het=True) for N, M in ((257, 65), (129, 128)) for Dy in (1, 3)]
    # one context, no set_data between: stationary only -> rbf + linear -> stationary only, the same part count -> other theta
    out += [_case("stale", "rbf_ard+bias", 257, 65, 3, 2), _case("stale", "rbf_ard+linear_ard", 257, 65, 3, 2),
            _case("stale", "rbf_ard+bias", 257, 65, 3, 2, variant=1), _case("stale", "rbf_ard+linear_ard", 257, 65, 3, 2, variant=1)]
    out += [_case("chunks", "rbf_ard+linear_ard", 262145, 65, 3, 1)]
    return out


CASES = _cases()
BY_NAME = dict((c["name"], c) for c in CASES)
PLAIN = [c["name"] for c in CASES if c["family"] not in ("stale", "chunks")]
STALE = [c["name"] for c in CASES if c["family"] == "stale"]
BLOCKED = [c["name"] for c in CASES if c["blocked"]]
DETERMINISM = "noise-rbf_ard+linear_ard-n257_m65_d3_dy3-het"
# the shapes the PEP / SVGP / EPDTC families run at: one m_edge, one dispatch (the fallback with the weights in memory)
FAMILY_SHAPES = ("m_edge-rbf_ard+linear_ard-n257_m129_d2_dy1-hom", "dispatch-matern32_ard+linear_ard-n193_m65_d17_dy1-hom")


def make_case(name):
    """the seeded inputs of one case: sparse_ld.make_case's for the stationary part of the form (its jittered grid for Z, its
    lengthscales, targets and noise), centred about the origin, with the Linear part(s) of the form added"""
    c = dict(BY_NAME[name])
    form, N, M, D, Dy = c["form"], c["N"], c["M"], c["D"], c["Dy"]
    base = {"linear_lone": None, "linear*rbf+white": "rbf_ard", "rbf_ard+linear*bias": "rbf_ard", "subset": "rbf_ard_subset",
            "zero_row": "rbf_ard"}.get(form, form.split("+")[0] if "linear" in form else form)
    allq = np.arange(D, dtype=np.int32)
    sfam = c["family"] if c["family"] in SL.FAMILIES else "subset"
    tmp = SL._case(sfam, base or "rbf_ard", N, M, D, Dy, het=c["het"], variant=c["variant"])
    old = SL.BY_NAME.get(tmp["name"])
    SL.BY_NAME[tmp["name"]] = tmp
    try:
        s = SL.make_case(tmp["name"])
    finally:
        if old is None:
            del SL.BY_NAME[tmp["name"]]
        else:
            SL.BY_NAME[tmp["name"]] = old
    shift = 0.0 if D == 1 else 0.5                               # (D = 1 is centred by sparse_ld already)
    X, Z, Xs1, Xs129 = (s[k] - shift for k in ("X", "Z", "Xs1", "Xs129"))
    if form == "linear_lone":
        specs = [linear_part(allq, 1)]
    elif form == "linear*rbf+white":
        rbf = s["specs"][0]
        specs = [linear_part(allq[:-1], 1, term=1), ("rbf", 0, np.array([1.3, float(rbf[2][-1])]), allq[-1:], 1),
                 ("white", 0, np.array([0.03]), allq, 0)]
    elif form == "rbf_ard+linear*bias":
        specs = list(s["specs"]) + [linear_part(allq, 1, term=1), ("bias", 0, np.array([0.7]), allq, 1)]
    elif form == "subset":
        specs = list(s["specs"]) + [linear_part([0, 2], 1)]
    elif form == "zero_row":
        specs = list(s["specs"]) + [linear_part(allq, 1)]
        X = X.copy()
        X[N // 2] = 0.0                                          # Kdiag of the Linear part is 0 there
    elif "linear" not in form:                                   # (the stationary-only members of the stale sequence)
        specs = list(s["specs"])
    else:
        specs = list(s["specs"]) + [linear_part(allq, form.endswith("_ard"))]
    c.update(specs=specs, X=np.ascontiguousarray(X), Z=np.ascontiguousarray(Z), R=s["R"], noise=s["noise"], Xs1=Xs1, Xs129=Xs129,
             block=s["block"] if c["blocked"] else (N // 3, max(1, N // 2)))
    return c


_MEMO = {}


def reference(name):
    """(case, long-double reference (blocked for `chunks`), this restatement at fp64, kappa = cond2(Kmm + 1e-8 I) <= 1e3) of a
    case, computed once per process and not to be modified"""
    if name not in _MEMO:
        KL.require_ld()
        c = make_case(name)
        blk = 4096 if c["blocked"] else None
        ref = vardtc(c["specs"], c["X"], c["Z"], c["R"], c["noise"], block=blk)
        SL._with_predictions(ref, c, lambda Xs, full: predict(c["specs"], c["Z"], Xs, ref, full))
        r64 = vardtc(c["specs"], c["X"], c["Z"], c["R"], c["noise"], dt=np.float64, block=blk)
        SL._with_predictions(r64, c, lambda Xs, full: predict(c["specs"], c["Z"], Xs, r64, full, dt=np.float64))
        kappa = float(np.linalg.cond(KL.f64(ref["Kmm"])))
        assert kappa <= KAPPA_CAP, "%s: cond2(Kmm + 1e-8 I) = %.3g exceeds the cap of the sweep" % (name, kappa)
        _MEMO[name] = (c, ref, r64, kappa)
    return _MEMO[name]


def family_inputs(c, L=1):
    """what the PEP and SVGP evaluations of a case need on top of it: one output column; q(u) = N(q_mean, q_L q_L^T) with L
    latent functions and signed weights (dF_dmu, dF_dv) for the backward pass, which is linear in them"""
    rng = np.random.default_rng([7, c["N"], c["M"], c["D"], L])
    M, N = c["M"], c["N"]
    q_L = np.stack([0.3 * np.eye(M) + 0.05 * np.tril(rng.standard_normal((M, M)), -1) / np.sqrt(M) for _ in range(L)])
    return dict(Y=np.ascontiguousarray(c["R"][:, :1]), q_mean=0.5 * rng.standard_normal((M, L)), q_L=q_L,
                dF=(rng.standard_normal((N, L)), -rng.uniform(0.2, 1.0, (N, L))))


# ---- the reference's own evaluations (tests/golden/sparse_lin/*.npz, written by tools/make_golden_sparse_lin.py) ------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sparse_lin")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))
# the tolerances the fixtures of the stationary kinds are held to (tests/test_gpu_sparse.py, test_gpu_pep.py, test_gpu_svgp.py):
# log marginal / bound 1e-9, gradients, Woodbury vector and predictive mean 1e-6, dL_dKmm and woodbury_inv 1e-4, predictive
# variance and covariance 1e-5
FIXTURE_TOL = dict(lml=1e-9, bound=1e-9, dL_dKmm=1e-4, woodbury_inv=1e-4, pred_var=1e-5, pred_cov=1e-5)
FIXTURE_TOL_DEFAULT = 1e-6


def load_fixture(name):
    fx = dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))
    fx["name"], fx["family"] = name, str(fx["family"])
    fx["specs"] = [(s[0], int(s[1]), np.array(s[2], dtype=np.float64), np.array(s[3], dtype=np.int32), int(s[4]))
                   for s in json.loads(str(fx["specs"]))]
    if fx["family"] == "epdtc":                                  # (the layout of tests/golden/epdtc: epdtc_np.load)
        for k in ("sweeps", "parallel_updates", "eta", "delta", "epsilon", "clamped"):
            fx[k] = fx[k].item()
        return fx
    fx["noise"] = np.asarray(fx["noise"], np.float64) if np.ndim(fx["noise"]) else float(fx["noise"])
    return fx


def make_kernel(fx):
    """the package's kernel of a fixture's part list (svgp_np.make_kernel with Linear leaves)"""
    import gpy_amd
    groups, seen = [], {}
    for kind, ard, th, dims, term in fx["specs"]:
        dims = [int(d) for d in dims]
        if kind == "linear":
            k = gpy_amd.Linear(len(dims), variances=th, ARD=bool(ard), active_dims=dims)
        else:
            k = SN.make_kernel(dict(specs=[(kind, ard, th, dims, 0)]))
        if term == 0:
            groups.append([k])
        elif term in seen:
            seen[term].append(k)
        else:
            seen[term] = [k]
            groups.append(seen[term])
    tops = [g[0] if len(g) == 1 else gpy_amd.Prod(g) for g in groups]
    return tops[0] if len(tops) == 1 else gpy_amd.Add(tops)


def epdtc_final(specs, X, Z, tau, v, lzt, dt=LD):
    """`epdtc_np.final` for expressions with Linear parts: this file's VarDTC with targets v / tau, precisions tau and no jitter
    on Kmm (expectation_propagation.py:482-492 passes Lm in, so var_dtc.py:93 adds none)"""
    tau, v = KL._a(tau, dt), KL._a(v, dt)
    keep = SL.JITTER
    SL.JITTER = 0.0
    try:
        r = vardtc(specs, X, Z, np.asarray(v / tau, dtype=np.float64)[:, None], np.asarray(1 / tau, dtype=np.float64), dt=dt,
                   max_n=1 << 20)
    finally:
        SL.JITTER = keep
    r["lml"] = r["lml"] + lzt
    return r


def restate_fixture(fx, dt=np.float64):
    """the quantities of a fixture from this file's restatement, under the fixture's names"""
    specs, X, Z, Y, Xs = fx["specs"], fx["X"], fx["Z"], fx["Y"], fx["Xs"]
    if fx["family"] == "epdtc":                                  # the whole trajectory with the recorded orders (epdtc_np.restate_fixture)
        import epdtc_np as E
        sign = np.where(Y[:, 0] == 1, 1.0, -1.0)
        Kmm, Kmn = E.covariances(specs, X, Z, dt)
        e = E.run(Kmm, Kmn, sign, orders=list(fx["orders"]), parallel=fx["parallel_updates"], eta=fx["eta"], delta=fx["delta"],
                  epsilon=fx["epsilon"], sweep=E.ref_sweep, dt=dt)
        r = epdtc_final(specs, X, Z, e["tau"], e["v"], e["log_Z_tilde"], dt)
        mu, var = predict(specs, Z, Xs, r, False, dt)
        return dict(lml=r["lml"], log_Z_tilde=e["log_Z_tilde"], tau_tilde=e["tau"], v_tilde=e["v"], cav_tau=e["cav_tau"],
                    cav_v=e["cav_v"], dtheta=r["dtheta"], dZ=r["dZ"], woodbury_vector=r["woodbury_vector"],
                    woodbury_inv=r["woodbury_inv"], dL_dKmm=r["dL_dKmm"], pred_mu=mu, pred_var=var, sweeps=e["sweeps"])
    if fx["family"] == "svgp":
        qL = fx["q_L"]
        with linear_admitted():
            st = SN.forward(specs, X, Z, fx["q_mean"], qL, dt=dt)
        r = svgp(specs, X, Z, fx["q_mean"], qL, (fx["dF_dmu"], fx["dF_dv"]), dt=dt, Xs={"s": Xs})
        flat = np.stack([np.asarray(r["dL_dchol"][d])[np.tril_indices(Z.shape[0])] for d in range(qL.shape[0])], axis=1)
        return dict(bound=np.sum(KL._a(fx["F"], dt)) - st["KL"], mu=r["mu"], v=r["v"], dtheta=r["dtheta"], dZ=r["dZ"], dL_dm=r["dL_dm"],
                    dL_dchol=flat, dL_dKmm=r["dL_dKmm"], dL_dKdiag=r["dL_dKdiag"], woodbury_vector=r["woodbury_vector"],
                    pred_mu=r["mus"], pred_var=r["vars"])
    if fx["family"] == "pep":
        r = pep(specs, X, Z, Y, fx["noise"], float(fx["alpha"]), dt=dt)
        extra = dict(dL_dthetaL=np.atleast_1d(r["dnoise"]))
    else:
        r = vardtc(specs, X, Z, Y, fx["noise"], dt=dt)
        extra = dict(dL_dthetaL=r["dnoise"] if np.ndim(r["dnoise"]) else np.atleast_1d(r["dnoise"]))
    mu, var = predict(specs, Z, Xs, r, False, dt)
    return dict(extra, lml=r["lml"], dtheta=r["dtheta"], dZ=r["dZ"], dL_dKmm=r["dL_dKmm"], dL_dKnm=r["dL_dKnm"],
                dL_dKdiag=r["dL_dKdiag"], woodbury_vector=r["woodbury_vector"], woodbury_inv=r["woodbury_inv"], pred_mu=mu,
                pred_var=var, pred_cov=predict(specs, Z, Xs, r, True, dt)[1])


def fixture_figures(got, fx):
    """{quantity: (max |got - fixture| / max |fixture|, its tolerance)} over what both hold"""
    out = {}
    for q, v in got.items():
        if q not in fx or v is None:
            continue
        ref = np.asarray(fx[q], dtype=np.float64)
        g = KL.f64(np.asarray(v)).reshape(ref.shape)
        out[q] = (float(np.abs(g - ref).max() / np.abs(ref).max()), FIXTURE_TOL.get(q, FIXTURE_TOL_DEFAULT))
    return out
