"""Long-double restatement of the sparse evaluation (VarDTC) for a sum of products that may hold Coregionalize factors (the
kernels `util.multioutput.ICM` / `LCM` build, reference `GPy/models/sparse_gp_coregionalized_regression.py`), and the shape sweep
that tests/test_oracle_sparse_coreg.py (CPU) and tests/test_gpu_sparse_coreg.py (GPU) share.

tests/sparse_ld.py is right for a Coregionalize factor in everything but one term, as it is for Linear (tests/sparse_lin_ld.py):
it gives the whole `update_gradients_diag` sum of a leaf to its FIRST parameter.  Kdiag of a Coregionalize leaf is
B[idx_n][idx_n] = sum_c W[idx_n][c]^2 + kappa[idx_n] (coregionalize.py:106-107), so the term goes to the row's own output
(coregionalize.py:145-151):

    d/dW[p][c]   sum_n w_n (other factors)_n Kdiag_n  =  2 W[p][c] sum_{n: idx_n = p} w_n (other factors)_n,
    d/dkappa[p]                                       =            sum_{n: idx_n = p} w_n (other factors)_n.

This helper runs sparse_ld.vardtc with "coregionalize" (and "linear") admitted and those leaves' share of the first-parameter
term set to exactly zero, and adds the term per kind itself, in the working type.  Everything else -- K, dK/dtheta in W and
kappa (through B), gradients_X (zero for the factor, coregionalize.py:153-154), Kdiag by point in psi0, the per-point noise
gradient and the predictive variance -- is kern_ld's and sparse_ld's own.  A part is kern_ld's: ("coregionalize", 100 rank + P,
[W.ravel(), kappa], [index column], term); the device takes B (`kern_ld.cabi_specs`) and returns S, which
`kern_ld.chain_coreg` takes to W and kappa.

Inputs (`make_case`): per output its share of the M inducing inputs on sparse_ld's jittered grid over the first <= 3 spatial
dimensions, lengthscales 0.75 grid spacings, W of order 0.4 next to kappa of order 0.7; cond2(Kmm + 1e-8 I) is asserted to stay
below 1e4 (`reference`).  The fp64 figure of the judge (`sparse_ld.bound`) is THIS restatement run at dt = float64.
"""
import contextlib
import glob
import json
import os

import numpy as np

import kern_ld as KL
import sparse_ld as SL
import sparse_lin_ld as LL

LD = KL.LD
EPS64 = KL.EPS64
KAPPA_CAP = 1e4
JUDGED = SL.JUDGED


@contextlib.contextmanager
def coreg_admitted():
    """sparse_ld takes "coregionalize" and "linear"; their leaves' share of its first-parameter diag term is exactly zero"""
    sup, dw = SL.SUPPORTED, SL._diag_weights

    def diag_weights(specs, X, dt):
        return [np.zeros_like(w) if specs[i][0] in ("linear", "coregionalize") else w for i, w in enumerate(dw(specs, X, dt))]
    SL.SUPPORTED = tuple(sup) + ("linear", "coregionalize")
    SL._diag_weights = diag_weights
    try:
        yield
    finally:
        SL.SUPPORTED, SL._diag_weights = sup, dw


def coreg_diag_term(specs, X, w, dt=LD):
    """update_gradients_diag(w, X) of the Coregionalize leaves in link order (W, then kappa; zero for every other leaf)"""
    X = np.asarray(X, np.float64)
    first = np.cumsum([0] + [KL.n_params(s) for s in specs])
    out = np.zeros(first[-1], dtype=dt)
    w = KL._a(np.asarray(w), dt).ravel()
    others = SL._diag_weights(specs, X, dt)
    for i, s in enumerate(specs):
        if s[0] != "coregionalize":
            continue
        P, r = s[1] % 100, s[1] // 100
        W = KL._a(s[2], dt)[:P * r].reshape(P, r)
        idx = X[:, int(s[3][0])].astype(int)
        small = np.array([np.sum((w * others[i])[idx == p]) for p in range(P)], dtype=dt)
        out[first[i]:first[i] + P * r] = (2 * W * small[:, None]).ravel()
        out[first[i] + P * r:first[i + 1]] = small
    return out


def vardtc(specs, X, Z, R, noise, dt=LD, block=None, **kw):
    """`sparse_ld.vardtc` for expressions with Coregionalize (and Linear) parts; dL_dKdiag_n = -Dy beta_n / 2 (sparse_gp.py:110)"""
    with coreg_admitted():
        r = SL.vardtc(specs, X, Z, R, noise, dt=dt, block=block, **kw)
    N, Dy = np.shape(X)[0], np.shape(R)[1]
    beta = 1 / np.maximum(KL._a(np.atleast_1d(np.asarray(noise, np.float64)).ravel(), dt), dt(SL.JITTER))
    r["dL_dKdiag"] = -Dy * (beta + np.zeros(N, dtype=dt)) / 2
    r["dtheta"] = r["dtheta"] + coreg_diag_term(specs, X, r["dL_dKdiag"], dt) + LL.linear_diag_term(specs, X, r["dL_dKdiag"], dt)
    cols = set(int(s[3][0]) for s in specs if s[0] == "coregionalize")
    other = set(int(d) for s in specs if s[0] not in ("white", "bias", "coregionalize") for d in s[3])
    r["dZ_zero_cols"] = sorted(set(r["dZ_zero_cols"]) | (cols - other))     # the index column: gradients_X is zero there
    return r


def objective(specs, X, Z, R, noise, dt=LD):
    """the bound alone (for central differences of the restatement's own objective)"""
    return vardtc(specs, X, Z, R, noise, dt=dt)["lml"]


predict = SL.predict
rel_err = SL.rel_err
bound = SL.bound
judge = SL.judge
cabi_specs = KL.cabi_specs
chain_coreg = KL.chain_coreg


def device_dtheta(specs, dev):
    """the device's concatenated gradient (S per Coregionalize part) in the restatement's link order (W, kappa)"""
    return chain_coreg(specs, np.asarray(dev, dtype=np.float64))


# ---- the shape sweep ---------------------------------------------------------------------------------------------------------
def coreg_part(P, col, rank=1, term=1, seed=0):
    """W of order 0.4 with mixed signs next to kappa of 0.6 .. 0.8: outputs that are correlated and a B of condition < 4"""
    rng = np.random.default_rng([11, P, rank, seed])
    W = 0.4 * rng.uniform(0.5, 1.0, (P, rank)) * np.where(rng.uniform(size=(P, rank)) < 0.3, -1.0, 1.0) / np.sqrt(rank)
    kappa = 0.6 + 0.2 * rng.uniform(size=P)
    return ("coregionalize", 100 * rank + P, np.concatenate([W.ravel(), kappa]), np.array([col], dtype=np.int32), term)


# form: the expression around a Coregionalize factor; `layout` how the rows carry their outputs
FORMS = ("icm_rbf_ard", "icm_rbf_iso", "icm_matern52", "icm_exponential", "icm_subset", "lcm2", "icm+bias+white", "coreg*bias",
         "linear*coreg", "rbf*bias*coreg", "icm_index_first", "rbf_only", "rbf+coreg")
LAYOUTS = ("sorted", "interleaved", "no_rows", "no_inducing")
FAMILIES = ("n_edge", "m_edge", "outputs", "dispatch", "noise", "stale", "chunks")


def _case(family, form, N, M, D, P, Dy=1, noise="hom", layout="sorted", variant=0):
    name = "%s-%s-n%d_m%d_d%d_p%d_dy%d-%s-%s" % (family, form, N, M, D, P, Dy, noise, layout) + ("-v%d" % variant if variant else "")
    return dict(name=name, family=family, form=form, N=N, M=M, D=D, P=P, Dy=Dy, noise_kind=noise, layout=layout, variant=variant,
                blocked=family == "chunks")


def _cases():
    out = []
    # rows: one | a tile short of, at and past 64 | five tiles | past the 2048-row chunk granule
    out += [_case("n_edge", "icm_rbf_ard", N, 33, 3, 2) for N in (1, 63, 64, 65, 257, 2049)]
    out += [_case("m_edge", "icm_rbf_ard", 257, M, 3, 2) for M in (1, 63, 64, 65, 129)]
    # outputs: P = 1 | 2 | 3 | 16; sorted with the output boundaries inside a tile (N_p = 65); idx = n mod P: every tile holds every
    # pair; an output with inducing points and no rows, and one with rows and no inducing point; the index column first
    out += [_case("outputs", "icm_rbf_ard", 65 * P, 33, 3, P) for P in (1, 2, 3)] + [_case("outputs", "icm_rbf_ard", 260, 48, 3, 16)]
    out += [_case("outputs", "icm_rbf_ard", 195, 33, 3, 3, layout=lay) for lay in ("interleaved", "no_rows", "no_inducing")]
    out += [_case("outputs", "icm_rbf_ard", 192, 48, 3, 16, layout="interleaved"), _case("outputs", "icm_index_first", 195, 33, 3, 3)]
    # total D = 2 | 16 | 17 (the product route serves every D; 17 is past what a pass fused over D <= 16 could take), one
    # lengthscale, a subset of the columns, two terms, a sum with Bias and White, no stationary factor, other stationary kinds,
    # a Coregionalize part that is a summand of its own (its weights are dL_dKnm and dL_dKmm themselves)
    out += [_case("dispatch", "icm_rbf_ard", 193, 33, D, 2) for D in (2, 16, 17)]
    out += [_case("dispatch", f, 193, 33, 3, 2) for f in ("icm_rbf_iso", "icm_subset", "lcm2", "icm+bias+white", "coreg*bias",
                                                           "icm_matern52", "icm_exponential", "linear*coreg", "rbf*bias*coreg",
                                                           "rbf+coreg")]
    out += [_case("noise", "icm_rbf_ard", 195, 33, 3, 3, noise="mixed"), _case("noise", "icm_rbf_ard", 195, 33, 3, 3, noise="het"),
            _case("noise", "icm_rbf_ard", 195, 33, 3, 3, Dy=3)]
    # one context, no set_data between: RBF alone -> ICM -> RBF alone (the same bytes as the first) -> ICM at other theta
    out += [_case("stale", "rbf_only", 195, 33, 3, 3), _case("stale", "icm_rbf_ard", 195, 33, 3, 3),
            _case("stale", "rbf_only", 195, 33, 3, 3), _case("stale", "icm_rbf_ard", 195, 33, 3, 3, variant=1)]
    out += [_case("chunks", "icm_rbf_ard", 262145, 33, 3, 2)]
    return out


CASES = _cases()
BY_NAME = dict((c["name"], c) for c in CASES)
PLAIN = [c["name"] for c in CASES if c["family"] not in ("stale", "chunks")]
STALE = [c["name"] for c in CASES if c["family"] == "stale"]
BLOCKED = [c["name"] for c in CASES if c["blocked"]]
DETERMINISM = "noise-icm_rbf_ard-n195_m33_d3_p3_dy1-mixed-sorted"


def _indices(n, P, layout, skip=None):
    """n output indices: sorted runs (as `build_XY` stacks them), or n mod P; `skip`: an output that gets none"""
    outs = [p for p in range(P) if p != skip]
    if layout == "interleaved":
        return np.array([outs[i % len(outs)] for i in range(n)], dtype=np.float64)
    return np.sort(np.array([outs[i * len(outs) // n] for i in range(n)], dtype=np.float64)) if n >= len(outs) else \
        np.array(outs[:n], dtype=np.float64)


def make_case(name):
    """the seeded inputs of one case: dict(specs (kern_ld's), X, Z, R, noise, Xs1, Xs129, idx_col, ...)"""
    c = dict(BY_NAME[name])
    N, M, D, P, Dy, form = c["N"], c["M"], c["D"], c["P"], c["Dy"], c["form"]
    col = 0 if form == "icm_index_first" else D - 1
    sp = [q for q in range(D) if q != col]                       # the spatial columns
    Ds = len(sp)
    gd = sp[:1] if form == "icm_subset" else sp[:min(Ds, 3)]    # the gridded columns: what the stationary factor sees
    fam = FAMILIES.index(c["family"])
    data = np.random.default_rng([3, fam, N, D, P, Dy, LAYOUTS.index(c["layout"])])
    rng = np.random.default_rng([5, fam, N, M, D, P, FORMS.index(form), c["variant"]])
    X = data.uniform(-0.5, 0.5, (N, D))
    X[:, col] = _indices(N, P, c["layout"], skip=P - 1 if c["layout"] == "no_rows" else None)
    zi = _indices(M, P, "sorted", skip=0 if c["layout"] == "no_inducing" else None)
    Z = rng.uniform(-0.5, 0.5, (M, D))
    Z[:, col] = zi
    g = 1
    # per output its own jittered grid (g: the finest of them); without a Coregionalize factor all M share one grid
    for sel in ([np.ones(M, dtype=bool)] if form in ("rbf_only", "rbf+coreg") else [zi == p for p in range(P)]):
        mp_ = int(np.sum(sel))
        if mp_ == 0:
            continue
        gp = SL._grid_side(mp_, len(gd))
        g = max(g, gp)
        sites = rng.permutation(gp ** len(gd))[:mp_]
        for a, q in enumerate(gd):
            Z[sel, q] = ((sites // gp ** a) % gp + 0.5 + rng.uniform(-0.2, 0.2, mp_)) / gp - 0.5
    scale = 1.0 + 0.2 * c["variant"]

    def ls(dims, ard):
        v = np.array([0.75 / g * rng.uniform(0.9, 1.1) if q in gd else 4.0 * np.sqrt(D) for q in dims])
        return scale * (v if ard else v[:1])

    def stat(kind, dims, ard, term, var=1.3):
        return (kind, int(ard), np.concatenate([[var * scale], ls(dims, ard)]), np.array(dims, dtype=np.int32), term)
    allq = np.arange(D, dtype=np.int32)
    if form in ("icm_rbf_ard", "icm_index_first"):
        specs = [stat("rbf", sp, 1, 1), coreg_part(P, col)]
    elif form == "icm_rbf_iso":
        specs = [stat("rbf", sp, 0, 1), coreg_part(P, col)]
    elif form == "icm_matern52":
        specs = [stat("matern52", sp, 1, 1, 1.1), coreg_part(P, col)]
    elif form == "icm_exponential":
        specs = [stat("exponential", sp, 0, 1, 0.8), coreg_part(P, col)]
    elif form == "icm_subset":
        specs = [stat("rbf", sp[:1], 1, 1), coreg_part(P, col, rank=2)]
    elif form == "lcm2":
        specs = [stat("rbf", sp, 1, 1), coreg_part(P, col, term=1), stat("matern32", sp, 0, 2, 0.7), coreg_part(P, col, rank=2, term=2, seed=1)]
    elif form == "icm+bias+white":
        specs = [stat("rbf", sp, 1, 1), coreg_part(P, col), ("bias", 0, np.array([0.2]), allq, 0), ("white", 0, np.array([0.03]), allq, 0)]
    elif form == "coreg*bias":
        specs = [coreg_part(P, col), ("bias", 0, np.array([0.7]), allq, 1), stat("rbf", sp, 1, 0, 0.5)]
    elif form == "linear*coreg":
        specs = [LL.linear_part(sp, 1, term=1), coreg_part(P, col), stat("rbf", sp, 1, 0, 0.5)]
    elif form == "rbf*bias*coreg":
        specs = [stat("rbf", sp, 1, 1), ("bias", 0, np.array([0.7]), allq, 1), coreg_part(P, col)]
    elif form == "rbf+coreg":                                    # alone in its term: no other factor to multiply up
        specs = [stat("rbf", sp, 1, 0), coreg_part(P, col, term=0)]
    else:
        assert form == "rbf_only"
        specs = [stat("rbf", sp, 1, 0)]
    freq = data.uniform(1.0, 3.0, (Ds, Dy))
    idx = X[:, col].astype(int)
    R = np.sin(2.0 * np.pi * X[:, gd] @ freq[:len(gd)] + 0.7 * idx[:, None]) + 0.2 * data.standard_normal((N, Dy))
    if c["noise_kind"] == "hom":
        noise = 0.05
    elif c["noise_kind"] == "mixed":                             # MixedNoise: one variance per output, by point
        noise = (0.03 + 0.02 * np.arange(P))[idx]
    else:
        noise = 0.03 + 0.1 * rng.uniform(0.0, 1.0, N)

    def new(n):
        Xs = rng.uniform(-0.5, 0.5, (n, D))
        Xs[:, col] = rng.integers(0, P, n)
        return Xs
    c.update(specs=specs, X=np.ascontiguousarray(X), Z=np.ascontiguousarray(Z), R=R, noise=noise, Xs1=new(1), Xs129=new(129),
             idx_col=col, block=(N // 3, max(1, N // 2)) if not c["blocked"] else (N // 3, 300))
    return c


_MEMO = {}


def reference(name):
    """(case, long-double reference (blocked for `chunks`), this restatement at fp64, kappa = cond2(Kmm + 1e-8 I) <= 1e4) of a
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


# ---- the reference's own evaluations (tests/golden/sparse_coreg/*.npz, written by tools/make_golden_sparse_coreg.py) -------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sparse_coreg")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))
# the tolerances the fixtures of the stationary kinds are held to in tests/test_gpu_sparse.py (sparse_lin_ld.FIXTURE_TOL)
FIXTURE_TOL = LL.FIXTURE_TOL
FIXTURE_TOL_DEFAULT = LL.FIXTURE_TOL_DEFAULT


def load_fixture(name):
    """a fixture with its part list in kern_ld's format; fx["P"], fx["noise"] (N per-point variances), fx["noise_out"] (per output)"""
    fx = dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))
    fx["name"] = name
    fx["specs"] = [(s[0], int(s[1]), np.array(s[2], dtype=np.float64), np.array(s[3], dtype=np.int32), int(s[4]))
                   for s in json.loads(str(fx["specs"]))]
    fx["P"] = int(fx["P"])
    return fx


def restate_fixture(fx, dt=np.float64):
    """the quantities of a fixture from this file's restatement, under the fixture's names"""
    specs, X, Z, Y, Xs = fx["specs"], fx["X"], fx["Z"], fx["Y"], fx["Xs"]
    r = vardtc(specs, X, Z, Y, fx["noise"], dt=dt)
    mu, var = predict(specs, Z, Xs, r, False, dt)
    idx = X[:, int(fx["idx_col"])].astype(int)
    dn = KL._a(r["dnoise"], dt).reshape(X.shape[0], -1).sum(axis=1)
    return dict(lml=r["lml"], dtheta=r["dtheta"], dZ=r["dZ"], dL_dKmm=r["dL_dKmm"], dL_dKnm=r["dL_dKnm"], dL_dKdiag=r["dL_dKdiag"],
                dL_dthetaL=np.array([np.sum(dn[idx == p]) for p in range(fx["P"])], dtype=dt),
                woodbury_vector=r["woodbury_vector"], woodbury_inv=r["woodbury_inv"], pred_mu=mu, pred_var=var,
                pred_cov=predict(specs, Z, Xs, r, True, dt)[1])


def fixture_figures(got, fx):
    """{quantity: (max |got - fixture| / max |fixture|, its tolerance)} over what both hold; a quantity that is identically zero
    in the fixture (dZ of an expression without a stationary factor) is held to its absolute size"""
    out = {}
    for q, v in got.items():
        if q not in fx or v is None:
            continue
        ref = np.asarray(fx[q], dtype=np.float64)
        g = KL.f64(np.asarray(v)).reshape(ref.shape)
        den = np.abs(ref).max()
        out[q] = (float(np.abs(g - ref).max() / (den if den > 0 else 1.0)), FIXTURE_TOL.get(q, FIXTURE_TOL_DEFAULT))
    return out


def make_kernel(fx):
    """the package's kernel of a fixture's part list: stationary / Bias / White / Linear leaves, Coregionalize from W and kappa"""
    import gpy_amd
    groups, seen = [], {}
    for kind, ard, th, dims, term in fx["specs"]:
        dims = [int(d) for d in dims]
        if kind == "coregionalize":
            P, r = ard % 100, ard // 100
            k = gpy_amd.Coregionalize(1, P, rank=r, W=th[:P * r].reshape(P, r), kappa=th[P * r:], active_dims=dims)
        else:
            k = LL.make_kernel(dict(specs=[(kind, ard, th, dims, 0)]))
        if term == 0:
            groups.append([k])
        elif term in seen:
            seen[term].append(k)
        else:
            seen[term] = [k]
            groups.append(seen[term])
    tops = [g[0] if len(g) == 1 else gpy_amd.Prod(g) for g in groups]
    return tops[0] if len(tops) == 1 else gpy_amd.Add(tops)
