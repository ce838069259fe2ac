"""Long-double (x86 80-bit) restatement of what an exact-GP context answers after an evaluation -- the predictive mean,
variance and full covariance, GP.predictive_gradients (core/gp.py:418-474) and Posterior.covariance_between_points
(posterior.py:109-130) -- and the shape sweep that tests/test_oracle_predict_ld.py (CPU) and tests/test_gpu_predict_shapes.py
(GPU) share.

Everything kernel-shaped comes from tests/kern_ld.py (and tests/osc_ld.py for Cosine / Sinc / ExpQuadCosine): K, Kdiag,
gradients_X, the part format (kind, ard, theta, active_dims, term), the column-oriented Cholesky, the triangular solves and the
explicit-sum matrix product.  No kernel formula is restated here except the derivative of a point-dependent diagonal:

    mu = K(X*, X) alpha,  var = Kdiag(X*) - colsum((L^-1 K(X, X*))^2),  cov = K(X*, X*) - (L^-1 Kx)^T (L^-1 Kx)      (kern_ld.predict)
    dmu[:, :, d] = gradients_X(1 (x) alpha_d^T, X*, X)                                                      (gp.py:442-445)
    dvar = gradients_X(-2 K(X*, X) Ky^-1, X*, X) + dKdiag/dX*                                              (gp.py:448,462-464)
    dKdiag/dx*_q = 0 for the stationary kinds (stationary.py:360-361), 2 v_q x*_q for Linear (linear.py:116-117), and for MLP
                   2 w_q x*_q v (2/pi) / (sqrt(1 - (p / (p + 1))^2) (p + 1)^2), p = sum_q w_q x*_q^2 + b   (mlp.py:133-147)
    covb = K(X1, X2) - (L^-1 K(X, X1))^T (L^-1 K(X, X2))

Every function takes `dt`: `np.longdouble` or `np.float64`, the same formulas in double precision -- what the judge uses to
measure how far an fp64 evaluation of the same input lies from the truth (e64; never a device figure).

The judge is the project's own (tests/sparse_ld.py: `rel_err`, `bound`):

    err(q) = max |got - q_ld| / max |q_ld|  <=  max(32 e64(q), 256 eps64 kappa),   kappa = cond2(Ky) of the fp64 Gram matrix,

and the columns of dmu / dvar outside every non-static part's active_dims must be exactly 0.  CEILING holds the standing
tolerances of the older tests; tests/test_oracle_predict_ld.py asserts that the bound of every case and quantity stays at or
below them, so that no case here is judged more loosely than it was before.

The sweep (N, M, D, Dy); inputs from `kern_ld.make_case` / `osc_ld.make_fused_case` with their deliberate edges (a duplicated
training row, a new point equal to a training point, a zero row for Linear / MLP -- moved from row N // 2 to row 3, see
`make_case` --, a pair one period apart for StdPeriodic), noise = 0.1 x scale:

    kinds   (65, 63, 33, 1) alone; (129, 130, 5, 4) next to a White, active_dims {0, 2, 3} (the oscillating kinds: one column):
            every variant with gradients_X -- the tile + 1 / second ARD group shape and the 128-row padding + 1 / four passes
    m_edge  N = 65, D = 3, Dy = 1, M = 1 | 63 | 64 | 65 (64 columns per workgroup of the column reduction), 128 | 129 (mp, the
            rectangular triangular products), 257 (three column tiles); one variant per route of part_gradients_X
    n_edge  M = 65, D = 3, Dy = 2, next to a White, N = 1 | 2 | 127 | 128 | 129 (npad), 255 | 256 | 257 (the 256-row staging
            block of the column reduction), 512 | 513 (one row split | 257 + 256 rows); N < M on purpose
    d_edge  N = 129, M = 65, Dy = 1, next to a White, D = 8 | 9, 16 | 17, 32 | 33 (the reduction's template width 9 / 17 / 33
            over D + 1; Linear: over D), 64 | 65 (several launches of 32 columns, the ones column with the last)
    dy      N = M = 65, D = 2, Dy = 1 | 2 | 4 | 5 (alpha[i * Dy + pass], one pass per output column)
    sum     N = 129, M = 65, D = 5, Dy = 2: rbf[0, 1] + matern32_ard[1, 2, 3] + linear[0] + white + bias; column 4 is nobody's
    covb    N = 129, D = 3, (M1, M2) = (1, 1), (1, 129), (129, 1), (63, 65), (128, 129), (130, 257) and (65, 65) at N = 513:
            m1p != m2p, the copy-out pitch; RBF alone, Matern32 times an RBF (the scratch buffers), Linear
"""
import numpy as np

import kern_ld as KL
import osc_ld as OS
import sparse_ld as SL

LD = KL.LD
EPS64 = KL.EPS64
JITTER = 1e-8
MAX_N = 513
QUANTITIES = ("mu", "var", "cov", "dmu", "dvar", "covb")
CEILING = dict(mu=1e-9, var=1e-9, cov=1e-9, covb=1e-9, dmu=1e-8, dvar=1e-8)
FAMILIES = ("kinds", "m_edge", "n_edge", "d_edge", "dy", "sum", "covb")
REPS = ("rbf_ard", "mlp_iso", "linear_ard", "stdperiodic_ard")           # one variant per route of part_gradients_X
KL_VARIANTS = dict((v[0], v) for v in KL.VARIANTS)
OS_VARIANTS = dict((v[0], v) for v in OS.VARIANTS)
STATIC = ("white", "bias", "coregionalize")


# ---- the restatement -----------------------------------------------------------------------------------------------------
def has_product(specs):
    return any(len(t) > 1 for t in KL.terms(specs))


def zero_cols(specs, D):
    """the input columns outside every non-static part's active_dims: dmu and dvar are exactly 0 there"""
    active = set(int(d) for s in specs if s[0] not in STATIC for d in s[3])
    return [q for q in range(D) if q not in active]


def dKdiag_dX(specs, Xs, dt=LD):
    """d Kdiag(x*_m) / d x*_mq (M x D) of a sum of parts, in the working type"""
    Xs = KL._a(Xs, dt)
    out = np.zeros(Xs.shape, dtype=dt)
    for kind, ard, th, dims, _ in specs:
        th = KL._a(th, dt)
        nd = len(dims)
        A = Xs[:, [int(d) for d in dims]]
        if kind == "linear":                                                     # linear.py:116-117
            g = 2 * np.broadcast_to(th, (nd,)) * A
        elif kind == "mlp":                                                      # mlp.py:133-147
            w = np.broadcast_to(th[1:-1], (nd,))
            p = np.sum(w * np.square(A), axis=1) + th[-1]
            common = th[0] * KL._c(dt)["two_over_pi"] / (np.sqrt(1 - np.square(p / (p + 1))) * np.square(p + 1))
            g = 2 * common[:, None] * w * A
        else:
            continue
        for a, q in enumerate(dims):
            out[:, int(q)] += g[:, a]
    return out


def dx_tensor(specs, Xs, X, dt=LD):
    """T[m, n, q] = dK(x*_m, x_n) / dx*_mq of a sum of parts (M x N x D): the unreduced terms of dmu and dvar, for the tests
    that plant a fault in the reduction over n"""
    assert not has_product(specs)
    lv = KL.leaves(specs, Xs, X, dt)
    M, D = np.shape(Xs)
    T = np.zeros((M, np.shape(X)[0], D), dtype=dt)
    for leaf in lv:
        for q in leaf.dims:
            d = leaf.dx(q)
            if d is not None:
                T[:, :, q] += d
    return T


def evaluate(specs, X, Y, noise, Xs, X1=None, X2=None, dt=LD, grads=True, max_n=MAX_N):
    """dict(mu, var, cov, dmu, dvar[, covb], alpha, L, Ki, Ky_diag_add) of the exact GP (specs, X, Y, noise) at the new points
    Xs; covb between X1 and X2 where given.  `grads=False` (or a product kernel, or a Poly part): no dmu / dvar."""
    ex = KL.exact(specs, X, Y, noise, jitter=JITTER, dt=dt, max_n=max_n)
    out = dict(alpha=ex["alpha"], L=ex["L"], Ki=ex["Ki"])
    out["mu"], out["var"], out["cov"] = KL.predict(specs, X, ex, Xs, dt)
    if grads and not has_product(specs) and KL.has_gradients_X(specs):
        M, D = np.shape(Xs)
        Dy = np.shape(Y)[1]
        lv = KL.leaves(specs, Xs, X, dt)
        dmu = np.zeros((M, D, Dy), dtype=dt)
        ones = np.ones((M, 1), dtype=dt)
        for d in range(Dy):
            dmu[:, :, d] = KL.gradients_X(specs, ones * ex["alpha"][:, d][None, :], Xs, X, dt, lv)[0]
        a2 = -2 * KL.matmul(KL.K(specs, Xs, X, dt, lv), ex["Ki"])
        out["dmu"] = dmu
        out["dvar"] = KL.gradients_X(specs, a2, Xs, X, dt, lv)[0] + dKdiag_dX(specs, Xs, dt)
        out["zero_cols"] = zero_cols(specs, D)
    if X1 is not None:
        T1 = KL.solve_lower(ex["L"], KL.K(specs, X, X1, dt) + np.zeros((np.shape(X)[0], np.shape(X1)[0]), dtype=dt))
        T2 = KL.solve_lower(ex["L"], KL.K(specs, X, X2, dt) + np.zeros((np.shape(X)[0], np.shape(X2)[0]), dtype=dt))
        out["covb"] = KL.K(specs, X1, X2, dt) - KL.matmul(T1.T, T2)
    return out


def kappa_of(specs, X, noise):
    """cond2 of the fp64 Gram matrix plus noise plus jitter"""
    Ky = np.array(KL.K(specs, X, None, np.float64), dtype=np.float64)
    n = Ky.shape[0]
    Ky[np.arange(n), np.arange(n)] += float(noise) + JITTER
    return float(np.linalg.cond(Ky))


# ---- the judge -------------------------------------------------------------------------------------------------------------
rel_err = SL.rel_err
bound = SL.bound


def judge(got, ref_ld, ref_64, kappa):
    """Hold every quantity of `got` to err(q) <= bound(q); the columns of dmu / dvar outside every non-static part's
    active_dims must be exactly zero.  Returns ({q: (err, bound)}, [what failed])."""
    figs, bad = {}, []
    for q in QUANTITIES:
        if q not in got or got[q] is None:
            continue
        assert q in ref_ld, "no reference for " + q
        e, b = rel_err(got[q], ref_ld[q]), bound(q, ref_ld, ref_64, kappa)
        figs[q] = (e, b)
        if not e <= b:
            bad.append("%s: %.3e > %.3e" % (q, e, b))
    for q in ("dmu", "dvar"):
        if q in got and got[q] is not None and np.shape(got[q]) == np.shape(ref_ld[q]):
            for col in ref_ld["zero_cols"]:
                if np.any(np.asarray(got[q])[:, col] != 0):
                    bad.append("%s column %d is outside every part's active_dims and must be exactly 0" % (q, col))
    return figs, bad


def figures_line(name, kappa, figs):
    return "FIG %s kappa %.3g " % (name, kappa) + " ".join("%s %.2e/%.2e=%.3f" % (q, e, b, e / b) for q, (e, b) in figs.items())


# ---- the sweep -------------------------------------------------------------------------------------------------------------
def _case(family, variant, label, N, M, D, Dy, M2=None):
    name = "%s-%s-%s-n%d_m%d_d%d_dy%d" % (family, variant, label, N, M, D, Dy) + ("_mm%d" % M2 if M2 is not None else "")
    return dict(name=name, family=family, variant=variant, label=label, N=N, M=M, D=D, Dy=Dy, M2=M2)


def _cases():
    out = []
    grad_variants = [v[0] for v in KL.VARIANTS if v[1] not in STATIC + ("poly",)] + [v[0] for v in OS.VARIANTS]
    for v in grad_variants:
        out += [_case("kinds", v, "alone", 65, 63, 33, 1), _case("kinds", v, "plus_white", 129, 130, 5, 4)]
    out += [_case("m_edge", v, "alone", 65, M, 3, 1) for v in REPS for M in (1, 63, 64, 65, 128, 129, 257)]
    out += [_case("n_edge", v, "plus_white", N, 65, 3, 2) for v in REPS for N in (1, 2, 127, 128, 129, 255, 256, 257, 512, 513)]
    out += [_case("d_edge", v, "plus_white", 129, 65, D, 1) for v in ("rbf_ard", "ratquad_ard", "linear_ard", "stdperiodic_ard")
            for D in (8, 9, 16, 17, 32, 33, 64, 65)]
    out += [_case("dy", v, "alone", 65, 65, 2, Dy) for v in ("rbf_iso", "linear_iso") for Dy in (1, 2, 4, 5)]
    out += [_case("sum", "rbf+matern32_ard+linear+white+bias", "sum", 129, 65, 5, 2)]
    for v, label in (("rbf_ard", "alone"), ("matern32_iso", "times_rbf"), ("linear_ard", "alone")):
        out += [_case("covb", v, label, 129, M1, 3, 1, M2) for M1, M2 in ((1, 1), (1, 129), (129, 1), (63, 65), (128, 129), (130, 257))]
        out += [_case("covb", v, label, 513, 65, 3, 1, 65)]
    return out


CASES = _cases()
NAMES = [c["name"] for c in CASES]
BY_NAME = dict((c["name"], c) for c in CASES)
assert len(BY_NAME) == len(CASES)
DETERMINISM = "n_edge-rbf_ard-plus_white-n513_m65_d3_dy2"


def by_family(family):
    return [c["name"] for c in CASES if c["family"] == family]


def _sum_specs():
    return [("rbf", 0, np.array([0.9, 1.1]), np.array([0, 1]), 0),
            ("matern32", 1, np.array([0.7, 0.8, 1.3, 2.0]), np.array([1, 2, 3]), 0),
            ("linear", 0, np.array([0.4]), np.array([0]), 0),
            ("white", 0, np.array([0.02]), np.arange(5), 0), ("bias", 0, np.array([0.3]), np.arange(5), 0)]


def make_case(name):
    """the seeded inputs of one case: dict(specs (as kern_ld takes them), dev (as the device takes them), X, Y, Xs, noise[, X1,
    X2], ...)"""
    c = dict(BY_NAME[name])
    shape = (c["N"], c["M"], c["D"], c["Dy"])
    if c["family"] == "sum":
        base = KL.make_case(KL_VARIANTS["linear_iso"], shape)                    # with the zero row of a Linear case
        specs, X, Xs = _sum_specs(), base["X"], base["X2"]
        scale = float(np.max(KL.Kdiag(specs, np.vstack([X, Xs]), np.float64)))
    else:
        if c["variant"] in OS_VARIANTS:
            base = OS.make_fused_case(OS_VARIANTS[c["variant"]], shape)
        else:
            base = KL.make_case(KL_VARIANTS[c["variant"]], shape)
        _, specs, X, Xs = dict((e[0], e) for e in KL.fused_exprs(base))[c["label"]]
        scale = base["scale"]
    if c["N"] >= 8 and not np.any(X[c["N"] // 2]):
        # the all-zero row of a Linear / MLP case sits at row N // 2 = 256 for N = 512 | 513: the row the 256-row blocks and the
        # row split single out, and a zero row adds nothing to a Linear reduction, so losing it would go unseen.  It moves to row 3.
        X = X.copy()
        X[[3, c["N"] // 2]] = X[[c["N"] // 2, 3]]
    c.update(specs=specs, dev=KL.cabi_specs(specs), X=X, Y=base["Y"], Xs=Xs, noise=0.1 * scale, scale=scale)
    if c["family"] == "covb":                                                    # X1 = the new points; X2: seeded, and its last
        rng = np.random.default_rng([77, c["N"], c["M"], c["M2"]])              # point equals the first of X1 (r = 0 in K(X1, X2))
        P2 = rng.standard_normal((c["M2"], X.shape[1]))
        P2[-1] = Xs[0]
        c.update(X1=Xs, X2=P2)
    return c


_MEMO = {}


def reference(name):
    """(case, long-double reference, the same in fp64, kappa) of a case, computed once per process and not to be modified"""
    if name not in _MEMO:
        KL.require_ld()
        c = make_case(name)
        args = (c["specs"], c["X"], c["Y"], c["noise"], c["Xs"], c.get("X1"), c.get("X2"))
        _MEMO[name] = (c, evaluate(*args, dt=LD), evaluate(*args, dt=np.float64), kappa_of(c["specs"], c["X"], c["noise"]))
    return _MEMO[name]


def bounds(name):
    """{q: bound(q)} of a case"""
    c, ref, r64, kappa = reference(name)
    return dict((q, bound(q, ref, r64, kappa)) for q in QUANTITIES if q in ref)
