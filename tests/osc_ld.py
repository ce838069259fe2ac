"""Long-double restatement of the three oscillating stationary kinds of the exact-GP device path -- Cosine, Sinc and
ExpQuadCosine (C-ABI kinds 12 / 13 / 14) -- on the leaf machinery of tests/kern_ld.py, and the seeded cases of their sweep.

Written from the formulas of the reference's classes (stationary.py:664-680 Cosine, :682-713 ExpQuadCosine, :717-743 Sinc):

    Cosine         K = v cos r                        dK/dr = -v sin r
    Sinc           K = v sin(2 pi r) / (2 pi r)       dK/dr = v (cos(2 pi r) - sinc(2 r)) / r      (K = v, dK/dr = 0 at r = 0)
    ExpQuadCosine  K = v exp(-2 pi^2 r^2) cos(2 pi r / T)
                   dK/dr = -4 pi^2 r K - v (2 pi / T) exp(-2 pi^2 r^2) sin(2 pi r / T)
                   dK/dT = v (2 pi r / T^2) exp(-2 pi^2 r^2) sin(2 pi r / T)

theta = [variance, lengthscale(s)] and, for ExpQuadCosine, the period linked last (:692-695).  r comes from coordinate
differences as in kern_ld; `_inv_dist` (1 / r, 0 at r = 0, :225-232) enters the lengthscale and X gradients exactly as for the
other stationary kinds.  Sinc's cos t - sin t / t (t = 2 pi r) cancels for small t; below t^2 = 1/4 it is summed from its
series sum_k (-1)^k 2k / (2k + 1)! t^2k in the working type (the reference switches to the leading term below r = 1e-5,
:733-743; the two agree to O(r^3)).

Importing this module REGISTERS the three kinds on `kern_ld._Leaf` (methods `_init_<kind>`, `_dparam_<kind>`, `_dx_<kind>`, the
hooks that class dispatches on), so that every function of kern_ld -- `K`, `Kdiag`, `dtheta`, `gradients_X`, `exact`,
`predict`, `fused_exprs` -- takes specs of these kinds, alone and next to the twelve it already knows.  Nothing of kern_ld's own
kinds changes.  `kern_ld.make_case` seeds by the index of a kind in its `KINDS`, so the cases of this sweep are seeded here;
they keep its edges (row 1 of X equals row 0, row 0 of X2 equals the last row of X, the subset shape uses columns 0, 2, 3) and
its SHAPES.

The kinds are positive definite over ONE input dimension only (cos |x - x'| is not a covariance for D > 1).  The K-level cases
(`make_case`) use every column: K and its gradients need no definiteness.  The inference-level cases (`make_fused_case`) put
the kind on one column of X."""
import json
import os

import numpy as np

import kern_ld as KL

LD = KL.LD
KINDS = ("cosine", "sinc", "expquadcosine")
KIND_IDS = {"cosine": 12, "sinc": 13, "expquadcosine": 14}
CLASS_NAMES = {"cosine": "Cosine", "sinc": "Sinc", "expquadcosine": "ExpQuadCosine"}
# (name, kind, ard)
VARIANTS = [("cosine_iso", "cosine", 0), ("cosine_ard", "cosine", 1), ("sinc_iso", "sinc", 0), ("sinc_ard", "sinc", 1),
            ("eqc_iso", "expquadcosine", 0), ("eqc_ard", "expquadcosine", 1)]
SHAPES = KL.SHAPES
SUBSET_SHAPE = KL.SUBSET_SHAPE
MIN_ENVELOPE = 0.1               # the median off-diagonal exp(-2 pi^2 r^2) of an ExpQuadCosine case must reach this


# ---- the leaves, registered on kern_ld._Leaf ------------------------------------------------------------------------------
def _sinc_diff(t, dt):
    """cos t - sin t / t in the working type: the series in u = t^2 below u = 1/4 (nine terms: the next is < 1e-23 of the
    first), the difference itself above"""
    u = np.square(t)
    small = u < dt(1) / 4
    us = np.where(small, u, 0)
    ser, fact = np.zeros_like(us), dt(1)
    term = np.ones_like(us)
    for k in range(1, 10):
        fact = fact * (2 * k) * (2 * k + 1)                # (2k + 1)!
        term = term * us
        ser = ser + (-1) ** k * dt(2 * k) / fact * term
    ts = np.where(small, 1, t)
    return np.where(small, ser, np.cos(ts) - np.sin(ts) / ts)


def _init_osc(self):
    th, kind, c, dt = self.th, self.kind, self.c, self.dt
    self.v = th[0]
    nl = self.nd if self.ard else 1
    self.ls = self._vec(th[1:1 + nl])
    r2 = np.zeros((self.N, self.M), dtype=dt)
    for a in range(self.nd):
        r2 = r2 + np.square(self._diff(a) / self.ls[a])
    r = np.sqrt(r2)
    self.r = r
    with np.errstate(divide="ignore"):
        self.inv = np.where(r != 0, 1 / np.where(r != 0, r, 1), 0)               # _inv_dist (stationary.py:225-232)
    v, pi = self.v, c["pi"]
    if kind == "cosine":                                                         # stationary.py:676-680
        self.K = v * np.cos(r)
        self.dK_dr = -v * np.sin(r)
    elif kind == "sinc":                                                         # stationary.py:730-743
        t = 2 * pi * r
        snc = np.where(r != 0, np.sin(t) / np.where(r != 0, t, 1), 1)
        self.K = v * snc
        self.dK_dr = v * _sinc_diff(t, dt) * self.inv
    else:                                                                        # expquadcosine (stationary.py:697-709)
        self.T = th[1 + nl]
        self.env = np.exp(-2 * pi * pi * r2)
        a = 2 * pi * r / self.T
        self.K = v * self.env * np.cos(a)
        w = v * self.env * np.sin(a)
        self.dK_dr = -4 * pi * pi * r * self.K - 2 * pi / self.T * w
        self.dK_dT = 2 * pi * r / self.T ** 2 * w
    self.np_ = 1 + nl + (1 if kind == "expquadcosine" else 0)


def _dparam_osc(self, k):
    nl = self.nd if self.ard else 1
    if k <= nl:
        return KL._Leaf._dparam_stationary(self, k)                              # variance and lengthscale(s)
    return self.dK_dT                                                            # stationary.py:703-709


for _kind in KINDS:
    setattr(KL._Leaf, "_init_" + _kind, _init_osc)
    setattr(KL._Leaf, "_dparam_" + _kind, _dparam_osc)
    setattr(KL._Leaf, "_dx_" + _kind, KL._Leaf._dx_stationary)


# ---- the cases ------------------------------------------------------------------------------------------------------------
def case_id(variant, shape):
    return KL.case_id(variant, shape)


def _theta(kind, sub, nd, rng):
    """kern_ld's lengthscales (sqrt(nd) x U(0.8, 1.6)); ExpQuadCosine's are 2 pi times those, so that its envelope
    exp(-2 pi^2 r^2) is the RBF's exp(-r'^2 / 2) at kern_ld's scaling and K keeps off-diagonal mass at 65 dimensions; its
    period lies in [0.5, 2]"""
    ls = KL._theta("rbf", 1, nd, rng)[1:]
    if kind == "cosine":
        return np.concatenate([[1.2], ls if sub else ls[:1]])
    if kind == "sinc":
        return np.concatenate([[0.8], ls if sub else ls[:1]])
    ls = 2 * np.pi * ls
    return np.concatenate([[1.1], ls if sub else ls[:1], [rng.uniform(0.5, 2.0)]])


def envelope_median(spec, X):
    """median over the off-diagonal pairs of exp(-2 pi^2 r^2) of an ExpQuadCosine part (None for N < 2)"""
    lf = KL._Leaf(spec, X, None, np.float64)
    off = ~np.eye(lf.N, dtype=bool)
    return float(np.median(lf.env[off])) if lf.N >= 2 else None


def _finish(name, kind, shape, spec, X, X2, rng):
    N, M, D, Dy = shape
    if kind == "expquadcosine" and N >= 2:
        med = envelope_median(spec, X)
        assert med >= MIN_ENVELOPE, "%s: median off-diagonal envelope %.3g < %.1f" % (name, med, MIN_ENVELOPE)
    scale = float(spec[2][0])                                   # Kdiag = variance
    Y = rng.standard_normal((N, Dy))
    return dict(name=name, kind=kind, shape=tuple(shape), spec=spec, X=X, X2=X2, Y=Y, G=rng.standard_normal((N, N)),
                G2=rng.standard_normal((N, M)), scale=scale, noise=0.1 * scale, E=rng.standard_normal((N, 2)),
                E2=rng.standard_normal((M, 2)))


def _inputs(kind, sub, shape, tag):
    N, M, D, Dy = shape
    rng = np.random.default_rng([100 + KINDS.index(kind), sub, N, M, D, tag])
    X = rng.standard_normal((N, D))
    X2 = rng.standard_normal((M, D))
    if N >= 2:
        X[1] = X[0]
        X2[0] = X[N - 1]
    return rng, X, X2


def make_case(variant, shape):
    """the K-level case of one (variant, shape): the kind over every column (the subset shape: columns 0, 2, 3)"""
    name, kind, sub = variant
    rng, X, X2 = _inputs(kind, sub, shape, 0)
    dims = np.array([0, 2, 3]) if tuple(shape) == SUBSET_SHAPE else np.arange(shape[2])
    spec = (kind, sub, _theta(kind, sub, len(dims), rng), dims, 0)
    return _finish(name, kind, shape, spec, X, X2, rng)


def fused_column(shape):
    """the one active column of the inference-level cases: 0, at the subset shape 2 (not the first column)"""
    return 2 if tuple(shape) == SUBSET_SHAPE else 0


def make_fused_case(variant, shape):
    """the inference-level case: the kind on ONE column of the same seeded N x D inputs (positive definite there); with
    `kern_ld.fused_exprs` it stands alone, next to a White and times an RBF on two further columns"""
    name, kind, sub = variant
    rng, X, X2 = _inputs(kind, sub, shape, 1)
    spec = (kind, sub, _theta(kind, sub, 1, rng), np.array([fused_column(shape)]), 0)
    return _finish(name, kind, shape, spec, X, X2, rng)


def fused_sweep():
    """[(tag, specs, X, Xs, case)] of every inference-level case of the GPU sweep"""
    out = []
    for v in VARIANTS:
        for s in SHAPES:
            c = make_fused_case(v, s)
            for label, specs, X, Xs in KL.fused_exprs(c):
                out.append((case_id(v, s) + "-" + label, specs, X, Xs, c))
    return out


def fp64_floor(specs, X, Y, noise, ex, nu=None):
    """the figure (eps64 x cond) of the fp64 evaluation of the same formulas on the same input against the long-double
    result `ex`: what a double-precision pipeline reaches on this case, never the device's figure"""
    e64 = KL.exact(specs, X, Y, noise, nu, dt=np.float64)
    return KL.grad_figure(e64["dtheta"], ex["dtheta"], ex["dtheta_cond"])


# ---- the fixtures from the reference's own code (tests/golden/osc, tools/make_golden_osc.py) ------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "osc")
INFERENCE_FIXTURES = ["cosine_iso_n160_d1", "rbf0_x_cosine1_n180_d2", "sinc_iso_n160_d1", "sinc1_plus_rbfard_n160_d3",
                      "eqc_iso_n180_d1", "sm3_bias_n200_d1", "studentt_eqc1_plus_rbf_n160_d2"]
TOL_LML, TOL_ALPHA, TOL_GRAD, TOL_K, TOL_PRED = 1e-10, 1e-9, 1e-8, 1e-13, 1e-9


def load_specs(s):
    return [(k, int(a), np.asarray(t, float), np.asarray(d, int), int(term)) for k, a, t, d, term in json.loads(str(s))]


def load_fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    g = {k: z[k] for k in z.files}
    if "specs" in g:
        g["specs"] = load_specs(g["specs"])
    if "nu" in g:
        g["nu"] = None if float(g["nu"]) < 0 else float(g["nu"])
    if "gseed" in g:
        rng = np.random.default_rng(1000 + int(g["gseed"]))
        M = g["Xs"].shape[0] if "Xs" in g else g["X2"].shape[0]
        g["G"] = rng.standard_normal((g["X"].shape[0],) * 2)
        g["G2"] = rng.standard_normal((g["X"].shape[0], M))
    return g


def toy_specs(theta):
    """the part list of the example's kernel (three ExpQuadCosine parts plus Bias) from the flat parameter vector of the toy
    fixture: [variance, lengthscale, period] x 3, Bias variance, noise variance"""
    return [("expquadcosine", 0, np.asarray(theta[3 * i:3 * i + 3], float), np.array([0]), 0) for i in range(3)] + \
        [("bias", 0, np.asarray(theta[9:10], float), np.array([0]), 0)]
