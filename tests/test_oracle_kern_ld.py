"""CPU: the long-double restatement of every kernel kind (tests/kern_ld.py) against the fp64 restatements the suite already
trusts (oracle.gp_oracle, periodic_np, linear_np, mlp_np, coreg_np through linear_np) and against the reference's own goldens,
at the shapes of the GPU sweep; the off-diagonal mass of every sweep case; and the sensitivity of the judge the GPU tests use
(tests/test_gpu_kernel_shapes.py): four wrong answers it has to reject at every shape.

Agreement bounds: K within 16 eps64 x max Kdiag, every gradient contraction within 16 eps64 x cond (cond = the sum of the
absolute values of the terms of that contraction).  The fp64 formulas sit at about 3.5 and 2.2 of those units.  oracle.gp_oracle
takes distances from |x|^2 + |y|^2 - 2 x.y as the reference does, which loses eps |x|^2 / r for close pairs (13.5 and 21 of
those units at N = 63, D = 2 even without coincident points) and is not exact at r = 0; what is compared for the four kinds it
serves are therefore its covariance functions, dK/dr and gradient reductions, given distances taken from coordinate
differences in fp64.  All comparisons run on the inputs of the GPU sweep, coincidences included."""
import json
import os

import numpy as np
import pytest

import kern_ld as KL
import mlp_np
import periodic_np
from oracle import gp_oracle as O

pytestmark = pytest.mark.skipif(not KL.HAVE_LD, reason="np.longdouble is not an extended format on this host")
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [(v, s) for v in KL.VARIANTS for s in KL.SHAPES]
IDS = [KL.case_id(v, s) for v, s in CASES]
GP_ORACLE_KINDS = ("rbf", "matern52", "matern32", "exponential")
EPS = KL.EPS64


def _fp64_restatement(case):
    """(K square, K rect, [dK/dtheta square], [dK/dtheta rect], gradX of G, gradX of G2 (None: Poly)) from the fp64 modules"""
    spec, X, X2, G, G2 = case["spec"], case["X"], case["X2"], case["G"], case["G2"]
    kind, ard, th, dims, _ = spec
    if kind in GP_ORACLE_KINDS:
        A, B = X[:, dims], X2[:, dims]
        ls = O._as_ls(th[1:], len(dims), bool(ard))
        dist = lambda B_: np.sqrt(np.sum(np.square((A[:, None, :] - B_[None, :, :]) / ls), -1))

        def grads(Gm, B_):
            dv, dl = O.update_gradients_full(kind, Gm, A, B_, th[0], th[1:], bool(ard), r=dist(A if B_ is None else B_))
            return np.concatenate([[dv], np.atleast_1d(dl)])

        def gx(Gm, B_):                                           # gp_oracle.gradients_X with the distances given
            B_ = A if B_ is None else B_
            r = dist(B_)
            tmp = 1.0 / np.where(r != 0.0, r, np.inf) * O.dK_dr(kind, r, th[0]) * Gm
            out = np.zeros(X.shape)
            out[:, dims] = np.sum(tmp[:, :, None] * (A[:, None, :] - B_[None, :, :]), axis=1) / ls ** 2
            return out
        return (O.K_of_r(kind, dist(A), th[0]), O.K_of_r(kind, dist(B), th[0]), grads(G, None), grads(G2, B), gx(G + G.T, None),
                gx(G2, B))
    mod = periodic_np if kind in ("ratquad", "stdperiodic") else mlp_np
    Ks, dKs, dXs = mod.leaf_parts(spec, X, None)
    Kr, dKr, dXr = mod.leaf_parts(spec, X, X2)
    con = lambda Gm, dK: np.array([np.sum(Gm * d) for d in dK])
    gxs = None if dXs is None else np.einsum("ij,ijq->iq", G + G.T, dXs)
    gxr = None if dXr is None else np.einsum("ij,ijq->iq", G2, dXr)
    return Ks, Kr, con(G, dKs), con(G2, dKr), gxs, gxr


@pytest.fixture(scope="module")
def ld_answers():
    """the long-double answers of the sweep, computed once per case and shared"""
    cache = {}

    def get(variant, shape, edges=True):
        key = (variant[0], tuple(shape), edges)
        if key not in cache:
            c = KL.make_case(variant, shape, edges)
            specs = [c["spec"]]
            lv_s, lv_r = KL.leaves(specs, c["X"]), KL.leaves(specs, c["X"], c["X2"])
            c["Ks"], c["Kr"] = KL.K(specs, c["X"], lv=lv_s), KL.K(specs, c["X"], c["X2"], lv=lv_r)
            c["dths"] = KL.dtheta(specs, c["G"], c["X"], lv=lv_s)
            c["dthr"] = KL.dtheta(specs, c["G2"], c["X"], c["X2"], lv=lv_r)
            if KL.has_gradients_X(specs):
                c["gxs"] = KL.gradients_X(specs, c["G"], c["X"], lv=lv_s)
                c["gxr"] = KL.gradients_X(specs, c["G2"], c["X"], c["X2"], lv=lv_r)
            cache[key] = c
        return cache[key]
    return get


@pytest.mark.parametrize("variant,shape", CASES, ids=IDS)
def test_long_double_agrees_with_the_fp64_restatements(variant, shape, ld_answers):
    c = ld_answers(variant, shape)
    Ks, Kr, gs, gr, gxs, gxr = _fp64_restatement(c)
    fk = max(KL.k_figure(Ks, c["Ks"], c["scale"]), KL.k_figure(Kr, c["Kr"], c["scale"]))
    fg = max(KL.grad_figure(gs, *c["dths"]), KL.grad_figure(gr, *c["dthr"]))
    fx = 0.0 if gxs is None else max(KL.grad_figure(gxs, *c["gxs"]), KL.grad_figure(gxr, *c["gxr"]))
    print("%s: K %.2f eps x scale, dtheta %.2f eps x cond, gradients_X %.2f eps x cond" % (KL.case_id(variant, shape), fk, fg, fx))
    assert fk <= 16 and fg <= 16 and fx <= 16
    kd = np.asarray(KL.Kdiag([c["spec"]], c["X"]))
    assert np.abs(kd - np.diag(c["Ks"])).max() <= 16 * EPS * c["scale"]           # Kdiag is the diagonal of K


@pytest.mark.parametrize("variant,shape", CASES, ids=IDS)
def test_the_double_precision_mode_of_the_module_agrees_too(variant, shape, ld_answers):
    """the same formulas with dt = float64 (what the GPU tests measure e64 with), on the inputs with every deliberate edge"""
    c = ld_answers(variant, shape)
    specs = [c["spec"]]
    fk = KL.k_figure(KL.K(specs, c["X"], c["X2"], dt=np.float64), c["Kr"], c["scale"])
    fg = KL.grad_figure(KL.dtheta(specs, c["G2"], c["X"], c["X2"], dt=np.float64)[0], *c["dthr"])
    fx = KL.grad_figure(KL.gradients_X(specs, c["G"], c["X"], dt=np.float64)[0], *c["gxs"]) if "gxs" in c else 0.0
    print("%s: K %.2f dtheta %.2f gradients_X %.2f" % (KL.case_id(variant, shape), fk, fg, fx))
    assert fk <= 16 and fg <= 16 and fx <= 16


@pytest.mark.parametrize("variant,shape", CASES, ids=IDS)
def test_every_sweep_case_keeps_off_diagonal_mass(variant, shape, ld_answers):
    """max off-diagonal |K| >= 1e-3 x scale, the deliberately coincident pair (0, 1) left out.  White has no off-diagonal by
    definition and N <= 2 has no other pair."""
    c = ld_answers(variant, shape)
    N = shape[0]
    if variant[1] == "white" or N <= 2:
        return
    off = np.abs(np.asarray(c["Ks"], dtype=float))
    off[np.arange(N), np.arange(N)] = 0.0
    off[0, 1] = off[1, 0] = 0.0
    print("%s: max off-diagonal %.3g x scale" % (KL.case_id(variant, shape), off.max() / c["scale"]))
    assert off.max() >= 1e-3 * c["scale"]


@pytest.mark.parametrize("variant", [v for v in KL.VARIANTS if v[1] in KL.STATIONARY], ids=lambda v: v[0])
def test_coincident_points_contribute_nothing_to_a_gradient(variant):
    """the r = 0 conventions (`_inv_dist`, stationary.py:225-232): with dL_dK non-zero only on coincident pairs, the lengthscale
    gradients and gradients_X vanish -- also for the Exponential kernel, whose dK/dr is not zero at r = 0"""
    c = KL.make_case(variant, (65, 63, 33, 1))
    specs = [c["spec"]]
    G2 = np.zeros((65, 63))
    G2[64, 0] = 1.5                                               # X2[0] == X[64]
    G = np.zeros((65, 65))
    G[0, 1], G[1, 0], G[5, 5] = 0.7, -0.2, 1.0                    # X[1] == X[0]
    for Gm, B in ((G2, c["X2"]), (G, None)):
        val, _ = KL.dtheta(specs, Gm, c["X"], B)
        nl = 33 if variant[2] else 1
        assert np.all(val[1:1 + nl] == 0) and val[0] != 0
        gx, _ = KL.gradients_X(specs, Gm, c["X"], B)
        assert np.all(gx == 0)


# ---- the reference's own goldens: one fixture per family ---------------------------------------------------------------------
GOLDENS = ["periodic/stdper_ard12_n160_d3", "periodic/ratquad_ard_active_n160_d3", "linear/linear_ard_active_n160_d3",
           "mlp/mlp_ard_active_n160_d3", "mlp/poly_o3_n160_d3", "coreg/lcm_m52_rbf_p2_r2_n110", "mlp/mlp0_x_rbf12_n160_d3"]


@pytest.mark.parametrize("name", GOLDENS)
def test_long_double_agrees_with_the_reference_goldens(name):
    z = np.load(os.path.join(HERE, "golden", name + ".npz"))
    specs = [(k, int(a), np.asarray(t, float), np.asarray(d, int), int(term)) for k, a, t, d, term in json.loads(str(z["specs"]))]
    X, Y = z["X"], z["Y"]
    scale = float(np.max(KL.Kdiag(specs, X)))
    row0 = KL.K(specs, X[:1], X)[0]
    print(name, "K_row0 %.2f eps x scale" % KL.k_figure(z["K_row0"], row0, scale))
    assert KL.k_ok(z["K_row0"], row0, scale)
    if "noise" not in z.files:                                    # the coregionalized fixtures carry one noise per output: K only
        return
    ex = KL.exact(specs, X, Y, float(z["noise"]), max_n=256)
    dth = KL.f64(ex["dtheta"])
    print(name, "lml %.2e dtheta %.2e" % (abs(float(ex["lml"]) - z["lml"]) / abs(z["lml"]),
                                          np.abs(dth - z["dtheta"]).max() / np.abs(z["dtheta"]).max()))
    assert abs(float(ex["lml"]) - z["lml"]) <= 1e-10 * abs(z["lml"])
    assert np.linalg.norm(KL.f64(ex["alpha"]) - z["alpha"]) <= 1e-9 * np.linalg.norm(z["alpha"])
    assert np.abs(dth - z["dtheta"]).max() <= 1e-8 * np.abs(z["dtheta"]).max()
    assert abs(float(ex["dnoise"]) - z["dnoise"]) <= 1e-8 * abs(z["dnoise"])
    if "gradX" in z.files and KL.has_gradients_X(specs):
        G = np.random.default_rng(1000 + int(z["gseed"])).standard_normal((X.shape[0],) * 2)
        gx = KL.f64(KL.gradients_X(specs, G, X)[0])
        assert np.abs(gx - z["gradX"]).max() <= 1e-8 * np.abs(z["gradX"]).max()


def test_long_double_agrees_with_a_stationary_golden():
    from conftest import load_golden
    g = load_golden("n64_d3_matern32_ard")
    spec = ("matern32", 1, np.concatenate([[g["variance"]], g["lengthscale"]]), np.arange(3), 0)
    assert KL.k_ok(g["K"], KL.K([spec], g["X"]), g["variance"])
    ex = KL.exact([spec], g["X"], g["Y"], float(g["noise"][0]))
    ref = np.concatenate([g["dvar"], g["dlen"]])
    assert abs(float(ex["lml"]) - g["lml"]) <= 1e-10 * abs(g["lml"])
    assert np.abs(KL.f64(ex["dtheta"]) - ref).max() <= 1e-8 * np.abs(ref).max()
    val, _ = KL.dtheta([spec], g["A"], g["X"], g["X2"])                          # the fixture's rectangular dL_dK
    refA = np.concatenate([g["dvar_A"], g["dlen_A"]])
    assert np.abs(KL.f64(val) - refA).max() <= 1e-8 * np.abs(refA).max()


def test_the_long_double_cholesky_and_lgamma():
    from scipy.special import gammaln
    rng = np.random.default_rng(5)
    A = rng.standard_normal((40, 40))
    S = A @ A.T + 40 * np.eye(40)
    L = KL.cholesky(np.asarray(S, dtype=KL.LD))
    assert np.abs(KL.f64(KL.matmul(L, L.T)) - S).max() <= 4 * EPS * np.abs(S).max()
    assert np.abs(KL.f64(L) - np.linalg.cholesky(S)).max() <= 1e-13 * np.abs(S).max() ** 0.5
    for x in (1.25, 2.5, 17.0, 34.25, 80.0):
        assert abs(float(KL.lgamma(x)) - gammaln(x)) <= 4 * EPS * max(1.0, abs(gammaln(x)))


# ---- the judge of the GPU tests rejects wrong answers ------------------------------------------------------------------------
@pytest.mark.parametrize("variant,shape", CASES, ids=IDS)
def test_the_comparator_rejects_four_wrong_answers(variant, shape, ld_answers):
    """copies of the long-double answer (rounded to fp64, as a perfect device would return it) that the judge has to refuse:
    one K entry moved by 1e-11 x scale; ARD gradient entries 31 and 32 swapped (where the kind has that many); one gradients_X
    row zeroed (where the kind has a gradients_X that is not identically zero); a constant scaled by 1 + 1e-11 (the whole of K(X, X),
    and the whole of gradients_X)"""
    c = ld_answers(variant, shape)
    specs = [c["spec"]]
    scale = c["scale"]
    e64 = lambda name, f, *a: KL.grad_tol(c[name][0], f(specs, *a, dt=np.float64)[0], c[name][1])
    tol_th = e64("dthr", KL.dtheta, c["G2"], c["X"], c["X2"])
    good_K, good_th = KL.f64(c["Kr"]), KL.f64(c["dthr"][0])
    assert KL.k_ok(good_K, c["Kr"], scale) and KL.grad_ok(good_th, c["dthr"][0], tol_th)       # the honest copy passes
    bad = good_K.copy()
    bad[-1, -1] += 1e-11 * scale
    assert not KL.k_ok(bad, c["Kr"], scale)
    assert not KL.k_ok(KL.f64(c["Ks"]) * (1 + 1e-11), c["Ks"], scale)            # a constant of the formula off in the 11th digit
    kind, ard = c["spec"][0], c["spec"][1]
    nd = len(c["spec"][3])
    if kind != "coregionalize" and ard and nd >= 33:
        off = 0 if kind == "linear" else 1                        # the first ARD entry within theta
        off += nd if kind == "stdperiodic" else 0                 # ... of the lengthscales, after the periods
        bad = good_th.copy()
        bad[[off + 31, off + 32]] = bad[[off + 32, off + 31]]
        assert not KL.grad_ok(bad, c["dthr"][0], tol_th)
    if "gxr" in c and np.any(c["gxr"][1] > 0):
        tol_x = e64("gxr", KL.gradients_X, c["G2"], c["X"], c["X2"])
        good_x = KL.f64(c["gxr"][0])
        assert KL.grad_ok(good_x, c["gxr"][0], tol_x)
        bad = good_x.copy()
        bad[int(np.argmax(np.abs(good_x).max(axis=1)))] = 0.0
        assert not KL.grad_ok(bad, c["gxr"][0], tol_x)
        assert not KL.grad_ok(good_x * (1 + 1e-11), c["gxr"][0], tol_x)
