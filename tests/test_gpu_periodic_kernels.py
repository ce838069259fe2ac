"""GPU (-m gpu): RatQuad and StdPeriodic (C-ABI kinds 6 / 7) through the fused exact-GP calls, the stateless kernel entry
points and the host classes, against fixtures from the reference's own code (tests/golden/periodic, made by
tools/make_golden_periodic.py) and against the NumPy restatement in periodic_np.py.  Tolerances as for the other kinds:
LML 1e-10 relative, alpha 1e-9, gradients 1e-8, K row 1e-13 variance, prediction 1e-9.

The Mauna-Loa fixture has calendar-year inputs.  Its RBF parts are evaluated by the reference through the expanded square
x^2 + x'^2 - 2 x x' (stationary.py `_unscaled_dist`), which carries ~1e-11 relative error at x ~ 2000; the device forms
x - x'.  That case is held to the standard tolerances against the NumPy restatement (which also forms x - x') and to
looser ones against the reference's numbers."""
import glob
import os

import numpy as np
import pytest

import gpy_amd
from gpy_amd import _lib as L

import periodic_np as P

pytestmark = pytest.mark.gpu
TOL_LML, TOL_ALPHA, TOL_GRAD, TOL_K, TOL_PRED = 1e-10, 1e-9, 1e-8, 1e-13, 1e-9
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(HERE, "golden", "periodic", "*.npz")))


def _load(name):
    z = np.load(os.path.join(HERE, "golden", "periodic", name + ".npz"))
    g = {k: z[k] for k in z.files}
    g["specs"] = P.load_specs(g["specs"])
    g["nu"] = None if float(g["nu"]) < 0 else float(g["nu"])
    rng = np.random.default_rng(1000 + int(g["gseed"]))
    g["G"] = rng.standard_normal((g["X"].shape[0],) * 2)
    g["G2"] = rng.standard_normal((g["X"].shape[0], g["Xs"].shape[0]))
    return g


def _loose(name):
    """tolerance factor against the reference's numbers (see the module docstring)"""
    return 1e4 if name.startswith("maunaloa") else 1.0


def leaf(spec):
    kind, ard, th, dims, _ = spec
    nd = len(dims)
    if kind == "ratquad":
        nl = nd if ard else 1
        return gpy_amd.RatQuad(nd, th[0], th[1:1 + nl], th[1 + nl], ARD=bool(ard), active_dims=dims)
    if kind == "stdperiodic":
        npr = nd if ard & 1 else 1
        return gpy_amd.StdPeriodic(nd, th[0], th[1:1 + npr], th[1 + npr:], ARD1=bool(ard & 1), ARD2=bool(ard & 2),
                                   active_dims=dims)
    if kind == "rbf":
        return gpy_amd.RBF(nd, th[0], th[1:], ARD=bool(ard), active_dims=dims)
    return gpy_amd.White(nd, th[0], active_dims=dims)


def kernel(specs):
    """the gpy_amd kernel expression of a part list"""
    summands = []
    for t in P.terms(specs):
        k = leaf(specs[t[0]])
        for i in t[1:]:
            k = k * leaf(specs[i])
        summands.append(k)
    k = summands[0]
    for s in summands[1:]:
        k = k + s
    return k


def _cabi_specs(specs):
    return [(k, a, th, d, t) for k, a, th, d, t in specs]


@pytest.mark.parametrize("name", NAMES)
def test_golden_through_the_c_abi(name):
    g = _load(name)
    f = _loose(name)
    specs = _cabi_specs(g["specs"])
    c = L.Context(0)
    try:
        c.set_data(g["X"], g["Y"])
        if g["nu"] is None:
            info, r = c.exact_inference_sum(specs, g["noise"], want_diag=True)
            assert abs(r["dnoise"] - g["dnoise"]) <= f * TOL_GRAD * abs(g["dnoise"])
        else:
            info, r = c.exact_studentt_sum(specs, g["nu"])
        assert info == 0
        assert abs(r["lml"] - g["lml"]) <= f * TOL_LML * abs(g["lml"])
        assert np.linalg.norm(r["alpha"] - g["alpha"]) <= f * TOL_ALPHA * np.linalg.norm(g["alpha"])
        assert np.abs(r["dtheta"] - g["dtheta"]).max() <= f * TOL_GRAD * np.abs(g["dtheta"]).max()
        K = c.fetch(L.FETCH_K)
        var = max(float(s[2][0]) for s in specs)
        assert np.abs(K[0] - g["K_row0"]).max() <= f * TOL_K * var
        if g["nu"] is None:
            mu, v = c.predict_sum(specs, g["Xs"])
            assert np.abs(mu - g["pred_mu"]).max() <= f * TOL_PRED and np.abs(v - g["pred_var"]).max() <= f * TOL_PRED
            _, cov = c.predict_sum(specs, g["Xs"], full_cov=True)
            assert np.abs(cov - g["pred_cov"]).max() <= f * TOL_PRED
        # the NumPy restatement at the standard tolerances (the calendar-year case included)
        lml, alpha, dth, _ = P.exact(g["specs"], g["X"], g["Y"], float(g["noise"]), g["nu"])
        assert abs(r["lml"] - lml) <= TOL_LML * abs(lml)
        assert np.linalg.norm(r["alpha"] - alpha) <= TOL_ALPHA * np.linalg.norm(alpha)
        assert np.abs(r["dtheta"] - dth).max() <= TOL_GRAD * np.abs(dth).max()
        Knp = P.expr(g["specs"], g["X"])[0]
        assert np.abs(K[0] - Knp[0]).max() <= TOL_K * var
    finally:
        c.close()


@pytest.mark.parametrize("name", [n for n in NAMES if not n.startswith("studentt")])
def test_golden_through_gpregression(name):
    g = _load(name)
    f = _loose(name)
    k = kernel(g["specs"])
    m = gpy_amd.GPRegression(g["X"], g["Y"], k, noise_var=float(g["noise"]))
    assert abs(m.log_likelihood() - g["lml"]) <= f * TOL_LML * abs(g["lml"])
    gref = np.concatenate([g["dtheta"], [g["dnoise"]]])
    assert np.abs(m.gradient - gref).max() <= f * TOL_GRAD * np.abs(gref).max()
    mu, var = m.predict_noiseless(g["Xs"])
    assert np.abs(mu - g["pred_mu"]).max() <= f * TOL_PRED and np.abs(var - g["pred_var"]).max() <= f * TOL_PRED


@pytest.mark.parametrize("name", NAMES)
def test_gradients_X_against_the_golden(name):
    g = _load(name)
    k = kernel(g["specs"])
    f = _loose(name)
    gx = k.gradients_X(g["G"], g["X"])
    assert np.abs(gx - g["gradX"]).max() <= f * TOL_GRAD * np.abs(g["gradX"]).max()
    gx2 = k.gradients_X(g["G2"], g["X"], g["Xs"])
    assert np.abs(gx2 - g["gradX2"]).max() <= f * TOL_GRAD * np.abs(g["gradX2"]).max()
    ref = P.gradients_X(g["specs"], g["G"], g["X"])
    assert np.abs(gx - ref).max() <= TOL_GRAD * np.abs(ref).max()


@pytest.mark.parametrize("name", ["stdper_ard12_n160_d3", "ratquad_ard_active_n160_d3"])
def test_single_kernel_entry_points(name):
    g = _load(name)
    (kind, ard, th, dims, _), = g["specs"]
    k = leaf(g["specs"][0])
    X = g["X"]
    Kp = k.K(X, g["Xs"])
    ref = P.leaf_parts(g["specs"][0], X, g["Xs"])[0]
    assert np.abs(Kp - ref).max() <= TOL_K * th[0]
    assert np.all(k.Kdiag(X) == th[0])
    k.update_gradients_full(g["G2"], X, g["Xs"])
    got = k.gradient.copy()
    want = np.array([np.sum(g["G2"] * d) for d in P.leaf_parts(g["specs"][0], X, g["Xs"])[1]])
    assert np.abs(got - want).max() <= TOL_GRAD * np.abs(want).max()


def _fd_predict(m, Xs, h=1e-5):
    D = Xs.shape[1]
    dmu = np.zeros((Xs.shape[0], D))
    dvar = np.zeros((Xs.shape[0], D))
    for q in range(D):
        e = np.zeros(D)
        e[q] = h
        mp, vp = m.predict_noiseless(Xs + e)
        mm, vm = m.predict_noiseless(Xs - e)
        dmu[:, q] = (mp - mm)[:, 0] / (2 * h)
        dvar[:, q] = (vp - vm)[:, 0] / (2 * h)
    return dmu, dvar


@pytest.mark.parametrize("composite", [False, True])
def test_predictive_gradients_against_central_differences(composite):
    g = _load("stdper_ard12_n160_d3")
    k = leaf(g["specs"][0])
    if composite:
        k = k + gpy_amd.RatQuad(3, 0.6, [0.9, 1.3, 1.1], 1.4, ARD=True)
    m = gpy_amd.GPRegression(g["X"], g["Y"], k, noise_var=0.1)
    Xs = g["Xs"][:6]
    dmu, dvar = m.predictive_gradients(Xs)
    fmu, fvar = _fd_predict(m, Xs)
    assert np.abs(dmu[:, :, 0] - fmu).max() <= 1e-6 * max(1.0, np.abs(fmu).max())
    assert np.abs(dvar - fvar).max() <= 1e-6 * max(1.0, np.abs(fvar).max())


def test_checkgrad_on_the_composite():
    g = _load("maunaloa_years_n300_d1")
    m = gpy_amd.GPRegression(g["X"], g["Y"], kernel(g["specs"]), noise_var=float(g["noise"]))
    assert m.checkgrad()


@pytest.mark.parametrize("N", [4096, 4224])
def test_composite_at_persistent_cholesky_sizes(N):
    rng = np.random.default_rng(N)
    x = np.sort(1958.0 + 62.0 * rng.random(N))
    X = x[:, None]
    Y = (0.02 * (x - 1958.0) + 0.5 * np.sin(2 * np.pi * x) + 0.1 * rng.standard_normal(N))[:, None]
    specs = [("rbf", 0, np.array([1.0, 30.0]), np.array([0]), 0), ("rbf", 0, np.array([0.3, 60.0]), np.array([0]), 1),
             ("stdperiodic", 0, np.array([1.0, 1.0, 1.2]), np.array([0]), 1),
             ("ratquad", 0, np.array([0.2, 1.5, 0.8]), np.array([0]), 0)]
    c = L.Context(0)
    try:
        c.set_data(X, Y)
        info, r = c.exact_inference_sum(specs, 0.05)
        assert info == 0
    finally:
        c.close()
    lml, alpha, dth, _ = P.exact(specs, X, Y, 0.05)
    assert abs(r["lml"] - lml) <= TOL_LML * abs(lml)
    assert np.linalg.norm(r["alpha"] - alpha) <= TOL_ALPHA * np.linalg.norm(alpha)
    assert np.abs(r["dtheta"] - dth).max() <= TOL_GRAD * np.abs(dth).max()


@pytest.mark.parametrize("cls", ["StdPeriodic", "RatQuad"])
def test_lone_kernel_takes_the_fused_call(cls, monkeypatch):
    g = _load("stdper_iso_n160_d3" if cls == "StdPeriodic" else "ratquad_iso_n180_d2")
    k = kernel(g["specs"])

    def no_host_K(*a, **kw):
        raise AssertionError("host-side K: the fused device call was not taken")
    monkeypatch.setattr(k, "K", no_host_K)
    m = gpy_amd.GPRegression(g["X"], g["Y"], k, noise_var=float(g["noise"]))
    assert abs(m.log_likelihood() - g["lml"]) <= TOL_LML * abs(g["lml"])


def test_sparse_and_grid_paths_reject_the_new_kinds():
    X = np.random.default_rng(0).standard_normal((64, 1))
    for k in (gpy_amd.StdPeriodic(1), gpy_amd.RatQuad(1), gpy_amd.RBF(1) * gpy_amd.StdPeriodic(1)):
        with pytest.raises(NotImplementedError, match="RatQuad|StdPeriodic"):
            gpy_amd.SparseGPRegression(X, np.sin(X), kernel=k, num_inducing=8)
    s = L.SparseContext(0)                          # the C-ABI's sparse entry: an error, no crash
    try:
        s.set_data(X, np.sin(X))
        with pytest.raises(L.MI355GPError):
            s.vardtc("stdperiodic", 0, np.array([1.0, 1.0, 1.0]), X[:8].copy(), 0.1)
    finally:
        s.close()
