"""GPU (-m gpu): the MLP and Poly kernels (C-ABI kinds 10 / 11) through the fused exact-GP calls, the stateless kernel entry
points and the host classes, against fixtures from the reference's own code (tests/golden/mlp, made by
tools/make_golden_mlp.py) and against the NumPy restatement in mlp_np.py.  Tolerances as for the other kinds
(tests/test_gpu_linear.py), no case loosened: LML 1e-10 relative, alpha 1e-9, gradients 1e-8, prediction 1e-9, K row 1e-13 x
scale -- the scale being max Kdiag(X) of the expression.  Every comparison prints its figure before it asserts."""
import glob
import os

import numpy as np
import pytest

import gpy_amd
from gpy_amd import _lib as L

import mlp_np as P

pytestmark = pytest.mark.gpu
TOL_LML, TOL_ALPHA, TOL_GRAD, TOL_K, TOL_PRED = 1e-10, 1e-9, 1e-8, 1e-13, 1e-9
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(HERE, "golden", "mlp", "*.npz")))
WITH_GRADX = [n for n in NAMES if "poly" not in n]
LONE = ["mlp_iso_n180_d2", "mlp_ard_active_n160_d3", "mlp_ard_n200_d40", "mlp_ard_x20_n160_d3", "poly_o3_n160_d3"]
kernel = P.gpy_amd_kernel


def _load(name):
    z = np.load(os.path.join(HERE, "golden", "mlp", name + ".npz"))
    g = {k: z[k] for k in z.files}
    g["specs"] = P.load_specs(g["specs"])
    g["nu"] = None if float(g["nu"]) < 0 else float(g["nu"])
    rng = np.random.default_rng(1000 + int(g["gseed"]))
    g["G"] = rng.standard_normal((g["X"].shape[0],) * 2)
    g["G2"] = rng.standard_normal((g["X"].shape[0], g["Xs"].shape[0]))
    return g


def test_the_twelve_cases_are_there():
    assert len(NAMES) == 12 and len(WITH_GRADX) == 9


@pytest.mark.parametrize("name", NAMES)
def test_golden_through_the_c_abi(name):
    g = _load(name)
    specs = P.cabi_specs(g["specs"])
    c = L.Context(0)
    try:
        c.set_data(g["X"], g["Y"])
        if g["nu"] is None:
            info, r = c.exact_inference_sum(specs, g["noise"], want_diag=True)
        else:
            info, r = c.exact_studentt_sum(specs, g["nu"])
        assert info == 0
        dth = P.gpy_dtheta(g["specs"], r["dtheta"])
        K = c.fetch(L.FETCH_K)
        lml, alpha, dth_np, dn_np, _ = P.exact(g["specs"], g["X"], g["Y"], float(g["noise"]), g["nu"])
        scale = P.Kdiag(g["specs"], g["X"]).max()
        print(name, "vs reference: lml %.2e alpha %.2e dtheta %.2e K %.2e" % (
            abs(r["lml"] - g["lml"]) / abs(g["lml"]), np.linalg.norm(r["alpha"] - g["alpha"]) / np.linalg.norm(g["alpha"]),
            np.abs(dth - g["dtheta"]).max() / np.abs(g["dtheta"]).max(), np.abs(K[0] - g["K_row0"]).max() / scale))
        if g["nu"] is None:
            assert abs(r["dnoise"] - g["dnoise"]) <= TOL_GRAD * abs(g["dnoise"])
        assert abs(r["lml"] - g["lml"]) <= TOL_LML * abs(g["lml"])
        assert np.linalg.norm(r["alpha"] - g["alpha"]) <= TOL_ALPHA * np.linalg.norm(g["alpha"])
        assert np.abs(dth - g["dtheta"]).max() <= TOL_GRAD * np.abs(g["dtheta"]).max()
        assert np.abs(K[0] - g["K_row0"]).max() <= TOL_K * scale
        assert np.array_equal(K, K.T)                               # the same order over q for (i, j) and (j, i)
        assert np.abs(np.diag(K) - P.Kdiag(g["specs"], g["X"])).max() <= TOL_K * scale      # the formula at i == j
        if g["nu"] is None:
            mu, v = c.predict_sum(specs, g["Xs"])
            print(name, "prediction: mu %.2e var %.2e" % (np.abs(mu - g["pred_mu"]).max(), np.abs(v - g["pred_var"]).max()))
            assert np.abs(mu - g["pred_mu"]).max() <= TOL_PRED and np.abs(v - g["pred_var"]).max() <= TOL_PRED
            _, cov = c.predict_sum(specs, g["Xs"], full_cov=True)
            assert np.abs(cov - g["pred_cov"]).max() <= TOL_PRED
            cb = c.covariance_between_points(specs, g["Xs"][:5].copy(), g["Xs"][5:].copy())
            assert np.abs(cb - g["pred_cov"][:5, 5:]).max() <= TOL_PRED
        # the NumPy restatement
        assert abs(r["lml"] - lml) <= TOL_LML * abs(lml)
        assert np.linalg.norm(r["alpha"] - alpha) <= TOL_ALPHA * np.linalg.norm(alpha)
        assert np.abs(dth - dth_np).max() <= TOL_GRAD * np.abs(dth_np).max()
        assert np.abs(K[0] - P.expr(g["specs"], g["X"])[0][0]).max() <= TOL_K * scale
    finally:
        c.close()


@pytest.mark.parametrize("name", [n for n in NAMES if not n.startswith("studentt")])
def test_golden_through_gpregression(name):
    g = _load(name)
    k = kernel(g["specs"])
    m = gpy_amd.GPRegression(g["X"], g["Y"], k, noise_var=float(g["noise"]))
    assert abs(m.log_likelihood() - g["lml"]) <= TOL_LML * abs(g["lml"])
    gref = np.concatenate([g["dtheta"], [g["dnoise"]]])
    print(name, "gradient %.2e" % (np.abs(m.gradient - gref).max() / np.abs(gref).max()))
    assert np.abs(m.gradient - gref).max() <= TOL_GRAD * np.abs(gref).max()
    mu, var = m.predict_noiseless(g["Xs"])
    assert np.abs(mu - g["pred_mu"]).max() <= TOL_PRED and np.abs(var - g["pred_var"]).max() <= TOL_PRED
    scale = P.Kdiag(g["specs"], g["X"]).max()
    assert np.abs(k.Kdiag(g["Xs"]) - g["Kdiag_Xs"]).max() <= TOL_K * scale


def test_studentt_through_the_inference_class():
    g = _load("studentt_mlp_rbf_n160_d3")
    k = kernel(g["specs"])
    post, lml, gd = gpy_amd.ExactStudentTInference().inference(k, g["X"], g["Y"], g["nu"])
    assert abs(lml - g["lml"]) <= TOL_LML * abs(g["lml"])
    assert abs(float(gd["dL_dnu"]) - g["dnoise"]) <= TOL_GRAD * abs(g["dnoise"])
    k.update_gradients_full(gd["dL_dK"], g["X"])
    assert np.abs(k.gradient - g["dtheta"]).max() <= TOL_GRAD * np.abs(g["dtheta"]).max()


@pytest.mark.parametrize("name", WITH_GRADX)
def test_gradients_X_against_the_golden(name):
    g = _load(name)
    k = kernel(g["specs"])
    gx = k.gradients_X(g["G"], g["X"])                               # X2 None: the weights c + c^T (mlp.py:124-127)
    gx2 = k.gradients_X(g["G2"], g["X"], g["Xs"])
    print(name, "gradX %.2e gradX2 %.2e" % (np.abs(gx - g["gradX"]).max() / np.abs(g["gradX"]).max(),
                                            np.abs(gx2 - g["gradX2"]).max() / np.abs(g["gradX2"]).max()))
    assert np.abs(gx - g["gradX"]).max() <= TOL_GRAD * np.abs(g["gradX"]).max()
    assert np.abs(gx2 - g["gradX2"]).max() <= TOL_GRAD * np.abs(g["gradX2"]).max()
    ref = P.gradients_X(g["specs"], g["G"], g["X"])
    assert np.abs(gx - ref).max() <= TOL_GRAD * np.abs(ref).max()


@pytest.mark.parametrize("name", LONE)
def test_single_kernel_entry_points(name):
    g = _load(name)
    spec = g["specs"][0]
    k = kernel(g["specs"])
    X = g["X"]
    scale = P.Kdiag(g["specs"], np.vstack([X, g["Xs"]])).max()
    Kp = k.K(X, g["Xs"])                                             # rectangular
    ref = P.leaf_parts(spec, X, g["Xs"])[0]
    assert Kp.shape == ref.shape and np.abs(Kp - ref).max() <= TOL_K * scale
    Ks = k.K(X)                                                      # square: bitwise symmetric, the diagonal is the formula
    assert np.array_equal(Ks, Ks.T) and np.abs(Ks - P.leaf_parts(spec, X)[0]).max() <= TOL_K * scale
    assert np.abs(k.Kdiag(X) - np.diag(Ks)).max() <= TOL_K * scale   # Kdiag on the host class
    k.update_gradients_full(g["G2"], X, g["Xs"])                     # a non-symmetric rectangular dL_dK
    got = np.atleast_1d(k.gradient).copy()
    want = np.array([np.sum(g["G2"] * d) for d in P.leaf_parts(spec, X, g["Xs"])[1]])
    print(name, "rectangular %.2e" % (np.abs(got - want).max() / np.abs(want).max()))
    assert got.shape == want.shape and np.abs(got - want).max() <= TOL_GRAD * np.abs(want).max()
    k.update_gradients_full(g["G"], X)                               # square, not symmetric
    got = np.atleast_1d(k.gradient).copy()
    want = np.array([np.sum(g["G"] * d) for d in P.leaf_parts(spec, X)[1]])
    assert np.abs(got - want).max() <= TOL_GRAD * np.abs(want).max()
    th = spec[2]
    raw = L.update_gradients_full(spec[0], spec[1], th, g["G"], np.ascontiguousarray(X[:, spec[3]]), None)
    assert raw.size == th.size                                       # theta and dtheta have the same length
    if spec[0] == "poly":
        assert raw[3] == 0.0                                         # ... the slot of the fixed order holds 0


def _fd_predict(specs, X, alpha, Lc, Xs, h=1e-5):
    """central differences of the RESTATEMENT's prediction (mlp_np.predict, itself checked against the fixtures)"""
    D = Xs.shape[1]
    dmu = np.zeros((Xs.shape[0], D))
    dvar = np.zeros((Xs.shape[0], D))
    for q in range(D):
        e = np.zeros(D)
        e[q] = h
        mp, vp = P.predict(specs, X, alpha, Lc, Xs + e)
        mm, vm = P.predict(specs, X, alpha, Lc, Xs - e)
        dmu[:, q] = (mp - mm)[:, 0] / (2 * h)
        dvar[:, q] = (vp - vm)[:, 0] / (2 * h)
    return dmu, dvar


@pytest.mark.parametrize("name", ["mlp_ard_active_n160_d3", "mlpard_rbf_bias_n160_d3", "mlp0_x_rbf12_n160_d3"])
def test_predictive_gradients_against_central_differences(name):
    """a lone MLP, a sum (both on the device) and a product (composed on the host from the device's gradients_X)"""
    g = _load(name)
    specs, X, Y, noise = g["specs"], g["X"], g["Y"], float(g["noise"])
    m = gpy_amd.GPRegression(X, Y, kernel(specs), noise_var=noise)
    Xs = g["Xs"][:6]
    dmu, dvar = m.predictive_gradients(Xs)
    _, alpha, _, _, Lc = P.exact(specs, X, Y, noise)
    fmu, fvar = _fd_predict(specs, X, alpha, Lc, Xs)
    print(name, "dmu %.2e dvar %.2e" % (np.abs(dmu[:, :, 0] - fmu).max(), np.abs(dvar - fvar).max()))
    assert np.abs(dmu[:, :, 0] - fmu).max() <= 1e-6 * max(1.0, np.abs(fmu).max())
    assert np.abs(dvar - fvar).max() <= 1e-6 * max(1.0, np.abs(fvar).max())


def test_predictive_gradients_with_a_poly_leaf_are_refused():
    g = _load("poly_o2_rbf_bias_n160_d3")
    m = gpy_amd.GPRegression(g["X"], g["Y"], kernel(g["specs"]), noise_var=float(g["noise"]))
    with pytest.raises(NotImplementedError, match="Poly"):
        m.predictive_gradients(g["Xs"][:3])
    c = L.Context(0)
    try:
        c.set_data(g["X"], g["Y"])
        info, _ = c.exact_inference_sum(g["specs"], g["noise"])
        assert info == 0
        with pytest.raises(L.MI355GPError, match="Poly"):
            c.predictive_gradients(g["specs"], g["Xs"][:3].copy())
    finally:
        c.close()
    with pytest.raises(L.MI355GPError, match="Poly"):
        L.gradients_X("poly", 0, np.array([1.0, 1.0, 1.0, 2.0]), g["G"], g["X"], None)


@pytest.mark.parametrize("name", ["mlpard_rbf_bias_n160_d3", "poly_o2_rbf_bias_n160_d3"])
def test_checkgrad_on_the_sum(name):
    g = _load(name)
    m = gpy_amd.GPRegression(g["X"], g["Y"], kernel(g["specs"]), noise_var=float(g["noise"]))
    assert m.checkgrad()


@pytest.mark.parametrize("N", [4096, 4224])
def test_sum_at_persistent_cholesky_sizes(N):
    """MLP(ARD, D = 40) + RBF: the persistent-Cholesky sizes, a ragged last tile at 4224, two 32-dimension record groups"""
    rng = np.random.default_rng(N)
    D = 40
    X = rng.standard_normal((N, D))
    w = rng.standard_normal(D) / np.sqrt(D)
    Y = (np.tanh(2.0 * (X @ w)) + 0.5 * np.sin(X[:, 0]) + 0.1 * rng.standard_normal(N))[:, None]
    specs = [("mlp", 1, np.concatenate([[1.2], np.linspace(0.02, 0.06, D), [0.4]]), np.arange(D), 0),
             ("rbf", 0, np.array([0.5, 6.0]), np.arange(D), 0)]
    c = L.Context(0)
    try:
        c.set_data(X, Y)
        info, r = c.exact_inference_sum(specs, 0.05)
        assert info == 0
        info2, r2 = c.exact_inference_sum(specs, 0.05)              # fixed-order reductions: the same bits again
        assert info2 == 0 and r["dtheta"].tobytes() == r2["dtheta"].tobytes() and r["lml"] == r2["lml"]
    finally:
        c.close()
    lml, alpha, dth = P.exact_sum_large(specs, X, Y, 0.05)
    print(N, "lml %.2e alpha %.2e dtheta %.2e" % (abs(r["lml"] - lml) / abs(lml), np.linalg.norm(r["alpha"] - alpha) /
                                                  np.linalg.norm(alpha), np.abs(r["dtheta"] - dth).max() / np.abs(dth).max()))
    assert abs(r["lml"] - lml) <= TOL_LML * abs(lml)
    assert np.linalg.norm(r["alpha"] - alpha) <= TOL_ALPHA * np.linalg.norm(alpha)
    assert np.abs(r["dtheta"] - dth).max() <= TOL_GRAD * np.abs(dth).max()


@pytest.mark.parametrize("name", ["mlp0_x_rbf12_n160_d3", "mlp_ard_n200_d40", "poly0_x_rbf12_n160_d3"])
def test_two_evaluations_give_identical_bits(name):
    g = _load(name)
    out = []
    for _ in range(2):
        c = L.Context(0)
        try:
            c.set_data(g["X"], g["Y"])
            info, r = c.exact_inference_sum(g["specs"], g["noise"])
            assert info == 0
            out.append(r["dtheta"].tobytes() + np.float64(r["lml"]).tobytes())
        finally:
            c.close()
    assert out[0] == out[1]


@pytest.mark.parametrize("name", ["mlp_iso_n180_d2", "mlp_ard_active_n160_d3", "poly_o3_n160_d3"])
def test_lone_kernel_takes_the_fused_call(name, monkeypatch):
    g = _load(name)
    k = kernel(g["specs"])

    def no_host_K(*a, **kw):
        raise AssertionError("host-side K: the fused device call was not taken")
    monkeypatch.setattr(k, "K", no_host_K)
    m = gpy_amd.GPRegression(g["X"], g["Y"], k, noise_var=float(g["noise"]))
    assert abs(m.log_likelihood() - g["lml"]) <= TOL_LML * abs(g["lml"])
    gref = np.concatenate([g["dtheta"], [g["dnoise"]]])
    assert m.gradient.shape == gref.shape and np.abs(m.gradient - gref).max() <= TOL_GRAD * np.abs(gref).max()
    mu, var = m.predict_noiseless(g["Xs"])                           # mi355gp_predict: per-point Kdiag
    assert np.abs(mu - g["pred_mu"]).max() <= TOL_PRED and np.abs(var - g["pred_var"]).max() <= TOL_PRED


THETA = {"mlp": np.array([1.0, 1.0, 1.0]), "poly": np.array([1.0, 1.0, 1.0, 2.0])}


@pytest.mark.parametrize("kind,cls", [("mlp", "MLP"), ("poly", "Poly")])
def test_sparse_and_grid_paths_reject_the_kind(kind, cls):
    from gpy_amd import grid as G
    X = np.random.default_rng(0).standard_normal((64, 1))
    leaf = getattr(gpy_amd, cls)
    for k in (leaf(1), gpy_amd.RBF(1) + leaf(1), gpy_amd.RBF(1) * leaf(1)):
        with pytest.raises(NotImplementedError, match=cls):
            gpy_amd.SparseGPRegression(X, np.sin(X), kernel=k, num_inducing=8)
    s = L.SparseContext(0)                          # the C-ABI's sparse entry: an error naming the kind, no crash
    try:
        s.set_data(X, np.sin(X))
        with pytest.raises(L.MI355GPError, match=cls):
            s.vardtc(kind, 0, THETA[kind], X[:8].copy(), 0.1)
        with pytest.raises(L.MI355GPError, match=cls):
            s.vardtc_sum([("rbf", 0, np.array([1.0, 1.0]), None, 0), (kind, 0, THETA[kind], None, 0)], X[:8].copy(), 0.1)
    finally:
        s.close()
    gr = G.GridContext.loopback(1, 1)
    try:
        with pytest.raises(NotImplementedError, match=cls):
            gr.exact_inference(kind, False, THETA[kind], 0.1)
    finally:
        gr.close()


@pytest.mark.parametrize("kind,cls", [("mlp", "MLP"), ("poly", "Poly")])
def test_kern_Kdiag_of_the_c_abi_rejects_the_kind(kind, cls):
    with pytest.raises(L.MI355GPError, match="diagonal of a %s .* depends on the points" % cls):
        L.kern_Kdiag(kind, THETA[kind], 4)


def test_bad_parameters_are_refused_before_any_launch():
    X = np.random.default_rng(1).standard_normal((32, 2))
    bad = [("mlp", 0, [0.0, 1.0, 1.0], "MLP"), ("mlp", 0, [1.0, -1.0, 1.0], "MLP"), ("mlp", 1, [1.0, 1.0, 0.0, 1.0], "MLP"),
           ("mlp", 0, [1.0, 1.0, 0.0], "MLP"), ("poly", 0, [0.0, 1.0, 1.0, 2.0], "Poly"), ("poly", 0, [1.0, -2.0, 1.0, 2.0], "Poly"),
           ("poly", 0, [1.0, 1.0, 0.0, 2.0], "Poly")]
    for kind, ard, th, cls in bad:
        with pytest.raises(L.MI355GPError, match="%s.*must be positive" % cls):
            L.kern_K(kind, ard, np.array(th), X)
    with pytest.raises(L.MI355GPError, match="order 0.5 of a Poly .* must be at least 1"):
        L.kern_K("poly", 0, np.array([1.0, 1.0, 1.0, 0.5]), X)
    c = L.Context(0)
    try:
        c.set_data(X, X[:, :1].copy())
        with pytest.raises(L.MI355GPError, match="MLP.*must be positive"):
            c.exact_inference_sum([("rbf", 0, np.array([1.0, 1.0]), None, 0), ("mlp", 1, np.array([1.0, 1.0, 0.0, 1.0]), None, 0)], 0.1)
        with pytest.raises(L.MI355GPError, match="Poly .* must be at least 1"):
            c.exact_inference("poly", 0, np.array([1.0, 1.0, 1.0, 0.0]), 0.1)
    finally:
        c.close()
