"""CPU: the NumPy restatement of expressions with MLP / Poly parts (mlp_np.py, scaled-input formulation) against the fixtures
made from the reference's own code (tests/golden/mlp, tools/make_golden_mlp.py) and against central differences of the log
marginal likelihood in every parameter; and the host-side pieces of `gpy_amd.MLP` / `gpy_amd.Poly` that need no GPU.

Tolerances are the project's (tests/test_gpu_linear.py), no case loosened: LML 1e-10 relative, alpha 1e-9, gradients 1e-8 of the
largest gradient, prediction 1e-9, K row 1e-13 x scale with scale = max Kdiag(X) of the expression.  The x20 fixture drives
the asin argument to within 0.012 of 1, the ill-conditioned end of the formula; the restatement still meets every bound
there (each test prints its figures)."""
import glob
import os

import numpy as np
import pytest

import gpy_amd
from gpy_amd import _lib as L
from gpy_amd import kern as GK

import mlp_np as P

TOL_LML, TOL_ALPHA, TOL_GRAD, TOL_K, TOL_PRED = 1e-10, 1e-9, 1e-8, 1e-13, 1e-9
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(HERE, "golden", "mlp", "*.npz")))
LONE_MLP = [n for n in NAMES if n.startswith("mlp_")]


def _load(name):
    z = np.load(os.path.join(HERE, "golden", "mlp", name + ".npz"))
    g = {k: z[k] for k in z.files}
    g["specs"] = P.load_specs(g["specs"])
    g["nu"] = None if float(g["nu"]) < 0 else float(g["nu"])
    rng = np.random.default_rng(1000 + int(g["gseed"]))
    g["G"] = rng.standard_normal((g["X"].shape[0],) * 2)
    g["G2"] = rng.standard_normal((g["X"].shape[0], g["Xs"].shape[0]))
    g["gdiag"] = np.random.default_rng(2000 + int(g["gseed"])).standard_normal(g["X"].shape[0])
    return g


def test_the_twelve_cases_are_there():
    assert len(NAMES) == 12 and len(LONE_MLP) == 4
    for n in NAMES:
        assert os.path.getsize(os.path.join(HERE, "golden", "mlp", n + ".npz")) < 1 << 20


@pytest.mark.parametrize("name", NAMES)
def test_restatement_against_the_reference(name):
    g = _load(name)
    specs, X, Y = g["specs"], g["X"], g["Y"]
    lml, alpha, dth, dn, Lc = P.exact(specs, X, Y, float(g["noise"]), g["nu"])
    scale = P.Kdiag(specs, X).max()
    figures = dict(lml=abs(lml - g["lml"]) / abs(g["lml"]),
                   alpha=np.linalg.norm(alpha - g["alpha"]) / np.linalg.norm(g["alpha"]),
                   dtheta=np.abs(dth - g["dtheta"]).max() / np.abs(g["dtheta"]).max(),
                   K=np.abs(P.expr(specs, X)[0][0] - g["K_row0"]).max() / scale)
    print(name, figures)
    assert figures["lml"] <= TOL_LML
    assert figures["alpha"] <= TOL_ALPHA
    assert figures["dtheta"] <= TOL_GRAD
    assert figures["K"] <= TOL_K
    if g["nu"] is None:
        assert abs(dn - g["dnoise"]) <= TOL_GRAD * abs(g["dnoise"])
    assert np.abs(P.Kdiag(specs, g["Xs"]) - g["Kdiag_Xs"]).max() <= TOL_K * scale
    if g["nu"] is None:
        mu, var = P.predict(specs, X, alpha, Lc, g["Xs"])
        _, cov = P.predict(specs, X, alpha, Lc, g["Xs"], full_cov=True)
        assert np.abs(mu - g["pred_mu"]).max() <= TOL_PRED
        assert np.abs(var - g["pred_var"]).max() <= TOL_PRED
        assert np.abs(cov - g["pred_cov"]).max() <= TOL_PRED
    if any(s[0] == "poly" for s in specs):
        assert "gradX" not in g and "gradX2" not in g                # the reference has no gradients_X for Poly
        with pytest.raises(AssertionError, match="Poly has no gradients_X"):
            P.gradients_X(specs, g["G"], X)
        return
    gx = P.gradients_X(specs, g["G"], X)
    gx2 = P.gradients_X(specs, g["G2"], X, g["Xs"])
    print(name, "gradX %.2e gradX2 %.2e" % (np.abs(gx - g["gradX"]).max() / np.abs(g["gradX"]).max(),
                                            np.abs(gx2 - g["gradX2"]).max() / np.abs(g["gradX2"]).max()))
    assert np.abs(gx - g["gradX"]).max() <= TOL_GRAD * np.abs(g["gradX"]).max()
    assert np.abs(gx2 - g["gradX2"]).max() <= TOL_GRAD * np.abs(g["gradX2"]).max()


@pytest.mark.parametrize("name", [n for n in NAMES if "d40" not in n])
def test_gradients_against_central_differences_of_the_lml(name):
    g = _load(name)
    specs, X, Y, noise, nu = g["specs"], g["X"], g["Y"], float(g["noise"]), g["nu"]
    dth = P.exact(specs, X, Y, noise, nu)[2]
    fd, k = np.zeros_like(dth), 0
    for i, s in enumerate(specs):
        for j in range(P.n_params(s)):
            h = 1e-6 * max(1.0, abs(s[2][j]))
            lm = []
            for sign in (1.0, -1.0):
                th = s[2].copy()
                th[j] += sign * h
                sp = list(specs)
                sp[i] = (s[0], s[1], th, s[3], s[4])
                lm.append(P.exact(sp, X, Y, noise, nu)[0])
            fd[k] = (lm[0] - lm[1]) / (2 * h)
            k += 1
    assert k == dth.size
    # central differences of an LML of size |lml| carry ~ eps |lml| / h of rounding
    assert np.abs(fd - dth).max() <= 1e-5 * max(1.0, np.abs(dth).max())


def test_the_lean_restatement_of_a_sum_agrees_with_the_dense_one():
    """`exact_sum_large` (what the N = 4096 GPU cases are held against) on the small sum fixtures"""
    for name in ("mlpard_rbf_bias_n160_d3", "mlp_iso_n180_d2", "mlp_ard_active_n160_d3", "mlp_ard_n200_d40"):
        g = _load(name)
        a = P.exact(g["specs"], g["X"], g["Y"], float(g["noise"]))
        b = P.exact_sum_large(g["specs"], g["X"], g["Y"], float(g["noise"]))
        assert abs(a[0] - b[0]) <= 1e-12 * abs(a[0]) and np.abs(a[1] - b[1]).max() <= 1e-11 * np.abs(a[1]).max()
        assert np.abs(a[2] - b[2]).max() <= 1e-11 * np.abs(a[2]).max()


def test_constructor_checks_and_parameters():
    k = gpy_amd.MLP(3)
    assert k.variance.values.tolist() == [1.0] and k.weight_variance.values.tolist() == [1.0]
    assert k.bias_variance.values.tolist() == [1.0] and not k.ARD and k.name == "mlp" and k.kind == "mlp"
    assert [p.name for p in k.parameters] == ["variance", "weight_variance", "bias_variance"]
    k = gpy_amd.MLP(3, weight_variance=0.5, ARD=True)                 # mlp.py:39-42: one value is spread over the dimensions
    assert k.weight_variance.values.tolist() == [0.5, 0.5, 0.5]
    with pytest.raises(AssertionError, match="Only one weight variance needed for non-ARD kernel"):
        gpy_amd.MLP(2, weight_variance=[1.0, 2.0])
    with pytest.raises(AssertionError):
        gpy_amd.MLP(2, active_dims=[0, 1, 2])
    p = gpy_amd.Poly(2)
    assert [q.name for q in p.parameters] == ["variance", "scale", "bias"] and p.order == 3.0 and p.name == "poly"
    assert p.variance.values.tolist() == [1.0] and p.scale.values.tolist() == [1.0] and p.bias.values.tolist() == [1.0]
    with pytest.raises(AssertionError, match="The order of the polynomial has to be at least 1."):
        gpy_amd.Poly(2, order=0.5)
    assert gpy_amd.kern.MLP is gpy_amd.MLP and GK.KERNEL_CLASSES["mlp"] is gpy_amd.MLP
    assert gpy_amd.kern.Poly is gpy_amd.Poly and GK.KERNEL_CLASSES["poly"] is gpy_amd.Poly
    assert not hasattr(gpy_amd.MLP, "input_sensitivity") and not hasattr(gpy_amd.Poly, "input_sensitivity")


def test_theta_and_part_specs():
    assert L.KIND_IDS["mlp"] == 10 and L.KIND_IDS["poly"] == 11
    assert gpy_amd.MLP(3, 1.3, 0.7, 0.4)._theta().tolist() == [1.3, 0.7, 0.4]
    a = gpy_amd.MLP(2, 1.3, [0.7, 1.6], 0.4, ARD=True, active_dims=[0, 2])
    assert a._theta().tolist() == [1.3, 0.7, 1.6, 0.4]
    p = gpy_amd.Poly(1, 0.6, 0.25, 1.1, order=2, active_dims=[1])
    assert p._theta().tolist() == [0.6, 0.25, 1.1, 2.0]
    k = a + gpy_amd.RBF(3) * p + gpy_amd.Linear(3) * gpy_amd.MLP(3) + gpy_amd.Bias(3)
    specs = k.part_specs()
    assert [(s[0], int(s[1]), s[4]) for s in specs] == [("mlp", 1, 0), ("rbf", 0, 1), ("poly", 0, 1), ("linear", 0, 2),
                                                        ("mlp", 0, 2), ("bias", 0, 0)]
    arr, keep, ntheta = L.make_parts(specs)
    assert ntheta == 4 + 2 + 4 + 1 + 3 + 1 and arr[0].kind == 10 and arr[0].ard == 1 and arr[0].n_active == 2
    assert arr[2].kind == 11 and arr[2].ard == 0 and arr[2].term == 1 and arr[4].kind == 10 and arr[4].term == 2
    # the fused gradient vector of the expression: the slot of Poly's order is dropped on install
    k._install_fused(np.arange(15.0))
    assert a.variance.gradient == 0.0 and a.weight_variance.gradient.tolist() == [1.0, 2.0] and a.bias_variance.gradient == 3.0
    assert (p.variance.gradient, p.scale.gradient, p.bias.gradient) == (6.0, 7.0, 8.0)
    assert k.parts[2].parts[0].variances.gradient == 10.0 and k.parts[2].parts[1].bias_variance.gradient == 13.0
    assert k.parts[3].variance.gradient == 14.0


def test_to_dict_round_trip_copy_and_reset():
    k = gpy_amd.MLP(2, 1.3, [0.7, 1.6], 0.4, ARD=True, active_dims=[0, 2], name="nn")
    d = k.to_dict()
    assert d["class"] == "GPy.kern.MLP" and d["weight_variance"] == [0.7, 1.6] and d["bias_variance"] == [0.4] and d["ARD"] is True
    for c in (gpy_amd.MLP.from_dict(d), k.copy()):
        assert c.to_dict() == d and c is not k
    k.reset_gradients()
    assert k.weight_variance.gradient.tolist() == [0.0, 0.0] and k.variance.gradient == 0.0 and k.bias_variance.gradient == 0.0
    p = gpy_amd.Poly(2, 0.6, 0.25, 1.1, order=2.0, name="pp")
    d = p.to_dict()
    assert d["class"] == "GPy.kern.Poly" and d["order"] == 2.0 and d["scale"] == [0.25] and d["bias"] == [1.1]
    for c in (gpy_amd.Poly.from_dict(d), p.copy()):
        assert c.to_dict() == d and c is not p and c.order == 2.0
    p.reset_gradients()
    assert p.scale.gradient == 0.0


def test_exact_only_and_point_dependent_diagonal():
    assert "mlp" in GK.EXACT_ONLY_KINDS and "poly" in GK.EXACT_ONLY_KINDS
    for leaf, nm in ((gpy_amd.MLP(2), "MLP"), (gpy_amd.Poly(2), "Poly")):
        assert isinstance(leaf, GK.DEVICE_KERNELS)
        assert GK.diag_depends_on_point(leaf) and GK.diag_depends_on_point(gpy_amd.RBF(2) + leaf)
        assert GK.diag_depends_on_point(gpy_amd.RBF(2) * leaf) and not GK.has_coregionalize(gpy_amd.RBF(2) + leaf)
        assert GK.exact_only_leaves(gpy_amd.RBF(2) + leaf) == [nm]
    assert not GK.diag_depends_on_point(gpy_amd.RBF(2) + gpy_amd.Bias(2))


def test_poly_raises_what_the_reference_raises():
    p = gpy_amd.Poly(2)
    X = np.zeros((3, 2))
    with pytest.raises(NotImplementedError, match="Poly"):
        p.gradients_X(np.zeros((3, 3)), X)
    with pytest.raises(NotImplementedError, match="Poly"):
        p.gradients_X_diag(np.zeros(3), X)
    with pytest.raises(NotImplementedError, match="Poly"):
        p.update_gradients_diag(np.zeros(3), X)
    with pytest.raises(NotImplementedError, match="predictive_gradients"):
        (gpy_amd.RBF(2) + p).gradients_X(np.zeros((3, 3)), X)


def test_sparse_model_refuses_both_on_the_host():
    X = np.random.default_rng(0).standard_normal((64, 1))
    for leaf, nm in ((gpy_amd.MLP(1), "MLP"), (gpy_amd.Poly(1), "Poly")):
        for k in (leaf, gpy_amd.RBF(1) + leaf, gpy_amd.RBF(1) * leaf):
            with pytest.raises(NotImplementedError, match=nm):
                gpy_amd.SparseGPRegression(X, np.sin(X), kernel=k, num_inducing=8)


@pytest.mark.parametrize("name", NAMES)
def test_host_Kdiag_against_the_fixture(name):
    g = _load(name)
    k = P.gpy_amd_kernel(g["specs"])
    scale = P.Kdiag(g["specs"], g["X"]).max()
    assert np.abs(k.Kdiag(g["Xs"]) - g["Kdiag_Xs"]).max() <= TOL_K * scale


@pytest.mark.parametrize("name", LONE_MLP)
def test_host_diagonal_gradients_against_the_reference(name):
    """update_gradients_diag / gradients_X_diag of `gpy_amd.MLP` are NumPy: against the reference's values in the fixture and
    against the restatement's derivative of Kdiag"""
    g = _load(name)
    k = P.gpy_amd_kernel(g["specs"])
    k.update_gradients_diag(g["gdiag"], g["X"])
    got = np.concatenate([np.atleast_1d(k.variance.gradient), np.atleast_1d(k.weight_variance.gradient),
                          np.atleast_1d(k.bias_variance.gradient)])
    gx = k.gradients_X_diag(g["gdiag"], g["X"])
    dth, dX = P.mlp_diag_grads(g["specs"][0], g["gdiag"], g["X"])
    for want_th, want_x in ((g["diag_dtheta"], g["gradXdiag"]), (dth, dX)):
        assert got.shape == want_th.shape and gx.shape == want_x.shape
        assert np.abs(got - want_th).max() <= TOL_GRAD * np.abs(want_th).max()
        assert np.abs(gx - want_x).max() <= TOL_GRAD * np.abs(want_x).max()


@pytest.mark.parametrize("name", ["mlpard_rbf_bias_n160_d3", "mlp0_x_rbf12_n160_d3", "lin0_x_mlp12_n160_d3"])
def test_gradients_X_diag_of_expressions_against_central_differences(name):
    g = _load(name)
    k = P.gpy_amd_kernel(g["specs"])
    w = np.random.default_rng(3).standard_normal(g["Xs"].shape[0])
    h = 1e-6
    fd = np.zeros(g["Xs"].shape)
    for q in range(g["Xs"].shape[1]):
        e = np.zeros(g["Xs"].shape[1])
        e[q] = h
        fd[:, q] = w * (P.Kdiag(g["specs"], g["Xs"] + e) - P.Kdiag(g["specs"], g["Xs"] - e)) / (2 * h)
    got = k.gradients_X_diag(w, g["Xs"])
    assert np.abs(got - fd).max() <= 1e-6 * max(1.0, np.abs(fd).max())
