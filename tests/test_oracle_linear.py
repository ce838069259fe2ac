"""CPU: the NumPy restatement of expressions with Linear parts (linear_np.py) against the fixtures made from the reference's
own code (tests/golden/linear, tools/make_golden_linear.py) and against central differences of the log marginal likelihood
in every parameter; and the host-side pieces of `gpy_amd.Linear` that need no GPU.

Tolerances are the project's (tests/test_gpu_periodic_kernels.py): LML 1e-10 relative, alpha 1e-9, gradients 1e-8 of the
largest gradient, prediction 1e-9, K row 1e-13 x scale with scale = max Kdiag(X) of the expression (a Linear part has no
variance that bounds K).

No case needs a loose factor.  The +50 fixture has a Ky of condition number 1.0e7 (entries up to 6.7e3 over a noise of 0.1,
against ~2e3 for the other cases) and a prediction variance that is the difference of two numbers of size 6.7e3; it still
meets the standard tolerances because the restatement forms alpha and the variance from the Cholesky factor (two triangular
solves, |L^-1 Kx|^2) as the reference and the device do.  Measured here, reference against restatement: LML 5e-12, alpha
1.9e-10, gradients 7e-12 relative, prediction variance 1.3e-11 absolute.  (With an explicit inverse in place of the
triangular solves the variance is off by 2e-6: do not "simplify" linear_np.predict.)"""
import glob
import os

import numpy as np
import pytest

import gpy_amd
from gpy_amd import _lib as L
from gpy_amd import kern as GK

import linear_np as P

TOL_LML, TOL_ALPHA, TOL_GRAD, TOL_K, TOL_PRED = 1e-10, 1e-9, 1e-8, 1e-13, 1e-9
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(HERE, "golden", "linear", "*.npz")))


def _load(name):
    z = np.load(os.path.join(HERE, "golden", "linear", name + ".npz"))
    g = {k: z[k] for k in z.files}
    g["specs"] = P.load_specs(g["specs"])
    g["nu"] = None if float(g["nu"]) < 0 else float(g["nu"])
    rng = np.random.default_rng(1000 + int(g["gseed"]))
    g["G"] = rng.standard_normal((g["X"].shape[0],) * 2)
    g["G2"] = rng.standard_normal((g["X"].shape[0], g["Xs"].shape[0]))
    return g



def test_the_eight_cases_are_there():
    assert len(NAMES) == 8


@pytest.mark.parametrize("name", NAMES)
def test_restatement_against_the_reference(name):
    g = _load(name)
    specs, X, Y = g["specs"], g["X"], g["Y"]
    lml, alpha, dth, dn, Lc = P.exact(specs, X, Y, float(g["noise"]), g["nu"])
    figures = dict(lml=abs(lml - g["lml"]) / abs(g["lml"]),
                   alpha=np.linalg.norm(alpha - g["alpha"]) / np.linalg.norm(g["alpha"]),
                   dtheta=np.abs(dth - g["dtheta"]).max() / np.abs(g["dtheta"]).max())
    print(name, figures)
    assert figures["lml"] <= TOL_LML
    assert figures["alpha"] <= TOL_ALPHA
    assert figures["dtheta"] <= TOL_GRAD
    if g["nu"] is None:
        assert abs(dn - g["dnoise"]) <= TOL_GRAD * abs(g["dnoise"])
    scale = P.Kdiag(specs, X).max()
    assert np.abs(P.expr(specs, X)[0][0] - g["K_row0"]).max() <= TOL_K * scale
    assert np.abs(P.Kdiag(specs, g["Xs"]) - g["Kdiag_Xs"]).max() <= TOL_K * scale
    if g["nu"] is None:
        mu, var = P.predict(specs, X, alpha, Lc, g["Xs"])
        _, cov = P.predict(specs, X, alpha, Lc, g["Xs"], full_cov=True)
        assert np.abs(mu - g["pred_mu"]).max() <= TOL_PRED
        assert np.abs(var - g["pred_var"]).max() <= TOL_PRED
        assert np.abs(cov - g["pred_cov"]).max() <= TOL_PRED
    gx = P.gradients_X(specs, g["G"], X)
    assert np.abs(gx - g["gradX"]).max() <= TOL_GRAD * np.abs(g["gradX"]).max()
    gx2 = P.gradients_X(specs, g["G2"], X, g["Xs"])
    assert np.abs(gx2 - g["gradX2"]).max() <= TOL_GRAD * np.abs(g["gradX2"]).max()


@pytest.mark.parametrize("name", NAMES)
def test_gradients_against_central_differences_of_the_lml(name):
    g = _load(name)
    specs, X, Y, noise, nu = g["specs"], g["X"], g["Y"], float(g["noise"]), g["nu"]
    dth = P.exact(specs, X, Y, noise, nu)[2]
    fd, k = np.zeros_like(dth), 0
    for i, s in enumerate(specs):
        for j in range(s[2].size):
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
    # central differences of an LML of size |lml| carry ~ eps |lml| / h of rounding (times its condition number for the +50 case)
    assert np.abs(fd - dth).max() <= (1e-3 if "shift50" in name else 1e-5) * max(1.0, np.abs(dth).max())


def test_the_lean_restatement_of_a_sum_agrees_with_the_dense_one():
    """`exact_sum_large` (what the N = 4096 GPU cases are held against) on the small sum fixtures"""
    for name in ("linard_rbf_bias_n160_d3", "linear_iso_n180_d2", "linear_ard_active_n160_d3"):
        g = _load(name)
        a = P.exact(g["specs"], g["X"], g["Y"], float(g["noise"]))
        b = P.exact_sum_large(g["specs"], g["X"], g["Y"], float(g["noise"]))
        assert abs(a[0] - b[0]) <= 1e-12 * abs(a[0]) and np.abs(a[1] - b[1]).max() <= 1e-11 * np.abs(a[1]).max()
        assert np.abs(a[2] - b[2]).max() <= 1e-11 * np.abs(a[2]).max()


def test_constructor_checks_and_parameters():
    k = gpy_amd.Linear(3)
    assert k.variances.values.tolist() == [1.0] and not k.ARD and k.name == "linear" and k.kind == "linear"
    k = gpy_amd.Linear(3, ARD=True)
    assert k.variances.values.tolist() == [1.0, 1.0, 1.0]
    assert [p.name for p in k.parameters] == ["variances"]
    with pytest.raises(AssertionError, match="Only one variance needed for non-ARD kernel"):
        gpy_amd.Linear(2, variances=[1.0, 2.0])
    with pytest.raises(AssertionError, match="bad number of variances, need one ARD variance per input_dim"):
        gpy_amd.Linear(3, variances=[1.0, 2.0], ARD=True)
    with pytest.raises(AssertionError):
        gpy_amd.Linear(2, active_dims=[0, 1, 2])
    assert gpy_amd.kern.Linear is gpy_amd.Linear and GK.KERNEL_CLASSES["linear"] is gpy_amd.Linear


def test_theta_and_part_specs():
    assert L.KIND_IDS["linear"] == 9
    assert gpy_amd.Linear(3, variances=0.7)._theta().tolist() == [0.7]
    a = gpy_amd.Linear(2, variances=[0.7, 1.6], ARD=True, active_dims=[0, 2])
    assert a._theta().tolist() == [0.7, 1.6]
    k = a + gpy_amd.RBF(3) * gpy_amd.Linear(1, active_dims=[1]) + gpy_amd.Bias(3)
    specs = k.part_specs()
    assert [(s[0], int(s[1]), s[4]) for s in specs] == [("linear", 1, 0), ("rbf", 0, 1), ("linear", 0, 1), ("bias", 0, 0)]
    arr, keep, ntheta = L.make_parts(specs)
    assert ntheta == 2 + 2 + 1 + 1 and arr[0].kind == 9 and arr[0].ard == 1 and arr[0].n_active == 2
    assert arr[2].kind == 9 and arr[2].ard == 0 and arr[2].term == 1


def test_to_dict_round_trip_and_copy():
    k = gpy_amd.Linear(2, variances=[0.7, 1.6], ARD=True, active_dims=[0, 2], name="lin")
    d = k.to_dict()
    assert d["class"] == "GPy.kern.Linear" and d["variances"] == [0.7, 1.6] and d["ARD"] is True
    for c in (gpy_amd.Linear.from_dict(d), k.copy()):
        assert c.to_dict() == d and c is not k


def test_exact_only_and_point_dependent_diagonal():
    assert "linear" in GK.EXACT_ONLY_KINDS
    lin = gpy_amd.Linear(2)
    assert GK.diag_depends_on_point(lin) and GK.diag_depends_on_point(gpy_amd.RBF(2) + lin)
    assert GK.diag_depends_on_point(gpy_amd.RBF(2) * lin) and not GK.diag_depends_on_point(gpy_amd.RBF(2) + gpy_amd.Bias(2))
    assert not GK.has_coregionalize(gpy_amd.RBF(2) + lin)
    assert GK.exact_only_leaves(gpy_amd.RBF(2) + lin) == ["Linear"]


@pytest.mark.parametrize("name", NAMES)
def test_host_Kdiag_and_diagonal_gradients(name):
    """Kdiag, update_gradients_diag and gradients_X_diag of the host classes are NumPy: against the fixture and the restatement"""
    g = _load(name)
    k = P.gpy_amd_kernel(g["specs"])
    scale = P.Kdiag(g["specs"], g["X"]).max()
    assert np.abs(k.Kdiag(g["Xs"]) - g["Kdiag_Xs"]).max() <= TOL_K * scale
    w = np.random.default_rng(3).standard_normal(g["Xs"].shape[0])
    h = 1e-6
    fd = np.zeros(g["Xs"].shape)
    for q in range(g["Xs"].shape[1]):
        if any(s[0] == "coregionalize" and s[3][0] == q for s in g["specs"]):
            continue                                              # the output-index column is no continuous input
        e = np.zeros(g["Xs"].shape[1])
        e[q] = h
        fd[:, q] = w * (P.Kdiag(g["specs"], g["Xs"] + e) - P.Kdiag(g["specs"], g["Xs"] - e)) / (2 * h)
    got = k.gradients_X_diag(w, g["Xs"])
    assert np.abs(got - fd).max() <= 1e-6 * max(1.0, np.abs(fd).max())


def test_update_gradients_diag():
    X = np.random.default_rng(5).standard_normal((20, 3))
    w = np.random.default_rng(6).standard_normal(20)
    k = gpy_amd.Linear(2, variances=[0.7, 1.6], ARD=True, active_dims=[0, 2])
    k.update_gradients_diag(w, X)
    assert np.allclose(k.variances.gradient, (w[:, None] * X[:, [0, 2]] ** 2).sum(0), rtol=1e-14)
    k = gpy_amd.Linear(3, variances=0.4)
    k.update_gradients_diag(w, X)
    assert np.allclose(k.variances.gradient, (w[:, None] * X ** 2).sum(), rtol=1e-14)
    assert np.allclose(k.input_sensitivity(), 0.4 * np.ones(3))
