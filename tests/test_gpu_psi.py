"""GPU: the RBF psi-statistics kernels (gpy_amd/csrc/psi.hip) through the stateless C-ABI entry points and the kernel
classes, against the long-double restatement of tests/psi_np.py, at the smallest shapes that cross each boundary the kernels
have: M below / across the 16-wide psi2 tile and the 64-wide psi1 tile (1, 63, 65, 130), N below / across the 16-row
iteration, the 64-row staging block and the 256-row workgroup (1, 63, 65, 257), Q in one padded group (1, 2, 3), two
dimension groups with two reduction records (33, 40), and N = 2051 > the 2048-row chunk with M = 8 (chunk boundary and the
fixed-order combine across chunks).

Bounds (tests/test_oracle_psi.py has the measurement): psi1 1e-13 * variance (the project's K tolerance); psi2 2.3e-14 and
the five gradients 8.5e-14, relative to max |value| -- ten times the float64 restatement's own distance from long double.
Device figures (one MI355X, worst over the cases below): psi1 4.5e-16 absolute, psi2 7.9e-16, dvariance 2.3e-15,
dlengthscale 6.0e-16, dZ 5.2e-16, dmu 8.3e-16, dS 1.0e-15 (iso cases with Q = 3 and Q = 40 included: the summed lengthscale
record over one and over two dimension groups).

The uncertain-input fit (`mi355gp_vardtc_inference_uncertain`, `VarDTC.inference` with a `NormalPosterior`,
`SparseGPRegression(X_variance=)`) is held to the sparse path's tolerances of tests/test_gpu_sparse.py -- log marginal 1e-9,
gradients, woodbury_vector and the predictive mean 1e-6, the predictive variance 1e-5, the lazy M x M matrices 1e-4 --
against the reference's own evaluation in tests/golden/psi/*.npz.  Device figures, worst over the six fixtures (the same
through all three routes): log marginal 1.5e-10, woodbury_vector 2.3e-7, dtheta 1.8e-9, noise gradient 1.8e-10, dZ 4.8e-8,
dmu 3.1e-9, dS 3.0e-9; the fixtures with a White part, whose Kmm is well conditioned, are met to 5e-13 or better.
"""
import numpy as np
import pytest

import psi_np as P
from gpy_amd import _lib

pytestmark = pytest.mark.gpu

LD = np.longdouble
TOL_PSI2, TOL_GRAD = 2.3e-14, 8.5e-14
CASES = [(1, 1, 1, True, False), (63, 63, 1, False, False), (65, 65, 2, True, False), (257, 130, 3, True, False),
         (65, 63, 33, True, False), (63, 65, 40, True, False), (2051, 8, 2, True, False), (65, 65, 3, True, True),
         (65, 65, 3, False, False), (63, 65, 40, False, False)]      # iso with D > 1: the summed lengthscale record, two groups
_ref = {}


def _case(c):
    """inputs and long-double reference of a case, computed once"""
    if c not in _ref:
        N, M, Q, ARD, w = c
        p = P.problem(N, M, Q, 100 + N + M + Q, ARD, w)
        st = P.psi_stats(p["var"], p["ls"], p["Z"], p["mu"], p["S"], p["weights"], dtype=LD)
        g = P.psi_grads(p["var"], p["ls"], ARD, p["Z"], p["mu"], p["S"], p["dL_dpsi0"], p["dL_dpsi1"], p["dL_dpsi2"], p["weights"],
                        dtype=LD)
        for a in st + tuple(g[1:]):
            a.setflags(write=False)
        _ref[c] = (p, st, g)
    return _ref[c]


def _rel(x, ref):
    return float(np.abs(np.asarray(x, dtype=LD) - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("c", CASES, ids=lambda c: "N%d_M%d_Q%d%s%s" % (c[0], c[1], c[2], "" if c[3] else "_iso", "_w" if c[4] else ""))
def test_psi1_and_psi2_match_the_long_double_restatement(c):
    p, st, _ = _case(c)
    psi1, psi2 = _lib.rbf_psi(p["var"], p["ls"], p["ARD"], p["Z"], p["mu"], p["S"], weights=p["weights"])
    e1, e2 = float(np.abs(psi1.astype(LD) - st[1]).max()), _rel(psi2, st[2])
    print("psi1 abs err %.2e (bound %.2e)  psi2 rel err %.2e (bound %.2e)" % (e1, 1e-13 * p["var"], e2, TOL_PSI2))
    assert e1 <= 1e-13 * p["var"]
    assert e2 <= TOL_PSI2
    assert np.array_equal(psi2, psi2.T)


@pytest.mark.parametrize("c", CASES, ids=lambda c: "N%d_M%d_Q%d%s%s" % (c[0], c[1], c[2], "" if c[3] else "_iso", "_w" if c[4] else ""))
def test_the_five_gradients_match_the_long_double_restatement(c):
    p, _, g = _case(c)
    got = _lib.rbf_psi_grad(p["var"], p["ls"], p["ARD"], p["Z"], p["mu"], p["S"], p["dL_dpsi0"], p["dL_dpsi1"], p["dL_dpsi2"],
                            weights=p["weights"])
    errs = {}
    for name, x, y in zip(("dvariance", "dlengthscale", "dZ", "dmu", "dS"), got, g):
        errs[name] = _rel(np.atleast_1d(x), np.atleast_1d(np.asarray(y)))
    print({k: "%.2e" % v for k, v in errs.items()}, "bound %.2e" % TOL_GRAD)
    for name, e in errs.items():
        assert e <= TOL_GRAD, (name, e)


def test_each_statistic_alone_gives_its_own_gradient():
    p, _, _ = _case((65, 65, 2, True, False))
    a = (p["var"], p["ls"], True, p["Z"], p["mu"], p["S"])
    for kw in (dict(dL_dpsi0=p["dL_dpsi0"]), dict(dL_dpsi1=p["dL_dpsi1"]), dict(dL_dpsi2=p["dL_dpsi2"])):
        ref = P.psi_grads(*a, dtype=LD, **kw)
        got = _lib.rbf_psi_grad(*a, **kw)
        for x, y in zip(got, ref):
            y = np.atleast_1d(np.asarray(y))
            if np.abs(y).max() == 0:
                assert not np.any(x)
            else:
                assert _rel(np.atleast_1d(x), y) <= TOL_GRAD


def test_two_evaluations_give_identical_bits():
    p, _, _ = _case((2051, 8, 2, True, False))
    a = (p["var"], p["ls"], True, p["Z"], p["mu"], p["S"])
    r1, r2 = _lib.rbf_psi(*a), _lib.rbf_psi(*a)
    assert all(np.array_equal(x, y) for x, y in zip(r1, r2))
    g1, g2 = (_lib.rbf_psi_grad(*a, p["dL_dpsi0"], p["dL_dpsi1"], p["dL_dpsi2"]) for _ in range(2))
    assert all(np.array_equal(np.atleast_1d(x), np.atleast_1d(y)) for x, y in zip(g1, g2))


def test_refusals_are_errors_that_name_what_was_refused():
    p, _, _ = _case((65, 65, 2, True, False))
    S = p["S"].copy()
    S[3, 1] = 0.0
    with pytest.raises(_lib.MI355GPError, match=r"S\[3\]\[1\]"):
        _lib.rbf_psi(p["var"], p["ls"], True, p["Z"], p["mu"], S)
    S[3, 1] = np.inf
    with pytest.raises(_lib.MI355GPError, match="positive and finite"):
        _lib.rbf_psi_grad(p["var"], p["ls"], True, p["Z"], p["mu"], S, dL_dpsi0=p["dL_dpsi0"])
    with pytest.raises(_lib.MI355GPError, match="lengthscale"):
        _lib.rbf_psi(p["var"], -p["ls"], True, p["Z"], p["mu"], p["S"])
    with pytest.raises(_lib.MI355GPError, match="at most 64"):
        _lib.rbf_psi(1.0, np.ones(1), False, np.zeros((2, 65)), np.zeros((3, 65)), np.ones((3, 65)))


def test_kernel_classes_honour_active_dims_inv_l_and_white_parts():
    import gpy_amd
    r = np.random.default_rng(5)
    N, M, D = 40, 7, 4
    q = gpy_amd.NormalPosterior(r.uniform(-3, 3, (N, D)), r.uniform(0.05, 1.0, (N, D)))
    Z = r.uniform(-3, 3, (M, D))
    dims = [3, 1]
    ls = np.array([0.9, 1.6])
    k = gpy_amd.RBF(2, variance=1.3, lengthscale=ls, ARD=True, active_dims=dims, inv_l=True)
    d0, d1, d2 = r.standard_normal(N), r.standard_normal((N, M)), r.standard_normal((M, M))
    a = (1.3, ls, Z[:, dims], q.mean[:, dims], q.variance[:, dims])
    st = P.psi_stats(*a, dtype=LD)
    g = P.psi_grads(1.3, ls, True, *a[2:], d0, d1, d2, dtype=LD)
    assert np.array_equal(k.psi0(Z, q), np.full(N, 1.3))
    assert np.abs(k.psi1(Z, q) - st[1]).max() <= 1e-13 * 1.3
    assert _rel(k.psi2(Z, q), st[2]) <= TOL_PSI2
    assert _rel(k.psi2n(Z, q[:3]).sum(0), P.psi_stats(1.3, ls, a[2], a[3][:3], a[4][:3], dtype=LD)[2]) <= TOL_PSI2
    k.update_gradients_expectations(d0, d1, d2, Z, q)
    assert abs(float(np.ravel(k.variance.gradient)[0]) - g[0]) <= TOL_GRAD * abs(g[0])
    assert _rel(k.lengthscale.gradient, g[1]) <= TOL_GRAD
    assert _rel(k.inv_l.gradient, g[1] * (np.asarray(ls, LD) ** 3 / -2)) <= TOL_GRAD
    dZ = k.gradients_Z_expectations(d0, d1, d2, Z, q)
    dmu, dS = k.gradients_qX_expectations(d0, d1, d2, Z, q)
    assert dZ.shape == Z.shape and not dZ[:, [0, 2]].any() and _rel(dZ[:, dims], g[2]) <= TOL_GRAD
    assert not dmu[:, [0, 2]].any() and _rel(dmu[:, dims], g[3]) <= TOL_GRAD and _rel(dS[:, dims], g[4]) <= TOL_GRAD
    s = k + gpy_amd.White(4, variance=0.2)
    assert np.array_equal(s.psi0(Z, q), np.full(N, 1.5)) and np.array_equal(s.psi2(Z, q), k.psi2(Z, q))
    s.update_gradients_expectations(d0, d1, d2, Z, q)
    assert abs(float(np.ravel(s.parts[1].variance.gradient)[0]) - d0.sum()) <= 1e-12 * np.abs(d0).sum()


# ---- the uncertain-input fit: the reference's fixtures (tests/golden/psi, tools/make_golden_psi.py) through the C-ABI entry
# point, VarDTC.inference and SparseGPRegression, at the tolerances of tests/test_gpu_sparse.py -------------------------------
import glob  # noqa: E402
import os  # noqa: E402

TOL_LML, TOL_FIT, TOL_VAR = 1e-9, 1e-6, 1e-5
FIXTURES = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "psi", "*.npz")))
FIX_IDS = [os.path.basename(f)[:-4] for f in FIXTURES]


def _fixture_kernel(g):
    import gpy_amd
    D, dims = g["mu"].shape[1], [int(d) for d in g["dims"]]
    sub = None if dims == list(range(D)) else dims
    k = gpy_amd.RBF(len(dims), variance=float(g["variance"]), lengthscale=g["ls"], ARD=bool(g["ARD"]), active_dims=sub)
    for w in g["white"]:
        k = k + gpy_amd.White(len(dims), variance=float(w), active_dims=sub)
    return k, dims


def _check_fit(tag, g, dims, lml, wv, dtheta, dnoise, dZ, dmu, dS):
    figs = {"lml": abs(lml - g["lml"]) / abs(g["lml"])}
    for name, x, y in (("woodbury_vector", wv, g["woodbury_vector"]), ("dtheta", dtheta, g["dtheta"]),
                       ("dnoise", np.atleast_1d(dnoise), g["dnoise"]), ("dZ", dZ, g["dZ"]), ("dmu", dmu, g["dmu"]), ("dS", dS, g["dS"])):
        figs[name] = _rel(x, np.asarray(y, dtype=LD))
    print(tag, {k: "%.2e" % v for k, v in figs.items()})
    assert figs.pop("lml") <= TOL_LML
    for name, e in figs.items():
        assert e <= TOL_FIT, (name, e)


@pytest.mark.parametrize("path", FIXTURES, ids=FIX_IDS)
def test_fixture_through_the_c_abi_fit_and_device_prediction(path):
    g = np.load(path)
    k, dims = _fixture_kernel(g)
    specs = k.part_specs()
    lone = len(specs) == 1                                  # a kernel on its own is given its active columns
    cols = dims if lone else slice(None)
    ctx = _lib.SparseContext(0)
    ctx.set_data(g["mu"][:, cols], g["Y"])
    ctx.set_input_variance(g["S"][:, cols])
    rc, r = ctx.vardtc_uncertain(specs, g["Z"][:, cols], float(g["noise"]))
    assert rc == 0
    pick = slice(None) if lone else dims
    if not lone:                                            # columns no part sees get no gradient
        rest = [d for d in range(g["mu"].shape[1]) if d not in dims]
        assert not r["dZ"][:, rest].any() and not r["dmu"][:, rest].any() and not r["dS"][:, rest].any()
    _check_fit("c-abi", g, dims, r["lml"], r["woodbury_vector"], r["dtheta"], r["dnoise"], r["dZ"][:, pick], r["dmu"][:, pick],
               r["dS"][:, pick])
    mu, var = ctx.predict(specs, g["Xs"][:, cols])
    assert _rel(mu, g["pred_mu"].astype(LD)) <= TOL_FIT and _rel(var, g["pred_var"].astype(LD)) <= TOL_VAR
    assert _rel(ctx.fetch(ctx.FETCH_DLDKMM), g["dL_dKmm"].astype(LD)) <= 1e-4         # (as tests/test_gpu_sparse.py)
    psi2 = P.psi_stats(float(g["variance"]), g["ls"], g["Z"][:, dims], g["mu"][:, dims], g["S"][:, dims], dtype=LD)[2]
    assert _rel(ctx.fetch(ctx.FETCH_PSI2), psi2) <= TOL_PSI2
    with pytest.raises(_lib.MI355GPError, match="uncertain inputs"):
        ctx.fetch_dL_dKnm(0, 1)


@pytest.mark.parametrize("path", FIXTURES, ids=FIX_IDS)
def test_fixture_through_vardtc_inference_and_sparse_gp_regression(path):
    import gpy_amd
    from gpy_amd.likelihoods import Gaussian
    from gpy_amd.sparse import VarDTC
    g = np.load(path)
    k, dims = _fixture_kernel(g)
    q = gpy_amd.NormalPosterior(g["mu"], g["S"])
    post, lml, gd = VarDTC().inference(k, q, g["Z"], Gaussian(variance=float(g["noise"])), g["Y"])
    f = gd["fused"]
    lone = f["dZ"].shape[1] == len(dims)
    pick = slice(None) if lone else dims
    _check_fit("VarDTC", g, dims, lml, post.woodbury_vector, f["dtheta"], gd["dL_dthetaL"], f["dZ"][:, pick], f["dmu"][:, pick],
               f["dS"][:, pick])
    assert _rel(gd["dL_dpsi0"], g["dL_dpsi0"].astype(LD)) <= TOL_FIT and _rel(np.asarray(gd["dL_dpsi1"]), g["dL_dpsi1"].astype(LD)) <= TOL_FIT
    assert _rel(np.asarray(gd["dL_dpsi2"]), g["dL_dpsi2"].astype(LD)) <= 1e-4 and _rel(np.asarray(gd["dL_dKmm"]), g["dL_dKmm"].astype(LD)) <= 1e-4
    k2, _ = _fixture_kernel(g)
    m = gpy_amd.SparseGPRegression(g["mu"], g["Y"], kernel=k2, Z=g["Z"], noise_var=float(g["noise"]), X_variance=g["S"])
    assert m.has_uncertain_inputs()
    M, D = g["Z"].shape
    grad = m.gradient                                       # [Z, kernel, noise]
    dZ = grad[:M * D].reshape(M, D)
    _check_fit("model", g, dims, m.log_likelihood(), m.posterior.woodbury_vector, grad[M * D:-1], grad[-1:], dZ[:, dims],
               m.grad_dict["fused"]["dmu"][:, pick], m.grad_dict["fused"]["dS"][:, pick])
    mu, var = m.predict(g["Xs"], include_likelihood=False)
    assert _rel(mu, g["pred_mu"].astype(LD)) <= TOL_FIT and _rel(var, g["pred_var"].astype(LD)) <= TOL_VAR


@pytest.mark.parametrize("D", [2, 1])
def test_checkgrad_of_sparse_gp_regression_with_rbf_plus_white_and_X_variance(D):
    """the reference's two tests of this configuration (testing/test_model.py: `SparseGPRegression` with `RBF + White`
    and `X_variance`, 2-D and 1-D): `m.checkgrad()` after randomising every parameter the way `m.randomize()` does there
    (standard normal draws, positive parameters through the softplus)"""
    import gpy_amd
    np.random.seed(3 + D)
    N = 50
    X = np.random.uniform(-3.0, 3.0, (N, D))
    Y = np.sin(X).sum(1, keepdims=True) + np.random.randn(N, 1) * 0.05
    m = gpy_amd.SparseGPRegression(X, Y, kernel=gpy_amd.RBF(D) + gpy_amd.White(D), X_variance=np.random.rand(N, D) + 1e-3, seed=1)
    pos = np.concatenate([np.full(p.size, bool(p.positive)) for p in m.flattened_parameters()])
    draw = np.random.randn(pos.size)
    m.param_array = np.where(pos, np.log1p(np.exp(draw)), draw)
    assert m.checkgrad(verbose=True)


def test_two_fits_in_fresh_contexts_give_identical_bits_across_a_chunk_boundary():
    """N = 2051 is just above the path's 2048-row chunk, M = 8: the chunk boundary and the fixed-order combine across chunks
    inside the fit, against the long-double restatement and twice for the bits"""
    p = P.fit_problem(2051, 8, 2, 2, 9, True, [0.3])
    ref = P.vardtc_uncertain(p["var"], p["ls"], True, p["white"], p["Z"], p["mu"], p["S"], p["Y"], p["noise"], dtype=LD)
    specs = [("rbf", True, np.concatenate([[p["var"]], p["ls"]]), None, 0), ("white", False, np.array([0.3]), None, 0)]
    out = []
    for _ in range(2):
        ctx = _lib.SparseContext(0)
        ctx.set_data(p["mu"], p["Y"])
        ctx.set_input_variance(p["S"])
        rc, r = ctx.vardtc_uncertain(specs, p["Z"], p["noise"])
        assert rc == 0
        out.append(r)
    a, b = out
    assert a["lml"] == b["lml"] and np.array_equal(a["dtheta"], b["dtheta"]) and np.array_equal(a["dZ"], b["dZ"])
    assert np.array_equal(a["dmu"], b["dmu"]) and np.array_equal(a["dS"], b["dS"])
    assert abs(a["lml"] - ref["lml"]) <= TOL_LML * abs(ref["lml"])
    dth = np.concatenate([[ref["dvar"]], ref["dl"], ref["dwhite"]]).astype(LD)
    for name, x, y in (("dtheta", a["dtheta"], dth), ("dZ", a["dZ"], ref["dZ"]), ("dmu", a["dmu"], ref["dmu"]), ("dS", a["dS"], ref["dS"]),
                       ("woodbury_vector", a["woodbury_vector"], ref["woodbury_vector"])):
        assert _rel(x, np.asarray(y)) <= TOL_FIT, name


def test_the_fit_refuses_by_name_through_the_c_abi():
    p = P.fit_problem(30, 5, 2, 1, 2, True, [])
    rbf = ("rbf", True, np.concatenate([[p["var"]], p["ls"]]), None, 0)
    ctx = _lib.SparseContext(0)
    ctx.set_data(p["mu"], p["Y"])
    with pytest.raises(_lib.MI355GPError, match="no input variances"):
        ctx.vardtc_uncertain([rbf], p["Z"], p["noise"])
    S = p["S"].copy()
    S[4, 1] = -0.1
    with pytest.raises(_lib.MI355GPError, match=r"S\[4\]\[1\]"):
        ctx.set_input_variance(S)
    with pytest.raises(_lib.MI355GPError, match="N x D"):
        ctx.set_input_variance(p["S"][:-1])
    ctx.set_input_variance(p["S"])
    with pytest.raises(_lib.MI355GPError, match="Bias"):
        ctx.vardtc_uncertain([rbf, ("bias", False, np.array([0.5]), None, 0)], p["Z"], p["noise"])
    with pytest.raises(_lib.MI355GPError, match="Matern52"):
        ctx.vardtc_uncertain([("matern52", False, np.array([1.0, 1.0]), None, 0)], p["Z"], p["noise"])
    with pytest.raises(_lib.MI355GPError, match="both RBF"):
        ctx.vardtc_uncertain([rbf, rbf], p["Z"], p["noise"])
    with pytest.raises(_lib.MI355GPError, match="product"):
        ctx.vardtc_uncertain([rbf[:4] + (1,), rbf[:4] + (1,)], p["Z"], p["noise"])
    with pytest.raises(_lib.MI355GPError, match="no RBF part"):
        ctx.vardtc_uncertain([("white", False, np.array([0.5]), None, 0)], p["Z"], p["noise"])
    with pytest.raises(_lib.MI355GPError, match="per-point noise"):
        ctx.vardtc_uncertain([rbf], p["Z"], np.full(30, 0.1))
    rc, r = ctx.vardtc_uncertain([rbf], p["Z"], p["noise"])          # the context is still good
    assert rc == 0 and np.isfinite(r["lml"])
    ctx.set_data(p["mu"], p["Y"])                                    # new data discard the variances
    with pytest.raises(_lib.MI355GPError, match="no input variances"):
        ctx.vardtc_uncertain([rbf], p["Z"], p["noise"])
