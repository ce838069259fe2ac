"""CPU: the NumPy restatement of the RBF psi-statistics (tests/psi_np.py) and the host classes around the device kernels.

The restatement is what tests/test_gpu_psi.py judges the device against, so it is checked here against central differences
of sum dL_dpsi0 psi0 + sum dL_dpsi1 * psi1 + sum dL_dpsi2 * psi2 in every parameter, Z, mu and S (in long double, where a
step of 1e-6 leaves a truncation error near 1e-11 and no visible rounding error).

tests/golden/psi/*.npz (tools/make_golden_psi.py) hold the reference's own values: `RBF.psi0/1/2`, the five outputs of
`psiDerivativecomputations`, and one whole `VarDTC.inference` with a `NormalPosterior` X plus the gradients
`SparseGP._update_gradients` derives from it, for iso / ARD, Q = 1, 2, 3, active_dims a strict subset, Dy = 1 and 3 and
RBF + White.  The restatement (statistics, chain rule and the whole uncertain-input evaluation) is compared with all of them.

Measured here, relative to max |value|, worst over the cases (|mu|, |z| <= 3, S in [0.05, 1]):
  float64 restatement against long-double restatement (the shapes of tests/test_gpu_psi.py):
    psi1 5.6e-16   psi2 2.3e-15   dvariance 3.1e-15   dlengthscale 1.3e-15   dZ 1.3e-15   dmu 8.4e-15   dS 5.6e-15
  long-double restatement against the reference's fixture values (float64, six fixtures):
    psi1 1.8e-16   psi2 5.9e-16   dvariance 1.3e-15   dlengthscale 1.2e-15   dZ 1.3e-15   dmu 1.2e-15   dS 6.9e-15
The larger of the two, times ten for a different summation order on the device, bounds the GPU tests: 2.3e-14 for psi2 and
8.5e-14 for the gradients.
The whole evaluation goes through two M x M factorisations of matrices with condition numbers up to ~1e8 (Kmm + 1e-8 I
without a White part), so the reference's float64 values sit further from long double: log marginal 2.3e-10, woodbury_vector
2.4e-7, dtheta 1.9e-9, noise gradient 2.8e-10, dZ 5.4e-8, dmu 3.2e-9, dS 3.1e-9 -- inside the tolerances the project holds
the sparse path to (tests/test_gpu_sparse.py: 1e-9, 1e-6, 1e-6), which are what the fit is held to here and on the device.
"""
import numpy as np
import pytest

import glob
import os

import psi_np as P

LD = np.longdouble
F64_PSI2, F64_GRAD = 2.3e-15, 8.5e-15          # the measured figures above, rounded up in the last digit
REF_PSI1, REF_PSI2, REF_GRAD = 1.9e-16, 5.9e-16, 6.9e-15      # restatement against the reference's fixtures, likewise
TOL_LML, TOL_FIT = 1e-9, 1e-6                  # the sparse path's tolerances (tests/test_gpu_sparse.py)
FIXTURES = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "psi", "*.npz")))


def fixture_args(g):
    """(variance, lengthscale, Z, mu, S) on the kernel's active columns"""
    d = g["dims"]
    return float(g["variance"]), g["ls"], g["Z"][:, d], g["mu"][:, d], g["S"][:, d]


def _rel(x, ref):
    return float(np.abs(np.asarray(x, dtype=LD) - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("N,M,Q,ARD,w", [(5, 4, 1, False, False), (6, 5, 2, True, False), (4, 6, 3, True, True),
                                         (3, 3, 3, False, True)])
def test_restatement_gradients_match_central_differences(N, M, Q, ARD, w):
    p = P.problem(N, M, Q, 7 + N + M + Q, ARD, w)
    g = P.psi_grads(p["var"], p["ls"], ARD, p["Z"], p["mu"], p["S"], p["dL_dpsi0"], p["dL_dpsi1"], p["dL_dpsi2"], p["weights"],
                    dtype=LD)
    # the objective uses dL_dpsi2 as given; the gradients symmetrise nothing either: psi2 is symmetric, so both agree
    base = dict(var=LD(p["var"]), ls=np.asarray(p["ls"], LD), Z=np.asarray(p["Z"], LD), mu=np.asarray(p["mu"], LD),
                S=np.asarray(p["S"], LD))

    def f(**kw):
        a = dict(base, **kw)
        return P.objective(a["var"], a["ls"], a["Z"], a["mu"], a["S"], p["dL_dpsi0"], p["dL_dpsi1"], p["dL_dpsi2"], p["weights"], LD)
    h = LD(1e-6)

    def fd(name, idx):
        up, dn = np.array(base[name], LD, ndmin=1).copy(), np.array(base[name], LD, ndmin=1).copy()
        up[idx] += h
        dn[idx] -= h
        if name == "var":
            up, dn = up[0], dn[0]
        return (f(**{name: up}) - f(**{name: dn})) / (2 * h)
    scale = max(float(np.abs(x).max()) for x in g[1:]) + abs(float(g[0]))
    assert abs(fd("var", 0) - g[0]) <= 1e-9 * scale
    if ARD:
        for q in range(Q):
            assert abs(fd("ls", q) - g[1][q]) <= 1e-9 * scale
    else:
        assert abs(fd("ls", 0) - g[1][0]) <= 1e-9 * scale
    for name, got in (("Z", g[2]), ("mu", g[3]), ("S", g[4])):
        for idx in np.ndindex(got.shape):
            assert abs(fd(name, idx) - got[idx]) <= 1e-9 * scale, (name, idx)


def test_float64_restatement_is_within_its_measured_distance_of_long_double():
    p = P.problem(65, 65, 2, 232, True, False)
    a = (p["var"], p["ls"], p["Z"], p["mu"], p["S"])
    s64, sld = P.psi_stats(*a), P.psi_stats(*a, dtype=LD)
    assert _rel(s64[2], sld[2]) <= F64_PSI2
    g = [P.psi_grads(p["var"], p["ls"], True, p["Z"], p["mu"], p["S"], p["dL_dpsi0"], p["dL_dpsi1"], p["dL_dpsi2"], dtype=t)
         for t in (np.float64, LD)]
    for x, y in zip(*g):
        assert _rel(x, np.asarray(y)) <= F64_GRAD


def test_psi2_is_the_weighted_sum_of_psi2n_and_psi_statistics_reduce_to_K_for_vanishing_S():
    p = P.problem(6, 5, 2, 3, True, True)
    _, psi1, psi2, psi2n = P.psi_stats(p["var"], p["ls"], p["Z"], p["mu"], p["S"], p["weights"], want_psi2n=True)
    assert np.allclose(psi2, np.einsum("n,nmo->mo", p["weights"], psi2n), rtol=1e-13)
    _, psi1, psi2 = P.psi_stats(p["var"], p["ls"], p["Z"], p["mu"], np.full_like(p["S"], 1e-14))
    r2 = (((p["mu"][:, None, :] - p["Z"][None, :, :]) / p["ls"]) ** 2).sum(-1)
    K = p["var"] * np.exp(-0.5 * r2)
    assert np.allclose(psi1, K, rtol=1e-10) and np.allclose(psi2, K.T @ K, rtol=1e-10)


def test_normal_posterior_holds_means_and_variances():
    import gpy_amd
    from gpy_amd.variational import NormalPosterior
    assert gpy_amd.NormalPosterior is NormalPosterior
    assert gpy_amd.core.parameterization.variational.NormalPosterior is NormalPosterior
    m, v = np.arange(12.0).reshape(4, 3), np.full((4, 3), 0.5)
    q = NormalPosterior(m, v)
    assert q.shape == (4, 3) and q.ndim == 2 and len(q) == 4 and q.has_uncertain_inputs()
    m[0, 0] = 99.0                                                     # a private copy
    assert q.mean[0, 0] == 0.0
    s = q[:, [0, 2]]
    assert isinstance(s, NormalPosterior) and s.shape == (4, 2) and np.array_equal(s.mean, q.mean[:, [0, 2]])
    assert np.array_equal(q[1:3].variance, v[1:3])
    c = q.copy()
    c.mean[:] = 0.0
    assert q.mean[1, 1] == 4.0
    with pytest.raises(ValueError):
        NormalPosterior(m, np.zeros((4, 3)))
    with pytest.raises(ValueError):
        NormalPosterior(m, v[:, :2])
    with pytest.raises(IndexError):
        q[0]


def test_sums_refuse_psi_statistics_of_anything_but_one_rbf_and_white_parts():
    """refused on the host, by name, before any device work"""
    import gpy_amd
    q = gpy_amd.NormalPosterior(np.zeros((3, 2)), np.ones((3, 2)))
    Z = np.zeros((2, 2))
    with pytest.raises(NotImplementedError, match="bias.*Bias"):
        (gpy_amd.RBF(2) + gpy_amd.Bias(2)).psi1(Z, q)
    with pytest.raises(NotImplementedError, match="second RBF"):
        (gpy_amd.RBF(2) + gpy_amd.RBF(2, name="other")).psi2(Z, q)
    with pytest.raises(NotImplementedError, match="Mat52"):
        (gpy_amd.Matern52(2) + gpy_amd.White(2)).update_gradients_expectations(None, None, None, Z, q)
    k = gpy_amd.RBF(2, variance=1.5) + gpy_amd.White(2, variance=0.25)
    assert np.array_equal(k.psi0(Z, q), np.full(3, 1.75))              # psi0 needs no device
    w = gpy_amd.White(2, variance=0.25)
    assert not w.psi1(Z, q).any() and w.psi1(Z, q).shape == (3, 2) and w.psi2(Z, q).shape == (2, 2)
    w.update_gradients_expectations(np.full(3, -2.0), None, None, Z, q)
    assert float(np.ravel(w.variance.gradient)[0]) == -6.0
    with pytest.raises(NotImplementedError, match="per data point"):
        gpy_amd.RBF(2).gradients_Z_expectations(None, None, np.zeros((3, 2, 2)), Z, q)


def test_the_fixture_set_covers_the_cases_it_was_asked_for():
    seen = [np.load(f) for f in FIXTURES]
    assert len(seen) >= 6
    assert {bool(g["ARD"]) for g in seen} == {True, False} and {len(g["dims"]) for g in seen} == {1, 2, 3}
    assert {g["Y"].shape[1] for g in seen} == {1, 3} and any(len(g["white"]) for g in seen)
    assert any(len(g["dims"]) < g["mu"].shape[1] for g in seen)
    assert all(np.abs(g["mu"]).max() <= 3 and 0.05 <= g["S"].min() and g["S"].max() <= 1 for g in seen)


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(f)[:-4] for f in FIXTURES])
def test_restatement_matches_the_references_statistics_and_chain_rule(path):
    g = np.load(path)
    a = fixture_args(g)
    st = P.psi_stats(*a, dtype=LD)
    assert np.array_equal(g["psi0"], np.asarray(st[0], dtype=np.float64))
    assert _rel(g["psi1"], st[1]) <= REF_PSI1 and _rel(g["psi2"], st[2]) <= REF_PSI2
    # the reference symmetrises dL_dpsi2 (rbf_psi_comp.py:109); psi2 is symmetric, so the restatement needs no such step
    gr = P.psi_grads(a[0], a[1], bool(g["ARD"]), *a[2:], g["k_d0"], g["k_d1"], g["k_d2"], dtype=LD)
    ref = (g["k_dtheta"][:1], g["k_dtheta"][1:], g["k_dZ"], g["k_dmu"], g["k_dS"])
    for name, x, y in zip(("dvariance", "dlengthscale", "dZ", "dmu", "dS"), ref, gr):
        assert _rel(x, np.atleast_1d(np.asarray(y))) <= REF_GRAD, name


def _fit(g, dtype=LD, **kw):
    a = fixture_args(g)
    return P.vardtc_uncertain(a[0], a[1], bool(g["ARD"]), list(g["white"]), *a[2:], g["Y"], float(g["noise"]), dtype=dtype, **kw)


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(f)[:-4] for f in FIXTURES])
def test_restated_uncertain_input_vardtc_matches_the_references_evaluation(path):
    g = np.load(path)
    v = _fit(g)
    assert abs(g["lml"] - v["lml"]) <= TOL_LML * abs(v["lml"])
    dtheta = np.concatenate([[v["dvar"]], v["dl"], v["dwhite"]]).astype(LD)
    for name, x, y in (("woodbury_vector", g["woodbury_vector"], v["woodbury_vector"]), ("dtheta", g["dtheta"], dtheta),
                       ("dnoise", g["dnoise"], np.atleast_1d(v["dnoise"])), ("dZ", g["dZ"], v["dZ"]), ("dmu", g["dmu"], v["dmu"]),
                       ("dS", g["dS"], v["dS"]), ("dL_dKmm", g["dL_dKmm"], v["dL_dKmm"]), ("dL_dpsi0", g["dL_dpsi0"], v["dL_dpsi0"]),
                       ("dL_dpsi1", g["dL_dpsi1"], v["dL_dpsi1"]), ("dL_dpsi2", g["dL_dpsi2"], v["dL_dpsi2"])):
        assert _rel(x, np.asarray(y)) <= TOL_FIT, name


@pytest.mark.parametrize("N,M,Q,Dy,ARD,white", [(9, 4, 1, 1, False, [0.2]), (10, 5, 2, 2, True, [0.3]), (8, 4, 3, 1, True, [])])
def test_restated_vardtc_gradients_match_central_differences_of_the_log_marginal(N, M, Q, Dy, ARD, white):
    p = P.fit_problem(N, M, Q, Dy, 11 + Q, ARD, white)
    keys = ("var", "ls", "ARD", "white", "Z", "mu", "S", "Y", "noise")

    def run(want_grads=False, **kw):
        return P.vardtc_uncertain(*[dict(p, **kw)[k] for k in keys], dtype=LD, want_grads=want_grads)
    g = run(True)
    h = LD(1e-6)

    def fd(name, idx):
        up, dn = np.array(p[name], LD, ndmin=1).copy(), np.array(p[name], LD, ndmin=1).copy()
        up[idx] += h
        dn[idx] -= h
        if name in ("var", "noise"):
            up, dn = up[0], dn[0]
        elif name == "white":
            up, dn = list(up), list(dn)
        return (run(**{name: up})["lml"] - run(**{name: dn})["lml"]) / (2 * h)
    # a central difference with h = 1e-6 in long double: the truncation error (h^2 times a third derivative over six) and the
    # rounding error both stay far below 1e-6 of the gradients' scale
    scale = max(float(np.abs(np.asarray(g[k], LD)).max()) for k in ("dvar", "dl", "dZ", "dmu", "dS", "dnoise"))
    assert abs(fd("var", 0) - g["dvar"]) <= 1e-6 * scale and abs(fd("noise", 0) - g["dnoise"]) <= 1e-6 * scale
    for q in range(len(g["dl"])):
        assert abs(fd("ls", q if ARD else 0) - g["dl"][q]) <= 1e-6 * scale
    for i in range(len(white)):
        assert abs(fd("white", i) - g["dwhite"][i]) <= 1e-6 * scale
    for name, key in (("Z", "dZ"), ("mu", "dmu"), ("S", "dS")):
        for idx in np.ndindex(g[key].shape):
            assert abs(fd(name, idx) - g[key][idx]) <= 1e-6 * scale, (name, idx)


# ---- routing and refusals over a recording context: no device --------------------------------------------------------------
class RecSparse(object):
    FETCH_DLDKMM, FETCH_WOODBURY_INV, FETCH_LM, FETCH_KMM, FETCH_PSI2, FETCH_DLDPSI2_BETA = range(6)
    sharded = False

    def __init__(self, device=0):
        self.log = []

    def set_data(self, X, Y):
        self.log.append(("set_data", np.array(X), np.array(Y)))
        self.N, self.D, self.Dy = X.shape[0], X.shape[1], Y.shape[1]

    def set_input_variance(self, S):
        self.log.append(("set_input_variance", np.array(S)))

    def _res(self, specs, Z):
        nth = sum(np.size(s[2]) for s in specs)
        return 0, dict(lml=-1.0, dnoise=0.5, dtheta=np.arange(1.0, 1.0 + nth), dZ=np.full(Z.shape, 3.0),
                       woodbury_vector=np.ones((Z.shape[0], self.Dy)), dL_dm=None, dmu=np.full((self.N, self.D), 4.0),
                       dS=np.full((self.N, self.D), 5.0))

    def vardtc_sum(self, specs, Z, noise, **kw):
        self.log.append(("vardtc_sum", [s[0] for s in specs]))
        return self._res(specs, Z)

    def vardtc_uncertain(self, specs, Z, noise, **kw):
        self.log.append(("vardtc_uncertain", [s[0] for s in specs], np.array(Z), np.array(noise)))
        return self._res(specs, Z)

    def fetch(self, which):
        return np.full((2, 2), float(which))

    def predict(self, specs, Xnew, full_cov=False, want_var=True):
        self.log.append(("sparse_predict", np.array(Xnew)))
        return np.zeros((Xnew.shape[0], self.Dy)), np.ones((Xnew.shape[0], 1))


@pytest.fixture
def rec(monkeypatch):
    from gpy_amd import _lib
    made = []

    class Ctx(RecSparse):
        def __init__(self, device=0):
            RecSparse.__init__(self, device)
            made.append(self)
    monkeypatch.setattr(_lib, "SparseContext", Ctx)
    return made


def _xy(D=3, N=12, Dy=2):
    r = np.random.default_rng(4)
    return r.uniform(-2, 2, (N, D)), r.uniform(0.1, 0.5, (N, D)), r.standard_normal((N, Dy)), r.uniform(-2, 2, (2, D))


def test_sparse_gp_regression_takes_X_variance_and_routes_to_the_uncertain_entry_point(rec):
    """(`SparseGPRegression(X, Y, X_variance=...)` is a TypeError without the feature)"""
    import gpy_amd
    X, S, Y, Z = _xy()
    k = gpy_amd.RBF(2, ARD=True, active_dims=[2, 0]) + gpy_amd.White(2, variance=0.1, active_dims=[2, 0])
    m = gpy_amd.SparseGPRegression(X, Y, kernel=k, Z=Z, X_variance=S)
    assert m.has_uncertain_inputs() and isinstance(m.X, gpy_amd.NormalPosterior) and m.X.shape == X.shape
    assert [c[0] for c in rec[0].log] == ["set_data", "set_input_variance", "vardtc_uncertain"]
    assert np.array_equal(rec[0].log[0][1], X) and np.array_equal(rec[0].log[1][1], S)      # full width; the parts carry active_dims
    assert rec[0].log[2][1] == ["rbf", "white"] and rec[0].log[2][3].size == 1
    # X's variance is data: the flat parameters are [Z, kernel, noise] as for certain inputs
    assert m.param_array.size == Z.size + 3 + 1 + 1
    certain = gpy_amd.SparseGPRegression(X, Y, kernel=gpy_amd.RBF(3), Z=Z)
    assert not certain.has_uncertain_inputs() and [c[0] for c in rec[1].log] == ["set_data", "vardtc_sum"]
    assert np.array_equal(m.Z.gradient, np.full(Z.shape, 3.0)) and m.log_likelihood() == -1.0
    gd = m.grad_dict
    assert set(gd) == {"dL_dKmm", "dL_dpsi0", "dL_dpsi1", "dL_dpsi2", "dL_dthetaL", "fused"}
    beta = 1.0 / float(np.ravel(m.likelihood.variance.values)[0])
    assert np.allclose(gd["dL_dpsi0"], -0.5 * 2 * beta) and gd["dL_dpsi0"].shape == (12,)
    assert np.allclose(np.asarray(gd["dL_dpsi1"]), beta * Y @ np.ones((2, 2)).T) and gd["dL_dpsi1"].shape == (12, 2)
    assert np.allclose(np.asarray(gd["dL_dpsi2"]), beta * 5.0) and np.allclose(np.asarray(gd["dL_dKmm"]), 0.0)
    assert np.array_equal(gd["fused"]["dmu"], np.full(X.shape, 4.0)) and np.array_equal(gd["fused"]["dS"], np.full(X.shape, 5.0))
    m.parameters_changed()                                             # the same data: nothing is uploaded again
    assert [c[0] for c in rec[0].log][3:] == ["vardtc_uncertain"]
    mu, var = m.predict(X[:5])
    assert rec[0].log[-1][0] == "sparse_predict" and mu.shape == (5, 2)
    with pytest.raises(NotImplementedError, match="uncertain new points"):
        m.predict(gpy_amd.NormalPosterior(X[:5], S[:5]))


def test_uncertain_input_refusals_name_what_was_refused(rec):
    import gpy_amd
    from gpy_amd.likelihoods import Gaussian
    from gpy_amd.sparse import VarDTC
    X, S, Y, Z = _xy()
    q = gpy_amd.NormalPosterior(X, S)
    lik = Gaussian(variance=0.1)
    inf = VarDTC()
    with pytest.raises(NotImplementedError, match="bias.*Bias"):
        inf.inference(gpy_amd.RBF(3) + gpy_amd.Bias(3), q, Z, lik, Y)
    with pytest.raises(NotImplementedError, match="Mat52"):
        inf.inference(gpy_amd.Matern52(3), q, Z, lik, Y)
    with pytest.raises(NotImplementedError, match="exactly one RBF"):
        inf.inference(gpy_amd.RBF(3) + gpy_amd.RBF(3, name="other"), q, Z, lik, Y)
    with pytest.raises(NotImplementedError, match="Prod"):
        inf.inference(gpy_amd.RBF(3) * gpy_amd.RBF(3, name="other"), q, Z, lik, Y)
    with pytest.raises(NotImplementedError, match="per-point"):
        inf.inference(gpy_amd.RBF(3), q, Z, lik, Y, precision=np.full(12, 2.0))
    with pytest.raises(NotImplementedError, match="precomputed statistics"):
        inf.inference(gpy_amd.RBF(3), q, Z, lik, Y, psi1=np.zeros((12, 2)))

    class Mean(object):
        def f(self, X):
            return np.zeros((X.shape[0], 2))
    with pytest.raises(ValueError, match="Mean function not implemented with uncertain inputs"):
        inf.inference(gpy_amd.RBF(3), q, Z, lik, Y, mean_function=Mean())
    with pytest.raises(ValueError, match="Mean function"):
        gpy_amd.SparseGPRegression(X, Y, Z=Z, X_variance=S, mean_function=Mean())
    assert not any(c[0].startswith("vardtc") for ctx in rec for c in ctx.log)                 # nothing reached a context
    inf.inference(gpy_amd.RBF(3), q, Z, lik, Y)
    rec[-1].sharded = True
    with pytest.raises(NotImplementedError, match="row-sharded"):
        inf.inference(gpy_amd.RBF(3), q, Z, lik, Y)
