"""GPU (-m gpu): Coregionalize (C-ABI kind 8) through the fused exact-GP calls, the stateless kernel entry points and the
host classes (GPCoregionalizedRegression, MixedNoise), against fixtures from the reference's own code (tests/golden/coreg,
made by tools/make_golden_coreg.py) and against the NumPy restatement in coreg_np.py.  Tolerances as for the other kinds:
LML 1e-10 relative, alpha 1e-9, gradients 1e-8, K 1e-13, prediction 1e-9."""
import glob
import os

import numpy as np
import pytest

import gpy_amd
from gpy_amd import _lib as L
from gpy_amd.util import multioutput

import coreg_np as C

pytestmark = pytest.mark.gpu
TOL_LML, TOL_ALPHA, TOL_GRAD, TOL_K, TOL_PRED = 1e-10, 1e-9, 1e-8, 1e-13, 1e-9
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(HERE, "golden", "coreg", "*.npz")))
GAUSS = [n for n in NAMES if not n.startswith("studentt")]


def _load(name):
    z = np.load(os.path.join(HERE, "golden", "coreg", name + ".npz"))
    g = {k: z[k] for k in z.files}
    g["specs"] = C.load_specs(g["specs"])
    g["nu"] = None if float(g["nu"]) < 0 else float(g["nu"])
    rng = np.random.default_rng(1000 + int(g["gseed"]))
    g["G"] = rng.standard_normal((g["X"].shape[0],) * 2)
    g["G2"] = rng.standard_normal((g["X"].shape[0], g["Xs"].shape[0]))
    return g


def _close(a, b, tol):
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert np.abs(a - b).max() <= tol * max(np.abs(b).max(), 1e-300), (np.abs(a - b).max(), np.abs(b).max())


def cabi_specs(specs):
    """the C-ABI part list: a Coregionalize part carries (P, B)"""
    out = []
    for s in specs:
        if s[0] == "coregionalize":
            B = C.coreg_WkB(s)[2]
            out.append(("coregionalize", s[1] % 100, (0.5 * (B + B.T)).ravel(), s[3], s[4]))
        else:
            out.append(s)
    return out


def to_gpy(specs, dth):
    """device dtheta (S for Coregionalize parts) -> GPy order (W, kappa)"""
    out, i = [], 0
    for s in specs:
        if s[0] == "coregionalize":
            P = s[1] % 100
            dW, dk = C.chain_W_kappa(dth[i:i + P * P].reshape(P, P), C.coreg_WkB(s)[0])
            out += [dW.ravel(), dk]
            i += P * P
        else:
            out.append(dth[i:i + s[2].size])
            i += s[2].size
    return np.concatenate(out)


def leaf(spec):
    kind, ard, th, dims, _ = spec
    if kind == "coregionalize":
        W, kappa, _ = C.coreg_WkB(spec)
        return gpy_amd.Coregionalize(1, ard % 100, rank=ard // 100, W=W, kappa=kappa, active_dims=dims, name="B")
    if kind == "white":
        return gpy_amd.White(len(dims), th[0], active_dims=dims)
    cls = {"rbf": gpy_amd.RBF, "matern52": gpy_amd.Matern52}[kind]
    return cls(len(dims), th[0], th[1:], ARD=bool(ard), active_dims=dims)


def kernel(specs):
    summands = []
    for t in C.terms(specs):
        summands.append(leaf(specs[t[0]]) if len(t) == 1 else gpy_amd.Prod([leaf(specs[i]) for i in t]))
    return summands[0] if len(summands) == 1 else gpy_amd.Add(summands)


def _evaluate(g, specs=None, X=None, Y=None):
    specs = cabi_specs(g["specs"]) if specs is None else specs
    X = g["X"] if X is None else X
    Y = g["Y"] if Y is None else Y
    ctx = L.Context()
    ctx.set_data(X, Y)
    if g["nu"] is None:
        rc, r = ctx.exact_inference_sum(specs, C.noise_vector(g["noises"], X), jitter=1e-8, want_diag=True)
    else:
        rc, r = ctx.exact_studentt_sum(specs, g["nu"])
    assert rc == 0
    return ctx, r


@pytest.mark.parametrize("name", NAMES)
def test_golden_through_the_c_abi(name):
    g = _load(name)
    ctx, r = _evaluate(g)
    assert abs(r["lml"] - g["lml"]) <= TOL_LML * abs(g["lml"])
    _close(r["alpha"], g["alpha"], TOL_ALPHA)
    _close(to_gpy(g["specs"], r["dtheta"]), g["dtheta"], TOL_GRAD)
    _, _, dL_dK, Ki, _ = C.exact(g["specs"], g["X"], g["Y"], g["noises"], g["nu"])
    i = 0
    for s, gl in zip(g["specs"], C.leaf_grads(g["specs"], g["X"], dL_dK)):  # S itself against the restatement
        n = gl.size
        _close(r["dtheta"][i:i + n], gl.ravel(), TOL_GRAD)
        i += n
    if g["nu"] is None:
        dn = np.bincount(g["X"][:, -1].astype(int), weights=r["diag_dL_dK"], minlength=len(g["noises"]))
        _close(dn, g["dnoise"], TOL_GRAD)
        mu, var = ctx.predict_sum(cabi_specs(g["specs"]), g["Xs"], full_cov=False)
        _close(mu, g["pred_mu"], TOL_PRED)
        _close(var, g["pred_var"], TOL_PRED)
        mu, cov = ctx.predict_sum(cabi_specs(g["specs"]), g["Xs"], full_cov=True)
        _close(mu, g["pred_mu"], TOL_PRED)
        _close(cov, g["pred_cov"], TOL_PRED)
        cb = ctx.covariance_between_points(cabi_specs(g["specs"]), g["Xs"][:7], g["Xs"][4:])
        _close(cb, g["pred_cov"][:7, 4:], TOL_PRED)
        Kfull = ctx.fetch(L.FETCH_K)
        _close(Kfull[0], g["K_row0"], TOL_K)


@pytest.mark.parametrize("name", NAMES)
def test_stateless_kern_K_and_update_gradients_full(name):
    g = _load(name)
    spec = [s for s in g["specs"] if s[0] == "coregionalize"][0]
    W, kappa, B = C.coreg_WkB(spec)
    P = spec[1] % 100
    Bs = (0.5 * (B + B.T)).ravel()
    idx, idxs = g["X"][:, -1:], g["Xs"][:, -1:]
    K = L.kern_K("coregionalize", P, Bs, idx)
    _close(K, B[idx[:, 0].astype(int)][:, idx[:, 0].astype(int)], TOL_K)
    K2 = L.kern_K("coregionalize", P, Bs, idx, idxs)
    _close(K2, B[idx[:, 0].astype(int)][:, idxs[:, 0].astype(int)], TOL_K)
    S = L.update_gradients_full("coregionalize", P, Bs, g["G"], idx)
    _close(S, C.bucket_S(g["G"], idx[:, 0].astype(int), idx[:, 0].astype(int), P).ravel(), TOL_GRAD)
    dW, dk = C.chain_W_kappa(S.reshape(P, P), W)
    _close(np.concatenate([dW.ravel(), dk]), g["ug"], TOL_GRAD)
    S2 = L.update_gradients_full("coregionalize", P, Bs, g["G2"], idx, idxs)
    dW, dk = C.chain_W_kappa(S2.reshape(P, P), W)
    _close(np.concatenate([dW.ravel(), dk]), g["ug2"], TOL_GRAD)
    k = leaf(spec)                                               # the host class: the same numbers
    k.update_gradients_full(g["G2"], g["X"], g["Xs"])
    _close(np.concatenate([k.W.gradient.ravel(), k.kappa.gradient]), g["ug2"], TOL_GRAD)
    _close(k.K(g["X"])[0], B[int(idx[0, 0])][idx[:, 0].astype(int)], TOL_K)


def _split(g):
    idx = g["X"][:, -1].astype(int)
    P = len(g["noises"])
    return [g["X"][idx == j, :-1] for j in range(P)], [g["Y"][idx == j] for j in range(P)]


@pytest.mark.parametrize("name", [n for n in GAUSS if "shuffled" not in n])
def test_gp_coregionalized_regression(name):
    g = _load(name)
    Xl, Yl = _split(g)
    X, _, _ = multioutput.build_XY(Xl, Yl)
    assert np.array_equal(X, g["X"])                             # the fixture rows are in build_XY's order
    liks = [gpy_amd.Gaussian(variance=v, name="Gaussian_noise_%d" % j) for j, v in enumerate(g["noises"])]
    m = gpy_amd.GPCoregionalizedRegression(Xl, Yl, kernel=kernel(g["specs"]), likelihoods_list=liks)
    assert abs(m.log_likelihood() - g["lml"]) <= TOL_LML * abs(g["lml"])
    _close(m.gradient, np.concatenate([g["dtheta"], g["dnoise"]]), TOL_GRAD)
    meta = {"output_index": g["Xs"][:, -1:].astype(int)}
    s = g["noises"][g["Xs"][:, -1].astype(int)]
    mu, var = m.predict(g["Xs"], Y_metadata=meta)
    _close(mu, g["pred_mu"], TOL_PRED)
    _close(var, g["pred_var"] + s[:, None], TOL_PRED)
    mu, cov = m.predict(g["Xs"], full_cov=True, Y_metadata=meta)
    _close(cov, g["pred_cov"] + np.diag(s), TOL_PRED)
    from scipy import stats
    lo, hi = m.predict_quantiles(g["Xs"], Y_metadata=meta)
    _close(lo, stats.norm.ppf(0.025) * np.sqrt(g["pred_var"] + s[:, None]) + g["pred_mu"], TOL_PRED)
    _close(hi, stats.norm.ppf(0.975) * np.sqrt(g["pred_var"] + s[:, None]) + g["pred_mu"], TOL_PRED)
    np.random.seed(3)
    assert m.checkgrad()


def test_default_model_fits_and_predicts_per_output():
    rng = np.random.default_rng(5)
    X1, X2 = rng.random((50, 1)) * 8, rng.random((30, 1)) * 5
    Y1 = np.sin(X1) + rng.standard_normal(X1.shape) * 0.05
    Y2 = -np.sin(X2) + rng.standard_normal(X2.shape) * 0.05
    np.random.seed(0)
    # the reference's test_multioutput_regression_1D: a given kernel is used as it is (here an RBF on the input column)
    m = gpy_amd.GPCoregionalizedRegression(X_list=[X1, X2], Y_list=[Y1, Y2], kernel=gpy_amd.RBF(1))
    assert isinstance(m.kern, gpy_amd.RBF) and isinstance(m.likelihood, gpy_amd.MixedNoise)
    assert m.checkgrad()
    # the default kernel: an ICM of an RBF (gp_coregionalized_regression.py:36-39)
    liks = [gpy_amd.Gaussian(variance=0.01), gpy_amd.Gaussian(variance=0.01)]
    m = gpy_amd.GPCoregionalizedRegression(X_list=[X1, X2], Y_list=[Y1, Y2], likelihoods_list=liks)
    assert m.kern.name == "coreg" and isinstance(m.kern.parts[1], gpy_amd.Coregionalize)
    assert m.checkgrad()
    before = m.log_likelihood()
    m.optimize(max_iters=200)
    assert m.log_likelihood() > before
    Xt = np.linspace(0.5, 4.5, 9)[:, None]
    for j, f in enumerate((np.sin, lambda x: -np.sin(x))):
        Xn = np.hstack([Xt, np.full_like(Xt, j)])
        mu, var = m.predict(Xn, Y_metadata={"output_index": np.full((9, 1), j)})
        assert np.abs(mu - f(Xt)).max() < 0.1 and np.all(var > 0), (j, m.param_array)


def test_determinism_bit_identical():
    g = _load("icm_rbf_p5_shuffled_n160")
    specs = cabi_specs(g["specs"])
    ctx = L.Context()
    ctx.set_data(g["X"], g["Y"])
    nv = C.noise_vector(g["noises"], g["X"])
    r1 = ctx.exact_inference_sum(specs, nv, want_diag=True)[1]
    r2 = ctx.exact_inference_sum(specs, nv, want_diag=True)[1]
    assert r1["dtheta"].tobytes() == r2["dtheta"].tobytes()
    assert r1["alpha"].tobytes() == r2["alpha"].tobytes()
    S1 = L.update_gradients_full("coregionalize", 5, specs[1][2], g["G"], g["X"][:, -1:])
    S2 = L.update_gradients_full("coregionalize", 5, specs[1][2], g["G"], g["X"][:, -1:])
    assert S1.tobytes() == S2.tobytes()


def test_shuffled_against_sorted_rows():
    g = _load("icm_rbf_p5_shuffled_n160")
    order = np.argsort(g["X"][:, -1], kind="stable")
    _, r1 = _evaluate(g)
    _, r2 = _evaluate(g, X=g["X"][order], Y=g["Y"][order])
    assert abs(r1["lml"] - r2["lml"]) <= TOL_LML * abs(r1["lml"])
    _close(r2["dtheta"], r1["dtheta"], TOL_GRAD)


@pytest.mark.parametrize("N,shuffle", [(4096, False), (4224, True)])
def test_large_against_numpy(N, shuffle):
    """inside the persistent-launch range (4096) and with a ragged last tile (4224), P = 4, ICM Matern52 ARD D = 3"""
    rng = np.random.default_rng(N)
    P, D = 4, 3
    idx = np.sort(rng.integers(0, P, N))
    if shuffle:
        idx = rng.permutation(idx)
    Xin = rng.random((N, D)) * 3.0
    X = np.hstack([Xin, idx[:, None].astype(float)])
    Y = (np.sin(Xin @ np.array([1.0, 0.6, 0.3])) * (1.0 + 0.2 * idx) + 0.1 * rng.standard_normal(N))[:, None]
    specs = [("matern52", 1, np.array([1.1, 0.9, 1.3, 0.7]), np.arange(D), 1),
             ("coregionalize", 104, np.array([0.8, -0.4, 0.6, 0.3, 0.4, 0.5, 0.3, 0.6]), np.array([D]), 1)]
    noises = np.array([0.1, 0.05, 0.2, 0.1])
    g = {"noises": noises, "nu": None}
    _, r = _evaluate(g, specs=cabi_specs(specs), X=X, Y=Y)
    lml, alpha, dL_dK, Ki, dn = C.exact(specs, X, Y, noises)
    assert abs(r["lml"] - lml) <= TOL_LML * abs(lml)
    _close(r["alpha"], alpha, TOL_ALPHA)
    gl = C.leaf_grads(specs, X, dL_dK)
    _close(r["dtheta"], np.concatenate([gl[0], gl[1].ravel()]), TOL_GRAD)
    _close(np.bincount(idx, weights=r["diag_dL_dK"], minlength=P), dn, TOL_GRAD)


def _ctx(X, Y):
    ctx = L.Context()
    ctx.set_data(X, Y)
    return ctx


def test_error_paths_return_errors():
    g = _load("icm_rbfard_p3_r1_n135")
    specs = cabi_specs(g["specs"])
    nv = C.noise_vector(g["noises"], g["X"])
    X = g["X"].copy()
    X[7, -1] = 3.0                                              # out of range for P = 3
    with pytest.raises(L.MI355GPError, match="3"):
        _ctx(X, g["Y"]).exact_inference_sum(specs, nv)
    X[7, -1] = 1.5                                              # not an integer
    with pytest.raises(L.MI355GPError, match="1.5"):
        _ctx(X, g["Y"]).exact_inference_sum(specs, nv)
    ctx = _ctx(g["X"], g["Y"])
    bad = [specs[0], ("coregionalize", 17, np.eye(17).ravel(), specs[1][3], 1)]
    with pytest.raises(L.MI355GPError, match="17"):
        ctx.exact_inference_sum(bad, nv)
    bad = [specs[0], ("coregionalize", 3, specs[1][2], np.array([1, 2]), 1)]
    with pytest.raises(L.MI355GPError, match="n_active"):
        ctx.exact_inference_sum(bad, nv)
    with pytest.raises(L.MI355GPError, match="-1"):
        L.kern_K("coregionalize", 3, specs[1][2], np.array([[0.0], [-1.0]]))
    rc, r = ctx.exact_inference_sum(specs, nv)                 # the context still works
    assert rc == 0 and abs(r["lml"] - g["lml"]) <= TOL_LML * abs(g["lml"])
    Xs = g["Xs"].copy()
    Xs[0, -1] = 5.0
    with pytest.raises(L.MI355GPError, match="5"):
        ctx.predict_sum(specs, Xs)
    k = kernel(g["specs"])
    with pytest.raises(NotImplementedError, match="Coregionalize"):
        gpy_amd.SparseGPRegression(g["X"], g["Y"], kernel=k, Z=g["X"][:10])
