"""CPU: what the inference classes send to the device for a kernel, pinned with recording stand-ins for `_lib.Context` and
`_lib.SparseContext` (no GPU work): the X that is uploaded, the `mi355gp_part` list (kind, ard, theta bits, active_dims, term)
and the context method that is called, for a lone kernel, a lone White / Coregionalize, a sum and a sum with a product, through
`ExactGaussianInference`, `ExactStudentTInference`, `Laplace`, `EP` and `VarDTC`; and the jitter ladder they all climb.

The single-kernel C entries (`mi355gp_exact_inference`, `mi355gp_predict`) build the one part {kind, ard, 0, NULL, theta} and
call the `_sum` entry, so the stand-in logs a call of `Context.exact_inference` / `Context.predict` as that `_sum` call: the
expectations below say what reaches the device, whichever of the two Python methods carried it; `Rec.single` notes the calls of
the single-kernel methods, which the package itself no longer makes."""
import numpy as np
import pytest

import gpy_amd
from gpy_amd import _lib
from gpy_amd.inference import ExactGaussianInference, ExactStudentTInference
from gpy_amd.sparse import VarDTC

N = 12


def _spec(s):
    dims = None if s[3] is None else tuple(int(i) for i in s[3])
    return (s[0], _lib.ard_id(s[0], s[1]), np.asarray(s[2], dtype=np.float64).tobytes(), dims, int(s[4]) if len(s) > 4 else 0)


def part(kind, ard, theta, dims, term):
    return (kind, ard, np.array(theta, dtype=np.float64).tobytes(), dims, term)


class Rec(object):
    """Stands for `_lib.Context` and `_lib.SparseContext`: logs (method, parts) and the arrays, answers with zeros of the right
    shapes.  `fail`: every factorisation reports info = 7, and the jitter it was given is logged."""
    FETCH_DLDKMM, FETCH_WOODBURY_INV, FETCH_LM, FETCH_KMM, FETCH_PSI2 = 0, 1, 2, 3, 4
    fail = False

    def __init__(self, device=0):
        self.log, self.X, self.arrays, self.jitters, self.single = [], None, {}, [], []

    def _info(self, extra):
        self.jitters.append(float(extra))
        return 7 if self.fail else 0

    def _ntheta(self, specs):
        return sum(np.asarray(s[2]).size for s in specs)

    def set_data(self, X, R):
        self.X, self.Dy = np.array(X), R.shape[1]

    def set_targets(self, R):
        pass

    def exact_inference(self, kind, ARD, theta, noise, **kw):
        self.single.append("exact_inference")
        return self.exact_inference_sum([(kind, ARD, theta, None, 0)], noise, **kw)

    def exact_inference_sum(self, specs, noise, jitter=1e-8, extra_jitter=0.0, **kw):
        self.log.append(("exact_inference_sum", [_spec(s) for s in specs]))
        n = self.X.shape[0]
        return self._info(extra_jitter), dict(lml=-1.0, dnoise=0.5, alpha=np.zeros((n, self.Dy)), diag_dL_dK=np.zeros(n),
                                              dtheta=np.arange(1.0, 1.0 + self._ntheta(specs)))

    def inference_given_K(self, K, noise, jitter=1e-8, extra_jitter=0.0, **kw):
        self.log.append(("inference_given_K", None))
        self.arrays["K"] = np.array(K)
        n = self.X.shape[0]
        return self._info(extra_jitter), dict(lml=-1.0, dnoise=0.5, alpha=np.zeros((n, self.Dy)), diag_dL_dK=np.zeros(n))

    def exact_studentt_sum(self, specs, nu, jitter=1e-8, extra_jitter=0.0):
        self.log.append(("exact_studentt_sum", [_spec(s) for s in specs]))
        return self._info(extra_jitter), dict(lml=-1.0, beta=2.0, scale=1.0, alpha=np.zeros((self.X.shape[0], self.Dy)),
                                              dtheta=np.zeros(self._ntheta(specs)))

    def predict(self, kind, ARD, theta, Xnew, full_cov=False, want_var=True):
        self.single.append("predict")
        return self.predict_sum([(kind, ARD, theta, None, 0)], Xnew, full_cov=full_cov)

    def predict_sum(self, specs, Xnew, full_cov=False, want_var=True):
        self.log.append(("predict_sum", [_spec(s) for s in specs]))
        self.arrays["Xnew"] = np.array(Xnew)
        return np.zeros((Xnew.shape[0], self.Dy)), np.ones((Xnew.shape[0], 1))

    def covariance_between_points(self, specs, X1, X2):
        self.log.append(("covariance_between_points", [_spec(s) for s in specs]))
        self.arrays["X1"], self.arrays["X2"] = np.array(X1), np.array(X2)
        return np.zeros((X1.shape[0], X2.shape[0]))

    def predictive_gradients(self, specs, Xnew, want_var=True):
        self.log.append(("predictive_gradients", [_spec(s) for s in specs]))
        self.arrays["Xnew"] = np.array(Xnew)
        M, D = Xnew.shape
        return np.ones((M, D, self.Dy)), np.full((M, D), 2.0)

    # the Laplace session (also EP's)
    def laplace_begin(self, specs):
        self.log.append(("laplace_begin", [_spec(s) for s in specs]))
        self._lap_ntheta = self._ntheta(specs)

    def laplace_newton(self, W, b, extra_jitter=0.0):
        n = self.X.shape[0]
        return self._info(extra_jitter), np.zeros(n), np.zeros(n), 0.0

    def laplace_finish(self, W, extra_jitter=0.0):
        return self._info(extra_jitter), np.zeros(self.X.shape[0]), 0.0

    def laplace_gradients(self, Ki_f, dL_dfhat):
        return np.zeros(self._lap_ntheta)

    def laplace_predict(self, specs, Xnew, wv, full_cov=False, want_var=True):
        self.log.append(("laplace_predict", [_spec(s) for s in specs]))
        self.arrays["Xnew"] = np.array(Xnew)
        return np.zeros((Xnew.shape[0], 1)), np.ones((Xnew.shape[0], 1))

    def ep_recompute(self, tau, v, extra_jitter=0.0, add_diag=0.0, want_sigma=True, want_ms=False):
        n = self.X.shape[0]
        return self._info(extra_jitter), np.zeros(n), np.ones(n), 0.0

    def ep_sweep(self, order, ysign, tau, v, eta=1.0, delta=1.0, **kw):
        n = self.X.shape[0]
        return dict(tau=np.array(tau), v=np.array(v), cav_tau=np.ones(n), cav_v=np.zeros(n), log_Z_hat=np.zeros(n),
                    mu=np.zeros(n), Sigma_diag=np.ones(n))

    # the sparse context
    def vardtc_sum(self, specs, Z, noise, extra_jitter=0.0, want_dL_dm=False, want_stage_ms=False):
        self.log.append(("vardtc_sum", [_spec(s) for s in specs]))
        self.arrays["Z"] = np.array(Z)
        return self._info(extra_jitter), dict(lml=-1.0, dnoise=0.5, dtheta=np.arange(1.0, 1.0 + self._ntheta(specs)),
                                              dZ=np.full(Z.shape, 3.0), woodbury_vector=np.zeros((Z.shape[0], self.Dy)),
                                              dL_dm=None)


class RecSparse(Rec):
    def predict(self, specs, Xnew, full_cov=False, want_var=True):
        self.log.append(("sparse_predict", [_spec(s) for s in specs]))
        self.arrays["Xnew"] = np.array(Xnew)
        return np.zeros((Xnew.shape[0], self.Dy)), np.ones((Xnew.shape[0], 1))


class Recorded(object):
    """the contexts the package made, in order, and the calls of `_lib.kern_K`"""

    def __init__(self, made, kern_K_calls):
        self.made, self.kern_K_calls = made, kern_K_calls


@pytest.fixture
def rec(monkeypatch):
    made = []

    def recording(base):
        class Ctx(base):
            def __init__(self, device=0):
                base.__init__(self, device)
                made.append(self)
        return Ctx
    monkeypatch.setattr(_lib, "Context", recording(Rec))
    monkeypatch.setattr(_lib, "SparseContext", recording(RecSparse))
    kern_K_calls = []

    def kern_K(kind, ARD, theta, X, X2=None, device=0):
        kern_K_calls.append((_spec((kind, ARD, theta, None, 0)), np.array(X)))
        return 2.0 * np.eye(X.shape[0], X.shape[0] if X2 is None else X2.shape[0])
    monkeypatch.setattr(_lib, "kern_K", kern_K)
    return Recorded(made, kern_K_calls)


def _data():
    rng = np.random.default_rng(5)
    X = rng.standard_normal((N, 3))
    X[:, 2] = np.arange(N) % 2                     # a column a Coregionalize can read as the output index
    Y = rng.standard_normal((N, 1))
    return X, Y, (Y > 0).astype(float), X[:5] + 0.25


ALL3 = (0, 1, 2)
CASES = {
    # name: (kernel, the X on the device as columns of the model's X (None = all of it), the parts)
    "rbf_dims20": (lambda: gpy_amd.RBF(2, 1.3, 0.7, active_dims=[2, 0]), [2, 0], [part("rbf", 0, [1.3, 0.7], None, 0)]),
    "linear": (lambda: gpy_amd.Linear(3, 0.4), None, [part("linear", 0, [0.4], None, 0)]),
    "mlp": (lambda: gpy_amd.MLP(3, 1.1, 0.6, 0.2), None, [part("mlp", 0, [1.1, 0.6, 0.2], None, 0)]),
    "stdperiodic": (lambda: gpy_amd.StdPeriodic(3, 0.9, 2.0, 0.8), None, [part("stdperiodic", 0, [0.9, 2.0, 0.8], None, 0)]),
    "rbf+white": (lambda: gpy_amd.RBF(3, 1.3, 0.7) + gpy_amd.White(3, 0.05), None,
                  [part("rbf", 0, [1.3, 0.7], ALL3, 0), part("white", 0, [0.05], ALL3, 0)]),
    "rbf*m32+bias": (lambda: gpy_amd.RBF(2, 1.3, 0.7, active_dims=[0, 1]) * gpy_amd.Matern32(1, 0.4, 2.0, active_dims=[2])
                     + gpy_amd.Bias(3, 0.3), None,
                     [part("rbf", 0, [1.3, 0.7], (0, 1), 1), part("matern32", 0, [0.4, 2.0], (2,), 1),
                      part("bias", 0, [0.3], ALL3, 0)]),
}
LONE_UNFUSED = {
    "white": lambda: gpy_amd.White(3, 0.05),
    "coregionalize": lambda: gpy_amd.Coregionalize(1, 2, W=[[1.0], [0.5]], kappa=[0.3, 0.4], active_dims=[2]),
}


def _cols(X, cols):
    return X if cols is None else X[:, cols]


@pytest.mark.parametrize("name", list(CASES))
def test_exact_gaussian_routes_a_kernel_expression(rec, name):
    make, cols, parts = CASES[name]
    X, Y, _, Xs = _data()
    k = make()
    inf = ExactGaussianInference()
    post, lml, grads = inf.inference(k, X, gpy_amd.Gaussian(0.1), Y)
    ctx, = rec.made
    assert np.array_equal(ctx.X, _cols(X, cols))
    assert ctx.log == [("exact_inference_sum", parts)] and ctx.jitters == [0.0]
    assert grads["dL_dK"].matches_kernel(k) and np.array_equal(grads["dL_dK"].fused_dtheta, np.arange(1.0, 1.0 + k.size))
    post._raw_predict(k, Xs, X)
    assert ctx.log[-1] == ("predict_sum", parts) and np.array_equal(ctx.arrays["Xnew"], _cols(Xs, cols))
    assert ctx.single == []                            # the package calls the `_sum` entries only
    post.covariance_between_points(k, X, Xs[:2], Xs[1:])
    assert ctx.log[-1] == ("covariance_between_points", parts)
    assert np.array_equal(ctx.arrays["X1"], _cols(Xs[:2], cols)) and np.array_equal(ctx.arrays["X2"], _cols(Xs[1:], cols))
    if name == "rbf*m32+bias":                         # products: refused before the device entry, the host composes them
        n_before = len(ctx.log)
        with pytest.raises(NotImplementedError, match="product kernels"):
            post._state.predictive_gradients(k, Xs)
        assert len(ctx.log) == n_before
        return
    dmu, dvar = post.predictive_gradients(k, Xs)
    assert dmu.shape == (5, 3, 1) and dvar.shape == (5, 3)
    assert ctx.log[-1] == ("predictive_gradients", parts) and np.array_equal(ctx.arrays["Xnew"], _cols(Xs, cols))
    if cols is not None:                               # scattered back over the lone kernel's active_dims
        assert np.all(dmu[:, cols, 0] == 1.0) and np.all(dmu[:, 1, 0] == 0.0)
        assert np.all(dvar[:, cols] == 2.0) and np.all(dvar[:, 1] == 0.0)


@pytest.mark.parametrize("name", list(LONE_UNFUSED))
def test_exact_gaussian_does_not_fuse_a_lone_white_or_coregionalize(rec, name):
    X, Y, _, _ = _data()
    k = LONE_UNFUSED[name]()
    post, lml, grads = ExactGaussianInference().inference(k, X, gpy_amd.Gaussian(0.1), Y)
    ctx, = rec.made
    assert np.array_equal(ctx.X, X) and ctx.log == [("inference_given_K", None)]
    if name == "white":
        assert np.array_equal(ctx.arrays["K"], 0.05 * np.eye(N)) and rec.kern_K_calls == []
    else:                                              # kern.K(X): the device K-build of the one kernel on its own column
        B = np.array([[1.3, 0.5], [0.5, 0.65]])
        (spec, Xk), = rec.kern_K_calls
        assert spec == part("coregionalize", 2, B.ravel(), None, 0) and np.array_equal(Xk, X[:, [2]])
        assert np.array_equal(ctx.arrays["K"], 2.0 * np.eye(N))
    assert not grads["dL_dK"].matches_kernel(k) and post.K is not None
    # prediction sends the lone kernel's one part and the points sliced by its active_dims; what the device makes of a kind
    # that it was not given at inference is the device's answer
    _, _, _, Xs = _data()
    post._raw_predict(k, Xs, X)
    one = part("white", 0, [0.05], None, 0) if name == "white" else part("coregionalize", 2, [1.3, 0.5, 0.5, 0.65], None, 0)
    assert ctx.log[-1] == ("predict_sum", [one])
    assert np.array_equal(ctx.arrays["Xnew"], Xs if name == "white" else Xs[:, [2]])


def test_exact_gaussian_with_K_given_does_not_fuse(rec):
    X, Y, _, _ = _data()
    k = gpy_amd.RBF(2, 1.3, 0.7, active_dims=[2, 0])
    K = 3.0 * np.eye(N)
    post, _, grads = ExactGaussianInference().inference(k, X, gpy_amd.Gaussian(0.1), Y, K=K)
    ctx, = rec.made
    assert np.array_equal(ctx.X, X) and ctx.log == [("inference_given_K", None)] and np.array_equal(ctx.arrays["K"], K)
    assert not grads["dL_dK"].matches_kernel(k) and rec.kern_K_calls == []


@pytest.mark.parametrize("name", list(CASES))
def test_studentt_laplace_and_ep_route_a_kernel_expression(rec, name):
    make, cols, parts = CASES[name]
    X, Y, Yc, Xs = _data()
    k = make()
    post, _, grads = ExactStudentTInference().inference(k, X, Y, 5.0)
    ctx = rec.made[-1]
    assert np.array_equal(ctx.X, _cols(X, cols)) and ctx.log == [("exact_studentt_sum", parts)] and ctx.jitters == [0.0]
    assert grads["dL_dK"].matches_kernel(k)
    post._raw_predict(k, Xs, X)
    assert ctx.log[-1] == ("predict_sum", parts) and np.array_equal(ctx.arrays["Xnew"], _cols(Xs, cols))
    assert ctx.single == []
    for inf in (gpy_amd.Laplace(), gpy_amd.EP()):
        np.random.seed(0)
        post, _, grads = inf.inference(k, X, gpy_amd.Bernoulli(), Yc)
        ctx = rec.made[-1]
        assert np.array_equal(ctx.X, _cols(X, cols)) and ctx.log == [("laplace_begin", parts)]
        assert ctx.jitters and set(ctx.jitters) == {0.0}
        assert grads["dL_dK"].matches_kernel(k)
        post._raw_predict(k, Xs, X)
        assert ctx.log[-1] == ("laplace_predict", parts) and np.array_equal(ctx.arrays["Xnew"], _cols(Xs, cols))
    assert len(rec.made) == 3


@pytest.mark.parametrize("name", list(LONE_UNFUSED))
def test_studentt_laplace_and_ep_refuse_a_lone_white_or_coregionalize(rec, name):
    X, Y, Yc, _ = _data()
    k = LONE_UNFUSED[name]()
    with pytest.raises(NotImplementedError, match="the MI355X Student-t path evaluates gpy_amd kernels on the device"):
        ExactStudentTInference().inference(k, X, Y, 5.0)
    with pytest.raises(NotImplementedError, match="the MI355X Laplace path evaluates gpy_amd kernels on the device"):
        gpy_amd.Laplace().inference(k, X, gpy_amd.Bernoulli(), Yc)
    with pytest.raises(NotImplementedError, match="the MI355X EP path evaluates gpy_amd kernels on the device"):
        gpy_amd.EP().inference(k, X, gpy_amd.Bernoulli(), Yc)
    with pytest.raises(NotImplementedError, match="the MI355X Student-t path evaluates gpy_amd kernels on the device"):
        ExactStudentTInference().inference(gpy_amd.RBF(3), X, Y, 5.0, K=np.eye(N))
    assert rec.made == [] and rec.kern_K_calls == []


@pytest.mark.parametrize("name", ["rbf_dims20", "rbf+white", "rbf*m32+bias"])
def test_vardtc_routes_a_kernel_expression(rec, name):
    make, cols, parts = CASES[name]
    X, Y, _, Xs = _data()
    Z = X[::3].copy()
    k = make()
    post, lml, grads = VarDTC().inference(k, X, Z, gpy_amd.Gaussian(0.1), Y)
    ctx, = rec.made
    assert np.array_equal(ctx.X, _cols(X, cols)) and np.array_equal(ctx.arrays["Z"], _cols(Z, cols))
    assert ctx.log == [("vardtc_sum", parts)] and ctx.jitters == [0.0]
    post._raw_predict(k, Xs, Z)
    assert ctx.log[-1] == ("sparse_predict", parts) and np.array_equal(ctx.arrays["Xnew"], _cols(Xs, cols))
    # the model driver installs the fused gradients of a lone kernel and of an expression alike, in link order, and scatters
    # a lone kernel's dZ over its active_dims
    m = gpy_amd.SparseGP(X, Y, Z, make(), gpy_amd.Gaussian(0.1))
    assert np.array_equal(m.kern.gradient, np.arange(1.0, 1.0 + m.kern.size))
    want_dZ = np.full(Z.shape, 3.0)
    if cols is not None:
        want_dZ[:, 1] = 0.0
    assert np.array_equal(m.Z.gradient, want_dZ)


def test_vardtc_accepts_and_refuses_what_it_did(rec):
    X, Y, _, _ = _data()
    Z, lik = X[::3].copy(), gpy_amd.Gaussian(0.1)
    for name, names in (("linear", "Linear"), ("mlp", "MLP"), ("stdperiodic", "StdPeriodic")):
        with pytest.raises(NotImplementedError, match="the MI355X sparse path does not evaluate %s kernels" % names):
            VarDTC().inference(CASES[name][0](), X, Z, lik, Y)
    with pytest.raises(NotImplementedError, match="the MI355X sparse path does not evaluate Coregionalize kernels"):
        VarDTC().inference(LONE_UNFUSED["coregionalize"](), X, Z, lik, Y)
    covers = "the MI355X sparse path covers gpy_amd's stationary kernels"
    for k in (gpy_amd.White(3, 0.05), gpy_amd.Bias(3, 0.3), gpy_amd.RBF(3) * gpy_amd.White(3, 0.05),
              gpy_amd.RBF(3) + gpy_amd.RBF(3) * gpy_amd.White(3, 0.05)):
        with pytest.raises(NotImplementedError, match=covers):
            VarDTC().inference(k, X, Z, lik, Y)
    with pytest.raises(NotImplementedError, match="precomputed statistics"):
        VarDTC().inference(gpy_amd.RBF(3), X, Z, lik, Y, psi1=np.zeros((N, 4)))
    assert rec.made == []


def _ladder_runs(rec, k, X, Y, Yc, maxtries, sparse):
    """[(name, jitters the factorisations were given)] of one failing run of each class"""
    runs = [("gaussian", lambda: ExactGaussianInference(maxtries=maxtries).inference(k, X, gpy_amd.Gaussian(0.1), Y)),
            ("studentt", lambda: ExactStudentTInference(maxtries=maxtries).inference(k, X, Y, 5.0)),
            ("laplace", lambda: gpy_amd.Laplace(maxtries=maxtries).inference(k, X, gpy_amd.Bernoulli(), Yc)),
            ("ep", lambda: gpy_amd.EP(maxtries=maxtries).inference(k, X, gpy_amd.Bernoulli(), Yc))]
    if sparse:
        runs.append(("vardtc", lambda: VarDTC(maxtries=maxtries).inference(k, X, X[::3].copy(), gpy_amd.Gaussian(0.1), Y)))
    out = []
    for name, run in runs:
        with pytest.raises(np.linalg.LinAlgError) as e:
            run()
        assert str(e.value) == "not positive definite, even with jitter."
        out.append((name, rec.made[-1].jitters))
    return out


@pytest.mark.parametrize("maxtries", [5, 2])
def test_every_inference_class_climbs_the_same_jitter_ladder(rec, monkeypatch, maxtries):
    """jitchol's ladder (reference `GPy/util/linalg.py:56-75`): a plain try, then mean(diag) * 1e-6, times 10 per rung, `maxtries`
    rungs, then LinAlgError("not positive definite, even with jitter.").  The mean is that of K's diagonal (of K + noise + 1e-8
    for the Gaussian case, whose factorisation is of that matrix); a Linear kernel's diagonal depends on the point."""
    monkeypatch.setattr(Rec, "fail", True)
    X, Y, Yc, _ = _data()
    for k, kd in ((gpy_amd.RBF(3, 2.0, 0.7), 2.0),
                  (gpy_amd.RBF(3, 2.0, 0.7) + gpy_amd.Bias(3, 0.5), 2.5),
                  (gpy_amd.Linear(3, 0.4), float(np.mean(0.4 * np.sum(X * X, 1))))):
        for name, jitters in _ladder_runs(rec, k, X, Y, Yc, maxtries, sparse=not isinstance(k, gpy_amd.Linear)):
            m = kd + 0.1 + 1e-8 if name == "gaussian" else kd
            assert len(jitters) == maxtries + 1 and jitters[0] == 0.0, (name, jitters)
            assert np.isclose(jitters[1], m * 1e-6, rtol=1e-14, atol=0.0), (name, jitters)
            # the cumulative form of the reference: every rung is ten times the one before, exactly
            assert all(jitters[i + 1] == jitters[i] * 10 for i in range(1, maxtries)), (name, jitters)


def test_non_positive_diagonal_is_reported_by_the_gaussian_path_only(rec, monkeypatch):
    monkeypatch.setattr(Rec, "fail", True)
    X, Y, _, _ = _data()
    K = np.eye(N)
    K[3, 3] = -1.0
    with pytest.raises(np.linalg.LinAlgError, match="not pd: non-positive diagonal elements"):
        ExactGaussianInference().inference(gpy_amd.RBF(3), X, gpy_amd.Gaussian(0.1), Y, K=K)
    assert rec.made[-1].jitters == [0.0]
