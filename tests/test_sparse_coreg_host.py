"""CPU: the host logic of Coregionalize on the sparse path -- what `sparse_path_kernel_check` admits where it is asked and still
refuses, that `VarDTC(coregionalize=True)` switches its context on (`set_coregionalize`) before the data arrive and hands over
the parts `ICM` / `LCM` build, every refusal by its name with no context made, `SparseGPCoregionalizedRegression`'s defaults,
flat parameter order and fixed index column of Z, and the binding table of include/mi355gp_sparse_coreg.h.  No device: a
recording context stands for `_lib.SparseContext`."""
import os
import re

import numpy as np
import pytest

import gpy_amd
from gpy_amd import _lib
from gpy_amd import kern as GK
from gpy_amd.epdtc import EPDTC
from gpy_amd.sparse import VarDTC, sparse_path_kernel_check
from gpy_amd.svgp import SVGP as SVGPInference
from gpy_amd.util import multioutput

HERE = os.path.dirname(os.path.abspath(__file__))


class Handed(Exception):
    """raised by the recording context once a part list has reached it"""


class Recording(object):
    FETCH_DLDKMM, FETCH_WOODBURY_INV, FETCH_LM, FETCH_KMM, FETCH_PSI2, FETCH_DLDPSI2_BETA = range(6)
    sharded = False
    made = []

    def __init__(self, device=0):
        self.calls, self.order = [], []
        Recording.made.append(self)

    def set_data(self, X, Y):
        self.order.append("set_data")
        self.N, self.D = np.shape(X)

    def set_linear(self, on=True):
        self.linear_on = bool(on)

    def set_coregionalize(self, on=True):
        self.order.append("set_coregionalize")
        self.coreg_on = bool(on)

    def vardtc_sum(self, specs, Z, noise, extra_jitter=0.0, **kw):
        self.calls.append([(s[0], int(s[1]), np.asarray(s[2]).tolist(), None if s[3] is None else list(s[3]), s[4]) for s in specs])
        self.noise, self.Z = np.array(noise), np.array(Z)
        raise Handed("vardtc_sum")

    def pep(self, *a, **kw):
        raise AssertionError("a Coregionalize part reached PEP / FITC")

    svgp_forward = epdtc_begin = pep


class Served(Recording):
    """a context that answers: zero gradients, a bound that depends on nothing, predictions of the right shape"""

    def vardtc_sum(self, specs, Z, noise, extra_jitter=0.0, **kw):
        self.calls.append([s[0] for s in specs])
        self.noise, self.Z = np.array(noise), np.array(Z)
        M = np.shape(Z)[0]
        nth = sum(np.size(s[2]) for s in specs)
        return 0, dict(lml=-1.0, dnoise=np.zeros(self.N), dtheta=np.zeros(nth), dZ=np.zeros((M, self.D)),
                       woodbury_vector=np.zeros((M, 1)), dL_dm=None)

    def predict(self, specs, Xnew, full_cov=False, want_var=True):
        n = np.shape(Xnew)[0]
        return np.zeros((n, 1)), np.ones((n, n)) if full_cov else np.ones((n, 1))


@pytest.fixture
def rec(monkeypatch):
    monkeypatch.setattr(Recording, "made", [])
    monkeypatch.setattr(_lib, "SparseContext", Recording)
    return Recording


@pytest.fixture
def served(monkeypatch):
    monkeypatch.setattr(Recording, "made", [])
    monkeypatch.setattr(_lib, "SparseContext", Served)
    return Served


def _data(N=30, M=6, P=2):
    rng = np.random.default_rng(3)
    X, Z = rng.uniform(-0.5, 0.5, (N, 3)), rng.uniform(-0.5, 0.5, (M, 3))
    X[:, 2], Z[:, 2] = np.sort(np.arange(N) % P), np.sort(np.arange(M) % P)
    return X, Z, np.sin(3 * X[:, :1]) + X[:, 2:3]


def _icm(P=2, kernel=None, W_rank=1):
    return multioutput.ICM(2, P, kernel or gpy_amd.RBF(2, 1.3, 0.7), W_rank=W_rank, W=0.4 * np.ones((P, W_rank)), kappa=0.5 * np.ones(P))


def _lists(P=2, n=12, seed=0):
    rng = np.random.default_rng(seed)
    X_list = [rng.uniform(-1, 1, (n + p, 2)) for p in range(P)]
    return X_list, [np.sin(3 * x[:, :1]) + 0.1 * p for p, x in enumerate(X_list)]


def test_the_kernel_check_admits_coregionalize_factors_where_it_is_asked():
    lcm = multioutput.LCM(2, 2, [gpy_amd.RBF(2), gpy_amd.Matern32(2)])
    for k in (_icm(), lcm, _icm() + gpy_amd.Bias(3) + gpy_amd.White(3), gpy_amd.Coregionalize(1, 2, active_dims=[2]) * gpy_amd.Bias(3),
              gpy_amd.RBF(2, active_dims=[0, 1]) * gpy_amd.Bias(3) * gpy_amd.Coregionalize(1, 2, active_dims=[2])):
        sparse_path_kernel_check(k, coregionalize=True)
        sparse_path_kernel_check(k, linear=True, coregionalize=True)
        for kw in ({}, {"linear": True}):                                 # not asked for: by name, with the way to ask
            with pytest.raises(NotImplementedError, match="does not evaluate Coregionalize kernels .*coregionalize=True"):
                sparse_path_kernel_check(k, **kw)
    both = gpy_amd.Linear(2, active_dims=[0, 1]) * gpy_amd.Coregionalize(1, 2, active_dims=[2])
    sparse_path_kernel_check(both, linear=True, coregionalize=True)       # Linear x Coregionalize: both switches
    with pytest.raises(NotImplementedError, match="does not evaluate Linear kernels .*linear=True"):
        sparse_path_kernel_check(both, coregionalize=True)
    with pytest.raises(NotImplementedError, match="does not evaluate Coregionalize kernels"):
        sparse_path_kernel_check(both, linear=True)
    # the values other tests read stay as they are
    assert "coregionalize" in GK.EXACT_ONLY_KINDS and "coregionalize" in GK.SPARSE_REFUSED_KINDS
    assert set(GK.EXACT_ONLY_KINDS) - set(GK.SPARSE_REFUSED_KINDS) == {"linear"}


def test_vardtc_switches_its_context_before_the_data_and_hands_over_the_parts(rec):
    X, Z, Y = _data()
    lik = gpy_amd.MixedNoise([gpy_amd.Gaussian(0.1), gpy_amd.Gaussian(0.3)])
    meta = {"output_index": X[:, 2:3].astype(int)}
    with pytest.raises(Handed):
        VarDTC(coregionalize=True).inference(_icm(), X, Z, lik, Y, Y_metadata=meta)
    c = rec.made[-1]
    assert c.order == ["set_coregionalize", "set_data"] and c.coreg_on and not hasattr(c, "linear_on")
    B = 0.16 * np.ones((2, 2)) + 0.5 * np.eye(2)
    (rbf, cg), = c.calls
    assert rbf == ("rbf", 0, [1.3, 0.7], [0, 1], 1)
    assert (cg[0], cg[1], cg[3], cg[4]) == ("coregionalize", 2, [2], 1) and np.allclose(cg[2], B.ravel(), rtol=1e-15, atol=0)
    assert c.D == 3 and np.array_equal(c.Z[:, 2], Z[:, 2])
    assert np.array_equal(c.noise, np.where(X[:, 2] == 0, 0.1, 0.3))      # MixedNoise: each row its output's variance
    lcm = multioutput.LCM(2, 2, [gpy_amd.RBF(2), gpy_amd.Matern32(2)], W_rank=2)
    with pytest.raises(Handed):
        VarDTC(coregionalize=True).inference(lcm, X, Z, lik, Y, Y_metadata=meta)
    assert [(s[0], s[1], s[4]) for s in rec.made[-1].calls[0]] == [("rbf", 0, 1), ("coregionalize", 2, 1), ("matern32", 0, 2),
                                                                  ("coregionalize", 2, 2)]
    with pytest.raises(Handed):                                           # both switches
        VarDTC(linear=True, coregionalize=True).inference(gpy_amd.Linear(2, active_dims=[0, 1])
                                                          * gpy_amd.Coregionalize(1, 2, active_dims=[2]), X, Z, lik, Y, Y_metadata=meta)
    assert rec.made[-1].linear_on and rec.made[-1].coreg_on
    with pytest.raises(Handed):                                           # a session that was not asked does not switch its context
        VarDTC().inference(gpy_amd.RBF(3), X, Z, gpy_amd.Gaussian(0.1), Y)
    assert not hasattr(rec.made[-1], "coreg_on")
    with pytest.raises(Handed):
        gpy_amd.SparseGP(X, Y, Z, _icm(), lik, inference_method=VarDTC(coregionalize=True), Y_metadata=meta)
    assert rec.made[-1].coreg_on


def test_every_refusal_is_by_name_and_before_a_context_is_made(rec):
    X, Z, Y = _data()
    M = Z.shape[0]
    Yc = (Y > 0).astype(float)
    k = _icm()
    # a class made without the switch, and the families that have none
    runs = [lambda **kw: VarDTC(**kw).inference(k, X, Z, gpy_amd.Gaussian(0.1), Y),
            lambda **kw: gpy_amd.FITC(**kw).inference(k, X, Z, gpy_amd.Gaussian(0.1), Y),
            lambda **kw: gpy_amd.PEP(0.5, **kw).inference(k, X, Z, gpy_amd.Gaussian(0.1), Y),
            lambda **kw: SVGPInference(**kw).inference(np.zeros((M, 1)), np.ones((M * (M + 1) // 2, 1)), k, X, Z, gpy_amd.Gaussian(0.1), Y),
            lambda **kw: EPDTC(**kw).inference(k, X, Z, gpy_amd.Bernoulli(), Yc)]
    for run in runs:
        for kw in ({}, {"linear": True}):
            with pytest.raises(NotImplementedError, match="sparse path does not evaluate Coregionalize kernels"):
                run(**kw)
    for cls in (gpy_amd.FITC, SVGPInference, EPDTC):                      # no `coregionalize=` keyword on them
        with pytest.raises(TypeError):
            cls(coregionalize=True)
    with pytest.raises(TypeError):
        gpy_amd.PEP(0.5, coregionalize=True)
    # P > 16, a White factor, a lone Coregionalize
    big = multioutput.ICM(2, 17, gpy_amd.RBF(2), W=np.zeros((17, 1)), kappa=np.ones(17))
    with pytest.raises(NotImplementedError, match="at most 16 outputs"):
        VarDTC(coregionalize=True).inference(big, X, Z, gpy_amd.Gaussian(0.1), Y)
    with pytest.raises(NotImplementedError, match="sparse path covers"):
        VarDTC(coregionalize=True).inference(gpy_amd.Coregionalize(1, 2, active_dims=[2]) * gpy_amd.White(3), X, Z, gpy_amd.Gaussian(0.1), Y)
    with pytest.raises(NotImplementedError, match="sparse path covers"):
        VarDTC(coregionalize=True).inference(gpy_amd.Coregionalize(1, 2, active_dims=[2]), X, Z, gpy_amd.Gaussian(0.1), Y)
    # uncertain inputs, NormalPosterior, BayesianGPLVM, X_variance on the model
    qX = gpy_amd.NormalPosterior(X, np.full(X.shape, 0.1))
    with pytest.raises(NotImplementedError, match=r"uncertain inputs: the part .*\(Prod of RBF, Coregionalize\) has no psi-statistics"):
        VarDTC(coregionalize=True).inference(k, qX, Z, gpy_amd.Gaussian(0.1), Y)
    with pytest.raises(NotImplementedError, match="Coregionalize"):
        gpy_amd.BayesianGPLVM(Y, 3, X=X, kernel=k, num_inducing=4)
    X_list, Y_list = _lists()
    with pytest.raises(NotImplementedError, match="SparseGPCoregionalizedRegression: X_variance"):
        gpy_amd.SparseGPCoregionalizedRegression(X_list, Y_list, X_variance=[np.full(x.shape, 0.1) for x in X_list])
    assert rec.made == []
    # a row-sharded context: by name, before set_data or any call
    inf = VarDTC(coregionalize=True)
    inf._ctx = Recording()
    inf._ctx.sharded = True
    with pytest.raises(NotImplementedError, match="Coregionalize kernel is not supported by a row-sharded sparse context"):
        inf.inference(k, X, Z, gpy_amd.Gaussian(0.1), Y)
    assert inf._ctx.calls == [] and not hasattr(inf._ctx, "N")
    # the grid mode names the kind as before
    from gpy_amd import grid as G
    with pytest.raises(NotImplementedError, match="Coregionalize"):
        G.GridContext.exact_inference(object.__new__(G.GridContext), "coregionalize", 2, np.ones(4), 0.1)


def test_the_model_has_the_references_defaults_and_a_fixed_index_column(served):
    X_list, Y_list = _lists(P=3)
    m = gpy_amd.SparseGPCoregionalizedRegression(X_list, Y_list, num_inducing=4, seed=1)
    assert gpy_amd.models.SparseGPCoregionalizedRegression is gpy_amd.SparseGPCoregionalizedRegression
    assert m.name == "SGPCR" and m.kern.name == "coreg" and isinstance(m.likelihood, gpy_amd.MixedNoise)
    assert [type(p).__name__ for p in m.kern.parts] == ["RBF", "Coregionalize"]
    rbf, B = m.kern.parts
    assert rbf.input_dim == 2 and B.output_dim == 3 and B.rank == 1 and list(B.active_dims) == [2]
    assert m.inference_method.coregionalize and served.made[-1].coreg_on
    # Z: num_inducing rows of each output's own inputs, stacked with the index column
    assert m.Z.shape == (12, 3) and np.array_equal(m.Z.values[:, 2], np.repeat([0.0, 1.0, 2.0], 4))
    for p in range(3):
        rows = m.Z.values[m.Z.values[:, 2] == p][:, :2]
        assert all(np.any(np.all(X_list[p] == r, axis=1)) for r in rows)
    # flat parameter order [Z, kernel (variance, lengthscale, W, kappa), one noise per output]
    assert m.param_array.size == 36 + 2 + 3 + 3 + 3
    assert np.array_equal(m.param_array[:36], m.Z.values.ravel())
    assert m.param_array[36] == 1.0 and m.param_array[37] == 1.0 and np.all(m.param_array[41:44] == 0.5)
    assert np.all(m.param_array[44:] == 1.0)
    assert np.array_equal(served.made[-1].noise, np.ones(m.num_data))
    # the index column does not move: under any assignment of the parameter vector, under checkgrad, under optimize
    x = m.param_array.copy()
    x[:36] += 0.25
    m.param_array = x
    assert np.array_equal(m.Z.values[:, 2], np.repeat([0.0, 1.0, 2.0], 4)) and np.allclose(m.Z.values[:, :2].ravel(), x[:36].reshape(12, 3)[:, :2].ravel())
    assert np.array_equal(served.made[-1].Z[:, 2], m.Z.values[:, 2])
    m.checkgrad()
    m.optimize(max_iters=3)
    assert np.array_equal(m.Z.values[:, 2], np.repeat([0.0, 1.0, 2.0], 4)) and np.all(m.Z.gradient[:, 2] == 0.0)
    # a list per output, the reference's assertion on a wrong length, one count per output
    m2 = gpy_amd.SparseGPCoregionalizedRegression(X_list, Y_list, num_inducing=[2, 3, 4], seed=1)
    assert np.array_equal(m2.Z.values[:, 2], np.repeat([0.0, 1.0, 2.0], [2, 3, 4]))
    with pytest.raises(AssertionError, match="Number of outputs"):
        gpy_amd.SparseGPCoregionalizedRegression(X_list, Y_list, Z_list=[X_list[0][:2]])
    m3 = gpy_amd.SparseGPCoregionalizedRegression(X_list, Y_list, Z_list=[x[:2] for x in X_list], W_rank=2, kernel_name="k")
    assert m3.kern.parts[1].rank == 2 and m3.kern.name == "k" and m3.Z.shape == (6, 3)


def test_two_constructions_share_no_inducing_list(served):
    """the reference appends into its mutable default `Z_list=[]`: a second model would carry the first one's inducing inputs"""
    X_list, Y_list = _lists()
    a = gpy_amd.SparseGPCoregionalizedRegression(X_list, Y_list, num_inducing=3)
    b = gpy_amd.SparseGPCoregionalizedRegression(X_list, Y_list, num_inducing=3)
    assert a.Z.shape == b.Z.shape == (6, 3)
    mine = []
    c = gpy_amd.SparseGPCoregionalizedRegression(X_list, Y_list, Z_list=mine, num_inducing=2)
    assert mine == [] and c.Z.shape == (4, 3)
    import inspect
    assert inspect.signature(gpy_amd.SparseGPCoregionalizedRegression.__init__).parameters["Z_list"].default is None


def test_predict_routes_the_noise_by_the_new_points_output_index(served):
    X_list, Y_list = _lists()
    lik = [gpy_amd.Gaussian(0.1, name="n0"), gpy_amd.Gaussian(0.4, name="n1")]
    m = gpy_amd.SparseGPCoregionalizedRegression(X_list, Y_list, likelihoods_list=lik, num_inducing=3)
    Xn = np.hstack([np.zeros((4, 2)), np.array([[0.0], [1.0], [1.0], [0.0]])])
    mu, var = m.predict(Xn, Y_metadata={"output_index": Xn[:, 2:3].astype(int)})
    assert np.allclose(var.ravel(), 1.0 + np.array([0.1, 0.4, 0.4, 0.1]))
    assert np.allclose(m.predict_noiseless(Xn)[1], 1.0)
    lo, hi = m.predict_quantiles(Xn, Y_metadata={"output_index": Xn[:, 2:3].astype(int)})
    assert np.all(hi > lo) and (hi - lo)[1] > (hi - lo)[0]
    assert m.posterior_samples_f(Xn, size=2).shape == (4, 1, 2)


def test_the_binding_table_matches_the_header():
    text = open(os.path.join(HERE, "..", "include", "mi355gp_sparse_coreg.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"\bint\s+(mi355gp_\w+)\s*\(([^;]*?)\)\s*;", text)
    assert [p[0] for p in protos] == list(_lib.SPARSE_COREG_ABI) == ["mi355gp_sparse_set_coregionalize"]
    assert [p.strip() for p in protos[0][1].split(",")] == ["mi355gp_sparse* s", "int on"]
    assert len(_lib.SPARSE_COREG_ABI["mi355gp_sparse_set_coregionalize"]) == 2
    # the diagnostics header: one entry point, in neither of the two headers whose prototypes tests/test_abi.py counts
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(HERE, "..", "include", "mi355gp_debug_sparse_coreg.h")).read(), flags=re.S)
    protos = re.findall(r"\bint\s+(mi355gp_\w+)\s*\(([^;]*?)\)\s*;", text)
    assert [p[0] for p in protos] == list(_lib.DEBUG_SPARSE_COREG_ABI) == ["mi355gp_dbg_sparse_set_fuse_cols"]
    assert [p.strip() for p in protos[0][1].split(",")] == ["mi355gp_sparse* s", "int on"]
    for counted in ("mi355gp.h", "mi355gp_debug.h"):
        assert "set_fuse_cols" not in open(os.path.join(HERE, "..", "include", counted)).read()
        assert "set_coregionalize" not in open(os.path.join(HERE, "..", "include", counted)).read()
