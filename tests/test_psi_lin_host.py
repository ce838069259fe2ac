"""CPU: the host routing of the Linear / Bias psi-statistics -- `psi_lin_bias=True` on `VarDTC`, `SparseGPRegression` and
`BayesianGPLVM` hands one RBF or Linear part with Bias and White parts to the context's uncertain-input entry point and tells
the context so (`set_psi_lin_bias`, once, before the first evaluation); what is out of scope is refused by name before any
context call; a class made without the keyword never reaches a context; and the binding table of include/mi355gp_psi_lin.h.
No device: a recording context stands for `_lib.SparseContext`."""
import os
import re

import numpy as np
import pytest

import gpy_amd
from gpy_amd import _lib
from gpy_amd.sparse import VarDTC

HERE = os.path.dirname(os.path.abspath(__file__))


class Handed(Exception):
    """raised by the recording context once a part list has reached it"""


class Recording(object):
    sharded = False
    made = []

    def __init__(self, device=0):
        self.log = []
        Recording.made.append(self)

    def set_data(self, X, Y):
        self.log.append("set_data")
        self.N, self.D = np.shape(X)

    def set_input_variance(self, S):
        self.log.append("set_input_variance")

    def set_linear(self, on=True):
        self.log.append("set_linear(%d)" % bool(on))

    def set_psi_lin_bias(self, on=True):
        self.log.append("set_psi_lin_bias(%d)" % bool(on))

    def vardtc_uncertain(self, specs, Z, noise, extra_jitter=0.0, **kw):
        self.log.append(("vardtc_uncertain", [s[0] for s in specs]))
        raise Handed("vardtc_uncertain")

    def vardtc_sum(self, specs, Z, noise, extra_jitter=0.0, **kw):
        self.log.append(("vardtc_sum", [s[0] for s in specs]))
        raise Handed("vardtc_sum")


@pytest.fixture
def rec(monkeypatch):
    monkeypatch.setattr(Recording, "made", [])
    monkeypatch.setattr(_lib, "SparseContext", Recording)
    return Recording


def _data(N=20, M=5, D=2, Dy=2):
    r = np.random.default_rng(4)
    X, Z = r.uniform(-1, 1, (N, D)), r.uniform(-1, 1, (M, D))
    return X, np.full((N, D), 0.1), Z, X @ r.standard_normal((D, Dy))


def _kernels():
    return ((lambda: gpy_amd.Linear(2, ARD=True) + gpy_amd.Bias(2) + gpy_amd.White(2), ["linear", "bias", "white"]),
            (lambda: gpy_amd.RBF(2, ARD=True) + gpy_amd.Bias(2), ["rbf", "bias"]))


def _routes(make, X, S, Z, Y, **kw):
    q = gpy_amd.NormalPosterior(X, S)
    return (lambda: VarDTC(**kw).inference(make(), q, Z, gpy_amd.Gaussian(0.1), Y),
            lambda: gpy_amd.SparseGPRegression(X, Y, kernel=make(), Z=Z, X_variance=S, **kw),
            lambda: gpy_amd.BayesianGPLVM(Y, 2, X=X, X_variance=S, Z=Z, kernel=make(), **kw),
            lambda: gpy_amd.SparseGP(q, Y, Z, make(), gpy_amd.Gaussian(0.1), inference_method=VarDTC(**kw)))


def test_every_class_hands_the_part_lists_to_the_context_and_switches_it_once(rec):
    X, S, Z, Y = _data()
    for make, want in _kernels():
        for run in _routes(make, X, S, Z, Y, psi_lin_bias=True):
            n0 = len(rec.made)
            with pytest.raises(Handed, match="vardtc_uncertain"):
                run()
            assert len(rec.made) == n0 + 1
            log = rec.made[-1].log
            assert log[0] == "set_psi_lin_bias(1)" and log.count("set_psi_lin_bias(1)") == 1      # before the data, once
            assert log[-1] == ("vardtc_uncertain", want) and "set_linear(1)" not in log
    # one session, two evaluations: the context is switched once
    inf = VarDTC(psi_lin_bias=True)
    assert inf.linear and inf.psi_lin_bias                          # the keyword implies linear=True
    q = gpy_amd.NormalPosterior(X, S)
    for _ in range(2):
        with pytest.raises(Handed):
            inf.inference(_kernels()[0][0](), q, Z, gpy_amd.Gaussian(0.1), Y)
    assert len(rec.made[-1].log) >= 2 and rec.made[-1].log.count("set_psi_lin_bias(1)") == 1
    assert [e for e in rec.made[-1].log if isinstance(e, tuple)] == [("vardtc_uncertain", ["linear", "bias", "white"])] * 2
    # certain inputs through the same session: Linear is taken there as with linear=True
    with pytest.raises(Handed, match="vardtc_sum"):
        inf.inference(_kernels()[0][0](), X, Z, gpy_amd.Gaussian(0.1), Y)


def test_without_the_keyword_nothing_reaches_a_context(rec):
    X, S, Z, Y = _data()
    for make, _ in _kernels():
        for run in _routes(make, X, S, Z, Y):
            with pytest.raises(NotImplementedError, match="has no psi-statistics on the MI355X sparse path.*psi_lin_bias=True"):
                run()
    with pytest.raises(NotImplementedError, match="has no psi-statistics"):
        VarDTC(linear=True).inference(gpy_amd.Linear(2), gpy_amd.NormalPosterior(X, S), Z, gpy_amd.Gaussian(0.1), Y)
    assert rec.made == []


def test_the_keyword_next_to_an_inference_method_made_without_it_is_refused(rec):
    X, S, Z, Y = _data()
    k = _kernels()[0][0]
    with pytest.raises(ValueError, match="psi_lin_bias=True, but the given inference_method was made without it"):
        gpy_amd.BayesianGPLVM(Y, 2, X=X, X_variance=S, Z=Z, kernel=k(), inference_method=VarDTC(), psi_lin_bias=True)
    assert rec.made == []
    with pytest.raises(Handed, match="vardtc_uncertain"):          # one made with it is taken as it is
        gpy_amd.BayesianGPLVM(Y, 2, X=X, X_variance=S, Z=Z, kernel=k(), inference_method=VarDTC(psi_lin_bias=True), psi_lin_bias=True)


def test_what_is_out_of_scope_is_refused_by_name_with_no_context_call(rec):
    X, S, Z, Y = _data()
    q = gpy_amd.NormalPosterior(X, S)
    lik = gpy_amd.Gaussian(0.1)
    inf = lambda: VarDTC(psi_lin_bias=True)
    for k, pat in ((gpy_amd.RBF(2) + gpy_amd.Linear(2), r"exactly one input-dependent part.*'rbf': RBF, 'linear': Linear"),
                   (gpy_amd.RBF(2) + gpy_amd.RBF(2, name="rbf2"), r"exactly one input-dependent part.*'rbf2': RBF"),
                   (gpy_amd.Linear(2) * gpy_amd.Bias(2) + gpy_amd.White(2), r"\(Prod of Linear, Bias\) has no psi-statistics"),
                   (gpy_amd.Matern52(2) + gpy_amd.Bias(2), r"'Mat52' \(Matern52\) has no psi-statistics"),
                   (gpy_amd.Bias(2) + gpy_amd.White(2), "exactly one input-dependent part")):
        with pytest.raises(NotImplementedError, match=pat):
            inf().inference(k, q, Z, lik, Y)
    with pytest.raises(NotImplementedError, match="per-point"):
        inf().inference(gpy_amd.Linear(2) + gpy_amd.Bias(2), q, Z, lik, Y, precision=np.full(X.shape[0], 10.0))
    with pytest.raises(ValueError, match="Mean function not implemented with uncertain inputs"):
        inf().inference(gpy_amd.Linear(2) + gpy_amd.Bias(2), q, Z, lik, Y, mean_function=object())
    assert rec.made == []
    sharded = inf()
    sharded._ctx = Recording()
    sharded._ctx.sharded = True
    with pytest.raises(NotImplementedError, match="row-sharded"):
        sharded.inference(gpy_amd.Linear(2) + gpy_amd.Bias(2) + gpy_amd.White(2), q, Z, lik, Y)
    assert sharded._ctx.log == []


def test_flat_parameter_order_of_bayesian_gplvm_with_linear_bias_white(monkeypatch):
    """[X.mean, X.variance, Z, variances, bias, white, noise]"""
    X, S, Z, Y = _data()
    N, D = X.shape
    M = Z.shape[0]

    def inference(self, kern, qX, Zv, likelihood, Yv, **kw):      # no device: constant results of the right shapes
        fused = {"dtheta": np.arange(4.0) + 1, "dZ": np.full(Zv.shape, 7.0), "dmu": np.full(qX.shape, 8.0), "dS": np.full(qX.shape, 9.0)}
        return None, -1.0, {"dL_dthetaL": np.array([5.0]), "fused": fused}
    monkeypatch.setattr(VarDTC, "inference", inference)
    k = gpy_amd.Linear(2, variances=[0.4, 0.6], ARD=True) + gpy_amd.Bias(2, variance=0.5) + gpy_amd.White(2, variance=0.2)
    m = gpy_amd.BayesianGPLVM(Y, 2, X=X, X_variance=S, Z=Z, kernel=k, likelihood=gpy_amd.Gaussian(0.3), psi_lin_bias=True)
    assert isinstance(m.inference_method, VarDTC) and m.inference_method.psi_lin_bias
    want = np.concatenate([X.ravel(), S.ravel(), Z.ravel(), [0.4, 0.6], [0.5], [0.2], [0.3]])
    assert np.array_equal(m.param_array, want)
    g = m.gradient
    assert np.array_equal(g[2 * N * D + M * D:], [1.0, 2.0, 3.0, 4.0, 5.0]) and np.all(g[2 * N * D:2 * N * D + M * D] == 7.0)
    assert np.allclose(g[:N * D], 8.0 - X.ravel())                  # the KL term's share on the means


def test_the_host_fallback_predicts_through_the_kernel_psi_methods():
    """a posterior that is no longer live: `Add.psi*(psi_lin_bias=True)` on the host, against the long-double restatement"""
    import psi_lin_ld as L
    from gpy_amd.sparse import SparsePosterior
    p = L.problem("linear", 25, 6, 3, 2, 8)
    ref = L.evaluate(p["k"], p["Z"], p["mu"], p["S"], p["Y"], p["noise"], np.float64)
    post = SparsePosterior(ref["woodbury_inv"], ref["woodbury_vector"], None, None)
    post.psi_lin_bias = True
    r = np.random.default_rng(2)
    q = gpy_amd.NormalPosterior(r.uniform(-2, 2, (5, 3)), r.uniform(0.05, 0.5, (5, 3)))
    mu, var = post._raw_predict(L.make_kernel(p["k"]), q, p["Z"])
    wm, wv = L.predict(p["k"], p["Z"], ref, q.mean.values, q.variance.values, np.longdouble)
    assert np.abs(mu - wm).max() <= 1e-12 * np.abs(wm).max() and np.abs(var - wv).max() <= 1e-11 * np.abs(wv).max()
    post.psi_lin_bias = False
    with pytest.raises(NotImplementedError, match="psi_lin_bias=True"):
        post._raw_predict(L.make_kernel(p["k"]), q, p["Z"])


def _protos(header):
    text = open(os.path.join(HERE, "..", "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.findall(r"\bint\s+(mi355gp_\w+)\s*\(([^;]*?)\)\s*;", text)


def test_the_binding_tables_match_the_headers_and_the_library_exports_them():
    """the feature switch alone in include/mi355gp_psi_lin.h, the row-kernel probe in the diagnostics header next to it"""
    import ctypes
    protos = _protos("mi355gp_psi_lin.h")
    assert [p[0] for p in protos] == list(_lib.PSI_LIN_ABI) == ["mi355gp_sparse_set_psi_lin_bias"]
    assert [" ".join(p.split()) for p in protos[0][1].split(",")] == ["mi355gp_sparse* s", "int on"]
    assert _lib.PSI_LIN_ABI["mi355gp_sparse_set_psi_lin_bias"] == [ctypes.c_void_p, ctypes.c_int]
    dbg = _protos("mi355gp_debug_psi_lin.h")
    assert [p[0] for p in dbg] == list(_lib.DEBUG_PSI_LIN_ABI) == ["mi355gp_dbg_psi_lin_rows"]
    params = [" ".join(p.split()) for p in dbg[0][1].split(",")]
    bound = _lib.DEBUG_PSI_LIN_ABI["mi355gp_dbg_psi_lin_rows"]
    assert len(bound) == len(params) == 19
    for c, b in zip(params, bound):
        if "double*" in c:
            assert getattr(b, "_dtype_", None) == np.dtype(np.float64) or b is ctypes.POINTER(ctypes.c_double), c
        elif c.startswith("int64_t"):
            assert b is ctypes.c_int64, c
        elif c.startswith("double"):
            assert b is ctypes.c_double, c
        else:
            assert c.startswith("int ") and b is ctypes.c_int, c
    names = list(_lib.PSI_LIN_ABI) + list(_lib.DEBUG_PSI_LIN_ABI)
    for name in names:                                               # not in mi355gp.h / mi355gp_debug.h: their count stays
        assert name not in _lib.ABI
    _lib.build()
    lib = _lib.lib()
    for name in names:
        assert hasattr(lib, name), "libmi355gp.so does not export %s" % name
