"""CPU: the host logic of the Linear kernel on the sparse path -- what `sparse_path_kernel_check` admits and still refuses,
that each inference family hands a Linear part to the device context, the jitter ladder's first rung for a kernel whose
diagonal depends on the inducing point, and the binding table of include/mi355gp_sparse_diag.h.  Linear is asked for: an
inference class made with `linear=True` takes it and tells its context so (`set_linear`); one made without refuses it by name,
as every one did before.  No device: a recording context stands for `_lib.SparseContext`."""
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

HERE = os.path.dirname(os.path.abspath(__file__))


class Handed(Exception):
    """raised by the recording context once a part list has reached it"""


class Recording(object):
    sharded = False
    fail = False                         # True: every factorisation reports info = 1 (the jitter ladder climbs)
    made = []

    def __init__(self, device=0):
        self.calls, self.jitters = [], []
        Recording.made.append(self)

    def set_data(self, X, Y):
        self.N, self.D = np.shape(X)

    def set_linear(self, on=True):
        self.linear_on = bool(on)

    def _entry(self, name, specs, jitter):
        self.calls.append((name, [(s[0], int(bool(s[1])), np.asarray(s[2]).tolist(), None if s[3] is None else list(s[3]), s[4])
                                  for s in specs]))
        self.jitters.append(float(jitter))
        if self.fail:
            return 1, {}
        raise Handed(name)

    def vardtc_sum(self, specs, Z, noise, extra_jitter=0.0, **kw):
        return self._entry("vardtc_sum", specs, extra_jitter)

    def pep(self, specs, Z, noise_variance, alpha, jitter, **kw):
        return self._entry("pep", specs, jitter)

    def svgp_forward(self, specs, Z, q_mean, q_chol, extra_jitter=0.0, **kw):
        return self._entry("svgp_forward", specs, extra_jitter)

    def epdtc_begin(self, specs, Z, jitter=0.0):
        return self._entry("epdtc_begin", specs, jitter)


@pytest.fixture
def rec(monkeypatch):
    monkeypatch.setattr(Recording, "made", [])
    monkeypatch.setattr(_lib, "SparseContext", Recording)
    return Recording


def _data(N=30, M=6, D=2):
    rng = np.random.default_rng(3)
    X, Z = rng.uniform(-0.5, 0.5, (N, D)), rng.uniform(-0.5, 0.5, (M, D))
    return X, Z, np.sin(3 * X[:, :1]) + X[:, 1:2]


def _runs(k, X, Z, Y, **kw):
    """(entry point, one inference call) of every family; kw: the classes' keywords (linear, maxtries)"""
    M = Z.shape[0]
    Yc = (Y > 0).astype(float)
    return (("vardtc_sum", lambda: VarDTC(**kw).inference(k, X, Z, gpy_amd.Gaussian(0.1), Y)),
            ("pep", lambda: gpy_amd.FITC(**kw).inference(k, X, Z, gpy_amd.Gaussian(0.1), Y)),
            ("pep", lambda: gpy_amd.PEP(0.5, **kw).inference(k, X, Z, gpy_amd.Gaussian(0.1), Y)),
            ("svgp_forward", lambda: SVGPInference(**kw).inference(np.zeros((M, 1)), np.ones((M * (M + 1) // 2, 1)), k, X, Z,
                                                                   gpy_amd.Gaussian(0.1), Y)),
            ("epdtc_begin", lambda: EPDTC(**kw).inference(k, X, Z, gpy_amd.Bernoulli(), Yc)))


def test_the_kernel_check_admits_linear_alone_in_sums_and_in_products():
    for k in (gpy_amd.Linear(2), gpy_amd.RBF(2) + gpy_amd.Linear(2), gpy_amd.RBF(2) + gpy_amd.Linear(2, ARD=True) + gpy_amd.White(2),
              gpy_amd.Linear(2) * gpy_amd.RBF(2), gpy_amd.Linear(2) * gpy_amd.Bias(2) + gpy_amd.RBF(2),
              gpy_amd.Linear(1, active_dims=[0]) * gpy_amd.Linear(1, active_dims=[1]) + gpy_amd.Bias(2)):
        sparse_path_kernel_check(k, linear=True)
        with pytest.raises(NotImplementedError, match="does not evaluate Linear kernels .*linear=True"):
            sparse_path_kernel_check(k)                                   # not asked for: refused by name, with the way to ask
    assert "linear" in GK.EXACT_ONLY_KINDS and "linear" not in GK.SPARSE_REFUSED_KINDS       # the grid path still refuses it
    assert set(GK.EXACT_ONLY_KINDS) - set(GK.SPARSE_REFUSED_KINDS) == {"linear"}
    assert GK.sparse_refused_leaves(gpy_amd.RBF(2) + gpy_amd.Linear(2)) == []


def test_every_family_hands_the_linear_part_to_the_context(rec):
    X, Z, Y = _data()
    k = gpy_amd.RBF(2, 1.3, 0.7) + gpy_amd.Linear(2, [0.4, 0.6], ARD=True)
    want = [("rbf", 0, [1.3, 0.7], [0, 1], 0), ("linear", 1, [0.4, 0.6], [0, 1], 0)]
    for entry, run in _runs(k, X, Z, Y, linear=True):
        with pytest.raises(Handed, match=entry):
            run()
        assert rec.made[-1].calls == [(entry, want)] and rec.made[-1].linear_on
    for entry, run in _runs(k, X, Z, Y):                                  # the classes as they are made by default
        with pytest.raises(NotImplementedError, match="does not evaluate Linear kernels"):
            run()
    assert all(c.calls for c in rec.made)                                 # (no context was made for those)
    with pytest.raises(Handed):                                           # a session that was not asked does not switch its context
        VarDTC().inference(gpy_amd.RBF(2), X, Z, gpy_amd.Gaussian(0.1), Y)
    assert not hasattr(rec.made[-1], "linear_on")
    lone = gpy_amd.Linear(1, 0.8, active_dims=[1])                        # alone: one part, the columns sliced on upload
    with pytest.raises(Handed):
        VarDTC(linear=True).inference(lone, X, Z, gpy_amd.Gaussian(0.1), Y)
    assert rec.made[-1].calls == [("vardtc_sum", [("linear", 0, [0.8], None, 0)])] and rec.made[-1].D == 1
    prod = gpy_amd.Linear(1, 0.5, active_dims=[0]) * gpy_amd.RBF(1, 1.0, 0.3, active_dims=[1]) + gpy_amd.White(2, 0.01)
    with pytest.raises(Handed):
        VarDTC(linear=True).inference(prod, X, Z, gpy_amd.Gaussian(0.1), Y)
    assert [(s[0], s[4]) for s in rec.made[-1].calls[0][1]] == [("linear", 1), ("rbf", 1), ("white", 0)]


def test_what_stays_refused_names_its_reason(rec):
    X, Z, Y = _data()
    lin = gpy_amd.RBF(2) + gpy_amd.Linear(2)
    for cls, make in (("MLP", lambda: gpy_amd.MLP(2)), ("Poly", lambda: gpy_amd.Poly(2)), ("RatQuad", lambda: gpy_amd.RatQuad(2)),
                      ("StdPeriodic", lambda: gpy_amd.StdPeriodic(2)), ("Cosine", lambda: gpy_amd.Cosine(2)),
                      ("Coregionalize", lambda: gpy_amd.Coregionalize(1, 2, active_dims=[1]))):
        for k in (make(), gpy_amd.Linear(2) + make()):
            for _, run in _runs(k, X, Z, Y, linear=True):
                with pytest.raises(NotImplementedError, match="sparse path does not evaluate %s kernels" % cls):
                    run()
    for k in (gpy_amd.RBF(2) * gpy_amd.White(2), gpy_amd.Linear(2) * gpy_amd.White(2)):      # a White factor, as before
        with pytest.raises(NotImplementedError, match="sparse path covers"):
            VarDTC(linear=True).inference(k, X, Z, gpy_amd.Gaussian(0.1), Y)
    # uncertain inputs: the psi-statistics of Linear are not there (a product names its factors)
    qX = gpy_amd.NormalPosterior(X, np.full(X.shape, 0.1))
    for k, pat in ((lin, r"'linear' \(Linear\)"), (gpy_amd.Linear(2), r"\(Linear\)"), (gpy_amd.RBF(2) * gpy_amd.Linear(2), r"\(Prod of RBF, Linear\)")):
        with pytest.raises(NotImplementedError, match="uncertain inputs: the part .*%s has no psi-statistics" % pat):
            VarDTC(linear=True).inference(k, qX, Z, gpy_amd.Gaussian(0.1), Y)
    with pytest.raises(NotImplementedError):
        gpy_amd.BayesianGPLVM(Y, 2, X=X, kernel=lin, num_inducing=4)
    assert rec.made == []
    # a row-sharded context: by name, before set_data or any call
    inf = VarDTC(linear=True)
    inf._ctx = Recording()
    inf._ctx.sharded = True
    with pytest.raises(NotImplementedError, match="Linear kernel is not supported by a row-sharded sparse context"):
        inf.inference(lin, X, Z, gpy_amd.Gaussian(0.1), Y)
    assert inf._ctx.calls == [] and not hasattr(inf._ctx, "N")
    with pytest.raises(Handed):                                           # (a stationary kernel is still served there)
        inf.inference(gpy_amd.RBF(2), X, Z, gpy_amd.Gaussian(0.1), Y)
    # the grid mode names Linear as before
    from gpy_amd import grid as G
    with pytest.raises(NotImplementedError, match="Linear"):
        G.GridContext.exact_inference(object.__new__(G.GridContext), "linear", False, np.array([1.0]), 0.1)


@pytest.mark.parametrize("maxtries", [5, 2])
def test_the_jitter_ladder_starts_at_the_mean_of_kdiag_at_the_inducing_points(rec, monkeypatch, maxtries):
    """jitchol's first rung is mean(diag Kmm) * 1e-6 (reference util/linalg.py:65); Kmm = K(Z, Z), and Kdiag(Z) of a Linear part
    depends on Z"""
    monkeypatch.setattr(Recording, "fail", True)
    X, Z, Y = _data()
    k = gpy_amd.RBF(2, 1.3, 0.7) + gpy_amd.Linear(2, [0.4, 0.6], ARD=True)
    kd = 1.3 + float(np.mean(np.sum(np.array([0.4, 0.6]) * Z * Z, axis=1)))
    assert np.isclose(float(np.mean(k.jitter_diag(Z))), kd, rtol=1e-15)
    assert kd != k.diag_variance()
    for entry, run in _runs(k, X, Z, Y, linear=True, maxtries=maxtries):
        n0 = len(rec.made)
        with pytest.raises(np.linalg.LinAlgError, match="not positive definite, even with jitter"):
            run()
        j = rec.made[n0].jitters
        base = 1e-6 if entry == "pep" else 0.0                           # PEP's own constant rides on every rung (pep.py:17)
        assert len(j) == maxtries + 1 and j[0] == base
        assert np.isclose(j[1] - base, kd * 1e-6, rtol=1e-9, atol=0.0), (entry, j)
    # today's kernels: the same number as before
    k0 = gpy_amd.RBF(2, 2.0, 0.7) + gpy_amd.Bias(2, 0.5)
    assert k0.jitter_diag(Z) == k0.diag_variance() == 2.5


def test_the_binding_table_matches_the_header():
    text = open(os.path.join(HERE, "..", "include", "mi355gp_sparse_diag.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"\bint\s+(mi355gp_\w+)\s*\(([^;]*?)\)\s*;", text)
    assert [p[0] for p in protos] == list(_lib.SPARSE_DIAG_ABI) == ["mi355gp_sparse_set_linear", "mi355gp_sparse_kdiag"]
    assert [p.strip() for p in protos[0][1].split(",")] == ["mi355gp_sparse* s", "int on"]
    assert len(_lib.SPARSE_DIAG_ABI["mi355gp_sparse_set_linear"]) == 2
    params = [p.strip() for p in protos[1][1].split(",")]
    assert [p.rsplit(" ", 1)[1].lstrip("*") for p in params] == ["s", "nparts", "parts", "w", "kd_out", "sums_out", "ddiag_out"]
    assert len(_lib.SPARSE_DIAG_ABI["mi355gp_sparse_kdiag"]) == len(params)
    assert all(("double*" in p.replace(" *", "*")) for p in params[3:])
