"""No GPU: the binding table of include/mi355gp_kgpr.h, the export of the model under GPy's names, what
`GPKroneckerGaussianRegression` refuses before any device work, and the float64 restatement tests/kgpr_ld.py against fixtures of the
reference's OWN model (tools/make_golden_kgpr.py -> tests/golden/kgpr)."""
import os
import re

import numpy as np
import pytest

import gpy_amd
from gpy_amd import _lib, kgpr

import kgpr_ld as KL

HERE = os.path.dirname(os.path.abspath(__file__))


def test_the_binding_table_is_the_header():
    text = open(os.path.join(HERE, "..", "include", "mi355gp_kgpr.h")).read()
    protos = re.findall(r"\bint\s+(mi355gp_\w+)\s*\(([^;]*?)\)\s*;", text)
    assert [p[0] for p in protos] == list(_lib.KGPR_ABI)
    assert [p[0][len("mi355gp_kgpr_"):] for p in protos] == ["create", "destroy", "set_data", "inference", "predict", "fetch", "get_ms", "wsyrk"]
    for name, params in protos:
        params = [p.strip() for p in params.split(",")]
        assert len(_lib.KGPR_ABI[name]) == len(params), name
        for p, t in zip(params, _lib.KGPR_ABI[name]):            # integers by value where the header has them by value
            assert (t in (_lib._ci, _lib._i64, _lib._cd)) == ("*" not in p), (name, p)
            if "*" not in p:
                assert t is {"int": _lib._ci, "int64_t": _lib._i64, "double": _lib._cd}[p.split()[0]], (name, p)
    assert int(re.search(r"#define MI355GP_KGPR_NUM_MS (\d+)", text).group(1)) == _lib.KGPR_NUM_MS == len(_lib.KgprContext.MS_NAMES)
    for i, n in enumerate(("U1", "S1", "U2", "S2", "YTILDE", "WI")):
        assert int(re.search(r"#define MI355GP_KGPR_FETCH_%s (\d+)" % n, text).group(1)) == i == getattr(_lib.KgprContext, "FETCH_" + n)


def test_exported_under_gpys_names():
    assert gpy_amd.models.GPKroneckerGaussianRegression is gpy_amd.GPKroneckerGaussianRegression is kgpr.GPKroneckerGaussianRegression
    assert "GPKroneckerGaussianRegression" in gpy_amd.__all__
    names = [f.__name__ for f in (kgpr.GPKroneckerGaussianRegression.optimize, kgpr.GPKroneckerGaussianRegression.checkgrad)]
    assert names == ["optimize", "checkgrad"] and gpy_amd.GP.optimize is kgpr.GPKroneckerGaussianRegression.optimize


class _NoGradients(object):
    input_dim = 1


@pytest.mark.parametrize("shapes, kw, what", [
    (((5, 1), (4, 1), (5, 3)), {}, "Y must be N1 x N2 = 5 x 4"),
    (((5, 2), (4, 1), (5, 4)), {}, "kern1.input_dim is 1, X1 has 2 columns"),
    (((5, 1), (4, 3), (5, 4)), {}, "kern2.input_dim is 1, X2 has 3 columns"),
    (((5, 1), (4, 1), (5, 4)), {"nan": True}, "not finite"),
    (((5, 1), (4, 1), (5, 4)), {"noise_var": 0.0}, "noise variance must be positive"),
    (((5, 1), (4, 1), (5, 4)), {"noise_var": -1.0}, "noise variance must be positive"),
    (((5, 1), (4, 1), (5, 4)), {"kern2": _NoGradients()}, "kern2 .* has no update_gradients_full"),
])
def test_refused_by_name_before_any_device_work(monkeypatch, shapes, kw, what):
    monkeypatch.setattr(_lib, "KgprContext", lambda *a, **k: pytest.fail("the device was reached"))
    monkeypatch.setattr(_lib, "kern_K", lambda *a, **k: pytest.fail("the device was reached"))
    kw = dict(kw)
    X1, X2, Y = (np.ones(s) for s in shapes)
    if kw.pop("nan", False):
        Y[2, 1] = np.nan
    k2 = kw.pop("kern2", None) or gpy_amd.Matern32(1)
    with pytest.raises((ValueError, NotImplementedError), match=what):
        gpy_amd.GPKroneckerGaussianRegression(X1, X2, Y, gpy_amd.RBF(1), k2, **kw)


@pytest.mark.parametrize("name", ["kgpr_12x9", "kgpr_30x5", "kgpr_5x30"])
def test_the_restatement_meets_the_references_own_model(name):
    """Same algorithm and the same LAPACK as the reference, summation order apart, at a condition of about 1e4: 1e-10 of max |value|."""
    g = np.load(os.path.join(HERE, "golden", "kgpr", name + ".npz"))
    X1, X2 = g["X1"], g["X2"]
    (K1, dv1, dl1), (K2, dv2, dl2) = KL.rbf(X1, g["var1"], g["ls1"]), KL.matern32(X2, g["var2"], g["ls2"])
    r = KL.restate(K1, K2, g["Y"], float(g["noise"]))
    grad = [np.sum(r["dK1"] * dv1), np.sum(r["dK1"] * dl1), np.sum(r["dK2"] * dv2), np.sum(r["dK2"] * dl2), r["dsig"]]
    mu, var = KL.restate_predict(r, KL.rbf(g["X1new"], g["var1"], g["ls1"], X1)[0], KL.matern32(g["X2new"], g["var2"], g["ls2"], X2)[0],
                                 np.full(len(g["X1new"]), g["var1"]), np.full(len(g["X2new"]), g["var2"]))
    for what, got, ref in (("lml", r["lml"], g["lml"]), ("grad", grad, g["grad"]), ("mu", mu[:, None], g["mu"]), ("var", var[:, None], g["var"])):
        e = KL.rel(got, ref)
        print("%s %s: %.3e" % (name, what, e))
        assert e <= 1e-10, (what, e)
