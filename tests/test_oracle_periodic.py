"""CPU: the NumPy restatement of RatQuad / StdPeriodic (periodic_np.py) against the fixtures made from the reference's own
code (tests/golden/periodic) and against central differences; the host classes' bookkeeping (constructor checks, link
order, to_dict / from_dict, part lists) and the sparse path's refusal of the two kinds, none of which needs a GPU."""
import glob
import os

import numpy as np
import pytest

import gpy_amd
from gpy_amd import _lib as L

import periodic_np as P

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(HERE, "golden", "periodic", "*.npz")))


def _load(name):
    z = np.load(os.path.join(HERE, "golden", "periodic", name + ".npz"))
    g = {k: z[k] for k in z.files}
    g["specs"] = P.load_specs(g["specs"])
    g["nu"] = None if float(g["nu"]) < 0 else float(g["nu"])
    rng = np.random.default_rng(1000 + int(g["gseed"]))
    g["G"] = rng.standard_normal((g["X"].shape[0],) * 2)
    g["G2"] = rng.standard_normal((g["X"].shape[0], g["Xs"].shape[0]))
    return g


def test_fixtures_present():
    assert len(NAMES) == 9


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_the_reference(name):
    g = _load(name)
    # the calendar-year case: the reference's RBF uses the expanded square (~1e-11 relative at x ~ 2000)
    f = 1e4 if name.startswith("maunaloa") else 1.0
    lml, alpha, dth, dn = P.exact(g["specs"], g["X"], g["Y"], float(g["noise"]), g["nu"])
    assert abs(lml - g["lml"]) <= f * 1e-10 * abs(g["lml"])
    assert np.linalg.norm(alpha - g["alpha"]) <= f * 1e-9 * np.linalg.norm(g["alpha"])
    assert np.abs(dth - g["dtheta"]).max() <= f * 1e-8 * np.abs(g["dtheta"]).max()
    if dn is not None:
        assert abs(dn - g["dnoise"]) <= f * 1e-8 * abs(g["dnoise"])
    K = P.expr(g["specs"], g["X"])[0]
    assert np.abs(K[0] - g["K_row0"]).max() <= f * 1e-13 * max(s[2][0] for s in g["specs"])
    for gx, ref in ((P.gradients_X(g["specs"], g["G"], g["X"]), g["gradX"]),
                    (P.gradients_X(g["specs"], g["G2"], g["X"], g["Xs"]), g["gradX2"])):
        assert np.abs(gx - ref).max() <= f * 1e-10 * np.abs(ref).max()


SPECS = [
    [("ratquad", 1, np.array([0.9, 0.7, 1.4, 2.5]), np.array([0, 2]), 0)],
    [("stdperiodic", 3, np.array([1.2, 1.3, 2.1, 0.8, 0.7, 1.2, 1.9]), np.array([0, 1, 2]), 0)],
    [("rbf", 0, np.array([1.2, 1.5]), np.array([0]), 1), ("stdperiodic", 1, np.array([0.8, 0.7, 1.1]), np.array([1]), 1),
     ("ratquad", 0, np.array([0.4, 1.1, 0.9]), np.array([0, 1, 2]), 0)],
]


@pytest.mark.parametrize("i", range(len(SPECS)))
def test_dK_dtheta_and_dK_dx_against_central_differences(i):
    specs = SPECS[i]
    rng = np.random.default_rng(i)
    X, X2 = rng.standard_normal((7, 3)), rng.standard_normal((5, 3))
    K, dK, dX = P.expr(specs, X, X2)
    h = 1e-6
    k = 0
    for s, (kind, ard, th, dims, term) in enumerate(specs):
        for j in range(th.size):
            up = [list(t) for t in specs]
            dn = [list(t) for t in specs]
            up[s][2] = th.copy()
            up[s][2][j] += h
            dn[s][2] = th.copy()
            dn[s][2][j] -= h
            fd = (P.expr(up, X, X2)[0] - P.expr(dn, X, X2)[0]) / (2 * h)
            assert np.abs(dK[k] - fd).max() <= 1e-7 * max(1.0, np.abs(fd).max()), (s, j)
            k += 1
    assert k == len(dK)
    for q in range(3):
        e = np.zeros(3)
        e[q] = h
        fd = (P.expr(specs, X + e, X2)[0] - P.expr(specs, X - e, X2)[0]) / (2 * h)
        assert np.abs(dX[..., q] - fd).max() <= 1e-7 * max(1.0, np.abs(fd).max())


def _names(k):
    out = []
    for n in k.parameter_names():
        n = n.split("[")[0]
        if n not in out:
            out.append(n)
    return out


def test_host_classes_link_order_and_theta():
    r = gpy_amd.RatQuad(2, variance=1.3, lengthscale=[0.7, 1.1], power=2.5, ARD=True)
    assert _names(r) == ["variance", "lengthscale", "power"]
    assert np.array_equal(r._theta(), [1.3, 0.7, 1.1, 2.5])
    p = gpy_amd.StdPeriodic(3, variance=0.9, period=[1.0, 2.0, 3.0], lengthscale=0.5, ARD1=True)
    assert _names(p) == ["variance", "period", "lengthscale"]
    assert np.array_equal(p._theta(), [0.9, 1.0, 2.0, 3.0, 0.5]) and p.ARD == 1
    assert gpy_amd.StdPeriodic(2, ARD2=True).ARD == 2
    assert L.KIND_IDS["ratquad"] == 6 and L.KIND_IDS["stdperiodic"] == 7
    assert L.ard_id("stdperiodic", 3) == 3 and L.ard_id("ratquad", True) == 1
    with pytest.raises(AssertionError, match="bad number of periods"):
        gpy_amd.StdPeriodic(3, period=[1.0, 2.0], ARD1=True)
    with pytest.raises(AssertionError, match="Only one lengthscale needed"):
        gpy_amd.StdPeriodic(2, lengthscale=[1.0, 2.0])


def test_to_dict_round_trip_and_part_specs():
    p = gpy_amd.StdPeriodic(1, 1.1, 1.0, 1.2, active_dims=[1])
    d = p.to_dict()
    assert d["class"] == "GPy.kern.StdPeriodic" and d["ARD1"] is False
    q = gpy_amd.StdPeriodic.from_dict(d)
    assert type(q) is gpy_amd.StdPeriodic and np.array_equal(q._theta(), p._theta())
    r = gpy_amd.RatQuad(1, 0.5, 2.0, 0.7)
    assert r.to_dict()["class"] == "GPy.kern.RatQuad" and gpy_amd.RatQuad.from_dict(r.to_dict())._theta()[-1] == 0.7
    k = gpy_amd.RBF(1, active_dims=[0]) * p + r
    specs = k.part_specs()
    assert [(s[0], s[4]) for s in specs] == [("rbf", 1), ("stdperiodic", 1), ("ratquad", 0)]
    assert k.diag_variance() == pytest.approx(1.0 * 1.1 + 0.5)
    p.update_gradients_diag(np.ones(4), None)
    assert p.variance.gradient == 4.0 and p.period.gradient == 0.0


def test_sparse_path_rejects_the_new_kinds_before_device_work():
    X = np.random.default_rng(0).standard_normal((32, 1))
    with pytest.raises(NotImplementedError, match="StdPeriodic"):
        gpy_amd.VarDTC().inference(gpy_amd.StdPeriodic(1), X, X[:4], gpy_amd.Gaussian(), np.sin(X))
    with pytest.raises(NotImplementedError, match="RatQuad"):
        gpy_amd.VarDTC().inference(gpy_amd.RatQuad(1) + gpy_amd.RBF(1), X, X[:4], gpy_amd.Gaussian(), np.sin(X))
