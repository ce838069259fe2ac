"""CPU: the reference-side binding of the missing-data loop, `integration/gpy_mi355x.py make_missing_data_loop` (the object bound at
`GPy/models/sparse_gp_minibatch.py:228`), over a RECORDING library: every entry point it calls follows the signatures of
include/mi355gp.h / include/mi355gp_sparse_missing.h, records the call and answers from the float64 restatement
(tests/missing_ld.py).  Proves the glue -- grouping and its order, NaN -> 0 with the mask, what is uploaded when, the part list,
the M x M x Dy `woodbury_inv`, where the gradients are installed -- independently of the device code; the numbers are those of a
fixture made by the reference's own loop (tests/golden/missing)."""
import ctypes
import os
import sys
import types

import numpy as np

import missing_ld as ML
from test_oracle_missing import FIXTURES, check_against_fixture, fixture_problem

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "integration"))


def _arr(ptr, shape):
    return np.ctypeslib.as_array(ptr, shape=shape)


class RecordingLib(object):
    def __init__(self):
        self.calls, self.c = [], {}

    def mi355gp_last_error(self):
        return b"recording"

    def mi355gp_sparse_create(self, device, ref):
        ref._obj.value = 1
        self.calls.append("create")
        return 0

    def mi355gp_sparse_set_data(self, ctx, X, N, D, Y, Dy):
        assert X.shape == (N, D) and Y.shape == (N, Dy) and not np.isnan(Y).any()
        self.c = dict(mu=X.copy(), Y0=Y.copy())
        self.calls.append("set_data")
        return 0

    def mi355gp_sparse_set_input_variance(self, ctx, S, N, D):
        self.c["S"] = S.copy()
        self.calls.append("set_input_variance")
        return 0

    def mi355gp_sparse_set_inputs(self, ctx, X, S, N, D):
        self.c.update(mu=X.copy(), S=_arr(S, (N, D)).copy())
        self.calls.append("set_inputs")
        return 0

    def mi355gp_sparse_set_output_groups(self, ctx, G, gof, W):
        Dy, N = self.c["Y0"].shape[1], self.c["Y0"].shape[0]
        self.c.update(gof=np.array([gof[d] for d in range(Dy)]), W=_arr(W, (N, G)).copy())
        assert np.all(self.c["Y0"][self.c["W"][:, self.c["gof"]] == 0] == 0)       # 0 where unobserved
        self.calls.append("set_output_groups")
        return 0

    def mi355gp_vardtc_inference_missing(self, ctx, nparts, parts, Z, M, noise, noise_len, extra, out, dtheta, dZ, wv, dmu, dS, ms):
        import gpy_mi355x
        c = self.c
        arr = ctypes.cast(parts, ctypes.POINTER(gpy_mi355x._Part))
        N, Q = c["mu"].shape
        kinds = [arr[i].kind for i in range(nparts)]
        assert kinds[0] == gpy_mi355x.MI355GP_RBF and all(k == gpy_mi355x.MI355GP_WHITE for k in kinds[1:]) and noise_len == 1
        ard = bool(arr[0].ard)
        nl = Q if ard else 1
        var, ls = arr[0].theta[0], np.array([arr[0].theta[1 + i] for i in range(nl)])
        white = [arr[i].theta[0] for i in range(1, nparts)]
        Y = np.where(c["W"][:, c["gof"]] > 0, c["Y0"], np.nan)
        r = ML.evaluate(var, ls, ard, white, Z, c["mu"], c["S"], Y, noise[0], np.float64, kl=False)
        assert list(r["group_of_output"]) == list(c["gof"])
        out[:] = 0.0
        out[0], out[1], out[5] = r["lml"], r["dnoise"], 1.0 / noise[0]
        th = np.concatenate([np.ravel(r["dvar"]), np.ravel(r["dl"]), np.ravel(r["dwhite"])])
        _arr(dtheta, (th.size,))[:] = th
        _arr(dZ, (M, Q))[:] = r["dZ"]
        _arr(wv, r["woodbury_vector"].shape)[:] = r["woodbury_vector"]
        _arr(dmu, (N, Q))[:] = r["dmu"]
        _arr(dS, (N, Q))[:] = r["dS"]
        c.update(r=r, g=0, Z=Z.copy(), var=var, ls=ls, white=white)
        self.calls.append("inference_missing")
        return 0

    def mi355gp_sparse_select_output_group(self, ctx, g):
        self.c["g"] = g
        self.calls.append("select%d" % g)
        return 0

    def mi355gp_sparse_fetch(self, ctx, which, out):
        c, r = self.c, self.c["r"]
        Kmm = ML.P._rbf_K(c["var"], np.broadcast_to(c["ls"] ** 2, (c["Z"].shape[1],)), c["Z"]) + (sum(c["white"]) + 1e-8) * np.eye(c["Z"].shape[0])
        out[:] = {0: r["dL_dKmm"], 1: r["woodbury_inv"][c["g"]], 2: np.linalg.cholesky(Kmm), 3: Kmm}[which]
        self.calls.append("fetch%d" % which)
        return 0


class _P(object):
    def __init__(self, v):
        self.values, self.gradient = np.atleast_1d(np.asarray(v, float)), None

    def __array__(self, dtype=None, copy=None):
        return self.values


class RBF(object):
    def __init__(self, var, ls, ARD):
        self.variance, self.lengthscale, self.ARD = _P(var), _P(ls), ARD


class White(object):
    def __init__(self, var):
        self.variance = _P(var)


class Add(object):
    def __init__(self, parts):
        self.parts = parts


def _model(p):
    lik = types.SimpleNamespace(gaussian_variance=lambda md=None: np.array([p["noise"]]), grad=None)
    lik.update_gradients = lambda g: setattr(lik, "grad", g)
    rbf = RBF(p["var"], p["ls"], p["ARD"])
    m = types.SimpleNamespace(kern=rbf if not p["white"] else Add([rbf] + [White(w) for w in p["white"]]),
                              X=types.SimpleNamespace(mean=_P(p["mu"]), variance=_P(p["S"])), Z=_P(p["Z"]), likelihood=lik,
                              Y_normalized=p["Y"], Y_metadata=None)
    m.X.mean.values, m.X.variance.values, m.Z.values = p["mu"], p["S"], p["Z"]
    return m


def _loop(L):
    import gpy_mi355x
    post = lambda **kw: types.SimpleNamespace(**kw)
    loop = gpy_mi355x.make_missing_data_loop(L, gpy=types.SimpleNamespace(Posterior=post), bind=False)
    return loop


def test_the_bound_loop_meets_the_references_loop_and_installs_the_gradients():
    g = np.load([f for f in FIXTURES if "white_dy12" in f][0])
    p = fixture_problem(g)
    L = RecordingLib()
    loop, m = _loop(L), _model(p)
    m._outer_values_update = lambda fv: loop.outer_values_update(m, fv)
    loop.outer_loop(m)
    G = g["W"].shape[1]
    assert L.calls[:5] == ["create", "set_data", "set_input_variance", "set_output_groups", "inference_missing"]
    assert [c for c in L.calls if c.startswith("select")] == ["select%d" % k for k in range(G)]
    assert np.array_equal(loop.group_of_output, g["group_of_output"]) and np.array_equal(loop.W, g["W"])
    fv, post = m.full_values, m.posterior
    assert sorted(fv) == ["dL_dKmm", "dL_dpsi0", "dL_dpsi1", "dL_dthetaL", "fused"]
    rbf, white = m.kern.parts
    check_against_fixture(dict(lml=m._log_marginal_likelihood, woodbury_vector=post.woodbury_vector, woodbury_inv=post.woodbury_inv,
                               dL_dKmm=fv["dL_dKmm"], dL_dpsi0=fv["dL_dpsi0"], dnoise=np.ravel(m.likelihood.grad),
                               dtheta=np.concatenate([rbf.variance.gradient, rbf.lengthscale.gradient, white.variance.gradient]),
                               dZ=m.Z.gradient, dmu=m.X.mean.gradient, dS=m.X.variance.gradient), g)
    assert post.woodbury_inv.shape == (16, 16, 12) and post.K.shape == post.K_chol.shape == (16, 16)
    r = ML.evaluate(p["var"], p["ls"], p["ARD"], p["white"], p["Z"], p["mu"], p["S"], p["Y"], p["noise"], kl=False)
    assert np.allclose(fv["dL_dpsi1"], np.asarray(r["dL_dpsi1"], float), rtol=1e-10, atol=1e-12)


def test_what_is_uploaded_when():
    g = np.load(FIXTURES[0])
    p = fixture_problem(g)
    L = RecordingLib()
    loop, m = _loop(L), _model(p)
    m._outer_values_update = lambda fv: None
    loop.outer_loop(m)
    n0 = len(L.calls)
    m.X.mean.values = p["mu"] + 0.01                                   # a step of q(X): 2 N Q doubles, Y and the groups stay
    loop.outer_loop(m)
    assert L.calls[n0] == "set_inputs" and "set_data" not in L.calls[n0:] and "set_output_groups" not in L.calls[n0:]
    n1 = len(L.calls)
    Y = p["Y"].copy()                                                  # an observed exact 0.0 against a NaN: the same zero-filled Y,
    i = tuple(np.argwhere(~np.isnan(Y))[3])                            # another mask -- everything is uploaded again
    Y[i] = 0.0
    m.Y_normalized = Y
    loop.outer_loop(m)
    assert "set_data" in L.calls[n1:]
    n2 = len(L.calls)
    Y2 = Y.copy()
    Y2[i] = np.nan
    m.Y_normalized = Y2
    loop.outer_loop(m)
    assert L.calls[n2:n2 + 3] == ["set_data", "set_input_variance", "set_output_groups"]


def test_other_kernels_are_refused_before_the_library_is_touched():
    import pytest
    g = np.load(FIXTURES[0])
    p = fixture_problem(g)

    class Matern52(RBF):
        pass
    L = RecordingLib()
    loop, m = _loop(L), _model(p)
    m.kern = Add([m.kern, Matern52(1.0, 1.0, False)])
    with pytest.raises(NotImplementedError, match="Matern52"):
        loop.outer_loop(m)
    assert not L.calls
