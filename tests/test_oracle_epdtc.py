"""CPU: EPDTC without a device.

The restatement tests/epdtc_np.py against every fixture of tests/golden/epdtc (the reference's own `EPDTC`, recorded orders) at
the standing tolerances of tests/ep_np.py (scalars 1e-10, vectors 1e-9, gradients 1e-8, prediction 1e-9); measured, worst over
the eight fixtures: sites 7.4e-14, log marginal 2.2e-15, gradients 1.1e-13, Woodbury vector 3.0e-14, prediction 2.2e-14.

The blocked sweep against the refactoring one in long double at b in {1, 2, 64, 128} with N on both sides of a multiple of b:
the two are the same map, so they differ by rounding alone; in float64 they differ by at most 5.7e-12 (below), long double's
unit roundoff is 4.9e-4 of float64's, which gives 2.8e-15; held to 1e-14.

The float64 restatement's own distance from long double over the shape cases the device is held at (epdtc_np.SHAPES), worst
over the refactoring and the blocked sweep, relative to max |value|: tau 5.62e-12, v 9.40e-15, cav_tau 3.11e-15, cav_v 1.38e-14,
log Z_hat 3.42e-15, mu_hat 5.10e-15, sigma2_hat 4.72e-15, recompute's mu 7.11e-16 and Sigma_diag 1.40e-15.  Ten times these
figures (epdtc_np.DEVICE_BOUND) is the device's bound in tests/test_gpu_epdtc.py.

Then: central differences of the converged bound, `EPDTC.inference` and `SparseGPClassification` end to end over a stand-in
context that answers with the restatement (the pattern of tests/test_svgp_host.py), every refusal by name, `to_dict`, and the
binding table `_lib.EPDTC_ABI` against the prototypes of include/mi355gp_epdtc.h."""
import os

import numpy as np
import pytest

import epdtc_np as E
import gpy_amd
import kern_ld as KL
import svgp_np as S
from conftest import ROOT
from gpy_amd import _lib
from gpy_amd.epdtc import EPDTC
from test_abi import _prototypes, _type_class

LD = np.longdouble
STANDING = {"lml": 1e-10, "log_Z_tilde": 1e-10, "tau_tilde": 1e-9, "v_tilde": 1e-9, "cav_tau": 1e-9, "cav_v": 1e-9, "dtheta": 1e-8,
            "dZ": 1e-8, "woodbury_vector": 1e-9, "pred_mu": 1e-9, "pred_var": 1e-9}


def _figures(got, fx, keys):
    fig = {q: (abs(got[q] - fx[q]) / abs(fx[q]) if q in ("lml", "log_Z_tilde") else E.rel(got[q], fx[q])) for q in keys}
    print({q: "%.1e" % v for q, v in fig.items()})
    return fig


def test_there_are_the_eight_fixtures_and_the_toy_problem():
    assert len(E.FIXTURES) == 8 and os.path.exists(os.path.join(E.GOLDEN, "toy_1d_optimize.npz"))
    fx = [E.load(n) for n in E.FIXTURES]
    assert sum(f["parallel_updates"] for f in fx) == 1 and sum(f["eta"] != 1.0 for f in fx) == 1 and sum("warm_tau" in f for f in fx) == 1
    assert all(float(f["cond_Kmm"]) < 1e6 and not f["clamped"] for f in fx)


@pytest.mark.parametrize("name", E.FIXTURES)
@pytest.mark.parametrize("sweep", ["refactoring", "blocked"])
def test_restatement_matches_the_reference(name, sweep):
    fx = E.load(name)
    r = E.restate_fixture(fx) if sweep == "refactoring" else E.restate_fixture(fx, sweep=E.blocked_sweep, b=E.B)
    assert r["sweeps"] == fx["sweeps"]
    for q, e in _figures(r, fx, STANDING).items():
        assert e <= STANDING[q], (q, e)


@pytest.mark.parametrize("b,N", [(1, 3), (2, 5), (2, 6), (64, 63), (64, 64), (64, 65), (64, 129), (128, 127), (128, 128), (128, 129)])
def test_blocked_sweep_is_the_refactoring_sweep_in_long_double(b, N):
    KL.require_ld()
    rng = np.random.default_rng(100 * b + N)
    M = 9
    X, Z = rng.uniform(0, 1, (N, 2)), rng.uniform(0, 1, (M, 2))
    specs = [("rbf", 0, np.array([1.4, 0.35]), np.arange(2), 0)]
    sign = np.where(np.sin(6 * X[:, 0]) + 0.3 * rng.standard_normal(N) > 0, 1.0, -1.0)
    Kmm, Kmn = E.covariances(specs, X, Z, LD)
    tau, v = np.zeros(N), np.zeros(N)
    for it in range(2):                                     # a cold sweep (first site + 1e-8), then one from its sites
        order = rng.permutation(N)
        a = E.ref_sweep(Kmm, Kmn, order, sign, 0.9, 0.8, tau, v, it == 0, LD)
        g = E.blocked_sweep(Kmm, Kmn, order, sign, 0.9, 0.8, tau, v, it == 0, b, LD)
        for k in E.SWEEP_KEYS:
            assert E.rel(g[k], a[k]) <= 1e-14, (it, k, E.rel(g[k], a[k]))
        tau, v = a["tau"], a["v"]


def test_float64_restatement_against_long_double_over_the_device_shapes():
    """the measurement behind epdtc_np.DEVICE_BOUND (figures in the module docstring)"""
    KL.require_ld()
    worst = dict.fromkeys(E.FP64_DISTANCE, 0.0)
    names = [s[0] for s in E.SHAPES]
    assert {s[1] for s in E.SHAPES} >= {1, E.B - 1, E.B, E.B + 1, 2 * E.B + 1} and {s[2] for s in E.SHAPES} >= {1, 63, 65, 129, 257}
    assert {s[3] for s in E.SHAPES} >= {1, 17, 33}
    for name in names:
        c, ref = E.reference(name)
        Kmm, Kmn = E.covariances(c["specs"], c["X"], c["Z"], np.float64)
        a = (c["order"], c["sign"], c["eta"], c["delta"], c["tau"], c["v"], True)
        for r in (E.blocked_sweep(Kmm, Kmn, *a, E.B, np.float64), E.ref_sweep(Kmm, Kmn, *a, np.float64)):
            for k in E.SWEEP_KEYS:
                worst[k] = max(worst[k], E.rel(r[k], ref[k]))
        mu, sd = E.recompute(Kmm, Kmn, c["tau"], c["v"], np.float64)
        worst["mu"], worst["Sigma_diag"] = max(worst["mu"], E.rel(mu, ref["mu"])), max(worst["Sigma_diag"], E.rel(sd, ref["Sigma_diag"]))
    print({k: "%.2e" % v for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= E.FP64_DISTANCE[k], (k, v)
    others = max(v for k, v in E.DEVICE_BOUND.items() if k != "tau")
    assert E.DEVICE_BOUND["tau"] <= 100 * 10 * others          # no case needs a bound more than 100 times the others'


def test_central_differences_of_the_converged_bound():
    """sites fixed ("alternated"): d bound / d (kernel parameters, Z) of the final evaluation against central differences"""
    fx = E.load("rbf_white_n130_m16_d2")
    tau, v, lzt = fx["tau_tilde"], fx["v_tilde"], float(fx["log_Z_tilde"])
    r = E.final(fx["specs"], fx["X"], fx["Z"], tau, v, lzt, np.float64)
    h = 1e-6

    def bound(specs, Z):
        return float(E.final(specs, fx["X"], Z, tau, v, lzt, np.float64)["lml"])
    k = 0
    for i, s in enumerate(fx["specs"]):
        for j in range(len(s[2])):
            def at(d):
                th = s[2].copy()
                th[j] += d
                return bound(fx["specs"][:i] + [(s[0], s[1], th, s[3], s[4])] + fx["specs"][i + 1:], fx["Z"])
            fd = (at(h) - at(-h)) / (2 * h)
            assert abs(fd - r["dtheta"][k]) <= 1e-6 * max(1.0, abs(fd)), (i, j, fd, r["dtheta"][k])
            k += 1
    for (a, q) in ((0, 0), (7, 1), (15, 0)):
        Zp, Zm = fx["Z"].copy(), fx["Z"].copy()
        Zp[a, q] += h
        Zm[a, q] -= h
        fd = (bound(fx["specs"], Zp) - bound(fx["specs"], Zm)) / (2 * h)
        assert abs(fd - r["dZ"][a, q]) <= 1e-6 * max(1.0, abs(fd)), (a, q, fd, r["dZ"][a, q])


# ---- the host classes over a stand-in context ----------------------------------------------------------------------------------
@pytest.fixture
def rctx(monkeypatch):
    made = []

    class Ctx(E.RestatementContext):
        def __init__(self, device=0):
            super(Ctx, self).__init__(device)
            made.append(self)
    monkeypatch.setattr(_lib, "SparseContext", Ctx)
    return made


def _replay(monkeypatch, orders):
    """np.random.permutation answers with the recorded orders, in turn"""
    it = iter([np.asarray(o) for o in orders])
    monkeypatch.setattr(np.random, "permutation", lambda n: next(it))


@pytest.mark.parametrize("name", ["rbf_iso_n150_m16_d2", "parallel_rbf_iso_n150_m16_d2", "fractional_rbf_iso_n150_m16_d2",
                                  "rbf_x_matern32_n140_m20_d2"])
def test_inference_follows_the_reference_over_the_stand_in(rctx, monkeypatch, name):
    fx = E.load(name)
    _replay(monkeypatch, fx["orders"])
    inf = EPDTC(eta=fx["eta"], delta=fx["delta"], parallel_updates=fx["parallel_updates"], max_iters=100)
    kern = S.make_kernel(fx)
    post, lml, gd = inf.inference(kern, fx["X"], fx["Z"], gpy_amd.Bernoulli(), fx["Y"])
    assert inf.iterations == fx["sweeps"]
    _, ga, lzt = inf._ep_approximation
    mu, var = post._raw_predict(kern, fx["Xs"], fx["Z"])
    got = dict(lml=lml, log_Z_tilde=lzt, tau_tilde=ga.tau, v_tilde=ga.v, cav_tau=inf._cav_params.tau, cav_v=inf._cav_params.v,
               dtheta=gd["fused"]["dtheta"], dZ=gd["fused"]["dZ"], woodbury_vector=post.woodbury_vector, pred_mu=mu, pred_var=var)
    for q, e in _figures(got, fx, STANDING).items():
        assert e <= STANDING[q], (q, e)
    ctx = rctx[0]
    calls = [c[0] for c in ctx.log]
    assert calls[:3] == ["set_data", "epdtc_begin", "epdtc_recompute"] and calls[-2:] == ["epdtc_inference", "predict"]
    assert ctx.log[0][1:] == (fx["X"].shape, fx["Y"].shape) and ctx.jitters == [0.0]
    sweeps = [c for c in ctx.log if c[0] == "epdtc_sweep"]
    if fx["parallel_updates"]:
        assert not sweeps
    else:
        assert [c[1] for c in sweeps] == [True] + [False] * (fx["sweeps"] - 1)      # only the run's first site sees the 1e-8
        assert all(np.array_equal(c[2], o) for c, o in zip(sweeps, fx["orders"]))
    assert set(gd) == {"dL_dKmm", "dL_dKdiag", "dL_dKnm", "dL_dthetaL", "dL_dm", "fused"}
    assert np.array_equal(gd["dL_dKdiag"], -0.5 * ga.tau) and np.size(gd["dL_dthetaL"]) == 0
    assert E.rel(np.asarray(gd["dL_dKmm"]), fx["dL_dKmm"]) <= 1e-8 and np.asarray(gd["dL_dKnm"]).shape == (fx["X"].shape[0], fx["Z"].shape[0])
    assert E.rel(np.asarray(post.woodbury_inv), fx["woodbury_inv"]) <= 1e-8
    # "alternated": a second call keeps the sites (no sweep), "nested" runs EP again
    n = len(ctx.log)
    inf.inference(kern, fx["X"], fx["Z"], gpy_amd.Bernoulli(), fx["Y"])
    assert [c[0] for c in ctx.log[n:]] == ["epdtc_begin", "epdtc_inference"]


def test_warm_start_across_a_change_of_kernel_parameters(rctx, monkeypatch):
    fx = E.load("warm_rbf_iso_n150_m16_d2")
    _replay(monkeypatch, list(fx["warm_orders"]) + list(fx["orders"]))
    inf = EPDTC(max_iters=100)
    warm = dict(fx, specs=fx["warm_specs"])
    inf.inference(S.make_kernel(warm), fx["X"], fx["Z"], gpy_amd.Bernoulli(), fx["Y"])
    assert E.rel(inf.ga_approx_old.tau, fx["warm_tau"]) <= 1e-9 and E.rel(inf.ga_approx_old.v, fx["warm_v"]) <= 1e-9
    inf.on_optimization_start()                                   # forgets the approximation, keeps ga_approx_old
    assert inf._ep_approximation is None and inf.ga_approx_old is not None
    post, lml, gd = inf.inference(S.make_kernel(fx), fx["X"], fx["Z"], gpy_amd.Bernoulli(), fx["Y"])
    assert inf.iterations == fx["sweeps"]
    got = dict(lml=lml, tau_tilde=inf._ep_approximation[1].tau, v_tilde=inf._ep_approximation[1].v, dtheta=gd["fused"]["dtheta"])
    for q, e in _figures(got, fx, got).items():
        assert e <= STANDING[q], (q, e)
    sweeps = [c[1] for c in rctx[0].log if c[0] == "epdtc_sweep"]
    assert sweeps.count(True) == 2                                # the first site of EACH run sees the 1e-8
    inf.reset()
    assert inf.ga_approx_old is None and inf._ep_approximation is None


def test_the_jitter_ladder_runs_on_the_begin_call(rctx, monkeypatch):
    fx = E.load("rbf_iso_n150_m16_d2")
    monkeypatch.setattr(E.RestatementContext, "fail_begin", 3)
    monkeypatch.setattr(E.RestatementContext, "epdtc_inference",
                        lambda self, specs, Z, tau, v, jitter=0.0, want_stage_ms=False: (self.jitters.append(("inference", jitter)), (1, {}))[1])
    inf = EPDTC(max_iters=2)
    with pytest.raises(np.linalg.LinAlgError):
        inf.inference(S.make_kernel(fx), fx["X"], fx["Z"], gpy_amd.Bernoulli(), fx["Y"])
    j = 1.5 * 1e-6                                                 # mean(diag K) * 1e-6, util/linalg.py:64
    assert rctx[0].jitters[:2] == [0.0, pytest.approx(j)] and rctx[0].jitters[-1] == ("inference", pytest.approx(j))


def test_model_defaults_gradient_and_prediction(rctx, monkeypatch):
    fx = E.load("rbf_iso_n150_m16_d2")
    np.random.seed(3)
    m = gpy_amd.SparseGPClassification(fx["X"], fx["Y"], num_inducing=7)
    assert isinstance(m.inference_method, EPDTC) and isinstance(m.kern, gpy_amd.RBF) and isinstance(m.likelihood, gpy_amd.Bernoulli)
    assert m.Z.shape == (7, 2) and all(any(np.array_equal(z, x) for x in fx["X"]) for z in m.Z.values)
    assert gpy_amd.models.SparseGPClassification is gpy_amd.SparseGPClassification
    assert [p.name for p in m.flattened_parameters()] == ["inducing inputs", "variance", "lengthscale"]
    m = gpy_amd.SparseGPClassification(fx["X"], fx["Y"], kernel=S.make_kernel(fx), Z=fx["Z"])
    # sites fixed ("alternated"): the model's gradient is that of its own bound
    x0, g0 = m.param_array.copy(), m.gradient.copy()
    for i in (0, 5, x0.size - 2, x0.size - 1):
        xp, xm = x0.copy(), x0.copy()
        xp[i] += 1e-6
        xm[i] -= 1e-6
        m.param_array = xp
        fp = m.log_likelihood()
        m.param_array = xm
        fd = (fp - m.log_likelihood()) / 2e-6
        assert abs(fd - g0[i]) <= 1e-6 * max(1.0, abs(fd)), (i, fd, g0[i])
    m.param_array = x0
    assert m.checkgrad()
    p, _ = m.predict(fx["Xs"])
    mu, var = m.predict_noiseless(fx["Xs"])
    assert p.shape == (13, 1) and np.all((p > 0) & (p < 1)) and mu.shape == (13, 1) and var.shape == (13, 1)
    assert m.posterior_samples_f(fx["Xs"], size=3).shape[0] == 13
    d = m.to_dict()
    assert d["class"] == "GPy.models.SparseGPClassification" and d["inference_method"]["class"].endswith("expectation_propagation.EPDTC")


def test_optimize_calls_the_hooks_and_improves_the_bound(rctx):
    z = np.load(os.path.join(E.GOLDEN, "toy_1d_optimize.npz"))
    m = gpy_amd.SparseGPClassification(z["X"], z["Y"], kernel=gpy_amd.RBF(1, variance=z["theta0"][0], lengthscale=z["theta0"][1]), Z=z["Z0"])
    start = m.log_likelihood()
    sweeps = lambda: sum(c[0] == "epdtc_sweep" for c in rctx[0].log)
    n0 = sweeps()
    m.optimize(max_iters=5)
    assert sweeps() > n0 and m.log_likelihood() > start          # on_optimization_start forgot the sites: EP ran again, once


# ---- refusals, to_dict, the binding table -----------------------------------------------------------------------------------------
def test_every_refusal_by_name_before_any_device_work(rctx):
    fx = E.load("rbf_iso_n150_m16_d2")
    X, Y, Z, k, lik = fx["X"], fx["Y"], fx["Z"], S.make_kernel(fx), gpy_amd.Bernoulli()
    inf = EPDTC()

    class Mean(object):
        def f(self, X):
            return np.zeros((X.shape[0], 1))
    with pytest.raises(NotImplementedError, match="mean function"):
        inf.inference(k, X, Z, lik, Y, mean_function=Mean())
    with pytest.raises(NotImplementedError, match="one output column"):
        inf.inference(k, X, Z, lik, np.hstack([Y, Y]))
    with pytest.raises(NotImplementedError, match="Bernoulli likelihood only, not Gaussian"):
        inf.inference(k, X, Z, gpy_amd.Gaussian(), Y)
    from gpy_amd.link_functions import Log
    with pytest.raises(NotImplementedError, match="probit link only, not Log"):
        inf.inference(k, X, Z, gpy_amd.Bernoulli(Log()), Y)
    with pytest.raises(NotImplementedError, match="NormalPosterior"):
        inf.inference(k, gpy_amd.NormalPosterior(X, np.full(X.shape, 0.1)), Z, lik, Y)
    for arg in ("Lm", "dL_dKmm", "psi0", "psi1", "psi2"):
        with pytest.raises(NotImplementedError, match="precomputed statistics"):
            inf.inference(k, X, Z, lik, Y, **{arg: np.eye(2)})
    with pytest.raises(NotImplementedError, match="sparse path"):
        inf.inference(gpy_amd.Linear(2), X, Z, lik, Y)
    with pytest.raises(ValueError, match="ep_mode"):
        EPDTC(ep_mode="other").inference(k, X, Z, lik, Y)
    assert not rctx                                               # no context was even made
    sharded = EPDTC()
    sharded._ctx = E.RestatementContext()
    sharded._ctx.sharded = True
    with pytest.raises(NotImplementedError, match="row-sharded"):
        sharded.inference(k, X, Z, lik, Y)
    assert sharded._ctx.log == []
    with pytest.raises(NotImplementedError, match="mean function"):
        gpy_amd.SparseGPClassification(X, Y, mean_function=Mean())
    with pytest.raises(NotImplementedError, match="SparseGPClassificationUncertainInput"):
        gpy_amd.SparseGPClassification(gpy_amd.NormalPosterior(X, np.full(X.shape, 0.1)), Y)
    with pytest.raises(AssertionError, match="outputs in"):
        gpy_amd.SparseGPClassification(X, 2.0 * Y)
    assert not rctx


def test_to_dict_and_import_paths(rctx, monkeypatch):
    lfi = gpy_amd.inference.latent_function_inference
    assert gpy_amd.EPDTC is EPDTC and lfi.EPDTC is EPDTC and lfi.expectation_propagation.EPDTC is EPDTC
    inf = EPDTC(epsilon=1e-5, eta=0.9, delta=0.8, always_reset=True, max_iters=50, ep_mode="nested", parallel_updates=True)
    d = inf.to_dict()
    assert d == {"class": "GPy.inference.latent_function_inference.expectation_propagation.EPDTC", "epsilon": 1e-5, "eta": 0.9,
                 "delta": 0.8, "always_reset": True, "max_iters": 50, "ep_mode": "nested", "parallel_updates": True, "loading": True}
    fx = E.load("parallel_rbf_iso_n150_m16_d2")
    inf = EPDTC(parallel_updates=True, max_iters=100)
    inf.inference(S.make_kernel(fx), fx["X"], fx["Z"], gpy_amd.Bernoulli(), fx["Y"])
    d = inf.to_dict()
    assert set(d["_ep_approximation"]) == {"post_params", "ga_approx", "log_Z_tilde"} and set(d["ga_approx_old"]) == {"tau", "v"}
    assert len(d["_ep_approximation"]["ga_approx"]["tau"]) == 150 and set(d["_ep_approximation"]["post_params"]) == {"mu", "Sigma_diag"}
    import json
    json.dumps(d)
    import pickle
    again = pickle.loads(pickle.dumps(inf))
    assert again._ctx is None and E.rel(again.ga_approx_old.tau, inf.ga_approx_old.tau) == 0.0


def test_the_binding_table_states_the_prototypes_of_the_epdtc_header():
    protos = _prototypes("mi355gp_epdtc.h")
    assert [p[0] for p in protos] == list(_lib.EPDTC_ABI) and len(protos) == 4 and all(p[1] == "int" for p in protos)
    assert not set(_lib.EPDTC_ABI) & (set(_lib.ABI) | set(_lib.DEBUG_LAUUM_ABI) | set(_lib.DEBUG_TILEOPS_ABI))
    for name, _, types in protos:
        bound = _lib.EPDTC_ABI[name]
        assert len(bound) == len(types), name
        for i, (c, b) in enumerate(zip(types, bound)):
            assert _type_class(c, b), (name, i, c, b)
        assert hasattr(_lib.lib(), name)
    import inspect
    assert "mi355gp_epdtc.h" in inspect.getsource(_lib.build)
    assert "mi355gp_epdtc.h" in open(os.path.join(ROOT, "gpy_amd", "csrc", "Makefile")).read()
    header = open(os.path.join(ROOT, "include", "mi355gp.h")).read()
    assert "epdtc" not in header.lower()                          # the drop-in header and its 84 prototypes are as they were
