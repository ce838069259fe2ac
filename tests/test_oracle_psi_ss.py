"""CPU: the spike-and-slab RBF psi-statistics and what stands on them -- the restatement of tests/psi_ss_ld.py against the
reference's own values in tests/golden/psi_ss/*.npz (tools/make_golden_psi_ss.py: `ssrbf_psi_comp.py`'s NumPy branch and
`SpikeAndSlabPrior`), its gradients against central differences of its own objective in long double, the far inducing point,
the measurement that bounds tests/test_gpu_psi_ss.py, and the host classes (posterior, prior, kernel dispatch, `VarDTC` routing,
`SSGPLVM`, every refusal) over a recording context (no device).

Measured here: the fp64 restatement's distance from the long-double one, relative to max |value| (psi1: absolute, in units of
the variance), the worst over psi_ss_ld.CASES -- the shapes of the device test:
    psi1 2.3e-15   psi2 2.3e-15   dvar 7.8e-16   dl 2.0e-14   dZ 3.8e-15   dmu 6.4e-15   dS 6.7e-15   dgamma 6.0e-14
(`F64_DISTANCE`, rounded up in the last digit; the test below prints the figures and holds them to twice these: NumPy's exp
differs by an ulp between its SIMD dispatches).  Times ten they bound
the device in tests/test_gpu_psi_ss.py.  Restatement (fp64) against the reference's fp64 fixture values, worst over the four
fixtures: statistics 6.4e-16, gradients 4.5e-15, KL and its gradients 0.  The whole evaluation (bound, KL, Woodbury pair, every
gradient, prediction at certain and at Gaussian points) against the three fit fixtures composed from the reference's pieces,
held to the sparse path's tolerances (1e-9 bound, 1e-6 gradients and means, 1e-5 variances): measured 2.4e-15 for the bound and
at most 4.3e-14 elsewhere."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

import psi_ss_ld as P

LD = np.longdouble
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(f for f in glob.glob(os.path.join(HERE, "golden", "psi_ss", "*.npz")) if not os.path.basename(f).startswith("fit_"))
FIX_IDS = [os.path.basename(f)[:-4] for f in FIXTURES]
FIT_FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "psi_ss", "fit_*.npz")))
FIT_IDS = [os.path.basename(f)[:-4] for f in FIT_FIXTURES]
TOL_LML, TOL_FIT, TOL_VAR = 1e-9, 1e-6, 1e-5       # the sparse path's tolerances (tests/test_gpu_sparse.py)
GRADS = ("dvar", "dl", "dZ", "dmu", "dS", "dgamma")
REF_STATS, REF_GRADS = 1e-15, 1e-14                 # restatement against the reference: a few ulps of a differently ordered sum


def _rel(x, ref):
    ref = np.asarray(ref, dtype=LD)
    return float(np.abs(np.asarray(x, dtype=LD) - ref).max() / max(float(np.abs(ref).max()), 1e-300))


def _args(g):
    d = g["dims"]
    return dict(variance=float(g["variance"]), lengthscale=g["lengthscale"], Z=g["Z"][:, d], mu=g["mu"][:, d], S=g["S"][:, d],
                gamma=g["gamma"][:, d])


def test_the_fixture_set_covers_the_cases_it_was_asked_for():
    assert FIX_IDS == ["ard", "far", "iso", "subset"]
    gs = dict((i, np.load(f)) for i, f in zip(FIX_IDS, FIXTURES))
    assert gs["ard"]["ARD"] == 1 and gs["iso"]["ARD"] == 0 and gs["iso"]["lengthscale"].size == 1
    assert len(gs["subset"]["dims"]) < gs["subset"]["D"]
    assert gs["iso"]["pi"].size == gs["iso"]["D"] and float(gs["iso"]["prior_variance"]) != 1.0
    for g in gs.values():
        assert np.all(g["gamma"][0] == 1e-9) and np.all(g["gamma"][1] == 1 - 1e-9)
        assert np.array_equal(g["dL2"], g["dL2"].T)             # the reference's dZ assumes a symmetric dL_dpsi2
        assert all(np.all(np.isfinite(g[k])) for k in g.files)


@pytest.mark.parametrize("path", FIXTURES, ids=FIX_IDS)
def test_restatement_matches_the_reference(path):
    g = np.load(path)
    a = _args(g)
    p0, p1, p2 = P.stats(**a)
    assert np.array_equal(p0, g["psi0"])
    assert _rel(p1, g["psi1"]) <= REF_STATS and _rel(p2, g["psi2"]) <= REF_STATS
    got = P.grads(dL_dpsi0=g["dL0"], dL_dpsi1=g["dL1"], dL_dpsi2=g["dL2"], **a)
    for k in GRADS:
        assert _rel(got[k], g[k]) <= REF_GRADS, k
    pi, v = g["pi"], float(g["prior_variance"])
    assert abs(P.kl(g["mu"], g["S"], g["gamma"], pi, v) - float(g["KL"])) <= 1e-14 * abs(float(g["KL"]))
    for x, k in zip(P.kl_grads(g["mu"], g["S"], g["gamma"], pi, v), ("kl_dmu", "kl_dS", "kl_dgamma")):
        assert _rel(x, g[k]) <= 1e-15, k


def test_the_fit_fixtures_cover_the_cases_they_were_asked_for():
    gs = [np.load(f) for f in FIT_FIXTURES]
    assert len(gs) == 3
    assert any(bool(g["ARD"]) for g in gs) and any(not bool(g["ARD"]) for g in gs)
    assert any(len(g["dims"]) < g["mu"].shape[1] for g in gs) and any(g["white"].size for g in gs) and any(not g["white"].size for g in gs)
    assert any(g["Y"].shape[1] > 1 for g in gs) and any(g["Y"].shape[1] == 1 for g in gs)
    for g in gs:
        assert float(g["cond"]) <= 1e4                            # the generator refuses more, and jitchol's ladder
        assert np.all(g["gamma"][0] == 1e-9) and np.all(g["gamma"][1] == 1 - 1e-9)
        assert all(np.all(np.isfinite(g[k])) for k in g.files)


def check_fit_against_fixture(r, g, pred=None):
    """hold an evaluation r (the quantities of `psi_ss_ld.evaluate`; `bound`, the q(X) gradients with the prior's share as
    Xmean_grad / Xvar_grad / Xgamma_grad where r has them) and predictions to a fit fixture at the sparse path's tolerances"""
    for q, tol in (("lml", TOL_LML), ("KL", TOL_LML), ("bound", TOL_LML)):
        if q in r:
            assert abs(float(r[q]) - float(g[q])) <= tol * abs(float(g[q])), (q, float(r[q]), float(g[q]))
    for q in ("woodbury_vector", "woodbury_inv", "dtheta", "dnoise", "Xmean_grad", "Xvar_grad", "Xgamma_grad"):
        if q in r:
            assert _rel(np.ravel(r[q]) if q == "dnoise" else r[q], g[q]) <= TOL_FIT, (q, _rel(np.ravel(r[q]) if q == "dnoise" else r[q], g[q]))
    for q in ("dZ", "dmu", "dS", "dgamma"):
        if q in r:
            assert _rel(r[q], P.widen(g[q], g)) <= TOL_FIT, (q, _rel(r[q], P.widen(g[q], g)))
    for q, tol in (("pred_mu", TOL_FIT), ("pred_var", TOL_VAR), ("upred_mu", TOL_FIT), ("upred_var", TOL_VAR)):
        if pred is not None and q in pred:
            assert _rel(pred[q], g[q]) <= tol, (q, _rel(pred[q], g[q]))


@pytest.mark.parametrize("path", FIT_FIXTURES, ids=FIT_IDS)
def test_restated_evaluation_and_prediction_match_the_references_composed_fit(path):
    """VarDTC.inference + SpikeAndSlabPrior + the gradients of SparseGP._update_gradients + Posterior._raw_predict, composed by
    tools/make_golden_psi_ss.py from the reference's own pieces"""
    import psi_lin_ld as PL
    g = np.load(path)
    c = P.fixture_problem(g)
    r = P.evaluate(c["k"], c["Z"], c["mu"], c["S"], c["gamma"], c["Y"], c["noise"], np.float64, pi=c["pi"])
    assert abs(r["kappa"] - float(g["cond"])) <= 1e-6 * float(g["cond"])
    r.update(Xmean_grad=r["dmu"] - r["kl_dmu"], Xvar_grad=r["dS"] - r["kl_dS"], Xgamma_grad=r["dgamma"] - r["kl_dgamma"])
    pm, pv = PL.predict_certain(c["kl"], c["Z"], r, g["Xs"], np.float64)
    um, uv = PL.predict(c["kl"], c["Z"], r, g["Xs"], g["Ss"], np.float64)
    check_fit_against_fixture(r, g, dict(pred_mu=pm, pred_var=pv, upred_mu=um, upred_var=uv))
    off = [q for q in range(c["k"]["D"]) if q not in c["k"]["dims"]]
    assert all(not np.any(r[q][:, off]) for q in ("dZ", "dmu", "dS", "dgamma"))


def test_the_far_inducing_point_gives_exact_zeros_and_no_nan():
    g = np.load(os.path.join(HERE, "golden", "psi_ss", "far.npz"))
    a = _args(g)
    far = int(g["M"]) // 2
    for dt in (np.float64, LD):
        p0, p1, p2 = P.stats(dtype=dt, **a)
        got = P.grads(dL_dpsi0=g["dL0"], dL_dpsi1=g["dL1"], dL_dpsi2=g["dL2"], dtype=dt, **a)
        assert all(np.all(np.isfinite(np.asarray(got[k], dtype=np.float64))) for k in GRADS)
        if dt is np.float64:                                             # exp(-1800) underflows in fp64, not in long double
            assert np.all(p1[:, far] == 0) and np.all(p2[far] == 0) and np.all(p2[:, far] == 0) and np.all(got["dZ"][far] == 0)
        else:
            assert np.abs(p1[:, far]).max() < 1e-300 and np.abs(got["dZ"][far]).max() < 1e-300
    assert np.all(g["psi1"][:, far] == 0) and np.all(g["dZ"][far] == 0)      # and so says the reference


@pytest.mark.parametrize("ARD", [True, False], ids=["ard", "iso"])
def test_long_double_gradients_against_central_differences_of_the_objective(ARD):
    c = P.make_case(7, 5, 3, ARD, True)
    kw = dict((k, np.asarray(c[k], dtype=LD)) for k in ("lengthscale", "Z", "mu", "S", "gamma"))
    kw["gamma"] = np.clip(kw["gamma"], LD(0.05), LD(0.95))             # a step of 1e-9 in gamma = 1e-9 would leave (0, 1)
    kw["variance"] = np.asarray([c["variance"]], dtype=LD)
    dL = (c["dL0"], c["dL1"], c["dL2_raw"])                            # not symmetric: the gradients are those of sym(dL_dpsi2)

    def f(**over):
        k = dict(kw, **over)
        return P.objective(k["variance"], k["lengthscale"], k["Z"], k["mu"], k["S"], k["gamma"], *dL, weights=c["weights"], dtype=LD)
    got = P.grads(kw["variance"], kw["lengthscale"], kw["Z"], kw["mu"], kw["S"], kw["gamma"], *dL, weights=c["weights"], dtype=LD)
    h = LD(1e-9)
    for name, key in (("variance", "dvar"), ("lengthscale", "dl"), ("Z", "dZ"), ("mu", "dmu"), ("S", "dS"), ("gamma", "dgamma")):
        x = kw[name]
        num = np.zeros(x.shape, dtype=LD)
        for i in np.ndindex(*x.shape):
            xp, xm = x.copy(), x.copy()
            xp[i] += h
            xm[i] -= h
            num[i] = (f(**{name: xp}) - f(**{name: xm})) / (2 * h)
        ana = np.asarray(got[key], dtype=LD).reshape(x.shape)
        assert _rel(ana, num) <= 1e-8, (name, _rel(ana, num))         # h^2 f''' / 6 ~ 1e-18, rounding 1e-19 / 1e-9


F64_DISTANCE = dict(psi1=2.3e-15, psi2=2.3e-15, dvar=7.8e-16, dl=2.0e-14, dZ=3.8e-15, dmu=6.4e-15, dS=6.7e-15, dgamma=6.0e-14)


def f64_distances(c):
    kw = dict((k, c[k]) for k in ("variance", "lengthscale", "Z", "mu", "S", "gamma", "weights"))
    d = dict(dL_dpsi0=c["dL0"], dL_dpsi1=c["dL1"], dL_dpsi2=c["dL2"])
    _, a1, a2 = P.stats(dtype=LD, **kw)
    _, b1, b2 = P.stats(dtype=np.float64, **kw)
    ga, gb = P.grads(dtype=LD, **dict(kw, **d)), P.grads(dtype=np.float64, **dict(kw, **d))
    out = dict(psi1=float(np.abs(b1 - a1).max()) / float(c["variance"]), psi2=_rel(b2, a2))
    out.update((k, _rel(gb[k], ga[k])) for k in GRADS)
    return out


def test_float64_distance_from_long_double_on_the_shapes_of_the_device_test():
    """the measurement that sets the device bounds: printed, and held to the figures the device test multiplies by ten"""
    worst = dict.fromkeys(F64_DISTANCE, 0.0)
    for name, N, M, Q, ARD, wt in P.CASES:
        d = f64_distances(P.make_case(N, M, Q, ARD, wt))
        print("%-14s %s" % (name, "  ".join("%s %.1e" % kv for kv in d.items())))
        worst = dict((k, max(worst[k], d[k])) for k in worst)
    print("worst          %s" % "  ".join("%s %.1e" % kv for kv in worst.items()))
    for k, v in worst.items():
        assert v <= 2 * F64_DISTANCE[k], (k, v)


@pytest.mark.parametrize("case", P.FIT_CASES, ids=[c[0] for c in P.FIT_CASES])
def test_fit_inputs_are_well_conditioned_and_the_float64_evaluation_is_close(case):
    name, N, M, Q, Dy, ARD, dims = case
    c = P.lattice_problem(N, M, Q, Dy, 7, ARD=ARD, dims=dims)
    r = P.evaluate(c["k"], c["Z"], c["mu"], c["S"], c["gamma"], c["Y"], c["noise"], LD)
    assert r["kappa"] <= 1e4, r["kappa"]
    r64 = P.evaluate(c["k"], c["Z"], c["mu"], c["S"], c["gamma"], c["Y"], c["noise"], np.float64)
    for q in ("lml", "dtheta", "dZ", "dmu", "dS", "dgamma", "woodbury_vector"):
        assert _rel(r64[q], r[q]) <= 1e-11, q
    if dims is not None:
        off = [q for q in range(Q) if q not in dims]
        assert all(np.all(r[q][:, off] == 0) for q in ("dZ", "dmu", "dS", "dgamma"))


def test_evaluation_gradients_against_central_differences_of_the_bound():
    c = P.lattice_problem(9, 4, 2, 2, 3)
    c["gamma"] = np.clip(c["gamma"], 0.05, 0.95)
    r = P.evaluate(c["k"], c["Z"], c["mu"], c["S"], c["gamma"], c["Y"], c["noise"], LD, pi=[0.3, 0.6], prior_variance=1.4)
    h = LD(1e-8)
    for name, grad in (("Z", r["dZ"]), ("mu", r["dmu"] - r["kl_dmu"]), ("S", r["dS"] - r["kl_dS"]), ("gamma", r["dgamma"] - r["kl_dgamma"])):
        x = np.asarray(c[name], dtype=LD)
        for i in [(0, 0), (2, 1), (x.shape[0] - 1, 1)]:
            xp, xm = x.copy(), x.copy()
            xp[i] += h
            xm[i] -= h
            fp, fm = (P.evaluate(c["k"], *[dict(c, **{name: y})[k] for k in ("Z", "mu", "S", "gamma", "Y", "noise")], dt=LD, pi=[0.3, 0.6],
                                 prior_variance=1.4)["bound"] for y in (xp, xm))
            assert abs((fp - fm) / (2 * h) - grad[i]) <= 1e-7 * max(1.0, abs(float(grad[i]))), (name, i)


# ---- the C-ABI table ------------------------------------------------------------------------------------------------------
def test_the_binding_table_matches_the_header_and_the_library_exports_it():
    from gpy_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(HERE, "..", "include", "mi355gp_psi_ss.h")).read(), flags=re.S)
    protos = re.findall(r"\bint\s+(mi355gp_\w+)\s*\(([^;]*?)\)\s*;", text)
    assert [p[0] for p in protos] == list(_lib.PSI_SS_ABI) == ["mi355gp_ssrbf_psi", "mi355gp_ssrbf_psi_grad", "mi355gp_sparse_set_binary_prob",
                                                                "mi355gp_sparse_set_inputs_ss", "mi355gp_vardtc_inference_ss"]
    for name, params in protos:
        params = [" ".join(p.split()) for p in params.split(",")]
        bound = _lib.PSI_SS_ABI[name]
        assert len(bound) == len(params), name
        for c, b in zip(params, bound):
            if "double*" in c:
                assert getattr(b, "_dtype_", None) == np.dtype(np.float64) or b is ctypes.POINTER(ctypes.c_double), (name, c)
            elif c.startswith("int64_t"):
                assert b is ctypes.c_int64, (name, c)
            elif c.startswith("double"):
                assert b is ctypes.c_double, (name, c)
            elif c.startswith("mi355gp_sparse*"):
                assert b is ctypes.c_void_p, (name, c)
            elif "mi355gp_part*" in c:
                assert b is ctypes.POINTER(_lib.Part), (name, c)
            else:
                assert c.startswith("int ") and b is ctypes.c_int, (name, c)
        assert name not in _lib.ABI                                   # not in mi355gp.h: its prototype count stays
    _lib.build()
    for name in _lib.PSI_SS_ABI:
        assert hasattr(_lib.lib(), name), "libmi355gp.so does not export %s" % name
    # the signatures of the Gaussian pair with gamma after S and dgamma_out after dS_out
    for ss, g, at in (("mi355gp_ssrbf_psi", "mi355gp_rbf_psi", (7,)), ("mi355gp_ssrbf_psi_grad", "mi355gp_rbf_psi_grad", (7, 20))):
        assert [b for i, b in enumerate(_lib.PSI_SS_ABI[ss]) if i not in at] == _lib.ABI[g]
    u = _lib.ABI["mi355gp_vardtc_inference_uncertain"]
    assert _lib.PSI_SS_ABI["mi355gp_vardtc_inference_ss"] == u[:-1] + [ctypes.POINTER(ctypes.c_double)] + u[-1:]


# ---- the host classes ------------------------------------------------------------------------------------------------------
def _q(N=6, Q=3, seed=0):
    r = np.random.default_rng(seed)
    return r.uniform(-2, 2, (N, Q)), r.uniform(0.1, 0.5, (N, Q)), r.uniform(0.1, 0.9, (N, Q))


def test_posterior_is_parameterized_and_a_sibling_of_the_normal_one():
    import gpy_amd
    from gpy_amd.variational import SpikeAndSlabPosterior, SpikeAndSlabPrior
    assert gpy_amd.SpikeAndSlabPosterior is SpikeAndSlabPosterior and gpy_amd.SpikeAndSlabPrior is SpikeAndSlabPrior
    V = gpy_amd.core.parameterization.variational
    assert V.SpikeAndSlabPosterior is SpikeAndSlabPosterior and V.SpikeAndSlabPrior is SpikeAndSlabPrior
    assert not issubclass(SpikeAndSlabPosterior, gpy_amd.NormalPosterior)
    m, v, g = _q()
    q = SpikeAndSlabPosterior(m, v, g)
    assert q.name == "latent space" and q.has_uncertain_inputs() and q.shape == (6, 3) and len(q) == 6 and q.num_data == 6 and q.input_dim == 3
    assert [p.name for p in q.parameters] == ["mean", "variance", "binary_prob"] and q.gamma is q.binary_prob
    assert q.variance.positive and not q.mean.positive and not q.binary_prob.positive
    assert np.array_equal(q.param_array, np.concatenate([m.ravel(), v.ravel(), g.ravel()]))
    s = q[1:5, [0, 2]]
    assert isinstance(s, SpikeAndSlabPosterior) and s.shape == (4, 2) and np.array_equal(s.binary_prob, g[1:5][:, [0, 2]])
    with pytest.raises(IndexError, match="both axes"):
        q[0]
    c = q.copy()
    c.mean[0, 0] += 1.0
    assert q.mean[0, 0] == m[0, 0] and isinstance(c, SpikeAndSlabPosterior)
    q.set_gradients((np.ones(m.shape), 2 * np.ones(m.shape), 3 * np.ones(m.shape)))
    assert np.all(q.mean.gradient == 1) and np.all(q.variance.gradient == 2) and np.all(q.binary_prob.gradient == 3)
    for bad, pat in (((m, v, g[:, :2]), "same shape"), ((m, -v, g), "positive"), ((m, v, np.where(g > 0.5, 1.0, g)), r"\(0, 1\)"),
                     ((m, v, g * np.nan), r"\(0, 1\)")):
        with pytest.raises(ValueError, match=pat):
            SpikeAndSlabPosterior(*bad)


@pytest.mark.parametrize("path", FIXTURES, ids=FIX_IDS)
def test_prior_kl_and_gradients_match_the_reference(path):
    import gpy_amd
    g = np.load(path)
    q = gpy_amd.SpikeAndSlabPosterior(g["mu"], g["S"], g["gamma"])
    prior = gpy_amd.SpikeAndSlabPrior(pi=g["pi"], variance=float(g["prior_variance"]))
    assert abs(prior.KL_divergence(q) - float(g["KL"])) <= 1e-14 * abs(float(g["KL"]))
    q.set_gradients((np.full(q.shape, 1.0), np.full(q.shape, 2.0), np.full(q.shape, 3.0)))
    prior.update_gradients_KL(q)                                      # subtracts
    assert _rel(1.0 - q.mean.gradient, g["kl_dmu"]) <= 1e-15 and _rel(2.0 - q.variance.gradient, g["kl_dS"]) <= 1e-15
    assert _rel(3.0 - q.binary_prob.gradient, g["kl_dgamma"]) <= 1e-15
    for kw, pat in ((dict(learnPi=True), "learnPi"), (dict(group_spike=True), "group_spike")):
        with pytest.raises(NotImplementedError, match=pat):
            gpy_amd.SpikeAndSlabPrior(**kw)
    with pytest.raises(ValueError, match="pi must be"):
        gpy_amd.SpikeAndSlabPrior(pi=1.0)


def test_kernels_dispatch_on_the_type_of_qX(monkeypatch):
    import gpy_amd
    from gpy_amd import _lib
    calls = []

    def psi(variance, lengthscale, ARD, Z, mu, S, gamma, weights=None, want_psi1=True, want_psi2=True, device=0):
        calls.append(("psi", Z.shape, mu.shape, gamma.copy(), want_psi1, want_psi2))
        return (np.zeros((mu.shape[0], Z.shape[0])) if want_psi1 else None, np.zeros((Z.shape[0],) * 2) if want_psi2 else None)

    def grad(variance, lengthscale, ARD, Z, mu, S, gamma, dL_dpsi0=None, dL_dpsi1=None, dL_dpsi2=None, weights=None, device=0):
        calls.append(("grad", Z.shape, mu.shape))
        D = mu.shape[1]
        return 1.0, np.full(D if ARD else 1, 2.0), np.full(Z.shape, 3.0), np.full(mu.shape, 4.0), np.full(mu.shape, 5.0), np.full(mu.shape, 6.0)
    monkeypatch.setattr(_lib, "ssrbf_psi", psi)
    monkeypatch.setattr(_lib, "ssrbf_psi_grad", grad)
    monkeypatch.setattr(_lib, "rbf_psi", lambda *a, **k: pytest.fail("a spike-and-slab qX took the Gaussian statistics"))
    monkeypatch.setattr(_lib, "rbf_psi_grad", lambda *a, **k: pytest.fail("a spike-and-slab qX took the Gaussian statistics"))
    m, v, g = _q(N=6, Q=4)
    q = gpy_amd.SpikeAndSlabPosterior(m, v, g)
    Z = np.zeros((5, 4))
    k = gpy_amd.RBF(2, ARD=True, active_dims=[1, 3])
    assert np.array_equal(k.psi0(Z, q), np.full(6, 1.0)) and k.psi1(Z, q).shape == (6, 5) and k.psi2(Z, q).shape == (5, 5)
    assert calls[0][1:3] == ((5, 2), (6, 2)) and np.array_equal(calls[0][3], g[:, [1, 3]]) and calls[0][4:] == (True, False)
    with pytest.raises(NotImplementedError, match="psi2n"):
        k.psi2n(Z, q)
    d = (np.zeros(6), np.zeros((6, 5)), np.zeros((5, 5)))
    gq = k.gradients_qX_expectations(*d, Z, q)
    assert len(gq) == 3 and all(x.shape == (6, 4) for x in gq)
    assert np.all(gq[2][:, [1, 3]] == 6.0) and np.all(gq[2][:, [0, 2]] == 0.0) and np.all(gq[0][:, [1, 3]] == 4.0)
    dZ = k.gradients_Z_expectations(*d, Z, q)
    assert np.all(dZ[:, [1, 3]] == 3.0) and np.all(dZ[:, [0, 2]] == 0.0)
    k.update_gradients_expectations(*d, Z, q)
    assert k.variance.gradient[0] == 1.0 and np.all(k.lengthscale.gradient == 2.0)
    w = gpy_amd.White(4, variance=0.3)
    assert all(not x.any() and x.shape == (6, 4) for x in w.gradients_qX_expectations(*d, Z, q)) and len(w.gradients_qX_expectations(*d, Z, q)) == 3
    assert len(w.gradients_qX_expectations(*d, Z, gpy_amd.NormalPosterior(m, v))) == 2
    add = gpy_amd.Add([k, w])
    assert np.array_equal(add.psi0(Z, q), np.full(6, 1.3)) and add.psi2(Z, q).shape == (5, 5)
    ga = add.gradients_qX_expectations(*d, Z, q)
    assert len(ga) == 3 and np.all(ga[2][:, [1, 3]] == 6.0)
    for other, name in ((gpy_amd.Bias(4), "Bias"), (gpy_amd.Linear(4), "Linear"), (gpy_amd.Matern52(4), "Matern52")):
        for kw in ({}, {"psi_lin_bias": True}):
            with pytest.raises(NotImplementedError, match=name):
                gpy_amd.Add([gpy_amd.RBF(4), other]).psi1(Z, q, **kw)


# ---- VarDTC and SSGPLVM over a recording context: no device ---------------------------------------------------------------------
from test_oracle_bgplvm import RecSparse  # noqa: E402


class RecSS(RecSparse):
    def set_binary_prob(self, gamma):
        self.log.append(("set_binary_prob", None if gamma is None else np.array(gamma)))

    def set_inputs_ss(self, X, S, gamma):
        self.log.append(("set_inputs_ss", np.array(X), np.array(S), np.array(gamma)))

    def vardtc_ss(self, specs, Z, noise, **kw):
        self.log.append(("vardtc_ss", [s[0] for s in specs], np.array(Z), np.array(noise)))
        rc, r = self._res(specs, Z)
        r["dgamma"] = np.full((self.N, self.D), 6.0)
        return rc, r


@pytest.fixture
def rec(monkeypatch):
    from gpy_amd import _lib
    made = []

    class Ctx(RecSS):
        def __init__(self, device=0):
            RecSS.__init__(self, device)
            made.append(self)
    monkeypatch.setattr(_lib, "SparseContext", Ctx)
    return made


def _problem(N=12, Q=3, Dy=4, M=5, seed=4):
    r = np.random.default_rng(seed)
    return (r.standard_normal((N, Dy)), r.uniform(-2, 2, (N, Q)), r.uniform(0.1, 0.5, (N, Q)), r.uniform(0.1, 0.9, (N, Q)),
            r.uniform(-2, 2, (M, Q)))


def test_vardtc_routes_a_spike_and_slab_posterior_to_its_own_entry(rec):
    import gpy_amd
    Y, X, S, G, Z = _problem()
    inf = gpy_amd.VarDTC()
    k, lik = gpy_amd.RBF(3, ARD=True) + gpy_amd.White(3, variance=0.1), gpy_amd.Gaussian(0.1)
    q = gpy_amd.SpikeAndSlabPosterior(X, S, G)
    post, lml, gd = inf.inference(k, q, Z, lik, Y)
    log = rec[0].log
    assert [c[0] for c in log] == ["set_data", "set_input_variance", "set_binary_prob", "vardtc_ss"] and log[3][1] == ["rbf", "white"]
    assert np.array_equal(log[2][1], G)
    assert sorted(gd["fused"]) == ["dS", "dZ", "dgamma", "dmu", "dtheta"] and np.all(gd["fused"]["dgamma"] == 6.0)
    assert sorted(gd) == ["dL_dKmm", "dL_dpsi0", "dL_dpsi1", "dL_dpsi2", "dL_dthetaL", "fused"]        # the uncertain path's
    # new inputs, the same Y: one three-array upload
    q2 = gpy_amd.SpikeAndSlabPosterior(X + 0.1, S, G * 0.9)
    inf.inference(k, q2, Z, lik, Y)
    assert [c[0] for c in log][4:] == ["set_inputs_ss", "vardtc_ss"] and np.array_equal(log[4][3], G * 0.9)
    # Gaussian inputs on the same session: gamma is cleared, not silently kept
    inf.inference(k, gpy_amd.NormalPosterior(X + 0.1, S), Z, lik, Y)
    assert [c[0] for c in log][6:] == ["set_binary_prob", "vardtc_uncertain"] and log[6][1] is None
    inf.inference(k, q2, Z, lik, Y)
    assert [c[0] for c in log][8:] == ["set_inputs_ss", "vardtc_ss"]
    # what it refuses, by name, before any upload
    n = len(log)
    for kern, pat in ((gpy_amd.Linear(3), "sslinear_psi_comp"), (gpy_amd.RBF(3) + gpy_amd.Bias(3), "Bias"),
                      (gpy_amd.Matern52(3), "Matern52"), (gpy_amd.RBF(3) * gpy_amd.RBF(3), "Prod")):
        with pytest.raises(NotImplementedError, match=pat):
            gpy_amd.VarDTC(psi_lin_bias=True).inference(kern, q, Z, lik, Y)
        with pytest.raises(NotImplementedError, match=pat):
            inf.inference(kern, q, Z, lik, Y)
    with pytest.raises(NotImplementedError, match="exactly one RBF"):
        inf.inference(gpy_amd.RBF(3) + gpy_amd.RBF(3), q, Z, lik, Y)
    with pytest.raises(NotImplementedError, match="heteroscedastic"):
        inf.inference(k, q, Z, gpy_amd.HeteroscedasticGaussian({"output_index": np.arange(12)[:, None]}), Y,
                      Y_metadata={"output_index": np.arange(12)[:, None]})
    assert len(log) == n


def test_every_other_consumer_refuses_the_type_by_name(rec):
    import gpy_amd
    Y, X, S, G, Z = _problem()
    q = gpy_amd.SpikeAndSlabPosterior(X, S, G)
    k, lik = gpy_amd.RBF(3), gpy_amd.Gaussian(0.1)
    pat = "SpikeAndSlabPosterior"
    for inf in (gpy_amd.FITC(), gpy_amd.PEP(alpha=0.5), gpy_amd.EPDTC()):
        with pytest.raises(NotImplementedError, match=pat):
            inf.inference(k, q, Z, lik, Y[:, :1])
    with pytest.raises(NotImplementedError, match=pat):
        gpy_amd.svgp.SVGP().inference(np.zeros((5, 1)), np.eye(5)[None], k, q, Z, lik, Y[:, :1])
    for inf in (gpy_amd.ExactGaussianInference(), gpy_amd.Laplace(), gpy_amd.EP(), gpy_amd.VarGauss(np.zeros((12, 1)), np.ones((12, 1))),
                gpy_amd.GaussianGridInference()):
        with pytest.raises(NotImplementedError, match=pat):
            inf.inference(k, q, lik, Y[:, :1])
    with pytest.raises(NotImplementedError, match=pat):
        gpy_amd.ExactStudentTInference().inference(k, q, Y[:, :1], 4.0)
    for make in (lambda: gpy_amd.SparseGPRegression(q, Y, Z=Z), lambda: gpy_amd.SparseGP(q, Y, Z, k, lik),
                 lambda: gpy_amd.SparseGPClassification(q, np.sign(Y[:, :1]), Z=Z), lambda: gpy_amd.SVGP(q, Y[:, :1], Z, k, lik)):
        with pytest.raises(NotImplementedError, match=pat):
            make()
    assert not rec                                                    # nobody made a context


def test_logistic_transform_round_trip_and_chain_rule(rec):
    import gpy_amd
    Y, X, S, G, Z = _problem()
    G[0, 0], G[1, 1] = 1e-9, 1 - 1e-9
    m = gpy_amd.SSGPLVM(Y, 3, X=X, X_variance=S, Gamma=G, Z=Z)
    N, Q = X.shape
    sl = slice(2 * N * Q, 3 * N * Q)
    x = m.optimizer_array
    lo, hi = m.GAMMA_LOWER, m.GAMMA_UPPER
    assert np.allclose(x[sl], np.log((G.ravel() - lo) / (hi - G.ravel())), rtol=1e-12)
    assert np.allclose(x[N * Q:2 * N * Q], np.log(S.ravel())) and np.array_equal(x[:N * Q], X.ravel())
    m.optimizer_array = x
    assert np.allclose(m.X.binary_prob.values, G, rtol=1e-9) and np.allclose(m.param_array[:sl.start], np.concatenate([X.ravel(), S.ravel()]))
    x2 = x.copy()
    x2[sl] = np.linspace(-50, 50, N * Q)                              # far out: gamma stays strictly inside (0, 1)
    m.optimizer_array = x2
    g = m.X.binary_prob.values
    assert np.all((g > 0) & (g < 1)) and g.min() >= lo and g.max() <= hi
    gr = m._grads(x2)
    gam = m.param_array[sl]
    raw = m.objective_function_gradients()
    assert np.allclose(gr[sl], raw[sl] * (gam - lo) * (hi - gam) / (hi - lo), rtol=1e-14)
    assert np.allclose(gr[N * Q:sl.start], raw[N * Q:sl.start] * m.param_array[N * Q:sl.start]) and np.array_equal(gr[:N * Q], raw[:N * Q])
    import pickle
    p = pickle.loads(pickle.dumps(m.X.binary_prob))                   # Param pickles as before: name, positive, gradient
    assert p.name == "binary_prob" and p.positive is False and np.array_equal(p, m.X.binary_prob)


def test_model_parameters_uploads_objective_and_gradients_over_a_recording_context(rec):
    import gpy_amd
    import gpy_amd as GPy
    assert GPy.models.ss_gplvm.SSGPLVM is gpy_amd.SSGPLVM and issubclass(gpy_amd.SSGPLVM, gpy_amd.SparseGP)
    with pytest.raises(NotImplementedError, match="ss_gplvm.SSGPLVM"):
        GPy.models.SSGPLVM
    Y, X, S, G, Z = _problem()
    N, Q, M = X.shape[0], X.shape[1], Z.shape[0]
    m = gpy_amd.SSGPLVM(Y, Q, X=X, X_variance=S, Gamma=G, Z=Z, pi=[0.3, 0.5, 0.7])
    assert m.name == "Spike_and_Slab GPLVM" and isinstance(m.X, gpy_amd.SpikeAndSlabPosterior) and m.has_uncertain_inputs()
    assert isinstance(m.kern, gpy_amd.RBF) and m.kern.ARD and isinstance(m.likelihood, gpy_amd.Gaussian)
    assert isinstance(m.variational_prior, gpy_amd.SpikeAndSlabPrior) and isinstance(m.inference_method, gpy_amd.VarDTC)
    assert m.parameters[0] is m.X and m.parameters[1] is m.Z
    assert [p.name for p in m.flattened_parameters()][:4] == ["mean", "variance", "binary_prob", "inducing inputs"]
    pa = m.param_array
    assert pa.size == 3 * N * Q + M * Q + (1 + Q) + 1 == len(m.parameter_names())
    assert np.array_equal(pa[:3 * N * Q], np.concatenate([X.ravel(), S.ravel(), G.ravel()])) and np.array_equal(pa[3 * N * Q:3 * N * Q + M * Q], Z.ravel())
    log = rec[0].log
    assert [c[0] for c in log] == ["set_data", "set_input_variance", "set_binary_prob", "vardtc_ss"]
    k = P.kl(X, S, G, [0.3, 0.5, 0.7], 1.0)
    kmu, kS, kg = P.kl_grads(X, S, G, [0.3, 0.5, 0.7], 1.0)
    assert np.isclose(m.log_likelihood(), -1.0 - k, rtol=1e-14) and np.isclose(m.objective_function(), 1.0 + k, rtol=1e-14)
    assert np.allclose(m.X.mean.gradient, 4.0 - kmu, rtol=1e-14) and np.allclose(m.X.variance.gradient, 5.0 - kS, rtol=1e-14)
    assert np.allclose(m.X.binary_prob.gradient, 6.0 - kg, rtol=1e-14)
    assert m.get_X_gradients(m.X)[2] is m.X.binary_prob.gradient
    # a step in q(X) goes through set_inputs_ss; Z alone uploads nothing
    new = pa.copy()
    new[2 * N * Q:3 * N * Q] *= 0.9
    m.param_array = new
    assert [c[0] for c in log][4:] == ["set_inputs_ss", "vardtc_ss"] and np.array_equal(log[4][3], G * 0.9)
    new[3 * N * Q] += 1.0
    m.param_array = new
    assert [c[0] for c in log][6:] == ["vardtc_ss"]
    assert m.checkgrad() in (True, False)                             # the plumbing runs (the recorded numbers are not a bound)
    # prediction: certain points, NormalPosterior points; spike-and-slab points are refused
    mu, var = m.predict(X[:5])
    assert log[-1][0] == "sparse_predict" and mu.shape == (5, Y.shape[1])
    mu, var = m.predict(gpy_amd.NormalPosterior(X[:5], S[:5]))
    assert log[-1][0] == "predict_uncertain" and mu.shape == var.shape == (5, Y.shape[1])
    with pytest.raises(NotImplementedError, match="spike-and-slab new points"):
        m.predict(gpy_amd.SpikeAndSlabPosterior(X[:5], S[:5], G[:5]))
    assert np.array_equal(m.input_sensitivity(), m.kern.input_sensitivity())
    assert np.array_equal(gpy_amd.SSGPLVM(Y, Q, X=X, X_variance=S, Gamma=G, Z=Z, kernel=gpy_amd.RBF(Q), pi=[0.3, 0.5, 0.7]).input_sensitivity(),
                          [0.3, 0.5, 0.7])


def test_model_defaults_follow_the_reference(rec):
    import gpy_amd
    from gpy_amd.util.initialization import initialize_latent
    Y = np.random.default_rng(3).standard_normal((15, 6))
    np.random.seed(5)
    m = gpy_amd.SSGPLVM(Y, 3, num_inducing=4)
    X0, fracs = initialize_latent("PCA", 3, Y)
    assert np.array_equal(m.X.mean.values, X0) and m.Z.shape == (4, 3)
    assert np.allclose(m.kern.lengthscale.values, fracs)              # fracs, not 1 / fracs: ss_gplvm.py:221
    g = m.X.binary_prob.values
    assert g.min() >= 1e-9 and g.max() <= 1 - 1e-9 and abs(g.mean() - 0.5) < 0.1 and 0.03 < g.std() < 0.2
    assert np.all((m.X.variance.values > 0) & (m.X.variance.values < 0.1))
    assert np.array_equal(m.variational_prior.pi, [0.5]) and m.variational_prior.variance == 1.0
    assert all(any(np.array_equal(z, x) for x in X0) for z in m.Z.values)


def test_model_refusals_name_what_they_refuse(rec):
    import gpy_amd
    Y, X, S, G, Z = _problem()
    for kw in (dict(group_spike=True), dict(IBP=True), dict(SLVM=True), dict(learnPi=True), dict(sharedX=True), dict(mpi_comm=object()),
               dict(normalizer=True), dict(variational_prior=gpy_amd.SpikeAndSlabPrior())):
        with pytest.raises(NotImplementedError, match=list(kw)[0]):
            gpy_amd.SSGPLVM(Y, 3, X=X, X_variance=S, Gamma=G, Z=Z, **kw)
    with pytest.raises(NotImplementedError, match="VarDTC_minibatch"):
        gpy_amd.SSGPLVM(Y, 3, X=X, X_variance=S, Gamma=G, Z=Z, inference_method=gpy_amd.FITC())
    with pytest.raises(NotImplementedError, match="sslinear_psi_comp"):
        gpy_amd.SSGPLVM(Y, 3, X=X, X_variance=S, Gamma=G, Z=Z, kernel=gpy_amd.Linear(3))
    with pytest.raises(ValueError, match="X must be"):
        gpy_amd.SSGPLVM(Y, 2, X=X)
    with pytest.raises(ValueError, match="Z must have"):
        gpy_amd.SSGPLVM(Y, 3, X=X, Z=Z[:, :2])
    m = gpy_amd.SSGPLVM(Y, 3, X=X, X_variance=S, Gamma=G, Z=Z)
    with pytest.raises(NotImplementedError, match="sslinear_psi_comp"):
        m.sample_W(3)
    with pytest.raises(NotImplementedError, match="infer_newX"):
        m.infer_newX(Y)
