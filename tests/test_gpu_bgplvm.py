"""GPU: `BayesianGPLVM`, `mi355gp_sparse_set_inputs` and prediction at uncertain points (`mi355gp_sparse_predict_uncertain`,
kernel `k_psi2n_contract` of gpy_amd/csrc/psi.hip).

The reference's fixtures (tests/golden/bgplvm, tools/make_golden_bgplvm.py) go through the model at the tolerances
tests/test_gpu_psi.py takes from the sparse path: bound 1e-9 relative, X.mean / X.variance / Z / kernel / noise gradients 1e-6,
predictive mean at uncertain points 1e-6, predictive variance 1e-5.

`k_psi2n_contract` is judged against the long-double restatement of tests/bgplvm_np.py GIVEN the device's own woodbury_vector
and woodbury_inv (from a real fit at each shape, so that no variance is clipped), at the smallest shapes that cross each
boundary the kernel has (bgplvm_np.EDGE_CASES): M below / across the 16-wide psi2 tile and the 64-wide psi1 tile (1, 15, 17,
65, 130), Mn below / across the row staging block (64 rows up to 16 dimensions, 32 up to 32, 16 beyond) and the 2048-row chunk
(1, 63, 65, 2051 with M = 8), Q in one padded group and in two (1, 3, 33, 40; 20: the 32-row block), Dy = 1, 3 and 4, 5 (four
output columns, the inverse's included, make one register group).
Bounds (tests/test_oracle_bgplvm.py has the measurement): mean 4.2e-15 and variance 1.3e-14 relative to psi0* -- ten times the
float64 restatement's own distance from long double.
Device figures (one MI355X, worst over the eleven shapes): mean 4.9e-16, variance 1.8e-15; two predictions give the same bytes.
Through the model, worst over the seven fixtures: bound 5.4e-13, X.mean gradient 1.9e-12, X.variance 4.3e-12, Z 9.8e-11, kernel
3.8e-12, noise 1.2e-12, woodbury_vector 1.4e-11, mean at uncertain points 9.4e-13, variance 2.9e-12; the fixtures with a White
part, whose Kmm is well conditioned, are met to 8e-14 or better.
"""
import glob
import os

import numpy as np
import pytest

import bgplvm_np as B
from gpy_amd import _lib

pytestmark = pytest.mark.gpu

LD = np.longdouble
TOL_PRED_MEAN, TOL_PRED_VAR = 4.2e-15, 1.3e-14
TOL_LML, TOL_FIT, TOL_VAR = 1e-9, 1e-6, 1e-5
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(f for f in glob.glob(os.path.join(HERE, "golden", "bgplvm", "*.npz")) if not os.path.basename(f).startswith("pca_"))
FIX_IDS = [os.path.basename(f)[:-4] for f in FIXTURES]


def _rel(x, ref, scale=None):
    ref = np.asarray(ref, dtype=LD)
    return float(np.abs(np.asarray(x, dtype=LD) - ref).max() / (np.abs(ref).max() if scale is None else scale))


def _specs(p):
    s = [("rbf", True, np.concatenate([[p["var"]], p["ls"]]), None, 0)]
    return s + [("white", False, np.array([w]), None, 0) for w in p["white"]]


def _fit(p, mu=None, S=None):
    ctx = _lib.SparseContext(0)
    ctx.set_data(p["mu"] if mu is None else mu, p["Y"])
    ctx.set_input_variance(p["S"] if S is None else S)
    rc, r = ctx.vardtc_uncertain(_specs(p), p["Z"], p["noise"])
    assert rc == 0
    return ctx, r


def _fixture_kernel(g):
    import gpy_amd
    D, dims = g["mu"].shape[1], [int(d) for d in g["dims"]]
    sub = None if dims == list(range(D)) else dims
    k = gpy_amd.RBF(len(dims), variance=float(g["variance"]), lengthscale=g["ls"], ARD=bool(g["ARD"]), active_dims=sub)
    for w in g["white"]:
        k = k + gpy_amd.White(len(dims), variance=float(w), active_dims=sub)
    return k, dims


@pytest.mark.parametrize("path", FIXTURES, ids=FIX_IDS)
def test_fixture_through_the_model(path):
    import gpy_amd
    g = np.load(path)
    k, dims = _fixture_kernel(g)
    N, D = g["mu"].shape
    M = g["Z"].shape[0]
    rest = [d for d in range(D) if d not in dims]
    m = gpy_amd.BayesianGPLVM(g["Y"], D, X=g["mu"], X_variance=g["S"], Z=g["Z"], kernel=k,
                              likelihood=gpy_amd.Gaussian(variance=float(g["noise"])))
    grad = m.gradient                                       # [X.mean, X.variance, Z, kernel, noise]
    gm, gs = grad[:N * D].reshape(N, D), grad[N * D:2 * N * D].reshape(N, D)
    dZ = grad[2 * N * D:2 * N * D + M * D].reshape(M, D)
    # the reference was handed the active columns only (tools/make_golden_bgplvm.py); the model's prior covers every column of
    # X, so the columns no part sees add their own KL term (restated, a sum over N numbers) to the reference's
    bound = float(g["bound"]) - (float(B.kl(g["mu"][:, rest], g["S"][:, rest], LD)[0]) if rest else 0.0)
    figs = {"bound": abs(m.log_likelihood() - bound) / abs(bound), "objective": abs(m.objective_function() + bound) / abs(bound)}
    for name, x, y in (("X.mean", gm[:, dims], g["Xmean_grad"]), ("X.variance", gs[:, dims], g["Xvar_grad"]), ("Z", dZ[:, dims], g["dZ"]),
                       ("theta", grad[2 * N * D + M * D:-1], g["dtheta"]), ("noise", grad[-1:], g["dnoise"]),
                       ("woodbury_vector", m.posterior.woodbury_vector, g["woodbury_vector"])):
        figs[name] = _rel(x, y)
    # the columns no part sees carry the KL term alone
    if rest:
        assert np.allclose(gm[:, rest], -g["mu"][:, rest], rtol=1e-15) and np.allclose(gs[:, rest], -0.5 * (1 - 1 / g["S"][:, rest]), rtol=1e-15)
        assert not dZ[:, rest].any()
    qn = gpy_amd.NormalPosterior(g["Xs"], g["Ss"])
    um, uv = m.predict_noiseless(qn)
    pm, pv = m.predict_noiseless(g["Xs"])
    figs.update(upred_mu=_rel(um, g["upred_mu"]), upred_var=_rel(uv, g["upred_var"]), pred_mu=_rel(pm, g["pred_mu"]),
                pred_var=_rel(pv, g["pred_var"]))
    print(os.path.basename(path), {k_: "%.2e" % v for k_, v in figs.items()})
    assert figs.pop("bound") <= TOL_LML and figs.pop("objective") <= TOL_LML
    assert figs.pop("upred_var") <= TOL_VAR and figs.pop("pred_var") <= TOL_VAR
    for name, e in figs.items():
        assert e <= TOL_FIT, (name, e)
    assert uv.min() > 1e-3                                  # nothing at the clip
    ym, yv = m.predict(qn)                                  # with the likelihood: the noise variance on top
    assert np.array_equal(ym, um) and np.allclose(yv, uv + float(g["noise"]), rtol=1e-14)


_edge = {}


def _edge_case(c):
    """one fit on the device per shape; the long-double prediction GIVEN the device's woodbury_vector / woodbury_inv, once"""
    if c not in _edge:
        p = B.edge_problem(c)
        ctx, r = _fit(p)
        wv, Wi = r["woodbury_vector"], ctx.fetch(ctx.FETCH_WOODBURY_INV)
        ref = B.predict_uncertain(p["var"], p["ls"], p["white"], p["Z"], wv, Wi, p["mu_new"], p["S_new"], LD, clip=False)
        for a in ref[:2]:
            a.setflags(write=False)
        _edge[c] = (p, ctx, ref)
    return _edge[c]


@pytest.mark.parametrize("c", B.EDGE_CASES, ids=B.edge_id)
def test_psi2n_contract_matches_the_long_double_restatement(c):
    """Bound: mean 4.2e-15, variance 1.3e-14 relative to psi0* (ten times the float64 restatement's distance from long double,
    tests/test_oracle_bgplvm.py).  Device, worst over the cases: mean 4.9e-16 (M33_Mn17_Q2_Dy4), variance 1.8e-15 (M17_Mn33_Q20_Dy1)."""
    p, ctx, (mean, var, psi0) = _edge_case(c)
    gm, gv = ctx.predict_uncertain(_specs(p), p["mu_new"], p["S_new"])
    assert gm.shape == gv.shape == (c[1], c[3])
    em, ev = _rel(gm, mean, scale=psi0), _rel(gv, var, scale=psi0)
    print(B.edge_id(c), "mean %.2e (bound %.2e)  variance %.2e (bound %.2e)  min variance %.3e" % (em, TOL_PRED_MEAN, ev, TOL_PRED_VAR,
                                                                                                 float(var.min())))
    assert var.min() > 1e-6 and gv.min() > 1e-6             # no variance is clipped
    assert em <= TOL_PRED_MEAN
    assert ev <= TOL_PRED_VAR
    gm2, none = ctx.predict_uncertain(_specs(p), p["mu_new"], p["S_new"], want_var=False)
    assert none is None and np.array_equal(gm2, gm)


def test_two_predictions_in_fresh_contexts_give_identical_bits_across_a_chunk_boundary():
    p = B.edge_problem((8, 2051, 2, 3, (0.3,)))
    out = []
    for _ in range(2):
        ctx, _r = _fit(p)
        out.append(ctx.predict_uncertain(_specs(p), p["mu_new"], p["S_new"]))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    again = ctx.predict_uncertain(_specs(p), p["mu_new"], p["S_new"])      # and twice in one context
    assert np.array_equal(again[0], out[1][0]) and np.array_equal(again[1], out[1][1])


def test_prediction_after_a_certain_input_fit_uses_its_posterior():
    p = B.edge_problem((17, 65, 2, 3, (0.3,)))
    ctx = _lib.SparseContext(0)
    ctx.set_data(p["mu"], p["Y"])
    rc, r = ctx.vardtc_sum(_specs(p), p["Z"], p["noise"])
    assert rc == 0
    wv, Wi = r["woodbury_vector"], ctx.fetch(ctx.FETCH_WOODBURY_INV)
    mean, var, psi0 = B.predict_uncertain(p["var"], p["ls"], p["white"], p["Z"], wv, Wi, p["mu_new"], p["S_new"], LD)
    gm, gv = ctx.predict_uncertain(_specs(p), p["mu_new"], p["S_new"])
    assert _rel(gm, mean, scale=psi0) <= TOL_PRED_MEAN and _rel(gv, var, scale=psi0) <= TOL_PRED_VAR
    # vanishing input variance: the certain-input prediction of the same posterior
    cm, cv = ctx.predict(_specs(p), p["mu_new"])
    zm, zv = ctx.predict_uncertain(_specs(p), p["mu_new"], np.full_like(p["S_new"], 1e-14))
    assert np.allclose(zm, cm, rtol=1e-9, atol=1e-11) and np.allclose(zv, np.broadcast_to(cv, zv.shape), rtol=1e-8, atol=1e-10)


@pytest.mark.parametrize("white", [False, True], ids=["rbf_ard", "rbf_white"])
def test_checkgrad(white):
    import gpy_amd
    np.random.seed(5 + white)
    N, Q, Dy, M = 30, 2, 3, 6
    t = np.random.uniform(-2, 2, (N, Q))
    Y = np.sin(t @ np.random.randn(Q, Dy)) + 0.05 * np.random.randn(N, Dy)
    k = gpy_amd.RBF(Q, ARD=True)
    if white:
        k = k + gpy_amd.White(Q, variance=0.1)
    m = gpy_amd.BayesianGPLVM(Y, Q, num_inducing=M, kernel=k)
    assert m.checkgrad(verbose=True)
    pos = np.concatenate([np.full(p.size, bool(p.positive)) for p in m.flattened_parameters()])
    draw = np.random.randn(pos.size)
    m.param_array = np.where(pos, np.log1p(np.exp(draw)), draw)            # as `m.randomize()` does in the reference's tests
    assert m.checkgrad(verbose=True)


def test_set_inputs_gives_the_bits_of_a_fresh_context_and_refuses_by_name():
    p = B.edge_problem((17, 65, 2, 3, (0.3,)))
    r = np.random.default_rng(3)
    mu2, S2 = p["mu"] + 0.1 * r.standard_normal(p["mu"].shape), p["S"] * r.uniform(0.5, 1.5, p["S"].shape)
    ctx, first = _fit(p)
    ctx.set_inputs(mu2, S2)
    with pytest.raises(_lib.MI355GPError, match="no result yet"):         # the last result is forgotten
        ctx.predict_uncertain(_specs(p), p["mu_new"], p["S_new"])
    rc, a = ctx.vardtc_uncertain(_specs(p), p["Z"], p["noise"])
    _, b = _fit(p, mu2, S2)
    assert rc == 0 and a["lml"] == b["lml"] != first["lml"]
    for key in ("dtheta", "dZ", "dmu", "dS", "woodbury_vector"):
        assert np.array_equal(a[key], b[key]), key
    ctx.set_inputs(p["mu"])                                               # the means alone: the variances stay
    rc, c = ctx.vardtc_uncertain(_specs(p), p["Z"], p["noise"])
    _, d = _fit(p, p["mu"], S2)
    assert c["lml"] == d["lml"] and np.array_equal(c["dS"], d["dS"])
    with pytest.raises(_lib.MI355GPError, match="N x D"):
        ctx.set_inputs(mu2[:-1], S2[:-1])
    with pytest.raises(_lib.MI355GPError, match="N x D"):
        ctx.set_inputs(mu2[:, :1], S2[:, :1])
    bad = S2.copy()
    bad[4, 1] = 0.0
    with pytest.raises(_lib.MI355GPError, match=r"S\[4\]\[1\]"):
        ctx.set_inputs(mu2, bad)
    fresh = _lib.SparseContext(0)
    with pytest.raises(_lib.MI355GPError, match="set_data first"):
        fresh.set_inputs(mu2, S2)
    sh = _lib.SparseContext(0)
    sh.attach_loopback(0, 1, 7701)
    sh.set_data(p["mu"], p["Y"])
    with pytest.raises(_lib.MI355GPError, match="row-sharded"):
        sh.set_inputs(mu2, S2)
    rc, e = ctx.vardtc_uncertain(_specs(p), p["Z"], p["noise"])          # the context is still good, its inputs unchanged
    assert rc == 0 and e["lml"] == c["lml"]


def test_predict_uncertain_refuses_by_name_and_the_context_still_predicts():
    import gpy_amd
    p = B.edge_problem((17, 65, 2, 3, (0.3,)))
    specs = _specs(p)
    ctx = _lib.SparseContext(0)
    ctx.set_data(p["mu"], p["Y"])
    with pytest.raises(_lib.MI355GPError, match="no result yet"):
        ctx.predict_uncertain(specs, p["mu_new"], p["S_new"])
    ctx.set_input_variance(p["S"])
    rc, r = ctx.vardtc_uncertain(specs, p["Z"], p["noise"])
    assert rc == 0
    good = ctx.predict_uncertain(specs, p["mu_new"], p["S_new"])

    def still_predicts():
        again = ctx.predict_uncertain(specs, p["mu_new"], p["S_new"])
        assert np.array_equal(again[0], good[0]) and np.array_equal(again[1], good[1])
    bad = p["S_new"].copy()
    bad[5, 1] = -0.5
    with pytest.raises(_lib.MI355GPError, match=r"S\[5\]\[1\]"):
        ctx.predict_uncertain(specs, p["mu_new"], bad)
    still_predicts()
    for other, pat in (([specs[0], ("bias", False, np.array([0.5]), None, 0)], "Bias"),
                       ([("matern52", True, np.array([1.0, 1.0, 1.0]), None, 0)], "Matern52"),
                       ([specs[0], specs[0]], "both RBF"), ([specs[0][:4] + (1,), specs[0][:4] + (1,)], "product"),
                       ([specs[1]], "no RBF part")):
        with pytest.raises(_lib.MI355GPError, match=pat):
            ctx.predict_uncertain(other, p["mu_new"], p["S_new"])
        still_predicts()
    # after an SVGP call the context describes an SVGP result (SVGP takes certain inputs: a context without variances)
    cs = _lib.SparseContext(0)
    cs.set_data(p["mu"], p["Y"])
    rc, _r = cs.vardtc_sum(specs, p["Z"], p["noise"])
    assert rc == 0
    before = cs.predict_uncertain(specs, p["mu_new"], p["S_new"])
    M = p["Z"].shape[0]
    info, _fw = cs.svgp_forward(specs, p["Z"], np.zeros((M, 1)), np.eye(M)[None], extra_jitter=1e-6)
    assert info == 0
    with pytest.raises(_lib.MI355GPError, match="SVGP"):
        cs.predict_uncertain(specs, p["mu_new"], p["S_new"])
    rc, _r = cs.vardtc_sum(specs, p["Z"], p["noise"])
    assert rc == 0 and np.array_equal(cs.predict_uncertain(specs, p["mu_new"], p["S_new"])[1], before[1])
    # a row-sharded context
    sh = _lib.SparseContext(0)
    sh.attach_loopback(0, 1, 7702)
    sh.set_data(p["mu"], p["Y"])
    rc, _r = sh.vardtc_sum(specs, p["Z"], p["noise"])
    assert rc == 0
    with pytest.raises(_lib.MI355GPError, match="row-sharded"):
        sh.predict_uncertain(specs, p["mu_new"], p["S_new"])
    assert np.isfinite(sh.predict(specs, p["mu_new"])[0]).all()
    # the model: full_cov at uncertain points is refused as in the reference
    m = gpy_amd.BayesianGPLVM(p["Y"], 2, X=p["mu"], X_variance=p["S"], Z=p["Z"])
    with pytest.raises(NotImplementedError, match="Full covariance"):
        m.predict(gpy_amd.NormalPosterior(p["mu_new"], p["S_new"]), full_cov=True)


def test_a_short_optimisation_lowers_the_objective_and_keeps_the_variances_positive():
    import gpy_amd
    Y, labels, _t = B.example_data()
    np.random.seed(1)
    m = gpy_amd.BayesianGPLVM(Y, 5, num_inducing=15)
    f0 = m.objective_function()
    m.optimize(max_iters=20)
    assert np.isfinite(m.objective_function()) and m.objective_function() < f0
    assert np.all(m.X.variance.values > 0) and np.all(np.isfinite(m.X.mean.values))
    mu, var = m.predict(m.X)                                # at the latent posteriors themselves
    assert mu.shape == var.shape == Y.shape and np.all(var > 0)
    f = m.posterior_samples_f(m.X.mean.values[:4], size=3)
    assert f.shape == (4, Y.shape[1], 3)
