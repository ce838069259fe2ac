"""CPU: FITC / PEP against the reference's own numbers, without a GPU.

1.  The fp64 restatement tests/pep_np.py meets every fixture of tests/golden/pep (the reference's FITC.inference / PEP.inference,
    the gradient assembly of sparse_gp.py:108-119 and Posterior._raw_predict) under the project's rule `sparse_ld.bound`:
    err(q) <= max(32 e64(q), 256 eps64 kappa), e64 = the distance of the fp64 restatement from the long-double one on the fixture's
    input, kappa = cond2(Kmm + 1e-6 I).  Measured: the worst err / bound over all fixtures and quantities is 0.66 (lml of
    fitc_rbf_iso_n200_m10_d1, 1.8e-12 against 2.8e-12: the log marginal is 0.31 there, a sum of terms of size 1e2); every other
    figure is at most 0.26 of its bound (dL_dKdiag of fitc_rbf_x_matern32, 6.7e-14 against 2.6e-13, kappa = 3.1).
2.  The restatement's gradient is the gradient of its log marginal (central differences).
3.  `PEP(1.0)` and `FITC()` give identical results.
4.  The classes and `SparseGP`, driven over a stand-in for `_lib.SparseContext` that answers with the restatement
    (`pep_np.RestatementContext`; the pattern of tests/test_svgp_host.py): the fixture's numbers, the flat parameter order
    [Z, kernel, noise], every refusal by name before a context is made, the jitter ladder.
5.  The host's check of sigma* (`mi355gp_pep_check_sigma`, the function the device call runs between its passes) names the row.
6.  The reference's import paths.
"""
import numpy as np
import pytest

import gpy_amd
import kern_ld as KL
import pep_np as P
from gpy_amd import _lib
from svgp_np import make_kernel

need_ld = pytest.mark.skipif(not KL.HAVE_LD, reason="np.longdouble is not an extended format on this host")


@need_ld
@pytest.mark.parametrize("name", P.FIXTURES)
def test_fp64_restatement_meets_the_reference_fixture(name):
    fx = P.load_fixture(name)
    r64, rld = P.restate_fixture(fx), P.restate_fixture(fx, dt=P.LD)
    kappa = float(np.linalg.cond(KL.f64(rld["Kmm"])))
    assert abs(kappa - float(fx["cond_Kmm"])) <= 1e-6 * kappa
    bad = []
    for q in P.FIXTURE_QUANTITIES:
        ref = np.asarray(fx[q])
        a64, ald = np.asarray(r64[q]).reshape(ref.shape), np.asarray(rld[q]).reshape(ref.shape)
        e, b = P.rel_err(a64, ref), max(32.0 * P.rel_err(a64, ald), 256.0 * KL.EPS64 * kappa)
        print("FIG %s %s %.2e (bound %.2e)" % (name, q, e, b))
        if not e <= b:
            bad.append("%s: %.3e > %.3e" % (q, e, b))
    assert not bad, bad


def _flat(fx):
    return np.concatenate([fx["Z"].ravel()] + [s[2] for s in fx["specs"]] + [[fx["noise"]]])


def _eval_flat(fx, x):
    nz = fx["Z"].size
    Z, o, specs = x[:nz].reshape(fx["Z"].shape), nz, []
    for s in fx["specs"]:
        specs.append((s[0], s[1], x[o:o + s[2].size], s[3], s[4]))
        o += s[2].size
    return P.pep(specs, fx["X"], Z, fx["Y"], x[o], fx["alpha"], dt=np.float64)


@pytest.mark.parametrize("name", ["fitc_matern52_ard_n250_m36_d3", "pep_alpha05_rbf_ard_n240_m32_d3",
                                  "pep_alpha01_rbf_white_bias_n160_m24_d2"])
def test_restatement_gradient_against_finite_differences(name):
    """The directional derivative of the restatement's log marginal along six random unit directions of (Z, theta, noise) and
    along each group on its own, by central differences with h = 1e-6, against its gradient.  With |log marginal| <= 4e2 the
    rounding error of a difference is a few eps |lml| kappa / h <= 1e-6 (kappa <= 65) and the truncation h^2 |d3| / 6 is smaller;
    the gradient norms are 1e1 ... 1e4, so the bound is 1e-6 of the gradient's norm plus that 1e-6 (the argument of
    tests/test_svgp_host.py's checkgrad test).  dZ columns that no part sees carry a zero gradient and a zero difference."""
    fx = P.load_fixture(name)
    x0 = _flat(fx)
    r = _eval_flat(fx, x0)
    g = np.concatenate([KL.f64(r["dZ"]).ravel(), KL.f64(r["dtheta"]), [float(r["dnoise"])]])
    assert g.shape == x0.shape
    nz, nk = fx["Z"].size, fx["dtheta"].size
    rng = np.random.default_rng(2)
    dirs = [rng.standard_normal(x0.size) for _ in range(6)]
    for lo, hi in ((0, nz), (nz, nz + nk), (nz + nk, nz + nk + 1)):
        d = np.zeros(x0.size)
        d[lo:hi] = rng.standard_normal(hi - lo)
        dirs.append(d)
    h = 1e-6
    for d in dirs:
        d = d / np.linalg.norm(d)
        num = (float(_eval_flat(fx, x0 + h * d)["lml"]) - float(_eval_flat(fx, x0 - h * d)["lml"])) / (2 * h)
        assert abs(num - g @ d) <= 1e-6 * np.linalg.norm(g[d != 0]) + 1e-6, (num, g @ d)


# ---- the classes over a restatement-backed stand-in context ---------------------------------------------------------------------
@pytest.fixture
def rctx(monkeypatch):
    made = []

    class Ctx(P.RestatementContext):
        def __init__(self, device=0):
            super(Ctx, self).__init__(device)
            made.append(self)
    monkeypatch.setattr(_lib, "SparseContext", Ctx)
    return made


BOUND = 1e-10        # the classes against the fixtures: the restatement's own distance (test 1, at most 3.8e-12) with room for none else


@pytest.mark.parametrize("name", P.FIXTURES)
def test_inference_returns_the_reference_grad_dict(rctx, name):
    fx = P.load_fixture(name)
    kern = make_kernel(fx)
    post, lml, gd = P.make_inference(fx).inference(kern, fx["X"], fx["Z"], gpy_amd.Gaussian(variance=fx["noise"]), fx["Y"])
    assert P.rel_err(lml, fx["lml"]) <= BOUND
    assert sorted(gd) == ["dL_dKdiag", "dL_dKmm", "dL_dKnm", "dL_dthetaL", "fused"]             # pep.py:88 (+ the device's reductions)
    for q, got in (("dL_dKdiag", gd["dL_dKdiag"]), ("dtheta", gd["fused"]["dtheta"]), ("dL_dthetaL", np.atleast_1d(gd["dL_dthetaL"])),
                   ("dL_dKmm", np.asarray(gd["dL_dKmm"])), ("dL_dKnm", np.asarray(gd["dL_dKnm"])),
                   ("woodbury_vector", post.woodbury_vector), ("woodbury_inv", np.asarray(post.woodbury_inv))):
        assert np.shape(got) == fx[q].shape and P.rel_err(got, fx[q]) <= BOUND, q
    assert P.rel_err(gd["fused"]["dZ"], kern._slice_X(fx["dZ"])) <= BOUND
    # what went to the device: the sliced X, one output column, the noise variance, alpha, const_jitter = 1e-6
    ctx = rctx[0]
    assert [c[0] for c in ctx.log[:2]] == ["set_data", "pep"]
    assert ctx.log[0][1:] == (kern._slice_X(fx["X"]).shape, (fx["X"].shape[0], 1))
    assert ctx.log[1][1:] == (kern._slice_X(fx["Z"]).shape, fx["noise"], fx["alpha"]) and ctx.jitters == [1e-6]
    # prediction through the posterior runs on the context while it is the latest result
    mu, var = post._raw_predict(kern, fx["Xs"], fx["Z"])
    _, cov = post._raw_predict(kern, fx["Xs"], fx["Z"], full_cov=True)
    assert ctx.log[-1][0] == "predict"
    assert P.rel_err(mu, fx["pred_mu"]) <= BOUND and P.rel_err(var, fx["pred_var"]) <= BOUND and P.rel_err(cov, fx["pred_cov"]) <= BOUND
    # a second call on the same data does not upload it again
    P.make_inference(fx)
    n_set = sum(c[0] == "set_data" for c in ctx.log)
    assert n_set == 1


def test_pep_alpha_one_is_fitc(rctx):
    fx = P.load_fixture("fitc_matern52_ard_n250_m36_d3")
    out = []
    for inf in (gpy_amd.FITC(), gpy_amd.PEP(1.0)):
        post, lml, gd = inf.inference(make_kernel(fx), fx["X"], fx["Z"], gpy_amd.Gaussian(variance=fx["noise"]), fx["Y"])
        out.append([np.asarray(v) for v in (lml, gd["dL_dKdiag"], gd["dL_dthetaL"], gd["fused"]["dtheta"], gd["fused"]["dZ"],
                                            gd["dL_dKmm"], gd["dL_dKnm"], post.woodbury_vector, post.woodbury_inv)])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*out))
    assert isinstance(gpy_amd.FITC(), gpy_amd.PEP) and gpy_amd.FITC().alpha == 1.0
    assert gpy_amd.FITC.const_jitter == gpy_amd.PEP.const_jitter == 1e-6 and gpy_amd.VarDTC.const_jitter == 1e-8


def test_sparse_gp_flat_parameter_order_and_gradient(rctx):
    fx = P.load_fixture("pep_alpha05_rbf_ard_n240_m32_d3")
    m = gpy_amd.core.SparseGP(fx["X"], fx["Y"], fx["Z"], make_kernel(fx), gpy_amd.Gaussian(variance=fx["noise"]),
                              inference_method=gpy_amd.PEP(0.5))
    names = [p.name for p in m.flattened_parameters()]
    assert names == ["inducing inputs", "variance", "lengthscale", "variance"]                  # sparse_gp.py:59: Z first
    nz, nk = fx["Z"].size, fx["dtheta"].size
    assert np.array_equal(m.param_array[:nz], fx["Z"].ravel()) and m.param_array[-1] == fx["noise"]
    assert P.rel_err(m.log_likelihood(), fx["lml"]) <= BOUND
    g = m.gradient
    assert g.size == nz + nk + 1
    assert P.rel_err(g[:nz], fx["dZ"].ravel()) <= BOUND and P.rel_err(g[nz:nz + nk], fx["dtheta"]) <= BOUND
    assert P.rel_err(g[-1:], fx["dL_dthetaL"]) <= BOUND
    mu, var = m.predict_noiseless(fx["Xs"])
    assert P.rel_err(mu, fx["pred_mu"]) <= BOUND and P.rel_err(var, fx["pred_var"]) <= BOUND
    np.random.seed(0)
    assert m.checkgrad()
    f = m.posterior_samples_f(fx["Xs"], size=3)
    assert f.shape == (7, 1, 3) and np.all(np.isfinite(f))
    # a new Z changes the result and keeps the data where it is
    x = m.param_array.copy()
    x[:nz] += 1e-3
    m.param_array = x
    assert m.log_likelihood() != fx["lml"] and sum(c[0] == "set_data" for c in rctx[0].log) == 1


def test_refusals_by_name_before_a_context_is_made(rctx):
    fx = P.load_fixture("fitc_rbf_white_bias_n180_m30_d2")
    k, lik = make_kernel(fx), gpy_amd.Gaussian(variance=fx["noise"])
    N = fx["X"].shape[0]
    for inf in (gpy_amd.FITC(), gpy_amd.PEP(0.5)):
        with pytest.raises(NotImplementedError, match="mean function"):
            inf.inference(k, fx["X"], fx["Z"], lik, fx["Y"], mean_function=object())
        het = gpy_amd.HeteroscedasticGaussian({"output_index": np.arange(N)[:, None]}, variance=0.1)
        with pytest.raises(NotImplementedError, match="per-point"):
            inf.inference(k, fx["X"], fx["Z"], het, fx["Y"], Y_metadata={"output_index": np.arange(N)[:, None]})
        with pytest.raises(NotImplementedError, match="NormalPosterior"):
            inf.inference(k, gpy_amd.NormalPosterior(fx["X"], np.full(fx["X"].shape, 0.1)), fx["Z"], lik, fx["Y"])
        with pytest.raises(NotImplementedError, match="2 output columns"):
            inf.inference(k, fx["X"], fx["Z"], lik, np.hstack([fx["Y"], fx["Y"]]))
        with pytest.raises(NotImplementedError, match="does not evaluate Linear kernels"):
            inf.inference(gpy_amd.Linear(2), fx["X"], fx["Z"], lik, fx["Y"])
        with pytest.raises(NotImplementedError, match="sparse path covers"):
            inf.inference(gpy_amd.White(2), fx["X"], fx["Z"], lik, fx["Y"])
    for alpha in (0.0, 1.5, -1.0):
        with pytest.raises(ValueError, match=r"outside \(0, 1\]"):
            gpy_amd.PEP(alpha).inference(k, fx["X"], fx["Z"], lik, fx["Y"])
    assert rctx == []                                                                          # no context was made
    inf = gpy_amd.FITC()
    inf.inference(k, fx["X"], fx["Z"], lik, fx["Y"])
    rctx[0].sharded = True
    with pytest.raises(NotImplementedError, match="row-sharded"):
        inf.inference(k, fx["X"], fx["Z"], lik, fx["Y"])
    # SparseGPRegression keeps its signature: the reference's takes no inference method
    with pytest.raises(TypeError):
        gpy_amd.SparseGPRegression(fx["X"], fx["Y"], inference_method=gpy_amd.FITC())


def test_the_jitter_ladder_retries_on_a_reported_info(rctx, monkeypatch):
    fx = P.load_fixture("fitc_rbf_iso_n200_m10_d1")
    k, lik = make_kernel(fx), gpy_amd.Gaussian(variance=fx["noise"])
    var = float(fx["specs"][0][2][0])
    monkeypatch.setattr(P.RestatementContext, "fail_infos", (3, 3))
    post, lml, gd = gpy_amd.FITC().inference(k, fx["X"], fx["Z"], lik, fx["Y"])
    assert np.allclose(rctx[0].jitters, [1e-6, 1e-6 + var * 1e-6, 1e-6 + var * 1e-5], rtol=1e-14, atol=0)   # util/linalg.py:61-75
    assert 0 < abs(lml - fx["lml"]) <= 0.05                  # evaluated with the larger jitter (the log marginal is 0.31, a sum of terms of 1e2)
    monkeypatch.setattr(P.RestatementContext, "fail_infos", (7,) * 6)
    with pytest.raises(gpy_amd.linalg.LinAlgError, match="not positive definite"):
        gpy_amd.FITC().inference(k, fx["X"], fx["Z"], lik, fx["Y"])
    assert np.allclose(rctx[1].jitters, [1e-6] + [1e-6 + var * 1e-6 * 10 ** i for i in range(5)], rtol=1e-14, atol=0)


def test_a_later_call_makes_the_lazy_results_stale(rctx):
    fx = P.load_fixture("fitc_rbf_iso_n200_m10_d1")
    k, lik, inf = make_kernel(fx), gpy_amd.Gaussian(variance=fx["noise"]), gpy_amd.FITC()
    post, _, gd = inf.inference(k, fx["X"], fx["Z"], lik, fx["Y"])
    kept = np.asarray(gd["dL_dKmm"]).copy()
    inf.inference(k, fx["X"], fx["Z"] + 1e-3, lik, fx["Y"])
    assert np.array_equal(np.asarray(gd["dL_dKmm"]), kept)                                     # fetched before: kept
    with pytest.raises(RuntimeError, match="overwritten by a later inference call"):
        np.asarray(gd["dL_dKnm"])


# ---- the host's check of sigma* --------------------------------------------------------------------------------------------------
def test_the_sigma_star_check_names_the_row():
    """In exact arithmetic sigma*_n = s2 + alpha (Knn_n - q_n) >= s2 > 0; with a noise variance of 1e-12 and a point on an inducing
    input (jitter 0) rounding decides its sign.  The device call hands every chunk's sigma* to this function between its passes;
    here it is called on the host alone."""
    check = _lib.lib().mi355gp_pep_check_sigma
    good = np.array([1e-12, 3.0, 0.5])
    assert check(good, good.size, 0, 1e-12, 1.0) == 0
    for bad_value in (-2.2e-16, 0.0, np.nan):
        s = np.concatenate([good, [bad_value], good, [-1.0]])
        assert check(s, s.size, 4096, 1e-12, 0.5) == -8
        msg = _lib.last_error()
        assert "row 4099" in msg and "not positive" in msg and "1e-12" in msg and "alpha 0.5" in msg, msg
    assert check(good, 0, 0, 1e-12, 1.0) == 0


def test_import_paths_of_the_reference():
    lfi = gpy_amd.inference.latent_function_inference
    assert lfi.FITC is gpy_amd.FITC and lfi.PEP is gpy_amd.PEP and lfi.fitc.FITC is gpy_amd.FITC and lfi.pep.PEP is gpy_amd.PEP
    assert gpy_amd.FITC().to_dict()["class"] == "GPy.inference.latent_function_inference.fitc.FITC"
    assert gpy_amd.PEP(0.3).to_dict() == {"class": "GPy.inference.latent_function_inference.pep.PEP", "alpha": 0.3}
    assert "mi355gp_pep_inference" in _lib.EXPORTED and "mi355gp_pep_check_sigma" in _lib.EXPORTED
