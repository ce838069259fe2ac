"""GPU (-m gpu): the FITC / PEP device path -- mi355gp_pep_inference with its two row kernels, the whitened tile GEMMs, the
split-K Gram and the signed weighted Gram, and mi355gp_sparse_predict / _fetch / _fetch_dLdKnm on its result.

Fixtures (tests/golden/pep, the reference's own FITC.inference / PEP.inference): every one through the classes and through
`SparseGP`, at the tolerances tests/test_gpu_sparse.py holds VarDTC's fixtures to: log marginal 1e-9, gradients 1e-6, dL_dKmm and
woodbury_inv 1e-4, prediction mean 1e-6, variance and covariance 1e-5.

Shape edges, judged against the long-double restatement tests/pep_np.py by `sparse_ld.bound`: err(q) <= max(32 e64(q),
256 eps64 kappa), e64 = the distance of the fp64 restatement from long double on the same input (never the device's figure),
kappa = cond2(Kmm + 1e-6 I).  Judged per case: lml, dtheta, dnoise, dZ, woodbury_vector, woodbury_inv, dL_dKmm, a block of
dL_dKnm rows, and the prediction (mean, variance, covariance) at 1 and at 129 points.  Families (pep_np.CASES):
    m_edge    N = 257, D = 2, alpha = 1: M = 1 | 127 (tile padding) | 128 | 129 (first persistent Kmm launch) | 257 (three tiles)
    n_edge    M = 65, D = 3, alpha = 0.5: N = 1 | 2 | 127 | 128 | 129 | 255 | 256 | 257 | 2049; N < M on purpose
    d_edge    N = 193, M = 65: D = 1 | 16 (fused gradient pass) | 17 (unfused) | 32 | 33 (two ARD groups)
    alpha     1 | 0.5 | 0.05 on matern32_ard
    kernels   rbf + white (a sum), rbf x matern32 + white (a product), rbf_ard on columns 0 and 2 of three
    chunks    N = 262145 at M = 128 and M = 65 (a product), against the blocked reference; the dL_dKnm block straddles the chunk
              boundary
Stale state: PEP -> VarDTC -> PEP with different M, and PEP -> SVGP -> PEP, on one context without set_data between; every
result equals that of a fresh context byte for byte.  Determinism: two calls give the same bytes for every output.  Refusals
reach the caller with the device's message.  The model: the toy optimisation, checkgrad, predict and posterior_samples_f.

Measured on an MI355X, worst err(q) per family (never a reason to tighten a bound; wv = woodbury_vector, Winv = woodbury_inv,
dKnm = the dL_dKnm block; err/bound = the worst ratio of a figure to its bound over the family; kappa <= 92, no bound above 5.2e-12):

    family        lml  dtheta  dnoise      dZ      wv    Winv    dKmm    dKnm   mu129  var129  cov129     mu1    var1    cov1  err/bound
    m_edge      2e-15   4e-15   4e-15   4e-14   1e-14   6e-15   2e-14   2e-14   6e-15   3e-15   3e-15   2e-15   9e-15   1e-14      0.083
    n_edge      2e-15   1e-14   2e-16   8e-15   2e-15   7e-15   2e-14   4e-15   3e-15   1e-15   2e-15   5e-14   2e-15   2e-15      0.050
    d_edge      4e-15   2e-15   4e-15   9e-14   9e-15   5e-15   2e-14   7e-15   4e-15   6e-15   6e-15   4e-14   1e-14   2e-14      0.113
    alpha       7e-16   9e-16   5e-16   8e-15   2e-15   2e-15   4e-15   3e-15   2e-15   1e-15   1e-15   2e-15   3e-16   4e-16      0.010
    kernels     7e-16   3e-15   5e-16   4e-14   2e-14   5e-15   1e-14   1e-14   3e-15   5e-15   5e-15   5e-15   4e-15   4e-15      0.012
    chunks      5e-14   4e-15   2e-14   1e-13   2e-14   3e-15   7e-14   2e-14   9e-15   5e-15   6e-15   4e-15   1e-13   1e-13      0.054
    stale       6e-16   6e-15   2e-15   1e-14   2e-15   3e-15   7e-15   7e-15   3e-15   1e-15   2e-15   3e-15   1e-15   2e-15      0.007

Against the fixtures the classes are within 2.2e-12 (the log marginal of the D = 1 fixture, 0.31 as a sum of terms of 1e2; every
other figure is below 5e-13).  The whole file: 39 cases, about 16 s of wall time, most of it the long-double references of the two
262145-row cases.
"""
import os

import numpy as np
import pytest

import kern_ld as KL
import pep_np as P

pytestmark = pytest.mark.gpu
need_ld = pytest.mark.skipif(not KL.HAVE_LD, reason="np.longdouble is not an extended format on this host")


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def device_eval(ctx, c, set_data=True, M=None):
    """everything the judge names, from the device"""
    from gpy_amd import _lib
    C = _lib.SparseContext
    if set_data:
        ctx.set_data(c["X"], c["Y"])
    info, r = ctx.pep(c["specs"], c["Z"], c["noise"], c["alpha"], P.JITTER)
    assert info == 0
    got = dict(lml=r["lml"], dtheta=r["dtheta"], dnoise=r["dnoise"], dZ=r["dZ"], woodbury_vector=r["woodbury_vector"], dL_dR=r["dL_dR"])
    r0, nr = c["block"]
    got["dL_dKnm_block"] = ctx.fetch_dL_dKnm(r0, nr)
    got["dL_dKmm"] = ctx.fetch(C.FETCH_DLDKMM)
    got["woodbury_inv"] = ctx.fetch(C.FETCH_WOODBURY_INV)
    got["Lm"], got["Kmm"] = ctx.fetch(C.FETCH_LM), ctx.fetch(C.FETCH_KMM)
    for tag in ("1", "129"):
        got["mu" + tag], got["var" + tag] = ctx.predict(c["specs"], c["Xs" + tag])
        got["cov" + tag] = ctx.predict(c["specs"], c["Xs" + tag], full_cov=True)[1]
    return got


def judged(name, got):
    c, ref, r64, kappa = P.reference(name)
    figs, bad = P.judge(got, ref, r64, kappa)
    print("%-44s kappa %8.1f  " % (name, kappa) + "  ".join("%s %.1e/%.1e" % (q, e, b) for q, (e, b) in figs.items()))
    assert not bad, "%s: %s" % (name, "; ".join(bad))
    assert set(figs) == set(P.JUDGED)
    # Kmm carries THIS family's jitter (1e-6, not VarDTC's 1e-8), dL_dKmm is symmetric
    assert P.rel_err(got["Kmm"], KL.f64(ref["Kmm"])) <= 1e-12
    assert np.abs(got["dL_dKmm"] - got["dL_dKmm"].T).max() <= 1e-13 * np.abs(got["dL_dKmm"]).max()
    return figs


@pytest.fixture(scope="module")
def ctx():
    from gpy_amd import _lib
    c = _lib.SparseContext(0)
    yield c
    c.close()


@need_ld
@pytest.mark.parametrize("name", [n for n in P.PLAIN if n not in P.STALE])
def test_shape_edges(ctx, name):
    c = P.reference(name)[0]
    judged(name, device_eval(ctx, c))


@need_ld
@pytest.mark.parametrize("name", P.BLOCKED)
def test_several_chunks(name):
    from gpy_amd import _lib
    c = P.reference(name)[0]
    ctx = _lib.SparseContext(0)
    try:
        judged(name, device_eval(ctx, c))
    finally:
        ctx.close()


def _same_bytes(a, b):
    for q in a:
        assert np.asarray(a[q]).tobytes() == np.asarray(b[q]).tobytes(), q


def _fresh(c):
    from gpy_amd import _lib
    ctx = _lib.SparseContext(0)
    try:
        return device_eval(ctx, c)
    finally:
        ctx.close()


@need_ld
def test_stale_state_pep_vardtc_pep_and_pep_svgp_pep():
    """one context, no set_data between: PEP (M = 129) -> VarDTC (M = 65) -> PEP (M = 65) -> SVGP (M = 65) -> PEP (M = 129); every
    PEP result is judged and equals a fresh context's byte for byte, and so does VarDTC's after PEP"""
    from gpy_amd import _lib
    a, b = (P.reference(n)[0] for n in P.STALE)
    assert np.array_equal(a["X"], b["X"]) and np.array_equal(a["Y"], b["Y"]) and a["M"] != b["M"]
    fresh_a, fresh_b = _fresh(a), _fresh(b)
    v = _lib.SparseContext(0)
    v.set_data(b["X"], b["Y"])
    info, fresh_v = v.vardtc_sum(b["specs"], b["Z"], b["noise"])
    fresh_v = dict(fresh_v, dL_dKnm=v.fetch_dL_dKnm(0, 257), psi2=v.fetch(4), dL_dKmm=v.fetch(0), Kmm=v.fetch(3))
    fresh_v.pop("dL_dm")
    v.close()
    ctx = _lib.SparseContext(0)
    got = device_eval(ctx, a)
    _same_bytes(got, fresh_a)
    judged(P.STALE[0], got)
    info, rv = ctx.vardtc_sum(b["specs"], b["Z"], b["noise"])                      # VarDTC after PEP: VarDTC's rows, psi2, 1e-8 jitter
    assert info == 0
    rv = dict(rv, dL_dKnm=ctx.fetch_dL_dKnm(0, 257), psi2=ctx.fetch(4), dL_dKmm=ctx.fetch(0), Kmm=ctx.fetch(3))
    rv.pop("dL_dm")
    _same_bytes(rv, fresh_v)
    got = device_eval(ctx, b, set_data=False)                                      # PEP after VarDTC
    _same_bytes(got, fresh_b)
    judged(P.STALE[1], got)
    with pytest.raises(_lib.MI355GPError, match="does not exist for a PEP"):
        ctx.fetch(4)
    M = b["M"]
    info, fw = ctx.svgp_forward(b["specs"], b["Z"], np.zeros((M, 1)), np.eye(M)[None])
    assert info == 0
    ctx.svgp_backward(np.ones((257, 1)), -0.5 * np.ones((257, 1)))
    with pytest.raises(_lib.MI355GPError, match="SVGP call"):
        ctx.fetch_dL_dKnm(0, 8)
    _same_bytes(device_eval(ctx, a, set_data=False), fresh_a)                      # PEP after SVGP
    ctx.close()


@need_ld
def test_two_calls_give_the_same_bytes():
    c = P.reference(P.DETERMINISM)[0]
    _same_bytes(_fresh(c), _fresh(c))


@need_ld
def test_refusals_reach_the_caller_with_the_devices_message():
    from gpy_amd import _lib
    c = P.reference("alpha-matern32_ard-n257_m65_d3-a0.5")[0]
    ctx = _lib.SparseContext(0)
    ctx.set_data(c["X"], np.hstack([c["Y"], c["Y"]]))
    with pytest.raises(_lib.MI355GPError, match="2 output columns"):
        ctx.pep(c["specs"], c["Z"], c["noise"], 0.5, P.JITTER)
    ctx.set_data(c["X"], c["Y"])
    for alpha in (0.0, 1.5):
        with pytest.raises(_lib.MI355GPError, match=r"outside \(0, 1\]"):
            ctx.pep(c["specs"], c["Z"], c["noise"], alpha, P.JITTER)
    ctx.set_input_variance(np.full(c["X"].shape, 0.01))
    with pytest.raises(_lib.MI355GPError, match="input variances"):
        ctx.pep(c["specs"], c["Z"], c["noise"], 0.5, P.JITTER)
    sh = _lib.SparseContext(0)
    sh.attach_loopback(0, 1, 4343)
    sh.set_data(c["X"], c["Y"])
    with pytest.raises(_lib.MI355GPError, match="row-sharded"):
        sh.pep(c["specs"], c["Z"], c["noise"], 0.5, P.JITTER)
    sh.close()
    # and the context still works after all that
    ctx.set_data(c["X"], c["Y"])
    judged(c["name"], device_eval(ctx, c, set_data=False))
    ctx.close()


# ---- the reference's fixtures through the classes and through SparseGP ------------------------------------------------------------
@pytest.mark.parametrize("name", P.FIXTURES)
def test_classes_and_model_against_reference_fixture(name):
    import gpy_amd
    from svgp_np import make_kernel
    fx = P.load_fixture(name)
    kern, lik = make_kernel(fx), gpy_amd.Gaussian(variance=fx["noise"])
    post, lml, gd = P.make_inference(fx).inference(kern, fx["X"], fx["Z"], lik, fx["Y"])
    figs = dict(lml=abs(lml - fx["lml"]) / abs(fx["lml"]), dtheta=_rel(gd["fused"]["dtheta"], fx["dtheta"]),
                dZ=_rel(gd["fused"]["dZ"], kern._slice_X(fx["dZ"])), dL_dthetaL=_rel(gd["dL_dthetaL"], fx["dL_dthetaL"]),
                dL_dKdiag=_rel(gd["dL_dKdiag"], fx["dL_dKdiag"]), dL_dKnm=_rel(np.asarray(gd["dL_dKnm"]), fx["dL_dKnm"]),
                woodbury_vector=_rel(post.woodbury_vector, fx["woodbury_vector"]),
                dL_dKmm=_rel(np.asarray(gd["dL_dKmm"]), fx["dL_dKmm"]), woodbury_inv=_rel(np.asarray(post.woodbury_inv), fx["woodbury_inv"]))
    mu, var = post._raw_predict(kern, fx["Xs"], fx["Z"])
    _, cov = post._raw_predict(kern, fx["Xs"], fx["Z"], full_cov=True)
    figs.update(pred_mu=_rel(mu, fx["pred_mu"]), pred_var=_rel(var, fx["pred_var"]), pred_cov=_rel(cov, fx["pred_cov"]))
    print(name, "  ".join("%s %.1e" % kv for kv in figs.items()))
    assert figs["lml"] <= 1e-9
    for q in ("dtheta", "dZ", "dL_dthetaL", "dL_dKdiag", "dL_dKnm", "woodbury_vector", "pred_mu"):
        assert figs[q] <= 1e-6, q
    for q in ("dL_dKmm", "woodbury_inv"):
        assert figs[q] <= 1e-4, q
    assert figs["pred_var"] <= 1e-5 and figs["pred_cov"] <= 1e-5
    # the model: flat order [Z, kernel, noise]
    m = gpy_amd.core.SparseGP(fx["X"], fx["Y"], fx["Z"], make_kernel(fx), gpy_amd.Gaussian(variance=fx["noise"]),
                              inference_method=P.make_inference(fx))
    assert abs(m.log_likelihood() - fx["lml"]) <= 1e-9 * abs(fx["lml"])
    nz = fx["Z"].size
    g = m.gradient
    assert g.size == nz + fx["dtheta"].size + 1
    assert _rel(g[:nz], fx["dZ"].ravel()) <= 1e-6 and _rel(g[nz:-1], fx["dtheta"]) <= 1e-6 and _rel(g[-1:], fx["dL_dthetaL"]) <= 1e-6
    mu, var = m._raw_predict(fx["Xs"])
    _, cov = m._raw_predict(fx["Xs"], full_cov=True)
    assert _rel(mu, fx["pred_mu"]) <= 1e-6 and _rel(var, fx["pred_var"]) <= 1e-5 and _rel(cov, fx["pred_cov"]) <= 1e-5


def test_toy_fitc_optimizes_to_the_reference_log_marginal():
    """1-D toy: `optimize()` raises the FITC log marginal; the end value is at least the reference's (40 L-BFGS-B iterations from the
    same start, stored by tools/make_golden_pep.py) minus 1e-3 of its size.  checkgrad passes; predict, predict_noiseless and
    posterior_samples_f return finite arrays of the right shapes."""
    import gpy_amd
    t = dict(np.load(os.path.join(P.GOLDEN, "toy_fitc.npz")))
    th = t["theta0"]
    m = gpy_amd.core.SparseGP(t["X"], t["Y"], t["Z0"], gpy_amd.RBF(1, variance=th[0], lengthscale=th[1]), gpy_amd.Gaussian(variance=th[2]),
                              inference_method=gpy_amd.FITC())
    l0 = m.log_likelihood()
    assert abs(l0 - float(t["lml_start"])) <= 1e-9 * abs(float(t["lml_start"]))
    np.random.seed(3)
    assert m.checkgrad()
    m.optimize(max_iters=int(t["maxiter"]))
    l1 = m.log_likelihood()
    print("toy: log marginal %.6f -> %.6f (reference %.6f -> %.6f)" % (l0, l1, float(t["lml_start"]), float(t["lml_end"])))
    assert l1 > l0
    assert l1 >= float(t["lml_end"]) - 1e-3 * abs(float(t["lml_end"]))
    assert m.checkgrad()
    Xs = np.linspace(0.0, 1.0, 33)[:, None]
    for mu, var in (m.predict(Xs), m.predict_noiseless(Xs)):
        assert mu.shape == (33, 1) and var.shape == (33, 1) and np.all(np.isfinite(mu)) and np.all(np.isfinite(var)) and np.all(var > 0)
    f = m.posterior_samples_f(Xs, size=5)
    assert f.shape == (33, 1, 5) and np.all(np.isfinite(f))
