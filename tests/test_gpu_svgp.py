"""GPU (-m gpu): the SVGP device path -- mi355gp_svgp_forward / _backward / _predict with the row-reduction and weight-forming
kernels of gpy_amd/csrc/svgp.hip -- at every shape edge, judged against the long-double restatement tests/svgp_np.py (80-bit;
tests/test_oracle_svgp.py holds that restatement to the reference's own fixtures), and the model `gpy_amd.core.SVGP` against
reference fixtures.

Judge (svgp_np.judge = sparse_ld.judge over SVGP's quantities): err(q) = max |got - q_ld| / max |q_ld| <= max(32 e64(q),
256 eps64 kappa), e64 = the distance of the fp64 restatement from long double on the same input (never the device's figure),
kappa = cond2(Kmm).  Judged per case: mu, v, KL, dtheta, dZ, dL_dm, dL_dchol, woodbury_vector, woodbury_inv and the prediction
(mean, variance, covariance) at 1 and at 129 new points.  The dF_dmu / dF_dv given to backward are the package likelihood's at
the LONG-DOUBLE mu and v rounded to fp64 (times batch_scale), the same for the device and both restatements: the device's own
mu and v are judged separately, so a forward error cannot hide in backward.  dZ columns outside every part's active_dims must be
exactly zero.

One module-scoped context serves the plain sweep in list order (svgp_np.CASES).  Families (N, M, D, L):
    m_edge    N = 257, D = 2, L = 1, M = 1 | 127 | 128 (m == mp) | 129 | 257 (three tiles)
    n_edge    M = 65, D = 3, L = 2, N = 1 | 2 | 127 | 128 | 129 | 257 | 2049; N < M on purpose
    latents   N = 129, M = 65, D = 2, L = 3 | 16 (L = 1 | 2 are everywhere else)
    dispatch  N = 193, M = 65, L = 1, D = 1 | 16 (fused gradient pass) | 17 (unfused) | 33 (two record groups)
    kernels   rbf + white (unfused), rbf[0,1] x matern32[2] + white, rbf on columns 0 and 2 of three; L = 2
    signed    Student-t: dF_dv of mixed sign (asserted); Bernoulli on a product
    stale     no set_data between: L = 2, M = 129 -> L = 1, M = 128 -> new Z and theta
    chunks    N = 262145, M = 65, L = 1: two chunks, the second ragged (blocked reference)
Determinism: one case twice in fresh contexts, identical bytes.

Measured on an MI355X, worst err(q) per family (a record, never a reason to tighten a bound; wv = woodbury_vector, Winv =
woodbury_inv; pmu / pvar / pcov: the prediction at 129 points; err/bound = the worst ratio of a figure to its bound):

    family            mu        v       KL   dtheta       dZ    dL_dm dL_dchol       wv     Winv      pmu     pvar     pcov err/bound
    m_edge         4e-15    4e-15    6e-16    7e-15    3e-14    2e-15    4e-15    3e-15    8e-15    8e-15    1e-14    2e-14   0.121
    n_edge         3e-15    2e-15    6e-16    2e-13    1e-14    2e-15    5e-15    1e-15    6e-15    2e-15    3e-15    4e-15   0.271
    latents        2e-15    2e-15    4e-16    9e-15    1e-14    2e-15    2e-15    1e-15    3e-15    2e-15    9e-15    1e-14   0.010
    dispatch       4e-15    4e-15    7e-16    5e-15    3e-14    3e-15    4e-15    3e-15    7e-15    4e-15    7e-15    9e-15   0.031
    kernels        2e-15    4e-15    2e-16    2e-14    2e-14    2e-15    4e-15    1e-15    4e-15    2e-15    2e-14    2e-14   0.029
    signed         2e-15    3e-15    1e-15    1e-15    6e-15    1e-15    3e-15    2e-15    5e-15    2e-15    3e-15    3e-15   0.008
    stale          4e-15    6e-15    5e-16    4e-15    2e-14    7e-15    6e-15    4e-15    9e-15    5e-15    4e-14    5e-14   0.007
    chunks         4e-15    4e-15    6e-16    7e-13    2e-14    8e-16    4e-14    2e-15    7e-15    2e-15    7e-15    9e-15   0.350

Model against the reference's fixtures (bound 1e-9, gradients 1e-6): bound <= 1e-9, dZ 1e-13, dtheta 3e-14, dL_dchol 3e-14,
dL_dm 4e-14; the toy classification went from -199.8995 to -49.4338 (reference -49.4342) at accuracy 0.915 (reference 0.915).
"""
import numpy as np
import pytest

import svgp_np as S

pytestmark = pytest.mark.gpu


def device_eval(ctx, c, dF, set_data=True):
    """one forward / backward / predict session of the device on a case"""
    if set_data:
        ctx.set_data(c["X"], c["Y"])
    info, fw = ctx.svgp_forward(c["specs"], c["Z"], c["q_mean"], c["q_L"])
    assert info == 0
    bw = ctx.svgp_backward(dF[0], dF[1])
    wv, wi = ctx.svgp_woodbury()
    got = dict(mu=fw["mu"], v=fw["v"], KL=fw["KL"], dtheta=bw["dtheta"], dZ=bw["dZ"], dL_dm=bw["dL_dm"], dL_dchol=bw["dL_dchol"],
               woodbury_vector=wv, woodbury_inv=wi)
    for tag, P in c["Xs"].items():
        got["mu" + tag], got["var" + tag] = ctx.svgp_predict(c["specs"], P, full_cov=False)
        got["cov" + tag] = ctx.svgp_predict(c["specs"], P, full_cov=True)[1]
    return got


def judged(name, got):
    c, dF, ref, r64, kappa = S.reference(name)
    figs, bad = S.judge(got, ref, r64, kappa)
    print("%-52s kappa %8.1f  " % (name, kappa) + "  ".join("%s %.1e/%.1e" % (q, e, b) for q, (e, b) in figs.items()))
    assert not bad, "%s: %s" % (name, "; ".join(bad))
    return figs


@pytest.fixture(scope="module")
def ctx():
    from gpy_amd import _lib
    return _lib.SparseContext(0)


@pytest.mark.parametrize("name", S.PLAIN)
def test_plain_sweep(ctx, name):
    c, dF, ref, r64, kappa = S.reference(name)
    if c["lik"] == "studentt":
        assert dF[1].min() < 0 < dF[1].max(), "this case is here for weights of mixed sign"
    judged(name, device_eval(ctx, c, dF))


def test_stale_state_sequence():
    """L = 2, M = 129 -> L = 1, M = 128 -> new Z and theta on one context without set_data between"""
    from gpy_amd import _lib
    ctx = _lib.SparseContext(0)
    X0 = None
    for name in S.STALE:
        c, dF, ref, r64, kappa = S.reference(name)
        assert X0 is None or np.array_equal(c["X"], X0)
        judged(name, device_eval(ctx, c, dF, set_data=X0 is None))
        X0 = c["X"]


@pytest.mark.parametrize("name", S.BLOCKED)
def test_several_chunks(name):
    from gpy_amd import _lib
    c, dF, ref, r64, kappa = S.reference(name)
    judged(name, device_eval(_lib.SparseContext(0), c, dF))


def test_two_fresh_contexts_give_identical_bytes():
    from gpy_amd import _lib
    c, dF, ref, r64, kappa = S.reference(S.DETERMINISM)
    a = device_eval(_lib.SparseContext(0), c, dF)
    b = device_eval(_lib.SparseContext(0), c, dF)
    for q in a:
        assert np.asarray(a[q]).tobytes() == np.asarray(b[q]).tobytes(), q


def test_refusals_leave_the_context_usable():
    from gpy_amd import _lib
    name = "n_edge-matern52_iso-n129_m65_d3_l2-gaussian"
    c, dF, ref, r64, kappa = S.reference(name)
    ctx = _lib.SparseContext(0)
    ctx.set_data(c["X"], c["Y"])
    ctx.M, ctx.L, ctx._svgp_ntheta = c["M"], c["L"], 2
    with pytest.raises(_lib.MI355GPError, match="run mi355gp_svgp_forward first"):
        ctx.svgp_backward(dF[0], dF[1])
    with pytest.raises(_lib.MI355GPError, match="run mi355gp_svgp_forward first"):
        ctx.svgp_predict(c["specs"], c["Xs"]["1"])
    with pytest.raises(_lib.MI355GPError, match="17 latent functions"):
        ctx.svgp_forward(c["specs"], c["Z"], np.zeros((c["M"], 17)), np.tile(np.eye(c["M"]), (17, 1, 1)))
    with pytest.raises(_lib.MI355GPError, match="not supported by the sparse path|sparse path"):
        ctx.svgp_forward([("linear", 0, np.array([1.0]), None, 0)], c["Z"], c["q_mean"], c["q_L"])
    bad_L = c["q_L"].copy()
    bad_L[1, 3, 3] = 0.0
    with pytest.raises(_lib.MI355GPError, match="Cholesky representation unstable"):
        ctx.svgp_forward(c["specs"], c["Z"], c["q_mean"], bad_L)
    # VarDTC's fetches and prediction describe VarDTC's result: refused after an SVGP call, by name
    got = device_eval(ctx, c, dF, set_data=False)
    for call in (lambda: ctx.fetch(0), lambda: ctx.fetch_dL_dKnm(0, 8), lambda: ctx.predict(c["specs"], c["Xs"]["1"])):
        with pytest.raises(_lib.MI355GPError, match="SVGP call"):
            call()
    # a VarDTC call ends the SVGP session; SVGP's backward / predict then ask for a forward
    info, r = ctx.vardtc_sum(c["specs"], c["Z"], 0.1)
    assert info == 0 and ctx.fetch(0).shape == (c["M"], c["M"])
    with pytest.raises(_lib.MI355GPError, match="run mi355gp_svgp_forward first"):
        ctx.svgp_backward(dF[0], dF[1])
    # input variances on the context: refused
    ctx.set_input_variance(np.full(c["X"].shape, 0.01))
    with pytest.raises(_lib.MI355GPError, match="input variances"):
        ctx.svgp_forward(c["specs"], c["Z"], c["q_mean"], c["q_L"])
    # a row-sharded context: refused
    sh = _lib.SparseContext(0)
    sh.attach_loopback(0, 1, 4242)
    sh.set_data(c["X"], c["Y"])
    with pytest.raises(_lib.MI355GPError, match="row-sharded"):
        sh.svgp_forward(c["specs"], c["Z"], c["q_mean"], c["q_L"])
    # and the first context still works after all that
    ctx.set_data(c["X"], c["Y"])
    judged(name, device_eval(ctx, c, dF, set_data=False))
    assert got["mu"].tobytes() == ctx.svgp_forward(c["specs"], c["Z"], c["q_mean"], c["q_L"])[1]["mu"].tobytes()


# ---- the model against the reference's fixtures (tolerances of tests/test_gpu_sparse.py: bound 1e-9, gradients 1e-6, predictive
#      mean 1e-6, variance and covariance 1e-5) ---------------------------------------------------------------------------------
def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


@pytest.mark.parametrize("name", ["gauss_rbf_ard_l2_n150_m40_d3_bs3", "bern_rbf_iso_l1_n300_m70_d2"])
def test_model_against_reference_fixture(name):
    import gpy_amd
    fx = S.load_fixture(name)
    N = fx["X"].shape[0]
    bs = fx["batch_scale"]
    # batch_scale = N_all / N_batch: the fixture's rows as the one minibatch of a data set `bs` times as long
    reps = int(round(bs))
    X_all, Y_all = np.tile(fx["X"], (reps, 1)), np.tile(fx["Y"], (reps, 1))
    m = gpy_amd.core.SVGP(X_all, Y_all, fx["Z"], S.make_kernel(fx), S.make_likelihood(fx), batchsize=N if reps > 1 else None, seed=0)
    m.set_data(fx["X"], fx["Y"])
    x = m.param_array.copy()
    nz, nk, nl = fx["Z"].size, fx["dtheta"].size, fx["dL_dthetaL"].size
    x[nz + nk + nl:] = np.concatenate([fx["q_chol"].ravel(), fx["q_mean"].ravel()])
    m.param_array = x
    assert abs(m.log_likelihood() - fx["bound"]) <= 1e-9 * abs(fx["bound"])
    gref = np.concatenate([fx["dZ"].ravel(), fx["dtheta"], fx["dL_dthetaL"], fx["dL_dchol"].ravel(), fx["dL_dm"].ravel()])
    assert m.gradient.shape == gref.shape
    for lo, hi, what in ((0, nz, "dZ"), (nz, nz + nk, "dtheta"), (nz + nk, nz + nk + nl, "dL_dthetaL"),
                         (nz + nk + nl, nz + nk + nl + fx["q_chol"].size, "dL_dchol"), (gref.size - fx["q_mean"].size, gref.size, "dL_dm")):
        if hi > lo:
            e = _rel(m.gradient[lo:hi], gref[lo:hi])
            print("%s %s %.2e" % (name, what, e))
            assert e <= 1e-6, what
    mu, var = m._raw_predict(fx["Xs"])
    _, cov = m._raw_predict(fx["Xs"], full_cov=True)
    assert _rel(mu, fx["pred_mu"]) <= 1e-6 and _rel(var, fx["pred_var"]) <= 1e-5 and _rel(cov, fx["pred_cov"]) <= 1e-5
    assert _rel(m.posterior.woodbury_vector, fx["woodbury_vector"]) <= 1e-6
    assert _rel(m.posterior.woodbury_inv, fx["woodbury_inv"]) <= 1e-4


def test_toy_classification_optimizes_to_the_reference_accuracy():
    """1-D two-class toy: `optimize()` raises the bound and reaches the training accuracy the reference reaches on the same data
    from the same start in the same number of L-BFGS-B iterations (stored by tools/make_golden_svgp.py)"""
    import os
    import gpy_amd
    t = dict(np.load(os.path.join(S.GOLDEN, "toy_classification.npz")))
    m = gpy_amd.SVGP(t["X"], t["Y"], t["Z0"], gpy_amd.RBF(1, variance=t["theta0"][0], lengthscale=t["theta0"][1]), gpy_amd.Bernoulli())
    b0 = m.log_likelihood()
    assert abs(b0 - float(t["bound_start"])) <= 1e-9 * abs(float(t["bound_start"]))
    m.optimize(max_iters=int(t["maxiter"]))
    b1 = m.log_likelihood()
    mu, _ = m._raw_predict(t["X"])
    acc = float(np.mean((mu[:, 0] > 0) == (t["Y"][:, 0] == 1)))
    print("toy: bound %.4f -> %.4f (reference %.4f -> %.4f), accuracy %.4f (reference %.4f)"
          % (b0, b1, float(t["bound_start"]), float(t["bound_end"]), acc, float(t["accuracy"])))
    assert b1 > b0
    assert acc >= float(t["accuracy"])
