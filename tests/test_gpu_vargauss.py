"""GPU (-m gpu): VarGauss on the exact context -- mi355gp_vargauss_forward / mi355gp_vargauss_backward inside the session of
mi355gp_laplace_begin, mi355gp_laplace_predict and the three fetches, i.e. csrc/vargauss.hip with its k_vg_*
kernels -- at every shape edge, judged against the long-double restatement tests/vargauss_ld.py (80-bit;
tests/test_oracle_vargauss.py holds it against the reference's own fixtures).

Judge (vargauss_ld.judge, the rule of laplace_ld.judge): err(q) = max |got - q_ld| / max |q_ld| <= max(32 e64(q), 256 eps64 kappa),
e64 = the distance of the same formulas in fp64 from long double on the same input (never the device's figure), kappa = cond2(A),
A = I + diag(beta) K diag(beta) in fp64; every dtheta entry within kern_ld.grad_tol.  Every case keeps kappa <= 1e4.  Judged per
case: m, var, log det A, tr Ai (forward); dalpha, dbeta, dtheta (backward, in the reference's form of dL_dK and in the exact one); the fetched K, woodbury_inv and dL_dK (each bitwise
symmetric); mu, var and cov at new points, after forward alone and again after backward with the same bytes; the woodbury_inv
fetched after forward and after backward (where it is one lauum of the resident X) with the same bytes.

Families (vargauss_ld.CASES), one module-scoped context each, in list order:
    n_edge       RBF-ARD + Bias, D = 3: N = 1 | 2 | 63 | 64 | 65 | 127 | 128 | 129 | 255 | 256 | 257 | 513
    signs        RBF iso, D = 2, N = 129 | 257: beta all positive; mixed signs; |beta| = 1e-2 on a tenth of the sites; beta up to 7;
                 dF_dv with exact zeros on a tenth of the sites and of both signs
    kernels      N = 129: RBF-ARD at D = 32 | 33, Matern32-ARD on a column subset, StdPeriodic-ARD, RatQuad-ARD, Linear + Bias,
                 MLP x RBF, ExpQuadCosine at D = 1; RBF x Coregionalize with P = 3 at N = 65
    points       N = 129, M = 1 | 127 | 128 | 129 | 257 new points, diagonal and full_cov
    stale        one context: N = 257; set_data at N = 129; a full Laplace newton / finish / gradients round (its bytes equal a
                 fresh context's); VarGauss again; exact_inference_sum; VarGauss again
    determinism  one case run in two fresh contexts: identical bytes of every output
    model        every fixture of the reference through GPVariationalGaussianApproximation at the CPU test's tolerances
                 (vargauss_ld.FIXTURE_TOL); checkgrad() on the Bernoulli toy model; the 2 N variational gradients by central differences; optimize() against the reference's bound

Measured on an MI355X: the worst err(q) per family and quantity -- a record, never a reason to tighten a bound (mu* / var* / cov* =
the prediction at every M of the family; dtheta = the worst entry in units of its own bound; err/bound = the worst ratio of a
figure to its bound over the family; kappa = the largest cond2(A)):

    family        m     var  logdet    trAi  dalpha   dbeta       K   wb_inv   dL_dK     mu*    var*    cov*  dtheta  err/bound  kappa
    n_edge    7e-16   2e-15   5e-16   2e-16   1e-15   1e-14   3e-16   3e-15   2e-15   8e-16   6e-15   4e-14  0.0040      0.005    209
    signs     9e-16   1e-14   6e-16   4e-16   9e-16   4e-14   2e-16   1e-14   7e-14   1e-15   6e-14   9e-14  0.0005      0.004   1217
    kernels   1e-15   3e-14   3e-16   1e-16   7e-16   6e-14   2e-15   1e-15   1e-15   2e-15   2e-14   4e-14  0.0007      0.011    118
    points    3e-16   1e-15   7e-17   1e-16   4e-16   9e-15   2e-16   1e-15   9e-16   5e-16   2e-15   3e-15  0.0002      0.002     81
    stale     7e-16   2e-15   4e-16   2e-16   4e-16   1e-14   3e-16   2e-15   2e-15   2e-15   3e-15   3e-15  0.0005      0.002    107

The exact form of dL_dK (`vargauss_backward(exact=True)`), same sweep: dL_dK 2e-15 / 8e-14 / 9e-16 / 1e-15 / 2e-15 and dtheta 0.0016 / 0.0007 /
0.0013 / 0.0002 / 0.0003 of its bound, by family in the order above.

The model family against the reference's fixtures (worst over the eight, relative to max |value|): m 1.6e-15, var 3.8e-14, lml 4.4e-16,
dalpha 1.9e-15, dbeta 2.6e-14, dL_dK_sym 1.2e-14, dL_dthetaL 6.8e-16, dtheta 1.9e-15, pred_mu 1.2e-15, pred_var 2.4e-14, pred_cov 3.4e-14.
Every case passed as the code stood at its first run.  The whole file: 46 tests, 15 s of wall time, most of it the long-double
reference at N = 513 (9 s)."""
import os
import signal
import time

import numpy as np
import pytest

import gpy_amd
from gpy_amd import _lib as L

import kern_ld as KL
import vargauss_ld as VL
from test_oracle_vargauss import check_model_against_fixture

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not KL.HAVE_LD, reason="np.longdouble is not an extended format on this host")]
LIMIT_S = 240


@pytest.fixture(autouse=True)
def _time_limit():
    def stop(signum, frame):
        raise TimeoutError("test exceeded its %d s limit" % LIMIT_S)
    old = signal.signal(signal.SIGALRM, stop)
    signal.alarm(LIMIT_S)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


@pytest.fixture(scope="module")
def ctxs():
    """one context per family, made when the family's first case runs"""
    held = {}
    yield held
    for c in held.values():
        c.close()


def family_ctx(ctxs, family):
    if family not in ctxs:
        ctxs[family] = L.Context(0)
    return ctxs[family]


def _predictions(ctx, c, got, bad, tag):
    for M in c["Ms"]:
        Xs = c["Xs%d" % M]
        mu, var = ctx.laplace_predict(c["dev_specs"], Xs, c["alpha"])
        mu2, cov = ctx.laplace_predict(c["dev_specs"], Xs, c["alpha"], full_cov=True)
        if mu.tobytes() != mu2.tobytes():
            bad.append("mu%d differs between the diagonal and the full_cov call (%s)" % (M, tag))
        for q, val in (("mu", mu), ("var", var), ("cov", cov)):
            key = "%s%d" % (q, M)
            if key in got and got[key].tobytes() != val.tobytes():
                bad.append("%s changed with backward" % key)
            got[key] = val


def evaluate(ctx, c, set_data=True):
    """every device call of a case: ({quantity: value}, [what a structural assertion found])"""
    specs = c["dev_specs"]
    got, bad = {}, []
    if set_data:
        ctx.set_data(c["X"], c["Y"])
    ctx.laplace_begin(specs)
    got["K"] = ctx.fetch(L.FETCH_K)
    info, got["m"], got["var"], got["logdet"], got["trAi"], got["ma"] = ctx.vargauss_forward(c["alpha"], c["beta"])
    assert info == 0
    _predictions(ctx, c, got, bad, "after forward")
    got["woodbury_inv"] = ctx.fetch(L.FETCH_KINV)
    got["dalpha"], got["dbeta"], dth = ctx.vargauss_backward(c["dF_dm"], c["dF_dv"])
    got["dtheta"] = KL.chain_coreg(c["specs"], dth)
    got["dL_dK"] = ctx.fetch(L.FETCH_DLDK)
    if ctx.fetch(L.FETCH_KINV).tobytes() != got["woodbury_inv"].tobytes():
        bad.append("woodbury_inv changed with backward")
    _predictions(ctx, c, got, bad, "after backward")
    if ctx.fetch(L.FETCH_DLDK).tobytes() != got["dL_dK"].tobytes() or ctx.fetch(L.FETCH_K).tobytes() != got["K"].tobytes():
        bad.append("dL_dK or K changed with the fetch of woodbury_inv")
    # the same evaluation again with the exact form of dL_dK: forward gives the same bytes, Ai stays in place under backward
    again = ctx.vargauss_forward(c["alpha"], c["beta"])
    if again[0] != 0 or any(np.asarray(a).tobytes() != np.asarray(got[q]).tobytes() for a, q in zip(again[1:], ("m", "var", "logdet", "trAi", "ma"))):
        bad.append("a second forward differs from the first")
    da, db, dth = ctx.vargauss_backward(c["dF_dm"], c["dF_dv"], exact=True)
    if da.tobytes() != got["dalpha"].tobytes() or db.tobytes() != got["dbeta"].tobytes():
        bad.append("the variational gradients differ between the two forms of backward")
    got["dtheta_exact"] = KL.chain_coreg(c["specs"], dth)
    got["dL_dK_exact"] = ctx.fetch(L.FETCH_DLDK)
    if ctx.fetch(L.FETCH_KINV).tobytes() != got["woodbury_inv"].tobytes():
        bad.append("woodbury_inv changed with the exact backward")
    _predictions(ctx, c, got, bad, "after the exact backward")
    for q in VL.SYMMETRIC:
        if not np.array_equal(got[q], got[q].T):
            bad.append("%s is not bitwise symmetric" % q)
    return got, bad


def _report(name, c, got, bad0, kappa, ref, r64, t_ref, t_dev):
    figs, bad = VL.judge(c, got, ref, r64, kappa)
    print()
    print("%-36s kappa %.0f  ref %.1f s dev %.2f s  " % (name, kappa, t_ref, t_dev)
          + "  ".join("%s %.1e/%.1e" % (q, e, b) for q, (e, b) in figs.items()))
    assert kappa <= 1e4, kappa
    assert not bad0, bad0
    assert not bad, bad
    assert set(figs) == set(VL.judged(c)) | {"dtheta", "dtheta_exact"}
    return figs


def _check(ctxs, name, set_data=True):
    t0 = time.time()
    c, ref, r64, kappa = VL.reference(name)
    t1 = time.time()
    try:
        got, bad0 = evaluate(family_ctx(ctxs, c["family"]), c, set_data)
    except L.MI355GPError as e:          # nothing more on this device after an error of the runtime
        pytest.exit("device error in %s, the sweep ends here: %s" % (name, e), returncode=3)
    return _report(name, c, got, bad0, kappa, ref, r64, t1 - t0, time.time() - t1)


@pytest.mark.parametrize("name", VL.NAMES["n_edge"])
def test_n_edge(name, ctxs):
    _check(ctxs, name)


@pytest.mark.parametrize("name", VL.NAMES["signs"])
def test_signs(name, ctxs):
    _check(ctxs, name)


@pytest.mark.parametrize("name", VL.NAMES["kernels"])
def test_kernels(name, ctxs):
    _check(ctxs, name)


@pytest.mark.parametrize("name", VL.NAMES["points"])
def test_points(name, ctxs):
    _check(ctxs, name)


def _laplace_round(ctx, c, aux):
    """a full Laplace newton / finish / gradients round on the context's data: the bytes of everything it returns"""
    W, b = aux.uniform(0.05, 0.3, c["N"]), 0.3 * aux.standard_normal(c["N"])
    ctx.laplace_begin(c["dev_specs"])
    info, a, Ka, ld = ctx.laplace_newton(W, b)
    assert info == 0
    info, d, ld2 = ctx.laplace_finish(W)
    assert info == 0
    dth = ctx.laplace_gradients(a, 0.1 * b)
    mu, var = ctx.laplace_predict(c["dev_specs"], c["Xs129"], a)
    return b"".join(np.asarray(x).tobytes() for x in (a, Ka, ld, d, ld2, dth, ctx.fetch(L.FETCH_KINV), ctx.fetch(L.FETCH_DLDK), mu, var))


def test_stale_state_of_one_context(ctxs):
    """the steps in order on one context; every VarGauss step is judged, a failing one does not hide the later ones"""
    s1, s2, s3, s4 = VL.NAMES["stale"]
    failed = []

    def step(name, set_data):
        try:
            _check(ctxs, name, set_data)
        except AssertionError as e:
            failed.append("%s: %s" % (name, e))
    step(s1, True)
    step(s2, True)
    c = VL.reference(s2)[0]
    ctx = family_ctx(ctxs, "stale")
    try:
        here = _laplace_round(ctx, c, np.random.default_rng(5))
        with pytest.raises(L.MI355GPError, match="call mi355gp_vargauss_forward first"):
            ctx.vargauss_backward(c["dF_dm"], c["dF_dv"])             # the session holds Laplace's factor, not VarGauss's
        fresh = L.Context(0)
        fresh.set_data(c["X"], c["Y"])
        there = _laplace_round(fresh, c, np.random.default_rng(5))
        fresh.close()
    except L.MI355GPError as e:
        pytest.exit("device error in the Laplace round of the stale family, the sweep ends here: %s" % e, returncode=3)
    if here != there:
        failed.append("the Laplace round after VarGauss differs from a fresh context's")
    step(s3, False)
    rc, _ = ctx.exact_inference_sum(c["dev_specs"], 0.1, want_diag=True)
    assert rc == 0
    with pytest.raises(L.MI355GPError, match="call mi355gp_laplace_begin first"):
        ctx.vargauss_forward(c["alpha"], c["beta"])
    step(s4, False)
    assert not failed, failed


def test_two_fresh_contexts_give_the_same_bytes():
    c = VL.make_case(VL.DETERMINISM)
    runs = []
    try:
        for _ in range(2):
            ctx = L.Context(0)
            got, bad = evaluate(ctx, c)
            ctx.close()
            assert not bad, bad
            runs.append(got)
    except L.MI355GPError as e:
        pytest.exit("device error in the determinism case, the sweep ends here: %s" % e, returncode=3)
    for q in runs[0]:
        assert np.asarray(runs[0][q]).tobytes() == np.asarray(runs[1][q]).tobytes(), q


def test_error_paths_return_a_message():
    c = VL.make_case("n_edge-rbf_ard+bias-n65")
    ctx = L.Context(0)
    try:
        ctx.set_data(c["X"], c["Y"])
        with pytest.raises(L.MI355GPError, match="call mi355gp_laplace_begin first"):
            ctx.vargauss_forward(c["alpha"], c["beta"])
        ctx.laplace_begin(c["dev_specs"])
        with pytest.raises(L.MI355GPError, match="call mi355gp_vargauss_forward first"):
            ctx.vargauss_backward(c["dF_dm"], c["dF_dv"])
        for bad_value in (0.0, np.nan, np.inf):
            beta = c["beta"].copy()
            beta[17] = bad_value
            with pytest.raises(L.MI355GPError, match=r"beta\[17\] = .* is not a finite non-zero number"):
                ctx.vargauss_forward(c["alpha"], beta)
        alpha = c["alpha"].copy()
        alpha[3] = np.nan
        with pytest.raises(L.MI355GPError, match=r"alpha\[3\] = nan is not finite"):
            ctx.vargauss_forward(alpha, c["beta"])
        assert ctx.vargauss_forward(c["alpha"], c["beta"])[0] == 0
        with pytest.raises(L.MI355GPError, match="holds a VarGauss evaluation"):
            ctx.laplace_gradients(c["alpha"], c["dF_dm"])
        with pytest.raises(L.MI355GPError, match=r"dF_dv\[0\] = inf is not finite"):
            ctx.vargauss_backward(c["dF_dm"], np.full(c["N"], np.inf))
        ctx.vargauss_backward(c["dF_dm"], c["dF_dv"])
        with pytest.raises(L.MI355GPError, match="one backward per forward"):
            ctx.vargauss_backward(c["dF_dm"], c["dF_dv"])
    finally:
        ctx.close()


# ---- the model ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", VL.FIXTURES)
def test_model_against_the_reference(name):
    g = VL.load_fixture(name)
    n = g["X"].shape[0]
    try:
        m = gpy_amd.GPVariationalGaussianApproximation(g["X"], g["Y"], VL.fixture_kernel(g["specs"]), VL.fixture_likelihood(g))
        m.inference_method.reference_gradient = True              # the fixtures hold the reference's form of dL_dK
        x = m.param_array
        x[-2 * n:-n], x[-n:] = g["alpha"][:, 0], g["beta"]
        m.param_array = x
        figs = check_model_against_fixture(m, g)
    except L.MI355GPError as e:
        pytest.exit("device error in %s, the sweep ends here: %s" % (name, e), returncode=3)
    print()
    print(name, "  ".join("%s %.1e/%.1e" % (q, e, VL.FIXTURE_TOL[q]) for q, e in figs.items()))
    bad = ["%s: %.3e > %.3e" % (q, e, VL.FIXTURE_TOL[q]) for q, e in figs.items() if not e <= VL.FIXTURE_TOL[q]]
    assert not bad, bad


def _toy():
    return np.load(os.path.join(VL.GOLDEN, "toy_1d_optimize.npz"))


def _toy_model(randomise):
    z = _toy()
    m = gpy_amd.GPVariationalGaussianApproximation(z["X"], z["Y"], gpy_amd.RBF(1), gpy_amd.Bernoulli())
    n = z["X"].shape[0]
    if randomise:
        rng = np.random.default_rng(3)
        x = m.param_array
        x[2:2 + n] = 0.2 * rng.standard_normal(n)
        x[2 + n:] = np.where(rng.random(n) < 0.3, -1.0, 1.0) * rng.uniform(0.5, 1.5, n)
        m.param_array = x
    return m, n


def test_checkgrad_on_the_toy_model():
    """`checkgrad()` of the whole parameter vector, as the model is built (alpha = 0, beta = 1) and at a random state with mixed
    signs.  It holds because the model's kernel gradient is the derivative of the bound (`mi355gp_vargauss_backward_exact`); with
    `reference_gradient=True` the ratios at the first state are 0.9959, 1.0117, 1.0105 against the tolerance of 1e-3: the
    reference's `np.dot(tmp*dF_dv, tmp.T)` (var_gauss.py:65) scales the ROWS of tmp by dF_dv where d var_i / dK asks for its
    COLUMNS (lengthscale gradient 2.66710 against 2.66551 by central differences)."""
    np.random.seed(1)
    for randomise in (False, True):
        m, _ = _toy_model(randomise)
        assert all(m.checkgrad(verbose=True) for _ in range(3))


def test_variational_gradients_are_exact():
    """central differences along random directions of the alpha block and of the beta block alone, at the start and at a random
    state with mixed signs: within 1e-5 (the rounding of a difference of two bounds of size 50 at a step of 1e-5)"""
    for randomise in (False, True):
        m, n = _toy_model(randomise)
        x = m.param_array.copy()
        g = m.objective_function_gradients().copy()
        rng = np.random.default_rng(7)
        for lo, hi in ((2, 2 + n), (2 + n, 2 + 2 * n)):
            dx = np.zeros_like(x)
            dx[lo:hi] = 1e-5 * rng.choice([-1.0, 1.0], hi - lo)
            m.param_array = x + dx
            f1 = m.objective_function()
            m.param_array = x - dx
            f2 = m.objective_function()
            m.param_array = x
            num, ana = (f1 - f2) / 2, float(dx.dot(g))
            print("block %d:%d numerical %.10e analytic %.10e" % (lo, hi, num, ana))
            assert abs(num - ana) <= 1e-5 * abs(ana) + 1e-12


def test_optimize_reaches_the_reference_bound():
    """One `optimize()` from the default start against the reference's own L-BFGS-B run (tests/golden/vargauss/toy_1d_optimize.npz:
    bound -47.226719 -> -14.487961 in 98 iterations, accuracy 0.95), at the 1e-3 that the Laplace and EP toy tests allow a bound.
    The start agrees to 1e-9; with the gradient of the bound the run goes past the reference's figure (-11.957 after 200
    iterations on the long-double restatement), where the reference's own form of the gradient stalls at -14.654 after 51."""
    z = _toy()
    m = gpy_amd.GPVariationalGaussianApproximation(z["X"], z["Y"], gpy_amd.RBF(1), gpy_amd.Bernoulli())
    start = m.log_likelihood()
    assert abs(start - float(z["lml_start"])) <= 1e-9 * abs(float(z["lml_start"]))
    m.optimize(max_iters=200)
    p, _ = m.predict(z["X"])
    acc = float(np.mean((p > 0.5) == (z["Y"] == 1)))
    print("bound %.6f -> %.6f (reference %.6f -> %.6f), accuracy %.4f (reference %.4f)" % (
        start, m.log_likelihood(), float(z["lml_start"]), float(z["lml_end"]), acc, float(z["accuracy"])))
    # the margin of the Laplace and EP toy tests: 1e-3 of the reference's figure
    assert m.log_likelihood() >= float(z["lml_end"]) - 1e-3 * abs(float(z["lml_end"]))
    assert acc >= float(z["accuracy"])
    f = m.posterior_samples_f(z["X"][:5], size=3)
    assert f.shape == (5, 1, 3) and np.isfinite(f).all()
    mu, var = m.predict_noiseless(z["X"][:5])
    assert mu.shape == (5, 1) and (var > 0).all()
