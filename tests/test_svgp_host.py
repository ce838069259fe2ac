"""CPU: `SVGP.inference` and the model `gpy_amd.core.SVGP` end to end over a stand-in for `_lib.SparseContext` that answers
the SVGP session with the fp64 restatement tests/svgp_np.py (no GPU work; the pattern of tests/test_host_routing.py): what is
sent to the device, the flat parameter order, where batch_scale goes, the model's gradient against finite differences of its own
bound, minibatches under a seed, and every refusal by name."""
import numpy as np
import pytest

import gpy_amd
import svgp_np as S
from gpy_amd import _lib
from gpy_amd.svgp import SVGP as SVGPInference
from gpy_amd.util import choleskies
from sparse_ld import rel_err
from test_oracle_svgp import BOUND


@pytest.fixture
def rctx(monkeypatch):
    made = []

    class Ctx(S.RestatementContext):
        def __init__(self, device=0):
            super(Ctx, self).__init__(device)
            made.append(self)
    monkeypatch.setattr(_lib, "SparseContext", Ctx)
    return made


def _model(fx, batchsize=None, seed=None, reps=1):
    X, Y = np.tile(fx["X"], (reps, 1)), np.tile(fx["Y"], (reps, 1))
    return gpy_amd.core.SVGP(X, Y, fx["Z"], S.make_kernel(fx), S.make_likelihood(fx), batchsize=batchsize, seed=seed)


def _set_q(m, fx):
    x = m.param_array.copy()
    x[x.size - fx["q_chol"].size - fx["q_mean"].size:] = np.concatenate([fx["q_chol"].ravel(), fx["q_mean"].ravel()])
    m.param_array = x


@pytest.mark.parametrize("name", S.FIXTURES)
def test_inference_returns_the_reference_grad_dict(rctx, name):
    fx = S.load_fixture(name)
    post, bound, gd = SVGPInference().inference(fx["q_mean"], fx["q_chol"], S.make_kernel(fx), fx["X"], fx["Z"], S.make_likelihood(fx),
                                                fx["Y"], batch_scale=fx["batch_scale"])
    assert rel_err(bound, fx["bound"]) <= BOUND
    for q, got in (("dL_dm", gd["dL_dm"]), ("dL_dchol", gd["dL_dchol"]), ("dL_dKdiag", gd["dL_dKdiag"]), ("dtheta", gd["fused"]["dtheta"]),
                   ("dZ", gd["fused"]["dZ"])):
        assert np.shape(got) == fx[q].shape and rel_err(got, fx[q]) <= BOUND, q
    if fx["dL_dthetaL"].size:
        assert rel_err(np.atleast_1d(gd["dL_dthetaL"]), fx["dL_dthetaL"]) <= BOUND
    else:
        assert gd["dL_dthetaL"] is None
    # what went to the device: the sliced X, L x M x M factors, the dF already times batch_scale
    ctx = rctx[0]
    M, L = fx["q_mean"].shape
    assert [c[0] for c in ctx.log] == ["set_data", "svgp_forward", "svgp_backward"]
    assert ctx.log[1][1:] == (fx["Z"].shape, (M, L), (L, M, M))
    assert rel_err(ctx.dF[0], fx["dF_dmu"] * fx["batch_scale"]) <= BOUND and rel_err(ctx.dF[1], fx["dF_dv"] * fx["batch_scale"]) <= BOUND
    # prediction through the posterior runs on the context while it is the latest result
    mu, var = post._raw_predict(S.make_kernel(fx), fx["Xs"], fx["Z"])
    assert ctx.log[-1][0] == "svgp_predict" and rel_err(mu, fx["pred_mu"]) <= BOUND and rel_err(var, fx["pred_var"]) <= BOUND
    assert rel_err(post.woodbury_vector, fx["woodbury_vector"]) <= BOUND and rel_err(post.woodbury_inv, fx["woodbury_inv"]) <= BOUND
    assert post.covariance.shape == (M, M, L)


def test_flat_parameter_order_and_initial_values(rctx):
    fx = S.load_fixture("gauss_rbf_ard_l2_n150_m40_d3_bs3")
    m = _model(fx)
    M, L = fx["q_mean"].shape
    names = [p.name for p in m.flattened_parameters()]
    assert names[0] == "inducing inputs" and names[-2:] == ["q_u_chol", "q_u_mean"]           # core/svgp.py:48-52 after sparse_gp.py:59
    assert names[1:-2] == ["variance", "lengthscale", "variance"]                              # kern, then the likelihood
    assert m.q_u_chol.shape == (M * (M + 1) // 2, L) and m.q_u_mean.shape == (M, L)
    assert not m.q_u_chol.positive and not m.q_u_mean.positive                                 # unconstrained
    assert np.array_equal(choleskies.flat_to_triang(m.q_u_chol.values), np.tile(np.eye(M), (L, 1, 1)))
    assert np.all(m.q_u_mean.values == 0)
    nz, nk = fx["Z"].size, fx["dtheta"].size
    assert m.param_array.size == nz + nk + 1 + m.q_u_chol.size + m.q_u_mean.size
    assert np.array_equal(m.param_array[:nz], fx["Z"].ravel())
    _set_q(m, fx)
    g = m.gradient
    assert np.array_equal(g[nz + nk + 1:nz + nk + 1 + m.q_u_chol.size], m.grad_dict["dL_dchol"].ravel())
    assert np.array_equal(g[-m.q_u_mean.size:], m.grad_dict["dL_dm"].ravel())
    assert np.array_equal(g[:nz], m.grad_dict["fused"]["dZ"].ravel())
    assert gpy_amd.SVGP is gpy_amd.core.SVGP and gpy_amd.inference.latent_function_inference.SVGP is SVGPInference


def test_batch_scale_reaches_dF_but_not_the_KL(rctx):
    fx = S.load_fixture("bern_rbf_iso_l1_n300_m70_d2")
    out = {}
    for bs in (1.0, 3.0):
        inf = SVGPInference()
        _, bound, gd = inf.inference(fx["q_mean"], fx["q_chol"], S.make_kernel(fx), fx["X"], fx["Z"], S.make_likelihood(fx), fx["Y"],
                                     batch_scale=bs)
        out[bs] = (bound, gd, rctx[-1].dF)
    (b1, g1, dF1), (b3, g3, dF3) = out[1.0], out[3.0]
    assert g1["KL"] == g3["KL"]
    assert np.array_equal(dF3[0], 3.0 * dF1[0]) and np.array_equal(dF3[1], 3.0 * dF1[1])
    assert abs((b3 + g3["KL"]) - 3.0 * (b1 + g1["KL"])) <= 1e-12 * abs(b3)                    # F.sum() scales, the KL does not
    assert np.array_equal(g3["dL_dKdiag"], 3.0 * g1["dL_dKdiag"])
    # the model: batch_scale = N_all / N_batch
    m = _model(fx, batchsize=fx["X"].shape[0], seed=0, reps=3)
    m.set_data(fx["X"], fx["Y"])
    _set_q(m, fx)
    assert abs(m.log_likelihood() - b3) <= 1e-12 * abs(b3)


@pytest.mark.parametrize("name", ["gauss_rbf_white_l1_n180_m36_d2", "bern_prod_subset_l1_n170_m30_d4",
                                  "poisson_matern32_iso_l1_n140_m20_d2_bs3"])
def test_model_gradient_against_finite_differences(rctx, name):
    """checkgrad at a fixture's point: the directional derivative of the bound along 6 random unit directions of the whole flat
    parameter vector and along each parameter group on its own, by central differences with h = 1e-6.  With |bound| <= 5e3
    the rounding error of a difference is eps |bound| / h <= 1e-6 and the truncation h^2 |d3| / 6 is smaller; the gradient norms
    are 1e2 ... 1e4, so the bound is 1e-6 of the gradient's norm plus that 1e-6.

    The Student-t fixture is not among the cases: dF_dv is a quadrature of its own (of the second derivative of log p), and with
    t_scale2 = 0.3 and deg_free = 4 the poles of the integrand lie 1.1 from the real axis against sqrt(2 v) up to 1.8, where the
    reference's 20-point rule is 2e-2 from the derivative of its own F (1e-3 at 40 points, 5e-7 at 120): the reference's
    gradient, which the package reproduces to 1e-12 (tests/test_oracle_svgp.py), is not the gradient of its bound there."""
    fx = S.load_fixture(name)
    reps = int(round(fx["batch_scale"]))                      # batch_scale = N_all / N_batch: the fixture's rows as one minibatch
    m = _model(fx, batchsize=fx["X"].shape[0] if reps > 1 else None, seed=0, reps=reps)
    m.set_data(fx["X"], fx["Y"])
    _set_q(m, fx)
    x0, g = m.param_array.copy(), m.gradient.copy()
    assert abs(m.log_likelihood() - fx["bound"]) <= BOUND * abs(fx["bound"])
    rng = np.random.default_rng(1)
    nz, nk, nl = fx["Z"].size, fx["dtheta"].size, fx["dL_dthetaL"].size
    groups = [(0, nz), (nz, nz + nk), (nz + nk, nz + nk + nl), (nz + nk + nl, x0.size - fx["q_mean"].size), (x0.size - fx["q_mean"].size, x0.size)]
    dirs = [rng.standard_normal(x0.size) for _ in range(6)]
    for lo, hi in groups:
        if hi > lo:
            d = np.zeros(x0.size)
            d[lo:hi] = rng.standard_normal(hi - lo)
            dirs.append(d)
    h = 1e-6
    for d in dirs:
        d = d / np.linalg.norm(d)
        m.param_array = x0 + h * d
        fp = m.log_likelihood()
        m.param_array = x0 - h * d
        fm = m.log_likelihood()
        num = (fp - fm) / (2 * h)
        support = d != 0
        assert abs(num - g @ d) <= 1e-6 * np.linalg.norm(g[support]) + 1e-6, (num, g @ d)
    m.param_array = x0


def test_stochastic_grad_changes_the_batch_deterministically_under_a_seed(rctx):
    fx = S.load_fixture("gauss_rbf_iso_l1_n200_m30_d2")

    def run(seed):
        m = _model(fx, batchsize=64, seed=seed)
        x = m.optimizer_array.copy()
        batches, grads = [m.X.copy()], []
        for _ in range(5):
            grads.append(m.stochastic_grad(x))
            batches.append(m.X.copy())
        return m, batches, grads
    m, b0, g0 = run(7)
    _, b1, g1 = run(7)
    _, b2, _ = run(8)
    assert all(np.array_equal(a, b) for a, b in zip(b0, b1)) and all(np.array_equal(a, b) for a, b in zip(g0, g1))
    assert any(not np.array_equal(a, b) for a, b in zip(b0, b2) if a.shape == b.shape) or any(a.shape != b.shape for a, b in zip(b0, b2))
    assert any(not np.array_equal(b0[i], b0[i + 1]) for i in range(5) if b0[i].shape == b0[i + 1].shape)
    # contiguous slices that cover the data once per epoch: 200 rows in slices of 64 -> 4 batches, the last of 8 rows
    sizes = sorted(b.shape[0] for b in b0[:4])
    assert sizes == [8, 64, 64, 64]
    rows = np.concatenate(b0[:4])
    assert np.array_equal(np.sort(rows[:, 0]), np.sort(fx["X"][:, 0]))
    for b in b0:
        i = int(np.flatnonzero(np.all(fx["X"] == b[0], axis=1))[0])
        assert np.array_equal(fx["X"][i:i + b.shape[0]], b)
    # the gradient is the objective's in the optimiser's parameters (log of the positive ones), on the batch, scaled to all data
    assert g0[0].shape == m.optimizer_array.shape
    assert m.grad_dict["dL_dKdiag"].shape == (m.X.shape[0],)
    pos = m._positive()
    assert np.array_equal(g0[-1], np.where(pos, -m.gradient * m.param_array, -m.gradient))
    assert np.allclose(np.exp(m.optimizer_array[pos]), m.param_array[pos]) and np.array_equal(m.optimizer_array[~pos], m.param_array[~pos])


def test_the_jitter_ladder_is_climbed_for_Kmm(rctx):
    fx = S.load_fixture("gauss_rbf_iso_l1_n200_m30_d2")
    S.RestatementContext.fail_info = 7
    try:
        with pytest.raises(gpy_amd.linalg.LinAlgError, match="not positive definite"):
            SVGPInference().inference(fx["q_mean"], fx["q_chol"], S.make_kernel(fx), fx["X"], fx["Z"], S.make_likelihood(fx), fx["Y"])
    finally:
        S.RestatementContext.fail_info = 0
    var = float(fx["specs"][0][2][0])
    assert np.allclose(rctx[0].jitters, [0.0] + [var * 1e-6 * 10 ** i for i in range(5)])      # util/linalg.py:61-75


def test_refusals_by_name(rctx):
    fx = S.load_fixture("gauss_rbf_iso_l1_n200_m30_d2")
    k, lik, inf = S.make_kernel(fx), S.make_likelihood(fx), SVGPInference()
    args = (fx["q_mean"], fx["q_chol"], k, fx["X"], fx["Z"], lik, fx["Y"])
    with pytest.raises(NotImplementedError, match="mean function"):
        inf.inference(*args, mean_function=object())
    with pytest.raises(NotImplementedError, match="KL_scale"):
        inf.inference(*args, KL_scale=0.5)
    with pytest.raises(NotImplementedError, match="certain inputs"):
        inf.inference(fx["q_mean"], fx["q_chol"], k, gpy_amd.NormalPosterior(fx["X"], np.full(fx["X"].shape, 0.1)), fx["Z"], lik, fx["Y"])
    mixed = gpy_amd.MixedNoise([gpy_amd.Gaussian(), gpy_amd.Gaussian()])
    with pytest.raises(NotImplementedError, match="MixedNoise likelihood has no variational_expectations"):
        inf.inference(fx["q_mean"], fx["q_chol"], k, fx["X"], fx["Z"], mixed, fx["Y"])
    with pytest.raises(NotImplementedError, match="does not evaluate Linear kernels"):
        inf.inference(fx["q_mean"], fx["q_chol"], gpy_amd.Linear(2), fx["X"], fx["Z"], lik, fx["Y"])
    with pytest.raises(NotImplementedError, match="sparse path covers"):
        inf.inference(fx["q_mean"], fx["q_chol"], gpy_amd.White(2), fx["X"], fx["Z"], lik, fx["Y"])
    M = fx["q_mean"].shape[0]
    with pytest.raises(NotImplementedError, match="17 latent functions"):
        inf.inference(np.zeros((M, 17)), np.zeros((M * (M + 1) // 2, 17)), k, fx["X"], fx["Z"], lik, np.zeros((fx["X"].shape[0], 17)))
    assert rctx == [] or all(c.log == [] for c in rctx)                                        # nothing reached the device
    inf.inference(*args)
    rctx[0].sharded = True
    with pytest.raises(NotImplementedError, match="row-sharded"):
        inf.inference(*args)
    with pytest.raises(NotImplementedError, match="mean function"):
        gpy_amd.SVGP(fx["X"], fx["Y"], fx["Z"], k, lik, mean_function=object())
    with pytest.raises(NotImplementedError, match="certain inputs"):
        gpy_amd.SVGP(gpy_amd.NormalPosterior(fx["X"], np.full(fx["X"].shape, 0.1)), fx["Y"], fx["Z"], k, lik)


def test_a_later_call_makes_the_posterior_stale(rctx):
    fx = S.load_fixture("gauss_rbf_iso_l1_n200_m30_d2")
    k, lik, inf = S.make_kernel(fx), S.make_likelihood(fx), SVGPInference()
    post, _, _ = inf.inference(fx["q_mean"], fx["q_chol"], k, fx["X"], fx["Z"], lik, fx["Y"])
    wv = post.woodbury_vector.copy()
    inf.inference(0.5 * fx["q_mean"], fx["q_chol"], k, fx["X"], fx["Z"], lik, fx["Y"])
    assert np.array_equal(post.woodbury_vector, wv)                                            # fetched before: kept
    with pytest.raises(RuntimeError, match="overwritten by a later inference call"):
        post.woodbury_inv
