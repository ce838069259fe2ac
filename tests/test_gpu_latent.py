"""GPU: the latent-input gradient pass (csrc/latent.hip) alone, inside the evaluation (`mi355gp_latent_inference_sum`) and
under the `GPLVM` model, against the long-double restatement of tests/latent_ld.py.

The kernel alone takes any symmetric W in the place of Ky^-1: tolerance max(16 d, 64 eps64) of max |value| per quantity, d = the
distance of latent_ld in fp64 from latent_ld in long double on the same input, measured at test time.  The evaluation is judged by
the exact path's rule, max(32 e64, 256 eps64 kappa) (tests/sparse_ld.py), with kappa = cond2(Ky) <= 1e4 asserted."""
import numpy as np
import pytest

import latent_ld as LL
import sparse_ld as SL

pytestmark = pytest.mark.gpu
KINDS = ("rbf", "matern52", "matern32", "exponential", "ratquad")
SLAB = 16                                                       # LKS of latent.hip: doubles of alpha per row in one k-slab

# (kind, ard, N, D, Dy, variant)
CASES = [("rbf", 1, N, 2, 3, "") for N in (1, 127, 128, 129, 257)]                                    # block edge, strips, J > I
CASES += [("matern52", 1, 129, D, 1, "") for D in (1, 15, 16, 31, 32)]                                 # the ones column moves
CASES += [("rbf", 0, 129, 3, Dy, "") for Dy in (1, 3, SLAB - 1, SLAB, SLAB + 1, 2 * SLAB + 1)]         # the remainder slab
CASES += [(k, ard, 130, 3, 5, "") for k in KINDS for ard in (0, 1)]
CASES += [("matern32", 1, 130, 3, 5, "twins"), ("exponential", 0, 130, 3, 5, "twins"), ("rbf", 1, 130, 3, 5, "offset")]


def _case(kind, ard, N, D, Dy, variant):
    rng = np.random.RandomState(1000 * N + 10 * D + Dy)
    X = rng.randn(N, D)
    if variant == "twins":
        X[70] = X[3]                                            # r = 0 off the diagonal, in another 64-column step: h = 0 there
    if variant == "offset":
        X += 100.0
    W = rng.randn(N, N) / np.sqrt(N)
    W = 0.5 * (W + W.T)
    theta = [1.3] + list(0.8 + rng.rand(D if ard else 1) * np.sqrt(D)) + ([1.7] if kind == "ratquad" else [])
    return np.array(theta), X, W, rng.randn(N, Dy)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s%d-n%d_d%d_dy%d%s" % c)
def test_the_kernel_alone_against_long_double(case):
    from gpy_amd import _lib
    kind, ard, N, D, Dy, variant = case
    theta, X, W, alpha = _case(*case)
    specs = [LL.spec(kind, ard, theta, range(D))]
    ref, r64 = LL.grad(specs, X, W, alpha), LL.grad(specs, X, W, alpha, np.float64)
    dX, rec = _lib.dbg_latent_grad(kind, ard, theta, X, W, alpha)
    got = (dX, LL.dtheta_from_records(kind, ard, theta, D, rec))
    for name, g, r, r6 in zip(("dX", "dtheta"), got, ref, r64):
        print("%s worst %.2e tolerance %.2e" % (name, LL.worst(g, r), LL.tol(r, r6)))
        assert g.shape == r.shape and LL.worst(g, r) <= LL.tol(r, r6), name
    again = _lib.dbg_latent_grad(kind, ard, theta, X, W, alpha)
    assert np.array_equal(again[0], dX) and np.array_equal(again[1], rec)


def _fit_case(N, Dy):
    rng = np.random.RandomState(N + Dy)
    X = rng.rand(N, 3) * 4.0
    specs = [("rbf", True, np.array([1.2, 0.9, 1.4]), np.array([0, 2], dtype=np.int32)), ("bias", False, np.array([0.3]), None)]
    ld_specs = [LL.spec("rbf", 1, specs[0][2], [0, 2]), LL.spec("bias", 0, specs[1][2], range(3))]
    return X, rng.randn(N, Dy), 0.35, specs, ld_specs


@pytest.mark.parametrize("N,Dy", [(129, 1), (129, 33), (257, 1), (257, 33)])
def test_the_evaluation_has_the_exact_entry_bytes_and_long_double_gradients(N, Dy):
    from gpy_amd import _lib
    X, Y, noise, specs, ld_specs = _fit_case(N, Dy)

    def run(entry):
        ctx = _lib.Context(0)
        ctx.set_data(X, Y)
        return getattr(ctx, entry)(specs, noise)[1]
    got, again, exact = run("latent_inference_sum"), run("latent_inference_sum"), run("exact_inference_sum")
    for q in ("lml", "logdet", "datafit", "dnoise", "trKinv", "alpha"):
        assert np.array_equal(got[q], exact[q]), q                # the same factor region
    for q in ("alpha", "dtheta", "dX", "lml"):
        assert np.array_equal(got[q], again[q]), q                # two fresh contexts, the same bytes
    ref, r64 = LL.evaluate(ld_specs, X, Y, noise), LL.evaluate(ld_specs, X, Y, noise, np.float64)
    kappa = float(np.linalg.cond(np.asarray(r64["Ki"], dtype=np.float64)))
    assert kappa <= 1e4
    assert not np.any(got["dX"][:, 1])                            # outside every part's active_dims
    for q in ("dtheta", "dX"):
        e, b = SL.rel_err(got[q], ref[q]), SL.bound(q, ref, r64, kappa)
        print("%s %.2e bound %.2e" % (q, e, b))
        assert e <= b, q


def test_gplvm_orders_its_parameters_checks_its_gradient_and_follows_X():
    import gpy_amd
    rng = np.random.RandomState(3)
    Y = np.tanh(rng.randn(20, 2).dot(rng.randn(2, 5))) + 0.05 * rng.randn(20, 5)
    m = gpy_amd.GPLVM(Y, 2)
    assert m.parameter_names()[:40] == ["latent_mean[%d]" % i for i in range(40)]
    assert [n.split(".")[0] for n in m.parameter_names()[40:]] == ["sum"] * 4 + ["Gaussian_noise"]
    np.random.seed(0)
    assert m.checkgrad()
    m.optimize(max_iters=5)
    assert m.checkgrad()
    specs = [LL.spec("rbf", 1, np.r_[m.kern.parts[0].variance, m.kern.parts[0].lengthscale], range(2)),
             LL.spec("bias", 0, m.kern.parts[1].variance, range(2))]
    args = (specs, np.asarray(m.X), Y, float(m.likelihood.variance[0]))                  # at the NEW X: set_X re-uploaded
    ref, r64 = LL.evaluate(*args), LL.evaluate(*args, dt=np.float64)
    kappa = float(np.linalg.cond(np.asarray(r64["Ki"], dtype=np.float64)))
    got = {"lml": m.log_likelihood(), "dX": m.X.gradient, "dtheta": m.gradient[40:44]}
    for q in got:
        assert SL.rel_err(got[q], ref[q]) <= SL.bound(q, ref, r64, kappa), q
    with pytest.raises(NotImplementedError, match="32"):
        gpy_amd.GPLVM(rng.randn(40, 3), 33, X=rng.randn(40, 33))
    with pytest.raises(NotImplementedError, match="Prod"):
        gpy_amd.GPLVM(Y, 2, kernel=gpy_amd.RBF(2) * gpy_amd.Matern32(2))
