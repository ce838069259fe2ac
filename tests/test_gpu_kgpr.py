"""GPU: Kronecker GP regression with two arbitrary kernels (gpy_amd/kgpr.py, csrc/kgpr.hip).

1. `k_kgpr_wsyrk` alone through `mi355gp_kgpr_wsyrk` on exact integers: entries in -3 .. 3, weights in -4 .. 4, every sum exact in
   float64, so the result equals the integer computation byte for byte and is exactly symmetric.
2. The model against the dense long-double yardstick of tests/kgpr_ld.py, GIVEN THE SAME factor matrices (the device-built K1, K2 and
   cross-covariances).  Bound: the device's distance from long double, relative to max |value|, is at most ten times
   the float64 restatement's own distance on the same inputs, with a floor of max(N1, N2) eps -- the backward error of a sum of
   that length, which keeps a lucky restatement from setting a bound of zero.  The restatement itself has to stay within 1e-9:
   the inputs are not ill-posed.  The kernel-parameter gradients are the model's `gradient` against the same kernels'
   `update_gradients_full` of the yardstick's dL_dK, under the same rule.
3. Two evaluations in fresh contexts give the same bytes; `checkgrad`; `optimize` does not lower the log likelihood."""
import numpy as np
import pytest

import gpy_amd
from gpy_amd import _lib

import kgpr_ld as KL

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
SHAPES = [(1, 1), (1, 7), (7, 1), (33, 17), (64, 8), (65, 9), (4, 129), (129, 4)]
PAIRS = {"rbf,mat32": lambda: (gpy_amd.RBF(1, variance=1.3, lengthscale=0.7), gpy_amd.Matern32(1, variance=0.8, lengthscale=0.5)),
         "rbf+bias,lin*rbf": lambda: (gpy_amd.RBF(1, variance=0.9, lengthscale=0.6) + gpy_amd.Bias(1, variance=0.4),
                                      gpy_amd.Linear(1, variances=0.7) * gpy_amd.RBF(1, variance=1.1, lengthscale=0.8))}


@pytest.mark.parametrize("widths", [(1, 1), (15, 17), (16, 128), (33, 130)])
@pytest.mark.parametrize("n", [1, 127, 128, 129, 257])
def test_wsyrk_is_exact_on_integers(n, widths):
    rng = np.random.RandomState(n * 1000 + widths[0])
    (Pa, da), (Pb, db) = ((rng.randint(-3, 4, (n, k)), rng.randint(-4, 5, k)) for k in widths)
    want = (np.dot(Pa * da, Pa.T) + np.dot(Pb * db, Pb.T)) / 2.0               # int64, then one exact halving
    C, _ = _lib.kgpr_wsyrk(Pa, da, Pb, db)
    assert C.tobytes() == want.astype(np.float64).tobytes()
    assert np.array_equal(C, C.T)


def _problem(N1, N2, pair, seed):
    rng = np.random.RandomState(seed)
    X1, X2 = np.linspace(0, 3, N1)[:, None], np.linspace(-1, 1, N2)[:, None]
    Y = np.sin(2 * X1) * np.cos(3 * X2.T) + 0.1 * rng.randn(N1, N2)
    k1, k2 = PAIRS[pair]()
    return X1, X2, Y, k1, k2, rng.uniform(0.05, 0.3), rng.uniform(0, 3, (3, 1)), rng.uniform(-1, 1, (130, 1))


@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("N1, N2", SHAPES)
def test_model_against_the_dense_long_double_yardstick(N1, N2, pair):
    X1, X2, Y, k1, k2, noise, X1n, X2n = _problem(N1, N2, pair, 7 * N1 + N2)
    m = gpy_amd.GPKroneckerGaussianRegression(X1, X2, Y, k1, k2, noise_var=noise)
    got = dict(lml=m.log_likelihood(), dsig=m.gradient[-1], dK1=m.grad_dict["dL_dK1"], dK2=m.grad_dict["dL_dK2"], grad=m.gradient[:-1].copy())
    got["mu"], got["var"] = (a[:, 0] for a in m.predict(X1n, X2n))
    assert np.array_equal(got["dK1"], got["dK1"].T) and np.array_equal(got["dK2"], got["dK2"].T)
    K1, K2, cross = k1.K(X1), k2.K(X2), (k1.K(X1n, X1), k2.K(X2n, X2), k1.Kdiag(X1n), k2.Kdiag(X2n))
    ref = KL.dense(K1, K2, Y, noise, *cross)
    r64 = KL.restate(K1, K2, Y, noise)
    r64["mu"], r64["var"] = KL.restate_predict(r64, *cross)

    def param_grad(d):                         # the kernels' own chain rule applied to a dL_dK pair
        k1.update_gradients_full(np.asarray(d["dK1"], np.float64), X1)
        k2.update_gradients_full(np.asarray(d["dK2"], np.float64), X2)
        return np.concatenate([k1.gradient, k2.gradient])
    ref["grad"], r64["grad"] = param_grad(ref), param_grad(r64)
    floor = max(N1, N2) * EPS
    for what in ("lml", "dsig", "dK1", "dK2", "grad", "mu", "var"):
        own, dev = KL.rel(r64[what], ref[what]), KL.rel(got[what], ref[what])
        print("%dx%d %s %s: restatement %.3e device %.3e bound %.3e" % (N1, N2, pair, what, own, dev, 10 * max(own, floor)))
        assert own <= 1e-9, (what, own)
        assert dev <= 10 * max(own, floor), (what, dev, own)


def test_two_fresh_contexts_give_the_same_bytes():
    out = []
    for _ in range(2):
        X1, X2, Y, k1, k2, noise, X1n, X2n = _problem(65, 9, "rbf+bias,lin*rbf", 3)
        m = gpy_amd.GPKroneckerGaussianRegression(X1, X2, Y, k1, k2, noise_var=noise)
        mu, var = m.predict(X1n, X2n)
        out.append(b"".join(np.asarray(a, np.float64).tobytes() for a in (m.log_likelihood(), m.gradient, m.grad_dict["dL_dK1"],
                                                                           m.grad_dict["dL_dK2"], mu, var, m.Wi, m.Ytilde, m.U1, m.U2)))
    assert out[0] == out[1]


def test_checkgrad_and_optimize():
    X1, X2, Y, k1, k2, noise, _, _ = _problem(33, 17, "rbf,mat32", 5)
    m = gpy_amd.GPKroneckerGaussianRegression(X1, X2, Y, k1, k2, noise_var=noise)
    np.random.seed(0)
    assert m.checkgrad()
    before = m.log_likelihood()
    m.optimize(max_iters=5)
    assert m.log_likelihood() >= before
