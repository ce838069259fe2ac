"""GPU: the device eigensolver of symmetric positive semi-definite matrices (csrc/eigh.hip) through `gpy_amd.linalg.eigh`.

Sizes around the block width b = 32: n in {1, 2, b-1, b, b+1, 2b-1, 2b, 2b+1, 3b (an odd number of blocks: the tournament's bye),
5b+3}; matrices: RBF on clustered 1-D inputs (numerical rank far below n), Matern32 on scattered inputs (well conditioned), Linear
with D = 3 (an exact null space), the identity, a diagonal with every value four times.  One larger case, n = 16 b = 512 on a smooth RBF
matrix + 1e-6 I (scattered 2-D inputs): columns that start nearly parallel and of equal norm, sixteen blocks, where convergence
within the sweep cap hangs on the order in which a pair's columns leave the subproblem.

Judged in long double, A the float64 input, the yardstick `numpy.linalg.eigh` on the same matrix and never the code under test:
  R = max|A V - V diag(w)| / ||A||_2 and O = max|V^T V - I| are each held to max(8 x LAPACK's figure, n eps): two backward-stable
  methods whose error constants grow like a low power of n;
  |w - w_lapack| <= n ||A||_2 (R_dev + R_lapack + O_dev + O_lapack), Weyl's bound on the two backward errors;
  w ascending, two calls give the same bytes, no sweep cap reached.
Every figure is printed before it is held to its bound (pytest -s shows them)."""
import functools

import numpy as np
import pytest

from gpy_amd import _lib as L
from gpy_amd import linalg

LD = np.longdouble
EPS = np.finfo(np.float64).eps
B = L.EIGH_B
SIZES = [1, 2, B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 1, 3 * B, 5 * B + 3]
KINDS = ["rbf_clustered", "matern32", "linear3", "identity", "diag4"]
CASES = [(k, n) for k in KINDS for n in SIZES] + [("rbf_smooth", 16 * B)]
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(np.finfo(LD).eps >= EPS, reason="np.longdouble is not an extended format here")]


def matrix(kind, n):
    rng = np.random.default_rng(1000 * (KINDS + ["rbf_smooth"]).index(kind) + n)
    if kind == "rbf_smooth":
        X = rng.uniform(0.0, 10.0, (n, 2))
        return np.exp(-0.5 * ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1) / 1.5 ** 2) + 1e-6 * np.eye(n)
    if kind == "rbf_clustered":
        x = np.repeat([-2.0, 0.5, 3.0], (n + 2) // 3)[:n] + 1e-3 * rng.standard_normal(n)
        return 1.7 * np.exp(-0.5 * (x[:, None] - x[None, :]) ** 2)
    if kind == "matern32":
        X = rng.uniform(0.0, np.sqrt(n), (n, 2))
        r = np.sqrt(3.0 * ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)) / 0.6
        return 0.8 * (1.0 + r) * np.exp(-r)
    if kind == "linear3":
        X = rng.standard_normal((n, 3))
        A = (X[:, None, :] * X[None, :, :] * np.array([0.5, 1.0, 2.0])).sum(-1)
        return 0.5 * (A + A.T)
    if kind == "identity":
        return np.eye(n)
    return np.diag(1.0 + (np.arange(n) // 4) * 0.25)


def figures(A, w, V):
    """(R, O) in long double"""
    Al, Vl = A.astype(LD), V.astype(LD)
    R = np.abs(Al @ Vl - Vl * w.astype(LD)[None, :]).max() / LD(np.linalg.norm(A, 2))
    O = np.abs(Vl.T @ Vl - np.eye(A.shape[0], dtype=LD)).max()
    return float(R), float(O)


@functools.lru_cache(maxsize=None)
def lapack(kind, n):
    A = matrix(kind, n)
    w, V = np.linalg.eigh(A)
    return (A, w) + figures(A, w, V)


@pytest.mark.parametrize("kind, n", CASES)
def test_eigh_against_lapack_in_long_double(kind, n):
    A, wl, Rl, Ol = lapack(kind, n)
    if kind == "rbf_clustered" and n >= 2 * B:
        assert (wl < 1e-12 * wl[-1]).sum() >= n / 3.0, "the clustered RBF matrix is not rank-deficient enough"
    w, V, info = linalg.eigh(A, return_info=True)
    R, O = figures(A, w, V)
    nrm = np.linalg.norm(A, 2)
    dw = np.abs(w - wl).max()
    bw = n * nrm * (R + Rl + O + Ol)
    print("eigh %-13s n %3d sweeps %2d  R %.2e (lapack %.2e)  O %.2e (lapack %.2e)  |dw| %.2e (bound %.2e)"
          % (kind, n, info["sweeps"], R, Rl, O, Ol, dw, bw))
    assert w.shape == (n,) and V.shape == (n, n)
    assert info["sweeps"] < info["max_sweeps"]
    assert np.all(np.diff(w) >= 0.0)
    assert R <= max(8.0 * Rl, n * EPS)
    assert O <= max(8.0 * Ol, n * EPS)
    assert dw <= bw
    w2, V2 = linalg.eigh(A)
    assert w.tobytes() == w2.tobytes() and V.tobytes() == V2.tobytes()
