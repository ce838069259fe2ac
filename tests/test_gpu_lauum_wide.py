"""GPU (-m gpu): X^T X on the 128 x 256 tile (`k_lauum_wide`) against the 128 x 128 tile (`k_lauum`) through `mi355gp_dbg_lauum`.

The wide tile keeps the slab size, the k -> MFMA-slice assignment and the accumulation order of the 128 x 128 one, so every
element of W sees the same fma chain: the two must agree BIT FOR BIT.  Sizes: nt = 2, 3, 4, 5, 9 tiles per dimension -- even and
odd tile rows, the diagonal block alone (even row) and as the second half of a pair (odd row), one and several pairs per row.
X is lower triangular: zeros above the diagonal inside the diagonal tiles, NaN in every tile strictly above it, so a tile that
must not be read poisons the result.

One size is also held against numpy in long double.  Bound: an element of W is a sum of K products accumulated by fma in some
order, so |W_ij - exact| <= gamma_K (|X|^T |X|)_ij with gamma_K = K u / (1 - K u), u = 2^-53 (Higham, Accuracy and Stability,
eq. 3.5; every fma rounds once, so the constant is K, not 2K - 1) -- the bound the 128 x 128 kernel meets for the same reason."""
import numpy as np
import pytest

from gpy_amd import _lib as L

pytestmark = pytest.mark.gpu

SIZES = (256, 384, 512, 640, 1152)


def _lower_with_poison(n, seed):
    rng = np.random.default_rng(seed)
    X = np.tril(rng.standard_normal((n, n)))
    nt = n // 128
    for ti in range(nt):
        X[ti * 128:(ti + 1) * 128, (ti + 1) * 128:] = np.nan      # tiles strictly above the diagonal
    return X


@pytest.fixture(scope="module")
def products():
    """n -> (X, W on the 128 x 128 tile, W on the 128 x 256 tile): computed once, never modified"""
    out = {}
    for n in SIZES:
        X = _lower_with_poison(n, seed=n)
        W0, _ = L.dbg_lauum(X, 0)
        W1, _ = L.dbg_lauum(X, 1)
        for a in (X, W0, W1):
            a.setflags(write=False)
        out[n] = (X, W0, W1)
    return out


@pytest.mark.parametrize("n", SIZES)
def test_wide_tile_equals_the_128_tile_bit_for_bit(products, n):
    _, W0, W1 = products[n]
    il = np.tril_indices(n)
    assert not np.isnan(W0[il]).any() and not np.isnan(W1[il]).any()
    assert np.array_equal(W1[il].view(np.int64), W0[il].view(np.int64))
    assert np.abs(W1[il]).max() > 1.0                             # something was computed


def test_wide_tile_against_long_double(products):
    n = 640
    X, W0, W1 = products[n]
    Xl = np.where(np.isnan(X), 0.0, X).astype(np.longdouble)     # the poisoned tiles are zeros of the triangular matrix
    ref = Xl.T @ Xl
    mag = np.abs(Xl).T @ np.abs(Xl)
    il = np.tril_indices(n)
    Ku = n * 2.0 ** -53                                           # K <= n rows for every element
    bound = (Ku / (1.0 - Ku)) * mag[il]
    for W in (W1, W0):
        err = np.abs(W[il].astype(np.longdouble) - ref[il])
        worst = float((err / bound).max())
        print("n=%d: max |err| / bound = %.3f, max |err| = %.3e" % (n, worst, float(err.max())))
        assert worst <= 1.0
