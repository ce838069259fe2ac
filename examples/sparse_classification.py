"""Toy 1-D classification with a sparse model: `SparseGPClassification` (EPDTC over ten inducing inputs, the reference's
`GPy/examples/classification.py: sparse_toy_linear_1d_classification`) next to `GPClassification` with EP on all the points,
on the same two Gaussian classes on the line.  Both are optimised; the two predictive curves are compared on a grid.

    python examples/sparse_classification.py
"""
import numpy as np

import gpy_amd as GPy


def toy_data(seed=4, n=100):
    rng = np.random.default_rng(seed)
    X = np.concatenate([rng.normal(-1.5, 1.0, n), rng.normal(1.5, 1.0, n)])[:, None]
    Y = np.concatenate([np.zeros(n), np.ones(n)])[:, None]
    return X, Y


def sparse_toy_linear_1d_classification(seed=4, num_inducing=10, optimize=True):
    X, Y = toy_data(seed)
    np.random.seed(seed)                  # Z is a random subset of X, and EP draws the order of every sweep from NumPy's generator
    m = GPy.models.SparseGPClassification(X, Y, num_inducing=num_inducing)
    return _fit("SparseGPClassification (EPDTC, M = %d)" % num_inducing, m, X, Y, optimize)


def toy_linear_1d_classification(seed=4, optimize=True):
    X, Y = toy_data(seed)
    np.random.seed(seed)
    m = GPy.models.GPClassification(X, Y, inference_method=GPy.inference.latent_function_inference.EP())
    return _fit("GPClassification (EP, N = %d)" % X.shape[0], m, X, Y, optimize)


def _fit(name, m, X, Y, optimize):
    print("%s: bound at the start: %.6f" % (name, m.log_likelihood()))
    if optimize:
        m.optimize()
    p, _ = m.predict(X)
    print("%s: bound: %.6f, kernel %s, training accuracy %.3f" % (
        name, m.log_likelihood(), m.kern.param_array, float(np.mean((p > 0.5) == (Y == 1)))))
    return m


if __name__ == "__main__":
    sparse = sparse_toy_linear_1d_classification()
    full = toy_linear_1d_classification()
    grid = np.linspace(-5.0, 5.0, 201)[:, None]
    ps, pf = sparse.predict(grid)[0], full.predict(grid)[0]
    print("largest difference of the two predictive curves p(y = 1 | x) on [-5, 5]: %.4f (at x = %.2f)"
          % (float(np.abs(ps - pf).max()), float(grid[np.abs(ps - pf).argmax(), 0])))
