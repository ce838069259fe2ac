"""Exact GP regression on a 3-D grid with `GPRegressionGrid`: 48 x 40 x 32 = 61440 noisy observations of a smooth function, where
the dense exact path would factor a 61440 x 61440 matrix.  The covariance of an RBF over a Cartesian grid is a Kronecker product of
three small matrices, so one evaluation is a few tensor mode products on vectors of 61440 doubles.  The fit optimises the three
lengthscales, the variance and the noise; the prediction is at points BETWEEN the grid points.

X must be the full grid, one row per grid point, with the last column varying fastest (`numpy.meshgrid(..., indexing="ij")`).

    python examples/grid_regression.py
"""
import numpy as np

import gpy_amd as GPy


def f(X):
    return np.sin(1.2 * X[:, 0]) * np.cos(0.8 * X[:, 1]) + 0.5 * np.tanh(X[:, 2] - 1.0)


def fit(sizes=(48, 40, 32), seed=2, max_iters=50):
    rng = np.random.default_rng(seed)
    axes = [np.sort(rng.uniform(0.0, 5.0, g)) for g in sizes]                    # an irregular grid: any distinct values do
    X = np.array(np.meshgrid(*axes, indexing="ij")).reshape(len(axes), -1).T
    Y = f(X)[:, None] + 0.1 * rng.standard_normal((X.shape[0], 1))
    m = GPy.models.GPRegressionGrid(X, Y, GPy.kern.RBF(3, ARD=True))
    start = m.log_likelihood()
    m.optimize(max_iters=max_iters)
    print("N = %d: log marginal %.3f -> %.3f, lengthscales %s, variance %.3f, noise variance %.4f" % (
        X.shape[0], start, m.log_likelihood(), np.round(np.asarray(m.kern.lengthscale), 3), float(m.kern.variance[0]),
        float(m.likelihood.variance[0])))
    Xs = np.column_stack([rng.uniform(a[0], a[-1], 200) for a in axes])          # between the grid points
    mu, var = m.predict(Xs)
    err = mu.ravel() - f(Xs)
    print("200 points between the grid points: rms error %.4f, mean predictive sd %.4f" % (
        float(np.sqrt(np.mean(err ** 2))), float(np.sqrt(var).mean())))
    return m


if __name__ == "__main__":
    fit()
