"""Kronecker GP regression on a 2-D surface: Y (60 x 45) observed at all combinations of 60 points X1 and 45 points X2, with an RBF
kernel on one side and Matern32 + Bias on the other.  Fit, then predict between the points.

    python examples/kronecker_regression.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpy_amd as GPy  # noqa: E402


def surface(x1, x2):
    return np.sin(1.5 * x1) * np.cos(2.0 * x2.T) + 0.3 * x2.T


def main():
    rng = np.random.RandomState(0)
    X1, X2 = np.linspace(0, 4, 60)[:, None], np.linspace(-1, 2, 45)[:, None]
    Y = surface(X1, X2) + 0.05 * rng.randn(60, 45)
    m = GPy.models.GPKroneckerGaussianRegression(X1, X2, Y, GPy.kern.RBF(1), GPy.kern.Matern32(1) + GPy.kern.Bias(1), noise_var=0.1)
    print("log likelihood before: %.4f  (sweeps of the two decompositions: %s)" % (m.log_likelihood(), (m.sweeps,)))
    m.optimize(max_iters=60)
    print("log likelihood after:  %.4f" % m.log_likelihood())
    for name, value in zip(m.parameter_names(), m.param_array):
        print("  %-28s %.5f" % (name, value))
    X1n, X2n = (X1[:-1] + X1[1:]) / 2, (X2[:-1] + X2[1:]) / 2          # the midpoints: 59 x 44 new combinations
    mu, var = m.predict(X1n, X2n)
    truth = surface(X1n, X2n).flatten(order="F")
    rmse = float(np.sqrt(np.mean((mu[:, 0] - truth) ** 2)))
    print("RMSE at the %d midpoints: %.4f (noise sd 0.05); mean predictive sd %.4f" % (mu.size, rmse, float(np.sqrt(var).mean())))
    assert rmse < 0.05


if __name__ == "__main__":
    main()
