"""A linear trend with a smooth departure and an offset (seeded, nothing downloaded) fitted with GPy's stock regression
kernel, RBF + Linear + Bias, through the drop-in API: fit, optimise, predict inside and outside the data, where the Linear
part carries the trend on and the predictive variance grows with the distance from the origin.

    python examples/linear_regression.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpy_amd as GPy  # noqa: E402


def main():
    rng = np.random.default_rng(0)
    X = rng.uniform(-3.0, 3.0, (400, 2))
    f = 1.5 + 0.8 * X[:, 0] - 0.4 * X[:, 1] + 0.5 * np.sin(2.0 * X[:, 0])
    Y = (f + 0.1 * rng.standard_normal(X.shape[0]))[:, None]
    k = GPy.kern.RBF(2, variance=1.0, lengthscale=1.0) + GPy.kern.Linear(2, ARD=True) + GPy.kern.Bias(2)
    m = GPy.models.GPRegression(X, Y, k, noise_var=0.1)
    print("initial log likelihood %.3f" % m.log_likelihood())
    m.optimize(max_iters=200)
    print("fitted  log likelihood %.3f" % m.log_likelihood())
    lin = k.parts[1]
    print("fitted Linear variances: %s   input sensitivity: %s" % (np.round(lin.variances.values, 4),
                                                                  np.round(lin.input_sensitivity(), 4)))
    Xf = np.array([[0.0, 0.0], [2.0, -1.0], [4.0, 0.0], [6.0, 0.0], [8.0, 2.0]])     # the last three lie outside the data
    mu, var = m.predict(Xf)
    for x, a, v in zip(Xf, mu[:, 0], var[:, 0]):
        trend = 1.5 + 0.8 * x[0] - 0.4 * x[1]
        print("x = (% .1f, % .1f)  predicted % .3f +- %.3f   (trend % .3f)" % (x[0], x[1], a, 2 * np.sqrt(v), trend))


if __name__ == "__main__":
    main()
