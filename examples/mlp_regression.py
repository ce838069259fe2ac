"""A step of finite width on a saturating trend (seeded, nothing downloaded) fitted with the arc-sine kernel, MLP + Bias, through
the drop-in API: fit, optimise, predict.  A stationary kernel has to choose one lengthscale for the jump and the plateaus; the
MLP kernel is not stationary and takes both.

    python examples/mlp_regression.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpy_amd as GPy  # noqa: E402


def main():
    rng = np.random.default_rng(0)
    X = rng.uniform(-3.0, 3.0, (300, 1))
    f = np.tanh(6.0 * (X[:, 0] - 0.5)) + 0.3 * np.tanh(X[:, 0])
    Y = (f + 0.1 * rng.standard_normal(X.shape[0]))[:, None]
    k = GPy.kern.MLP(1, variance=1.0, weight_variance=10.0, bias_variance=10.0) + GPy.kern.Bias(1)
    m = GPy.models.GPRegression(X, Y, k, noise_var=0.1)
    print("initial log likelihood %.3f" % m.log_likelihood())
    m.optimize(max_iters=200)
    lml = m.log_likelihood()
    assert np.isfinite(lml)
    print("fitted  log likelihood %.3f" % lml)
    mlp = k.parts[0]
    print("fitted MLP variance %.4f  weight_variance %.4f  bias_variance %.4f" % (
        mlp.variance.values[0], mlp.weight_variance.values[0], mlp.bias_variance.values[0]))
    Xf = np.array([[-2.0], [0.0], [0.4], [0.6], [1.0], [2.5]])
    mu, var = m.predict(Xf)
    for x, a, v in zip(Xf[:, 0], mu[:, 0], var[:, 0]):
        truth = np.tanh(6.0 * (x - 0.5)) + 0.3 * np.tanh(x)
        print("x = % .1f  predicted % .3f +- %.3f   (noise-free % .3f)" % (x, a, 2 * np.sqrt(v), truth))


if __name__ == "__main__":
    main()
