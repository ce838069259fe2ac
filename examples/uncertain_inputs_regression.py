"""A sine observed at input locations that are themselves known only up to noise (seeded, nothing downloaded): the recorded
x_n differs from the true location by a Gaussian error of known variance.  Sparse GP regression is fitted twice through the
drop-in API, once treating the recorded inputs as exact and once with `X_variance`, i.e. inputs q(x_n) = N(x_n, s_n^2)
whose RBF psi-statistics are evaluated on the device.  The inputs' distributions are data here, not parameters: the bound
averages the function over q(x_n), so the spread of f under q(x_n) is charged to the fit (the trace term of the bound) and
the two fits settle on different noise variances and lengthscales; both are printed next to the truth.

    python examples/uncertain_inputs_regression.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpy_amd as GPy  # noqa: E402


def main():
    rng = np.random.default_rng(0)
    N, s_in, s_out = 300, 0.3, 0.05
    x_true = rng.uniform(-3.0, 3.0, (N, 1))
    Y = np.sin(2.0 * x_true) + s_out * rng.standard_normal((N, 1))
    X = x_true + s_in * rng.standard_normal((N, 1))                  # what was recorded
    Z = np.linspace(-3.0, 3.0, 15)[:, None]
    Xf = np.linspace(-2.5, 2.5, 6)[:, None]
    for name, kw in (("certain inputs  ", {}), ("uncertain inputs", {"X_variance": np.full((N, 1), s_in ** 2)})):
        m = GPy.models.SparseGPRegression(X, Y, kernel=GPy.kern.RBF(1), Z=Z.copy(), noise_var=0.1, **kw)
        m.optimize(max_iters=200)
        mu, _ = m.predict(Xf, include_likelihood=False)
        print("%s log likelihood % .2f  noise variance %.4f (true %.4f)  lengthscale %.3f  max |mean - sin| %.3f"
              % (name, m.log_likelihood(), float(np.ravel(m.likelihood.variance.values)[0]), s_out ** 2,
                 float(np.ravel(m.kern.lengthscale.values)[0]), float(np.abs(mu - np.sin(2.0 * Xf)).max())))


if __name__ == "__main__":
    main()
