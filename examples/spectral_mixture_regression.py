"""A seeded 1-D signal with two incommensurate periods (1 and sqrt 7) under a slow trend, fitted with a spectral-mixture kernel
(Wilson and Adams 2013): a sum of three `ExpQuadCosine` parts plus `Bias`, through the drop-in API.  The periods are learned
from the data -- `StdPeriodic` would need them fixed in advance -- and the fit extrapolates beyond the data, where an `RBF` fit
of the same points falls back to its mean.

`ExpQuadCosine` is k(r) = variance exp(-2 pi^2 r^2) cos(2 pi r / period) in the scaled distance r = |x - x'| / lengthscale, so
the period in input units is lengthscale x period and the envelope's width is lengthscale / (2 pi).

    python examples/spectral_mixture_regression.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpy_amd as GPy  # noqa: E402

# the start: [variance, lengthscale, period] of the three parts, Bias variance, noise variance.  Two parts start near (not at)
# the two periods -- 1.1 and 2.4 in input units -- the third is the trend: a period far beyond the data.
THETA0 = np.array([0.5, 30.0, 1.1 / 30.0, 0.3, 40.0, 2.4 / 40.0, 0.5, 60.0, 5.0, 0.1, 0.05])


def signal(N, half_width, seed):
    rng = np.random.default_rng(seed)
    x = np.sort(rng.uniform(-half_width, half_width, N))
    return x[:, None], truth(x)[:, None] + 0.1 * rng.standard_normal((N, 1))


def truth(x):
    return np.sin(2 * np.pi * x) + 0.6 * np.sin(2 * np.pi * x / np.sqrt(7.0) + 0.4) + 0.15 * x


def build_model(X, Y, theta0=THETA0):
    parts = [GPy.kern.ExpQuadCosine(1, variance=theta0[3 * i], lengthscale=theta0[3 * i + 1], period=theta0[3 * i + 2])
             for i in range(3)]
    k = parts[0] + parts[1] + parts[2] + GPy.kern.Bias(1, variance=theta0[9])
    return GPy.models.GPRegression(X, Y, k, noise_var=theta0[10])


def learned_periods(kern):
    """the periods of the ExpQuadCosine parts in input units"""
    return np.array([float(p.lengthscale.values[0]) * float(p.period.values[0]) for p in kern.leaves()
                     if isinstance(p, GPy.kern.ExpQuadCosine)])


def main():
    X, Y = signal(400, 10.0, 0)
    m = build_model(X, Y)
    print("initial log likelihood %.3f" % m.log_likelihood())
    m.optimize(max_iters=300)
    print("fitted  log likelihood %.3f" % m.log_likelihood())
    print("learned periods (input units): %s   (the signal's: 1 and %.4f)" % (
        np.array2string(np.sort(learned_periods(m.kern)), precision=4), np.sqrt(7.0)))
    r = GPy.models.GPRegression(X, Y, GPy.kern.RBF(1) + GPy.kern.Bias(1))
    r.optimize(max_iters=300)
    Xf = np.linspace(10.0, 13.0, 121)[:, None]                       # beyond the data
    rmse = lambda model: float(np.sqrt(np.mean((model.predict(Xf)[0][:, 0] - truth(Xf[:, 0])) ** 2)))
    print("extrapolation RMSE on [10, 13]: spectral mixture %.3f, RBF %.3f" % (rmse(m), rmse(r)))


if __name__ == "__main__":
    main()
