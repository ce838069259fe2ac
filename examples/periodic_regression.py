"""A CO2-like series (trend + annual cycle + noise on calendar-year inputs, seeded, nothing downloaded) fitted with the
Mauna-Loa composite of Rasmussen & Williams section 5.4.3, RBF + RBF * StdPeriodic + RatQuad + White, through the drop-in
API, then predicted five years ahead.

    python examples/periodic_regression.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpy_amd as GPy  # noqa: E402


def main():
    rng = np.random.default_rng(0)
    x = np.arange(1960.0, 2020.0, 1.0 / 12.0)                            # monthly, 60 years
    y = 315.0 + 1.3 * (x - 1960.0) + 0.012 * (x - 1960.0) ** 2 + 3.0 * np.sin(2 * np.pi * x) + 0.4 * rng.standard_normal(x.size)
    X, Y = x[:, None], ((y - y.mean()) / y.std())[:, None]
    # starting values on the scale of the standardised series: the annual cycle is ~0.1 of its spread, the noise ~0.01
    k = (GPy.kern.RBF(1, variance=1.0, lengthscale=30.0)
         + GPy.kern.RBF(1, variance=0.005, lengthscale=60.0) * GPy.kern.StdPeriodic(1, variance=1.0, period=1.05, lengthscale=1.0)
         + GPy.kern.RatQuad(1, variance=1e-3, lengthscale=10.0, power=1.0)
         + GPy.kern.White(1, variance=1e-5))
    m = GPy.models.GPRegression(X, Y, k, noise_var=1e-4)
    print("initial log likelihood %.3f" % m.log_likelihood())
    m.optimize(max_iters=200)
    print("fitted  log likelihood %.3f" % m.log_likelihood())
    per = k.parts[1].parts[1]
    print("fitted period: %.4f years" % float(per.period.values[0]))
    Xf = np.arange(2020.0, 2025.0, 1.0 / 12.0)[:, None]
    mu, var = m.predict(Xf)
    mu = mu[:, 0] * y.std() + y.mean()
    sd = np.sqrt(var[:, 0]) * y.std()
    for i in range(0, Xf.shape[0], 12):
        print("%.2f  %.2f +- %.2f" % (Xf[i, 0], mu[i], 2 * sd[i]))


if __name__ == "__main__":
    main()
