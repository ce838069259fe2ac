"""Trend plus wiggle with a sparse GP: a sine on a slope (seeded, nothing downloaded), fitted with
`SparseGPRegression(RBF + Linear + Bias)` and with an RBF kernel alone, both with M = 20 inducing inputs, and predicted well
outside the data.  Inside the data the two fits agree.  Outside, the RBF-only fit falls back to its prior mean of zero within a
few lengthscales, while the Linear part carries on what it took of the trend, with error bars that say how little the data pin
down the split between the two parts: its learned variance is printed next to both extrapolations.
The Linear kernel's diagonal K(x, x) = variance x^2 depends on the point, so the sparse bound, its gradients and the predictive
variance take Kdiag per point on the device; the sparse classes do that where they are asked to (`linear=True`).

    python examples/sparse_linear_regression.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpy_amd as GPy  # noqa: E402


def main():
    rng = np.random.default_rng(0)
    X = np.sort(rng.uniform(-3.0, 3.0, (400, 1)), 0)
    slope = 1.0
    Y = np.sin(3.0 * X) + slope * X + 0.1 * rng.standard_normal(X.shape)
    Z0 = np.linspace(-3.0, 3.0, 20)[:, None]
    Xin, Xout = np.array([[0.4]]), np.array([[8.0]])
    fits = (("RBF + Linear + Bias", GPy.kern.RBF(1, lengthscale=0.3) + GPy.kern.Linear(1) + GPy.kern.Bias(1)),
            ("RBF alone         ", GPy.kern.RBF(1, lengthscale=0.3)))
    for name, k in fits:
        m = GPy.models.SparseGPRegression(X, Y, kernel=k, Z=Z0.copy(), noise_var=0.1, linear=True)   # Linear leaves: asked for
        start = m.log_likelihood()
        m.optimize(max_iters=200)
        (mi, vi), (mo, vo) = m.predict_noiseless(Xin), m.predict_noiseless(Xout)
        print("%s bound % .2f -> % .2f  noise variance %.4f (true 0.0100)" % (
            name, start, m.log_likelihood(), float(np.ravel(m.likelihood.variance.values)[0])))
        print("%s   at x = 0.4: %.3f +- %.3f (f = %.3f)   at x = 8.0: %.3f +- %.3f (trend %.3f)" % (
            name, mi[0, 0], np.sqrt(vi[0, 0]), np.sin(1.2) + slope * 0.4, mo[0, 0], np.sqrt(vo[0, 0]), slope * 8.0))
        lin = [p for p in m.kern.leaves() if p.kind == "linear"]
        if lin:
            print("%s   learned slope variance %.3f (slope^2 = %.3f)" % (name, float(lin[0].variances.values[0]), slope ** 2))


if __name__ == "__main__":
    main()
