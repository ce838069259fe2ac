"""Toy 1-D classification with the variational Gaussian approximation (Opper and Archambeau 2009) next to the Laplace
approximation: the data of examples/classification.py, a Bernoulli likelihood with the probit link and an RBF kernel.
`GPVariationalGaussianApproximation` optimises a true lower bound of the log marginal likelihood over the kernel parameters
and its 2 N variational parameters (alpha, beta); `Laplace` optimises its approximation of it.

    python examples/vargauss_classification.py
"""
import numpy as np

import gpy_amd as GPy

from classification import toy_data


def fit(seed=4, max_iters=200):
    X, Y = toy_data(seed)
    grid = np.linspace(X.min() - 1.0, X.max() + 1.0, 200)[:, None]
    vg = GPy.models.GPVariationalGaussianApproximation(X, Y, GPy.kern.RBF(1), GPy.likelihoods.Bernoulli())
    lap = GPy.core.GP(X, Y, kernel=GPy.kern.RBF(1), likelihood=GPy.likelihoods.Bernoulli(),
                      inference_method=GPy.inference.latent_function_inference.Laplace())
    curves = {}
    for name, m in (("VarGauss", vg), ("Laplace", lap)):
        start = m.log_likelihood()
        m.optimize(max_iters=max_iters)
        p, _ = m.predict(X)
        curves[name] = m.predict(grid)[0]
        print("%-8s bound %.6f -> %.6f, kernel %s, training accuracy %.3f" % (
            name, start, m.log_likelihood(), m.kern.param_array, float(np.mean((p > 0.5) == (Y == 1)))))
    print("largest difference of the two predictive curves: %.4f" % float(np.abs(curves["VarGauss"] - curves["Laplace"]).max()))
    return vg, lap


if __name__ == "__main__":
    fit()
