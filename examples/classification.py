"""Toy 1-D classification with the Laplace approximation, the way the reference's
`GPy/examples/classification.py:toy_linear_1d_classification_laplace` fits it: two Gaussian classes on the line, a Bernoulli
likelihood with the probit link, an RBF kernel, `Laplace` inference, then hyper-parameter optimisation.

    python examples/classification.py
"""
import numpy as np

import gpy_amd as GPy


def toy_linear_1d_classification_laplace(seed=4, optimize=True):
    rng = np.random.default_rng(seed)
    X = np.concatenate([rng.normal(-1.5, 1.0, 30), rng.normal(1.5, 1.0, 30)])[:, None]
    Y = np.concatenate([np.zeros(30), np.ones(30)])[:, None]
    likelihood = GPy.likelihoods.Bernoulli()
    laplace_inf = GPy.inference.latent_function_inference.Laplace()
    kernel = GPy.kern.RBF(1)
    m = GPy.core.GP(X, Y, kernel=kernel, likelihood=likelihood, inference_method=laplace_inf)
    print("log marginal likelihood at the start: %.6f" % m.log_likelihood())
    if optimize:
        m.optimize()
    p, _ = m.predict(X)
    print("log marginal likelihood: %.6f, kernel %s, training accuracy %.3f" % (
        m.log_likelihood(), m.kern.param_array, float(np.mean((p > 0.5) == (Y == 1)))))
    return m


if __name__ == "__main__":
    toy_linear_1d_classification_laplace()
