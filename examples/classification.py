"""Toy 1-D classification, the way the reference's `GPy/examples/classification.py` fits it
(`toy_linear_1d_classification_laplace` and `toy_linear_1d_classification`): two Gaussian classes on the line, a Bernoulli
likelihood with the probit link, an RBF kernel, `Laplace` inference and then `EP` inference on the same data, each followed
by hyper-parameter optimisation.

    python examples/classification.py
"""
import numpy as np

import gpy_amd as GPy


def toy_data(seed=4):
    rng = np.random.default_rng(seed)
    X = np.concatenate([rng.normal(-1.5, 1.0, 30), rng.normal(1.5, 1.0, 30)])[:, None]
    Y = np.concatenate([np.zeros(30), np.ones(30)])[:, None]
    return X, Y


def toy_linear_1d_classification_laplace(seed=4, optimize=True):
    X, Y = toy_data(seed)
    likelihood = GPy.likelihoods.Bernoulli()
    laplace_inf = GPy.inference.latent_function_inference.Laplace()
    kernel = GPy.kern.RBF(1)
    m = GPy.core.GP(X, Y, kernel=kernel, likelihood=likelihood, inference_method=laplace_inf)
    return _fit("Laplace", m, X, Y, optimize)


def toy_linear_1d_classification(seed=4, optimize=True):
    """the reference's default for GPClassification: expectation propagation ("alternated": EP runs once at the start of the
    optimisation, the hyper-parameters are then optimised against its sites)"""
    X, Y = toy_data(seed)
    np.random.seed(seed)                                  # EP draws the order of every sweep from NumPy's global generator
    m = GPy.models.GPClassification(X, Y, inference_method=GPy.inference.latent_function_inference.EP())
    return _fit("EP", m, X, Y, optimize)


def _fit(name, m, X, Y, optimize):
    print("%s: log marginal likelihood at the start: %.6f" % (name, m.log_likelihood()))
    if optimize:
        m.optimize()
    p, _ = m.predict(X)
    print("%s: log marginal likelihood: %.6f, kernel %s, training accuracy %.3f" % (
        name, m.log_likelihood(), m.kern.param_array, float(np.mean((p > 0.5) == (Y == 1)))))
    return m


if __name__ == "__main__":
    toy_linear_1d_classification_laplace()
    toy_linear_1d_classification()
