"""Robust regression, the shape of the reference's Student-t toy (`GPy/examples/regression.py`, a sine with a few corrupted
points): a Gaussian-noise GP against a GP with a Student-t likelihood and `Laplace` inference, both with an RBF kernel and both
optimised, and the error of each against the clean function.

    python examples/robust_regression.py
"""
import numpy as np

import gpy_amd as GPy


def toy_data(seed=12, N=150, corrupted=15):
    rng = np.random.default_rng(seed)
    X = np.sort(rng.uniform(0.0, 10.0, (N, 1)), 0)
    Y = np.sin(X) + 0.1 * rng.standard_normal(X.shape)
    idx = rng.choice(N, corrupted, replace=False)
    Y[idx, 0] += 5.0 * np.where(rng.random(corrupted) < 0.5, -1.0, 1.0)
    Xt = np.linspace(0.2, 9.8, 60)[:, None]
    return X, Y, Xt, np.sin(Xt)


def student_t_approx(seed=12, optimize=True, max_iters=50):
    X, Y, Xt, ft = toy_data(seed)
    m_gauss = GPy.models.GPRegression(X, Y, GPy.kern.RBF(1))
    t_distribution = GPy.likelihoods.StudentT(deg_free=5, sigma2=2)
    laplace_inf = GPy.inference.latent_function_inference.Laplace()
    m_t = GPy.core.GP(X, Y, kernel=GPy.kern.RBF(1), likelihood=t_distribution, inference_method=laplace_inf)
    for name, m in (("Gaussian", m_gauss), ("Student-t (Laplace)", m_t)):
        if optimize:
            m.optimize(max_iters=max_iters)
        err = float(np.sqrt(np.mean(np.square(m.predict_noiseless(Xt)[0] - ft))))
        print("%-20s log marginal likelihood %.4f, parameters %s, rms error to the clean function %.4f" % (
            name, m.log_likelihood(), np.array2string(m.param_array, precision=4), err))
    return m_gauss, m_t


if __name__ == "__main__":
    student_t_approx()
