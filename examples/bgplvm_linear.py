"""Bayesian PCA: a Bayesian GP latent variable model with the kernel `Linear(ARD) + Bias + White`, on data generated here
(seeded, nothing loaded): Y = X W + offset + noise with TWO true latent dimensions, embedded in 8 output dimensions.  The model
is given four latent dimensions; the bound, with the KL term of the standard normal prior on the latent points, switches off
the two it does not need -- their ARD variances fall towards zero, which is what the printed variances show.  The Linear and
Bias psi-statistics run on the device where the model is made with `psi_lin_bias=True`; a step uploads the latent means and
variances only.  The fitted model then predicts at certain and at uncertain latent points.

    python examples/bgplvm_linear.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpy_amd as GPy  # noqa: E402


def data(seed=0, N=80, Dy=8):
    r = np.random.default_rng(seed)
    X = r.standard_normal((N, 2))
    W = r.standard_normal((2, Dy))
    return X @ W + 0.5 + 0.1 * r.standard_normal((N, Dy)), X


def main():
    Y, X_true = data()
    np.random.seed(1)
    Q = 4
    kernel = GPy.Linear(Q, ARD=True) + GPy.Bias(Q, variance=0.1) + GPy.White(Q, variance=0.01)
    m = GPy.models.BayesianGPLVM(Y, input_dim=Q, num_inducing=10, kernel=kernel, psi_lin_bias=True)
    print("objective at the PCA initialisation % .3f" % m.objective_function())
    m.optimize(max_iters=300)
    print("objective after optimisation       % .3f   noise variance %.5f"
          % (m.objective_function(), float(np.ravel(m.likelihood.variance.values)[0])))
    v = np.ravel(m.kern.parts[0].variances.values)
    print("ARD variances of the Linear part:", " ".join("%.5f" % a for a in v))
    print("latent dimensions in use (variance above 1%% of the largest): %d of %d (the data have 2)" % (int(np.sum(v > 0.01 * v.max())), Q))
    print("Bias variance %.4f  White variance %.5f" % (float(m.kern.parts[1].variance.values[0]), float(m.kern.parts[2].variance.values[0])))
    mean, var = m.X.mean.values[:3], m.X.variance.values[:3]
    mu_c, var_c = m.predict(mean)
    mu_u, var_u = m.predict(GPy.NormalPosterior(mean, var))
    for i in range(3):
        print("point %d: max |mean - Y| %.3f at its latent mean; mean predictive variance %.4f there, %.4f at q(x)"
              % (i, float(np.abs(mu_c[i] - Y[i]).max()), float(var_c[i].mean()), float(var_u[i].mean())))


if __name__ == "__main__":
    main()
