"""Bayesian GP latent variable model on data generated here (seeded, nothing loaded): three labelled clusters on a 2-D latent
manifold, embedded non-linearly in 12 output dimensions.  The model is given five latent dimensions and an ARD RBF kernel; the
bound, with the KL term of the standard normal prior on the latent points, switches the dimensions it does not need off: their
ARD weights 1 / lengthscale^2 fall towards zero, which is what the printed weights show.  Every evaluation -- psi-statistics,
the bound, the gradients in the means and variances of q(X), Z and the kernel -- runs on the device; a step uploads the latent
means and variances only.  The fitted model then predicts at certain latent points (the cluster centres) and at uncertain ones
(the same centres with the clusters' spread as input variance).

    python examples/bgplvm.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpy_amd as GPy  # noqa: E402


def data(seed=0, n_per=30, Dy=12):
    r = np.random.default_rng(seed)
    centres = np.array([[-1.5, -1.0], [1.5, -0.5], [0.0, 1.6]])
    labels = np.repeat(np.arange(3), n_per)
    t = centres[labels] + 0.35 * r.standard_normal((3 * n_per, 2))
    A, B = r.standard_normal((2, Dy)), r.standard_normal((2, Dy))
    Y = np.sin(t @ A) + 0.5 * np.tanh(t @ B) * (t[:, :1] * t[:, 1:]) + 0.05 * r.standard_normal((3 * n_per, Dy))
    return Y, labels


def main():
    Y, labels = data()
    np.random.seed(1)
    m = GPy.models.BayesianGPLVM(Y, input_dim=5, num_inducing=15)
    print("objective at the PCA initialisation % .3f" % m.objective_function())
    m.optimize(max_iters=300)
    print("objective after optimisation       % .3f   noise variance %.5f"
          % (m.objective_function(), float(np.ravel(m.likelihood.variance.values)[0])))
    ard = 1.0 / np.ravel(m.kern.lengthscale.values) ** 2
    print("ARD weights 1 / lengthscale^2:", " ".join("%.4f" % a for a in ard))
    print("latent dimensions in use (weight above 1%% of the largest): %d of 5" % int(np.sum(ard > 0.01 * ard.max())))
    mean, var = m.X.mean.values, m.X.variance.values
    centres = np.stack([mean[labels == c].mean(0) for c in range(3)])
    spread = np.stack([mean[labels == c].var(0) + var[labels == c].mean(0) for c in range(3)])
    mu_c, var_c = m.predict(centres)
    mu_u, var_u = m.predict(GPy.NormalPosterior(centres, spread))
    for c in range(3):
        err = float(np.abs(mu_c[c] - Y[labels == c].mean(0)).max())
        print("cluster %d: at its centre  max |mean - cluster mean of Y| %.3f, mean predictive variance %.4f;  "
              "at N(centre, cluster spread) %.4f" % (c, err, float(var_c[c].mean()), float(var_u[c].mean())))


if __name__ == "__main__":
    main()
