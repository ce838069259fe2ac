"""Bayesian GPLVM with a Matern-5/2 kernel: the psi-statistics come from Gauss-Hermite quadrature on the device.

`VarDTC(psi_gh=True)` opts in to the quadrature (11 nodes, the same node in every latent dimension, as in the reference's
`PSICOMP_GH`); without it a Matern kernel under uncertain inputs is refused.  Outputs depend on two of three latent dimensions;
printed are the bound before and after the fit and the ARD weights 1 / l^2.

    python examples/bgplvm_matern.py          (needs the GPU)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpy_amd as GPy  # noqa: E402


def main(N=100, Q=3, Dy=6, M=15, iters=100, seed=0):
    rng = np.random.default_rng(seed)
    t = rng.uniform(-1.5, 1.5, (N, 2))
    Y = np.hstack([np.sin(2 * t), np.cos(t), t[:, :1] * t[:, 1:], np.abs(t[:, :1])]) + 0.05 * rng.standard_normal((N, Dy))
    Y = (Y - Y.mean(0)) / Y.std(0)
    np.random.seed(seed)
    m = GPy.models.BayesianGPLVM(Y, Q, num_inducing=M, kernel=GPy.kern.Matern52(Q, ARD=True),
                                 inference_method=GPy.inference.latent_function_inference.VarDTC(psi_gh=True))
    f0 = m.objective_function()
    m.optimize(max_iters=iters)
    print("objective %.2f -> %.2f" % (f0, m.objective_function()))
    print("ARD weights 1/l^2 " + "  ".join("%6.3f" % w for w in 1.0 / m.kern.lengthscale.values ** 2))
    mu, var = m.predict(m.X.mean.values[:3])
    print("prediction at the first three latent means:\n", np.round(mu, 3))
    return m


if __name__ == "__main__":
    main()
