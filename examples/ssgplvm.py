"""Spike-and-slab GPLVM next to the Bayesian GPLVM: outputs that depend on two of five latent dimensions.

`SSGPLVM` switches a latent dimension off per point through the slab probabilities gamma; `BayesianGPLVM` does it per model
through the ARD lengthscales.  Both are fitted to the same data from the same start; printed are the mean gamma per dimension
next to the ARD weights 1 / l^2 of the two fits.

    python examples/ssgplvm.py          (needs the GPU)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpy_amd as GPy  # noqa: E402


def main(N=120, Q=5, Dy=8, M=20, iters=150, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N, Q))
    W = rng.standard_normal((2, Dy))
    Y = np.sin(X[:, :2]) @ W + np.cos(X[:, :1] * X[:, 1:2]) @ rng.standard_normal((1, Dy)) + 0.05 * rng.standard_normal((N, Dy))
    Y = (Y - Y.mean(0)) / Y.std(0)
    X0 = 0.5 * X + 0.5 * rng.standard_normal((N, Q))              # a start that remembers the truth in every dimension alike
    S0 = np.full((N, Q), 0.1)
    Z0 = X0[rng.permutation(N)[:M]].copy()
    np.random.seed(seed)
    ss = GPy.SSGPLVM(Y, Q, X=X0, X_variance=S0, Gamma=np.full((N, Q), 0.5), Z=Z0,
                     kernel=GPy.RBF(Q, ARD=True) + GPy.White(Q, variance=0.01), pi=0.5)
    bg = GPy.BayesianGPLVM(Y, Q, X=X0, X_variance=S0, Z=Z0, kernel=GPy.RBF(Q, ARD=True) + GPy.White(Q, variance=0.01))
    for name, m in (("SSGPLVM", ss), ("BayesianGPLVM", bg)):
        f0 = m.objective_function()
        m.optimize(max_iters=iters)
        print("%-14s objective %.2f -> %.2f" % (name, f0, m.objective_function()))
    print("dimension                 " + "  ".join("%6d" % q for q in range(Q)))
    print("SSGPLVM  mean gamma       " + "  ".join("%6.3f" % g for g in ss.X.binary_prob.values.mean(0)))
    print("SSGPLVM  ARD weight 1/l^2 " + "  ".join("%6.3f" % w for w in 1.0 / ss.kern.parts[0].lengthscale.values ** 2))
    print("BGPLVM   ARD weight 1/l^2 " + "  ".join("%6.3f" % w for w in 1.0 / bg.kern.parts[0].lengthscale.values ** 2))
    return ss, bg


if __name__ == "__main__":
    main()
