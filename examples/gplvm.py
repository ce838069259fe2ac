"""GPLVM on a synthetic low-rank data set: 300 points on a two-dimensional sheet, observed through 40 noisy output columns.
The latent inputs are parameters; every optimiser step is one device call that returns the objective, the kernel's gradients and
dL/dX together (needs the MI355X).

    python examples/gplvm.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpy_amd  # noqa: E402


def main():
    rng = np.random.RandomState(0)
    Z = rng.randn(300, 2)
    Y = np.tanh(Z.dot(rng.randn(2, 40))) + 0.05 * rng.randn(300, 40)
    m = gpy_amd.GPLVM(Y, 2)
    print("parameters: %d (X %d, kernel %d, noise 1)" % (m.size, m.X.size, m.kern.size))
    print("log marginal likelihood at the PCA start: %.3f   checkgrad: %s" % (m.log_likelihood(), m.checkgrad()))
    m.optimize(max_iters=100)
    print("after 100 steps: %.3f   noise variance %.4f" % (m.log_likelihood(), float(m.likelihood.variance[0])))
    mu, var = m.predict(np.asarray(m.X)[:5])
    print("reconstruction error of the first rows: %.3e" % np.abs(mu - Y[:5]).max())


if __name__ == "__main__":
    main()
