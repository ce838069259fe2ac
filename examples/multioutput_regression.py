"""Two related outputs observed at different inputs (the reference's test_multioutput_regression_1D: sin on [0, 8] and -sin
on [0, 5], seeded, nothing downloaded), fitted through the drop-in API with GPCoregionalizedRegression and its default kernel
(an ICM of an RBF) and one Gaussian noise per output, then predicted per output: the second output also where only the first
one was observed.

    python examples/multioutput_regression.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpy_amd as GPy  # noqa: E402


def main():
    rng = np.random.default_rng(0)
    np.random.seed(0)                                                   # the default W of Coregionalize is drawn with np.random
    X1 = rng.random((50, 1)) * 8
    X2 = rng.random((30, 1)) * 5
    Y1 = np.sin(X1) + rng.standard_normal(X1.shape) * 0.05
    Y2 = -np.sin(X2) + rng.standard_normal(X2.shape) * 0.05
    liks = [GPy.likelihoods.Gaussian(variance=0.01), GPy.likelihoods.Gaussian(variance=0.01)]
    m = GPy.models.GPCoregionalizedRegression(X_list=[X1, X2], Y_list=[Y1, Y2], likelihoods_list=liks)   # ICM of an RBF
    print("gradient check: %s" % m.checkgrad())
    print("initial log likelihood %.3f" % m.log_likelihood())
    m.optimize(max_iters=200)
    print("fitted  log likelihood %.3f" % m.log_likelihood())
    B = m.kern.parts[1]
    print("B =\n%s" % np.array2string(B.B, precision=3))
    Xt = np.linspace(0.0, 8.0, 9)[:, None]
    for j, name in enumerate(("sin", "-sin")):
        Xn = np.hstack([Xt, np.full_like(Xt, j)])                       # the output index goes in the last column
        mu, var = m.predict(Xn, Y_metadata={"output_index": np.full((Xt.shape[0], 1), j)})
        print("output %d (%s):" % (j, name))
        for x, mm, v in zip(Xt[:, 0], mu[:, 0], var[:, 0]):
            print("  x = %.1f  %+.3f +- %.3f" % (x, mm, 2 * np.sqrt(v)))


if __name__ == "__main__":
    main()
