"""Sparse binary classification with SVGP: a full-batch fit by L-BFGS-B, then a few hundred Adadelta steps on minibatches through
`stochastic_grad` (the reference's `GPy.core.SVGP`, Hensman, Matthews and Ghahramani 2015).  Needs the MI355X.

    python examples/svgp_classification.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpy_amd  # noqa: E402


def data(N, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, (N, 2))
    f = np.sin(2.0 * X[:, 0]) + np.cos(1.5 * X[:, 1]) - 0.3
    Y = (rng.random(N) < 0.5 * (1.0 + np.tanh(2.5 * f))).astype(float)[:, None]
    return X, Y


def accuracy(m, X, Y):
    mu, var = m._raw_predict(X)
    p = m.likelihood.predictive_mean(mu, var)
    return float(np.mean((p[:, 0] > 0.5) == (Y[:, 0] == 1)))


def adadelta(m, steps, rho=0.9, eps=1e-6):
    """hand-written Adadelta (Zeiler 2012) on the model's optimizer_array; a stochastic optimiser is not part of the package"""
    x = m.optimizer_array.copy()
    Eg, Ed = np.zeros_like(x), np.zeros_like(x)
    for t in range(steps):
        g = m.stochastic_grad(x)                      # gradient of the NEGATIVE bound on the next minibatch
        Eg = rho * Eg + (1 - rho) * g * g
        d = -np.sqrt(Ed + eps) / np.sqrt(Eg + eps) * g
        Ed = rho * Ed + (1 - rho) * d * d
        x = x + d
        if (t + 1) % 100 == 0:
            print("  step %4d  minibatch bound (scaled to all data) %.2f" % (t + 1, m.log_likelihood()))
    m.optimizer_array = x


def main():
    X, Y = data(4000)
    Xt, Yt = data(1000, seed=1)
    g = np.linspace(-1.75, 1.75, 6)
    Z = np.array([[a, b] for a in g for b in g])       # 36 inducing points on a grid
    kern = gpy_amd.RBF(2, variance=1.0, lengthscale=0.6)

    m = gpy_amd.SVGP(X, Y, Z, kern, gpy_amd.Bernoulli())
    print("full batch: bound %.2f, test accuracy %.3f" % (m.log_likelihood(), accuracy(m, Xt, Yt)))
    m.optimize(max_iters=60)
    print("after 60 L-BFGS-B iterations: bound %.2f, test accuracy %.3f" % (m.log_likelihood(), accuracy(m, Xt, Yt)))

    ms = gpy_amd.SVGP(X, Y, Z, gpy_amd.RBF(2, variance=1.0, lengthscale=0.6), gpy_amd.Bernoulli(), batchsize=250, seed=0)
    print("minibatches of 250 (batch_scale %.0f):" % (X.shape[0] / 250.0))
    adadelta(ms, 300)
    ms.set_data(X, Y)
    ms.optimizer_array = ms.optimizer_array              # one evaluation on all data
    print("after 300 Adadelta steps: bound on all data %.2f, test accuracy %.3f" % (ms.log_likelihood(), accuracy(ms, Xt, Yt)))


if __name__ == "__main__":
    main()
