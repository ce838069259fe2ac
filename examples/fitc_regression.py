"""The classic sparse GP next to the variational one on the same 1-D data (seeded, nothing downloaded): a FITC fit (Snelson and
Ghahramani's fully independent training conditional, `inference_method=GPy.inference.latent_function_inference.FITC()`) and a
VarDTC fit of `GPy.core.SparseGP` with M = 10 inducing inputs from the same start.  The data are dense on the left, where the
function wiggles, and thin on the right, where it is smooth.  FITC's per-point variance sigma*_n = noise + Knn - Qnn lets it
explain what the inducing inputs miss as noise, so it is free to move them; VarDTC pays for the same gap in the trace term of its
bound.  Where each placed its inducing inputs is printed, with the noise variance and lengthscale each settled on.

    python examples/fitc_regression.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpy_amd as GPy  # noqa: E402


def main():
    rng = np.random.default_rng(0)
    X = np.sort(np.concatenate([rng.uniform(0.0, 1.0, 240), rng.uniform(1.0, 3.0, 60)]))[:, None]
    f = np.where(X < 1.0, np.sin(12.0 * X), np.sin(12.0) + 0.3 * (X - 1.0))
    Y = f + 0.1 * rng.standard_normal(X.shape)
    Z0 = np.linspace(0.0, 3.0, 10)[:, None]
    Xs = np.linspace(0.0, 3.0, 61)[:, None]
    fs = np.where(Xs < 1.0, np.sin(12.0 * Xs), np.sin(12.0) + 0.3 * (Xs - 1.0))
    lfi = GPy.inference.latent_function_inference
    for name, method in (("FITC  ", lfi.FITC()), ("VarDTC", lfi.VarDTC())):
        m = GPy.core.SparseGP(X, Y, Z0.copy(), GPy.kern.RBF(1, lengthscale=0.2), GPy.likelihoods.Gaussian(variance=0.1),
                              inference_method=method)
        start = m.log_likelihood()
        m.optimize(max_iters=200)
        mu, _ = m.predict_noiseless(Xs)
        print("%s objective % .2f -> % .2f  noise variance %.4f (true 0.0100)  lengthscale %.3f  rms(mean - f) %.3f"
              % (name, start, m.log_likelihood(), float(np.ravel(m.likelihood.variance.values)[0]),
                 float(np.ravel(m.kern.lengthscale.values)[0]), float(np.sqrt(np.mean((mu - fs) ** 2)))))
        print("%s inducing inputs: %s" % (name, " ".join("%.2f" % z for z in np.sort(m.Z.values[:, 0]))))


if __name__ == "__main__":
    main()
