"""Writes tests/golden/kgpr/*.npz: the reference's OWN `GPKroneckerGaussianRegression` (run in place through oracle.ref_loader, where
the reference tree exists) on three small problems -- the inputs, the kernel parameters, lml, the parameter gradients in link order
(kern1: variance, lengthscale; kern2: variance, lengthscale; noise) and mu, var at new points.  tests/test_kgpr_host.py holds the
float64 restatement tests/kgpr_ld.py against them.  Usage: python tools/make_golden_kgpr.py"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader  # noqa: E402

SHAPES = [(12, 9), (30, 5), (5, 30)]


def load_model(ns):
    core = sys.modules["GPy.core"]
    if not hasattr(core, "Model"):
        core.Model = importlib.import_module("GPy.core.model").Model
    sys.modules["GPy.likelihoods"].Gaussian = ns.Gaussian
    sys.modules["GPy"].likelihoods = sys.modules["GPy.likelihoods"]
    ref_loader._stub("GPy.models", os.path.join(ref_loader._REF, "models"))
    return importlib.import_module("GPy.models.gp_kronecker_gaussian_regression").GPKroneckerGaussianRegression


def main():
    ns = ref_loader.load()
    Model = load_model(ns)
    out = os.path.join(ROOT, "tests", "golden", "kgpr")
    os.makedirs(out, exist_ok=True)
    for n, (N1, N2) in enumerate(SHAPES):
        rng = np.random.RandomState(100 + n)
        X1, X2 = np.sort(rng.uniform(0, 3, (N1, 1)), 0), np.sort(rng.uniform(0, 2, (N2, 1)), 0)
        Y = np.sin(2 * X1) * np.cos(3 * X2.T) + 0.1 * rng.randn(N1, N2)
        theta = dict(var1=1.3, ls1=0.7, var2=0.8, ls2=0.5, noise=0.15)
        k1 = ns.RBF(1, variance=theta["var1"], lengthscale=theta["ls1"])
        k2 = ns.Matern32(1, variance=theta["var2"], lengthscale=theta["ls2"])
        # the paramz stand-in replaces the likelihood's Param by whatever `likelihood.variance = noise_var` is given: give it a Param
        m = Model(X1, X2, Y, k1, k2, noise_var=sys.modules["GPy.core"].Param("variance", theta["noise"]))
        m.parameters_changed()
        X1n, X2n = rng.uniform(0, 3, (4, 1)), rng.uniform(0, 2, (3, 1))
        mu, var = m.predict(X1n, X2n)
        grad = np.concatenate([np.ravel(k1.variance.gradient), np.ravel(k1.lengthscale.gradient), np.ravel(k2.variance.gradient),
                               np.ravel(k2.lengthscale.gradient), np.ravel(m.likelihood.variance.gradient)]).astype(np.float64)
        np.savez(os.path.join(out, "kgpr_%dx%d.npz" % (N1, N2)), X1=X1, X2=X2, Y=Y, X1new=X1n, X2new=X2n, lml=float(m.log_likelihood()),
                 grad=grad, mu=np.asarray(mu, dtype=np.float64), var=np.asarray(var, dtype=np.float64), **theta)
        print("kgpr_%dx%d: lml %.12f" % (N1, N2, float(m.log_likelihood())))


if __name__ == "__main__":
    main()
