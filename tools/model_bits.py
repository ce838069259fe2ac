"""Bit-for-bit record of what the model classes compute through the host layer (inference classes, posteriors, lazy views), for
comparing two versions of the PYTHON code over the same built library (MI355GP_LIB chooses it): the host hands the same bytes
to the same entry points, so any differing array is a defect of the host layer.

    python tools/model_bits.py --out FILE.npz    one seeded `parameters_changed` and one `predict` per model at N = 129, M = 33,
                                                 D = 3 (one row past a 128 tile, one column past a 32 chunk):
        gpr                     GPRegression, two output columns
        sgpr_scalar / _het / _xvar   SparseGPRegression with one noise variance; SparseGP with per-point noise;
                                SparseGPRegression with X_variance (uncertain inputs)
        fitc, pep               SparseGP with FITC() and PEP(0.5)
        svgp_gauss / _bern      the SVGP model, Gaussian and Bernoulli, batchsize 64: one minibatch step (`stochastic_grad`)
        bgplvm                  BayesianGPLVM, prediction at certain and at uncertain new points
        class_laplace / _ep     GPClassification with Laplace() and EP()
      -- per model: log-likelihood, the flat gradient, predictions, and every member of `grad_dict` and of the posterior
         (woodbury_vector, woodbury_inv, woodbury_chol, K, K_chol) materialised, the lazy ones included
    python tools/model_bits.py --compare A B     name every array whose bytes differ; exit status 1 if any does

The dumps are device results: compare two of the same machine, keep none as a fixture.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]
N, M, D, NS = 129, 33, 3, 17


def dump(path):
    import gpy_amd as G
    np.random.seed(129)                       # EP draws the order of its sweeps from NumPy's global generator
    rng = np.random.default_rng(129)
    X = rng.uniform(0.0, 1.0, (N, D))
    Y2 = np.sin(2.0 * np.pi * X @ rng.uniform(1.0, 3.0, (D, 2))) + 0.2 * rng.standard_normal((N, 2))
    Y1 = Y2[:, :1].copy()
    Yc = (Y1 > 0.0).astype(np.float64)
    Z = X[rng.permutation(N)[:M]] + 0.01 * rng.standard_normal((M, D))
    S = rng.uniform(0.001, 0.01, (N, D))
    Xs, Ss = rng.uniform(0.0, 1.0, (NS, D)), rng.uniform(0.001, 0.01, (NS, D))
    index = lambda n: {"output_index": np.arange(n)[:, None]}
    out = {}

    def kernel(white=True):
        k = G.RBF(D, variance=1.3, lengthscale=[0.3, 0.4, 0.5], ARD=True)
        return k + G.White(D, variance=0.05) if white else k

    def put(name, value):
        if isinstance(value, dict):
            for k in sorted(value):
                put(name + "/" + k, value[k])
        elif isinstance(value, (tuple, list)):
            for i, v in enumerate(value):
                put("%s/%d" % (name, i), v)
        elif value is not None:
            out[name] = np.ascontiguousarray(np.asarray(value, dtype=np.float64))

    def record(name, m, predict_at, **predict_kw):
        """one seeded step of every parameter, then everything the evaluation left behind, then one prediction"""
        step = np.random.default_rng(len(name)).uniform(0.97, 1.03, m.param_array.size)
        m.param_array = m.param_array * step
        put(name + "/lml", m.log_likelihood())
        put(name + "/gradient", m.gradient)
        put(name + "/grad_dict", m.grad_dict)
        for member in ("woodbury_vector", "woodbury_inv", "woodbury_chol", "K", "K_chol"):
            put(name + "/posterior/" + member, getattr(m.posterior, member, None))
        for tag, Xnew in predict_at.items():
            put(name + "/predict/" + tag, m.predict(Xnew, **predict_kw))

    record("gpr", G.GPRegression(X, Y2, kernel(), noise_var=0.04), {"certain": Xs})
    record("sgpr_scalar", G.SparseGPRegression(X, Y2, kernel(), Z=Z, noise_var=0.04), {"certain": Xs})
    record("sgpr_het", G.SparseGP(X, Y1, Z, kernel(), G.HeteroscedasticGaussian(index(N), variance=0.04), Y_metadata=index(N)),
           {"certain": Xs}, Y_metadata=index(NS))
    record("sgpr_xvar", G.SparseGPRegression(X, Y2, kernel(), Z=Z, noise_var=0.04, X_variance=S), {"certain": Xs})
    record("fitc", G.SparseGP(X, Y1, Z, kernel(), G.Gaussian(variance=0.04), inference_method=G.FITC()), {"certain": Xs})
    record("pep", G.SparseGP(X, Y1, Z, kernel(), G.Gaussian(variance=0.04), inference_method=G.PEP(0.5)), {"certain": Xs})
    for name, Y, lik in (("svgp_gauss", Y1, G.Gaussian(variance=0.04)), ("svgp_bern", Yc, G.Bernoulli())):
        m = G.SVGP(X, Y, Z, kernel(), lik, batchsize=64, seed=3)
        put(name + "/stochastic_grad", m.stochastic_grad(m.optimizer_array * 1.01))
        record(name, m, {"certain": Xs})
    record("bgplvm", G.BayesianGPLVM(Y2, D, X=X, X_variance=S, Z=Z, kernel=kernel()),
           {"certain": Xs, "uncertain": G.NormalPosterior(Xs, Ss)})
    record("class_laplace", G.GPClassification(X, Yc, kernel(white=False), inference_method=G.Laplace()), {"certain": Xs})
    record("class_ep", G.GPClassification(X, Yc, kernel(white=False), inference_method=G.EP()), {"certain": Xs})
    np.savez(path, **out)
    print("model_bits: %d arrays, %d doubles -> %s (library %s, package %s)"
          % (len(out), sum(a.size for a in out.values()), path, G._lib.LIB_PATH, os.path.dirname(G.__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.compare:
        from sparse_bits import compare
        return compare(*a.compare)
    if not a.out:
        ap.error("--out FILE or --compare A B")
    dump(a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
