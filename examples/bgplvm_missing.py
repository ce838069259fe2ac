"""Bayesian GPLVM with missing data on the MI355X: fit data with about 30 % of the entries removed, predict the removed entries
at the learned q(X) and print their RMSE next to column-mean imputation.

    python examples/bgplvm_missing.py        (needs the GPU)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpy_amd as GPy  # noqa: E402


def main(N=200, Q=2, Dy=8, M=25, seed=0):
    r = np.random.default_rng(seed)
    latent = r.uniform(-2, 2, (N, Q))
    A, ph = r.standard_normal((Q, Dy)), r.uniform(0, 2 * np.pi, Dy)
    Yfull = np.sin(latent.dot(A) + ph) + 0.05 * r.standard_normal((N, Dy))
    # four patterns of missing rows shared by the columns (about 30 % of all entries), as modalities absent for some rows
    Y = Yfull.copy()
    for k in range(1, 4):
        Y[np.ix_(r.uniform(size=N) < 0.4, np.arange(Dy) % 4 == k)] = np.nan
    gone = np.isnan(Y)
    col_mean = np.nanmean(Y, 0)
    # the latent points start from a PCA of the mean-imputed data (the model itself needs X when Y holds NaNs)
    Yi = np.where(gone, col_mean, Y) - col_mean
    X0 = np.linalg.svd(Yi, full_matrices=False)[0][:, :Q] * np.sqrt(N)
    np.random.seed(seed)
    m = GPy.models.BayesianGPLVMMiniBatch(Y, Q, X=X0, num_inducing=M, missing_data=True)
    m.optimize(max_iters=300)
    mu, _ = m.predict_noiseless(m.X)
    rmse = lambda a: float(np.sqrt(np.mean((a[gone] - Yfull[gone]) ** 2)))
    print("entries removed: %.1f %%   bound %.2f" % (100 * gone.mean(), m.log_likelihood()))
    print("RMSE of the removed entries: model %.4f   column means %.4f" % (rmse(mu), rmse(np.broadcast_to(col_mean, Y.shape))))


if __name__ == "__main__":
    main()
