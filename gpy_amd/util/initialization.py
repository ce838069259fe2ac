"""Initial latent points for the latent variable models (reference `GPy/util/initialization.py:12-59`)."""
import numpy as np

from .pca import PCA


def initialize_latent(init, input_dim, Y):
    """(X (N x input_dim), fracs (input_dim)): standard normal draws, with `init == 'PCA'` the leading
    min(input_dim, Dy) columns replaced by Y's principal components; every column is then centred and scaled to unit
    standard deviation.  fracs: each dimension's share of the variance, the largest scaled to one (the default ARD
    lengthscales of `BayesianGPLVM` are 1 / fracs)."""
    Y = np.asarray(Y, dtype=np.float64)
    Xr = np.random.normal(0, 1, (Y.shape[0], input_dim))
    if init == "PCA":
        p = PCA(Y)
        PC = p.project(Y, min(input_dim, Y.shape[1]))
        Xr[:PC.shape[0], :PC.shape[1]] = PC
        var = 0.1 * p.fracs[:input_dim]
    elif init == "random":
        var = Xr.var(0)
    else:
        raise ValueError("initialize_latent: init = %r is not supported; 'PCA' and 'random' are" % (init,))
    Xr -= Xr.mean(0)
    Xr /= Xr.std(0)
    return Xr, var / var.max()
