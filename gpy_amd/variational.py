"""Gaussian input distributions for the psi-statistics (reference `GPy/core/parameterization/variational.py`).

`NormalPosterior(means, variances)` is a plain data holder for q(x_n) = N(mean_n, diag variance_n): what the kernels'
`psi0 / psi1 / psi2` and their gradient methods take in place of X.  It carries no KL term and no parameters."""
import numpy as np


class NormalPosterior(object):
    def __init__(self, means, variances, name="latent space"):
        self.mean = np.array(means, dtype=np.float64, ndmin=2)
        self.variance = np.array(variances, dtype=np.float64, ndmin=2)
        if self.mean.shape != self.variance.shape:
            raise ValueError("means %r and variances %r must have the same shape" % (self.mean.shape, self.variance.shape))
        if not (np.all(np.isfinite(self.mean)) and np.all(np.isfinite(self.variance)) and np.all(self.variance > 0.0)):
            raise ValueError("NormalPosterior: means must be finite and variances positive and finite")
        self.name = name

    shape = property(lambda self: self.mean.shape)
    ndim = 2
    num_data = property(lambda self: self.mean.shape[0])
    input_dim = property(lambda self: self.mean.shape[1])

    def has_uncertain_inputs(self):
        return True

    def __len__(self):
        return self.mean.shape[0]

    def __getitem__(self, s):
        """row / column slicing of means and variances alike (reference `variational.py:133-150`); the result stays 2-D"""
        m, v = self.mean[s], self.variance[s]
        if m.ndim != 2:
            raise IndexError("NormalPosterior: an index must keep both axes (slices or index arrays)")
        return NormalPosterior(m, v, name=self.name)

    def copy(self):
        return NormalPosterior(self.mean.copy(), self.variance.copy(), name=self.name)
