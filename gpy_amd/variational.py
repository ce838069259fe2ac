"""Gaussian input distributions for the psi-statistics (reference `GPy/core/parameterization/variational.py`).

`NormalPosterior(means, variances)` holds q(x_n) = N(mean_n, diag variance_n): what the kernels' `psi0 / psi1 / psi2` and
their gradient methods take in place of X.  It is a `Parameterized` with the two `Param`s `mean` (unconstrained) and
`variance` (positive), linked in that order (reference `variational.py:98-106`): a model that links it (`BayesianGPLVM`)
optimises them, a model that only keeps it (`SparseGP` with `X_variance`) treats them as data.
`NormalPrior` is the standard normal prior p(x_n) = N(0, I) with the KL term KL(q || p) and its gradients (`:29-37`)."""
import numpy as np

from .param import Param, Parameterized


class NormalPosterior(Parameterized):
    def __init__(self, means, variances, name="latent space"):
        super(NormalPosterior, self).__init__(name)
        mean = np.array(means, dtype=np.float64, ndmin=2)
        variance = np.array(variances, dtype=np.float64, ndmin=2)
        if mean.shape != variance.shape:
            raise ValueError("means %r and variances %r must have the same shape" % (mean.shape, variance.shape))
        if not (np.all(np.isfinite(mean)) and np.all(np.isfinite(variance)) and np.all(variance > 0.0)):
            raise ValueError("NormalPosterior: means must be finite and variances positive and finite")
        self.mean = Param("mean", mean, positive=False)
        self.variance = Param("variance", variance, positive=True)
        self.link_parameters(self.mean, self.variance)

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
        m, v = self.mean.values[s], self.variance.values[s]
        if m.ndim != 2:
            raise IndexError("NormalPosterior: an index must keep both axes (slices or index arrays)")
        return NormalPosterior(m, v, name=self.name)

    def copy(self):
        return NormalPosterior(self.mean.values.copy(), self.variance.values.copy(), name=self.name)

    def set_gradients(self, grad):
        """(dL/dmean, dL/dvariance) (reference `variational.py:108-109`)"""
        self.mean.gradient, self.variance.gradient = grad

    def KL(self, other):
        """KL(self || other) for another `NormalPosterior` of the same shape (reference `variational.py:165-173`)"""
        m0, v0 = self.mean.values, self.variance.values
        m1, v1 = other.mean.values, other.variance.values
        return 0.5 * (np.sum(v0 / v1) + ((m1 - m0) ** 2 / v1).sum() - self.num_data * self.input_dim
                      + np.sum(np.log(v1)) - np.sum(np.log(v0)))


class NormalPrior(Parameterized):
    """p(x_n) = N(0, I) (reference `variational.py:25-37`); O(N Q) NumPy on the host."""

    def __init__(self, name="normal_prior"):
        super(NormalPrior, self).__init__(name)

    def KL_divergence(self, variational_posterior):
        mean, S = variational_posterior.mean.values, variational_posterior.variance.values
        return 0.5 * ((mean * mean).sum() + (S - np.log(S)).sum() - mean.size)

    def update_gradients_KL(self, variational_posterior):
        """subtracts the KL term's gradients from the posterior's mean / variance gradients, in place"""
        q = variational_posterior
        q.mean.gradient = q.mean.gradient - q.mean.values
        q.variance.gradient = q.variance.gradient - (1.0 - 1.0 / q.variance.values) * 0.5
