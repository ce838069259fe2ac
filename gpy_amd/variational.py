"""Gaussian input distributions for the psi-statistics (reference `GPy/core/parameterization/variational.py`).

`NormalPosterior(means, variances)` holds q(x_n) = N(mean_n, diag variance_n): what the kernels' `psi0 / psi1 / psi2` and
their gradient methods take in place of X.  It is a `Parameterized` with the two `Param`s `mean` (unconstrained) and
`variance` (positive), linked in that order (reference `variational.py:98-106`): a model that links it (`BayesianGPLVM`)
optimises them, a model that only keeps it (`SparseGP` with `X_variance`) treats them as data.
`NormalPrior` is the standard normal prior p(x_n) = N(0, I) with the KL term KL(q || p) and its gradients (`:29-37`).

`SpikeAndSlabPosterior(means, variances, binary_prob)` holds q(x_nq) = gamma_nq N(mean_nq, variance_nq) + (1 - gamma_nq) delta_0
(reference `variational.py:175-230`), the posterior of `SSGPLVM`: a sibling of `NormalPosterior`, not a subclass, so that
nothing written for Gaussian inputs takes it by accident.  `SpikeAndSlabPrior(pi, variance)` is p(x_nq) = pi_q N(0, variance) +
(1 - pi_q) delta_0 with its KL term and gradients (`:39-96`); pi is fixed."""
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


class SpikeAndSlabPosterior(Parameterized):
    def __init__(self, means, variances, binary_prob, name="latent space"):
        super(SpikeAndSlabPosterior, self).__init__(name)
        mean = np.array(means, dtype=np.float64, ndmin=2)
        variance = np.array(variances, dtype=np.float64, ndmin=2)
        gamma = np.array(binary_prob, dtype=np.float64, ndmin=2)
        if mean.shape != variance.shape or mean.shape != gamma.shape:
            raise ValueError("means %r, variances %r and binary_prob %r must have the same shape"
                             % (mean.shape, variance.shape, gamma.shape))
        if not (np.all(np.isfinite(mean)) and np.all(np.isfinite(variance)) and np.all(variance > 0.0)):
            raise ValueError("SpikeAndSlabPosterior: means must be finite and variances positive and finite")
        if not np.all((gamma > 0.0) & (gamma < 1.0)):
            raise ValueError("SpikeAndSlabPosterior: binary_prob must lie strictly inside (0, 1)")
        self.mean = Param("mean", mean, positive=False)
        self.variance = Param("variance", variance, positive=True)
        self.binary_prob = Param("binary_prob", gamma, positive=False)   # (0, 1): a model sees it through a logistic transform
        self.link_parameters(self.mean, self.variance, self.binary_prob)

    gamma = property(lambda self: self.binary_prob)
    shape = property(lambda self: self.mean.shape)
    ndim = 2
    num_data = property(lambda self: self.mean.shape[0])
    input_dim = property(lambda self: self.mean.shape[1])

    def has_uncertain_inputs(self):
        return True

    def __len__(self):
        return self.mean.shape[0]

    def __getitem__(self, s):
        """row / column slicing of the three arrays alike (reference `variational.py:208-230`); the result stays 2-D"""
        m, v, g = self.mean.values[s], self.variance.values[s], self.binary_prob.values[s]
        if m.ndim != 2:
            raise IndexError("SpikeAndSlabPosterior: an index must keep both axes (slices or index arrays)")
        return SpikeAndSlabPosterior(m, v, g, name=self.name)

    def copy(self):
        return SpikeAndSlabPosterior(self.mean.values.copy(), self.variance.values.copy(), self.binary_prob.values.copy(),
                                     name=self.name)

    def set_gradients(self, grad):
        """(dL/dmean, dL/dvariance, dL/dbinary_prob) (reference `variational.py:194-195`)"""
        self.mean.gradient, self.variance.gradient, self.binary_prob.gradient = grad


def refuse_spike_and_slab(X, who):
    """every consumer but `VarDTC` / `SSGPLVM` names the type it does not take"""
    if isinstance(X, SpikeAndSlabPosterior):
        raise NotImplementedError("%s: a SpikeAndSlabPosterior X is not implemented on the MI355X path; VarDTC (the inference of "
                                  "SSGPLVM) takes one" % who)


class SpikeAndSlabPrior(Parameterized):
    """p(x_nq) = pi_q N(0, variance) + (1 - pi_q) delta_0 (reference `variational.py:39-96` with learnPi = False and no group
    spike); pi: one probability or one per dimension, fixed (it is not a parameter here).  O(N Q) NumPy on the host."""

    def __init__(self, pi=0.5, variance=1.0, name="SpikeAndSlabPrior", learnPi=False, group_spike=False):
        super(SpikeAndSlabPrior, self).__init__(name)
        if learnPi or group_spike:
            raise NotImplementedError("SpikeAndSlabPrior: %s is not implemented on the MI355X path"
                                      % ("learnPi" if learnPi else "group_spike"))
        self.pi = np.atleast_1d(np.asarray(pi, dtype=np.float64))
        self.variance = float(variance)
        if self.pi.ndim != 1 or not np.all((self.pi > 0.0) & (self.pi < 1.0)) or not self.variance > 0.0:
            raise ValueError("SpikeAndSlabPrior: pi must be one probability or one per dimension, inside (0, 1); variance positive")

    def KL_divergence(self, variational_posterior):
        q = variational_posterior
        mu, S, g, pi, v = q.mean.values, q.variance.values, q.binary_prob.values, self.pi, self.variance
        kg = (g * np.log(g / pi)).sum() + ((1.0 - g) * np.log((1.0 - g) / (1.0 - pi))).sum()
        return kg + (g * (np.log(v) - 1.0 + mu * mu / v + S / v - np.log(S))).sum() / 2.0

    def update_gradients_KL(self, variational_posterior):
        """subtracts the KL term's gradients from the posterior's mean / variance / binary_prob gradients, in place"""
        q = variational_posterior
        mu, S, g, pi, v = q.mean.values, q.variance.values, q.binary_prob.values, self.pi, self.variance
        dg = np.log((1.0 - pi) / pi * g / (1.0 - g)) + ((mu * mu + S) / v - np.log(S) + np.log(v) - 1.0) / 2.0
        q.binary_prob.gradient = q.binary_prob.gradient - dg
        q.mean.gradient = q.mean.gradient - g * mu / v
        q.variance.gradient = q.variance.gradient - (1.0 / v - 1.0 / S) * g / 2.0
