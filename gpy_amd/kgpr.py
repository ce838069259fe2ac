"""Kronecker GP regression with two arbitrary kernels, backed by libmi355gp.so -- drop-in for
`GPy.models.GPKroneckerGaussianRegression` (reference `GPy/models/gp_kronecker_gaussian_regression.py`; Stegle et al. 2011).

The data are a matrix Y (N1 x N2), the covariance of vec(Y) = Y.flatten(order='F') is K2(X2) (x) K1(X1) + sigma^2 I.  One evaluation
builds K1 = kern1.K(X1) and K2 = kern2.K(X2) on the device as every model here does, hands the two matrices to a context of its own
(`_lib.KgprContext`, include/mi355gp_kgpr.h) and receives the log marginal likelihood, dL_dsigma2, dL_dK1 and dL_dK2; the kernels
turn those into their parameters' gradients with `update_gradients_full`, so every kernel and every `Add` / `Prod` of kernels
serves.  Both eigendecompositions, the rotations, the spectral pass and the weighted rank-k products behind dL_dK run on the device;
nothing of size N1 N2 x N1 N2 exists anywhere.  This is another model than `GPRegressionGrid` (kron.py), which takes one RBF on a
Cartesian grid.

`Wi`, `Ytilde` (N1 N2, order 'F', as the reference holds them), `U1` and `U2` are lazy views of what stays resident on the device.

Refused by name, before any device work: shapes that do not fit together (the reference's three asserts), a Y with entries that
are not finite, a noise variance that is not positive, a kernel without `update_gradients_full`, more than
`_lib.EIGH_MAX_N` points on a side."""
import numpy as np

from . import _lib
from .lazy import LazyArray, freeze
from .likelihoods import Gaussian
from .models import GradientCheck, ObjectiveOptimizer
from .param import Parameterized


class KgprView(LazyArray):
    """A result of a `KgprContext`'s last evaluation (`which` = `KgprContext.FETCH_*`); `flat`: the N1 x N2 matrix as the vector
    of its columns, the reference's `flatten(order='F')`."""
    stale = ("this device-resident result was overwritten by a later evaluation of the model; materialise it (np.asarray) before "
             "the parameters change")

    def __init__(self, ctx, which, shape, flat=False):
        self._ctx, self._which, self._token, self._flat = ctx, which, ctx.call_token, flat
        self.shape = (shape[0] * shape[1],) if flat else tuple(shape)
        self.ndim = len(self.shape)

    size = property(lambda self: int(np.prod(self.shape)))

    def _current(self):
        return self._ctx.call_token == self._token

    def _materialise(self):
        a = self._ctx.fetch(self._which)
        return np.ascontiguousarray(a.T).ravel() if self._flat else a


def check_inputs(X1, X2, Y, kern1, kern2):
    """the reference's three asserts and what the device path adds, each by name"""
    X1, X2, Y = np.asarray(X1, dtype=np.float64), np.asarray(X2, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    if X1.ndim != 2 or X2.ndim != 2 or Y.ndim != 2:
        raise ValueError("Kronecker regression: X1, X2 and Y must be two-dimensional, got shapes %r, %r, %r" % (X1.shape, X2.shape, Y.shape))
    for k, X, which in ((kern1, X1, 1), (kern2, X2, 2)):
        if not callable(getattr(k, "update_gradients_full", None)):
            raise NotImplementedError("Kronecker regression: kern%d (%s) has no update_gradients_full, which is how the model hands it "
                                      "dL_dK%d" % (which, type(k).__name__, which))
        if k.input_dim != X.shape[1]:
            raise ValueError("Kronecker regression: kern%d.input_dim is %d, X%d has %d columns" % (which, k.input_dim, which, X.shape[1]))
    if Y.shape != (X1.shape[0], X2.shape[0]):
        raise ValueError("Kronecker regression: Y must be N1 x N2 = %d x %d (the rows of X1 by the rows of X2), got shape %r"
                         % (X1.shape[0], X2.shape[0], Y.shape))
    if max(Y.shape) > _lib.EIGH_MAX_N or min(Y.shape) < 1:
        raise ValueError("Kronecker regression: Y is %d x %d, each side takes 1 to the limit of %d points" % (Y.shape + (_lib.EIGH_MAX_N,)))
    if not np.isfinite(Y).all():
        raise ValueError("Kronecker regression: Y has entries that are not finite")


def check_noise(variance):
    v = float(np.ravel(variance)[0])
    if not (v > 0.0 and np.isfinite(v)):
        raise ValueError("Kronecker regression: the noise variance must be positive, got %r" % v)
    return v


class GPKroneckerGaussianRegression(GradientCheck, ObjectiveOptimizer, Parameterized):
    """(reference `gp_kronecker_gaussian_regression.py:9-117`, same arguments): parameters in the order kern1, kern2, Gaussian noise."""

    def __init__(self, X1, X2, Y, kern1, kern2, noise_var=1., name="KGPR", device=0):
        super(GPKroneckerGaussianRegression, self).__init__(name)
        check_inputs(X1, X2, Y, kern1, kern2)
        check_noise(noise_var)
        self.X1, self.X2, self.Y = freeze(X1), freeze(X2), freeze(Y)
        self.kern1, self.kern2 = kern1, kern2
        self.link_parameter(self.kern1)
        self.link_parameter(self.kern2)
        self.likelihood = Gaussian(variance=noise_var)
        self.link_parameter(self.likelihood)
        self.num_data1, self.input_dim1 = self.X1.shape
        self.num_data2, self.input_dim2 = self.X2.shape
        self.device = device
        self._ctx = _lib.KgprContext(device)
        self._ctx.set_data(self.Y)
        self._log_marginal_likelihood = None
        self.sweeps = None
        self.parameters_changed()

    def log_likelihood(self):
        return self._log_marginal_likelihood

    def parameters_changed(self):
        """(reference `gp_kronecker_gaussian_regression.py:53-94`)"""
        noise = check_noise(self.likelihood.variance.values)
        K1, K2 = self.kern1.K(self.X1), self.kern2.K(self.X2)
        lml, dL_dsigma2, dL_dK1, dL_dK2, self.sweeps = self._ctx.inference(K1, K2, noise)
        self._log_marginal_likelihood = lml
        self.kern1.update_gradients_full(dL_dK1, self.X1)
        self.kern2.update_gradients_full(dL_dK2, self.X2)
        self.likelihood.variance.gradient = dL_dsigma2
        self.grad_dict = {"dL_dK1": dL_dK1, "dL_dK2": dL_dK2, "dL_dthetaL": dL_dsigma2}
        c, shape = self._ctx, (self.num_data1, self.num_data2)
        self.Wi, self.Ytilde = KgprView(c, c.FETCH_WI, shape, flat=True), KgprView(c, c.FETCH_YTILDE, shape, flat=True)
        self.U1 = KgprView(c, c.FETCH_U1, (self.num_data1, self.num_data1))
        self.U2 = KgprView(c, c.FETCH_U2, (self.num_data2, self.num_data2))

    def predict(self, X1new, X2new):
        """Mean and variance (diagonal only, as the reference) at all combinations of X1new x X2new, flat index i + M1 j:
        `(mu[:, None], var[:, None])` (reference `gp_kronecker_gaussian_regression.py:96-117`).  kron(B, A) is never formed."""
        X1new, X2new = np.asarray(X1new, dtype=np.float64), np.asarray(X2new, dtype=np.float64)
        if X1new.ndim != 2 or X1new.shape[1] != self.input_dim1 or X2new.ndim != 2 or X2new.shape[1] != self.input_dim2:
            raise ValueError("Kronecker regression: X1new must be M1 x %d and X2new M2 x %d, got shapes %r and %r"
                             % (self.input_dim1, self.input_dim2, X1new.shape, X2new.shape))
        mu, var = self._ctx.predict(self.kern1.K(X1new, self.X1), self.kern2.K(X2new, self.X2), self.kern1.Kdiag(X1new),
                                    self.kern2.Kdiag(X2new))
        return mu[:, None], var[:, None]
