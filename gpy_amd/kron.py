"""Exact Gaussian GP regression with inputs on a full Cartesian grid, backed by libmi355gp.so -- drop-in for
`GPy.models.GPRegressionGrid`, `GPy.core.GpGrid`, `GPy.inference.latent_function_inference.GaussianGridInference` and
`GridPosterior` (reference `GPy/models/gp_grid_regression.py`, `core/gp_grid.py`, `inference/latent_function_inference/
gaussian_grid_inference.py`, `grid_posterior.py`; Gilboa, Saatci and Cunningham 2015).

The covariance of a product kernel over a grid G_1 x ... x G_D is K = K_1 (x) ... (x) K_D.  One evaluation builds the D matrices
K_d and their derivative factors on the host (`gpy_amd.kern.GridRBF`, NumPy on G_d x G_d), takes `numpy.linalg.eigh` of each, and
makes two device calls on a context of its own (`_lib.KronContext`, include/mi355gp_kron.h): `solve` leaves alpha resident and
returns y^T alpha and sum log(V + noise), `quadforms` returns, for each of the D + 2 parameters, alpha^T ((x)A_d) alpha and
sum_i ((x)gamma_d)_i / (V_i + noise).  Everything of size N is a chain of tensor mode products on the device; nothing N x N exists
anywhere, and the model never creates an exact (N x N) context.

Where this differs from the reference, by design:
  * the grid values of a column are its SORTED unique values.  The reference takes `list(set(X[:, d]))`, hash order: ascending for
    integer-valued coordinates (its own test), arbitrary for generic reals, where it computes a wrong marginal likelihood.
  * `numpy.linalg.eigh` instead of `np.linalg.eig` on the symmetric K_d; every judged quantity is invariant to the choice.
  * X is checked to be the full grid, row n the n-th grid point with the LAST column varying fastest (the order the reference's
    `kron_mvprod` assumes silently); anything else is refused with a message that says what was found.
  * prediction follows the reference in using the likelihood variance WITHOUT the 1e-8 that inference adds, but not in forming the
    dense M x N cross-covariance: mu_m = sum_i alpha_i prod_d k_d^m[i_d] and the variance reduction sum_i prod_d (Q_d^T k_d^m)[i_d]^2
    / (V_i + noise) are contracted on the device from the D blocks M x G_d.

Accepted: one `RBF` over all D columns, `ARD=True`, or one lengthscale (for D > 1 the reference raises an IndexError there; here the
one lengthscale serves every dimension and its gradient is the sum of the D per-dimension gradients).  Refused by name, before any
device work: any other kernel or kernel expression, `inv_l=True`, `active_dims` that are not all columns, several output columns, a
likelihood other than `Gaussian`, a mean function, `full_cov=True`, `predictive_gradients`, `posterior_samples(_f)`,
`posterior_covariance_between_points`, and an X that is not a full grid in the stated order."""
import numpy as np

from . import _lib
from .inference import LatentFunctionInference
from .kern import RBF
from .lazy import ArrayIdentity
from .likelihoods import Gaussian
from .models import GP
from .variational import refuse_spike_and_slab

log_2_pi = np.log(2 * np.pi)


def grid_values(X):
    """The grid of X (N x D): the D arrays of sorted unique column values, after checking that X is the full Cartesian grid of
    them with row n the n-th grid point, last column fastest.  ValueError says what was found otherwise."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError("grid regression: X must be N x D with N, D >= 1, got shape %r" % (X.shape,))
    if not np.isfinite(X).all():
        raise ValueError("grid regression: X has entries that are not finite")
    N, D = X.shape
    xg = [np.unique(X[:, d]) for d in range(D)]
    G = [int(g.size) for g in xg]
    total = 1
    for g in G:
        total *= g
    if total != N:
        raise ValueError("grid regression: X is not a full grid: its columns have %s distinct values, a full grid of them has %d "
                         "points, X has %d rows" % (" x ".join(str(g) for g in G), total, N))
    idx = np.arange(N)
    for d in range(D - 1, -1, -1):
        bad = np.nonzero(X[:, d] != xg[d][idx % G[d]])[0]
        if bad.size:
            n = int(bad[0])
            want, i = [], n
            for e in range(D - 1, -1, -1):
                want.insert(0, xg[e][i % G[e]])
                i //= G[e]
            raise ValueError("grid regression: X is not the grid in row-major order with the last column varying fastest: row %d is "
                             "(%s), the grid expects (%s)" % (n, ", ".join("%g" % v for v in X[n]), ", ".join("%g" % v for v in want)))
        idx = idx // G[d]
    return xg


def check_kernel(kern, D):
    """the kernels grid regression takes (module docstring); returns the D lengthscales"""
    if not isinstance(kern, RBF):
        raise NotImplementedError("grid regression takes one RBF kernel over all input columns, not %s: other kernels and kernel "
                                  "expressions are not implemented on the MI355X grid path" % type(kern).__name__)
    if kern.use_invLengthscale:
        raise NotImplementedError("grid regression with RBF(inv_l=True) is not implemented on the MI355X grid path")
    if kern.input_dim != D or not np.array_equal(kern.active_dims, np.arange(D)):
        raise NotImplementedError("grid regression needs a kernel over all %d input columns, this one has active_dims %s"
                                  % (D, kern.active_dims.tolist()))
    ls = np.asarray(kern.lengthscale.values, dtype=np.float64).ravel()
    return ls.copy() if ls.size == D else np.full(D, ls[0])


def check_targets(Y):
    Y = np.asarray(Y, dtype=np.float64)
    if Y.ndim != 2 or Y.shape[1] != 1:
        raise NotImplementedError("grid regression takes one output column, Y has shape %r: several outputs are not implemented "
                                  "on the MI355X grid path" % (np.shape(Y),))
    return Y


def check_likelihood(likelihood):
    if type(likelihood) is not Gaussian:
        raise NotImplementedError("grid regression takes the Gaussian likelihood, not %s" % type(likelihood).__name__)
    return float(np.ravel(likelihood.variance.values)[0])


class _GridState(object):
    """One context and what it holds: the grid of the X last validated and the Y last uploaded, both kept by identity."""

    def __init__(self, device, context=None):
        self.device = device
        self.ctx = (context or _lib.KronContext)(device)
        self._idX = self._idY = None
        self.xg = None
        self.call_token = 0

    def ensure_data(self, X, Y):
        if self._idX is None or not self._idX.matches(X):
            self.xg = grid_values(X)
            self._idX, self._idY = ArrayIdentity(X), None
        if self._idY is None or not self._idY.matches(Y):
            if np.shape(Y)[0] != np.shape(X)[0]:
                raise ValueError("grid regression: X has %d rows and Y %d" % (np.shape(X)[0], np.shape(Y)[0]))
            self.ctx.set_data([g.size for g in self.xg], np.ravel(Y))
            self._idY = ArrayIdentity(Y)


class GridPosterior(object):
    """(reference `grid_posterior.py:8-61`): `alpha` (N x 1) and `V_kron` (N x 1) are materialised on first use -- alpha is
    fetched from the device, V_kron is the Kronecker product of the per-dimension eigenvalues -- `Qs` and `QTs` are the D
    eigenvector matrices.  Either of `alpha_kron` and `V_kron` may be given as a callable that returns the array."""

    def __init__(self, alpha_kron=None, QTs=None, Qs=None, V_kron=None):
        if alpha_kron is None or QTs is None or Qs is None or V_kron is None:
            raise ValueError("insufficient information for predictions")
        self._alpha_kron, self._qTs, self._qs, self._v_kron = alpha_kron, QTs, Qs, V_kron

    @property
    def alpha(self):
        if callable(self._alpha_kron):
            self._alpha_kron = self._alpha_kron()
        return self._alpha_kron

    @property
    def V_kron(self):
        if callable(self._v_kron):
            self._v_kron = self._v_kron()
        return self._v_kron

    @property
    def QTs(self):
        return self._qTs

    @property
    def Qs(self):
        return self._qs

    def __getstate__(self):                      # the device handle never travels: what is lazy is materialised
        self.alpha, self.V_kron
        d = dict(self.__dict__)
        d["_state"] = None
        return d


class GaussianGridInference(LatentFunctionInference):
    """Exact inference for a Gaussian likelihood and inputs on a grid (reference `gaussian_grid_inference.py:24-114`)."""

    def __init__(self, device=0, context=None):
        """`context`: the class of the device context (tests put a recording one here)"""
        self.device, self._context = device, context
        self._state = None

    def to_dict(self):
        return {"class": "GPy.inference.latent_function_inference.gaussian_grid_inference.GaussianGridInference"}

    def kron_mvprod(self, A, b):
        """(x)A_d b on the HOST as the reference does it (`:35-48`), for callers that use it directly; the model does not"""
        x = np.asarray(b, dtype=np.float64).reshape(-1)
        N = x.size
        for d in range(len(A) - 1, -1, -1):
            G = len(A[d])
            x = np.dot(np.asarray(A[d]), x.reshape(N // G, G).T).reshape(-1)
        return x.reshape(-1, 1)

    def inference(self, kern, X, likelihood, Y, Y_metadata=None):
        refuse_spike_and_slab(X, "GaussianGridInference")
        X = np.asarray(X)
        if X.ndim != 2:
            raise ValueError("grid regression: X must be N x D, got shape %r" % (X.shape,))
        N, D = X.shape
        ls = check_kernel(kern, D)
        check_targets(Y)
        noise = check_likelihood(likelihood) + 1e-8
        if self._state is None:
            self._state = _GridState(self.device, self._context)
        st = self._state
        st.ensure_data(X, Y)
        st.call_token += 1
        token, xg, ctx = st.call_token, st.xg, st.ctx

        oneD = kern.get_one_dimensional_kernel(D)
        Qs, QTs, lams = [], [], []
        for d in range(D):
            oneD.lengthscale = ls[d]
            lam, Q = np.linalg.eigh(oneD.K(xg[d][:, None]))
            Qs.append(Q)
            QTs.append(Q.T)
            lams.append(lam)
        yTa, sumlog = ctx.solve(Qs, lams, noise)
        log_likelihood = -0.5 * (yTa + sumlog + N * log_2_pi)

        factors, gammas = [], []
        for t in range(D + 2):
            A, gam = [], []
            for d in range(D):
                oneD.lengthscale = ls[d]
                if t < D:
                    Ad = oneD.dKd_dLen(xg[d][:, None], (t == d), lengthscale=ls[t])
                elif t == D:
                    Ad = oneD.dKd_dVar(xg[d][:, None])
                else:
                    Ad = np.identity(xg[d].size)
                A.append(Ad)
                gam.append(np.einsum("ij,ij->j", Qs[d], np.dot(Ad.T, Qs[d])))      # diag(Q^T A^T Q)
            factors.append(A)
            gammas.append(gam)
        q, s = ctx.quadforms(factors, gammas)
        derivs = 0.5 * q - 0.5 * s
        dL_dLen = derivs[:D].copy() if kern.lengthscale.size == D else np.array([derivs[:D].sum()])

        def V_kron():
            V = np.ones(1)
            for lam in lams:
                V = np.kron(V, lam)
            return V.reshape(-1, 1)

        def alpha():
            if st.call_token != token:
                raise RuntimeError("alpha of this GridPosterior was overwritten on the device by a later inference call")
            return st.ctx.fetch_alpha().reshape(-1, 1)
        post = GridPosterior(alpha_kron=alpha, QTs=QTs, Qs=Qs, V_kron=V_kron)
        post._state, post._token, post._xg, post._ls = st, token, xg, ls
        return post, log_likelihood, {"dL_dLen": dL_dLen, "dL_dVar": float(derivs[D]), "dL_dthetaL": float(derivs[D + 1])}


class GpGrid(GP):
    """A GP model for grid inputs (reference `core/gp_grid.py:30-116`); the inference method is always `GaussianGridInference`."""

    def __init__(self, X, Y, kernel, likelihood, inference_method=None, name="gp grid", Y_metadata=None, normalizer=False,
                 device=0, mean_function=None):
        if mean_function is not None:
            raise NotImplementedError("grid regression with a mean function is not implemented on the MI355X grid path")
        X = np.asarray(X)
        if X.ndim != 2:
            raise ValueError("grid regression: X must be N x D, got shape %r" % (X.shape,))
        check_kernel(kernel, X.shape[1])
        check_targets(Y)
        check_likelihood(likelihood)
        grid_values(X)
        if not isinstance(inference_method, GaussianGridInference):
            inference_method = GaussianGridInference(device=device)          # (reference `gp_grid.py:47`: whatever was passed)
        super(GpGrid, self).__init__(X, Y, kernel, likelihood, inference_method=inference_method, name=name,
                                     Y_metadata=Y_metadata, device=device,
                                     normalizer=bool(normalizer) if normalizer in (None, True, False) else normalizer)

    def parameters_changed(self):
        """(reference `gp_grid.py:61-63`)"""
        self.posterior, self._log_marginal_likelihood, self.grad_dict = self.inference_method.inference(
            self.kern, self.X, self.likelihood, self.Y_normalized, self.Y_metadata)
        self.likelihood.update_gradients(self.grad_dict["dL_dthetaL"])
        self.kern.update_gradients_direct(self.grad_dict["dL_dVar"], self.grad_dict["dL_dLen"])

    def _raw_predict(self, Xnew, full_cov=False, kern=None):
        """mean and variance of the latent function at Xnew (reference `gp_grid.py:87-116`, its noise convention: the likelihood
        variance without the 1e-8 of inference), contracted on the device from the D blocks K_d(Xnew[:, d], grid_d)."""
        if full_cov:
            raise NotImplementedError("full_cov=True is not implemented for grid regression on the MI355X grid path")
        if kern is not None and kern is not self.kern:
            raise NotImplementedError("prediction with another kernel is not implemented for grid regression")
        post = self.posterior
        st = post._state
        if st is None or st.call_token != post._token:
            raise RuntimeError("the posterior of this model is not the device's latest: call parameters_changed() first")
        Xnew = np.asarray(Xnew, dtype=np.float64)
        D = self.X.shape[1]
        if Xnew.ndim != 2 or Xnew.shape[1] != D or Xnew.shape[0] < 1:
            raise ValueError("grid regression: Xnew must be M x %d with M >= 1, got shape %r" % (D, Xnew.shape))
        oneD = self.kern.get_one_dimensional_kernel(D)
        kx, bx = [], []
        for d in range(D):
            oneD.lengthscale = post._ls[d]
            k = oneD.K(Xnew[:, d:d + 1], post._xg[d][:, None])
            kx.append(k)
            bx.append(np.dot(k, post.Qs[d]))
        mu, red = st.ctx.predict(kx, bx, float(np.ravel(self.likelihood.variance.values)[0]))
        var = float(np.ravel(self.kern.variance.values)[0]) - red
        return mu.reshape(-1, 1), var.reshape(-1, 1)

    def _refuse(self, what):
        raise NotImplementedError("%s is not implemented for grid regression on the MI355X grid path" % what)

    def predictive_gradients(self, Xnew, kern=None):
        self._refuse("predictive_gradients")

    def posterior_samples_f(self, X, size=10, **predict_kwargs):
        self._refuse("posterior_samples_f")

    def posterior_samples(self, X, size=10, Y_metadata=None, likelihood=None, **predict_kwargs):
        self._refuse("posterior_samples")

    def posterior_covariance_between_points(self, X1, X2, Y_metadata=None, likelihood=None, include_likelihood=True):
        self._refuse("posterior_covariance_between_points")

    def to_dict(self):
        return {"class": "GPy.core.GpGrid", "name": self.name, "kernel": self.kern.to_dict(), "likelihood": self.likelihood.to_dict(),
                "inference_method": self.inference_method.to_dict()}


class GPRegressionGrid(GpGrid):
    """Gaussian process regression for grid inputs using Kronecker products (reference `models/gp_grid_regression.py:10-35`).
    The default kernel is the reference's `RBF(1)`, which is only right for one input column: for D > 1 pass
    `RBF(D, ARD=True)` (the default then fails the kernel check by name, as it fails in the reference by an IndexError)."""

    def __init__(self, X, Y, kernel=None, Y_metadata=None, normalizer=None, device=0):
        if kernel is None:
            kernel = RBF(1, device=device)   # no other kernels implemented so far
        super(GPRegressionGrid, self).__init__(X, Y, kernel, Gaussian(), name="GP Grid regression", Y_metadata=Y_metadata,
                                               normalizer=normalizer, device=device)

    def to_dict(self):
        return dict(super(GPRegressionGrid, self).to_dict(), **{"class": "GPy.models.GPRegressionGrid"})
