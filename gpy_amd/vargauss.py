"""`VarGauss` inference backed by libmi355gp.so -- drop-in for `GPy.inference.latent_function_inference.VarGauss` (reference
`GPy/inference/latent_function_inference/var_gauss.py:9-69`): the variational Gaussian approximation of Opper and Archambeau
(2009), q(f) = N(K alpha, (K^-1 + diag(beta^2))^-1), for one output column and any likelihood with `variational_expectations`.

One evaluation is two device calls inside the session of the exact context that `Laplace` and `EP` use (`laplace.begin_session`):
`mi355gp_vargauss_forward` factors A = I + diag(beta) K diag(beta) and returns m = K alpha, diag Sigma and the three scalars of
the KL term; the likelihood's variational expectations are O(N) host work on those vectors; `mi355gp_vargauss_backward` returns
both variational gradients and every kernel part's dL/dtheta.  K, A's factor and inverse, dL_dK and the posterior's woodbury_inv
never leave the device unless a caller materialises the lazy proxies.

Where this differs from the reference, by design: the kernel gradient is the derivative of the bound.  The reference forms the
dF_dv term of dL_dK as `np.dot(tmp*dF_dv, tmp.T)` (`:65`), which scales the ROWS of tmp = Ai beta_i / beta_j by dF_dv, where
d var_i / dK = tmp[:, i] tmp[:, i]^T asks for its COLUMNS: tmp diag(dF_dv) tmp^T.  The two agree only where dF_dv is the same at
every point (a Gaussian likelihood); elsewhere the reference's kernel gradients fail a finite-difference check (1-D toy problem,
default start: lengthscale gradient 2.66710 against 2.66551) and L-BFGS stalls on them.  `VarGauss(..., reference_gradient=True)`
gives the reference's form, for comparison with it; the variational gradients and the bound are the same either way.  Also: diag Sigma is Kdiag - colsumsq(L_A^-1 diag(beta) K), not the cancelling
beta^-2 - Ai_ii beta^-2; `grad_dict['dL_dK']` is SYMMETRISED, (dL_dK + dL_dK^T) / 2 -- the only part a
symmetric dK/dtheta sees; and the posterior is Posterior(woodbury_vector = alpha, woodbury_inv = diag(beta) Ai diag(beta)), which
equals the reference's K^-1 - K^-1 Sigma K^-1 without inverting K.

Not implemented, refused by name: a mean function, several output columns or latent functions, a device quadrature, a sparse or
grid variant."""
import numpy as np

from . import _lib
from .inference import LatentFunctionInference
from .laplace import begin_session, entry_checks
from .lazy import DeviceResult, LazyArray, kernel_signature
from .linalg import jitter_ladder
from .posterior import PosteriorExact
from .variational import refuse_spike_and_slab


class _LazySigma(LazyArray):
    """Sigma = K - K diag(beta) Ai diag(beta) K = K - K woodbury_inv K (N x N), formed on fetch from the two fetched matrices."""

    def __init__(self, K, woodbury_inv):
        self._K, self._wi = K, woodbury_inv
        self.shape = K.shape

    def fetch(self):
        if self._host is None:
            K = np.asarray(self._K)
            self._host = K - K.dot(np.asarray(self._wi)).dot(K)
        return self._host


class VarGaussPosterior(PosteriorExact):
    """Posterior(woodbury_vector = alpha, woodbury_inv = diag(beta) Ai diag(beta), K) with mean = K alpha as the device returned
    it and a lazy `covariance` (Sigma).  There is no Cholesky factor of a Ky, so `woodbury_chol` is None."""

    def __init__(self, woodbury_vector, woodbury_inv, K, mean, state=None):
        super(VarGaussPosterior, self).__init__(woodbury_chol=None, woodbury_vector=woodbury_vector, K=K,
                                                woodbury_inv=woodbury_inv, state=state)
        self._mean = mean
        self._covariance = _LazySigma(K, woodbury_inv)

    @property
    def covariance(self):
        return self._covariance

    def predictive_gradients(self, kern, Xnew, pred_var=None):
        raise NotImplementedError("predictive_gradients is not implemented for a non-Gaussian likelihood on this backend")

    def covariance_between_points(self, kern, X, X1, X2):
        raise NotImplementedError("covariance_between_points is not implemented for a non-Gaussian likelihood on this backend")


class VarGauss(LatentFunctionInference):
    def __init__(self, alpha, beta, device=0, maxtries=5, reference_gradient=False):
        """alpha (N x 1) and beta (N, signed and unconstrained): the variational parameters, `Param`s whose `.gradient` every
        call of `inference` sets.  `reference_gradient`: dL_dK and the kernel gradients in the reference's row-scaled form
        (see the module's docstring) instead of the derivative of the bound."""
        self.alpha, self.beta = alpha, beta
        self.reference_gradient = reference_gradient
        self.device, self.maxtries = device, maxtries
        self._state = None

    def to_dict(self):
        return {"class": "GPy.inference.latent_function_inference.var_gauss.VarGauss"}

    def inference(self, kern, X, likelihood, Y, mean_function=None, Y_metadata=None, Z=None):
        refuse_spike_and_slab(X, "VarGauss")
        if mean_function is not None:
            raise NotImplementedError("VarGauss inference with a mean function is not implemented on the MI355X path")
        Y = entry_checks("VarGauss", "VarGauss inference", kern, Y)
        if not hasattr(likelihood, "variational_expectations"):
            raise NotImplementedError("VarGauss inference needs a likelihood with variational_expectations, %s has none"
                                      % type(likelihood).__name__)
        n = Y.shape[0]
        alpha, beta = np.asarray(self.alpha, dtype=np.float64), np.asarray(self.beta, dtype=np.float64)
        if alpha.size != n or beta.size != n:
            raise ValueError("VarGauss: alpha has %d and beta %d entries for %d data points" % (alpha.size, beta.size, n))
        st, kd = begin_session(self, kern, X, Y)
        ctx = st.ctx
        # A's diagonal is 1 + beta_i^2 K_ii: jitchol's ladder on the info codes of its device factorisation
        m, var, logdet, trAi, ma = jitter_ladder(lambda jit: ctx.vargauss_forward(alpha, beta, jit), kd, self.maxtries)[0]
        m, var = m[:, None], var[:, None]
        F, dF_dm, dF_dv, dF_dthetaL = likelihood.variational_expectations(Y, m, var, Y_metadata=Y_metadata)
        dL_dthetaL = dF_dthetaL.sum(1).sum(1) if dF_dthetaL is not None else np.array([])
        KL = 0.5 * (logdet + trAi - n + ma)
        log_marginal = float(np.sum(F) - KL)
        dalpha, dbeta, dtheta = ctx.vargauss_backward(dF_dm, dF_dv, exact=not self.reference_gradient)
        self.alpha.gradient = dalpha.reshape(np.shape(self.alpha))
        self.beta.gradient = dbeta.reshape(np.shape(self.beta))

        wv = alpha.reshape(n, 1).copy()
        st.woodbury_vector = wv
        dL_dK = DeviceResult(st, _lib.FETCH_DLDK, n, st.call_token, kernel_sig=kernel_signature(kern), fused_dtheta=dtheta)
        post = VarGaussPosterior(woodbury_vector=wv, woodbury_inv=DeviceResult(st, _lib.FETCH_KINV, n, st.call_token),
                                 K=DeviceResult(st, _lib.FETCH_K, n, st.call_token), mean=m, state=st)
        return post, log_marginal, {"dL_dK": dL_dK, "dL_dthetaL": dL_dthetaL, "fused": dtheta}

