"""`Laplace` inference backed by libmi355gp.so -- drop-in for `GPy.inference.latent_function_inference.Laplace` (reference
`GPy/inference/latent_function_inference/laplace.py:122-353`) for one output column.

The mode search is Rasmussen & Williams' Newton iteration with a Brent line search, as in the reference.  Per iteration the
device factors B = I + W^1/2 K W^1/2 and returns the full-step `Ki_f` and `K Ki_f` (`mi355gp_laplace_newton`); because
f_trial = K (Ki_f + s dKi_f) = f + s K dKi_f is linear in the step size s, the line search is O(N) host arithmetic.  The
likelihood's derivatives are O(N) host work; K, B, its factor and inverse, dL_dK and the posterior's woodbury_inv never leave
the device unless a caller materialises the lazy proxies."""
import warnings

import numpy as np

from . import _lib
from .inference import LatentFunctionInference, _DeviceState
from .lazy import DeviceResult, kernel_signature
from .linalg import jitter_ladder
from .posterior import PosteriorExact
from .variational import refuse_spike_and_slab


class _LaplaceState(_DeviceState):
    """The device state of a Laplace posterior: prediction goes through `mi355gp_laplace_predict`."""

    def predict(self, kern, Xnew, full_cov=False):
        return self.ctx.laplace_predict(kern.part_specs(), kern._slice_X(Xnew), self.woodbury_vector, full_cov=full_cov)

    def predictive_gradients(self, kern, Xnew, want_var=True):
        raise NotImplementedError("predictive_gradients of a Laplace posterior")

    def covariance_between_points(self, kern, X1, X2):
        raise NotImplementedError("covariance_between_points of a Laplace posterior")


def entry_checks(name, what, kern, Y):
    """The entry checks `Laplace` and `EP` share (`name` in the kernel sentence, `what` in the other); returns Y as float64."""
    Y = np.asarray(Y, dtype=np.float64)
    if Y.ndim != 2 or Y.shape[1] > 1:
        raise NotImplementedError("%s on the MI355X path takes one output column, Y has shape %r" % (what, Y.shape))
    if not getattr(kern, "fused_alone", False):          # a lone White / Bias / Coregionalize, or a foreign kernel
        raise NotImplementedError("the MI355X %s path evaluates gpy_amd kernels on the device" % name)
    return Y


def begin_session(inf, kern, X, Y):
    """The start of a session of the exact context, for `Laplace` and `EP`: X and Y uploaded, K = kern.K(X) resident
    (`mi355gp_laplace_begin`).  Returns (the device state, the mean of K's diagonal for the jitter ladder)."""
    X = np.asarray(X)
    if inf._state is None:
        inf._state = _LaplaceState(inf.device)
    st = inf._state
    st.ensure_data(kern._slice_X(X), _lib.f64(Y))
    st.call_token += 1
    st.ctx.laplace_begin(kern.part_specs())
    return st, float(np.mean(kern.jitter_diag(X)))


class LaplacePosterior(PosteriorExact):
    """Posterior(woodbury_vector = Ki_fhat, woodbury_inv = K_Wi_i, K) of reference `laplace.py:146`: there is no Cholesky
    factor of a Ky, so `woodbury_chol` is None."""

    def __init__(self, woodbury_vector, woodbury_inv, K, state=None):
        super(LaplacePosterior, self).__init__(woodbury_chol=None, woodbury_vector=woodbury_vector, K=K,
                                               woodbury_inv=woodbury_inv, state=state)

    def predictive_gradients(self, kern, Xnew, pred_var=None):
        raise NotImplementedError("predictive_gradients is not implemented for a non-Gaussian likelihood on this backend")

    def covariance_between_points(self, kern, X, X1, X2):
        raise NotImplementedError("covariance_between_points is not implemented for a non-Gaussian likelihood on this backend")


class Laplace(LatentFunctionInference):
    def __init__(self, device=0, maxtries=5):
        self.device, self.maxtries = device, maxtries
        self._mode_finding_tolerance = 1e-4
        self._mode_finding_max_iter = 30
        self.bad_fhat = False
        self.first_run = True
        self._previous_Ki_fhat = None
        self._state = None
        self.iterations = 0                  # Newton steps of the last call

    def to_dict(self):
        return {"class": "GPy.inference.latent_function_inference.laplace.Laplace"}

    def _W(self, likelihood, f, Y, Y_metadata):
        W = -likelihood.d2logpdf_df2(f, Y, Y_metadata=Y_metadata)
        if np.any(np.isnan(W)):
            raise ValueError("One or more element(s) of W is NaN")
        if not likelihood.log_concave:       # (reference `laplace.py:319-321`)
            W = np.clip(W, 1e-6, 1e+30)
        return W

    def inference(self, kern, X, likelihood, Y, mean_function=None, Y_metadata=None):
        assert mean_function is None, "inference with a mean function not implemented"
        refuse_spike_and_slab(X, "Laplace")
        Y = entry_checks("Laplace", "Laplace inference", kern, Y)
        st, kd = begin_session(self, kern, X, Y)
        ctx, n = st.ctx, Y.shape[0]

        def ladder(attempt):
            """jitchol's ladder on the info codes of the device factorisation of B, whose diagonal is 1 + W_i K_ii"""
            return jitter_ladder(attempt, kd, self.maxtries)[0]

        # ---- rasm_mode (reference `laplace.py:148-231`), cold start from Ki_f = 0 (:138) ----
        from scipy import optimize
        Ki_f = np.zeros_like(Y)
        f = np.zeros_like(Y)

        def obj(Ki_f, f):
            return -0.5 * np.sum(Ki_f * f) + np.sum(likelihood.logpdf(f, Y, Y_metadata=Y_metadata))
        difference, iteration = np.inf, 0
        while difference > self._mode_finding_tolerance and iteration < self._mode_finding_max_iter:
            W = self._W(likelihood, f, Y, Y_metadata)
            grad = likelihood.dlogpdf_df(f, Y, Y_metadata=Y_metadata)
            if np.any(np.isnan(grad)):
                raise ValueError("One or more element(s) of grad is NaN")
            b = W * f + grad
            a, Ka, _ = ladder(lambda jit: ctx.laplace_newton(W, b, jit))
            dKi_f = a[:, None] - Ki_f
            Kd = Ka[:, None] - f             # K dKi_f, because f = K Ki_f

            def inner_obj(step):
                return -obj(Ki_f + step * dKi_f, f + step * Kd)
            try:
                step = optimize.brent(inner_obj, tol=1e-4, maxiter=12)
            except Exception as e:           # SciPy >= 1.11: BracketError on a line that is flat to rounding (at the mode)
                if type(e).__name__ != "BracketError":
                    raise
                step = 0.0
            # Brent returns the step to 1e-4 only, which leaves 1e-4 of the distance to the mode behind: where the full Newton
            # step is as good to rounding (1e-12 of the objective) it is taken instead
            f_step, f_full = inner_obj(step), inner_obj(1.0)
            if f_full <= f_step + 1e-12 * max(1.0, abs(f_step)):
                step = 1.0
            Ki_f_new, f_new = Ki_f + step * dKi_f, f + step * Kd
            old_obj, new_obj = obj(Ki_f, f), obj(Ki_f_new, f_new)
            if new_obj < old_obj - 1e-12 * max(1.0, abs(old_obj)):      # (the reference compares without the rounding slack)
                raise ValueError("Shouldn't happen, brent optimization failing")
            difference = np.abs(new_obj - old_obj)
            Ki_f, f = Ki_f_new, f_new
            iteration += 1
        self.iterations = iteration
        if difference > self._mode_finding_tolerance:
            if not self.bad_fhat:
                warnings.warn("Not perfect mode found (f_hat). difference: {}, iteration: {} out of max {}".format(
                    difference, iteration, self._mode_finding_max_iter))
            self.bad_fhat = True
        elif self.bad_fhat:
            self.bad_fhat = False
            warnings.warn("f_hat now fine again. difference: {}, iteration: {} out of max {}".format(
                difference, iteration, self._mode_finding_max_iter))
        f_hat, Ki_fhat = f, Ki_f

        # ---- mode_computations (reference `laplace.py:233-306`) ----
        W = self._W(likelihood, f_hat, Y, Y_metadata)
        diag_Ki_W_i, logdet_I_KW = ladder(lambda jit: ctx.laplace_finish(W, jit))
        log_marginal = -0.5 * np.sum(Ki_fhat * f_hat) + np.sum(likelihood.logpdf(f_hat, Y, Y_metadata=Y_metadata)) \
            - 0.5 * logdet_I_KW
        dW_df = -likelihood.d3logpdf_df3(f_hat, Y, Y_metadata=Y_metadata)
        if np.any(np.isnan(dW_df)):
            raise ValueError("One or more element(s) of dW_df is NaN")
        dL_dfhat = -0.5 * (diag_Ki_W_i[:, None] * dW_df)
        dtheta = ctx.laplace_gradients(Ki_fhat, dL_dfhat)
        dL_dthetaL = np.zeros(likelihood.size)
        if likelihood.size > 0 and not getattr(likelihood, "is_fixed", False):
            # (reference `laplace.py:276-299`) explicit: sum dlogpdf_dtheta_i + 0.5 diag(Ki_W_i) . d2logpdf_df2_dtheta_i; implicit:
            # dL_dfhat^T (I - K K_Wi_i) K dlogpdf_df_dtheta_i = s . dlogpdf_df_dtheta_i with the one device vector s
            dlik, dlik_grad, dlik_hess = likelihood._laplace_gradients(f_hat, Y, Y_metadata=Y_metadata)
            s = ctx.laplace_implicit(dL_dfhat)
            for i in range(likelihood.size):
                dL_dthetaL[i] = (np.sum(dlik[i]) + 0.5 * np.sum(diag_Ki_W_i * dlik_hess[i][:, 0])) + np.dot(s, dlik_grad[i][:, 0])

        self.f_hat, self.W, self.diag_Ki_W_i = f_hat, W, diag_Ki_W_i
        self._previous_Ki_fhat = Ki_fhat.copy()
        st.woodbury_vector = Ki_fhat
        dL_dK = DeviceResult(st, _lib.FETCH_DLDK, n, st.call_token, kernel_sig=kernel_signature(kern), fused_dtheta=dtheta)
        post = LaplacePosterior(woodbury_vector=Ki_fhat, woodbury_inv=DeviceResult(st, _lib.FETCH_KINV, n, st.call_token),
                                K=DeviceResult(st, _lib.FETCH_K, n, st.call_token), state=st)
        return post, float(log_marginal), {"dL_dK": dL_dK, "dL_dthetaL": dL_dthetaL}
