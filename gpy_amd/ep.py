"""`EP` inference backed by libmi355gp.so -- drop-in for `GPy.inference.latent_function_inference.EP` (reference
`GPy/inference/latent_function_inference/expectation_propagation.py:187-417`) for one output column, a zero prior mean and the
Bernoulli likelihood with the probit link.

EP runs inside a Laplace session of the exact context: K is resident, `mi355gp_ep_recompute` factors B = I + S^1/2 K S^1/2
(S = diag(tau_tilde)) and forms mu and Sigma, `mi355gp_ep_sweep` does one sequential pass over the sites with its N rank-one
updates of the N x N Sigma on the device.  With `parallel_updates=True` the site updates are O(N) NumPy on mu and diag(Sigma).
The final pass is the session's own calls with W = tau_tilde, b = v_tilde (alpha, log det B, the woodbury_inv, dL_dK, the kernel
gradients, prediction).  Nothing N x N leaves the device unless a caller materialises the lazy proxies."""
import numpy as np

from . import _lib
from .inference import LatentFunctionInference
from .laplace import begin_session, entry_checks
from .lazy import DeviceResult, kernel_signature
from .likelihoods import Bernoulli
from .linalg import jitter_ladder
from .link_functions import Probit
from .posterior import PosteriorEP
from .variational import refuse_spike_and_slab

log_2_pi = np.log(2 * np.pi)


class marginalMoments(object):
    """moments of the tilted distributions; the normaliser is carried as its logarithm (the reference exponentiates at
    `bernoulli.py:92` and takes the log again at `expectation_propagation.py:357`)"""

    def __init__(self, num_data):
        self.log_Z_hat = np.empty(num_data, dtype=np.float64)
        self.mu_hat = np.full(num_data, np.nan)
        self.sigma2_hat = np.full(num_data, np.nan)

    @property
    def Z_hat(self):
        return np.exp(self.log_Z_hat)


class cavityParams(object):
    def __init__(self, num_data):
        self.tau = np.empty(num_data, dtype=np.float64)
        self.v = np.empty(num_data, dtype=np.float64)

    def to_dict(self):
        return {"tau": self.tau.tolist(), "v": self.v.tolist()}


class gaussianApproximation(object):
    def __init__(self, v, tau):
        self.tau = tau
        self.v = v

    def to_dict(self):
        return {"tau": self.tau.tolist(), "v": self.v.tolist()}


class posteriorParams(object):
    """mu and diag(Sigma) of q(f); the full Sigma of the reference's class of this name stays on the device"""

    def __init__(self, mu, Sigma_diag, logdet=None):
        self.mu, self.Sigma_diag, self.logdet = mu, Sigma_diag, logdet

    def to_dict(self):
        return {"mu": self.mu.tolist(), "Sigma_diag": self.Sigma_diag.tolist()}


class EP(LatentFunctionInference):
    _per_optimization = ("_ep_approximation",)

    def __init__(self, epsilon=1e-6, eta=1., delta=1., always_reset=False, max_iters=np.inf, ep_mode="alternated",
                 parallel_updates=False, device=0, maxtries=5):
        self.always_reset = always_reset
        self.epsilon, self.eta, self.delta, self.max_iters = epsilon, eta, delta, max_iters
        self.ep_mode = ep_mode
        self.parallel_updates = parallel_updates
        self.device, self.maxtries = device, maxtries
        self._state = None
        self.iterations = 0                  # sweeps of the last run of expectation_propagation
        self.reset()

    def reset(self):
        self.ga_approx_old = None
        self._ep_approximation = None

    def _stop_criteria(self, ga_approx):
        tau_diff = np.mean(np.square(ga_approx.tau - self.ga_approx_old.tau))
        v_diff = np.mean(np.square(ga_approx.v - self.ga_approx_old.v))
        return (tau_diff < self.epsilon) and (v_diff < self.epsilon)

    def to_dict(self):
        """(reference `expectation_propagation.py:232-243,397-417`, without the N x N members of post_params)"""
        d = {"class": "GPy.inference.latent_function_inference.expectation_propagation.EP", "epsilon": self.epsilon,
             "eta": self.eta, "delta": self.delta, "always_reset": self.always_reset, "max_iters": self.max_iters,
             "ep_mode": self.ep_mode, "parallel_updates": self.parallel_updates, "loading": True}
        if self.ga_approx_old is not None:
            d["ga_approx_old"] = self.ga_approx_old.to_dict()
        if self._ep_approximation is not None:
            post, ga, cav, lz = self._ep_approximation
            d["_ep_approximation"] = {"post_params": post.to_dict(), "ga_approx": ga.to_dict(), "cav_params": cav.to_dict(),
                                      "log_Z_tilde": float(lz)}
        return d

    def _with_ladder(self, attempt):
        """jitchol's ladder on the info codes of the device factorisation of B"""
        return jitter_ladder(attempt, self._kd, self.maxtries)[0]

    # ---- the public entry point (reference `expectation_propagation.py:246-277`) -----------------------------------------
    def inference(self, kern, X, likelihood, Y, mean_function=None, Y_metadata=None, precision=None, K=None):
        refuse_spike_and_slab(X, "EP")
        if mean_function is not None:
            raise NotImplementedError("EP on the MI355X path takes a zero prior mean: a mean function is not implemented")
        if precision is not None:
            raise NotImplementedError("EP on the MI355X path does not take precision=: the site precisions stay on the device path")
        if K is not None:
            raise NotImplementedError("EP on the MI355X path builds K on the device from the kernel: K= is not taken")
        Y = entry_checks("EP", "EP", kern, Y)
        if not isinstance(likelihood, Bernoulli):
            raise NotImplementedError("EP on the MI355X path matches moments for the Bernoulli likelihood only, not %s"
                                      % type(likelihood).__name__)
        if not isinstance(likelihood.gp_link, Probit):
            raise NotImplementedError("EP on the MI355X path matches moments for the probit link only, not %s"
                                      % type(likelihood.gp_link).__name__)
        if self.ep_mode not in ("nested", "alternated"):
            raise ValueError("ep_mode value not valid")
        if self.always_reset:
            self.reset()
        st, self._kd = begin_session(self, kern, X, Y)
        self._ctx, n = st.ctx, Y.shape[0]

        if self.ep_mode == "nested":
            self._ep_approximation = None
        if self._ep_approximation is None:
            self._ep_approximation = self.expectation_propagation(Y, likelihood, Y_metadata)
        post_params, ga_approx, cav_params, log_Z_tilde = self._ep_approximation
        return self._inference(kern, st, n, Y, ga_approx, cav_params, likelihood, log_Z_tilde, Y_metadata)

    # ---- the sweeps (reference `expectation_propagation.py:279-361`) ----------------------------------------------------
    def _recompute(self, ga_approx, add_diag=0.0):
        """`posteriorParams._recompute` on the device; the full Sigma is formed only where the sequential sweep needs it"""
        mu, sd, logdet = self._with_ladder(lambda jit: self._ctx.ep_recompute(ga_approx.tau, ga_approx.v, jit, add_diag,
                                                                              want_sigma=not self.parallel_updates))
        return posteriorParams(mu, sd, logdet)

    def expectation_propagation(self, Y, likelihood, Y_metadata=None):
        num_data, data_dim = Y.shape
        assert data_dim == 1, "This EP methods only works for 1D outputs"
        Y = np.array(Y, dtype=np.float64)
        marg_moments = marginalMoments(num_data)
        cav_params = cavityParams(num_data)
        ga_approx, post_params = self._init_approximations(num_data)
        stop, iterations = False, 0
        while not stop and iterations < self.max_iters:
            self._local_updates(num_data, cav_params, post_params, marg_moments, ga_approx, likelihood, Y, Y_metadata)
            new = self._recompute(ga_approx)
            post_params.mu, post_params.Sigma_diag, post_params.logdet = new.mu, new.Sigma_diag, new.logdet
            if iterations > 0:
                stop = self._stop_criteria(ga_approx)
            self.ga_approx_old = gaussianApproximation(ga_approx.v.copy(), ga_approx.tau.copy())
            iterations += 1
        self.iterations = iterations
        return post_params, ga_approx, cav_params, self._log_Z_tilde(marg_moments, ga_approx, cav_params)

    def _init_approximations(self, num_data):
        """cold start (Sigma = K + 1e-7 I, mu = 0) or warm start from the sites of the last run: the one device call serves both"""
        if self.ga_approx_old is None:
            ga_approx = gaussianApproximation(np.zeros(num_data), np.zeros(num_data))
        else:
            assert self.ga_approx_old.v.size == num_data, "data size mis-match: did you change the data? try resetting!"
            ga_approx = gaussianApproximation(self.ga_approx_old.v, self.ga_approx_old.tau)
        return ga_approx, self._recompute(ga_approx, add_diag=1e-7)

    def _local_updates(self, num_data, cav_params, post_params, marg_moments, ga_approx, likelihood, Y, Y_metadata=None,
                       update_order=None):
        if update_order is None:
            update_order = np.random.permutation(num_data)
        if not self.parallel_updates:
            r = self._ctx.ep_sweep(update_order, likelihood._ep_sign(Y[:, 0]), ga_approx.tau, ga_approx.v, self.eta, self.delta)
            ga_approx.tau, ga_approx.v = r["tau"], r["v"]
            cav_params.tau, cav_params.v = r["cav_tau"], r["cav_v"]
            marg_moments.log_Z_hat = r["log_Z_hat"]
            post_params.mu, post_params.Sigma_diag = r["mu"], r["Sigma_diag"]
            return
        # every site sees the same q(f), so the order does not matter and the updates are whole-vector arithmetic
        eps = np.finfo(float).eps
        cav_params.tau = 1. / post_params.Sigma_diag - self.eta * ga_approx.tau
        cav_params.v = post_params.mu / post_params.Sigma_diag - self.eta * ga_approx.v
        marg_moments.log_Z_hat, marg_moments.mu_hat, marg_moments.sigma2_hat = likelihood.log_moments_match_ep(
            Y[:, 0], cav_params.tau, cav_params.v)
        delta_tau = self.delta / self.eta * (1. / marg_moments.sigma2_hat - 1. / post_params.Sigma_diag)
        delta_v = self.delta / self.eta * (marg_moments.mu_hat / marg_moments.sigma2_hat - post_params.mu / post_params.Sigma_diag)
        ga_approx.tau = np.maximum(ga_approx.tau + delta_tau, eps)
        ga_approx.v = ga_approx.v + delta_v

    def _log_Z_tilde(self, marg_moments, ga_approx, cav_params):
        return np.sum(marg_moments.log_Z_hat + 0.5 * log_2_pi + 0.5 * np.log(1 + ga_approx.tau / cav_params.tau)
                      - 0.5 * (ga_approx.v ** 2 / (cav_params.tau + ga_approx.tau))
                      + 0.5 * (cav_params.v * ((ga_approx.tau / cav_params.tau * cav_params.v - 2.0 * ga_approx.v)
                                               / (cav_params.tau + ga_approx.tau))))

    # ---- the final pass (reference `expectation_propagation.py:363-395`) -------------------------------------------------
    def _ep_marginal(self, ga_approx, Z_tilde):
        """(log marginal, alpha): v^T Sigma v of the reference is v^T mu, mu = K alpha"""
        alpha, mu, B_logdet = self._with_ladder(lambda jit: self._ctx.laplace_newton(ga_approx.tau, ga_approx.v, jit))
        log_marginal = 0.5 * (-len(ga_approx.tau) * log_2_pi - B_logdet + np.sum(ga_approx.v * mu)) + Z_tilde
        return float(log_marginal), alpha

    def _inference(self, kern, st, n, Y, ga_approx, cav_params, likelihood, Z_tilde, Y_metadata=None):
        ctx = self._ctx
        log_marginal, alpha = self._ep_marginal(ga_approx, Z_tilde)
        self._with_ladder(lambda jit: ctx.laplace_finish(ga_approx.tau, jit))
        dtheta = ctx.laplace_gradients(alpha, np.zeros(n))       # dL_dK = 0.5 (alpha alpha^T - Wi), reduced per kernel part
        alpha = alpha[:, None]
        st.woodbury_vector = alpha
        dL_dK = DeviceResult(st, _lib.FETCH_DLDK, n, st.call_token, kernel_sig=kernel_signature(kern), fused_dtheta=dtheta)
        dL_dthetaL = likelihood.ep_gradients(Y, cav_params.tau, cav_params.v, None, Y_metadata=Y_metadata, quad_mode="gh")
        post = PosteriorEP(woodbury_vector=alpha, woodbury_inv=DeviceResult(st, _lib.FETCH_KINV, n, st.call_token),
                           K=DeviceResult(st, _lib.FETCH_K, n, st.call_token), state=st)
        return post, log_marginal, {"dL_dK": dL_dK, "dL_dthetaL": dL_dthetaL, "dL_dm": alpha}
