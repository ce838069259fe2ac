"""`EPDTC` inference and `SparseGPClassification` backed by libmi355gp.so -- drop-ins for
`GPy.inference.latent_function_inference.EPDTC` (reference `expectation_propagation.py:436-578`) and
`GPy.models.SparseGPClassification` (reference `models/sparse_gp_classification.py:12-50`) for certain inputs, one output
column, a zero prior mean and the Bernoulli likelihood with the probit link.

EP runs over the DTC posterior q(f) = N(mu, Sigma), Sigma = Knm (Kmm + Kmn diag(tau) Knm)^-1 Kmn, on the sparse device context
(include/mi355gp_epdtc.h): `epdtc_begin` builds and factors Kmm, `epdtc_recompute` is `posteriorParamsDTC._recompute`,
`epdtc_sweep` one sequential pass over the sites in blocks of 64 (with `parallel_updates=True` the site updates are O(N) NumPy
on mu and diag(Sigma)).  After convergence `epdtc_inference` is the VarDTC evaluation with targets v / tau, per-point precision
tau and no jitter on Kmm (the reference passes `Lm`, `var_dtc.py:93` is skipped); its result lies where VarDTC's does, so
prediction and the lazy views are the sparse path's own.  Nothing N x M leaves the device."""
import numpy as np

from .ep import cavityParams, gaussianApproximation, marginalMoments, posteriorParams
from .ep import EP as _EP
from .kern import RBF
from .lazy import LazyNM
from .likelihoods import Bernoulli
from .link_functions import Probit
from .linalg import LinAlgError, jitter_ladder
from .sparse import SparseGP, SparseSession, sparse_path_kernel_check
from .variational import NormalPosterior, refuse_spike_and_slab

log_2_pi = np.log(2 * np.pi)


class EPDTC(SparseSession):
    _per_optimization = ("_ep_approximation",)
    _stop_criteria = _EP._stop_criteria

    def __init__(self, epsilon=1e-6, eta=1., delta=1., always_reset=False, max_iters=np.inf, ep_mode="alternated",
                 parallel_updates=False, device=0, maxtries=5, linear=False):
        super(EPDTC, self).__init__(device=device, maxtries=maxtries, linear=linear)
        self.always_reset = always_reset
        self.epsilon, self.eta, self.delta, self.max_iters = epsilon, eta, delta, max_iters
        self.ep_mode = ep_mode
        self.parallel_updates = parallel_updates
        self.iterations = 0                  # sweeps of the last run of expectation_propagation
        self.reset()

    def reset(self):
        self.ga_approx_old = None
        self._ep_approximation = None

    def to_dict(self):
        """(reference `expectation_propagation.py:232-243,577-578`)"""
        d = {"class": "GPy.inference.latent_function_inference.expectation_propagation.EPDTC", "epsilon": self.epsilon,
             "eta": self.eta, "delta": self.delta, "always_reset": self.always_reset, "max_iters": self.max_iters,
             "ep_mode": self.ep_mode, "parallel_updates": self.parallel_updates, "loading": True}
        if self.ga_approx_old is not None:
            d["ga_approx_old"] = self.ga_approx_old.to_dict()
        if self._ep_approximation is not None:
            post, ga, lz = self._ep_approximation
            d["_ep_approximation"] = {"post_params": post.to_dict(), "ga_approx": ga.to_dict(), "log_Z_tilde": float(lz)}
        return d

    # ---- the public entry point (reference `expectation_propagation.py:437-492`) ------------------------------------------
    def inference(self, kern, X, Z, likelihood, Y, mean_function=None, Y_metadata=None, Lm=None, dL_dKmm=None, psi0=None,
                  psi1=None, psi2=None):
        if mean_function is not None:
            raise NotImplementedError("EPDTC on the MI355X path takes a zero prior mean: a mean function is not implemented")
        refuse_spike_and_slab(X, "EPDTC")
        if isinstance(X, NormalPosterior):
            raise NotImplementedError("EPDTC on the MI355X path takes certain inputs: a NormalPosterior X "
                                      "(SparseGPClassificationUncertainInput) is not implemented")
        if any(a is not None for a in (Lm, dL_dKmm, psi0, psi1, psi2)):
            raise NotImplementedError("precomputed statistics (Lm, dL_dKmm, psi0, psi1, psi2) are not accepted by EPDTC on the "
                                      "MI355X path")
        Y = np.asarray(Y, dtype=np.float64)
        if Y.ndim != 2 or Y.shape[1] != 1:
            raise NotImplementedError("EPDTC takes one output column (ep in 1D only, expectation_propagation.py:442), got Y of "
                                      "shape %r" % (Y.shape,))
        if not isinstance(likelihood, Bernoulli):
            raise NotImplementedError("EPDTC on the MI355X path matches moments for the Bernoulli likelihood only, not %s"
                                      % type(likelihood).__name__)
        if not isinstance(likelihood.gp_link, Probit):
            raise NotImplementedError("EPDTC on the MI355X path matches moments for the probit link only, not %s"
                                      % type(likelihood.gp_link).__name__)
        sparse_path_kernel_check(kern, self.linear)
        if self.ep_mode not in ("nested", "alternated"):
            raise ValueError("ep_mode value not valid")
        self._refuse_sharded("a row-sharded sparse context is not supported by EPDTC")
        if self.always_reset:
            self.reset()
        Xs, Zs = kern._slice_X(X), kern._slice_X(Z)
        self._ensure(Xs, Y)
        specs = kern.part_specs()
        # Lm = jitchol(kern.K(Z)) (:448-450): the ladder runs on the device factorisation's info, its jitter stays on Kmm
        _, self._jitter = jitter_ladder(lambda jit: self._ctx.epdtc_begin(specs, Zs, jit), lambda: kern.jitter_diag(Z), self.maxtries)
        if self.ep_mode == "nested":
            self._ep_approximation = None
        if self._ep_approximation is None:
            self._ep_approximation = self.expectation_propagation(Y, likelihood, Y_metadata)
        post_params, ga_approx, log_Z_tilde = self._ep_approximation

        info, r = self._ctx.epdtc_inference(specs, Zs, ga_approx.tau, ga_approx.v, self._jitter,
                                            want_stage_ms=self.collect_stage_ms)
        if info != 0:
            raise LinAlgError("not positive definite, even with jitter.")
        self._token += 1
        self.last_stage_ms = r.get("stage_ms")
        M, N = Zs.shape[0], Xs.shape[0]
        post, dL_dKmm = self._posterior(kern, M, r["woodbury_vector"])
        grad_dict = {"dL_dKmm": dL_dKmm,
                     "dL_dKdiag": -0.5 * ga_approx.tau,                               # var_dtc.py:218 with beta = tau
                     "dL_dKnm": LazyNM(self, N, M),
                     "dL_dthetaL": likelihood.exact_inference_gradients(r["dL_dR"], Y_metadata),
                     "dL_dm": None,
                     "fused": {"dtheta": r["dtheta"], "dZ": r["dZ"]}}
        return post, r["lml"] + log_Z_tilde, grad_dict

    # ---- the sweeps (reference `expectation_propagation.py:494-575`) ------------------------------------------------------
    def _recompute(self, ga_approx):
        """`posteriorParamsDTC._recompute` on the device"""
        info, mu, sd = self._ctx.epdtc_recompute(ga_approx.tau, ga_approx.v)
        if info != 0:
            raise LinAlgError("not positive definite, even with jitter.")
        return posteriorParams(mu, sd)

    def expectation_propagation(self, Y, likelihood, Y_metadata=None):
        num_data, data_dim = Y.shape
        assert data_dim == 1, "This EP methods only works for 1D outputs"
        marg_moments = marginalMoments(num_data)
        cav_params = cavityParams(num_data)
        ga_approx, post_params = self._init_approximations(num_data)
        self._first_site = True              # the first site visited sees Sigma_ii + 1e-8 (:538, :547), cold or warm
        stop, iterations = False, 0
        while not stop and iterations < self.max_iters:
            self._local_updates(num_data, cav_params, post_params, marg_moments, ga_approx, likelihood, Y, Y_metadata)
            post_params = self._recompute(ga_approx)
            post_params.Sigma_diag = np.maximum(post_params.Sigma_diag, np.finfo(float).eps)
            if iterations > 0:
                stop = self._stop_criteria(ga_approx)
            self.ga_approx_old = gaussianApproximation(ga_approx.v.copy(), ga_approx.tau.copy())
            iterations += 1
        self.iterations = iterations
        self._cav_params = cav_params
        return post_params, ga_approx, self._log_Z_tilde(marg_moments, ga_approx, cav_params)

    def _init_approximations(self, num_data):
        """cold start (tau = v = 0: Sigma_diag = diag(Qnn), mu = 0) or warm start from the sites of the last run; either way
        every Sigma_ii carries 1e-8 until the first rank-one update (:538, :547)"""
        if self.ga_approx_old is None:
            ga_approx = gaussianApproximation(np.zeros(num_data), np.zeros(num_data))
        else:
            assert self.ga_approx_old.v.size == num_data, "data size mis-match: did you change the data? try resetting!"
            ga_approx = gaussianApproximation(self.ga_approx_old.v, self.ga_approx_old.tau)
        post_params = self._recompute(ga_approx)
        post_params.Sigma_diag = post_params.Sigma_diag + 1e-8
        return ga_approx, post_params

    def _local_updates(self, num_data, cav_params, post_params, marg_moments, ga_approx, likelihood, Y, Y_metadata=None,
                       update_order=None):
        if update_order is None:
            update_order = np.random.permutation(num_data)
        if not self.parallel_updates:
            r = self._ctx.epdtc_sweep(update_order, likelihood._ep_sign(Y[:, 0]), ga_approx.tau, ga_approx.v, self.eta,
                                      self.delta, first=self._first_site)
            self._first_site = False
            ga_approx.tau, ga_approx.v = r["tau"], r["v"]
            cav_params.tau, cav_params.v = r["cav_tau"], r["cav_v"]
            marg_moments.log_Z_hat, marg_moments.mu_hat, marg_moments.sigma2_hat = r["log_Z_hat"], r["mu_hat"], r["sigma2_hat"]
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
        """(reference `expectation_propagation.py:514-520`, with log Z_hat carried as a logarithm)"""
        mu_tilde = ga_approx.v / ga_approx.tau
        mu_cav = cav_params.v / cav_params.tau
        sigma2_sigma2tilde = 1. / cav_params.tau + 1. / ga_approx.tau
        return np.sum(marg_moments.log_Z_hat + 0.5 * log_2_pi + 0.5 * np.log(sigma2_sigma2tilde)
                      + 0.5 * ((mu_cav - mu_tilde) ** 2) / sigma2_sigma2tilde)


class SparseGPClassification(SparseGP):
    """Sparse Gaussian-process classification (reference `GPy/models/sparse_gp_classification.py:12-50`): the reference's
    signature and defaults -- an RBF kernel, `Bernoulli()`, Z a random `num_inducing` rows of X, `EPDTC()`."""

    def __init__(self, X, Y=None, likelihood=None, kernel=None, Z=None, num_inducing=10, Y_metadata=None, mean_function=None,
                 inference_method=None, normalizer=False, device=0):
        if mean_function is not None:
            raise NotImplementedError("SparseGPClassification on the MI355X path takes a zero prior mean: a mean function is not "
                                      "implemented")
        if normalizer:
            raise NotImplementedError("SparseGPClassification: a normalizer is not implemented on the MI355X path")
        refuse_spike_and_slab(X, "SparseGPClassification")
        if isinstance(X, NormalPosterior):
            raise NotImplementedError("SparseGPClassification takes certain inputs: a NormalPosterior X "
                                      "(SparseGPClassificationUncertainInput) is not implemented on the MI355X path")
        X = np.asarray(X, dtype=np.float64)
        if kernel is None:
            kernel = RBF(X.shape[1], device=device)
        if likelihood is None:
            likelihood = Bernoulli()
        if isinstance(likelihood, Bernoulli):
            likelihood.check_targets(Y)
        if Z is None:
            i = np.random.permutation(X.shape[0])[:num_inducing]
            Z = X[i].copy()
        else:
            assert np.asarray(Z).shape[1] == X.shape[1]
        if inference_method is None:
            inference_method = EPDTC(device=device)
        super(SparseGPClassification, self).__init__(X, Y, Z, kernel, likelihood, inference_method=inference_method,
                                                     name="SparseGPClassification", device=device, Y_metadata=Y_metadata)

    def optimize(self, max_iters=100, messages=False, gtol=1e-6):
        """`SparseGP.optimize` between the inference method's hooks (reference `core/gp.py:677-684`): in "alternated" mode EP runs
        once at the start and the sites stay fixed while the kernel and Z move"""
        self.inference_method.on_optimization_start()
        try:
            return super(SparseGPClassification, self).optimize(max_iters=max_iters, messages=messages, gtol=gtol)
        finally:
            self.inference_method.on_optimization_end()

    def to_dict(self):
        return {"class": "GPy.models.SparseGPClassification", "name": self.name, "kernel": self.kern.to_dict(),
                "likelihood": self.likelihood.to_dict(), "inference_method": self.inference_method.to_dict()}
