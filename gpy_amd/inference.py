"""`ExactGaussianInference` backed by libmi355gp.so -- drop-in for
`GPy.inference.latent_function_inference.ExactGaussianInference` (reference
`GPy/inference/latent_function_inference/exact_gaussian_inference.py:11-88`).

`inference(kern, X, likelihood, Y, mean_function=None, Y_metadata=None, K=None, variance=None, Z_tilde=None)`
returns `(Posterior, log_marginal_likelihood, {'dL_dK', 'dL_dthetaL', 'dL_dm'})` like the reference; with a
gpy_amd kernel the whole evaluation (K build, Cholesky, alpha, Ky^-1, all gradients) is one C-ABI call and the
N x N results stay in HBM behind lazy proxies.  The jitter ladder of `jitchol` (reference
`GPy/util/linalg.py:56-75`) runs here, on LAPACK-style `info` codes from the device factorisation, and raises
the same `numpy.linalg.LinAlgError` messages (`gpy_amd.linalg.jitter_ladder`).  A kernel, leaf or combination, describes itself
to the device through `Kern.part_specs()` / `_slice_X()` / `jitter_diag()`.
"""
import numpy as np

from . import _lib
from .lazy import ArrayIdentity, DeviceResult, kernel_signature
from .likelihoods import Gaussian
from .linalg import jitter_ladder
from .posterior import PosteriorExact, StudentTPosterior
from .variational import refuse_spike_and_slab


class LatentFunctionInference(object):
    """What every inference class of the package shares with GPy's base (reference `latent_function_inference/__init__.py:38-49`):
    the optimisation hooks, which do nothing but forget the members named in `_per_optimization` (EP's approximation,
    reference `expectation_propagation.py:220-221`), and pickling without the members named in `_device_members` -- device
    handles and the identities of what was uploaded never travel (cf. reference `rbf.py:313-318`)."""
    _device_members = ("_state",)
    _per_optimization = ()

    def on_optimization_start(self):
        for name in self._per_optimization:
            setattr(self, name, None)

    def on_optimization_end(self):
        pass

    def __getstate__(self):
        d = dict(self.__dict__)
        d.update(dict.fromkeys(self._device_members))
        return d


class _DeviceState(object):
    """One uploaded (X, R) pair and the HBM buffers behind it."""

    def __init__(self, device):
        self.ctx = _lib.Context(device)
        self._idX = self._idR = None
        self.call_token = 0
        self.kern = None

    def __getstate__(self):              # the HBM buffers and the ctypes handle never travel
        return {"_idX": None, "_idR": None, "call_token": self.call_token, "kern": None, "ctx": None}

    def ensure_data(self, X, R):
        """Upload X / R unless the device already holds exactly these data.  An array the caller froze (the model drivers
        keep private read-only copies of X and Y, like GPy's `ObsAr`, reference `core/gp.py:44-60`) is recognised by
        identity in O(1); anything writable is compared element by element with a private copy (O(N D), negligible next
        to the N^3 step) -- an in-place edit of a caller-owned buffer is never missed."""
        same_x = self._idX is not None and self._idX.matches(X)
        if not same_x or self._idR is None or self._idR.value().shape != R.shape:
            self.ctx.set_data(X, R)
            self._idX, self._idR = ArrayIdentity(X), ArrayIdentity(R)
        elif not self._idR.matches(R):
            self.ctx.set_targets(R)
            self._idR = ArrayIdentity(R)

    @property
    def X(self):
        return None if self._idX is None else self._idX.value()

    @property
    def R(self):
        return None if self._idR is None else self._idR.value()

    def invalidate(self):
        """Forget what was uploaded: the next inference call uploads X and R again."""
        self._idX = self._idR = None

    def fetch(self, which, fortran_order=False):
        return self.ctx.fetch(which, fortran_order=fortran_order)

    def covariance_between_points(self, kern, X1, X2):
        # a lone kernel's active_dims were applied when X was uploaded: the new points are sliced the same way
        return self.ctx.covariance_between_points(kern.part_specs(), kern._slice_X(X1), kern._slice_X(X2))

    def predictive_gradients(self, kern, Xnew, want_var=True):
        """(dmu (M x D x Dy), dvar (M x D)) -- reference `core/gp.py:418-474`; raises NotImplementedError for kernel
        expressions the device entry does not take (products), which the caller then evaluates on the host."""
        from .kern import Poly
        if any(isinstance(k, Poly) for k in kern.leaves()):
            raise NotImplementedError("Poly has no gradients_X (reference `poly.py:47-48`)")       # before any device work
        specs = kern.part_specs()
        if any(s[4] != 0 for s in specs):                        # a non-zero term id: a factor of a product
            raise NotImplementedError("product kernels")
        Xs = kern._slice_X(Xnew)
        dmu, dvar = self.ctx.predictive_gradients(specs, Xs, want_var=want_var)
        if Xs.shape[1] == np.asarray(Xnew).shape[1]:
            return dmu, dvar
        full_mu = np.zeros((Xs.shape[0], np.asarray(Xnew).shape[1], dmu.shape[2]))   # active_dims of a single kernel
        full_mu[:, kern.active_dims, :] = dmu
        full_var = None
        if dvar is not None:
            full_var = np.zeros((Xs.shape[0], np.asarray(Xnew).shape[1]))
            full_var[:, kern.active_dims] = dvar
        return full_mu, full_var

    def predict(self, kern, Xnew, full_cov=False):
        return self.ctx.predict_sum(kern.part_specs(), kern._slice_X(Xnew), full_cov=full_cov)


class ExactGaussianInference(LatentFunctionInference):
    _device_members = ("_state", "_last")        # (`_last` holds the device state of the last call)

    def __init__(self, device=0, maxtries=5):
        self.device = device
        self.maxtries = maxtries
        self._state = None
        self.last_stage_ms = None
        self.collect_stage_ms = False
        self.keep_diag = True      # N doubles per call: diag(Ky^-1) for LOO without fetching the N x N inverse
        self._last = None

    def to_dict(self):
        return {"class": "GPy.inference.latent_function_inference.exact_gaussian_inference.ExactGaussianInference"}

    def LOO(self, kern, X, Y, likelihood, posterior, Y_metadata=None, K=None):
        """Leave-one-out log predictive densities (reference `exact_gaussian_inference.py:76-88`):
        -(0.5 log 2pi - 0.5 log c_ii + 0.5 g_i^2 / c_ii) with g = woodbury_vector, c = Ky^-1.  diag(Ky^-1) comes from the
        device's diag(dL_dK) = 0.5 (|alpha_i|^2 - Dy c_ii); the N x N inverse is never fetched."""
        g = np.asarray(posterior.woodbury_vector)
        last = self._last
        if last is not None and last["diag_dL_dK"] is not None and last["alpha"] is g:
            c_diag = ((np.sum(g * g, axis=1) - 2.0 * last["diag_dL_dK"]) / last["Dy"])[:, None]
        else:
            c_diag = np.diag(np.asarray(posterior.woodbury_inv))[:, None]
        neg = 0.5 * np.log(2 * np.pi) - 0.5 * np.log(c_diag) + 0.5 * (g ** 2) / c_diag
        return -neg

    def _run_with_ladder(self, attempt, diagA):
        """`attempt(extra_jitter)` -> (info, result) under jitchol's ladder"""
        (res,), _ = jitter_ladder(attempt, diagA, self.maxtries, check_diag=True)
        return res

    def inference(self, kern, X, likelihood, Y, mean_function=None, Y_metadata=None, K=None, variance=None,
                  Z_tilde=None):
        refuse_spike_and_slab(X, "ExactGaussianInference")
        X = np.asarray(X)
        Y = np.asarray(Y, dtype=np.float64)
        if variance is None:
            variance = likelihood.gaussian_variance(Y_metadata)
        noise = np.atleast_1d(np.asarray(variance, dtype=np.float64)).ravel()
        # (reference :42-50) R = Y - m; without a mean function R IS Y (same object every iteration: O(1) data check)
        R = _lib.f64(Y) if mean_function is None else _lib.f64(Y - mean_function.f(X))
        n = X.shape[0]
        # a lone White / Bias / Coregionalize, a foreign kernel or a given K: K comes from the host (`inference_given_K`)
        fused = K is None and getattr(kern, "fused_alone", False)
        Xdev = kern._slice_X(X) if fused else _lib.f64(X)
        if self._state is None:
            self._state = _DeviceState(self.device)
        st = self._state
        st.ensure_data(Xdev, R)
        st.call_token += 1
        want_ms = self.collect_stage_ms
        # Gaussian.exact_inference_gradients == sum(diag(dL_dK)) == trace(dL_dK), which the device already reduces:
        # only likelihoods with per-row noise terms need the N-vector diag(dL_dK) shipped back.
        trace_only = isinstance(likelihood, Gaussian) and noise.size == 1
        want_diag = self.keep_diag or not trace_only

        if fused:
            specs = kern.part_specs()
            diagA = kern.jitter_diag(X) + noise + 1e-8

            def attempt(extra):
                return st.ctx.exact_inference_sum(specs, noise, jitter=1e-8, extra_jitter=extra, want_alpha=True,
                                                  want_diag=want_diag, want_stage_ms=want_ms)
            res = self._run_with_ladder(attempt, diagA)
            sig = kernel_signature(kern)
            K_view = DeviceResult(st, _lib.FETCH_K, n, st.call_token)
            dL_dK = DeviceResult(st, _lib.FETCH_DLDK, n, st.call_token, kernel_sig=sig, fused_dtheta=res["dtheta"])
        else:
            if K is None:
                K = kern.K(X)
            K = _lib.f64(K)
            diagA = np.diag(K) + noise + 1e-8

            def attempt(extra):
                return st.ctx.inference_given_K(K, noise, jitter=1e-8, extra_jitter=extra, want_diag=want_diag,
                                                want_stage_ms=want_ms)
            res = self._run_with_ladder(attempt, diagA)
            K_view = K
            dL_dK = DeviceResult(st, _lib.FETCH_DLDK, n, st.call_token)
        self.last_stage_ms = res.get("stage_ms")

        log_marginal = res["lml"]
        if Z_tilde is not None:
            log_marginal += Z_tilde
        alpha = res["alpha"]
        if trace_only:
            dL_dthetaL = res["dnoise"]
        else:
            dL_dthetaL = likelihood.exact_inference_gradients(res["diag_dL_dK"], Y_metadata)
        self._last = {"alpha": alpha, "diag_dL_dK": res.get("diag_dL_dK"), "Dy": R.shape[1], "state": st,
                      "token": st.call_token}
        post = PosteriorExact(
            woodbury_chol=DeviceResult(st, _lib.FETCH_L, n, st.call_token, fortran_order=True),
            woodbury_vector=alpha, K=K_view,
            woodbury_inv=DeviceResult(st, _lib.FETCH_KINV, n, st.call_token), state=st)
        return post, log_marginal, {"dL_dK": dL_dK, "dL_dthetaL": dL_dthetaL, "dL_dm": alpha}


class ExactStudentTInference(LatentFunctionInference):
    """Student-t PROCESS inference (reference `exact_studentt_inference.py:13-52`): `inference(kern, X, Y, nu, mean_function=None,
    K=None)` -> (posterior, log_marginal, {'dL_dK', 'dL_dnu', 'dL_dm'}).  Same device pipeline as the Gaussian case
    (C-ABI `mi355gp_exact_studentt_sum`); the kernel gradients ride on the lazy dL_dK like in `ExactGaussianInference`."""

    def __init__(self, device=0, maxtries=5):
        self.device, self.maxtries = device, maxtries
        self._state = None

    def to_dict(self):
        return {"class": "GPy.inference.latent_function_inference.exact_studentt_inference.ExactStudentTInference"}

    def inference(self, kern, X, Y, nu, mean_function=None, K=None):
        from scipy.special import digamma
        if K is not None or not getattr(kern, "fused_alone", False):
            raise NotImplementedError("the MI355X Student-t path evaluates gpy_amd kernels on the device")
        refuse_spike_and_slab(X, "ExactStudentTInference")
        X = np.asarray(X)
        Y = np.asarray(Y, dtype=np.float64)
        m = 0 if mean_function is None else mean_function.f(X)
        R = _lib.f64(Y - m)
        specs = kern.part_specs()
        if self._state is None:
            self._state = _DeviceState(self.device)
        st = self._state
        st.ensure_data(kern._slice_X(X), R)
        st.call_token += 1
        nu = float(np.asarray(nu).ravel()[0])
        (r,), extra = jitter_ladder(lambda extra: st.ctx.exact_studentt_sum(specs, nu, jitter=1e-8, extra_jitter=extra),
                                    lambda: kern.jitter_diag(X), self.maxtries)
        N, beta = Y.shape[0], r["beta"]
        dL_dnu = -N / (nu - 2.0) + digamma(0.5 * (nu + N)) - digamma(0.5 * nu)
        dL_dnu -= np.log(1 + beta / (nu - 2.0))
        dL_dnu += ((nu + N) * beta) / ((nu - 2) * (beta + nu - 2))
        dL_dnu *= 0.5
        sig = kernel_signature(kern)
        dL_dK = DeviceResult(st, _lib.FETCH_DLDK, N, st.call_token, kernel_sig=sig, fused_dtheta=r["dtheta"])
        # beta of the reference's StudentTPosterior is sum(alpha * K alpha) = sum(alpha * R) - jitter |alpha|^2 (posterior.py:345)
        beta_post = beta - (1e-8 + extra) * float(np.sum(r["alpha"] ** 2))
        post = StudentTPosterior(deg_free=nu, beta=beta_post,
                                 woodbury_chol=DeviceResult(st, _lib.FETCH_L, N, st.call_token, fortran_order=True),
                                 woodbury_vector=r["alpha"], K=DeviceResult(st, _lib.FETCH_K, N, st.call_token),
                                 woodbury_inv=DeviceResult(st, _lib.FETCH_KINV, N, st.call_token), state=st)
        return post, r["lml"], {"dL_dK": dL_dK, "dL_dnu": dL_dnu, "dL_dm": r["scale"] * r["alpha"]}
