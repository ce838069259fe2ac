"""Sparse GP regression (VarDTC) backed by libmi355gp.so -- drop-in for the hot path of
`GPy.inference.latent_function_inference.VarDTC` + `GPy.core.SparseGP` / `GPy.models.SparseGPRegression`
(reference `var_dtc.py:66-215`, `core/sparse_gp.py:76-119`, `models/sparse_gp_regression.py:20-60`) for certain inputs
and a homoscedastic Gaussian likelihood (BASELINE config 5).

`VarDTC.inference(kern, X, Z, likelihood, Y, ...)` returns `(Posterior, log_marginal, grad_dict)` with the reference's
keys, for gpy_amd's stationary kernels, `Linear` where the class is made with `linear=True`, products of those and Bias, and sums
(`Add`) of those and White / Bias parts, a scalar or per-point
Gaussian noise variance and an optional mean function.  The N x M matrix `dL_dKnm` is never resident: the kernel and
inducing-input gradients that `SparseGP._update_gradients` derives from it are reduced on the device in the second
streaming pass and travel in `grad_dict['fused']`; `dL_dKmm` is a lazy device view and `dL_dKnm` a lazy object that a
foreign consumer can materialise in row blocks (`mi355gp_sparse_fetch_dLdKnm`).

Uncertain inputs: an X that is a `NormalPosterior` (or `SparseGPRegression(X, Y, X_variance=...)`) is evaluated through the
RBF psi-statistics on the device (`mi355gp_vardtc_inference_uncertain`) for one RBF kernel alone or summed with White parts
and one noise variance; `grad_dict` then has the reference's keys `dL_dpsi0 / dL_dpsi1 / dL_dpsi2` in place of
`dL_dKdiag / dL_dKnm`, and `fused` also carries the gradients with respect to the inputs' means and variances.
`VarDTC(psi_lin_bias=True)` (and the models' keyword of the same name) takes one RBF or Linear part with Bias and White parts
there (`mi355gp_sparse_set_psi_lin_bias`, include/mi355gp_psi_lin.h); made without it the classes refuse those as before.

Multi-output kernels: `VarDTC(coregionalize=True)` takes Coregionalize factors with certain inputs -- the `ICM` / `LCM` kernels of
`util.multioutput` with a `MixedNoise` likelihood -- and `SparseGPCoregionalizedRegression` (reference
`models/sparse_gp_coregionalized_regression.py`) is the `SparseGP` built on it, with inducing inputs that carry a fixed output
index (`mi355gp_sparse_set_coregionalize`, include/mi355gp_sparse_coreg.h); made without the keyword the classes refuse the kind
as before.

`BayesianGPLVM` (reference `models/bayesian_gplvm.py`) is the `SparseGP` whose inputs are parameters: it consumes those
gradients, subtracts the KL term of the standard normal prior, uploads a step's new means and variances without Y
(`mi355gp_sparse_set_inputs`) and predicts at uncertain new points on the device (`mi355gp_sparse_predict_uncertain`).
"""
import numpy as np

from . import _lib
from .inference import LatentFunctionInference
from .kern import RBF, Add, Bias, Coregionalize, Linear, Prod, White, diag_depends_on_point, exact_only_leaves, has_coregionalize
from .lazy import ArrayIdentity, LazyMM, LazyNM, LazyPsi1, freeze, kernel_signature
from .likelihoods import Gaussian
from .linalg import LinAlgError, jitter_ladder
from .models import PredictionCallers
from .param import Param, Parameterized
from .variational import NormalPosterior, NormalPrior, SpikeAndSlabPosterior, SpikeAndSlabPrior, refuse_spike_and_slab


class SessionPosterior(object):
    """A posterior made by a `SparseSession`: `_device` = {"ctx", "token", "owner", "sig"} names the context, the session
    (`owner`), its evaluation count when the posterior was made and the kernel's signature."""
    _device = None

    def _live(self, kern=None):
        """True while the posterior is the context's latest result (and, given a kernel, `kern` is the one it was made with)"""
        dev = self._device
        return (dev is not None and dev["owner"]._token == dev["token"]
                and (kern is None or kernel_signature(kern) == dev["sig"]))


class SparsePosterior(SessionPosterior):
    """`Posterior(woodbury_inv, woodbury_vector, K=Kmm, K_chol=Lm)` of the reference (`var_dtc.py:213`,
    `posterior.py:21-77`); prediction follows `Posterior._raw_predict` (`posterior.py:198-262`) and runs on the device
    (C-ABI `mi355gp_sparse_predict`) while the posterior is the context's latest result."""

    psi_lin_bias = False        # made by an inference class with psi_lin_bias=True: the host fallback asks `Add` for the same

    def __init__(self, woodbury_inv, woodbury_vector, K, K_chol, device=None):
        self.woodbury_inv, self.woodbury_vector, self.K, self.K_chol = woodbury_inv, woodbury_vector, K, K_chol
        self._device = device

    def __getstate__(self):
        d = dict(self.__dict__)
        d["_device"] = None
        for k in ("woodbury_inv", "K", "K_chol"):
            d[k] = np.asarray(d[k])
        return d

    def _raw_predict(self, kern, Xnew, pred_var, full_cov=False):
        dev, live = self._device, self._live(kern)
        if isinstance(Xnew, SpikeAndSlabPosterior):
            raise NotImplementedError("prediction at spike-and-slab new points (a SpikeAndSlabPosterior Xnew) is not implemented; "
                                      "pass their means, or a NormalPosterior")
        if isinstance(Xnew, NormalPosterior):
            return self._raw_predict_uncertain(kern, Xnew, pred_var, full_cov, dev if live else None)
        if live:
            return dev["ctx"].predict(kern.part_specs(), kern._slice_X(Xnew), full_cov=full_cov)
        Kx = kern.K(pred_var, Xnew)                                   # (M, N*): foreign kernel / stale device state
        mu = np.dot(Kx.T, self.woodbury_vector)
        Wi = np.asarray(self.woodbury_inv)
        if full_cov:
            var = kern.K(Xnew) - np.dot(Kx.T, np.dot(Wi, Kx))
        else:
            var = (kern.Kdiag(Xnew) - np.sum(np.dot(Wi.T, Kx) * Kx, 0))[:, None]
            var = np.clip(var, 1e-15, np.inf)                        # posterior.py:248
        return mu, var

    def _raw_predict_uncertain(self, kern, Xnew, pred_var, full_cov, dev):
        """at points q(x*) = N(mean, diag variance) (reference `posterior.py:249-269`): on the device
        (C-ABI `mi355gp_sparse_predict_uncertain`) while the posterior is the context's latest result, otherwise from
        `kern.psi0 / psi1 / psi2n` on the host, in row blocks that keep the N* x M x M array bounded"""
        if full_cov:
            raise NotImplementedError("Full covariance at uncertain new points is not implemented (the reference has none either)")
        if dev is not None:
            return dev["ctx"].predict_uncertain(kern.part_specs(), kern._slice_X(Xnew.mean), kern._slice_X(Xnew.variance))
        la, Wi = np.asarray(self.woodbury_vector), np.asarray(self.woodbury_inv)
        M, n = la.shape[0], Xnew.shape[0]
        step = max(1, (1 << 22) // (M * M))                          # at most 32 MB of psi2n at a time
        mu, var = np.empty((n, la.shape[1])), np.empty((n, la.shape[1]))
        kw = {"psi_lin_bias": True} if self.psi_lin_bias and isinstance(kern, Add) else {}
        for r0 in range(0, n, step):
            q = Xnew[r0:r0 + step]
            psi0, psi1, psi2n = kern.psi0(pred_var, q, **kw), kern.psi1(pred_var, q, **kw), kern.psi2n(pred_var, q, **kw)
            mb = np.dot(psi1, la)
            vb = np.einsum("nmo,md,od->nd", psi2n, la, la) - mb * mb + psi0[:, None] - np.einsum("nmo,mo->n", psi2n, Wi)[:, None]
            mu[r0:r0 + step], var[r0:r0 + step] = mb, np.clip(vb, 1e-15, np.inf)
        return mu, var

    def predictive_gradients(self, kern, Xnew, pred_var=None):
        """(reference `core/gp.py:418-474` with `_predictive_variable` = Z): M is small, the M x M Woodbury inverse comes to
        the host and the reductions over the inducing points run through `kern.gradients_X`."""
        return _host_predictive_gradients(kern, Xnew, pred_var, self.woodbury_vector, self.woodbury_inv)

    def covariance_between_points(self, kern, X, X1, X2):
        """K(X1, X2) - K(X1, Z) woodbury_inv K(Z, X2) (reference `posterior.py:109-130`)"""
        return kern.K(X1, X2) - np.dot(kern.K(X1, X), np.dot(np.asarray(self.woodbury_inv), kern.K(X, X2)))


class MissingDataPosterior(SessionPosterior):
    """The posterior of a fit with missing data (reference `sparse_gp_minibatch.py:274-283`): `woodbury_vector` (M x Dy) and a
    3-D `woodbury_inv` (M x M x Dy, `woodbury_inv[:, :, d]` = the matrix of output d's group), expanded from the G matrices on
    the device when it is first read.  Prediction (`posterior.py:233-246`, `:268`) runs on the device, one contraction per
    group, while the posterior is the context's latest result; afterwards on the host from the expanded array, if it was read
    in time."""

    def __init__(self, woodbury_vector, group_of_output, K, K_chol, device=None):
        self.woodbury_vector, self.group_of_output, self.K, self.K_chol = woodbury_vector, np.asarray(group_of_output), K, K_chol
        self._device, self._wi = device, None

    @property
    def woodbury_inv(self):
        if self._wi is None:
            if not self._live():
                raise RuntimeError("MissingDataPosterior.woodbury_inv: the device context has moved on to a later evaluation; "
                                   "read woodbury_inv (or predict) before the next one")
            ctx, gof = self._device["ctx"], self.group_of_output
            M = self.woodbury_vector.shape[0]
            wi = np.empty((M, M, gof.size))
            for g in range(int(gof.max()) + 1):
                ctx.select_output_group(g)
                wi[:, :, gof == g] = ctx.fetch(ctx.FETCH_WOODBURY_INV)[:, :, None]
            self._wi = wi
        return self._wi

    def __getstate__(self):
        """as `SparsePosterior`: no device handle travels; the lazy members are materialised (woodbury_inv while it still can be)"""
        d = dict(self.__dict__)
        if d["_wi"] is None and self._live():
            d["_wi"] = self.woodbury_inv
        d["_device"] = None
        for k in ("K", "K_chol"):
            d[k] = np.asarray(d[k])
        return d

    def _raw_predict(self, kern, Xnew, pred_var, full_cov=False):
        if isinstance(Xnew, SpikeAndSlabPosterior):
            raise NotImplementedError("prediction at spike-and-slab new points (a SpikeAndSlabPosterior Xnew) is not implemented; "
                                      "pass their means, or a NormalPosterior")
        uncertain = isinstance(Xnew, NormalPosterior)
        if uncertain and full_cov:
            raise NotImplementedError("Full covariance at uncertain new points is not implemented (the reference has none either)")
        if self._live(kern) and not full_cov:
            ctx = self._device["ctx"]
            if uncertain:
                return ctx.predict_missing(kern.part_specs(), kern._slice_X(Xnew.mean), kern._slice_X(Xnew.variance))
            return ctx.predict_missing(kern.part_specs(), kern._slice_X(Xnew))
        Wi, la = self.woodbury_inv, np.asarray(self.woodbury_vector)
        if uncertain:                                                  # posterior.py:250-269 with the 3-D woodbury_inv, in row
            M, n = la.shape[0], Xnew.shape[0]                          # blocks that keep the N* x M x M array bounded
            step = max(1, (1 << 22) // (M * M))                        # at most 32 MB of psi2n at a time
            mu, var = np.empty((n, la.shape[1])), np.empty((n, la.shape[1]))
            for r0 in range(0, n, step):
                q = Xnew[r0:r0 + step]
                psi0, psi1, psi2n = kern.psi0(pred_var, q), kern.psi1(pred_var, q), kern.psi2n(pred_var, q)
                mb = np.dot(psi1, la)
                vb = np.einsum("nmo,md,od->nd", psi2n, la, la) - mb * mb + psi0[:, None] - np.einsum("nmo,mod->nd", psi2n, Wi)
                mu[r0:r0 + step], var[r0:r0 + step] = mb, np.clip(vb, 1e-15, np.inf)
            return mu, var
        Kx = kern.K(pred_var, Xnew)
        mu = np.dot(Kx.T, la)
        if full_cov:                                                   # posterior.py:233-237
            Kxx = kern.K(Xnew)
            return mu, np.stack([Kxx - Kx.T.dot(Wi[:, :, i]).dot(Kx) for i in range(Wi.shape[2])], axis=2)
        Kd = kern.Kdiag(Xnew)
        var = np.stack([Kd - np.sum(np.dot(Wi[:, :, i].T, Kx) * Kx, 0) for i in range(Wi.shape[2])], axis=1)
        return mu, np.clip(var, 1e-15, np.inf)


def _host_predictive_gradients(kern, Xnew, pred_var, woodbury_vector, woodbury_inv):
    """`GP.predictive_gradients` (reference `core/gp.py:440-474`, woodbury_inv.ndim == 2) composed from `kern.gradients_X`
    (device reductions) and the M x M / N x N Woodbury inverse."""
    Xnew = np.asarray(Xnew, dtype=np.float64)
    wv = np.asarray(woodbury_vector)
    mean_jac = np.empty((Xnew.shape[0], Xnew.shape[1], wv.shape[1]))
    for i in range(wv.shape[1]):
        mean_jac[:, :, i] = kern.gradients_X(wv[:, i:i + 1].T * np.ones((Xnew.shape[0], 1)), Xnew, pred_var)
    var_jac = kern.gradients_X_diag(np.ones(Xnew.shape[0]), Xnew)
    a2 = -2.0 * np.dot(kern.K(Xnew, pred_var), np.asarray(woodbury_inv))
    return mean_jac, var_jac + kern.gradients_X(a2, Xnew, pred_var)


def sparse_path_kernel_check(kern, linear=False, coregionalize=False):
    """What the sparse device context evaluates (VarDTC and SVGP alike); anything else is refused by name.  `linear`: the
    inference class was made with `linear=True` and takes Linear leaves; without it they are refused like the other kinds
    that only the exact path has, as they were before the sparse path could evaluate them.  `coregionalize`: likewise for
    Coregionalize leaves (`VarDTC(coregionalize=True)`, the one class that takes them), as factors of a product -- what `ICM` /
    `LCM` build -- with at most 16 outputs."""
    refused = [k for k in exact_only_leaves(kern)
               if not (linear and k == "Linear") and not (coregionalize and k == "Coregionalize")]
    if refused:
        hint = "; Linear: make the inference class with linear=True" if "Linear" in refused else ""
        if "Coregionalize" in refused:
            hint += "; Coregionalize: VarDTC(coregionalize=True) or SparseGPCoregionalizedRegression"
        raise NotImplementedError("the MI355X sparse path does not evaluate %s kernels (the exact GPRegression path does%s)"
                                  % (", ".join(sorted(set(refused))), hint))
    for k in (kern.leaves() if coregionalize else []):
        if isinstance(k, Coregionalize) and k.output_dim > 16:
            raise NotImplementedError("the MI355X sparse path evaluates Coregionalize kernels with at most 16 outputs, %r has %d"
                                      % (k.name, k.output_dim))
    # stationary and Linear kernels, products (Prod, reference `prod.py:58-99`) of stationary / Linear / Bias / Coregionalize
    # factors, and sums (Add) of those and of White / Bias parts
    def _prod_ok(k):
        return isinstance(k, Prod) and not any(isinstance(f, (White, Add, Prod)) for f in k.parts)
    lone = getattr(kern, "is_leaf", False) and kern.fused_alone          # (not a lone White / Bias)
    ok = lone or _prod_ok(kern) or (
        isinstance(kern, Add) and all(_prod_ok(p) if isinstance(p, Prod) else not isinstance(p, Add) for p in kern.parts))
    if not ok:
        raise NotImplementedError("the MI355X sparse path covers gpy_amd's stationary kernels and Linear, products of "
                                  "stationary / Linear / Bias factors and sums (Add) of those and of White / Bias parts")


def noise_variances(likelihood, Y_metadata, precision=None):
    """the Gaussian noise variances as a flat array: the likelihood's, or 1 / precision where one is given (var_dtc.py:78-80)"""
    if precision is None:
        return np.atleast_1d(np.asarray(likelihood.gaussian_variance(Y_metadata), dtype=np.float64)).ravel()
    return 1.0 / np.atleast_1d(np.asarray(precision, dtype=np.float64)).ravel()


class SparseSession(LatentFunctionInference):
    """The host side that `VarDTC`, `PEP` / `FITC` and `SVGP` share: one sparse device context, made on first use; the identities
    of the (X, Y) it holds, so that `set_data` runs only when they change; and `_token`, the count of evaluations, by which a
    posterior or a lazy view knows whether it is still the context's latest result.  An `inference` method is its refusals,
    `_ensure`, one `_run` over a context call and the results built by `_posterior` / `_device_dict`."""
    _device_members = ("_ctx", "_X", "_Y")

    coregionalize = False       # `VarDTC(coregionalize=True)` alone takes Coregionalize leaves; the other families have no keyword

    def __init__(self, device=0, maxtries=5, linear=False, psi_lin_bias=False):
        self.device, self.maxtries = device, maxtries
        # psi_lin_bias: uncertain inputs take one RBF or Linear part with Bias and White parts (`VarDTC`); implies `linear`
        self.psi_lin_bias = bool(psi_lin_bias)
        self.linear = bool(linear) or self.psi_lin_bias   # take Linear leaves (Kdiag by point on the device); off: refused by name, as before
        self._ctx = None
        self._X = self._Y = None
        self._token = 0
        self.last_stage_ms = None
        self.collect_stage_ms = False

    def _refuse_sharded(self, message):
        if self._ctx is not None and getattr(self._ctx, "sharded", False):
            raise NotImplementedError(message)

    def _ensure(self, X, Y):
        """one context, `set_data` only when X or Y changed (True then): frozen arrays (the model driver's X / Y) are
        recognised by identity, anything else by a full comparison"""
        if self._ctx is None:
            self._ctx = _lib.SparseContext(self.device)
            if self.psi_lin_bias:
                self._ctx.set_psi_lin_bias(True)                       # (switches Linear on as well)
            elif self.linear:
                self._ctx.set_linear(True)
            if self.coregionalize:
                self._ctx.set_coregionalize(True)                      # (before set_data: it keeps the rows for the index check)
        if self._X is not None and self._X.matches(X) and self._Y.matches(Y):
            return False
        self._ctx.set_data(X, Y)
        self._X, self._Y = ArrayIdentity(X), ArrayIdentity(Y)
        return True

    def _run(self, kern, call, Z):
        """One evaluation: `call(extra_jitter)` -> (info, result) on the context under jitchol's ladder (util/linalg.py:56-75)
        for Kmm, whose first rung is mean(diag Kmm) * 1e-6 (:65): `kern.jitter_diag(Z)`, one number unless a Linear leaf makes
        the diagonal depend on the inducing point.  Its result is then the context's latest: everything made from earlier
        ones is stale."""
        (r,), _ = jitter_ladder(call, lambda: kern.jitter_diag(Z), self.maxtries)
        self._token += 1
        self.last_stage_ms = r.get("stage_ms")
        return r

    def _device_dict(self, kern):
        return {"ctx": self._ctx, "token": self._token, "owner": self, "sig": kernel_signature(kern)}

    def _posterior(self, kern, M, woodbury_vector):
        """(`SparsePosterior` of the evaluation just run, its lazy dL_dKmm)"""
        C = _lib.SparseContext
        post = SparsePosterior(woodbury_inv=LazyMM(self, C.FETCH_WOODBURY_INV, M), woodbury_vector=woodbury_vector,
                               K=LazyMM(self, C.FETCH_KMM, M), K_chol=LazyMM(self, C.FETCH_LM, M), device=self._device_dict(kern))
        post.psi_lin_bias = self.psi_lin_bias
        return post, LazyMM(self, C.FETCH_DLDKMM, M)


class VarDTC(SparseSession):
    const_jitter = 1e-8
    _device_members = SparseSession._device_members + ("_S", "_G", "_groups_of", "_groups_mask")
    _S = None                                                        # identity of the uploaded input variances
    _G = None                                                        # ... and of the slab probabilities (None: Gaussian inputs)
    _groups_of = None                                                # the uploaded Y (its identity) the context's output groups belong to
    _groups_mask = None                                              # ... and the (group_of_output, W) that were uploaded with it

    def __init__(self, device=0, maxtries=5, linear=False, psi_lin_bias=False, coregionalize=False):
        """`coregionalize=True`: the kernel may hold Coregionalize factors (`util.multioutput.ICM` / `LCM`) with certain inputs;
        the context is told so (`mi355gp_sparse_set_coregionalize`).  Made without it the class refuses them by name, as before."""
        super(VarDTC, self).__init__(device=device, maxtries=maxtries, linear=linear, psi_lin_bias=psi_lin_bias)
        self.coregionalize = bool(coregionalize)

    def to_dict(self):
        return {"class": "GPy.inference.latent_function_inference.var_dtc.VarDTC"}

    def _ensure(self, X, Y):
        if super(VarDTC, self)._ensure(X, Y):
            self._S = self._G = None                                   # (set_data discards input variances and slab probabilities)

    def _ensure_uncertain(self, mu, S, R):
        if (self._ctx is not None and self._X is not None and self._Y.matches(R) and self._X.value().shape == mu.shape
                and not self._X.matches(mu)):
            self._ctx.set_inputs(mu, S)                                # the same Y, new inputs: Y is not uploaded again
            self._X, self._S = ArrayIdentity(mu), ArrayIdentity(S)
        else:
            self._ensure(mu, R)
            if self._S is None or not self._S.matches(S):
                self._ctx.set_input_variance(S)
                self._S = ArrayIdentity(S)
        if self._G is not None:                                        # the context last held spike-and-slab inputs
            self._ctx.set_binary_prob(None)
            self._G = None

    def _ensure_ss(self, mu, S, G, R):
        if (self._ctx is not None and self._X is not None and self._Y.matches(R) and self._X.value().shape == mu.shape
                and not (self._X.matches(mu) and self._S is not None and self._S.matches(S)
                         and self._G is not None and self._G.matches(G))):
            self._ctx.set_inputs_ss(mu, S, G)                          # the same Y, new inputs: Y is not uploaded again
            self._X, self._S, self._G = ArrayIdentity(mu), ArrayIdentity(S), ArrayIdentity(G)
            return
        self._ensure(mu, R)
        if self._S is None or not self._S.matches(S):
            self._ctx.set_input_variance(S)
            self._S = ArrayIdentity(S)
        if self._G is None or not self._G.matches(G):
            self._ctx.set_binary_prob(G)
            self._G = ArrayIdentity(G)

    def _inference_uncertain(self, kern, qX, Z, likelihood, Y, Y_metadata, mean_function, precision, Z_tilde):
        """X is a `NormalPosterior`: the psi-statistics form of the same evaluation (reference `var_dtc.py:66-215` with
        `uncertain_inputs`), for one RBF kernel alone or summed with White parts and ONE noise variance."""
        if mean_function is not None:                                  # var_dtc.py:85-86
            raise ValueError("Mean function not implemented with uncertain inputs or heteroscedasticity")
        ss = isinstance(qX, SpikeAndSlabPosterior)                     # -> mi355gp_vardtc_inference_ss: one RBF and White parts
        parts = kern.parts if isinstance(kern, Add) else [kern]
        covered = (RBF, Linear, Bias, White) if self.psi_lin_bias and not ss else (RBF, White)
        for p in parts:
            if type(p) not in covered:
                what = type(p).__name__ if p.is_leaf else "%s of %s" % (type(p).__name__, ", ".join(type(f).__name__ for f in p.leaves()))
                if ss:
                    raise NotImplementedError("spike-and-slab inputs: the part %r (%s) has no psi-statistics on the MI355X sparse "
                                              "path; one RBF kernel and White parts are covered (the reference's Linear "
                                              "statistics, sslinear_psi_comp, are not implemented)" % (p.name, what))
                if self.psi_lin_bias:
                    raise NotImplementedError("uncertain inputs: the part %r (%s) has no psi-statistics on the MI355X sparse path; "
                                              "one RBF or Linear kernel with Bias and White parts is covered" % (p.name, what))
                raise NotImplementedError("uncertain inputs: the part %r (%s) has no psi-statistics on the MI355X sparse path; "
                                          "one RBF kernel and White parts are covered (one RBF or Linear kernel with Bias and "
                                          "White parts: make the inference class with psi_lin_bias=True)" % (p.name, what))
        rbfs = [p for p in parts if isinstance(p, (RBF, Linear))]
        if len(rbfs) != 1 and self.psi_lin_bias and not ss:
            raise NotImplementedError("uncertain inputs: exactly one input-dependent part (RBF or Linear) is covered, got %d (%s); "
                                      "psi2 of two has cross terms that need E[k1 k2^T]"
                                      % (len(rbfs), ", ".join("%r: %s" % (p.name, type(p).__name__) for p in rbfs)))
        if len(rbfs) != 1:
            raise NotImplementedError("uncertain inputs: exactly one RBF part is covered, got %d (%s)"
                                      % (len(rbfs), ", ".join(repr(p.name) for p in rbfs)))
        Y = np.asarray(Y, dtype=np.float64)
        noise = noise_variances(likelihood, Y_metadata, precision)
        if noise.size > 1:                                             # var_dtc.py:243
            raise NotImplementedError("heteroscedastic (per-point) noise is not implemented with uncertain inputs")
        mu, S, Zs = kern._slice_X(qX.mean), kern._slice_X(qX.variance), kern._slice_X(Z)
        R = _lib.f64(Y)
        self._refuse_sharded("uncertain inputs are not supported by a row-sharded sparse context")
        specs = kern.part_specs()
        if ss:
            self._ensure_ss(mu, S, kern._slice_X(qX.binary_prob), R)
            call = self._ctx.vardtc_ss
        else:
            self._ensure_uncertain(mu, S, R)
            call = self._ctx.vardtc_uncertain
        r = self._run(kern, lambda extra: call(specs, Zs, noise, extra_jitter=extra, want_stage_ms=self.collect_stage_ms), Z)
        M, N = Zs.shape[0], mu.shape[0]
        post, dL_dKmm = self._posterior(kern, M, r["woodbury_vector"])
        beta = float(1.0 / np.fmax(noise, self.const_jitter)[0])
        grad_dict = {"dL_dKmm": dL_dKmm,
                     "dL_dpsi0": -0.5 * Y.shape[1] * beta * np.ones(N),             # var_dtc.py:218
                     "dL_dpsi1": LazyPsi1(beta, R, r["woodbury_vector"]),
                     "dL_dpsi2": LazyMM(self, _lib.SparseContext.FETCH_DLDPSI2_BETA, M, scale=beta),
                     "dL_dthetaL": likelihood.exact_inference_gradients(r["dnoise"], Y_metadata),
                     "fused": {"dtheta": r["dtheta"], "dZ": r["dZ"], "dmu": r["dmu"], "dS": r["dS"]}}
        if ss:
            grad_dict["fused"]["dgamma"] = r["dgamma"]
        return post, r["lml"] + (0.0 if Z_tilde is None else Z_tilde), grad_dict

    def _inference_missing(self, kern, qX, Z, likelihood, Y, Y_metadata, mean_function, precision, Lm, dL_dKmm, psi0, psi1, psi2,
                           Z_tilde):
        """NaNs in Y define groups of output columns with the same observed rows (order: first output index, reference
        `stochastics.py:57-79`); one device call evaluates the reference's loop over them (`sparse_gp_minibatch.py:228-286`):
        `mi355gp_sparse_set_output_groups` + `mi355gp_vardtc_inference_missing`.  X is a `NormalPosterior`, the kernel one RBF
        alone or summed with White parts, the noise one variance.  Everything else is refused by name before a context is
        touched."""
        if any(a is not None for a in (Lm, dL_dKmm, psi0, psi1, psi2)):
            raise NotImplementedError("precomputed statistics are not accepted by the MI355X sparse path")
        if isinstance(qX, SpikeAndSlabPosterior):
            raise NotImplementedError("missing_data: spike-and-slab inputs are not implemented with missing data on the MI355X path")
        if not isinstance(qX, NormalPosterior):
            raise NotImplementedError("missing_data: certain inputs (the reference's SparseGPMiniBatch) are not implemented on the "
                                      "MI355X path; missing data is handled for a NormalPosterior X (BayesianGPLVMMiniBatch)")
        if self.psi_lin_bias or self.linear or self.coregionalize:
            raise NotImplementedError("missing_data: an inference class made with psi_lin_bias, linear or coregionalize is not "
                                      "implemented with missing data; make it as VarDTC()")
        if mean_function is not None:
            raise ValueError("Mean function not implemented with uncertain inputs or heteroscedasticity")
        parts = kern.parts if isinstance(kern, Add) else [kern]
        for p in parts:
            if type(p) not in (RBF, White):
                raise NotImplementedError("missing_data: the part %r (%s) is not implemented with missing data on the MI355X path; "
                                          "one RBF kernel and White parts are" % (p.name, type(p).__name__))
        if sum(isinstance(p, RBF) for p in parts) != 1:
            raise NotImplementedError("missing_data: exactly one RBF part is covered, got %d" % sum(isinstance(p, RBF) for p in parts))
        noise = noise_variances(likelihood, Y_metadata, precision)
        if noise.size > 1:
            raise NotImplementedError("heteroscedastic (per-point) noise is not implemented with missing data")
        self._refuse_sharded("missing data is not supported by a row-sharded sparse context")
        gof, W, Y0 = _lib.output_groups(Y)
        empty = [int(np.argmax(gof == g)) for g in range(W.shape[1]) if not W[:, g].any()]
        if empty:
            raise ValueError("missing_data: output column %d has no observed entry" % empty[0])
        mu, S, Zs = kern._slice_X(qX.mean), kern._slice_X(qX.variance), kern._slice_X(Z)
        self._ensure_uncertain(mu, S, Y0)
        # set_data forgets the groups, set_inputs keeps them; and the zero-filled Y alone does not tell a NaN from an observed 0.0:
        # the mask is compared as well
        if (self._groups_of is not self._Y or not np.array_equal(self._groups_mask[0], gof)
                or not np.array_equal(self._groups_mask[1], W)):
            self._ctx.set_output_groups(gof, W)
            self._groups_of, self._groups_mask = self._Y, (gof, W)
        specs = kern.part_specs()
        r = self._run(kern, lambda extra: self._ctx.vardtc_missing(specs, Zs, noise, extra_jitter=extra,
                                                                   want_stage_ms=self.collect_stage_ms), Z)
        M = Zs.shape[0]
        C = _lib.SparseContext
        post = MissingDataPosterior(r["woodbury_vector"], gof, K=LazyMM(self, C.FETCH_KMM, M), K_chol=LazyMM(self, C.FETCH_LM, M),
                                    device=self._device_dict(kern))
        beta = float(1.0 / np.fmax(noise, self.const_jitter)[0])
        counts = np.bincount(gof, minlength=W.shape[1]).astype(np.float64)           # outputs per group
        grad_dict = {"dL_dKmm": LazyMM(self, C.FETCH_DLDKMM, M),
                     "dL_dpsi0": -0.5 * beta * W.dot(counts),                         # -beta/2 times the outputs observed at n
                     "dL_dpsi1": LazyPsi1(beta, Y0, r["woodbury_vector"]),
                     "dL_dthetaL": likelihood.exact_inference_gradients(r["dnoise"], Y_metadata),
                     "fused": {"dtheta": r["dtheta"], "dZ": r["dZ"], "dmu": r["dmu"], "dS": r["dS"],
                               "group_scalars": r["group_scalars"], "group_of_output": gof, "W": W}}
        return post, r["lml"] + (0.0 if Z_tilde is None else Z_tilde), grad_dict

    def inference(self, kern, X, Z, likelihood, Y, Y_metadata=None, mean_function=None, precision=None, Lm=None,
                  dL_dKmm=None, psi0=None, psi1=None, psi2=None, Z_tilde=None, missing_data=False):
        if missing_data:
            return self._inference_missing(kern, X, Z, likelihood, Y, Y_metadata, mean_function, precision, Lm, dL_dKmm, psi0, psi1,
                                           psi2, Z_tilde)
        if self._groups_of is not None:                                # the context last held a fit with missing data
            self._ctx.set_output_groups(None, None)
            self._groups_of = self._groups_mask = None
        uncertain = isinstance(X, (NormalPosterior, SpikeAndSlabPosterior))
        if not uncertain:
            sparse_path_kernel_check(kern, self.linear, self.coregionalize)
        if any(a is not None for a in (Lm, dL_dKmm, psi0, psi1, psi2)):
            raise NotImplementedError("precomputed statistics are not accepted by the MI355X sparse path")
        if uncertain:
            return self._inference_uncertain(kern, X, Z, likelihood, Y, Y_metadata, mean_function, precision, Z_tilde)
        Y = np.asarray(Y, dtype=np.float64)
        noise = noise_variances(likelihood, Y_metadata, precision)
        het = noise.size > 1
        if het and mean_function is not None:                          # var_dtc.py:85-86
            raise ValueError("Mean function not implemented with uncertain inputs or heteroscedasticity")
        m = 0 if mean_function is None else mean_function.f(X)
        Xs, Zs = kern._slice_X(X), kern._slice_X(Z)
        R = _lib.f64(Y - m)
        if has_coregionalize(kern):
            self._refuse_sharded("a Coregionalize kernel is not supported by a row-sharded sparse context: its Kdiag depends on the "
                                 "point, so the sums over rows would need another all-reduce")
        if diag_depends_on_point(kern):
            self._refuse_sharded("a Linear kernel is not supported by a row-sharded sparse context: its Kdiag depends on the "
                                 "point, so the sums over rows would need another all-reduce")
        self._ensure(Xs, R)
        specs = kern.part_specs()
        r = self._run(kern, lambda extra: self._ctx.vardtc_sum(specs, Zs, noise, extra_jitter=extra,
                                                               want_dL_dm=mean_function is not None,
                                                               want_stage_ms=self.collect_stage_ms), Z)
        M, N = Zs.shape[0], Xs.shape[0]
        post, dL_dKmm = self._posterior(kern, M, r["woodbury_vector"])
        beta = 1.0 / np.fmax(noise, self.const_jitter)
        dL_dR = (r["dnoise"][:, None] if r["dnoise"].ndim == 1 else r["dnoise"]) if het else r["dnoise"]   # N x Dy (var_dtc.py:240-256)
        grad_dict = {"dL_dKmm": dL_dKmm,
                     "dL_dKdiag": -0.5 * Y.shape[1] * (beta * np.ones(N)),            # var_dtc.py:218
                     "dL_dKnm": LazyNM(self, N, M),
                     "dL_dthetaL": likelihood.exact_inference_gradients(dL_dR, Y_metadata),
                     "dL_dm": r["dL_dm"],
                     "fused": {"dtheta": r["dtheta"], "dZ": r["dZ"]}}
        return post, r["lml"] + (0.0 if Z_tilde is None else Z_tilde), grad_dict


class SparseGP(PredictionCallers, Parameterized):
    """Model driver: the `SparseGP.parameters_changed` sequence (reference `core/sparse_gp.py:76-119`).
    Flat parameter order follows GPy's links: [Z, kern.variance, kern.lengthscale..., noise variance]
    (`sparse_gp.py:59`: Z is linked at index 0)."""

    _takes_spike_and_slab = False                # SSGPLVM alone holds a SpikeAndSlabPosterior; every other model refuses it by name

    def __init__(self, X, Y, Z, kernel, likelihood, inference_method=None, name="sparse gp", device=0, mean_function=None,
                 Y_metadata=None, X_variance=None):
        super(SparseGP, self).__init__(name)
        self.mean_function, self.Y_metadata = mean_function, Y_metadata
        self.Y = freeze(Y)                           # private read-only copies (cf. `ObsAr`, reference `core/gp.py:44-60`)
        if not self._takes_spike_and_slab:
            refuse_spike_and_slab(X, type(self).__name__)
        if isinstance(X, (NormalPosterior, SpikeAndSlabPosterior)):   # (reference `core/sparse_gp.py:45-51`)
            self.X = X.copy()
        elif X_variance is not None:                 # data, not a parameter: the flat parameter order is unchanged
            self.X = NormalPosterior(X, X_variance)
        else:
            self.X = freeze(X)
        if self.has_uncertain_inputs() and mean_function is not None:
            raise ValueError("Mean function not implemented with uncertain inputs or heteroscedasticity")
        self.Y_normalized = self.Y
        self.num_data, self.input_dim = self.X.shape
        self.output_dim = self.Y.shape[1]
        self.Z = Param("inducing inputs", np.asarray(Z, dtype=np.float64), positive=False)
        self.num_inducing = self.Z.shape[0]
        self.kern, self.likelihood = kernel, likelihood
        self.inference_method = inference_method or VarDTC(device=device)
        self.link_parameter(self.Z)
        self.link_parameter(self.kern)
        self.link_parameter(self.likelihood)
        self.posterior = None
        self.parameters_changed()

    def has_uncertain_inputs(self):
        """(reference `core/sparse_gp.py:68-69`)"""
        return isinstance(self.X, (NormalPosterior, SpikeAndSlabPosterior))

    def parameters_changed(self):
        # certain and uncertain inputs alike: the kernel and inducing-input gradients of `_update_gradients` (reference
        # `core/sparse_gp.py:88-118`, both branches) were reduced on the device and arrive in grad_dict['fused']
        self.posterior, self._log_marginal_likelihood, self.grad_dict = self.inference_method.inference(
            self.kern, self.X, self.Z.values, self.likelihood, self.Y_normalized, Y_metadata=self.Y_metadata,
            mean_function=self.mean_function)
        self.likelihood.update_gradients(self.grad_dict["dL_dthetaL"])
        if self.mean_function is not None:                                      # sparse_gp.py:84-85
            self.mean_function.update_gradients(self.grad_dict["dL_dm"], self.X)
        fused = self.grad_dict["fused"]
        self.kern._install_fused(fused["dtheta"])
        self.Z.gradient = fused["dZ"] if fused["dZ"].shape == self.Z.shape else self._scatter_dZ(fused["dZ"])

    def _scatter_dZ(self, dZ):
        full = np.zeros(self.Z.shape)
        full[:, self.kern.active_dims] = dZ
        return full

    def log_likelihood(self):
        return self._log_marginal_likelihood

    def objective_function(self):
        return -float(self._log_marginal_likelihood)

    def objective_function_gradients(self):
        return -self.gradient

    @property
    def _predictive_variable(self):
        """(reference `core/sparse_gp.py:72-74`)"""
        return self.Z.values

    def _raw_predict(self, Xnew, full_cov=False, kern=None):
        """(reference `core/sparse_gp.py:121-160` -> `posterior.py:198-262`; same signature as `GP._raw_predict`)"""
        if isinstance(Xnew, (NormalPosterior, SpikeAndSlabPosterior)):
            raise NotImplementedError("prediction at uncertain new points is not implemented; pass their means")
        mu, var = self.posterior._raw_predict(self.kern if kern is None else kern, np.asarray(Xnew), self.Z.values,
                                              full_cov=full_cov)
        if self.mean_function is not None:
            mu = mu + self.mean_function.f(Xnew)
        return mu, var

    def predict(self, Xnew, full_cov=False, Y_metadata=None, kern=None, likelihood=None, include_likelihood=True):
        """(reference `core/gp.py:308-365`, inherited by `SparseGP`: same argument order)"""
        mu, var = self._raw_predict(Xnew, full_cov, kern=kern)
        if include_likelihood:
            likelihood = self.likelihood if likelihood is None else likelihood
            mu, var = likelihood.predictive_values(mu, var, full_cov=full_cov,
                                                   Y_metadata=self.Y_metadata if Y_metadata is None else Y_metadata)
        return mu, var

    # ---- the optimiser's view of the parameters: positive ones (kernel, noise) in log space, the others untransformed --------
    def _positive(self):
        return np.concatenate([np.full(p.size, bool(p.positive)) for p in self.flattened_parameters()])

    @property
    def optimizer_array(self):
        pos, p = self._positive(), self.param_array
        return np.where(pos, np.log(np.where(pos, p, 1.0)), p)

    @optimizer_array.setter
    def optimizer_array(self, x):
        pos = self._positive()
        self.param_array = np.where(pos, np.exp(np.where(pos, x, 0.0)), x)

    def _grads(self, x):
        """gradient of the objective (the negative bound) in the optimiser's parameters at x"""
        self.optimizer_array = x
        pos, g = self._positive(), self.objective_function_gradients()
        return np.where(pos, g * self.param_array, g)

    def optimize(self, max_iters=100, messages=False, gtol=1e-6):
        """L-BFGS-B on `optimizer_array`"""
        from scipy.optimize import minimize

        def f(x):
            try:
                g = self._grads(x)
            except LinAlgError:
                return 1e300, np.zeros_like(x)
            return self.objective_function(), g
        res = minimize(f, self.optimizer_array, jac=True, method="L-BFGS-B",
                       options={"maxiter": max_iters, "gtol": gtol, "disp": bool(messages)})
        self.optimizer_array = res.x
        return res


class SparseGPRegression(SparseGP):
    """(reference `GPy/models/sparse_gp_regression.py:20-60`): Z defaults to a random subset of X.  `linear=True`: the kernel
    may hold Linear leaves (`VarDTC(linear=True)`).  `psi_lin_bias=True`: with `X_variance`, one RBF or Linear part with Bias
    and White parts (`VarDTC(psi_lin_bias=True)`; implies `linear`)."""

    def __init__(self, X, Y, kernel=None, Z=None, num_inducing=10, noise_var=1., device=0, seed=None, mean_function=None,
                 X_variance=None, linear=False, psi_lin_bias=False):
        refuse_spike_and_slab(X, "SparseGPRegression")
        X = np.asarray(X, dtype=np.float64)
        if kernel is None:
            kernel = RBF(X.shape[1], device=device)
        if Z is None:
            i = np.random.default_rng(seed).permutation(X.shape[0])[:min(num_inducing, X.shape[0])]
            Z = X[i].copy()
        super(SparseGPRegression, self).__init__(X, Y, Z, kernel, Gaussian(variance=noise_var),
                                                 inference_method=(VarDTC(device=device, psi_lin_bias=True) if psi_lin_bias else
                                                                   VarDTC(device=device, linear=True) if linear else None),
                                                 name="sparse_gp", device=device, mean_function=mean_function,
                                                 X_variance=X_variance)


class SparseGPCoregionalizedRegression(SparseGP):
    """Sparse multi-output GP regression with coregionalization (reference
    `GPy/models/sparse_gp_coregionalized_regression.py:11-99`): a `SparseGP` with `VarDTC(coregionalize=True)`, the per-output
    inputs stacked with an output-index column (`util.multioutput.build_XY`), an `ICM` of `RBF(D - 1)` unless a kernel is given,
    `MixedNoise` (one Gaussian noise per output) and inducing inputs that carry an output index: `Z_list[i]` belongs to
    output i, by default `num_inducing` (one number, or one per output) random rows of `X_list[i]`.  The flat parameter order
    is [Z, kernel, noise]; the index column of Z is fixed (the reference's `self['.*inducing'][:, -1].fix()`): its gradient is
    exactly zero and no assignment to the parameter vector moves it.  `predict(Xnew, Y_metadata={'output_index': ...})` takes
    Xnew with the index column appended."""

    def __init__(self, X_list, Y_list, Z_list=None, kernel=None, likelihoods_list=None, num_inducing=10, X_variance=None,
                 name="SGPCR", W_rank=1, kernel_name="coreg", device=0, seed=None):
        from .util import multioutput
        if X_variance is not None:
            raise NotImplementedError("SparseGPCoregionalizedRegression: X_variance (uncertain inputs) is not implemented on the "
                                      "MI355X path: a Coregionalize part has no psi-statistics")
        X, Y, self.output_index = multioutput.build_XY(X_list, Y_list)
        Ny = len(Y_list)
        if kernel is None:
            kernel = multioutput.ICM(input_dim=X.shape[1] - 1, num_outputs=Ny, kernel=RBF(X.shape[1] - 1, device=device),
                                     W_rank=W_rank, name=kernel_name)
        likelihood = multioutput.build_likelihood(Y_list, self.output_index, likelihoods_list)
        if Z_list is not None and len(Z_list):
            assert len(Z_list) == Ny, "Number of outputs do not match length of inducing inputs list."
            Z_list = [np.asarray(Zi, dtype=np.float64) for Zi in Z_list]
        else:                                        # (a list of the call's own: the reference appends into its shared default)
            ni = np.asarray([num_inducing] * Ny if isinstance(num_inducing, (int, np.integer)) else num_inducing)
            assert ni.size == Ny, "Number of outputs do not match length of inducing inputs list."
            rng = np.random.default_rng(seed)
            Z_list = [np.asarray(Xi, dtype=np.float64)[rng.permutation(np.shape(Xi)[0])[:n]].copy() for n, Xi in zip(ni, X_list)]
        Z, _, Iz = multioutput.build_XY(Z_list)
        self._Z_index = np.asarray(Iz, dtype=np.float64).ravel()       # before SparseGP.__init__: the first evaluation reads Z
        super(SparseGPCoregionalizedRegression, self).__init__(X, Y, Z, kernel, likelihood,
                                                               inference_method=VarDTC(device=device, coregionalize=True),
                                                               name=name, device=device,
                                                               Y_metadata={"output_index": self.output_index})

    @property
    def param_array(self):
        return SparseGP.param_array.fget(self)

    @param_array.setter
    def param_array(self, x):
        """as `Parameterized.param_array`, with the index column of Z held at the outputs the inducing inputs belong to"""
        x = np.array(x, dtype=np.float64).ravel()
        D = self.input_dim
        x[D - 1:self.Z.size:D] = self._Z_index
        SparseGP.param_array.fset(self, x)


class BayesianGPLVM(SparseGP):
    """Bayesian GP latent variable model (reference `GPy/models/bayesian_gplvm.py:12-100`): a `SparseGP` whose inputs are the
    parameters of q(X) = prod_n N(mean_n, diag variance_n), with the standard normal prior's KL term subtracted from the
    bound.  The flat parameter order is [X.mean, X.variance, Z, kernel, noise] (X is linked at index 0).  The bound, its
    gradients in every parameter -- the means and variances of q(X) included -- and prediction at certain or uncertain
    latent points run on the device through the uncertain-input path of `VarDTC`: the kernel is one `RBF` alone or summed
    with `White` parts (the reference's default, `RBF(input_dim, ARD=True)`, is covered).  `psi_lin_bias=True`
    (`VarDTC(psi_lin_bias=True)`): one `RBF` or `Linear` part with `Bias` and `White` parts -- `Linear(Q, ARD=True) + Bias + White`
    is Bayesian PCA; the flat parameter order is then [X.mean, X.variance, Z, variances, bias, white, noise]."""

    def __init__(self, Y, input_dim, X=None, X_variance=None, init="PCA", num_inducing=10, Z=None, kernel=None,
                 inference_method=None, likelihood=None, name="bayesian gplvm", device=0, mpi_comm=None, normalizer=None,
                 missing_data=False, stochastic=False, batchsize=1, Y_metadata=None, psi_lin_bias=False):
        for arg, value, default in (("mpi_comm", mpi_comm, None), ("normalizer", normalizer, None),
                                    ("missing_data", missing_data, False), ("stochastic", stochastic, False),
                                    ("batchsize", batchsize, 1)):
            if value is not default and value != default:
                raise NotImplementedError("BayesianGPLVM: %s = %r is not implemented on the MI355X path (the minibatch / MPI "
                                          "variant, missing data and normalizers are out of scope%s)"
                                          % (arg, value, "; BayesianGPLVMMiniBatch takes missing_data=True" if arg == "missing_data" else ""))
        Y = np.asarray(Y, dtype=np.float64)
        if X is None:
            from .util.initialization import initialize_latent
            X, fracs = initialize_latent(init, input_dim, Y)
        else:
            X = np.asarray(X, dtype=np.float64)
            fracs = np.ones(input_dim)
        if X.shape != (Y.shape[0], input_dim):
            raise ValueError("BayesianGPLVM: X must be %d x %d (one latent point per row of Y), got %r"
                             % (Y.shape[0], input_dim, X.shape))
        self.init = init
        if X_variance is None:
            X_variance = np.random.uniform(0, 0.1, X.shape)
        if Z is None:
            Z = np.random.permutation(X.copy())[:num_inducing]
        Z = np.asarray(Z, dtype=np.float64)
        if Z.ndim != 2 or Z.shape[1] != X.shape[1]:
            raise ValueError("BayesianGPLVM: Z must have %d columns, got shape %r" % (X.shape[1], Z.shape))
        if kernel is None:
            kernel = RBF(input_dim, lengthscale=1.0 / fracs, ARD=True, device=device)
        if likelihood is None:
            likelihood = Gaussian()
        self.variational_prior = NormalPrior()
        if psi_lin_bias:
            if inference_method is None:
                inference_method = VarDTC(device=device, psi_lin_bias=True)
            elif not getattr(inference_method, "psi_lin_bias", False):
                raise ValueError("BayesianGPLVM: psi_lin_bias=True, but the given inference_method was made without it; make it "
                                 "with VarDTC(psi_lin_bias=True) or leave inference_method out")
        super(BayesianGPLVM, self).__init__(NormalPosterior(X, X_variance), Y, Z, kernel, likelihood,
                                            inference_method=inference_method, name=name, device=device, Y_metadata=Y_metadata)
        self.link_parameter(self.X, index=0)

    def set_X_gradients(self, X, X_grad):
        """(dL/dmean, dL/dvariance) onto the two parameters of a `NormalPosterior` (reference `bayesian_gplvm.py:76-78`)"""
        X.mean.gradient, X.variance.gradient = X_grad

    def get_X_gradients(self, X):
        """the (mean, variance) gradients of a `NormalPosterior` (reference `bayesian_gplvm.py:80-82`)"""
        return X.mean.gradient, X.variance.gradient

    def _scatter_X(self, g):
        if g.shape == self.X.shape:
            return g
        full = np.zeros(self.X.shape)
        full[:, self.kern.active_dims] = g
        return full

    def parameters_changed(self):
        super(BayesianGPLVM, self).parameters_changed()
        self._log_marginal_likelihood = self._log_marginal_likelihood - self.variational_prior.KL_divergence(self.X)
        # gradients_qX_expectations of the reference (bayesian_gplvm.py:91-96): the device reduced them inside the fit
        fused = self.grad_dict["fused"]
        self.set_X_gradients(self.X, (self._scatter_X(fused["dmu"]), self._scatter_X(fused["dS"])))
        self.variational_prior.update_gradients_KL(self.X)
        self._Xgrad = self.X.gradient.copy()

    def _raw_predict(self, Xnew, full_cov=False, kern=None):
        """as `SparseGP._raw_predict`; a `NormalPosterior` Xnew is predicted at as a distribution (reference
        `posterior.py:249-269`)"""
        if not isinstance(Xnew, NormalPosterior):
            return super(BayesianGPLVM, self)._raw_predict(Xnew, full_cov=full_cov, kern=kern)
        return self.posterior._raw_predict(self.kern if kern is None else kern, Xnew, self.Z.values, full_cov=full_cov)

    def infer_newX(self, Y_new, optimize=True):
        raise NotImplementedError("BayesianGPLVM.infer_newX is not implemented on the MI355X path")


class BayesianGPLVMMiniBatch(BayesianGPLVM):
    """Bayesian GPLVM with missing data (reference `GPy/models/bayesian_gplvm_minibatch.py` on `sparse_gp_minibatch.py`): with
    `missing_data=True` NaNs in Y mark unobserved entries, output columns with the same observed rows are evaluated as one group
    and the bound is the sum of the groups' bounds minus the KL term (`kl_factr` = 1).  The whole loop is one device call
    (`VarDTC.inference(..., missing_data=True)`); the flat parameter order is [X.mean, X.variance, Z, kernel, noise].  With
    `missing_data=False` it is `BayesianGPLVM`'s evaluation.  The kernel is one `RBF` alone or summed with `White` parts.
    `predict(Xnew)` at certain or `NormalPosterior` points returns N* x Dy means and per-output variances.  Refused by name:
    `stochastic=True`, `batchsize != 1`, a normalizer, `X_variance=False` (the sparse GPLVM), non-Gaussian likelihoods, `infer_newX`.
    With NaNs in Y the PCA initialisation has nothing to decompose: pass X."""
    kl_factr = 1.0

    def __init__(self, Y, input_dim, X=None, X_variance=None, init="PCA", num_inducing=10, Z=None, kernel=None,
                 inference_method=None, likelihood=None, name="bayesian gplvm", normalizer=None, missing_data=False,
                 stochastic=False, batchsize=1, device=0):
        who = "BayesianGPLVMMiniBatch"
        if stochastic:
            raise NotImplementedError("%s: stochastic=True (minibatches over outputs) is not implemented on the MI355X path" % who)
        if batchsize != 1:
            raise NotImplementedError("%s: batchsize = %r is not implemented on the MI355X path (it belongs to stochastic=True)" % (who, batchsize))
        if normalizer is not None and normalizer is not False:
            raise NotImplementedError("%s: normalizer = %r is not implemented on the MI355X path" % (who, normalizer))
        if X_variance is False:
            raise NotImplementedError("%s: X_variance=False (the sparse GPLVM with certain latent points) is not implemented on the "
                                      "MI355X path" % who)
        if likelihood is not None and not isinstance(likelihood, Gaussian):
            raise NotImplementedError("%s: the likelihood %s is not implemented on the MI355X path; Gaussian is" % (who, type(likelihood).__name__))
        if inference_method is not None and (not isinstance(inference_method, VarDTC) or inference_method.psi_lin_bias):
            raise NotImplementedError("%s: the inference method must be a plain VarDTC() (psi_lin_bias and the reference's "
                                      "VarDTC_minibatch are not implemented with this class)" % who)
        Y = np.asarray(Y, dtype=np.float64)
        self.missing_data = bool(missing_data)
        if np.isnan(Y).any():
            if not self.missing_data:
                raise ValueError("%s: Y holds NaNs; pass missing_data=True" % who)
            if X is None:
                raise ValueError("%s: Y holds NaNs, which the PCA initialisation of the latent points cannot decompose; pass X" % who)
        super(BayesianGPLVMMiniBatch, self).__init__(Y, input_dim, X=X, X_variance=X_variance, init=init, num_inducing=num_inducing,
                                                     Z=Z, kernel=kernel, inference_method=inference_method, likelihood=likelihood,
                                                     name=name, device=device)

    def parameters_changed(self):
        if not self.missing_data:
            return super(BayesianGPLVMMiniBatch, self).parameters_changed()
        self.posterior, self._log_marginal_likelihood, self.grad_dict = self.inference_method.inference(
            self.kern, self.X, self.Z.values, self.likelihood, self.Y_normalized, Y_metadata=self.Y_metadata, missing_data=True)
        self.likelihood.update_gradients(self.grad_dict["dL_dthetaL"])
        fused = self.grad_dict["fused"]
        self.kern._install_fused(fused["dtheta"])
        self.Z.gradient = fused["dZ"] if fused["dZ"].shape == self.Z.shape else self._scatter_dZ(fused["dZ"])
        self._log_marginal_likelihood = self._log_marginal_likelihood - self.kl_factr * self.variational_prior.KL_divergence(self.X)
        self.set_X_gradients(self.X, (self._scatter_X(fused["dmu"]), self._scatter_X(fused["dS"])))
        self.variational_prior.update_gradients_KL(self.X)
        self._Xgrad = self.X.gradient.copy()

    def infer_newX(self, Y_new, optimize=True):
        raise NotImplementedError("BayesianGPLVMMiniBatch.infer_newX is not implemented on the MI355X path")


class SSGPLVM(SparseGP):
    """Spike-and-slab GP latent variable model (reference `GPy/models/ss_gplvm.py:177-270`): a `SparseGP` whose inputs are the
    parameters of q(x_nq) = gamma_nq N(mean_nq, variance_nq) + (1 - gamma_nq) delta_0, with the spike-and-slab prior's KL term
    subtracted from the bound; gamma switches a latent dimension off per point where ARD does so per model.  The flat
    parameter order is [X.mean, X.variance, X.binary_prob, Z, kernel, noise].  The bound and its gradients in every parameter
    run on the device through `VarDTC` (`mi355gp_vardtc_inference_ss`): the kernel is one `RBF` alone or summed with `White`
    parts.  Defaults as the reference's: gamma = 0.5 + 0.1 randn clipped to [1e-9, 1 - 1e-9], `RBF(input_dim,
    lengthscale=fracs, ARD=True)` -- `fracs`, where `BayesianGPLVM` takes `1 / fracs`: the reference differs between the two
    (`ss_gplvm.py:221`, `bayesian_gplvm.py:46`) and is followed -- `Gaussian()`, Z a permutation of X's rows, pi = 0.5.  The
    optimiser sees gamma through the reference's `Logistic(1e-10, 1 - 1e-10)` transform (`variational.py:181`)."""
    GAMMA_LOWER, GAMMA_UPPER = 1e-10, 1.0 - 1e-10
    _takes_spike_and_slab = True

    def __init__(self, Y, input_dim, X=None, X_variance=None, Gamma=None, init="PCA", num_inducing=10, Z=None, kernel=None,
                 inference_method=None, likelihood=None, name="Spike_and_Slab GPLVM", group_spike=False, IBP=False, SLVM=False,
                 alpha=2., beta=2., connM=None, tau=None, mpi_comm=None, pi=None, learnPi=False, normalizer=False, sharedX=False,
                 variational_prior=None, device=0, Y_metadata=None):
        for arg, value in (("group_spike", group_spike), ("IBP", IBP), ("SLVM", SLVM), ("learnPi", learnPi), ("sharedX", sharedX),
                           ("mpi_comm", mpi_comm), ("normalizer", normalizer), ("variational_prior", variational_prior)):
            if value is not None and value is not False:
                raise NotImplementedError("SSGPLVM: %s = %r is not implemented on the MI355X path (the IBP / SLVM / group-spike "
                                          "posteriors, learning pi, shared X, MPI and normalizers are out of scope)" % (arg, value))
        if inference_method is not None and not isinstance(inference_method, VarDTC):
            raise NotImplementedError("SSGPLVM: the inference method %s is not implemented on the MI355X path (the reference's "
                                      "default, VarDTC_minibatch, included); VarDTC is" % type(inference_method).__name__)
        Y = np.asarray(Y, dtype=np.float64)
        if X is None:
            from .util.initialization import initialize_latent
            X, fracs = initialize_latent(init, input_dim, Y)
        else:
            X = np.asarray(X, dtype=np.float64)
            fracs = np.ones(input_dim)
        if X.shape != (Y.shape[0], input_dim):
            raise ValueError("SSGPLVM: X must be %d x %d (one latent point per row of Y), got %r" % (Y.shape[0], input_dim, X.shape))
        self.init = init
        if X_variance is None:
            X_variance = np.random.uniform(0, 0.1, X.shape)
        if Gamma is None:
            Gamma = np.clip(0.5 + 0.1 * np.random.randn(X.shape[0], input_dim), 1e-9, 1.0 - 1e-9)
        if Z is None:
            Z = np.random.permutation(X.copy())[:num_inducing]
        Z = np.asarray(Z, dtype=np.float64)
        if Z.ndim != 2 or Z.shape[1] != X.shape[1]:
            raise ValueError("SSGPLVM: Z must have %d columns, got shape %r" % (X.shape[1], Z.shape))
        if kernel is None:
            kernel = RBF(input_dim, lengthscale=fracs, ARD=True, device=device)
        if any(isinstance(k, Linear) for k in kernel.leaves()):
            raise NotImplementedError("SSGPLVM: a Linear kernel needs the spike-and-slab Linear statistics (sslinear_psi_comp), "
                                      "which are not implemented on the MI355X path; one RBF kernel and White parts are")
        if likelihood is None:
            likelihood = Gaussian()
        self.variational_prior = SpikeAndSlabPrior(pi=0.5 if pi is None else pi)
        super(SSGPLVM, self).__init__(SpikeAndSlabPosterior(X, X_variance, Gamma), Y, Z, kernel, likelihood,
                                      inference_method=inference_method, name=name, device=device, Y_metadata=Y_metadata)
        self.link_parameter(self.X, index=0)

    def set_X_gradients(self, X, X_grad):
        """(reference `ss_gplvm.py:245-247`)"""
        X.mean.gradient, X.variance.gradient, X.binary_prob.gradient = X_grad

    def get_X_gradients(self, X):
        """(reference `ss_gplvm.py:249-251`)"""
        return X.mean.gradient, X.variance.gradient, X.binary_prob.gradient

    def _scatter_X(self, g):
        if g.shape == self.X.shape:
            return g
        full = np.zeros(self.X.shape)
        full[:, self.kern.active_dims] = g
        return full

    def parameters_changed(self):
        super(SSGPLVM, self).parameters_changed()
        self._log_marginal_likelihood = self._log_marginal_likelihood - self.variational_prior.KL_divergence(self.X)
        # gradients_qX_expectations of the reference (ss_gplvm.py:266): the device reduced them inside the fit
        fused = self.grad_dict["fused"]
        self.set_X_gradients(self.X, tuple(self._scatter_X(fused[k]) for k in ("dmu", "dS", "dgamma")))
        self.variational_prior.update_gradients_KL(self.X)

    # ---- the optimiser's view: as SparseGP's, with gamma through Logistic(1e-10, 1 - 1e-10) (paramz transformations.Logistic) ----
    def _logistic(self):
        return np.concatenate([np.full(p.size, p is self.X.binary_prob) for p in self.flattened_parameters()])

    @property
    def optimizer_array(self):
        x, lg, p = SparseGP.optimizer_array.fget(self), self._logistic(), self.param_array
        lo, hi = self.GAMMA_LOWER, self.GAMMA_UPPER
        g = np.clip(np.where(lg, p, 0.5), lo + 1e-10 * (hi - lo), hi - 1e-10 * (hi - lo))
        return np.where(lg, np.log((g - lo) / (hi - g)), x)

    @optimizer_array.setter
    def optimizer_array(self, x):
        x = np.asarray(x, dtype=np.float64)
        pos, lg = self._positive(), self._logistic()
        lo, hi = self.GAMMA_LOWER, self.GAMMA_UPPER
        g = lo + (hi - lo) / (1.0 + np.exp(-np.where(lg, x, 0.0)))
        self.param_array = np.where(lg, g, np.where(pos, np.exp(np.where(pos, x, 0.0)), x))

    def _grads(self, x):
        g, lg, p = super(SSGPLVM, self)._grads(x), self._logistic(), self.param_array
        lo, hi = self.GAMMA_LOWER, self.GAMMA_UPPER
        return np.where(lg, g * (p - lo) * (hi - p) / (hi - lo), g)

    def input_sensitivity(self):
        """(reference `ss_gplvm.py:272-276`)"""
        return self.kern.input_sensitivity() if getattr(self.kern, "ARD", False) else self.variational_prior.pi

    def _raw_predict(self, Xnew, full_cov=False, kern=None):
        """as `SparseGP._raw_predict`; a `NormalPosterior` Xnew is predicted at as a distribution (the Woodbury pair does not care
        how it was made); a `SpikeAndSlabPosterior` Xnew is refused"""
        if not isinstance(Xnew, (NormalPosterior, SpikeAndSlabPosterior)):
            return super(SSGPLVM, self)._raw_predict(Xnew, full_cov=full_cov, kern=kern)
        return self.posterior._raw_predict(self.kern if kern is None else kern, Xnew, self.Z.values, full_cov=full_cov)

    def sample_W(self, nSamples, raw_samples=False):
        raise NotImplementedError("SSGPLVM.sample_W needs a Linear kernel, whose spike-and-slab statistics (sslinear_psi_comp) are "
                                  "not implemented on the MI355X path")

    def infer_newX(self, Y_new, optimize=True):
        raise NotImplementedError("SSGPLVM.infer_newX is not implemented on the MI355X path")
