"""Stochastic variational GP (SVGP; Hensman, Fusi and Lawrence 2013; Hensman, Matthews and Ghahramani 2015) backed by
libmi355gp.so: the sparse method for data sets optimised in minibatches and for non-Gaussian likelihoods (reference
`GPy/inference/latent_function_inference/svgp.py:10-121`, `GPy/core/svgp.py:11-105`).

`SVGP.inference(q_u_mean, q_u_chol, kern, X, Z, likelihood, Y, ...)` returns `(posterior, log_marginal, grad_dict)` with the
reference's keys.  One evaluation is a two-call session on the sparse device context around the likelihood's quadrature, which
stays on the host (O(N L)):

    forward (`mi355gp_svgp_forward`)  ->  likelihood.variational_expectations  ->  times batch_scale  ->  backward

The N x M matrix `dL_dKmn` is never resident as a whole: the kernel and inducing-input gradients that `core/svgp.py:57-65`
derives from `dL_dKmm`, `dL_dKmn` and `dL_dKdiag` are reduced on the device and travel in `grad_dict['fused']`, the form
`SparseGP.parameters_changed` installs.  Kernels: what the sparse path takes (stationary kinds, White, Bias, sums, products).
Not covered: a mean function, uncertain inputs, `KL_scale != 1`, natural gradients, a row-sharded context."""
import numpy as np

from . import _lib
from .lazy import LazyArray, freeze
from .param import Param
from .sparse import SessionPosterior, SparseGP, SparseSession, sparse_path_kernel_check
from .util import choleskies
from .variational import NormalPosterior, refuse_spike_and_slab


class SVGPPosterior(SessionPosterior):
    """`Posterior(mean=q_u_mean, cov=S.T, K=Kmm, prior_mean=0)` of the reference (`svgp.py:121`, `posterior.py:79-107,176-209`):
    woodbury_vector = Kmm^-1 m and woodbury_inv[:, :, d] = Kmm^-1 - Kmm^-1 S_d Kmm^-1 stay on the device and prediction
    (`posterior.py:220-248`) runs there (C-ABI `mi355gp_svgp_predict`) while the posterior is the context's latest result."""

    def __init__(self, mean, chol, device):
        self.mean, self._chol, self._device = mean, chol, device
        self._wv = self._winv = None

    def _fetch(self, want_inv):
        if self._wv is None or (want_inv and self._winv is None):
            if not self._live():
                raise RuntimeError(LazyArray.stale)
            self._wv, wi = self._device["ctx"].svgp_woodbury(want_inv=want_inv)
            if wi is not None:
                self._winv = wi

    @property
    def covariance(self):
        """S, M x M x L (the reference's `cov=S.T` of a D x M x M array of symmetric matrices)"""
        return np.dstack([np.dot(L, L.T) for L in self._chol])

    @property
    def woodbury_vector(self):
        self._fetch(False)
        return self._wv

    @property
    def woodbury_inv(self):
        self._fetch(True)
        return self._winv

    def __getstate__(self):
        if self._live():
            self._fetch(True)
        d = dict(self.__dict__)
        d["_device"] = None
        return d

    def _raw_predict(self, kern, Xnew, pred_var, full_cov=False):
        if self._live(kern):
            return self._device["ctx"].svgp_predict(kern.part_specs(), kern._slice_X(Xnew), full_cov=full_cov)
        Kx = kern.K(pred_var, Xnew)                                   # (M, N*): foreign kernel / stale device state
        wv, Wi = self.woodbury_vector, self.woodbury_inv
        mu = np.dot(Kx.T, wv)
        if full_cov:
            Kxx = kern.K(Xnew)
            return mu, np.dstack([Kxx - np.dot(Kx.T, np.dot(Wi[:, :, i], Kx)) for i in range(Wi.shape[2])])
        Kxx = kern.Kdiag(Xnew)
        var = np.stack([Kxx - np.sum(np.dot(Wi[:, :, i].T, Kx) * Kx, 0) for i in range(Wi.shape[2])], axis=1)
        return mu, np.clip(var, 1e-15, np.inf)                        # posterior.py:248


class SVGP(SparseSession):
    """The inference class (reference `svgp.py:8-121`)."""

    def to_dict(self):
        return {"class": "GPy.inference.latent_function_inference.svgp.SVGP"}

    def inference(self, q_u_mean, q_u_chol, kern, X, Z, likelihood, Y, mean_function=None, Y_metadata=None, KL_scale=1.0,
                  batch_scale=1.0):
        if mean_function is not None:
            raise NotImplementedError("SVGP on the MI355X path has no mean function (svgp.py:29-31,62-74,103-107 are not built)")
        refuse_spike_and_slab(X, "SVGP")
        if isinstance(X, NormalPosterior):
            raise NotImplementedError("SVGP on the MI355X path takes certain inputs; uncertain inputs are covered by VarDTC")
        if KL_scale != 1.0:
            raise NotImplementedError("KL_scale = %r: SVGP on the MI355X path evaluates the bound with KL_scale = 1, as the "
                                      "reference's own model does (core/svgp.py:55)" % (KL_scale,))
        if not hasattr(likelihood, "variational_expectations"):
            raise NotImplementedError("the %s likelihood has no variational_expectations, which SVGP needs (svgp.py:77)"
                                      % type(likelihood).__name__)
        sparse_path_kernel_check(kern, self.linear)
        self._refuse_sharded("SVGP is not supported by a row-sharded sparse context")
        q_u_mean = _lib.f64(np.asarray(q_u_mean))
        Y = np.asarray(Y, dtype=np.float64)
        num_inducing, num_outputs = q_u_mean.shape
        if not 1 <= num_outputs <= 16:
            raise NotImplementedError("%d latent functions: the MI355X SVGP path takes between 1 and 16" % num_outputs)
        L = choleskies.flat_to_triang(np.asarray(q_u_chol, dtype=np.float64))                  # svgp.py:16
        assert L.shape == (num_outputs, num_inducing, num_inducing), "q_u_chol does not match q_u_mean"
        Xs, Zs = kern._slice_X(X), kern._slice_X(Z)
        assert Zs.shape[0] == num_inducing, "q_u_mean does not match Z"
        self._ensure(Xs, _lib.f64(Y))
        specs = kern.part_specs()
        fw = self._run(kern, lambda extra: self._ctx.svgp_forward(specs, Zs, q_u_mean, L, extra_jitter=extra,
                                                                  want_stage_ms=self.collect_stage_ms), Z)   # Kmm (svgp.py:40)
        # quadrature for the likelihood (svgp.py:77), rescaled if working on a batch (:80-82)
        F, dF_dmu, dF_dv, dF_dthetaL = likelihood.variational_expectations(Y, fw["mu"], fw["v"], Y_metadata=Y_metadata)
        F, dF_dmu, dF_dv = F * batch_scale, dF_dmu * batch_scale, dF_dv * batch_scale
        if dF_dthetaL is not None:
            dF_dthetaL = dF_dthetaL.sum(1).sum(1) * batch_scale
        bw = self._ctx.svgp_backward(dF_dmu, dF_dv, want_stage_ms=self.collect_stage_ms)
        if self.collect_stage_ms:
            self.last_stage_ms = {"forward": fw.get("stage_ms"), "backward": bw.get("stage_ms")}
        log_marginal = F.sum() - fw["KL"]                                                       # svgp.py:111
        post = SVGPPosterior(q_u_mean, L, self._device_dict(kern))
        grad_dict = {"dL_dKdiag": dF_dv.sum(1), "dL_dm": bw["dL_dm"], "dL_dchol": choleskies.triang_to_flat(bw["dL_dchol"]),
                     "dL_dthetaL": dF_dthetaL, "fused": {"dtheta": bw["dtheta"], "dZ": bw["dZ"]},
                     "mu": fw["mu"], "v": fw["v"], "KL": fw["KL"]}
        return post, log_marginal, grad_dict


class _MiniSlices(object):
    """Minibatch slices: contiguous slices of `batchsize` rows (the last one of an epoch may be shorter) in an order that is
    shuffled anew for every epoch by a seeded generator.  (The reference draws them with `climin.util.draw_mini_slices`,
    `core/svgp.py:33-36`; climin is not a dependency here.)"""

    def __init__(self, n, batchsize, seed):
        self.n, self.batchsize = int(n), int(batchsize)
        assert 1 <= self.batchsize, "batchsize must be positive"
        self.rng = np.random.default_rng(seed)
        self.order = []

    def __iter__(self):
        return self

    def __next__(self):
        if not self.order:
            starts = np.arange(0, self.n, self.batchsize)
            self.order = list(starts[self.rng.permutation(starts.size)])
        s = int(self.order.pop(0))
        return slice(s, min(s + self.batchsize, self.n))


class SVGPModel(SparseGP):
    """`GPy.core.SVGP` (reference `core/svgp.py:11-105`) without natural gradients: q(u_d) = N(m_d, L_d L_d^T) with the
    lower-triangular factors as parameters.  Flat parameter order: Z, kern, likelihood, q_u_chol, q_u_mean (`core/svgp.py:48-52`
    link the last two after `SparseGP.__init__`); q_u_chol and q_u_mean are unconstrained, identity factors and zeros at first.

    batchsize: None evaluates the bound on all data; otherwise every `new_batch()` / `stochastic_grad()` takes the next
    minibatch: contiguous slices of `batchsize` rows in an order reshuffled every epoch by `numpy.random.default_rng(seed)`
    (the reference uses climin's slicer; this package does not depend on climin).  `batch_scale` = N_all / N_batch.
    `optimize()` is the inherited full-batch L-BFGS-B; a stochastic optimiser is not part of the package."""

    def __init__(self, X, Y, Z, kernel, likelihood, batchsize=None, seed=None, device=0, name="SVGP", Y_metadata=None,
                 num_latent_functions=None, mean_function=None, linear=False):
        if mean_function is not None:
            raise NotImplementedError("SVGP on the MI355X path has no mean function")
        refuse_spike_and_slab(X, "SVGP")
        if isinstance(X, NormalPosterior):
            raise NotImplementedError("SVGP on the MI355X path takes certain inputs")
        self.batchsize = batchsize
        self.X_all, self.Y_all = freeze(X), freeze(Y)
        num_inducing = np.shape(Z)[0]
        L = self.Y_all.shape[1] if num_latent_functions is None else int(num_latent_functions)
        # (created before SparseGP.__init__ evaluates the model once; linked after it, as the reference links them)
        self.chol = Param("q_u_chol", choleskies.triang_to_flat(np.tile(np.eye(num_inducing)[None, :, :], (L, 1, 1))),
                          positive=False)
        self.m = Param("q_u_mean", np.zeros((num_inducing, L)), positive=False)
        if batchsize is None:
            X_batch, Y_batch = self.X_all, self.Y_all
        else:
            self.slicer = _MiniSlices(self.X_all.shape[0], batchsize, seed)
            X_batch, Y_batch = self.new_batch()
        super(SVGPModel, self).__init__(X_batch, Y_batch, Z, kernel, likelihood, inference_method=SVGP(device=device, linear=linear), name=name,
                                        device=device, Y_metadata=Y_metadata)
        self.link_parameter(self.chol)
        self.link_parameter(self.m)

    q_u_chol = property(lambda self: self.chol)
    q_u_mean = property(lambda self: self.m)

    def parameters_changed(self):
        self.posterior, self._log_marginal_likelihood, self.grad_dict = self.inference_method.inference(
            self.m.values, self.chol.values, self.kern, self.X, self.Z.values, self.likelihood, self.Y, None, self.Y_metadata,
            KL_scale=1.0, batch_scale=float(self.X_all.shape[0]) / float(self.X.shape[0]))
        # the kernel and inducing-input gradients of core/svgp.py:57-65 were reduced on the device
        fused = self.grad_dict["fused"]
        self.kern._install_fused(fused["dtheta"])
        self.Z.gradient = fused["dZ"] if fused["dZ"].shape == self.Z.shape else self._scatter_dZ(fused["dZ"])
        if self.grad_dict["dL_dthetaL"] is not None:
            self.likelihood.update_gradients(self.grad_dict["dL_dthetaL"])
        self.m.gradient = self.grad_dict["dL_dm"]
        self.chol.gradient = self.grad_dict["dL_dchol"]

    def set_data(self, X, Y):
        """Set the data without calling parameters_changed (reference `core/svgp.py:80-86`)"""
        assert np.shape(X)[1] == self.Z.shape[1]
        self.X, self.Y = freeze(X), freeze(Y)
        self.Y_normalized = self.Y
        self.num_data = self.X.shape[0]

    def new_batch(self):
        """the next minibatch (X, Y) of the complete data (reference `core/svgp.py:88-93`)"""
        i = next(self.slicer)
        return self.X_all[i], self.Y_all[i]

    def stochastic_grad(self, parameters):
        """the gradient at `parameters` (an `optimizer_array`) on the next minibatch (reference `core/svgp.py:95-97`)"""
        self.set_data(*self.new_batch())
        return self._grads(parameters)
