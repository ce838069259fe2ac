"""FITC and power-EP (PEP) sparse inference for a Gaussian likelihood, backed by libmi355gp.so -- drop-in for
`GPy.inference.latent_function_inference.FITC` (reference `fitc.py:10-88`; Snelson and Ghahramani's fully independent training
conditional) and `GPy.inference.latent_function_inference.PEP` (reference `pep.py:8-93`; Bui, Yan and Turner, arXiv:1605.07066).
`PEP(alpha=1)` is FITC -- the reference's two `inference` methods are then the same arithmetic line for line -- and
`alpha -> 0` approaches `VarDTC`.  One device entry point, `mi355gp_pep_inference`, serves both classes.

    m = gpy_amd.core.SparseGP(X, Y, Z, kernel, gpy_amd.Gaussian(), inference_method=gpy_amd.FITC())

`inference(kern, X, Z, likelihood, Y, mean_function=None, Y_metadata=None)` returns `(posterior, log_marginal, grad_dict)`
with the reference's keys `dL_dKmm`, `dL_dKdiag`, `dL_dKnm`, `dL_dthetaL` (`pep.py:88`); the matrices are lazy device views as
`VarDTC`'s are, and `grad_dict['fused']` carries the kernel and inducing-input gradients that `SparseGP._update_gradients`
(reference `core/sparse_gp.py:108-119`) derives from them, reduced on the device.

Covered: what the sparse device context evaluates (`sparse_path_kernel_check`), certain inputs, ONE output column and ONE noise
variance.  Refused by name: a mean function (the reference asserts), per-point noise (the reference raises), a
`NormalPosterior` X, several output columns (the reference's `v.reshape(-1, 1)`) and a row-sharded context.
"""
import numpy as np

from . import _lib
from .lazy import LazyNM
from .sparse import SparseSession, noise_variances, sparse_path_kernel_check
from .variational import NormalPosterior, refuse_spike_and_slab


class PEP(SparseSession):
    const_jitter = 1e-6                                       # (pep.py:17, fitc.py:17; VarDTC's is 1e-8)

    def __init__(self, alpha, device=0, maxtries=5, linear=False):
        super(PEP, self).__init__(device=device, maxtries=maxtries, linear=linear)
        self.alpha = alpha

    def to_dict(self):
        return {"class": "GPy.inference.latent_function_inference.pep.PEP", "alpha": self.alpha}

    def _refusals(self, kern, X, likelihood, Y, mean_function, Y_metadata):
        """everything that is out of scope, by name, before a context exists; returns the noise variance"""
        name = type(self).__name__
        if mean_function is not None:                             # pep.py:24, fitc.py:22
            raise NotImplementedError("%s: inference with a mean function is not implemented (the reference asserts the same)" % name)
        refuse_spike_and_slab(X, name)
        if isinstance(X, NormalPosterior):
            raise NotImplementedError("%s: uncertain inputs (a NormalPosterior X) are not implemented; VarDTC covers them" % name)
        alpha = float(self.alpha)
        if not (0.0 < alpha <= 1.0):
            raise ValueError("%s: alpha = %r is outside (0, 1] (1 is FITC; VarDTC is the limit alpha -> 0)" % (name, self.alpha))
        sigma_n = noise_variances(likelihood, Y_metadata)
        if sigma_n.size > 1:                                      # pep.py:30-32, fitc.py:28-30
            raise NotImplementedError("%s: no hetero (per-point) noise with this implementation" % name)
        if np.ndim(Y) != 2 or np.shape(Y)[1] != 1:
            raise NotImplementedError("%s: %s output columns; one is covered (the reference's v.reshape(-1, 1))"
                                      % (name, np.shape(Y)[1] if np.ndim(Y) == 2 else "no"))
        sparse_path_kernel_check(kern, self.linear)
        self._refuse_sharded("%s: a row-sharded sparse context is not supported" % name)
        return float(sigma_n[0])

    def inference(self, kern, X, Z, likelihood, Y, mean_function=None, Y_metadata=None):
        s2 = self._refusals(kern, X, likelihood, Y, mean_function, Y_metadata)
        alpha = float(self.alpha)
        Xs, Zs = kern._slice_X(X), kern._slice_X(Z)
        R = _lib.f64(Y)
        self._ensure(Xs, R)
        specs = kern.part_specs()
        # the ladder's jitter comes on top of const_jitter (pep.py:40-41,50)
        r = self._run(kern, lambda extra: self._ctx.pep(specs, Zs, s2, alpha, self.const_jitter + extra,
                                                        want_stage_ms=self.collect_stage_ms), Z)
        M, N = Zs.shape[0], Xs.shape[0]
        post, dL_dKmm = self._posterior(kern, M, r["woodbury_vector"])                   # woodbury_inv = Kmmi - P (pep.py:91)
        grad_dict = {"dL_dKmm": dL_dKmm,
                     "dL_dKdiag": alpha * r["dL_dR"],                                                   # pep.py:88
                     "dL_dKnm": LazyNM(self, N, M),
                     # likelihood.exact_inference_gradients(dL_dR) + 0.5 (1 - alpha) / alpha N / sigma_n (pep.py:86-87)
                     "dL_dthetaL": r["dnoise"],
                     "fused": {"dtheta": r["dtheta"], "dZ": r["dZ"]}}
        return post, r["lml"], grad_dict


class FITC(PEP):
    """`GPy.inference.latent_function_inference.FITC` (reference `fitc.py:10-88`): `PEP` with alpha = 1."""

    def __init__(self, device=0, maxtries=5, linear=False):
        super(FITC, self).__init__(1.0, device=device, maxtries=maxtries, linear=linear)

    def to_dict(self):
        return {"class": "GPy.inference.latent_function_inference.fitc.FITC"}
