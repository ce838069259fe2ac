"""Per-call host overhead of the inference classes, on the CPU: `inference()` of VarDTC (certain inputs), PEP, SVGP and
ExactGaussianInference over a stand-in context that answers at once with zero arrays of the right shapes, so that what is timed
is the Python between the caller and the C-ABI -- data identity checks, the jitter ladder, the posterior and its lazy views.

    python tools/host_overhead.py [--calls 3000] [--n 129] [--m 33]      one JSON line: microseconds per call, per class

To compare two versions of the package, run the copy of this file in each tree in turn, several times each, interleaved.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
D = 3


class ZeroContext(object):
    """Stands for `_lib.Context` and `_lib.SparseContext`: every evaluation succeeds (info = 0) with zeros."""
    FETCH_DLDKMM, FETCH_WOODBURY_INV, FETCH_LM, FETCH_KMM, FETCH_PSI2, FETCH_DLDPSI2_BETA = 0, 1, 2, 3, 4, 5
    sharded = False

    def __init__(self, device=0):
        self.N = self.D = self.Dy = self.M = 0

    @staticmethod
    def _ntheta(specs):
        return sum(np.asarray(s[2]).size for s in specs)

    def set_data(self, X, Y):
        (self.N, self.D), self.Dy = X.shape, Y.shape[1]

    def set_targets(self, R):
        pass

    def set_input_variance(self, S):
        pass

    def set_inputs(self, X, S=None):
        pass

    def _fit(self, specs, Z, cols, **more):
        self.M = Z.shape[0]
        return 0, dict(lml=-1.0, dnoise=0.5, dtheta=np.zeros(self._ntheta(specs)), dZ=np.zeros(Z.shape),
                       woodbury_vector=np.zeros((self.M, cols)), **more)

    def vardtc_sum(self, specs, Z, noise, extra_jitter=0.0, want_dL_dm=False, want_stage_ms=False):
        rc, r = self._fit(specs, Z, self.Dy, dL_dm=None)
        if np.size(noise) > 1:
            r["dnoise"] = np.zeros(self.N)
        return rc, r

    def vardtc_uncertain(self, specs, Z, noise, extra_jitter=0.0, want_dmu_dS=True, want_stage_ms=False):
        return self._fit(specs, Z, self.Dy, dmu=np.zeros((self.N, self.D)), dS=np.zeros((self.N, self.D)))

    def pep(self, specs, Z, noise_variance, alpha, jitter, want_stage_ms=False):
        return self._fit(specs, Z, 1, dL_dR=np.zeros(self.N))

    def svgp_forward(self, specs, Z, q_mean, q_chol, extra_jitter=0.0, want_stage_ms=False):
        self.M, self.L, self._nth = Z.shape[0], q_mean.shape[1], self._ntheta(specs)
        return 0, dict(mu=np.zeros((self.N, self.L)), v=np.ones((self.N, self.L)), KL=0.0, logdet_Kmm=0.0, logdet_S=np.zeros(self.L))

    def svgp_backward(self, dF_dmu, dF_dv, want_stage_ms=False):
        return dict(dtheta=np.zeros(self._nth), dZ=np.zeros((self.M, self.D)), dL_dm=np.zeros((self.M, self.L)),
                    dL_dchol=np.zeros((self.L, self.M, self.M)))

    def svgp_woodbury(self, want_inv=True):
        return np.zeros((self.M, self.L)), (np.zeros((self.M, self.M, self.L)) if want_inv else None)

    def svgp_predict(self, specs, Xnew, full_cov=False, want_var=True):
        return np.zeros((Xnew.shape[0], self.L)), np.ones((Xnew.shape[0], self.L))

    def exact_inference_sum(self, specs, noise, jitter=1e-8, extra_jitter=0.0, want_alpha=True, want_diag=False, want_stage_ms=False):
        return 0, dict(lml=-1.0, dnoise=0.5, alpha=np.zeros((self.N, self.Dy)), diag_dL_dK=np.zeros(self.N) if want_diag else None,
                       dtheta=np.zeros(self._ntheta(specs)))

    def predict(self, specs, Xnew, full_cov=False, want_var=True):
        return np.zeros((Xnew.shape[0], self.Dy)), np.ones((Xnew.shape[0], 1))

    predict_sum = predict

    def predict_uncertain(self, specs, mu_new, S_new, want_var=True):
        return np.zeros((mu_new.shape[0], self.Dy)), np.ones((mu_new.shape[0], self.Dy))

    def fetch(self, which, fortran_order=False):
        n = self.M or self.N
        return np.zeros((n, n))

    def fetch_dL_dKnm(self, row0, nrows):
        return np.zeros((nrows, self.M))


def measure(calls, N, M):
    import gpy_amd as G
    from gpy_amd import _lib
    from gpy_amd.lazy import freeze
    from gpy_amd.svgp import SVGP as SVGPInference
    from gpy_amd.util import choleskies
    _lib.Context = _lib.SparseContext = ZeroContext
    rng = np.random.default_rng(N)
    X, Y, Z = freeze(rng.uniform(0.0, 1.0, (N, D))), freeze(rng.standard_normal((N, 1))), rng.uniform(0.0, 1.0, (M, D))
    kern, lik = G.RBF(D, variance=1.3, lengthscale=[0.3, 0.4, 0.5], ARD=True) + G.White(D, variance=0.05), G.Gaussian(variance=0.04)
    q_mean, q_chol = np.zeros((M, 1)), choleskies.triang_to_flat(np.eye(M)[None])
    vardtc, pep, svgp, exact = G.VarDTC(), G.PEP(0.5), SVGPInference(), G.ExactGaussianInference()
    cases = {"VarDTC": lambda: vardtc.inference(kern, X, Z, lik, Y),
             "PEP": lambda: pep.inference(kern, X, Z, lik, Y),
             "SVGP": lambda: svgp.inference(q_mean, q_chol, kern, X, Z, lik, Y),
             "ExactGaussianInference": lambda: exact.inference(kern, X, lik, Y)}
    res = {}
    for name, call in cases.items():
        for _ in range(200):
            call()
        t0 = time.perf_counter()
        for _ in range(calls):
            call()
        res[name] = round((time.perf_counter() - t0) / calls * 1e6, 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3000)
    ap.add_argument("--n", type=int, default=129)
    ap.add_argument("--m", type=int, default=33)
    a = ap.parse_args()
    print(json.dumps({"calls": a.calls, "N": a.n, "M": a.m, "us_per_call": measure(a.calls, a.n, a.m)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
