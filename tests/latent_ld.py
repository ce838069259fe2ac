"""Long-double restatement of what the latent-input gradient pass (gpy_amd/csrc/latent.hip) computes, on top of kern_ld: with
G = 0.5 (alpha alpha^T - Dy W), dL/dX = kern.gradients_X(G, X) (stationary.py:330-358, X2 = None: the weights G + G^T) and
dL/dtheta = sum_ij G_ij dK_ij/dtheta in link order.  Every function takes the working type `dt` (long double or float64: the
fp64 evaluation measures how far double precision itself lies from the truth on that input)."""
import numpy as np

import kern_ld as KL

LD, EPS64 = KL.LD, KL.EPS64


def spec(kind, ard, theta, dims):
    """one part in kern_ld's form; dims: its active columns"""
    return (kind, int(ard), np.asarray(theta, dtype=np.float64), list(dims), 0)


def dL_dK(W, alpha, dt=LD):
    a, W = np.asarray(alpha, dtype=dt), np.asarray(W, dtype=dt)
    return (KL.matmul(a, a.T) - a.shape[1] * W) / 2


def grad(specs, X, W, alpha, dt=LD):
    """(dL/dX (N x D), dL/dtheta in link order) for ANY symmetric W in the place of Ky^-1"""
    G = dL_dK(W, alpha, dt)
    lv = KL.leaves(specs, X, None, dt)
    return KL.gradients_X(specs, G, X, None, dt, lv)[0], KL.dtheta(specs, G, X, None, dt, lv)[0]


def dtheta_from_records(kind, ard, theta, D, rec):
    """the host finish of one stationary part's two reduction records (csrc/parts.h, part_dtheta)"""
    out = [rec[0] / theta[0]]
    out += [-rec[2 + q] / theta[1 + q] for q in range(D)] if ard else [-rec[1] / theta[1]]
    if kind == "ratquad":
        out.append(rec[34])
    return np.array(out)


def evaluate(specs, X, Y, noise, dt=LD):
    """the whole evaluation: dict(lml, alpha, dtheta, dnoise, dX, Ki) from kern_ld.exact"""
    ex = KL.exact(specs, X, Y, noise, dt=dt, max_n=X.shape[0])
    ex["dX"] = KL.gradients_X(specs, ex["dL_dK"], X, None, dt)[0]
    return ex


def tol(ref_ld, ref_64):
    """the rule of tests/test_gpu_psi_gh.py: max(16 d, 64 eps64) of max |value|, d = the distance of the fp64 restatement"""
    scale = np.max(np.abs(ref_ld))
    d = np.max(np.abs(np.asarray(ref_64, dtype=LD) - ref_ld)) / scale if scale > 0 else 0
    return float(max(16 * d, 64 * EPS64) * scale)


def worst(got, ref_ld):
    return float(np.max(np.abs(np.asarray(got, dtype=LD) - ref_ld)))
