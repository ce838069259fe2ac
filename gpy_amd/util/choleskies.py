"""Packed lower-triangular factors as SVGP's `q_u_chol` stores them (reference `GPy/util/choleskies.py:23-52,82-83`).

The flat form has one column per latent function and the lower triangle row by row: flat[m (m + 1) / 2 + mm, d] = L[d, m, mm]
for mm <= m.  Host bookkeeping of O(L M^2) entries; nothing here runs on the device."""
import numpy as np


def safe_root(N):
    j = int(round(np.sqrt(N)))
    if j * j != N:
        raise ValueError("N is not square!")
    return j


def flat_to_triang(flat_mat):
    """(N, D) -> (D, M, M) lower-triangular, N = M (M + 1) / 2 (reference `choleskies.py:23-33`)"""
    flat_mat = np.asarray(flat_mat)
    N, D = flat_mat.shape
    M = (-1 + safe_root(8 * N + 1)) // 2
    ret = np.zeros((D, M, M), dtype=flat_mat.dtype)
    r, c = np.tril_indices(M)                  # row-major over the lower triangle: the reference's loop order
    ret[:, r, c] = flat_mat.T
    return ret


def triang_to_flat(L):
    """(D, M, M) -> (N, D): the lower triangles, row by row (reference `choleskies.py:41-52`)"""
    L = np.asarray(L)
    M = L.shape[-1]
    r, c = np.tril_indices(M)
    return np.ascontiguousarray(L[:, r, c].T)


def triang_to_cov(L):
    """(reference `choleskies.py:79-80`)"""
    return np.dstack([np.dot(L[:, :, i], L[:, :, i].T) for i in range(L.shape[-1])])


def multiple_dpotri(Ls):
    """(L_d L_d^T)^-1 for every d (reference `choleskies.py:82-83`, LAPACK dpotri on each factor)"""
    from scipy.linalg import lapack
    out = np.empty(np.shape(Ls))
    for i in range(out.shape[0]):
        Si, info = lapack.dpotri(np.asfortranarray(np.tril(Ls[i])), lower=1)
        if info != 0:
            Si = np.full(Si.shape, np.inf)
        out[i] = np.tril(Si) + np.tril(Si, -1).T
    return out
