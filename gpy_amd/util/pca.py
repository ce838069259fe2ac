"""Principal component analysis for the latent initialisation (reference `GPy/util/pca.py:22-78`, without the plotting):
the data are centred and scaled per column, the eigen-decomposition is the primal one (D x D) when N >= D and the dual one
(N x N) otherwise.  Host NumPy: O(N D min(N, D)) once per model."""
import numpy as np


class PCA(object):
    def __init__(self, X):
        self.mu = self.sigma = None
        Xc = self.center(X)
        n, d = Xc.shape
        if n >= d:                                                  # primal: eigenvectors of X^T X
            vals, vecs = np.linalg.eigh(np.dot(Xc.T, Xc))
        else:                                                       # dual: those of X X^T, mapped back through X^T
            dvals, dvecs = np.linalg.eigh(np.dot(Xc, Xc.T))
            keep = np.argsort(np.abs(dvals))[-d:]
            vals = dvals[keep]
            vecs = np.dot(Xc.T, dvecs[:, keep]) / np.sqrt(n * np.abs(vals))
            vecs = vecs / np.sqrt(np.sum(vecs * vecs, 0))
        order = np.argsort(vals)[::-1]
        self.eigvals, self.eigvectors = vals[order], vecs[:, order]
        self.fracs = self.eigvals / self.eigvals.sum()
        self.Q = self.eigvals.shape[0]

    def center(self, X):
        """(X - mean) / std per column with the mean and std of the first call; NaNs are replaced by the column mean"""
        X = np.array(X, dtype=np.float64)
        nan = np.isnan(X)
        if self.mu is None:
            masked = np.ma.masked_array(X, nan)
            self.mu = np.asarray(masked.mean(0).filled(0.0))
            self.sigma = np.asarray(masked.std(0).filled(0.0))
        X[nan] = np.broadcast_to(self.mu, X.shape)[nan]
        return (X - self.mu) / np.where(self.sigma == 0, 1e-30, self.sigma)

    def project(self, X, Q=None):
        """X in the space of the Q leading principal directions"""
        Q = self.Q if Q is None else Q
        if Q > np.shape(X)[1]:
            raise IndexError("PCA.project: %d components asked of %d-dimensional data" % (Q, np.shape(X)[1]))
        return np.dot(self.center(X), self.eigvectors[:, :Q])
