"""Helper, no test: Kronecker GP regression with two arbitrary kernels (gpy_amd/kgpr.py) restated twice.

`restate` / `restate_predict`: the reference's algebra (`GPy/models/gp_kronecker_gaussian_regression.py:53-117`) in NumPy with
`np.linalg.eigh`, in the `dtype` asked for.  `dense` : the yardstick in long double from Ky = kron(K2, K1) + sigma^2 I of size
N1 N2 by Cholesky (tests/kron_ld.py) -- no eigendecomposition in it.  Both take the factor MATRICES, as the device session does.
`rbf`, `matern32`: K and dK/d(variance, lengthscale) of the two kernels the reference's fixtures use, for 1-D inputs."""
import numpy as np

from kron_ld import LD, cholesky, solve_lower, solve_upper_T


def restate(K1, K2, Y, noise, dtype=np.float64):
    K1, K2, Y, noise = np.asarray(K1, dtype), np.asarray(K2, dtype), np.asarray(Y, dtype), dtype(noise)
    N1, N2 = Y.shape
    S1, U1 = np.linalg.eigh(K1)
    S2, U2 = np.linalg.eigh(K2)
    W = np.kron(S2, S1) + noise
    Y_ = U1.T.dot(Y).dot(U2)
    Wi = 1 / W
    Ytilde = Y_.flatten(order="F") * Wi
    lml = -0.5 * N1 * N2 * np.log(2 * np.pi) - 0.5 * np.sum(np.log(W)) - 0.5 * np.dot(Y_.flatten(order="F"), Ytilde)
    Yt = Ytilde.reshape(N1, N2, order="F")
    tmp = U1.dot(Yt)
    dK1 = .5 * (tmp * S2).dot(tmp.T)
    tmp = U2.dot(Yt.T)
    dK2 = .5 * (tmp * S1).dot(tmp.T)
    Wr = Wi.reshape(N1, N2, order="F")
    dK1 += -0.5 * (U1 * np.dot(Wr, S2)).dot(U1.T)
    dK2 += -0.5 * (U2 * np.dot(Wr.T, S1)).dot(U2.T)
    return dict(lml=lml, dsig=-0.5 * Wi.sum() + 0.5 * np.sum(np.square(Ytilde)), dK1=dK1, dK2=dK2, Wi=Wi, Ytilde=Ytilde, U1=U1, U2=U2,
                noise=noise)


def restate_predict(r, k1xf, k2xf, k1xx, k2xx):
    dt = r["U1"].dtype
    A, B = np.asarray(k1xf, dt).dot(r["U1"]), np.asarray(k2xf, dt).dot(r["U2"])
    N1, N2 = A.shape[1], B.shape[1]
    mu = A.dot(r["Ytilde"].reshape(N1, N2, order="F")).dot(B.T).flatten(order="F")
    BA = np.kron(B, A)
    return mu, np.kron(np.asarray(k2xx, dt), np.asarray(k1xx, dt)) - np.sum(BA ** 2 * r["Wi"], 1) + r["noise"]


def dense(K1, K2, Y, noise, k1xf, k2xf, k1xx, k2xx):
    """dict(lml, dsig, dK1, dK2, mu, var) in long double from the dense N1 N2 x N1 N2 covariance"""
    K1, K2, Y = (np.asarray(a, LD) for a in (K1, K2, Y))
    N1, N2 = Y.shape
    n = N1 * N2
    Ky = np.kron(K2, K1) + LD(noise) * np.eye(n, dtype=LD)
    L = cholesky(Ky)
    y = Y.flatten(order="F")
    alpha = solve_upper_T(L, solve_lower(L, y[:, None]))[:, 0]
    Li = solve_lower(L, np.eye(n, dtype=LD))
    Kyi = np.dot(Li.T, Li)
    pi = LD(4) * np.arctan(LD(1))
    lml = -LD(n) / 2 * np.log(2 * pi) - np.sum(np.log(np.diag(L))) - np.dot(y, alpha) / 2
    G = ((np.outer(alpha, alpha) - Kyi) / 2).reshape(N2, N1, N2, N1)          # flat index i + N1 j: [j, i, j', i']
    Ks = np.kron(np.asarray(k2xf, LD), np.asarray(k1xf, LD))
    V = solve_lower(L, Ks.T)
    return dict(lml=lml, dsig=(np.dot(alpha, alpha) - np.trace(Kyi)) / 2, dK1=np.einsum("jakb,jk->ab", G, K2),
                dK2=np.einsum("jakb,ab->jk", G, K1), mu=np.dot(Ks, alpha),
                var=np.kron(np.asarray(k2xx, LD), np.asarray(k1xx, LD)) - np.sum(V * V, 0) + LD(noise))


def rel(got, ref):
    """max |got - ref| / max |ref| in long double"""
    got, ref = np.asarray(got, LD), np.asarray(ref, LD)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), np.finfo(np.float64).tiny))


def _r(X, X2, ls):
    X2 = X if X2 is None else X2
    return np.abs(X[:, :1] - X2[:, :1].T) / ls


def rbf(X, var, ls, X2=None):
    """(K, dK/dvariance, dK/dlengthscale)"""
    r = _r(X, X2, ls)
    E = np.exp(-0.5 * r * r)
    return var * E, E, var * E * r * r / ls


def matern32(X, var, ls, X2=None):
    r = _r(X, X2, ls)
    E = np.exp(-np.sqrt(3.) * r)
    return var * (1 + np.sqrt(3.) * r) * E, (1 + np.sqrt(3.) * r) * E, var * 3 * r * r * E / ls
