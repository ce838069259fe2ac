"""Restatement of the Kronecker grid path (gpy_amd/kron.py, csrc/kron.hip) in a chosen working type, float64 or long double, for
the tests to judge the device and the host classes by.  No device, no gpy_amd import.

Two restatements:
  * `evaluate` / `predict`: the structured algebra of GPy's `GaussianGridInference.inference` and `GpGrid._raw_predict` FROM THE
    EIGENVECTORS Q_d, THE EIGENVALUES lam_d, y AND THE NOISE TERM AS GIVEN (float64 inputs taken as exact): alpha, y^T alpha,
    sum log(V + noise), and per parameter set q_t = alpha^T ((x)A_d) alpha, s_t = sum ((x)gamma_d) / (V + noise); mu and the
    variance reduction of new points.  The flat index has the LAST dimension fastest; V and (x)gamma multiply from d = 0 up.
  * `dense`: the same quantities from the dense N x N covariance (Cholesky), which knows nothing of eigenvectors: for small N.

`grid_factors` builds K_d, the derivative factors of the D + 2 parameters (D lengthscales, variance, noise) and, given Q, their
gammas in the working type, in the convention of GPy's GridRBF (variance^(1/D) per dimension)."""
import os

import numpy as np

LD = np.longdouble
HAVE_LD = bool(np.finfo(np.longdouble).eps < 1e-18)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kron")
FIXTURES = ["d1_g9_iso", "d2_6x5_ard", "d3_5x4x3_ard", "d4_3x2x3x2_ard", "d3_4x1x3_ard", "d2_7x3_ard_unequal"]


def load_fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    g = {k: z[k] for k in z.files}
    D = g["X"].shape[1]
    g["Qs"] = [g["Q%d" % d] for d in range(D)]
    g["lams"] = [g["lam%d" % d] for d in range(D)]
    return g


def _a(x, dt):
    return np.asarray(x, dtype=dt)


def mode(A, x, dt=LD):
    """one mode product: x (P x G), A (R x G) -> out (R x P), out[r][p] = sum_k A[r][k] x[p][k]"""
    return np.dot(_a(A, dt), _a(x, dt).T)


def kron_mv(As, x, dt=LD):
    """((x)_d A_d) x, last dimension contracted first (the reference's kron_mvprod)"""
    x = _a(x, dt).reshape(-1)
    for d in range(len(As) - 1, -1, -1):
        G = np.shape(As[d])[1]
        x = mode(As[d], x.reshape(x.size // G, G), dt).reshape(-1)
    return x


def kron_vec(vs, dt=LD):
    """(x)_d v_d, multiplied from d = 0 up"""
    out = _a(vs[0], dt).reshape(-1)
    for v in vs[1:]:
        out = (out[:, None] * _a(v, dt).reshape(1, -1)).reshape(-1)
    return out


def evaluate(Qs, lams, y, noise, factors=(), gammas=(), dt=LD):
    """dict(alpha (N), yTa, sumlog, q (nmat), s (nmat), V (N))"""
    noise = dt(noise)
    V = kron_vec(lams, dt)
    t = kron_mv([_a(Q, dt).T for Q in Qs], y, dt) / (V + noise)
    alpha = kron_mv(Qs, t, dt)
    r = dict(alpha=alpha, V=V, yTa=np.dot(_a(y, dt).reshape(-1), alpha), sumlog=np.sum(np.log(V + noise)))
    r["q"] = np.array([np.dot(alpha, kron_mv(A, alpha, dt)) for A in factors], dtype=dt)
    r["s"] = np.array([np.sum(kron_vec(g, dt) / (V + noise)) for g in gammas], dtype=dt)
    return r


def _contract(vec, fs, dt):
    """sum_i vec_i prod_d fs[d][m][i_d] for every m: (M)"""
    M = np.shape(fs[0])[0]
    G = np.shape(fs[-1])[1]
    T = np.dot(_a(vec, dt).reshape(-1, G), _a(fs[-1], dt).T)                 # (P, M)
    for d in range(len(fs) - 2, -1, -1):
        G = np.shape(fs[d])[1]
        T = (T.reshape(-1, G, M) * _a(fs[d], dt).T[None, :, :]).sum(1)
    return T.reshape(M)


def predict(alpha, lams, kx, bx, noise_pred, dt=LD):
    """(mu (M), variance reduction (M)) from alpha, the eigenvalues and the D blocks kx[d] (M x G_d), bx[d] = kx[d] Q_d"""
    w = dt(1) / (kron_vec(lams, dt) + dt(noise_pred))
    return _contract(alpha, kx, dt), _contract(w, [_a(b, dt) ** 2 for b in bx], dt)


def to_host(r):
    """float64 copies of a result dict"""
    return {k: np.asarray(v, dtype=np.float64) for k, v in r.items()}


# ---- the host side: K_d, derivative factors and gammas of an RBF on a grid ----------------------------------------------------
def grid_of(xg):
    """the N x D grid of the D value arrays, last column fastest"""
    return np.array(np.meshgrid(*xg, indexing="ij")).reshape(len(xg), -1).T.copy()


def grid_factors(xg, variance, ls, dt=LD):
    """(Kds, factors): Kds[d] the G_d x G_d factor of dimension d; factors[t][d] the derivative factor of parameter t (t < D:
    lengthscale t; t = D: variance; t = D + 1: noise) in dimension d (GPy grid_kerns.py:55-73)"""
    D = len(xg)
    vd = dt(variance) ** (dt(1) / dt(D))
    r2 = [((_a(x, dt)[:, None] - _a(x, dt)[None, :]) / dt(ls[d])) ** 2 for d, x in enumerate(xg)]
    E = [np.exp(-r / dt(2)) for r in r2]
    Kds = [vd * e for e in E]
    factors = []
    for t in range(D):
        lt = dt(ls[t]) ** (dt(1) / dt(D))
        factors.append([Kds[d] * r2[d] / lt if d == t else Kds[d] / lt for d in range(D)])
    factors.append(list(E))
    factors.append([np.eye(len(x), dtype=dt) for x in xg])
    return Kds, factors


def gammas_of(Qs, factors, dt=LD):
    """gammas[t][d] = diag(Q_d^T A_d^(t)T Q_d)"""
    return [[np.einsum("ij,ij->j", _a(Q, dt), np.dot(_a(A, dt).T, _a(Q, dt))) for Q, A in zip(Qs, As)] for As in factors]


def cross_blocks(xg, Xs, variance, ls, dt=LD):
    """kx[d] = K_d(Xs[:, d], grid_d) (M x G_d)"""
    D = len(xg)
    vd = dt(variance) ** (dt(1) / dt(D))
    return [vd * np.exp(-(((_a(Xs[:, d], dt)[:, None] - _a(xg[d], dt)[None, :]) / dt(ls[d])) ** 2) / dt(2)) for d in range(D)]


# ---- the dense restatement -----------------------------------------------------------------------------------------------------
def kron_mat(Ms, dt=LD):
    out = _a(Ms[0], dt)
    for M in Ms[1:]:
        M = _a(M, dt)
        out = (out[:, None, :, None] * M[None, :, None, :]).reshape(out.shape[0] * M.shape[0], out.shape[1] * M.shape[1])
    return out


def cholesky(A):
    A = A.copy()
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - np.dot(L[j, :j], L[j, :j])
        if not d > 0:
            raise np.linalg.LinAlgError("not positive definite at column %d" % j)
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - np.dot(L[j + 1:, :j], L[j, :j])) / L[j, j]
    return L


def solve_lower(L, B):
    X = np.array(B, dtype=L.dtype, copy=True)
    for i in range(L.shape[0]):
        X[i] = (X[i] - np.dot(L[i, :i], X[:i])) / L[i, i]
    return X


def solve_upper_T(L, B):
    """L^T X = B"""
    X = np.array(B, dtype=L.dtype, copy=True)
    for i in range(L.shape[0] - 1, -1, -1):
        X[i] = (X[i] - np.dot(L[i + 1:, i], X[i + 1:])) / L[i, i]
    return X


def dense(xg, variance, ls, y, noise, Xs=None, noise_pred=None, dt=LD):
    """The same quantities from the dense covariance: dict(alpha, yTa, sumlog (= log det Ky), lml, grad (D + 2: dL/dlengthscale_t,
    dL/dvariance, dL/dnoise), and with Xs: mu, red (variance reduction with Ky = K + noise_pred I))"""
    Kds, factors = grid_factors(xg, variance, ls, dt)
    K = kron_mat(Kds, dt)
    N = K.shape[0]
    yv = _a(y, dt).reshape(-1)
    L = cholesky(K + dt(noise) * np.eye(N, dtype=dt))
    alpha = solve_upper_T(L, solve_lower(L, yv))
    Kyi = solve_upper_T(L, solve_lower(L, np.eye(N, dtype=dt)))
    r = dict(alpha=alpha, yTa=np.dot(yv, alpha), sumlog=dt(2) * np.sum(np.log(np.diag(L))))
    r["lml"] = lml_of(r, N, dt)
    grad = []
    for As in factors:
        dK = kron_mat(As, dt)
        grad.append((np.dot(alpha, np.dot(dK, alpha)) - np.sum(Kyi * dK.T)) / dt(2))
    r["grad"] = np.array(grad, dtype=dt)
    if Xs is not None:
        Ks = kron_rows(cross_blocks(xg, np.asarray(Xs), variance, ls, dt), dt)
        Lp = L if noise_pred is None or noise_pred == noise else cholesky(K + dt(noise_pred) * np.eye(N, dtype=dt))
        W = solve_lower(Lp, Ks.T)
        r["mu"] = np.dot(Ks, alpha)
        r["red"] = np.sum(W * W, axis=0)
    return r


def _pi(dt):
    return dt(4) * np.arctan(dt(1))


def kron_rows(kx, dt=LD):
    """row m: (x)_d kx[d][m] (M x N)"""
    out = _a(kx[0], dt)
    for k in kx[1:]:
        k = _a(k, dt)
        out = (out[:, :, None] * k[:, None, :]).reshape(out.shape[0], -1)
    return out


def lml_of(r, N, dt=LD):
    """the log marginal likelihood from y^T alpha and sum log(V + noise)"""
    return -(dt(r["yTa"]) + dt(r["sumlog"]) + dt(N) * np.log(dt(2) * _pi(dt))) / dt(2)


def grad_of(r, dt=LD):
    """the D + 2 derivatives from q and s"""
    return (_a(r["q"], dt) - _a(r["s"], dt)) / dt(2)


def rel_err(got, ref):
    """max |got - ref| / max |ref|, in the wider of the two types; inf where the shapes differ"""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape:
        return float("inf")
    dt = LD if LD in (got.dtype.type, ref.dtype.type) else np.float64
    got, ref = got.astype(dt), ref.astype(dt)
    if ref.size == 0:
        return 0.0
    den = np.max(np.abs(ref))
    err = np.max(np.abs(got - ref))
    return float(err / den) if den > 0 else float(err)
