"""Long-double (x86 80-bit, eps 1.08e-19) restatement of every kernel kind of the exact-GP device path and of sums / products
of them: K, Kdiag, the contractions sum_ij G_ij dK_ij/dtheta_k in link order, gradients_X, and the exact-GP quantities from a
long-double Cholesky.  Written from the formulas of the reference's kernel classes:

    stationary.py:130-168 (distances), :225-232 (_inv_dist: 1/r, 0 where r == 0), :193-213 (parameter gradients), :330-358
    (gradients_X), rbf.py:51-55, stationary.py:382-386 (Exponential), :488-492 (Matern32), :585-589 (Matern52), :781-798
    (RatQuad), standard_periodic.py:118-139,536-580, linear.py:66-114, mlp.py:48-147, poly.py:15-49, static.py:63-173,
    coregionalize.py:82-157, add.py:58-84, prod.py:58-121.

Distances are taken from coordinate differences, so coincident points give r = 0 exactly and, through `_inv_dist`, no
contribution to any gradient.  Every constant (pi, 2/pi, sqrt 3, sqrt 5) is computed in the working type; no matrix product goes
through `dot` / `@` (explicit sums over the contracted axis); the derivative of K with respect to one parameter is formed,
contracted and dropped before the next one, so nothing of size N x M x nparams is ever held.

specs: [(kind, ard, theta, active_dims, term)] as in the other restatements (periodic_np, linear_np, mlp_np): theta of the
stationary kinds [variance, lengthscale(s)], RatQuad [.., power], StdPeriodic [variance, period(s), lengthscale(s)] with
ard = ARD1 | ARD2 << 1, Linear the variances, MLP [variance, weight variance(s), bias variance], Poly [variance, scale, bias,
order] (three parameters), White / Bias [variance], Coregionalize [W (P x rank, row-major) | kappa] with ard = rank * 100 + P.
Parts with the same non-zero term id are the factors of one product.

Every function takes `dt`, the working type: `np.longdouble` (the default) or `np.float64` -- the same formulas in double
precision, which is what the tests use to measure how far an fp64 evaluation of this input lies from the truth.

The second half of the module holds the shape sweep (inputs and parameters) that the CPU tests, the GPU tests and
tools/make_golden_kernel_shapes.py share."""
import numpy as np

LD = np.longdouble
HAVE_LD = bool(np.finfo(np.longdouble).eps < 1e-18)
EPS64 = float(np.finfo(np.float64).eps)
STATIONARY = ("rbf", "matern52", "matern32", "exponential", "ratquad")


def require_ld():
    assert np.finfo(np.longdouble).eps < 1e-18, "np.longdouble is not an extended format on this host"


def _c(dt):
    """constants in the working type"""
    one = dt(1)
    pi = 4 * np.arctan(one)
    return dict(pi=pi, two_over_pi=2 / pi, s3=np.sqrt(dt(3)), s5=np.sqrt(dt(5)), half=one / 2)


def _a(x, dt):
    return np.asarray(x, dtype=dt)


def n_params(spec):
    kind, ard, th = spec[0], spec[1], spec[2]
    return 3 if kind == "poly" else len(th)


def terms(specs):
    out, ids = [], {}
    for i, s in enumerate(specs):
        t = s[4]
        if t == 0:
            out.append([i])
        elif t in ids:
            out[ids[t]].append(i)
        else:
            ids[t] = len(out)
            out.append([i])
    return out


class _Leaf(object):
    """K of one part and its derivatives one at a time: `dparam(k)` (N x M), `dx(q)` (N x M: dK_ij / dX_iq, None where it is
    identically zero), `has_dx` False for Poly (poly.py:47-48 raises)."""
    has_dx = True

    def __init__(self, spec, X, X2, dt):
        kind, ard, th, dims, _ = spec
        self.kind, self.ard, self.dt = kind, ard, dt
        self.dims = [int(d) for d in dims]
        self.th = _a(th, dt)
        self.sym = X2 is None
        self.A = _a(X, dt)[:, self.dims]
        self.B = self.A if self.sym else _a(X2, dt)[:, self.dims]
        self.N, self.M, self.nd = self.A.shape[0], self.B.shape[0], len(self.dims)
        self.c = _c(dt)
        getattr(self, "_init_" + (kind if kind not in STATIONARY else "stationary"))()

    def _diff(self, a):
        return self.A[:, a][:, None] - self.B[:, a][None, :]

    def _vec(self, v):
        return np.broadcast_to(v, (self.nd,))

    # ---- stationary kinds and RatQuad -------------------------------------------------------------------------------
    def _init_stationary(self):
        th, kind, c = self.th, self.kind, self.c
        self.v = th[0]
        nl = self.nd if self.ard else 1
        self.ls = self._vec(th[1:1 + nl])
        r2 = np.zeros((self.N, self.M), dtype=self.dt)
        for a in range(self.nd):
            r2 = r2 + np.square(self._diff(a) / self.ls[a])
        r = np.sqrt(r2)
        self.r = r
        with np.errstate(divide="ignore"):
            self.inv = np.where(r != 0, 1 / np.where(r != 0, r, 1), 0)           # _inv_dist (stationary.py:225-232)
        v = self.v
        if kind == "rbf":
            self.K = v * np.exp(-r2 / 2)
            self.dK_dr = -r * self.K
        elif kind == "exponential":
            self.K = v * np.exp(-r)
            self.dK_dr = -self.K
        elif kind == "matern32":
            e = v * np.exp(-c["s3"] * r)
            self.K = (1 + c["s3"] * r) * e
            self.dK_dr = -3 * r * e
        elif kind == "matern52":
            e = v * np.exp(-c["s5"] * r)
            self.K = (1 + c["s5"] * r + self.dt(5) / 3 * r2) * e
            self.dK_dr = -(self.dt(5) / 3) * r * (1 + c["s5"] * r) * e
        else:                                                                    # ratquad (stationary.py:781-798)
            self.power = th[1 + nl]
            self.lg = np.log1p(r2 / 2)
            self.K = v * np.exp(-self.power * self.lg)
            self.dK_dr = -v * self.power * r * np.exp(-(self.power + 1) * self.lg)
        self.np_ = 1 + nl + (1 if kind == "ratquad" else 0)

    def _dparam_stationary(self, k):
        if k == 0:
            return self.K / self.v
        nl = self.nd if self.ard else 1
        if k <= nl:
            if self.ard:                                                         # stationary.py:203-210,234-235
                a = k - 1
                return -(self.dK_dr * self.inv) * np.square(self._diff(a)) / self.ls[a] ** 3
            return -self.dK_dr * self.r / self.ls[0]                             # stationary.py:212-213
        return -self.K * self.lg                                                 # dK/dpower (stationary.py:790-798)

    def _dx_stationary(self, a):
        return self.dK_dr * self.inv * self._diff(a) / self.ls[a] ** 2           # stationary.py:330-358

    # ---- StdPeriodic (standard_periodic.py:118-133,536-580) ---------------------------------------------------------
    def _init_stdperiodic(self):
        th = self.th
        self.v = th[0]
        npr = self.nd if self.ard & 1 else 1
        self.T = self._vec(th[1:1 + npr])
        self.ls = self._vec(th[1 + npr:])
        self.npr, self.nl = npr, (self.nd if self.ard & 2 else 1)
        s = np.zeros((self.N, self.M), dtype=self.dt)
        for a in range(self.nd):
            s = s + np.square(np.sin(self.c["pi"] * self._diff(a) / self.T[a]) / self.ls[a])
        self.K = self.v * np.exp(-s / 2)
        self.np_ = 1 + self.npr + self.nl

    def _dT(self, a):
        base = self.c["pi"] * self._diff(a) / self.T[a]
        return self.K * np.sin(base) * np.cos(base) * base / (self.T[a] * self.ls[a] ** 2)

    def _dl(self, a):
        base = self.c["pi"] * self._diff(a) / self.T[a]
        return self.K * np.square(np.sin(base)) / self.ls[a] ** 3

    def _dparam_stdperiodic(self, k):
        if k == 0:
            return self.K / self.v
        if k <= self.npr:
            return self._dT(k - 1) if self.ard & 1 else sum(self._dT(a) for a in range(self.nd))
        k -= 1 + self.npr
        return self._dl(k) if self.ard & 2 else sum(self._dl(a) for a in range(self.nd))

    def _dx_stdperiodic(self, a):
        base = self.c["pi"] * self._diff(a) / self.T[a]
        return -self.c["pi"] / (2 * self.T[a] * self.ls[a] ** 2) * np.sin(2 * base) * self.K

    # ---- Linear (linear.py:66-114) ----------------------------------------------------------------------------------
    def _ab(self, a):
        return self.A[:, a][:, None] * self.B[:, a][None, :]

    def _init_linear(self):
        self.vq = self._vec(self.th)
        self.K = np.zeros((self.N, self.M), dtype=self.dt)
        for a in range(self.nd):
            self.K = self.K + self.vq[a] * self._ab(a)
        self.np_ = len(self.th)

    def _dparam_linear(self, k):
        return self._ab(k) if self.ard else sum(self._ab(a) for a in range(self.nd))

    def _dx_linear(self, a):
        return np.broadcast_to(self.vq[a] * self.B[:, a][None, :], (self.N, self.M))

    # ---- MLP (mlp.py:48-147) ----------------------------------------------------------------------------------------
    def _init_mlp(self):
        th = self.th
        self.v, self.b = th[0], th[-1]
        self.w = self._vec(th[1:-1])
        s = np.zeros((self.N, self.M), dtype=self.dt) + self.b
        for a in range(self.nd):
            s = s + self.w[a] * self._ab(a)
        self.s = s
        self.qi = (np.sum(self.w * np.square(self.A), axis=1) + self.b + 1)[:, None]
        self.qj = (np.sum(self.w * np.square(self.B), axis=1) + self.b + 1)[None, :]
        self.K = self.v * self.c["two_over_pi"] * np.arcsin(s / np.sqrt(self.qi * self.qj))
        self.cc = self.v * self.c["two_over_pi"] / np.sqrt(self.qi * self.qj - s * s)      # dK/ds at fixed norms (mlp.py:105)
        self.np_ = len(th)

    def _dw(self, a):
        a2, b2 = np.square(self.A[:, a])[:, None], np.square(self.B[:, a])[None, :]
        return self.cc * (self._ab(a) - self.s * (a2 / self.qi + b2 / self.qj) / 2)

    def _dparam_mlp(self, k):
        if k == 0:
            return self.K / self.v
        if k == self.np_ - 1:
            return self.cc * (1 - self.s * (1 / self.qi + 1 / self.qj) / 2)
        return self._dw(k - 1) if self.ard else sum(self._dw(a) for a in range(self.nd))

    def _dx_mlp(self, a):                                                        # mlp.py:124-130
        return self.cc * self.w[a] * (self.B[:, a][None, :] - self.s * self.A[:, a][:, None] / self.qi)

    # ---- Poly (poly.py:15-49) ---------------------------------------------------------------------------------------
    def _init_poly(self):
        self.v, self.scale, self.bias, self.order = self.th
        d = np.zeros((self.N, self.M), dtype=self.dt)
        for a in range(self.nd):
            d = d + self._ab(a)
        self.d = d
        self.base = self.scale * d + self.bias
        self.K = self.v * self.base ** self.order
        self.np_ = 3
        self.has_dx = False

    def _dparam_poly(self, k):
        if k == 0:
            return self.base ** self.order
        pm1 = self.v * self.order * self.base ** (self.order - 1)
        return pm1 * self.d if k == 1 else pm1

    # ---- White / Bias (static.py:63-173) ----------------------------------------------------------------------------
    def _init_white(self):
        self.E = np.eye(self.N, dtype=self.dt) if self.sym else np.zeros((self.N, self.M), dtype=self.dt)
        self.K = self.th[0] * self.E
        self.np_ = 1

    def _dparam_white(self, k):
        return self.E

    def _init_bias(self):
        self.K = np.zeros((self.N, self.M), dtype=self.dt) + self.th[0]
        self.np_ = 1

    def _dparam_bias(self, k):
        return np.ones((self.N, self.M), dtype=self.dt)

    # ---- Coregionalize (coregionalize.py:82-157) --------------------------------------------------------------------
    def _init_coregionalize(self):
        P, r = self.ard % 100, self.ard // 100
        self.P, self.rank = P, r
        self.W = self.th[:P * r].reshape(P, r)
        self.kappa = self.th[P * r:]
        Bm = np.sum(self.W[:, None, :] * self.W[None, :, :], axis=2)
        Bm[np.arange(P), np.arange(P)] += self.kappa
        self.Bm = Bm
        self.ia = np.asarray(self.A[:, 0], dtype=np.float64).astype(int)
        self.ib = np.asarray(self.B[:, 0], dtype=np.float64).astype(int)
        self.K = Bm[self.ia][:, self.ib]
        self.np_ = P * r + P

    def _dparam_coregionalize(self, k):
        ea = lambda p: (self.ia == p).astype(self.dt)[:, None]
        eb = lambda p: (self.ib == p).astype(self.dt)[None, :]
        if k < self.P * self.rank:                                               # dB/dW_pc = e_p W[:, c]^T + W[:, c] e_p^T
            p, c = divmod(k, self.rank)
            return ea(p) * self.W[self.ib, c][None, :] + self.W[self.ia, c][:, None] * eb(p)
        p = k - self.P * self.rank
        return ea(p) * eb(p)

    # ---- common -----------------------------------------------------------------------------------------------------
    def dparam(self, k):
        return getattr(self, "_dparam_" + (self.kind if self.kind not in STATIONARY else "stationary"))(k)

    def dx(self, q):
        """dK_ij / dX_iq for column q of X; None if the part does not depend on it"""
        if self.kind in ("white", "bias", "coregionalize") or q not in self.dims:
            return None
        return getattr(self, "_dx_" + (self.kind if self.kind not in STATIONARY else "stationary"))(self.dims.index(q))

    def dx_abs(self, q):
        """what one rounding error inside dx(q) is relative to: |dx(q)|, except where the formula itself subtracts or takes a
        sine near a multiple of pi.  MLP: |c w| (|y_q| + |s x_q / q_i|), the two terms of mlp.py:124-130; StdPeriodic: the
        rounding of the argument 2 pi d / T moves sin by |2 Delta cos 2 Delta| eps, so |sin 2 Delta| + |2 Delta cos 2 Delta|."""
        a = self.dims.index(q)
        if self.kind == "mlp":
            return np.abs(self.cc * self.w[a]) * (np.abs(self.B[:, a])[None, :] + np.abs(self.s * self.A[:, a][:, None] / self.qi))
        if self.kind == "stdperiodic":
            b2 = 2 * self.c["pi"] * self._diff(a) / self.T[a]
            return np.abs(self.c["pi"] / (2 * self.T[a] * self.ls[a] ** 2) * self.K) * (np.abs(np.sin(b2)) + np.abs(b2 * np.cos(b2)))
        return np.abs(self.dx(q))


def leaf_Kdiag(spec, X, dt=LD):
    kind, ard, th, dims, _ = spec
    th = _a(th, dt)
    A = _a(X, dt)[:, [int(d) for d in dims]]
    nd = A.shape[1]
    if kind == "linear":                                                         # linear.py:84-85
        return np.sum(np.broadcast_to(th, (nd,)) * np.square(A), axis=1)
    if kind == "mlp":                                                            # mlp.py:61-64
        p = np.sum(np.broadcast_to(th[1:-1], (nd,)) * np.square(A), axis=1) + th[-1]
        return th[0] * _c(dt)["two_over_pi"] * np.arcsin(p / (p + 1))
    if kind == "poly":                                                           # poly.py:33-34
        return th[0] * (th[1] * np.sum(np.square(A), axis=1) + th[2]) ** th[3]
    if kind == "coregionalize":                                                  # coregionalize.py:106-107
        P, r = ard % 100, ard // 100
        W = th[:P * r].reshape(P, r)
        return (np.sum(W * W, axis=1) + th[P * r:])[np.asarray(A[:, 0], dtype=np.float64).astype(int)]
    return np.zeros(A.shape[0], dtype=dt) + th[0]


def _prod(mats):
    out = mats[0]
    for m in mats[1:]:
        out = out * m
    return out


def leaves(specs, X, X2=None, dt=LD):
    return [_Leaf(s, X, X2, dt) for s in specs]


def K(specs, X, X2=None, dt=LD, lv=None):
    lv = lv or leaves(specs, X, X2, dt)
    out = 0
    for t in terms(specs):
        out = out + _prod([lv[i].K for i in t])
    return out


def Kdiag(specs, X, dt=LD):
    out = 0
    for t in terms(specs):
        out = out + _prod([leaf_Kdiag(specs[i], X, dt) for i in t])
    return out


def _weights(specs, lv, G):
    """per leaf: dL_dK times the other factors of its product (prod.py:86-99)"""
    out = [None] * len(specs)
    for t in terms(specs):
        for i in t:
            out[i] = _prod([G] + [lv[j].K for j in t if j != i])
    return out


def dtheta(specs, G, X, X2=None, dt=LD, lv=None):
    """(sum_ij G_ij dK_ij/dtheta_k, sum_ij |G_ij dK_ij/dtheta_k|) over all parameters in link order"""
    lv = lv or leaves(specs, X, X2, dt)
    G = _a(G, dt)
    val, cond = [], []
    for leaf, W in zip(lv, _weights(specs, lv, G)):
        for k in range(leaf.np_):
            t = W * leaf.dparam(k)
            val.append(np.sum(t))
            cond.append(np.sum(np.abs(t)))
    return np.array(val, dtype=dt), np.array(cond, dtype=dt)


def has_gradients_X(specs):
    return all(s[0] != "poly" for s in specs)


def gradients_X(specs, G, X, X2=None, dt=LD, lv=None):
    """(kern.gradients_X(G, X, X2), its per-entry cond), both N x D.  X2 None: the weights are G + G^T against X itself
    (stationary.py:340-344, linear.py:108-114, mlp.py:124-127); that sum is itself rounded by whoever forms it, so the cond of
    this form weighs every term with |G_ij| + |G_ji|.  A row of gradients_X can be a sum of one term (M = 1), so the cond
    also counts the subtraction inside a term where the formula has one (`_Leaf.dx_abs`)."""
    assert has_gradients_X(specs), "Poly has no gradients_X (poly.py:47-48)"
    lv = lv or leaves(specs, X, X2, dt)
    G = _a(G, dt)
    Gs, Ga = (G + G.T, np.abs(G) + np.abs(G).T) if X2 is None else (G, np.abs(G))
    N, D = np.shape(X)
    val, cond = np.zeros((N, D), dtype=dt), np.zeros((N, D), dtype=dt)
    Ws, Wa = _weights(specs, lv, Gs), _weights(specs, lv, Ga)
    for leaf, W, Wab in zip(lv, Ws, Wa):
        for q in leaf.dims:
            d = leaf.dx(q)
            if d is not None:
                val[:, q] += np.sum(W * d, axis=1)
                cond[:, q] += np.sum(np.abs(Wab) * leaf.dx_abs(q), axis=1)
    return val, cond


# ---- the exact-GP quantities from a column-oriented Cholesky ----------------------------------------------------------------
def cholesky(A, max_n=129):
    """lower factor, one vector update per column (left-looking), in the type of A"""
    A = np.array(A)
    n = A.shape[0]
    assert n <= max_n, "the long-double Cholesky is meant for N <= %d" % max_n
    L = np.zeros_like(A)
    for j in range(n):
        col = A[j:, j] - np.sum(L[j:, :j] * L[j, :j][None, :], axis=1)
        assert col[0] > 0, "not positive definite at column %d" % j
        L[j, j] = np.sqrt(col[0])
        L[j + 1:, j] = col[1:] / L[j, j]
    return L


def solve_lower(L, B):
    T = np.zeros_like(B)
    for j in range(L.shape[0]):
        T[j] = (B[j] - np.sum(L[j, :j][:, None] * T[:j], axis=0)) / L[j, j]
    return T


def solve_upper_T(L, B):
    """L^-T B"""
    T = np.zeros_like(B)
    for j in range(L.shape[0] - 1, -1, -1):
        T[j] = (B[j] - np.sum(L[j + 1:, j][:, None] * T[j + 1:], axis=0)) / L[j, j]
    return T


def matmul(A, B):
    """A B by explicit sums over the contracted axis, one output column block at a time"""
    out = np.zeros((A.shape[0], B.shape[1]), dtype=A.dtype)
    for j in range(B.shape[1]):
        out[:, j] = np.sum(A * B[:, j][None, :], axis=1)
    return out


def lgamma(x, dt=LD):
    """log Gamma(x), x > 0: recurrence up to x >= 20, then the Stirling series (error < 1e-22 there)"""
    x = dt(x)
    shift = dt(0)
    while x < 20:
        shift = shift + np.log(x)
        x = x + 1
    pi = _c(dt)["pi"]
    ser = 0
    for num, den, k in ((1, 12, 1), (-1, 360, 3), (1, 1260, 5), (-1, 1680, 7), (1, 1188, 9), (-691, 360360, 11), (1, 156, 13)):
        ser = ser + dt(num) / dt(den) / x ** k
    return (x - dt(1) / 2) * np.log(x) - x + np.log(2 * pi) / 2 + ser - shift


def exact(specs, X, Y, noise, nu=None, jitter=1e-8, dt=LD, max_n=129):
    """ExactGaussianInference (exact_gaussian_inference.py) or, with nu, the Student-t process (exact_studentt_inference.py:20-52):
    dict(lml, logdet, alpha, L, Linv, Ki, dL_dK, dtheta, dtheta_cond, dnoise)"""
    lv = leaves(specs, X, None, dt)
    Kx = K(specs, X, None, dt, lv)
    Y = _a(Y, dt)
    N, Dy = Y.shape
    pi = _c(dt)["pi"]
    Ky = np.array(Kx)
    Ky[np.arange(N), np.arange(N)] += (dt(0) if nu is not None else _a(noise, dt)) + dt(jitter)      # noise: one variance or N
    L = cholesky(Ky, max_n)
    Li = solve_lower(L, np.eye(N, dtype=dt))
    Ki = matmul(Li.T, Li)
    alpha = solve_upper_T(L, solve_lower(L, Y))
    logdet = 2 * np.sum(np.log(np.diag(L)))
    aaT = matmul(alpha, alpha.T)
    if nu is None:
        lml = (-N * Dy * np.log(2 * pi) - Dy * logdet - np.sum(alpha * Y)) / 2
        dL_dK = (aaT - Dy * Ki) / 2
        dnoise = np.sum(np.diag(dL_dK))
    else:
        nu = dt(nu)
        beta = np.sum(alpha * Y)
        lml = (-N * np.log((nu - 2) * pi) - logdet - (nu + N) * np.log1p(beta / (nu - 2))) / 2 + \
            lgamma((nu + N) / 2, dt) - lgamma(nu / 2, dt)
        dL_dK = ((nu + N) / (nu + beta - 2) * aaT - Ki) / 2
        dnoise = None
    val, cond = dtheta(specs, dL_dK, X, None, dt, lv)
    return dict(lml=lml, logdet=logdet, alpha=alpha, L=L, Linv=Li, Ki=Ki, dL_dK=dL_dK, dtheta=val, dtheta_cond=cond, dnoise=dnoise)


def predict(specs, X, ex, Xs, dt=LD):
    """(mu, var (M x 1), cov (M x M)) of the latent function at Xs (posterior.py:273-302) from the result of `exact`"""
    Kx = K(specs, X, Xs, dt)
    mu = matmul(Kx.T, ex["alpha"])
    T = solve_lower(ex["L"], Kx)
    var = (Kdiag(specs, Xs, dt) - np.sum(T * T, axis=0))[:, None]
    cov = K(specs, Xs, None, dt) - matmul(T.T, T)
    return mu, var, cov


def f64(x):
    """rounded once to double"""
    return np.asarray(x, dtype=np.float64)


# ---- the judge the GPU tests use -----------------------------------------------------------------------------------------
def k_figure(got, K_ld, scale):
    """max |got - K_ld| in units of eps64 x scale"""
    return float(np.max(np.abs(_a(got, LD) - K_ld)) / (EPS64 * LD(scale)))


def k_ok(got, K_ld, scale, tol=1e-13):
    """|K - K_ld| <= 1e-13 x scale, entry by entry (shape included)"""
    return np.shape(got) == np.shape(K_ld) and bool(np.all(np.abs(_a(got, LD) - K_ld) <= LD(tol) * LD(scale)))


def grad_tol(ref_ld, ref_64, cond, factor=256.0):
    """per-entry bound max(32 e64, factor eps64 cond): e64 = |fp64 restatement - long double| on the same input"""
    e64 = np.abs(_a(ref_64, LD) - ref_ld)
    return np.maximum(32 * e64, LD(factor) * LD(EPS64) * cond)


def grad_figure(got, ref_ld, cond):
    """worst |got - ref_ld| / (eps64 cond) over the entries (entries with cond 0 must be matched exactly: inf otherwise)"""
    err = np.abs(_a(got, LD) - ref_ld)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(cond > 0, err / (LD(EPS64) * np.where(cond > 0, cond, 1)), np.where(err > 0, np.inf, 0))
    return float(np.max(f)) if f.size else 0.0


def grad_ok(got, ref_ld, tol):
    """every entry inside its own bound (shape included)"""
    return np.shape(got) == np.shape(ref_ld) and bool(np.all(np.abs(_a(got, LD) - ref_ld) <= tol))


# ---- the shape sweep ------------------------------------------------------------------------------------------------------
# (N, M, D, Dy): the smallest shapes at which each mechanism of the device kernels engages (64 x 64 tiles, 32-dimension
# chunks / ARD groups, 128-row padding, four output columns in registers)
SHAPES = [(1, 1, 1, 1), (2, 3, 3, 1), (63, 1, 2, 1), (64, 65, 32, 2), (65, 63, 33, 1), (65, 64, 65, 5), (129, 130, 5, 4)]
SUBSET_SHAPE = (129, 130, 5, 4)          # the shape at which active_dims is a strict subset (columns 0, 2, 3)
STUDENTT_SHAPE = (65, 63, 33, 1)
COREG_P = 3
# (name, kind, ard or rank / order)
VARIANTS = [("rbf_iso", "rbf", 0), ("rbf_ard", "rbf", 1), ("matern52_iso", "matern52", 0), ("matern52_ard", "matern52", 1),
            ("matern32_iso", "matern32", 0), ("matern32_ard", "matern32", 1), ("exponential_iso", "exponential", 0),
            ("exponential_ard", "exponential", 1), ("ratquad_iso", "ratquad", 0), ("ratquad_ard", "ratquad", 1),
            ("stdperiodic_iso", "stdperiodic", 0), ("stdperiodic_ard", "stdperiodic", 3), ("linear_iso", "linear", 0),
            ("linear_ard", "linear", 1), ("mlp_iso", "mlp", 0), ("mlp_ard", "mlp", 1), ("poly_o1", "poly", 1), ("poly_o3", "poly", 3),
            ("white", "white", 0), ("bias", "bias", 0), ("coreg_r1", "coregionalize", 1), ("coreg_r2", "coregionalize", 2)]
KINDS = ("rbf", "matern52", "matern32", "exponential", "white", "bias", "ratquad", "stdperiodic", "coregionalize", "linear", "mlp",
         "poly")


def case_id(variant, shape):
    return "%s-n%d_m%d_d%d_dy%d" % ((variant[0],) + tuple(shape))


def _theta(kind, sub, nd, rng):
    """moderate parameters; lengthscales grow like sqrt(nd) so that K keeps off-diagonal mass at 65 dimensions"""
    ls = np.sqrt(nd) * rng.uniform(0.8, 1.6, nd)
    if kind in ("rbf", "matern52", "matern32", "exponential"):
        return np.concatenate([[1.3], ls if sub else ls[:1]])
    if kind == "ratquad":
        return np.concatenate([[0.9], ls if sub else ls[:1], [1.7]])
    if kind == "stdperiodic":                       # periods are multiples of 1/8: a pair exactly one period apart exists in fp64
        T = rng.integers(12, 25, nd) / 8.0
        return np.concatenate([[1.1], T if sub & 1 else T[:1], ls if sub & 2 else ls[:1]])
    if kind == "linear":
        v = rng.uniform(0.5, 1.5, nd) / nd
        return v if sub else v[:1]
    if kind == "mlp":
        w = rng.uniform(0.5, 1.5, nd) / nd
        return np.concatenate([[1.2], w if sub else w[:1], [0.4]])
    if kind == "poly":
        return np.array([0.8, 0.25 / nd, 2.0, float(sub)])        # scale x.y + bias stays away from 0: no cancellation in the base
    if kind in ("white", "bias"):
        return np.array([0.7])
    W = rng.uniform(-1.0, 1.0, (COREG_P, sub))
    return np.concatenate([W.ravel(), rng.uniform(0.3, 0.9, COREG_P)])


def make_case(variant, shape, edges=True):
    """the seeded inputs of one (variant, shape): dict(spec, X, X2, Y, G (N x N), G2 (N x M), noise, ...).

    Deliberate edges: row 1 of X equals row 0 and row 0 of X2 equals the last row of X (N >= 2); Linear / MLP / Poly get one
    all-zero input row; StdPeriodic gets one pair of points exactly one period apart in the first active dimension.
    `edges=False` leaves the seeded inputs as they are (for references whose distance formula is not exact at r = 0)."""
    name, kind, sub = variant
    N, M, D, Dy = shape
    rng = np.random.default_rng([KINDS.index(kind), sub, N, M, D])
    X = rng.standard_normal((N, D))
    X2 = rng.standard_normal((M, D))
    dims = np.array([0, 2, 3]) if tuple(shape) == SUBSET_SHAPE else np.arange(D)
    if kind == "coregionalize":
        dims = np.array([D - 1])
        X[:, D - 1] = rng.integers(0, COREG_P, N)
        X2[:, D - 1] = rng.integers(0, COREG_P, M)
    th = _theta(kind, sub, len(dims), rng)
    if edges and kind in ("linear", "mlp", "poly") and N >= 3:
        X[N // 2] = 0.0
    if edges and N >= 2:
        X[1] = X[0]
        X2[0] = X[N - 1]
    if edges and kind == "stdperiodic" and N >= 3:
        X[2, dims[0]] = 0.25
        X[N - 1, dims[0]] = 0.25 + th[1]                          # exact: both are multiples of 1/8
        X2[0] = X[N - 1]
    ard = sub if kind != "coregionalize" else sub * 100 + COREG_P
    if kind == "poly":
        ard = 0
    spec = (kind, ard, th, dims, 0)
    scale = float(np.max(Kdiag([spec], np.vstack([X, X2]), np.float64)))
    Y = rng.standard_normal((N, Dy))
    return dict(name=name, kind=kind, shape=tuple(shape), spec=spec, X=X, X2=X2, Y=Y, G=rng.standard_normal((N, N)),
                G2=rng.standard_normal((N, M)), scale=scale, noise=0.1 * scale, E=rng.standard_normal((N, 2)),
                E2=rng.standard_normal((M, 2)))


def fused_exprs(case):
    """the three expressions of the fused calls: the kind alone, next to a White, and as a factor of a product with an RBF on two
    further columns (disjoint active_dims): [(label, specs, X, Xs)]"""
    spec, X, X2 = case["spec"], case["X"], case["X2"]
    D = X.shape[1]
    white = ("white", 0, np.array([0.05 * case["scale"]]), np.arange(D), 0)
    rbf = ("rbf", 1, np.array([1.1, 1.4, 0.8]), np.array([D, D + 1]), 1)
    return [("alone", [spec], X, X2), ("plus_white", [spec, white], X, X2),
            ("times_rbf", [spec[:4] + (1,), rbf], np.hstack([X, case["E"]]), np.hstack([X2, case["E2"]]))]


def cabi_specs(specs):
    """the part list the device takes: a Coregionalize entry becomes (B symmetrised, ard = P)"""
    out = []
    for s in specs:
        if s[0] == "coregionalize":
            lf = _Leaf(s, np.zeros((1, int(s[3][0]) + 1)), None, np.float64)
            out.append((s[0], s[1] % 100, (0.5 * (lf.Bm + lf.Bm.T)).ravel(), s[3], s[4]))
        else:
            out.append(s)
    return out


def chain_coreg(specs, dev, dt=LD):
    """the device's concatenated gradients in link order: a Coregionalize part's S (P x P) becomes dW = (S + S^T) W, then
    dkappa = diag S (coregionalize.py:123-128); the slot of a Poly part's fixed order (0) is dropped"""
    out, i = [], 0
    for s in specs:
        if s[0] == "coregionalize":
            P, r = s[1] % 100, s[1] // 100
            S = np.asarray(dev[i:i + P * P], dtype=np.float64).reshape(P, P)
            W = np.asarray(s[2][:P * r], dtype=np.float64).reshape(P, r)
            out += [((S + S.T) @ W).ravel(), np.diag(S).copy()]
            i += P * P
        elif s[0] == "poly":
            assert dev[i + 3] == 0.0
            out.append(np.asarray(dev[i:i + 3]))
            i += 4
        else:
            out.append(np.asarray(dev[i:i + len(s[2])]))
            i += len(s[2])
    return np.concatenate(out)
