"""Covariance functions backed by libmi355gp.so -- drop-in for the hot-path methods of the reference's kernels:

    K(X, X2=None), Kdiag(X), update_gradients_full(dL_dK, X, X2=None), update_gradients_diag(dL_dKdiag, X), gradients_X(...)

`Kern` is the base of every kernel here, after `GPy/kern/src/kern.py:12-361`: the common constructor part, `active_dims`
slicing (`kern.py:112-117`), `+` / `*`, serialisation, the cached device K-build and gradient passes, and the expression
interface through which the inference classes describe any kernel, leaf or combination, to the C-ABI (`leaves`, `part_specs`,
`_slice_X`, `jitter_diag`).  The leaves: the stationary kernels `RBF` / `ExpQuad` / `Matern52` / `Matern32` / `Exponential` /
`OU` / `RatQuad` / `Cosine` / `Sinc` / `ExpQuadCosine` (`GPy/kern/src/stationary.py`, `rbf.py`), `StdPeriodic`,
`Coregionalize`, `Linear`, `MLP`, `Poly` and the static `White` / `Bias`; the combinations: `Add` and `Prod`.  Same constructor arguments, parameter names, link order and `.gradient`
side effects as the reference.  All array math runs in hand-written HIP kernels (csrc/kern*.hip); there is no NumPy fallback.
"""
import numpy as np

from . import _lib
from .lazy import ArrayIdentity, DeviceResult
from .param import Param, Parameterized
from .variational import SpikeAndSlabPosterior


class _KCache(object):
    """`@Cache_this(limit=3)` of the reference's `Stationary.K` (`stationary.py:96-105`, paramz `Cacher`): the last
    `limit` results keyed by (X, X2) and the exact parameter bits, so the K that the inference step evaluated is not
    recomputed (upload + build + download) when the gradient / prediction step asks for it again.
    paramz caches only for `Observable` inputs and invalidates through their observers.  Here an input is recognised either
    by identity -- only if it is FROZEN (read-only through its whole base chain, which is how the model drivers hold X) --
    or by a full element-wise comparison with a private copy (O(N D), nothing next to the N^2 D build); never by a sampled
    fingerprint or by the address of a writable buffer.  The cached matrix is shared between callers and therefore
    read-only: `K = k.K(X).copy()` before editing it in place (the reference hands out its cache entry writable, and an
    in-place edit silently corrupts later hits)."""

    def __init__(self, limit=3):
        self.limit = limit
        self.entries = []            # [(idX, idX2, theta bytes, value)], most recent last

    def get(self, X, X2, theta, compute):
        tb = theta.tobytes()
        for i, (ix, ix2, t, v) in enumerate(self.entries):
            if t == tb and ix.matches(X) and ix2.matches(X2):
                self.entries.append(self.entries.pop(i))
                return v
        v = compute()
        v.setflags(write=False)      # shared between callers, like paramz's cached arrays
        self.entries.append((ArrayIdentity(X), ArrayIdentity(X2), tb, v))
        if len(self.entries) > self.limit:
            self.entries.pop(0)
        return v

    def clear(self):
        self.entries = []


class Kern(Parameterized):
    """Base of every kernel (reference `GPy/kern/src/kern.py:12-361`).  A subclass sets `kind` (the C-ABI's name for it) and
    `_gpy_class`, links its parameters and gives `_theta()`, `Kdiag`, `_install_gradients(g)` and the diagonal gradients;
    `ARD` is what the C-ABI takes as `ard` for the kind."""
    kind = None                # name understood by the C-ABI
    _gpy_class = None          # "class" string for to_dict (resolvable by GPy's loader)
    _support_GPU = True
    is_leaf = True             # not an Add / Prod: what a Prod takes as a factor
    fused_alone = True         # the fused inference entries take it on its own (a lone White / Bias / Coregionalize: they do not)
    diag_is_constant = True    # Kdiag does not depend on the point

    def __init__(self, input_dim, active_dims, name, device=0):
        super(Kern, self).__init__(name)
        self.input_dim = int(input_dim)
        self.device = device
        self.useGPU = True
        if active_dims is None:
            active_dims = np.arange(self.input_dim)
        self.active_dims = np.atleast_1d(np.asarray(active_dims, dtype=np.int_))
        assert self.active_dims.size == self.input_dim, "input_dim=%d does not match len(active_dims)=%d" % (
            self.input_dim, self.active_dims.size)
        self._K_cache = _KCache(limit=3)

    def __getstate__(self):
        d = dict(self.__dict__)
        d["_K_cache"] = _KCache(limit=3)
        return d

    # ---- the expression interface: how the inference classes describe a kernel, leaf or combination, to the C-ABI ---------
    def leaves(self):
        """the leaf kernels of the expression in link (= parameter, = gradient) order"""
        return [self]

    def part_specs(self):
        """[(kind, ARD, theta, active_dims, term)] for the C-ABI (`mi355gp_part`).  A kernel on its own is one part without
        active_dims: its column slicing is applied to X on upload (`_slice_X`)."""
        return [(self.kind, self.ARD, self._theta(), None, 0)]

    def _slice_X(self, X):
        """The X the device is given for this kernel: the active columns (reference `kern.py:112-117`); a combination hands
        over all of X, its parts carry their active_dims in `part_specs`."""
        X = np.asarray(X)
        if X.shape[1] == self.input_dim and np.array_equal(self.active_dims, np.arange(self.input_dim)):
            return _lib.f64(X)
        assert X.shape[1] > self.active_dims.max(), "At least %d dimensional X needed, X.shape=%r" % (
            self.active_dims.max() + 1, X.shape)
        return _lib.f64(X[:, self.active_dims])

    def diag_variance(self):
        """Kdiag where it is one number (`diag_is_constant`; theta starts with the variance)"""
        return float(self._theta()[0])

    def jitter_diag(self, X):
        """diag K(X, X) as jitchol's mean(diag(A)) needs it (reference `util/linalg.py:65`): one number where it is constant,
        `Kdiag(X)` where a Coregionalize, Linear, MLP or Poly leaf makes it depend on the point"""
        return self.Kdiag(X) if diag_depends_on_point(self) else self.diag_variance()

    def _install_fused(self, g):
        """install the concatenated gradients of a fused inference call, leaf by leaf"""
        i = 0
        for p in self.leaves():
            k = p._theta().size
            p._install_gradients(g[i:i + k])
            i += k

    # ---- the hot-path interface -----------------------------------------------------------------------
    def K(self, X, X2=None):
        """Covariance matrix K(X, X2), built on the device (reference `stationary.py:105-115`, `@Cache_this(limit=3)` :105)."""
        X = np.asarray(X)
        X2 = None if X2 is None else np.asarray(X2)
        theta = self._theta()

        def compute():
            Xs = self._slice_X(X)
            X2s = None if X2 is None else self._slice_X(X2)
            return _lib.kern_K(self.kind, self.ARD, theta, Xs, X2s, device=self.device)
        return self._K_cache.get(X, X2, theta, compute)

    def update_gradients_full(self, dL_dK, X, X2=None):
        """Writes the parameters' `.gradient` (reference `stationary.py:193-213`).

        When `dL_dK` is the device-resident result of a gpy_amd inference call for this kernel the gradients were already
        reduced on the GPU in the same pass and are simply installed."""
        if isinstance(dL_dK, DeviceResult) and X2 is None and dL_dK.matches_kernel(self):
            g = dL_dK.fused_dtheta
        else:
            g = _lib.update_gradients_full(self.kind, self.ARD, self._theta(), np.asarray(dL_dK), self._slice_X(X),
                                           None if X2 is None else self._slice_X(X2), device=self.device)
        self._install_gradients(g)

    def update_gradients_diag(self, dL_dKdiag, X):
        raise NotImplementedError

    def gradients_X(self, dL_dK, X, X2=None):
        """dL/dX from dL_dK (reference `stationary.py:245-252,330-358`), reduced on the device."""
        g = _lib.gradients_X(self.kind, self.ARD, self._theta(), np.asarray(dL_dK), self._slice_X(X),
                             None if X2 is None else self._slice_X(X2), device=self.device)
        if g.shape[1] == np.asarray(X).shape[1]:
            return g
        full = np.zeros(np.asarray(X).shape)          # active_dims slicing (kernel_slice_operations.py:113-136)
        full[:, self.active_dims] = g
        return full

    def gradients_X_diag(self, dL_dKdiag, X):
        """zero where the diagonal is constant (reference `stationary.py:360-361`, `static.py:40-41`,
        `standard_periodic.py:582-583`, `coregionalize.py:156-157`)"""
        return np.zeros(np.asarray(X).shape)

    def __add__(self, other):
        return Add([self, other])

    def __mul__(self, other):
        return Prod([self, other])

    # ---- bookkeeping ----------------------------------------------------------------------------------
    def to_dict(self):
        """JSON-serialisable description with the reference's "class" string (`kern.py:63-76`); subclasses add their own keys"""
        return {"class": self._gpy_class, "name": self.name, "input_dim": self.input_dim,
                "active_dims": self.active_dims.tolist()}

    @classmethod
    def from_dict(cls, d):
        d = dict(d)
        d.pop("class", None)
        d.pop("useGPU", None)
        return cls(**d)

    def copy(self):
        return self.__class__.from_dict(self.to_dict())


class Stationary(Kern):
    def __init__(self, input_dim, variance=1., lengthscale=None, ARD=False, active_dims=None, name=None,
                 useGPU=True, device=0):
        super(Stationary, self).__init__(input_dim, active_dims, name or self.kind, device)
        self.ARD = bool(ARD)
        if not self.ARD:
            if lengthscale is None:
                lengthscale = np.ones(1)
            else:
                lengthscale = np.asarray(lengthscale, dtype=float)
                assert lengthscale.size == 1, "Only 1 lengthscale needed for non-ARD kernel"
        else:
            if lengthscale is not None:
                lengthscale = np.asarray(lengthscale, dtype=float)
                assert lengthscale.size in [1, self.input_dim], "Bad number of lengthscales"
                if lengthscale.size != self.input_dim:
                    lengthscale = np.ones(self.input_dim) * lengthscale
            else:
                lengthscale = np.ones(self.input_dim)
        self.variance = Param("variance", variance)
        self.lengthscale = Param("lengthscale", lengthscale)
        assert self.variance.size == 1
        self.link_parameters(self.variance, self.lengthscale)

    def _theta(self):
        return _lib.theta_vec(self.variance.values, self.lengthscale.values, self.ARD, self.input_dim)

    def Kdiag(self, X):
        """(reference `stationary.py:170-173`)"""
        return _lib.kern_Kdiag(self.kind, self._theta(), np.asarray(X).shape[0])

    def _install_gradients(self, g):
        self.variance.gradient = g[0]
        self.lengthscale.gradient = g[1:] if self.ARD else g[1]

    def update_gradients_diag(self, dL_dKdiag, X):
        """(reference `stationary.py:182-191`)"""
        self.variance.gradient = np.sum(dL_dKdiag)
        self.lengthscale.gradient = 0.

    def update_gradients_direct(self, dL_dVar, dL_dLen):
        """install gradients computed elsewhere (reference `stationary.py:215-223`)"""
        self.variance.gradient = dL_dVar
        self.lengthscale.gradient = dL_dLen

    def input_sensitivity(self, summarize=True):
        """variance / lengthscale^2 per input dimension (reference `stationary.py:363-364`)"""
        return float(self.variance.values[0]) * np.ones(self.input_dim) / np.asarray(self.lengthscale.values) ** 2

    def reset_gradients(self):
        self.variance.gradient = 0.
        self.lengthscale.gradient = np.zeros(self.input_dim) if self.ARD else 0.

    def to_dict(self):
        """(reference `stationary.py:83-88`)"""
        d = super(Stationary, self).to_dict()
        d.update(variance=self.variance.values.tolist(), lengthscale=self.lengthscale.values.tolist(), ARD=self.ARD,
                 useGPU=True)
        return d


class RBF(Stationary):
    """k(r) = variance * exp(-r^2/2)  (reference `GPy/kern/src/rbf.py:51-52`); `inv_l=True` re-parameterises by
    the inverse squared lengthscale exactly like the reference (`rbf.py:29-33,328-330,373-375`)."""
    kind = "rbf"
    _gpy_class = "GPy.kern.RBF"

    def __init__(self, input_dim, variance=1., lengthscale=None, ARD=False, active_dims=None, name="rbf",
                 useGPU=True, inv_l=False, device=0):
        super(RBF, self).__init__(input_dim, variance, lengthscale, ARD, active_dims, name, useGPU, device)
        self.use_invLengthscale = bool(inv_l)
        if self.use_invLengthscale:
            self.unlink_parameter(self.lengthscale)
            self.inv_l = Param("inv_lengthscale", 1. / self.lengthscale.values ** 2)
            self.link_parameter(self.inv_l)

    def parameters_changed(self):
        if self.use_invLengthscale:
            self.lengthscale[:] = 1. / np.sqrt(self.inv_l.values + 1e-200)

    def get_one_dimensional_kernel(self, dim):
        """the per-dimension kernel of grid regression (reference `rbf.py:333-338`)"""
        return GridRBF(input_dim=1, variance=self.variance.values.copy(), originalDimensions=dim)

    def _install_gradients(self, g):
        super(RBF, self)._install_gradients(g)
        if self.use_invLengthscale:
            self.inv_l.gradient = self.lengthscale.gradient * (self.lengthscale.values ** 3 / -2.)

    def update_gradients_diag(self, dL_dKdiag, X):
        super(RBF, self).update_gradients_diag(dL_dKdiag, X)
        if self.use_invLengthscale:
            self.inv_l.gradient = self.lengthscale.gradient * (self.lengthscale.values ** 3 / -2.)

    # ---- psi-statistics for Gaussian inputs qX = NormalPosterior (reference `rbf.py:344-367`, `psi_comp/rbf_psi_comp.py`) and,
    # chosen by the type of qX, for a SpikeAndSlabPosterior (`psi_comp/ssrbf_psi_comp.py`; C-ABI mi355gp_ssrbf_psi / _grad) ----
    def _psi_operands(self, Z, qX):
        return self._slice_X(Z), self._slice_X(qX.mean), self._slice_X(qX.variance)

    def _ss_operands(self, Z, qX):
        return self._psi_operands(Z, qX) + (self._slice_X(qX.binary_prob),)

    def psi0(self, Z, qX):
        return np.full(qX.mean.shape[0], float(self.variance.values[0]))

    def psi1(self, Z, qX):
        if isinstance(qX, SpikeAndSlabPosterior):
            return _lib.ssrbf_psi(self.variance.values, self.lengthscale.values, self.ARD, *self._ss_operands(Z, qX),
                                  want_psi2=False, device=self.device)[0]
        Zs, mu, S = self._psi_operands(Z, qX)
        return _lib.rbf_psi(self.variance.values, self.lengthscale.values, self.ARD, Zs, mu, S, want_psi2=False,
                            device=self.device)[0]

    def psi2(self, Z, qX):
        if isinstance(qX, SpikeAndSlabPosterior):
            return _lib.ssrbf_psi(self.variance.values, self.lengthscale.values, self.ARD, *self._ss_operands(Z, qX),
                                  want_psi1=False, device=self.device)[1]
        Zs, mu, S = self._psi_operands(Z, qX)
        return _lib.rbf_psi(self.variance.values, self.lengthscale.values, self.ARD, Zs, mu, S, want_psi1=False,
                            device=self.device)[1]

    def psi2n(self, Z, qX):
        """N x M x M ON THE HOST for a foreign consumer that wants the summands; the inference path never forms it.
        The cost is O(N) C-ABI calls: every row validates, uploads Z and allocates its buffers again (the device kernel has no
        per-row output mode yet)."""
        if isinstance(qX, SpikeAndSlabPosterior):
            raise NotImplementedError("RBF.psi2n: the per-point psi2 of a SpikeAndSlabPosterior is not implemented (the reference's "
                                      "ssrbf_psi_comp has no return_psi2_n either)")
        Zs, mu, S = self._psi_operands(Z, qX)
        return np.stack([_lib.rbf_psi(self.variance.values, self.lengthscale.values, self.ARD, Zs, mu[n:n + 1], S[n:n + 1],
                                      want_psi1=False, device=self.device)[1] for n in range(mu.shape[0])])

    def _psi_grad(self, dL_dpsi0, dL_dpsi1, dL_dpsi2, Z, qX):
        if dL_dpsi2 is not None and np.ndim(dL_dpsi2) != 2:
            raise NotImplementedError("RBF psi gradients take dL_dpsi2 as M x M (the summed psi2), not per data point")
        if isinstance(qX, SpikeAndSlabPosterior):
            return _lib.ssrbf_psi_grad(self.variance.values, self.lengthscale.values, self.ARD, *self._ss_operands(Z, qX),
                                       dL_dpsi0=dL_dpsi0, dL_dpsi1=dL_dpsi1, dL_dpsi2=dL_dpsi2, device=self.device)
        Zs, mu, S = self._psi_operands(Z, qX)
        return _lib.rbf_psi_grad(self.variance.values, self.lengthscale.values, self.ARD, Zs, mu, S, dL_dpsi0, dL_dpsi1,
                                 dL_dpsi2, device=self.device)

    def _scatter(self, g, like):
        if g.shape == np.shape(like):
            return g
        full = np.zeros(np.shape(like))
        full[:, self.active_dims] = g
        return full

    def update_gradients_expectations(self, dL_dpsi0, dL_dpsi1, dL_dpsi2, Z, qX):
        dvar, dl = self._psi_grad(dL_dpsi0, dL_dpsi1, dL_dpsi2, Z, qX)[:2]
        self._install_gradients(np.concatenate([[dvar], dl]))

    def gradients_Z_expectations(self, dL_dpsi0, dL_dpsi1, dL_dpsi2, Z, qX):
        return self._scatter(self._psi_grad(dL_dpsi0, dL_dpsi1, dL_dpsi2, Z, qX)[2], Z)

    def gradients_qX_expectations(self, dL_dpsi0, dL_dpsi1, dL_dpsi2, Z, qX):
        g = self._psi_grad(dL_dpsi0, dL_dpsi1, dL_dpsi2, Z, qX)
        return tuple(self._scatter(x, qX.mean) for x in g[3:])        # (dmean, dvariance[, dbinary_prob])

    def to_dict(self):
        d = super(RBF, self).to_dict()
        d["inv_l"] = self.use_invLengthscale
        return d


class GridRBF(object):
    """One dimension's factor of an RBF on a Cartesian grid (reference `GPy/kern/src/grid_kerns.py:11-76`): an RBF on one
    column with variance^(1 / originalDimensions), so that the Kronecker product over the D dimensions carries the variance once.
    Host NumPy on G_d x G_d matrices: `GaussianGridInference` builds them per evaluation, the device never sees X.  Not a `Kern`:
    it has no parameters of its own to optimise (`lengthscale` is set by the caller per dimension, as the reference does)."""

    def __init__(self, input_dim=1, variance=1., lengthscale=None, ARD=False, active_dims=None, name="gridRBF",
                 originalDimensions=1, useGPU=False):
        assert int(input_dim) == 1 and not ARD, "GridRBF is the one-dimensional factor of a grid kernel"
        self.input_dim, self.name, self.originalDimensions = 1, name, int(originalDimensions)
        self.variance = float(np.ravel(np.asarray(variance, dtype=np.float64))[0])
        self.lengthscale = 1.0 if lengthscale is None else float(np.ravel(np.asarray(lengthscale, dtype=np.float64))[0])

    def _scaled_dist(self, X, X2=None):
        X = np.asarray(X, dtype=np.float64).reshape(-1, 1)
        X2 = X if X2 is None else np.asarray(X2, dtype=np.float64).reshape(-1, 1)
        return np.abs(X - X2.T) / float(np.ravel(self.lengthscale)[0])

    def K_of_r(self, r):
        return (self.variance ** (float(1) / self.originalDimensions)) * np.exp(-0.5 * r ** 2)

    def K(self, X, X2=None):
        return self.K_of_r(self._scaled_dist(X, X2))

    def dKdVar_of_r(self, r):
        return np.exp(-0.5 * r ** 2)

    def dKdLen_of_r(self, r, dimCheck, lengthscale):
        """(reference `grid_kerns.py:64-73`): the factor of dimension d in d K / d lengthscale_t, with r^2 where d is t"""
        k = (self.variance ** (float(1) / self.originalDimensions)) * np.exp(-0.5 * r ** 2)
        lengthscale = float(np.ravel(lengthscale)[0])
        if dimCheck:
            return k * (r ** 2) / (lengthscale ** (float(1) / self.originalDimensions))
        return k / (lengthscale ** (float(1) / self.originalDimensions))

    def dKd_dVar(self, X, X2=None):
        return self.dKdVar_of_r(self._scaled_dist(X, X2))

    def dKd_dLen(self, X, dimension, lengthscale, X2=None):
        return self.dKdLen_of_r(self._scaled_dist(X, X2), dimension, lengthscale)


class ExpQuad(Stationary):
    """The exponentiated quadratic k(r) = variance * exp(-r^2/2) (reference `stationary.py:623-662`): the same
    function as `RBF` without the psi-statistics / `inv_l` extras; serialises as "GPy.kern.ExpQuad"."""
    kind = "rbf"
    _gpy_class = "GPy.kern.ExpQuad"

    def __init__(self, input_dim, variance=1., lengthscale=None, ARD=False, active_dims=None, name="ExpQuad", **kw):
        super(ExpQuad, self).__init__(input_dim, variance, lengthscale, ARD, active_dims, name, **kw)


class Matern52(Stationary):
    """k(r) = variance (1 + sqrt5 r + 5/3 r^2) exp(-sqrt5 r)  (reference `stationary.py:585-589`)."""
    kind = "matern52"
    _gpy_class = "GPy.kern.Matern52"

    def __init__(self, input_dim, variance=1., lengthscale=None, ARD=False, active_dims=None, name="Mat52", **kw):
        super(Matern52, self).__init__(input_dim, variance, lengthscale, ARD, active_dims, name, **kw)


class Matern32(Stationary):
    """k(r) = variance (1 + sqrt3 r) exp(-sqrt3 r)  (reference `stationary.py:488-492`)."""
    kind = "matern32"
    _gpy_class = "GPy.kern.Matern32"

    def __init__(self, input_dim, variance=1., lengthscale=None, ARD=False, active_dims=None, name="Mat32", **kw):
        super(Matern32, self).__init__(input_dim, variance, lengthscale, ARD, active_dims, name, **kw)


class Exponential(Stationary):
    """k(r) = variance exp(-r)  (reference `stationary.py:382-386`)."""
    kind = "exponential"
    _gpy_class = "GPy.kern.Exponential"

    def __init__(self, input_dim, variance=1., lengthscale=None, ARD=False, active_dims=None, name="Exponential", **kw):
        super(Exponential, self).__init__(input_dim, variance, lengthscale, ARD, active_dims, name, **kw)


class OU(Exponential):
    """Ornstein-Uhlenbeck = the exponential kernel under its other name (reference `stationary.py:416-454`)."""
    _gpy_class = "GPy.kern.OU"

    def __init__(self, input_dim, variance=1., lengthscale=None, ARD=False, active_dims=None, name="OU", **kw):
        super(OU, self).__init__(input_dim, variance, lengthscale, ARD, active_dims, name, **kw)


class RatQuad(Stationary):
    """Rational quadratic k(r) = variance (1 + r^2/2)^-power (reference `stationary.py:747-802`): the stationary
    machinery plus a third parameter, `power`, linked after the lengthscale (`:757-760`) and reduced on the device in
    the same gradient pass (`dK/dpower = -K log1p(r^2/2)`, `:790-798`)."""
    kind = "ratquad"
    _gpy_class = "GPy.kern.RatQuad"

    def __init__(self, input_dim, variance=1., lengthscale=None, power=2., ARD=False, active_dims=None, name="RatQuad",
                 **kw):
        super(RatQuad, self).__init__(input_dim, variance, lengthscale, ARD, active_dims, name, **kw)
        self.power = Param("power", power)
        assert self.power.size == 1
        self.link_parameter(self.power)

    def _theta(self):
        return np.concatenate([super(RatQuad, self)._theta(), [float(self.power.values[0])]])

    def _install_gradients(self, g):
        super(RatQuad, self)._install_gradients(g[:-1])
        self.power.gradient = g[-1]

    def update_gradients_diag(self, dL_dKdiag, X):
        """(reference `stationary.py:800-802`)"""
        super(RatQuad, self).update_gradients_diag(dL_dKdiag, X)
        self.power.gradient = 0.

    def reset_gradients(self):
        super(RatQuad, self).reset_gradients()
        self.power.gradient = 0.

    def to_dict(self):
        d = super(RatQuad, self).to_dict()
        d["power"] = self.power.values.tolist()
        return d


class Cosine(Stationary):
    """k(r) = variance cos r  (reference `stationary.py:664-680`).  Positive definite over one input dimension only:
    give it one active column, alone or times a kernel on the others (`RBF * Cosine`: the locally periodic kernel)."""
    kind = "cosine"
    _gpy_class = "GPy.kern.Cosine"

    def __init__(self, input_dim, variance=1., lengthscale=None, ARD=False, active_dims=None, name="Cosine", **kw):
        super(Cosine, self).__init__(input_dim, variance, lengthscale, ARD, active_dims, name, **kw)


class Sinc(Stationary):
    """k(r) = variance sinc(2 r) = variance sin(2 pi r) / (2 pi r)  (reference `stationary.py:717-743`): the band-limited
    prior.  One active column, as `Cosine`."""
    kind = "sinc"
    _gpy_class = "GPy.kern.Sinc"

    def __init__(self, input_dim, variance=1., lengthscale=None, ARD=False, active_dims=None, name="Sinc", **kw):
        super(Sinc, self).__init__(input_dim, variance, lengthscale, ARD, active_dims, name, **kw)


class ExpQuadCosine(Stationary):
    """k(r) = variance exp(-2 pi^2 r^2) cos(2 pi r / period), one component of the spectral-mixture kernel of Wilson and
    Adams 2013 (reference `stationary.py:682-713`): the stationary machinery plus a third parameter, `period`, linked
    after the lengthscale (`:692-695`) and reduced on the device in the same gradient pass (`:703-709`).  One active
    column, as `Cosine`; a sum of these learns periodicities from data."""
    kind = "expquadcosine"
    _gpy_class = "GPy.kern.ExpQuadCosine"

    def __init__(self, input_dim, variance=1., lengthscale=None, period=1., ARD=False, active_dims=None,
                 name="ExpQuadCosine", **kw):
        super(ExpQuadCosine, self).__init__(input_dim, variance, lengthscale, ARD, active_dims, name, **kw)
        self.period = Param("period", period)
        assert self.period.size == 1
        self.link_parameter(self.period)

    def _theta(self):
        return np.concatenate([super(ExpQuadCosine, self)._theta(), [float(self.period.values[0])]])

    def _install_gradients(self, g):
        super(ExpQuadCosine, self)._install_gradients(g[:-1])
        self.period.gradient = g[-1]

    def update_gradients_diag(self, dL_dKdiag, X):
        """(reference `stationary.py:711-713`)"""
        super(ExpQuadCosine, self).update_gradients_diag(dL_dKdiag, X)
        self.period.gradient = 0.

    def reset_gradients(self):
        super(ExpQuadCosine, self).reset_gradients()
        self.period.gradient = 0.

    def to_dict(self):
        d = super(ExpQuadCosine, self).to_dict()
        d["period"] = self.period.values.tolist()
        return d


class StdPeriodic(Kern):
    """Standard periodic kernel k(x, y) = variance exp(-1/2 sum_q (sin(pi (x_q - y_q) / T_q) / l_q)^2) (reference
    `GPy/kern/src/standard_periodic.py:15-133`).  Not stationary in GPy's class sense (no function of r), but it runs
    on the same device paths: its own K-build and gradient kernels (C-ABI kind `MI355GP_STDPERIODIC`) and a row
    reduction for `gradients_X`.  Parameters are linked as in the reference: variance, period, lengthscale; `ARD1` /
    `ARD2` give one period / lengthscale per input dimension."""
    kind = "stdperiodic"
    _gpy_class = "GPy.kern.StdPeriodic"

    def __init__(self, input_dim, variance=1., period=None, lengthscale=None, ARD1=False, ARD2=False, active_dims=None,
                 name="std_periodic", useGPU=True, device=0):
        super(StdPeriodic, self).__init__(input_dim, active_dims, name, device)
        self.ARD1, self.ARD2 = bool(ARD1), bool(ARD2)          # standard_periodic.py:56-88
        if not self.ARD1:
            if period is not None:
                period = np.asarray(period, dtype=float)
                assert period.size == 1, "Only one period needed for non-ARD kernel"
            else:
                period = np.ones(1)
        else:
            if period is not None:
                period = np.asarray(period, dtype=float)
                assert period.size == self.input_dim, "bad number of periods"
            else:
                period = np.ones(self.input_dim)
        if not self.ARD2:
            if lengthscale is not None:
                lengthscale = np.asarray(lengthscale, dtype=float)
                assert lengthscale.size == 1, "Only one lengthscale needed for non-ARD kernel"
            else:
                lengthscale = np.ones(1)
        else:
            if lengthscale is not None:
                lengthscale = np.asarray(lengthscale, dtype=float)
                assert lengthscale.size == self.input_dim, "bad number of lengthscales"
            else:
                lengthscale = np.ones(self.input_dim)
        self.variance = Param("variance", variance)
        assert self.variance.size == 1, "Variance size must be one"
        self.period = Param("period", period)
        self.lengthscale = Param("lengthscale", lengthscale)
        self.link_parameters(self.variance, self.period, self.lengthscale)

    @property
    def ARD(self):
        """the C-ABI's `ard` of this kind: bit 0 = ARD1, bit 1 = ARD2"""
        return int(self.ARD1) | (int(self.ARD2) << 1)

    def _theta(self):
        return np.concatenate([[float(self.variance.values[0])], np.asarray(self.period.values, dtype=float).ravel(),
                               np.asarray(self.lengthscale.values, dtype=float).ravel()])

    def Kdiag(self, X):
        """the variance (reference `standard_periodic.py:135-139`)"""
        return _lib.kern_Kdiag(self.kind, self._theta(), np.asarray(X).shape[0])

    def _install_gradients(self, g):
        npr = self.period.size
        self.variance.gradient = g[0]
        self.period.gradient = g[1:1 + npr] if self.ARD1 else g[1]
        self.lengthscale.gradient = g[1 + npr:] if self.ARD2 else g[1 + npr]

    def update_gradients_diag(self, dL_dKdiag, X):
        """(reference `standard_periodic.py:536-540`)"""
        self.variance.gradient = np.sum(dL_dKdiag)
        self.period.gradient = 0.
        self.lengthscale.gradient = 0.

    def reset_gradients(self):
        self.variance.gradient = 0.
        self.period.gradient = np.zeros(self.input_dim) if self.ARD1 else 0.
        self.lengthscale.gradient = np.zeros(self.input_dim) if self.ARD2 else 0.

    def input_sensitivity(self, summarize=True):
        """(reference `standard_periodic.py:585-586`)"""
        return float(self.variance.values[0]) * np.ones(self.input_dim) / np.asarray(self.lengthscale.values) ** 2

    def to_dict(self):
        """(reference `standard_periodic.py:96-111`)"""
        d = super(StdPeriodic, self).to_dict()
        d.update(variance=self.variance.values.tolist(), period=self.period.values.tolist(),
                 lengthscale=self.lengthscale.values.tolist(), ARD1=self.ARD1, ARD2=self.ARD2, useGPU=True)
        return d


class Coregionalize(Kern):
    """Coregionalization kernel k(x, x') = B[x, x'] over an input column of integer output indices, B = W W^T + diag(kappa)
    (reference `GPy/kern/src/coregionalize.py:15-157`).  On the device it is C-ABI kind `MI355GP_COREGIONALIZE`: a factor
    of the product terms that `util.multioutput.ICM` / `LCM` build, assembled in the K-build and reduced by the bucketed
    gradient pass into S (P x P), which `_install_gradients` turns into dkappa = diag(S), dW = (S + S^T) W (`:110-128`).
    W is linked untransformed (`positive=False`), kappa positive, in the reference's order."""
    kind = "coregionalize"
    _gpy_class = "GPy.kern.Coregionalize"
    fused_alone = False
    diag_is_constant = False

    def __init__(self, input_dim, output_dim, rank=1, W=None, kappa=None, active_dims=None, name="coregion", device=0):
        assert int(input_dim) == 1, "Coregionalize acts on one input column (the output index): input_dim must be 1"
        assert active_dims is None or np.size(active_dims) == 1, "Coregionalize takes one active dimension"
        super(Coregionalize, self).__init__(1, active_dims, name, device)
        self.output_dim = int(output_dim)
        self.rank = int(rank)
        if self.rank > self.output_dim:
            print("Warning: Unusual choice of rank, it should normally be less than the output_dim.")
        if W is None:
            W = 0.5 * np.random.randn(self.output_dim, self.rank) / np.sqrt(self.rank)
        else:
            W = np.asarray(W, dtype=float)
            assert W.shape == (self.output_dim, self.rank)
        if kappa is None:
            kappa = 0.5 * np.ones(self.output_dim)
        else:
            kappa = np.asarray(kappa, dtype=float)
            assert kappa.shape == (self.output_dim,)
        self.W = Param("W", W, positive=False)
        self.kappa = Param("kappa", kappa)
        self.link_parameters(self.W, self.kappa)
        self.parameters_changed()

    @property
    def ARD(self):
        """the C-ABI's `ard` of this kind: the number of outputs P"""
        return self.output_dim

    def parameters_changed(self):
        """(reference `coregionalize.py:80-81`)"""
        self.B = np.dot(self.W.values, self.W.values.T) + np.diag(self.kappa.values)

    def _theta(self):
        """B, P x P row-major, symmetrised (W / kappa may have been edited in place since the last parameters_changed)"""
        Wv = self.W.values
        B = np.dot(Wv, Wv.T) + np.diag(self.kappa.values)
        return (0.5 * (B + B.T)).ravel()

    def _slice_X(self, X):
        X = np.asarray(X)
        return _lib.f64(X[:, self.active_dims])                   # [-1]: the last column (test_kernel.py:864)

    def Kdiag(self, X):
        """diag(B)[idx] (reference `coregionalize.py:106-107`): O(N) host work"""
        idx = self._index(self._slice_X(X))
        return np.diag(self._theta().reshape(self.output_dim, self.output_dim))[idx]

    def _index(self, Xs):
        v = np.asarray(Xs).ravel()
        idx = v.astype(np.int_)
        if not np.all((idx == v) & (idx >= 0) & (idx < self.output_dim)):
            bad = v[~((idx == v) & (idx >= 0) & (idx < self.output_dim))][0]
            raise ValueError("Coregionalize: output index %r is not an integer in [0, %d)" % (bad, self.output_dim))
        return idx

    def _install_gradients(self, g):
        """(reference `coregionalize.py:109-128`) the device reduces dL_dK -- in the fused inference call's bucketed pass, or a
        rectangular reduction of a given dL_dK -- to S (P x P, S[a][b] = sum of dL_dK over rows of output a and columns of
        output b) -> dkappa = diag(S), dW = (S + S^T) W (`:123-128`; its dL_dK_small is S^T)"""
        S = np.asarray(g, dtype=float).reshape(self.output_dim, self.output_dim)
        self.kappa.gradient = np.diag(S).copy()
        self.W.gradient = np.dot(S + S.T, self.W.values)

    def update_gradients_diag(self, dL_dKdiag, X):
        """(reference `coregionalize.py:145-151`)"""
        idx = self._index(self._slice_X(X))
        small = np.bincount(idx, weights=np.asarray(dL_dKdiag, dtype=float).ravel(), minlength=self.output_dim)
        self.W.gradient = 2.0 * self.W.values * small[:, None]
        self.kappa.gradient = small

    def reset_gradients(self):
        self.W.gradient = 0.
        self.kappa.gradient = 0.

    def gradients_X(self, dL_dK, X, X2=None):
        """(reference `coregionalize.py:153-154`)"""
        return np.zeros(np.asarray(X).shape)

    def to_dict(self):
        """(reference `coregionalize.py:159-174`)"""
        d = super(Coregionalize, self).to_dict()
        d.update(useGPU=True, W=self.W.values.tolist(), kappa=self.kappa.values.tolist(), output_dim=self.output_dim)
        return d

    @classmethod
    def from_dict(cls, d):
        return super(Coregionalize, cls).from_dict(dict(d, W=np.array(d["W"]), kappa=np.array(d["kappa"])))


class Linear(Kern):
    """Linear kernel k(x, y) = sum_q variances_q x_q y_q (reference `GPy/kern/src/linear.py:13-114`).  Not stationary: the
    diagonal K(x, x) = sum_q variances_q x_q^2 depends on the point.  On the device it is C-ABI kind `MI355GP_LINEAR`: a
    dot-product K-build and gradient pass of its own, alone, in `Add` and as a `Prod` factor; `Kdiag` and the diagonal
    gradients are O(N D) host arithmetic.  One parameter, `variances` (one value, or one per input dimension with `ARD`)."""
    kind = "linear"
    _gpy_class = "GPy.kern.Linear"
    diag_is_constant = False

    def __init__(self, input_dim, variances=None, ARD=False, active_dims=None, name="linear", useGPU=True, device=0):
        super(Linear, self).__init__(input_dim, active_dims, name, device)
        self.ARD = bool(ARD)
        if not self.ARD:                                               # linear.py:37-48
            if variances is not None:
                variances = np.asarray(variances, dtype=float)
                assert variances.size == 1, "Only one variance needed for non-ARD kernel"
            else:
                variances = np.ones(1)
        else:
            if variances is not None:
                variances = np.asarray(variances, dtype=float)
                assert variances.size == self.input_dim, "bad number of variances, need one ARD variance per input_dim"
            else:
                variances = np.ones(self.input_dim)
        self.variances = Param("variances", variances)
        self.link_parameter(self.variances)

    def _theta(self):
        return np.asarray(self.variances.values, dtype=np.float64).ravel().copy()

    def Kdiag(self, X):
        """(reference `linear.py:84-85`)"""
        return np.sum(self._theta() * np.square(self._slice_X(X)), -1)

    def _install_gradients(self, g):
        self.variances.gradient = np.asarray(g, dtype=float).copy() if self.ARD else g[0]

    def update_gradients_diag(self, dL_dKdiag, X):
        """(reference `linear.py:100-105`)"""
        tmp = np.asarray(dL_dKdiag, dtype=float).ravel()[:, None] * self._slice_X(X) ** 2
        self.variances.gradient = tmp.sum(0) if self.ARD else np.atleast_1d(tmp.sum())

    def reset_gradients(self):
        self.variances.gradient = np.zeros(self.input_dim) if self.ARD else 0.

    def gradients_X_diag(self, dL_dKdiag, X):
        """(reference `linear.py:140-141`): 2 variances_q x_q dL_dKdiag, zero outside the active dimensions"""
        X = np.asarray(X, dtype=float)
        out = np.zeros(X.shape)
        out[:, self.active_dims] = 2. * self._theta() * np.asarray(dL_dKdiag, dtype=float).ravel()[:, None] * self._slice_X(X)
        return out

    def input_sensitivity(self, summarize=True):
        """(reference `linear.py:151-152`)"""
        return np.ones(self.input_dim) * self._theta()

    # ---- psi-statistics for Gaussian inputs qX = NormalPosterior (reference `linear.py:158-181`, `psi_comp/linear_psi_comp.py`):
    # plain NumPy on the host, the yardstick and the fallback of the device path (`psi_lin_bias=True` on the inference classes).
    # With v_q the variances, s_q = sum_n S_nq:  psi0_n = sum_q v_q (mu_nq^2 + S_nq),  psi1 = (mu v) Z^T,
    # psi2_n = psi1_n psi1_n^T + Z diag(v^2 S_n) Z^T
    def _psi_operands(self, Z, qX):
        v = self._theta() * np.ones(self.input_dim)
        return v, self._slice_X(Z), self._slice_X(qX.mean), self._slice_X(qX.variance)

    def psi0(self, Z, qX):
        v, _, mu, S = self._psi_operands(Z, qX)
        return np.sum(v * (np.square(mu) + S), 1)

    def psi1(self, Z, qX):
        v, Zs, mu, _ = self._psi_operands(Z, qX)
        return np.dot(mu * v, Zs.T)

    def psi2(self, Z, qX):
        v, Zs, mu, S = self._psi_operands(Z, qX)
        p1 = np.dot(mu * v, Zs.T)
        return np.dot(p1.T, p1) + np.dot(Zs * (v * v * S.sum(0)), Zs.T)

    def psi2n(self, Z, qX):
        v, Zs, mu, S = self._psi_operands(Z, qX)
        p1 = np.dot(mu * v, Zs.T)
        return p1[:, :, None] * p1[:, None, :] + np.einsum("mq,nq,oq->nmo", Zs, v * v * S, Zs)

    def _psi_grad(self, dL_dpsi0, dL_dpsi1, dL_dpsi2, Z, qX):
        """(dvariances per dimension, dZ, dmu, dS), the last three over the active columns"""
        if np.ndim(dL_dpsi2) != 2:
            raise NotImplementedError("Linear psi gradients take dL_dpsi2 as M x M (the summed psi2), not per data point")
        v, Zs, mu, S = self._psi_operands(Z, qX)
        d0, d1 = np.asarray(dL_dpsi0, dtype=float).ravel(), np.asarray(dL_dpsi1, dtype=float)
        E2 = np.asarray(dL_dpsi2, dtype=float)
        E2 = E2 + E2.T
        T = d1 + np.dot(np.dot(mu * v, Zs.T), E2)              # dL / d psi1, the psi1 psi1^T half of psi2 included
        TZ, EZ, s = np.dot(T, Zs), np.dot(E2, Zs), S.sum(0)
        ze = 0.5 * np.sum(Zs * EZ, 0)                          # diag(Z^T dL_dpsi2 Z)
        dv = np.dot(d0, np.square(mu) + S) + np.sum(mu * TZ, 0) + 2. * v * s * ze
        dZ = np.dot(T.T, mu * v) + v * v * s * EZ
        dmu = TZ * v + 2. * d0[:, None] * v * mu
        dS = v * v * ze + d0[:, None] * v
        return dv, dZ, dmu, dS

    def _scatter(self, g, like):
        if g.shape == np.shape(like):
            return g
        full = np.zeros(np.shape(like))
        full[:, self.active_dims] = g
        return full

    def update_gradients_expectations(self, dL_dpsi0, dL_dpsi1, dL_dpsi2, Z, qX):
        dv = self._psi_grad(dL_dpsi0, dL_dpsi1, dL_dpsi2, Z, qX)[0]
        self.variances.gradient = dv.copy() if self.ARD else np.atleast_1d(dv.sum())

    def gradients_Z_expectations(self, dL_dpsi0, dL_dpsi1, dL_dpsi2, Z, qX):
        return self._scatter(self._psi_grad(dL_dpsi0, dL_dpsi1, dL_dpsi2, Z, qX)[1], Z)

    def gradients_qX_expectations(self, dL_dpsi0, dL_dpsi1, dL_dpsi2, Z, qX):
        g = self._psi_grad(dL_dpsi0, dL_dpsi1, dL_dpsi2, Z, qX)
        return self._scatter(g[2], qX.mean), self._scatter(g[3], qX.mean)

    def to_dict(self):
        """(reference `linear.py:54-59`)"""
        d = super(Linear, self).to_dict()
        d.update(variances=self.variances.values.tolist(), ARD=self.ARD, useGPU=True)
        return d


class MLP(Kern):
    """Multi-layer-perceptron (arc-sine, neural-network) kernel (reference `GPy/kern/src/mlp.py:11-147`):

        k(x, y) = variance (2/pi) asin( (w.x.y + b) / sqrt((w.x.x + b + 1)(w.y.y + b + 1)) ),  w.x.y = sum_q w_q x_q y_q

    with `weight_variance` w (one value, or one per input dimension with `ARD`) and `bias_variance` b.  Not stationary: the
    diagonal depends on the point.  On the device it is C-ABI kind `MI355GP_MLP`: a K-build and a gradient pass of their own
    (`k_kbuild_dot`, `k_grad_dot`), alone, in `Add` and as a `Prod` factor; `gradients_X` is reduced on the device, `Kdiag` and
    the diagonal gradients are O(N D) host arithmetic.  Parameters in link order: `variance`, `weight_variance`,
    `bias_variance`."""
    kind = "mlp"
    _gpy_class = "GPy.kern.MLP"
    diag_is_constant = False

    def __init__(self, input_dim, variance=1., weight_variance=1., bias_variance=1., ARD=False, active_dims=None, name="mlp",
                 useGPU=True, device=0):
        super(MLP, self).__init__(input_dim, active_dims, name, device)
        self.ARD = bool(ARD)
        if self.ARD:                                                   # mlp.py:39-42
            wv = np.empty((self.input_dim,))
            wv[:] = weight_variance
            weight_variance = wv
        else:
            weight_variance = np.asarray(weight_variance, dtype=float)
            assert weight_variance.size == 1, "Only one weight variance needed for non-ARD kernel"
        self.variance = Param("variance", variance)
        self.weight_variance = Param("weight_variance", weight_variance)
        self.bias_variance = Param("bias_variance", bias_variance)
        assert self.variance.size == 1 and self.bias_variance.size == 1
        self.link_parameters(self.variance, self.weight_variance, self.bias_variance)

    def _theta(self):
        return np.concatenate([[float(self.variance.values[0])],
                               np.asarray(self.weight_variance.values, dtype=np.float64).ravel(),
                               [float(self.bias_variance.values[0])]])

    def _vwb(self):
        th = self._theta()
        return th[0], th[1:-1], th[-1]

    def _comp_prod(self, X):
        """p_i = sum_q w_q x_iq^2 + b over the active columns (reference `mlp.py:90-95`)"""
        _, w, b = self._vwb()
        return np.sum(w * np.square(self._slice_X(X)), -1) + b

    def Kdiag(self, X):
        """(reference `mlp.py:61-64`)"""
        p = self._comp_prod(X)
        return float(self.variance.values[0]) * (2. / np.pi) * np.arcsin(p / (p + 1.))

    def _install_gradients(self, g):
        self.variance.gradient = g[0]
        self.weight_variance.gradient = np.asarray(g[1:-1], dtype=float).copy() if self.ARD else g[1]
        self.bias_variance.gradient = g[-1]

    def _diag_common(self, dL_dKdiag, X):
        """cd_i of the diagonal forms (reference `mlp.py:133-139`)"""
        v, _, _ = self._vwb()
        p = self._comp_prod(X)
        g = np.asarray(dL_dKdiag, dtype=float).ravel()
        return v * (2. / np.pi) / (np.sqrt(1. - np.square(p / (p + 1.))) * np.square(p + 1.)) * g, p, g

    def update_gradients_diag(self, dL_dKdiag, X):
        """(reference `mlp.py:72-76,133-147`)"""
        v, w, b = self._vwb()
        cd, p, g = self._diag_common(dL_dKdiag, X)
        self.variance.gradient = np.sum(g * self.Kdiag(X)) / v
        if self.ARD:
            self.weight_variance.gradient = np.dot(cd, np.square(self._slice_X(X)))
        else:
            self.weight_variance.gradient = np.sum(cd * (p - b)) / w[0]
        self.bias_variance.gradient = np.sum(cd)

    def gradients_X_diag(self, dL_dKdiag, X):
        """(reference `mlp.py:86-88,147`): 2 cd_i w_q x_iq, zero outside the active dimensions"""
        _, w, _ = self._vwb()
        cd, _, _ = self._diag_common(dL_dKdiag, X)
        X = np.asarray(X, dtype=float)
        out = np.zeros(X.shape)
        out[:, self.active_dims] = 2. * cd[:, None] * w * self._slice_X(X)
        return out

    def reset_gradients(self):
        self.variance.gradient = 0.
        self.weight_variance.gradient = np.zeros(self.input_dim) if self.ARD else 0.
        self.bias_variance.gradient = 0.

    def to_dict(self):
        d = super(MLP, self).to_dict()
        d.update(variance=self.variance.values.tolist(), weight_variance=self.weight_variance.values.tolist(),
                 bias_variance=self.bias_variance.values.tolist(), ARD=self.ARD, useGPU=True)
        return d


class Poly(Kern):
    """Polynomial kernel k(x, y) = variance (scale x.y + bias)^order (reference `GPy/kern/src/poly.py:10-49`); `order` (a
    float >= 1) is fixed, not a parameter.  C-ABI kind `MI355GP_POLY`, evaluated by the same device kernels as `MLP`, alone,
    in `Add` and as a `Prod` factor.  As in the reference, `gradients_X`, `gradients_X_diag` and `update_gradients_diag` raise
    `NotImplementedError` (`:45-49`), so a model whose kernel holds a Poly leaf has no `predictive_gradients`."""
    kind = "poly"
    _gpy_class = "GPy.kern.Poly"
    diag_is_constant = False

    def __init__(self, input_dim, variance=1., scale=1., bias=1., order=3., active_dims=None, name="poly", useGPU=True,
                 device=0):
        super(Poly, self).__init__(input_dim, active_dims, name, device)
        self.ARD = False
        self.variance = Param("variance", variance)
        self.scale = Param("scale", scale)
        self.bias = Param("bias", bias)
        assert self.variance.size == 1 and self.scale.size == 1 and self.bias.size == 1
        self.link_parameters(self.variance, self.scale, self.bias)
        assert order >= 1, "The order of the polynomial has to be at least 1."          # poly.py:22
        self.order = float(order)

    def _theta(self):
        """[variance, scale, bias, order]: the order travels with the parameters and has no gradient"""
        return np.array([float(self.variance.values[0]), float(self.scale.values[0]), float(self.bias.values[0]), self.order])

    def Kdiag(self, X):
        """(reference `poly.py:33-34`: the diagonal of K) variance (scale |x|^2 + bias)^order"""
        v, a, c0, order = self._theta()
        return v * (a * np.sum(np.square(self._slice_X(X)), -1) + c0) ** order

    def _install_gradients(self, g):
        self.variance.gradient, self.scale.gradient, self.bias.gradient = g[0], g[1], g[2]     # (g[3]: the order's slot, 0)

    def update_gradients_diag(self, dL_dKdiag, X):
        raise NotImplementedError("Poly has no update_gradients_diag (reference `poly.py:45-46`)")

    def gradients_X(self, dL_dK, X, X2=None):
        raise NotImplementedError("Poly has no gradients_X (reference `poly.py:47-48`), so an expression with a Poly leaf has "
                                  "no predictive_gradients either")

    def gradients_X_diag(self, dL_dKdiag, X):
        raise NotImplementedError("Poly has no gradients_X_diag (reference `poly.py:49-50`)")

    def reset_gradients(self):
        self.variance.gradient = self.scale.gradient = self.bias.gradient = 0.

    def to_dict(self):
        d = super(Poly, self).to_dict()
        d.update(variance=self.variance.values.tolist(), scale=self.scale.values.tolist(), bias=self.bias.values.tolist(),
                 order=self.order, useGPU=True)
        return d


# kernels the exact-GP device path evaluates as one part (the fused inference call takes them alone or in Add / Prod)
DEVICE_KERNELS = (Stationary, StdPeriodic, Linear, MLP, Poly)
# kinds the exact path alone evaluates in full: the grid path rejects every one of them, the sparse path all but Linear
EXACT_ONLY_KINDS = ("ratquad", "stdperiodic", "coregionalize", "linear", "mlp", "poly", "cosine", "sinc", "expquadcosine")
# ... of which the sparse path (certain inputs, one device) takes Linear where it is asked to (`linear=True` on the inference
# class): its Kdiag travels by point
SPARSE_REFUSED_KINDS = tuple(k for k in EXACT_ONLY_KINDS if k != "linear")


def has_coregionalize(kern):
    """True if the expression holds a Coregionalize part (its Kdiag then depends on the point)"""
    return any(isinstance(k, Coregionalize) for k in kern.leaves())


def diag_depends_on_point(kern):
    """True if Kdiag of the kernel or expression is not a constant: it holds a Coregionalize, Linear, MLP or Poly leaf"""
    return any(not k.diag_is_constant for k in kern.leaves())


def _spec_dims(f):
    dims = np.asarray(f.active_dims)
    if np.any(dims < 0):
        raise ValueError("%s: negative active_dims are resolved against X by the kernel alone; give a kernel inside Add / Prod "
                         "non-negative active_dims" % type(f).__name__)
    return dims


def exact_only_leaves(kern):
    """names of the kernels in `kern` (a foreign object has none) that only the exact-GP path evaluates"""
    return [type(k).__name__ for k in (kern.leaves() if isinstance(kern, Kern) else []) if k.kind in EXACT_ONLY_KINDS]


def sparse_refused_leaves(kern):
    """names of the kernels in `kern` that the sparse path does not evaluate (`SPARSE_REFUSED_KINDS`)"""
    return [type(k).__name__ for k in (kern.leaves() if isinstance(kern, Kern) else []) if k.kind in SPARSE_REFUSED_KINDS]


class Static(Kern):
    """White / Bias (reference `GPy/kern/src/static.py:10-60`): one `variance` parameter, no input dependence; K and its
    gradients are host arithmetic."""
    fused_alone = False

    def __init__(self, input_dim, variance=1., active_dims=None, name=None, device=0):
        super(Static, self).__init__(input_dim, active_dims, name or self.kind, device)
        self.ARD = False
        self.variance = Param("variance", variance)
        self.link_parameter(self.variance)

    def _theta(self):
        return np.array([float(self.variance.values[0])])

    def Kdiag(self, X):
        return np.full(np.asarray(X).shape[0], float(self.variance.values[0]))

    def update_gradients_diag(self, dL_dKdiag, X):
        self.variance.gradient = np.sum(dL_dKdiag)

    def _install_gradients(self, g):
        self.variance.gradient = g[0]

    def gradients_X(self, dL_dK, X, X2=None):
        return np.zeros(np.asarray(X).shape)

    def to_dict(self):
        d = super(Static, self).to_dict()
        d["variance"] = self.variance.values.tolist()
        return d


class White(Static):
    """(reference `static.py:63-98`): variance on the diagonal of K(X), zero cross-covariance."""
    kind = "white"
    _gpy_class = "GPy.kern.White"

    def K(self, X, X2=None):
        n = np.asarray(X).shape[0]
        return np.eye(n) * float(self.variance.values[0]) if X2 is None else np.zeros((n, np.asarray(X2).shape[0]))

    def update_gradients_full(self, dL_dK, X, X2=None):
        self.variance.gradient = np.trace(np.asarray(dL_dK)) if X2 is None else 0.

    # psi-statistics (reference `static.py:40-60,83-93`): psi0 = variance, psi1 = psi2 = 0
    def psi0(self, Z, qX):
        return np.full(qX.mean.shape[0], float(self.variance.values[0]))

    def psi1(self, Z, qX):
        return np.zeros((qX.mean.shape[0], np.asarray(Z).shape[0]))

    def psi2(self, Z, qX):
        return np.zeros((np.asarray(Z).shape[0],) * 2)

    def psi2n(self, Z, qX):
        return np.zeros((qX.mean.shape[0],) + (np.asarray(Z).shape[0],) * 2)

    def update_gradients_expectations(self, dL_dpsi0, dL_dpsi1, dL_dpsi2, Z, qX):
        self.variance.gradient = np.sum(dL_dpsi0)

    def gradients_Z_expectations(self, dL_dpsi0, dL_dpsi1, dL_dpsi2, Z, qX):
        return np.zeros(np.asarray(Z).shape)

    def gradients_qX_expectations(self, dL_dpsi0, dL_dpsi1, dL_dpsi2, Z, qX):
        return tuple(np.zeros(qX.mean.shape) for _ in range(3 if isinstance(qX, SpikeAndSlabPosterior) else 2))


class Bias(Static):
    """(reference `static.py:151-173`): constant covariance."""
    kind = "bias"
    _gpy_class = "GPy.kern.Bias"

    def K(self, X, X2=None):
        n = np.asarray(X).shape[0]
        return np.full((n, n if X2 is None else np.asarray(X2).shape[0]), float(self.variance.values[0]))

    def update_gradients_full(self, dL_dK, X, X2=None):
        self.variance.gradient = np.sum(np.asarray(dL_dK))

    # psi-statistics (reference `static.py:133-189`): psi0 = psi1 = variance, psi2_n = variance^2
    def psi0(self, Z, qX):
        return np.full(qX.mean.shape[0], float(self.variance.values[0]))

    def psi1(self, Z, qX):
        return np.full((qX.mean.shape[0], np.asarray(Z).shape[0]), float(self.variance.values[0]))

    def psi2(self, Z, qX):
        return np.full((np.asarray(Z).shape[0],) * 2, float(self.variance.values[0]) ** 2 * qX.mean.shape[0])

    def psi2n(self, Z, qX):
        return np.full((qX.mean.shape[0],) + (np.asarray(Z).shape[0],) * 2, float(self.variance.values[0]) ** 2)

    def update_gradients_expectations(self, dL_dpsi0, dL_dpsi1, dL_dpsi2, Z, qX):
        if np.ndim(dL_dpsi2) != 2:
            raise NotImplementedError("Bias psi gradients take dL_dpsi2 as M x M (the summed psi2), not per data point")
        self.variance.gradient = (np.sum(dL_dpsi0) + np.sum(dL_dpsi1)
                                  + 2. * float(self.variance.values[0]) * np.sum(dL_dpsi2) * qX.mean.shape[0])

    def gradients_Z_expectations(self, dL_dpsi0, dL_dpsi1, dL_dpsi2, Z, qX):
        return np.zeros(np.asarray(Z).shape)

    def gradients_qX_expectations(self, dL_dpsi0, dL_dpsi1, dL_dpsi2, Z, qX):
        return np.zeros(qX.mean.shape), np.zeros(qX.mean.shape)


class CombinationKernel(Kern):
    """Common part of `Add` and `Prod` (reference `GPy/kern/src/kern.py:363-451`): owns the parts, spans their input
    columns, and describes itself to the C-ABI as a list of parts with term ids (`mi355gp_part`)."""
    is_leaf = False

    def __init__(self, parts, name):
        super(CombinationKernel, self).__init__(max(int(p.active_dims.max()) + 1 for p in parts), None, name,
                                                parts[0].device)
        self.parts = parts
        for p in parts:
            self.link_parameter(p)

    def leaves(self):
        out = []
        for p in self.parts:
            out.extend(p.leaves())
        return out

    def _slice_X(self, X):
        return _lib.f64(np.asarray(X))

    def _refuse_poly_gradients_X(self):
        """a Poly leaf has no gradients_X (reference `poly.py:47-48`): raise its error before any part does device work"""
        for k in self.leaves():
            if isinstance(k, Poly):
                k.gradients_X(None, None)

    def to_dict(self):
        return {"class": self._gpy_class, "name": self.name, "parts": [p.to_dict() for p in self.parts]}

    @classmethod
    def from_dict(cls, d):
        raise NotImplementedError("%s.from_dict: build the parts with their own from_dict and combine them" % cls.__name__)

    def copy(self):
        return self.__class__([p.copy() for p in self.parts], name=self.name)

    def diag_variance(self):
        """Kdiag of the expression (a constant for stationary / static leaves; not meaningful when `diag_depends_on_point`)"""
        return float(self.Kdiag(np.zeros((1, self.input_dim)))[0])


class Add(CombinationKernel):
    """Sum of kernels (reference `GPy/kern/src/add.py:12-100`).  With `gpy_amd.ExactGaussianInference` the sum is
    assembled and differentiated on the device in the same fused call as a single kernel (C-ABI
    `mi355gp_exact_inference_sum`); parameter / gradient order = the parts' link order.  Parts may be `Prod`s."""
    _gpy_class = "GPy.kern.Add"

    def __init__(self, parts, name="sum"):
        flat = []
        for p in parts:
            flat.extend(p.parts if isinstance(p, Add) else [p])          # add.py:24-33 flattens nested sums
        assert all(getattr(p, "is_leaf", False) or isinstance(p, Prod) for p in flat), \
            "Add supports stationary, StdPeriodic, Linear, MLP, Poly, White, Bias, Coregionalize and Prod parts"
        super(Add, self).__init__(flat, name)

    def part_specs(self):
        """[(kind, ARD, theta, active_dims, term)] for the C-ABI (active_dims index the columns of the model's X);
        the factors of a `Prod` part share a non-zero term id."""
        specs, term = [], 0
        for p in self.parts:
            if isinstance(p, Prod):
                term += 1
                specs.extend((f.kind, f.ARD, f._theta(), _spec_dims(f), term) for f in p.parts)
            else:
                specs.append((p.kind, p.ARD, p._theta(), _spec_dims(p), 0))
        return specs

    def K(self, X, X2=None):
        out = None
        for p in self.parts:
            Kp = p.K(X, X2)
            out = Kp if out is None else out + Kp
        return out

    def Kdiag(self, X):
        return sum(p.Kdiag(X) for p in self.parts)

    def update_gradients_full(self, dL_dK, X, X2=None):
        """(reference `add.py:81-82`).  A device-resident dL_dK of the fused sum call carries every part's gradient."""
        if isinstance(dL_dK, DeviceResult) and X2 is None and dL_dK.matches_kernel(self):
            self._install_fused(dL_dK.fused_dtheta)
            return
        G = np.asarray(dL_dK)
        for p in self.parts:
            p.update_gradients_full(G, X, X2)

    def update_gradients_diag(self, dL_dKdiag, X):
        for p in self.parts:
            p.update_gradients_diag(dL_dKdiag, X)

    def gradients_X(self, dL_dK, X, X2=None):
        self._refuse_poly_gradients_X()
        G = np.asarray(dL_dK)
        return sum(p.gradients_X(G, X, X2) for p in self.parts)

    def gradients_X_diag(self, dL_dKdiag, X):                                    # add.py:102-105
        return sum(p.gradients_X_diag(dL_dKdiag, X) for p in self.parts)

    # ---- psi-statistics (reference `add.py:107-266`).  By default one RBF part and White parts only: White's psi1 is zero, so
    # the cross terms of psi2 vanish and every part sees the same dL_dpsi0/1/2.  `psi_lin_bias=True`: one input-dependent part,
    # RBF or Linear, with any number of Bias and White parts; Bias (b = the sum of their variances) crosses with the psi1 of
    # the input-dependent part:  psi2_n += b (psi1_n 1^T + 1 psi1_n^T) + b^2, and every part sees dL_dpsi1 plus the OTHER
    # parts' psi1 times (dL_dpsi2 + dL_dpsi2^T).  Two input-dependent parts stay refused (their cross term needs E[k1 k2^T]).
    def _psi_parts(self, psi_lin_bias=False, qX=None):
        how = "; Linear and Bias parts: pass psi_lin_bias=True"
        if isinstance(qX, SpikeAndSlabPosterior):                     # one RBF part and White parts, whatever the keyword says
            psi_lin_bias, how = False, " (spike-and-slab inputs: the Linear statistics, sslinear_psi_comp, are not implemented)"
        if psi_lin_bias:
            for p in self.parts:
                if type(p) not in (RBF, Linear, Bias, White):
                    what = type(p).__name__ if p.is_leaf else "%s of %s" % (type(p).__name__, ", ".join(type(f).__name__ for f in p.leaves()))
                    raise NotImplementedError("psi-statistics of a sum cover one RBF or Linear part with Bias and White parts; "
                                              "part %r is a %s" % (p.name, what))
            dep = [p for p in self.parts if isinstance(p, (RBF, Linear))]
            if len(dep) != 1:
                raise NotImplementedError("psi-statistics of a sum cover ONE input-dependent part (RBF or Linear; psi2 of two has "
                                          "cross terms that need E[k1 k2^T]), got %d (%s)"
                                          % (len(dep), ", ".join("%r: %s" % (p.name, type(p).__name__) for p in dep)))
            return self.parts
        for p in self.parts:
            if not isinstance(p, (RBF, White)):
                raise NotImplementedError("psi-statistics of a sum cover one RBF part and White parts; part %r is a %s%s"
                                          % (p.name, type(p).__name__, how))
        if sum(isinstance(p, RBF) for p in self.parts) > 1:
            raise NotImplementedError("psi-statistics of a sum cover ONE RBF part (psi2 of two has cross terms); part %r is "
                                      "a second RBF" % [p.name for p in self.parts if isinstance(p, RBF)][1])
        return self.parts

    def _bias_sum(self):
        return float(sum(float(p.variance.values[0]) for p in self.parts if isinstance(p, Bias)))

    def _dep_part(self):
        return [p for p in self.parts if isinstance(p, (RBF, Linear))][0]

    def psi0(self, Z, qX, psi_lin_bias=False):
        return sum(p.psi0(Z, qX) for p in self._psi_parts(psi_lin_bias, qX))

    def psi1(self, Z, qX, psi_lin_bias=False):
        return sum(p.psi1(Z, qX) for p in self._psi_parts(psi_lin_bias, qX))

    def psi2(self, Z, qX, psi_lin_bias=False):
        out = sum(p.psi2(Z, qX) for p in self._psi_parts(psi_lin_bias, qX))
        b = self._bias_sum() if psi_lin_bias else 0.0
        if b != 0.0:                                      # the pairs of Bias parts, and Bias against the input-dependent part
            c = self._dep_part().psi1(Z, qX).sum(0)
            n = qX.mean.shape[0]
            out = out + b * (c[:, None] + c[None, :]) + n * (b * b - sum(float(p.variance.values[0]) ** 2 for p in self.parts
                                                                         if isinstance(p, Bias)))
        return out

    def psi2n(self, Z, qX, psi_lin_bias=False):
        out = sum(p.psi2n(Z, qX) for p in self._psi_parts(psi_lin_bias, qX))
        b = self._bias_sum() if psi_lin_bias else 0.0
        if b != 0.0:
            p1 = self._dep_part().psi1(Z, qX)
            out = out + b * (p1[:, :, None] + p1[:, None, :]) + (b * b - sum(float(p.variance.values[0]) ** 2 for p in self.parts
                                                                            if isinstance(p, Bias)))
        return out

    def _psi1_eff(self, parts, dL_dpsi1, dL_dpsi2, Z, qX):
        """per part: dL_dpsi1 + (the other parts' psi1) (dL_dpsi2 + dL_dpsi2^T) (reference `add.py:147-266`)"""
        if not any(isinstance(p, Bias) for p in parts):
            return [dL_dpsi1] * len(parts)
        if np.ndim(dL_dpsi2) != 2:
            raise NotImplementedError("psi gradients of a sum take dL_dpsi2 as M x M (the summed psi2), not per data point")
        E2 = np.asarray(dL_dpsi2, dtype=float)
        E2 = E2 + E2.T
        p1 = [None if isinstance(p, White) else p.psi1(Z, qX) for p in parts]
        out = []
        for i, p in enumerate(parts):
            if isinstance(p, White):
                out.append(dL_dpsi1)
                continue
            others = [p1[j] for j in range(len(parts)) if j != i and p1[j] is not None]
            out.append(np.asarray(dL_dpsi1) + np.dot(sum(others), E2) if others else dL_dpsi1)
        return out

    def update_gradients_expectations(self, dL_dpsi0, dL_dpsi1, dL_dpsi2, Z, qX, psi_lin_bias=False):
        parts = self._psi_parts(psi_lin_bias, qX)
        for p, d1 in zip(parts, self._psi1_eff(parts, dL_dpsi1, dL_dpsi2, Z, qX)):
            p.update_gradients_expectations(dL_dpsi0, d1, dL_dpsi2, Z, qX)

    def gradients_Z_expectations(self, dL_dpsi0, dL_dpsi1, dL_dpsi2, Z, qX, psi_lin_bias=False):
        parts = self._psi_parts(psi_lin_bias, qX)
        return sum(p.gradients_Z_expectations(dL_dpsi0, d1, dL_dpsi2, Z, qX)
                   for p, d1 in zip(parts, self._psi1_eff(parts, dL_dpsi1, dL_dpsi2, Z, qX)))

    def gradients_qX_expectations(self, dL_dpsi0, dL_dpsi1, dL_dpsi2, Z, qX, psi_lin_bias=False):
        parts = self._psi_parts(psi_lin_bias, qX)
        gs = [p.gradients_qX_expectations(dL_dpsi0, d1, dL_dpsi2, Z, qX)
              for p, d1 in zip(parts, self._psi1_eff(parts, dL_dpsi1, dL_dpsi2, Z, qX))]
        return tuple(sum(g[i] for g in gs) for i in range(len(gs[0])))


class Prod(CombinationKernel):
    """Product of kernels (reference `GPy/kern/src/prod.py:24-99`; nested products are flattened, `:33-41`).  Fused on the
    device like `Add`: the factors share a term id of `mi355gp_part`, K is multiplied up factor by factor in the
    K-build kernel and each factor's gradient pass weights dL_dK by the other factors' covariances."""
    _gpy_class = "GPy.kern.Prod"

    def __init__(self, kernels, name="mul"):
        flat = []
        for k in kernels:
            flat.extend(k.parts if isinstance(k, Prod) else [k])
        assert all(getattr(k, "is_leaf", False) for k in flat), \
            "Prod supports stationary, StdPeriodic, Linear, MLP, Poly, White, Bias and Coregionalize factors"
        super(Prod, self).__init__(flat, name)

    def part_specs(self):
        return [(f.kind, f.ARD, f._theta(), _spec_dims(f), 1) for f in self.parts]

    def K(self, X, X2=None):                                                     # prod.py:58-65
        out = None
        for p in self.parts:
            Kp = p.K(X, X2)
            out = Kp if out is None else out * Kp
        return out

    def Kdiag(self, X):                                                          # prod.py:67-71
        out = None
        for p in self.parts:
            d = p.Kdiag(X)
            out = d if out is None else out * d
        return out

    def update_gradients_full(self, dL_dK, X, X2=None):
        """(reference `prod.py:86-99`): every factor sees dL_dK times the product of the other factors."""
        if isinstance(dL_dK, DeviceResult) and X2 is None and dL_dK.matches_kernel(self):
            self._install_fused(dL_dK.fused_dtheta)
            return
        G = np.asarray(dL_dK)
        Ks = [p.K(X, X2) for p in self.parts]
        for i, p in enumerate(self.parts):
            W = G
            for j, Kj in enumerate(Ks):
                if j != i:
                    W = W * Kj
            p.update_gradients_full(W, X, X2)

    def update_gradients_diag(self, dL_dKdiag, X):                               # prod.py:101-111
        ds = [p.Kdiag(X) for p in self.parts]
        for i, p in enumerate(self.parts):
            w = np.asarray(dL_dKdiag, dtype=float)
            for j, d in enumerate(ds):
                if j != i:
                    w = w * d
            p.update_gradients_diag(w, X)

    def gradients_X(self, dL_dK, X, X2=None):                                    # prod.py:113-121
        self._refuse_poly_gradients_X()
        G = np.asarray(dL_dK)
        Ks = [p.K(X, X2) for p in self.parts]
        out = 0.
        for i, p in enumerate(self.parts):
            W = G
            for j, Kj in enumerate(Ks):
                if j != i:
                    W = W * Kj
            out = out + p.gradients_X(W, X, X2)
        return out

    def gradients_X_diag(self, dL_dKdiag, X):
        """every factor sees dL_dKdiag times the other factors' diagonals (the product rule on `prod.py:67-71`)"""
        ds = [p.Kdiag(X) for p in self.parts]
        out = 0.
        for i, p in enumerate(self.parts):
            w = np.asarray(dL_dKdiag, dtype=float)
            for j, d in enumerate(ds):
                if j != i:
                    w = w * d
            out = out + p.gradients_X_diag(w, X)
        return out


KERNEL_CLASSES = {"rbf": RBF, "expquad": ExpQuad, "matern52": Matern52, "matern32": Matern32, "exponential": Exponential,
                  "white": White, "bias": Bias, "ratquad": RatQuad, "stdperiodic": StdPeriodic, "coregionalize": Coregionalize,
                  "linear": Linear, "mlp": MLP, "poly": Poly, "cosine": Cosine, "sinc": Sinc, "expquadcosine": ExpQuadCosine}
