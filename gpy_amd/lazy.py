"""Lazy host views of the N x N results that stay resident in HBM.

GPy's contract hands `dL_dK` (N x N) from the inference method to the kernel and stores `woodbury_chol` / `K`
in the Posterior (reference `core/gp.py:278-280`, `exact_gaussian_inference.py:74`).  Shipping those over PCIe
every optimiser iteration would dominate the run, so the drop-in returns `DeviceResult` proxies: they behave
as arrays for foreign consumers (`np.asarray`, indexing, arithmetic -> one fetch, cached) while gpy_amd's own
kernels recognise them and never leave the device.
"""
import numpy as np

from . import _lib


def frozen(a):
    """True when nobody can write through `a` or any array it is a view of: every ndarray in its base chain is
    read-only and the chain ends in memory NumPy itself owns.  Only such arrays can be recognised by IDENTITY from one
    call to the next; GPy gets the same guarantee from `ObsAr` observers (reference `core/gp.py:44-60`)."""
    while isinstance(a, np.ndarray):
        if a.flags.writeable:
            return False
        a = a.base
    return a is None


def freeze(a):
    """A private, read-only float64 C-contiguous copy of `a` (what the model drivers keep as X / Y)."""
    b = np.array(a, dtype=np.float64, order="C", copy=True)
    b.setflags(write=False)
    return b


class ArrayIdentity(object):
    """Remembers one host array so that a later call can tell whether it was handed THE SAME DATA.
    A frozen array (see `frozen`) is remembered by object identity: O(1) per call, and it cannot have been edited in place.
    Anything else is remembered as a private copy and compared element by element (O(size), like paramz would re-run the
    computation for a plain ndarray): a sampled fingerprint can miss an in-place edit, identity of a writable buffer can
    alias a different array after the allocator reuses the address."""

    __slots__ = ("obj", "copy")

    def __init__(self, a):
        if a is None:
            self.obj = self.copy = None
        elif frozen(a):
            self.obj, self.copy = a, None
        else:
            self.obj, self.copy = None, np.array(a, copy=True)

    def matches(self, b):
        if b is None:
            return self.obj is None and self.copy is None
        if self.obj is not None:
            if b is self.obj and frozen(b):
                return True
            ref = self.obj
        elif self.copy is not None:
            ref = self.copy
        else:
            return False
        b = np.asarray(b)
        return ref.shape == b.shape and ref.dtype == b.dtype and np.array_equal(ref, b)

    def value(self):
        return self.obj if self.obj is not None else self.copy


class LazyArray(object):
    """The array protocol of a host view of a result that lives on the device: `np.asarray`, indexing, `.T`, `len`, arithmetic,
    `copy / sum / dot` and pickling all go through `fetch()`, which materialises once and keeps the host copy.
    A subclass supplies `shape`, `_materialise()` (the host array) and, unless the view belongs to a sparse session (`_bind`),
    `_current()`: is the result still the latest of its context?  `stale` is what a fetch after a later call raises."""
    __array_priority__ = 100.0
    ndim = 2
    dtype = np.dtype(np.float64)
    stale = "device-resident result overwritten by a later inference call"
    _host = None

    size = property(lambda self: self.shape[0] * self.shape[1])

    def _bind(self, session):
        """a view of the evaluation `session` (a `sparse.SparseSession`) has just run"""
        self._ctx, self._owner, self._token = session._ctx, session, session._token

    def _current(self):
        return self._owner._token == self._token

    def _require_current(self):
        if self._ctx is None:
            raise RuntimeError("this result was detached from its device context (unpickled) before being fetched")
        if not self._current():
            raise RuntimeError(self.stale)

    def fetch(self):
        if self._host is None:
            self._require_current()
            self._host = self._materialise()
        return self._host

    def __getstate__(self):
        """Pickling materialises the host copy (while the device still holds it) and drops the device handle."""
        d = dict(self.__dict__)
        if d.get("_host") is None:
            try:
                d["_host"] = self.fetch()
            except Exception:
                d["_host"] = None
        d["_ctx"] = None
        return d

    def __array__(self, dtype=None, copy=None):
        a = self.fetch()
        return a if dtype is None else a.astype(dtype, copy=False)

    def __getitem__(self, idx):
        return self.fetch()[idx]

    def __len__(self):
        return self.shape[0]

    @property
    def T(self):
        return self.fetch().T

    def copy(self):
        return self.fetch().copy()

    def sum(self, *a, **k):
        return self.fetch().sum(*a, **k)

    def dot(self, other):
        return self.fetch().dot(other)

    def __neg__(self):
        return -self.fetch()

    def __repr__(self):
        which = "which=%d, " % self._which if hasattr(self, "_which") else ""
        return "%s(%sshape=%r, %s)" % (type(self).__name__, which, self.shape,
                                       "materialised" if self._host is not None else "on device")


def _binop(name):
    def f(self, other):
        return getattr(self.fetch(), name)(other)
    return f


for _n in ("__add__", "__radd__", "__sub__", "__rsub__", "__mul__", "__rmul__", "__truediv__", "__rtruediv__",
           "__matmul__", "__rmatmul__"):
    setattr(LazyArray, _n, _binop(_n))


class DeviceResult(LazyArray):
    """One of the N x N results of an exact-path context (`inference._DeviceState`), `which` = `_lib.FETCH_*`."""
    stale = ("this device-resident result was overwritten by a later inference call; "
             "materialise it (np.asarray) before re-running inference")

    def __init__(self, ctx, which, n, token, fortran_order=False, kernel_sig=None, fused_dtheta=None):
        self._ctx, self._which, self._token = ctx, which, token    # token: a stale proxy must not read newer buffers
        self.shape = (n, n)
        self._fortran = fortran_order
        self._kernel_sig = kernel_sig
        self.fused_dtheta = fused_dtheta

    def matches_kernel(self, kern):
        return self.fused_dtheta is not None and self._kernel_sig == kernel_signature(kern)

    def _current(self):
        return self._ctx.call_token == self._token

    def _materialise(self):
        return self._ctx.fetch(self._which, fortran_order=self._fortran)


class LazyMM(LazyArray):
    """Lazy M x M result (`SparseContext.FETCH_*`) of a sparse session's last evaluation, times `scale` if one is given
    (dL_dpsi2 = beta * dL_dpsi2_beta, `var_dtc.py:220-233`)."""

    def __init__(self, session, which, M, scale=None):
        self._bind(session)
        self._which, self.shape, self._scale = which, (M, M), scale

    def _materialise(self):
        a = self._ctx.fetch(self._which)
        return a if self._scale is None else self._scale * a


class LazyNM(LazyArray):
    """dL_dKnm (N x M) of a sparse session's last evaluation.  It is never resident as a whole on the device (3.3 GB at
    N = 200000, M = 2048): gpy_amd's own model driver uses the reductions the device made from it (`grad_dict['fused']`); a
    FOREIGN consumer -- e.g. GPy's `SparseGP._update_gradients` handing it to `kern.update_gradients_full(dL_dKnm, X, Z)`
    (reference `core/sparse_gp.py:108-119`) -- gets it materialised in row blocks (`blocks()`), or entirely (`np.asarray`)."""

    def __init__(self, session, N, M, block=8192):
        self._bind(session)
        self.shape, self._block = (N, M), block

    def blocks(self, rows=None):
        """yields (row0, row1, dL_dKnm[row0:row1]) over the whole matrix"""
        self._require_current()
        step = rows or self._block
        for r0 in range(0, self.shape[0], step):
            r1 = min(self.shape[0], r0 + step)
            yield r0, r1, self._ctx.fetch_dL_dKnm(r0, r1 - r0)

    def _materialise(self):
        out = np.empty(self.shape)
        for r0, r1, B in self.blocks():
            out[r0:r1] = B
        return out


class LazyPsi1(LazyArray):
    """dL_dpsi1 = beta R v^T (N x M, reference `var_dtc.py:219`) of an uncertain-input call.  The device forms it on the fly
    inside the gradient kernels and never holds it; a foreign consumer gets the rank-Dy product from the host, formed anew
    for every use: the view holds host arrays only, is always current and keeps no N x M copy."""

    def __init__(self, beta, R, wv):
        self._beta, self._R, self._wv = beta, R, wv
        self.shape = (R.shape[0], wv.shape[0])

    def fetch(self):
        return self._beta * np.dot(self._R, self._wv.T)

    def __getstate__(self):
        return self.__dict__


def kernel_signature(kern):
    """Identity of a kernel evaluation: class, ARD flag, active dims and the exact parameter bits (per part for sums)."""
    parts = getattr(kern, "parts", None)
    if parts is not None:
        return (type(kern).__name__,) + tuple(kernel_signature(p) for p in parts)
    return (kern.kind, bool(kern.ARD), tuple(int(i) for i in kern.active_dims), kern._theta().tobytes())
