"""GPy's `util` package on this path: `util.linalg` (the device factorisations) and `util.multioutput` (host bookkeeping)."""
from .. import linalg  # noqa: F401
from . import multioutput  # noqa: F401
