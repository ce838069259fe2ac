"""GPy's `util` package on this path: `util.linalg` (the device factorisations), `util.multioutput` and
`util.choleskies` (host bookkeeping), `util.initialization` / `util.pca` (latent initialisation)."""
from .. import linalg  # noqa: F401
from . import multioutput  # noqa: F401
from . import choleskies  # noqa: F401
from . import pca  # noqa: F401
from . import initialization  # noqa: F401
