"""`GPLVM`: the Gaussian-process latent variable model (reference `GPy/models/gplvm.py:11-49`) -- an exact GP whose inputs X are
parameters.  Every optimiser step needs dL/dX = `kern.gradients_X(dL_dK, X)`; here it comes out of the evaluation's own gradient
phase (`mi355gp_latent_inference_sum`, csrc/latent.hip): one pass over the resident Ky^-1 and alpha gives dL/dX and the kernel's
parameter sums, X alone travels to the device between steps (`mi355gp_latent_set_X`) and no N x N array leaves it."""
import numpy as np

from .inference import ExactGaussianInference
from .kern import RBF, Bias
from .likelihoods import Gaussian
from .models import GP
from .param import Param


class GPLVM(GP):
    """`GPLVM(Y, input_dim, init='PCA', X=None, kernel=None, name="gplvm", Y_metadata=None, normalizer=False)` as the reference's;
    the flat parameter order is [X, kernel, noise].  Kernels: sums of RBF, Matern52, Matern32, Exponential / OU, RatQuad, White and
    Bias parts over at most 32 latent dimensions; anything else is refused by name (`ExactGaussianInference(latent=True)`)."""

    def __init__(self, Y, input_dim, init='PCA', X=None, kernel=None, name="gplvm", Y_metadata=None, normalizer=False, device=0,
                 mean_function=None):
        if mean_function is not None:
            raise NotImplementedError("GPLVM with a mean function: R = Y - m(X) would depend on the latent inputs")
        Y = np.asarray(Y, dtype=np.float64)
        if X is None:
            from .util.initialization import initialize_latent
            X, fracs = initialize_latent(init, input_dim, Y)
        else:
            X, fracs = np.asarray(X, dtype=np.float64), np.ones(input_dim)
        if X.shape != (Y.shape[0], input_dim):
            raise ValueError("GPLVM: X must be %d x %d (one latent point per row of Y), got %r" % (Y.shape[0], input_dim, X.shape))
        if kernel is None:
            kernel = RBF(input_dim, lengthscale=fracs, ARD=input_dim > 1, device=device) + Bias(input_dim, np.exp(-2), device=device)
        self._latent = None                        # until X is a parameter, GP's constructor evaluates at the initial X
        super(GPLVM, self).__init__(X, Y, kernel, Gaussian(), inference_method=ExactGaussianInference(device=device, latent=True),
                                    name=name, Y_metadata=Y_metadata, device=device, normalizer=normalizer)
        self.X = self._latent = Param("latent_mean", X, positive=False)
        self.link_parameter(self.X, index=0)
        self.parameters_changed()

    def parameters_changed(self):
        """(reference `gplvm.py:47-49`; dL/dX is a result of the same device call as the kernel's gradients)"""
        super(GPLVM, self).parameters_changed()
        if self._latent is not None:
            self.X.gradient = self.grad_dict["dL_dX"]
