"""Multi-output bookkeeping after `GPy/util/multioutput.py`: stacking per-output data with an output-index column, the
MixedNoise likelihood and the ICM / LCM coregionalized kernels.  Host work only (O(N) arrays, no kernel math); the kernels
they build run on the device like any other product / sum (C-ABI kind `MI355GP_COREGIONALIZE`)."""
import warnings

import numpy as np

from ..kern import Coregionalize, Prod
from ..likelihoods import Gaussian, MixedNoise


def index_to_slices(index):
    """nested list of slices: for every integer of `index`, the runs where it occurs (reference `multioutput.py:6-36`)"""
    if len(index) == 0:
        return []
    ind = np.asarray(index, dtype=int)
    ret = [[] for i in range(ind.max() + 1)]
    ind_ = np.hstack((ind, ind[0] + ind[-1] + 1))
    switchpoints = np.nonzero(ind_ - np.roll(ind_, +1))[0]
    for ind_i, (a, b) in zip(ind[switchpoints[:-1]], zip(switchpoints, switchpoints[1:])):
        ret[ind_i].append(slice(a, b))
    return ret


def get_slices(input_list):
    """(reference `multioutput.py:39-44`)"""
    _s = np.cumsum([0] + [_x.shape[0] for _x in input_list])
    return [slice(a, b) for a, b in zip(_s[:-1], _s[1:])]


def build_XY(input_list, output_list=None, index=None):
    """X = the stacked inputs with the output index appended as the last column, Y = the stacked outputs, I = the index
    column (reference `multioutput.py:47-66`)"""
    num_outputs = len(input_list)
    if output_list is not None:
        assert num_outputs == len(output_list)
        Y = np.vstack(output_list)
    else:
        Y = None
    if index is not None:
        assert len(index) == num_outputs
        I = np.hstack([np.repeat(j, _x.shape[0]) for _x, j in zip(input_list, index)])
    else:
        I = np.hstack([np.repeat(j, _x.shape[0]) for _x, j in zip(input_list, range(num_outputs))])
    X = np.vstack(input_list)
    X = np.hstack([X, I[:, None]])
    return X, Y, I[:, None]


def build_likelihood(Y_list, noise_index, likelihoods_list=None):
    """MixedNoise over one Gaussian per output (reference `multioutput.py:69-80`)"""
    Ny = len(Y_list)
    if likelihoods_list is None:
        likelihoods_list = [Gaussian(name="Gaussian_noise_%s" % j) for y, j in zip(Y_list, range(Ny))]
    else:
        assert len(likelihoods_list) == Ny
    return MixedNoise(likelihoods_list=likelihoods_list)


def ICM(input_dim, num_outputs, kernel, W_rank=1, W=None, kappa=None, name="ICM"):
    """Intrinsic coregionalization model: kernel * Coregionalize on the index column `input_dim` (reference
    `multioutput.py:83-112`)"""
    if kernel.input_dim != input_dim:
        kernel.input_dim = input_dim
        warnings.warn("kernel's input dimension overwritten to fit input_dim parameter.")
    return Prod([kernel, Coregionalize(1, num_outputs, active_dims=[input_dim], rank=W_rank, W=W, kappa=kappa, name="B",
                                       device=getattr(kernel, "device", 0))], name=name)


def LCM(input_dim, num_outputs, kernels_list, W_rank=1, name="ICM"):
    """Linear coregionalization model: a sum of ICMs (reference `multioutput.py:115-133`)"""
    K = ICM(input_dim, num_outputs, kernels_list[0], W_rank, name="%s%s" % (name, 0))
    for j, kernel in enumerate(kernels_list[1:], start=1):
        K += ICM(input_dim, num_outputs, kernel, W_rank, name="%s%s" % (name, j))
    return K
