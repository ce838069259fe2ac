"""gpy_amd -- MI355X-native (gfx950) backend for GPy's exact-GP hot path.

    from gpy_amd import RBF, Matern52, Gaussian, ExactGaussianInference, GPRegression

Host code is Python + ctypes over the C-ABI in include/mi355gp.h; every array operation of the path
(K build, Cholesky, triangular inverse, Ky^-1, alpha, gradient reductions, prediction) is a hand-written
HIP kernel in gpy_amd/csrc.  No PyTorch, no NumPy fallback: without an MI355X the compute calls raise.
"""
from . import _lib
from ._lib import MI355GPError, build, device_count
from .inference import ExactGaussianInference, ExactStudentTInference
from .laplace import Laplace, LaplacePosterior
from .ep import EP
from .vargauss import VarGauss, VarGaussPosterior
from .kron import GaussianGridInference, GpGrid, GPRegressionGrid, GridPosterior
from .kern import (OU, RBF, Add, Prod, Bias, Coregionalize, Cosine, ExpQuad, ExpQuadCosine, Sinc, Exponential, Linear, Matern32, Matern52, MLP, Poly, RatQuad,
                   Stationary, StdPeriodic, White)
from .likelihoods import Bernoulli, Gaussian, HeteroscedasticGaussian, MixedNoise, Poisson, StudentT
from .models import (GP, GPClassification, GPCoregionalizedRegression, GPHeteroscedasticRegression, GPRegression,
                     GPVariationalGaussianApproximation)
from .posterior import PosteriorEP, PosteriorExact, StudentTPosterior
from .sparse import SSGPLVM, BayesianGPLVM, BayesianGPLVMMiniBatch, SparseGP, SparseGPCoregionalizedRegression, SparseGPRegression, VarDTC
from .pep import FITC, PEP
from .epdtc import EPDTC, SparseGPClassification
from .svgp import SVGPModel as SVGP
from .svgp import SVGPPosterior
from .variational import NormalPosterior, NormalPrior, SpikeAndSlabPosterior, SpikeAndSlabPrior

__all__ = ["RBF", "OU", "ExpQuad", "HeteroscedasticGaussian", "StudentTPosterior", "Matern52", "Matern32", "Exponential", "RatQuad", "Cosine", "Sinc", "ExpQuadCosine", "StdPeriodic", "Coregionalize", "Linear", "MLP", "Poly", "MixedNoise", "Stationary", "White", "Bias", "Add", "Prod", "Gaussian", "ExactGaussianInference", "ExactStudentTInference",
           "PosteriorExact", "GP", "GPRegression", "GPHeteroscedasticRegression", "GPCoregionalizedRegression", "Laplace", "LaplacePosterior", "EP", "PosteriorEP", "Bernoulli", "StudentT", "Poisson", "GPClassification", "VarDTC", "SparseGP", "SparseGPRegression", "SparseGPCoregionalizedRegression", "SVGP", "SVGPPosterior", "NormalPosterior", "NormalPrior", "SpikeAndSlabPosterior", "SpikeAndSlabPrior", "BayesianGPLVM", "BayesianGPLVMMiniBatch", "SSGPLVM", "FITC", "PEP", "EPDTC", "SparseGPClassification", "VarGauss", "VarGaussPosterior", "GPVariationalGaussianApproximation", "GaussianGridInference", "GridPosterior", "GpGrid", "GPRegressionGrid", "MI355GPError", "build", "device_count"]

# GPy's import paths, so that `import gpy_amd as GPy` reads like the reference on this path:
#   GPy.kern.RBF, GPy.likelihoods.Gaussian, GPy.models.GPRegression / SparseGPRegression / GPHeteroscedasticRegression,
#   GPy.models.GPClassification, GPy.likelihoods.Bernoulli / StudentT / Poisson, GPy.likelihoods.link_functions.Probit /
#   Identity / Log,
#   GPy.core.GP / SparseGP / SVGP, GPy.inference.latent_function_inference.ExactGaussianInference / VarDTC / Laplace / EP / SVGP,
#   GPy.inference.latent_function_inference.FITC / PEP (and .fitc.FITC, .pep.PEP),
#   GPy.inference.latent_function_inference.EPDTC (and .expectation_propagation.EPDTC), GPy.models.SparseGPClassification,
#   GPy.inference.latent_function_inference.VarGauss (and .var_gauss.VarGauss), GPy.models.GPVariationalGaussianApproximation,
#   GPy.models.GPRegressionGrid, GPy.core.GpGrid, GPy.inference.latent_function_inference.GaussianGridInference (and
#   .gaussian_grid_inference.GaussianGridInference, .grid_posterior.GridPosterior), GPy.kern.GridRBF,
#   GPy.util.choleskies, GPy.models.BayesianGPLVM, GPy.models.BayesianGPLVMMiniBatch (and .bayesian_gplvm_minibatch), GPy.util.initialization.initialize_latent,
#   GPy.models.SparseGPCoregionalizedRegression, GPy.models.ss_gplvm.SSGPLVM,
#   GPy.core.parameterization.variational.SpikeAndSlabPosterior / SpikeAndSlabPrior
from . import ep, epdtc, inference, kern, kron, laplace, likelihoods, link_functions, linalg, models, pep, sparse, svgp, util, vargauss  # noqa: E402
import types as _types  # noqa: E402

models.SparseGPRegression = SparseGPRegression
models.SparseGPCoregionalizedRegression = SparseGPCoregionalizedRegression
models.BayesianGPLVM = BayesianGPLVM
models.BayesianGPLVMMiniBatch = BayesianGPLVMMiniBatch
models.bayesian_gplvm_minibatch = _types.SimpleNamespace(BayesianGPLVMMiniBatch=BayesianGPLVMMiniBatch)
models.ss_gplvm = _types.SimpleNamespace(SSGPLVM=SSGPLVM)         # (GPy.models.SSGPLVM itself keeps refusing: models.__getattr__)
models.SparseGPClassification = SparseGPClassification
models.GPRegressionGrid = GPRegressionGrid
core = _types.SimpleNamespace(GP=GP, GpGrid=GpGrid, gp_grid=_types.SimpleNamespace(GpGrid=GpGrid), SparseGP=SparseGP, SVGP=SVGP, svgp=_types.SimpleNamespace(SVGP=SVGP), parameterization=_types.SimpleNamespace(
    variational=_types.SimpleNamespace(NormalPosterior=NormalPosterior, NormalPrior=NormalPrior,
                                       SpikeAndSlabPosterior=SpikeAndSlabPosterior, SpikeAndSlabPrior=SpikeAndSlabPrior)))
likelihoods.mixed_noise = _types.SimpleNamespace(MixedNoise=MixedNoise)
inference.latent_function_inference = _types.SimpleNamespace(
    ExactGaussianInference=ExactGaussianInference, ExactStudentTInference=ExactStudentTInference, VarDTC=VarDTC,
    PosteriorExact=PosteriorExact, StudentTPosterior=StudentTPosterior, Laplace=Laplace,
    laplace=_types.SimpleNamespace(Laplace=Laplace), EP=EP, PosteriorEP=PosteriorEP,
    expectation_propagation=_types.SimpleNamespace(EP=EP, EPDTC=EPDTC), EPDTC=EPDTC, posterior=_types.SimpleNamespace(PosteriorEP=PosteriorEP, PosteriorExact=PosteriorExact),
    exact_gaussian_inference=_types.SimpleNamespace(ExactGaussianInference=ExactGaussianInference),
    var_dtc=_types.SimpleNamespace(VarDTC=VarDTC), SVGP=svgp.SVGP, svgp=_types.SimpleNamespace(SVGP=svgp.SVGP),
    FITC=FITC, PEP=PEP, fitc=_types.SimpleNamespace(FITC=FITC), pep=_types.SimpleNamespace(PEP=PEP),
    VarGauss=VarGauss, var_gauss=_types.SimpleNamespace(VarGauss=VarGauss),
    GaussianGridInference=GaussianGridInference, GridPosterior=GridPosterior,
    gaussian_grid_inference=_types.SimpleNamespace(GaussianGridInference=GaussianGridInference),
    grid_posterior=_types.SimpleNamespace(GridPosterior=GridPosterior))
