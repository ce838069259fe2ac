"""Link functions of the non-Gaussian likelihoods (reference `GPy/likelihoods/link_functions.py`): the map from the latent
function value f to the likelihood's parameter and its first three derivatives.  O(N) host arithmetic."""
import numpy as np
from scipy.special import ndtr

_SQRT_2PI = np.sqrt(2.0 * np.pi)


def std_norm_cdf(x):
    """Phi(x), tail-safe (reference `GPy/util/univariate_Gaussian.py:6`: scipy's ndtr)."""
    return ndtr(x)


def std_norm_pdf(x):
    """phi(x) with the argument clipped to +-1e150 so that its square stays finite (reference `univariate_Gaussian.py:10-12`)."""
    x = np.clip(x, -1e150, 1e150)
    return np.exp(-0.5 * np.square(x)) / _SQRT_2PI


class GPTransformation(object):
    def transf(self, f):
        raise NotImplementedError

    def dtransf_df(self, f):
        raise NotImplementedError

    def d2transf_df2(self, f):
        raise NotImplementedError

    def d3transf_df3(self, f):
        raise NotImplementedError

    def to_dict(self):
        raise NotImplementedError


class Probit(GPTransformation):
    """g(f) = Phi^-1(mu), i.e. mu = Phi(f) (reference `link_functions.py:109-139`)."""

    def transf(self, f):
        return std_norm_cdf(f)

    def dtransf_df(self, f):
        return std_norm_pdf(f)

    def d2transf_df2(self, f):
        return -f * std_norm_pdf(f)

    def d3transf_df3(self, f):
        return (np.square(f) - 1.0) * std_norm_pdf(f)

    def to_dict(self):
        return {"class": "GPy.likelihoods.link_functions.Probit"}


_EXP_LIMIT = np.log(np.finfo(np.float64).max)


def safe_exp(f):
    """exp(f) with the argument clipped from above at log(DBL_MAX), so it never overflows (reference `GPy/util/misc.py:16-18`)."""
    return np.exp(np.clip(f, -np.inf, _EXP_LIMIT))


class Identity(GPTransformation):
    """g(f) = f (reference `link_functions.py:77-107`)."""

    def transf(self, f):
        return f

    def dtransf_df(self, f):
        return np.ones_like(f)

    def d2transf_df2(self, f):
        return np.zeros_like(f)

    def d3transf_df3(self, f):
        return np.zeros_like(f)

    def to_dict(self):
        return {"class": "GPy.likelihoods.link_functions.Identity"}


class Log(GPTransformation):
    """g(f) = log(mu), i.e. mu = exp(f) and so is every derivative (reference `link_functions.py:205-222`)."""

    def transf(self, f):
        return safe_exp(f)

    def dtransf_df(self, f):
        return safe_exp(f)

    def d2transf_df2(self, f):
        return safe_exp(f)

    def d3transf_df3(self, f):
        return safe_exp(f)

    def to_dict(self):
        return {"class": "GPy.likelihoods.link_functions.Log"}
