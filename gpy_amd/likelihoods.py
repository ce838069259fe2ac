"""Gaussian likelihood: the caller-side contract of the exact-inference hot path
(reference `GPy/likelihoods/gaussian.py:43,69-79,102-110`).  O(1)/O(N) host bookkeeping only."""
import numpy as np

from .param import Param, Parameterized


class Gaussian(Parameterized):
    def __init__(self, variance=1., name="Gaussian_noise"):
        super(Gaussian, self).__init__(name)
        self.variance = Param("variance", variance)
        self.link_parameter(self.variance)

    def gaussian_variance(self, Y_metadata=None):
        return self.variance

    def exact_inference_gradients(self, dL_dKdiag, Y_metadata=None):
        return np.sum(dL_dKdiag)

    def update_gradients(self, grad):
        self.variance.gradient = grad

    def variational_expectations(self, Y, m, v, gh_points=None, Y_metadata=None):
        """E_q[log p(y | f)] for q(f) = N(m, v), its derivatives in m and v and in the noise variance, in closed form
        (reference `gaussian.py:336-345`): (F, dF_dmu, dF_dv, dF_dtheta), the last of shape (1, N, L)."""
        if self.variance.size != 1:
            raise NotImplementedError("variational_expectations takes one noise variance, not %d" % self.variance.size)
        Y, m, v = np.asarray(Y), np.asarray(m), np.asarray(v)
        lik_var = self.variance.values.ravel()[0].astype(np.result_type(m.dtype, np.float64))
        q = np.square(Y) + np.square(m) + v - 2 * m * Y
        F = -0.5 * np.log(2 * np.pi) - 0.5 * np.log(lik_var) - 0.5 * q / lik_var
        dF_dmu = (Y - m) / lik_var
        dF_dv = np.ones_like(v) * (-0.5 / lik_var)
        dF_dtheta = -0.5 / lik_var + 0.5 * q / (lik_var ** 2)
        return F, dF_dmu, dF_dv, dF_dtheta.reshape(1, Y.shape[0], Y.shape[1])

    def predictive_values(self, mu, var, full_cov=False, Y_metadata=None):
        if full_cov:
            var = var + np.eye(var.shape[0]) * float(self.variance.values[0])
        else:
            var = var + float(self.variance.values[0])
        return mu, var

    def predictive_quantiles(self, mu, var, quantiles, Y_metadata=None):
        """(reference `gaussian.py:118-119`)"""
        from scipy import stats
        return [stats.norm.ppf(q / 100.) * np.sqrt(var + float(self.variance.values[0])) + mu for q in quantiles]

    def log_predictive_density(self, y_test, mu_star, var_star, Y_metadata=None):
        """independent Gaussian predictive densities (reference `gaussian.py:329-334`)"""
        v = var_star + float(self.variance.values[0])
        return -0.5 * np.log(2 * np.pi) - 0.5 * np.log(v) - 0.5 * np.square(y_test - mu_star) / v

    def samples(self, gp, Y_metadata=None):
        """observations drawn around latent values (reference `gaussian.py:316-327`)"""
        gp = np.asarray(gp)
        return gp + np.sqrt(float(self.variance.values[0])) * np.random.normal(size=gp.shape)

    def to_dict(self):
        return {"class": "GPy.likelihoods.Gaussian", "name": self.name, "variance": self.variance.values.tolist()}


class HeteroscedasticGaussian(Gaussian):
    """One noise variance per data point (reference `GPy/likelihoods/gaussian.py:347-371`): `variance` has as many entries
    as `Y_metadata['output_index']`, `gaussian_variance` hands the length-N vector to the inference call (the device adds it
    to the diagonal of K) and the noise gradients are the matching entries of diag(dL_dK), which the device returns as an
    N-vector (`mi355gp_exact_inference(..., diag_dLdK_out)`)."""

    def __init__(self, Y_metadata, variance=1., name="het_Gauss"):
        n = np.asarray(Y_metadata["output_index"]).shape
        Parameterized.__init__(self, name)
        self.variance = Param("variance", np.ones(n).ravel() * variance)
        self.link_parameter(self.variance)

    def gaussian_variance(self, Y_metadata=None):
        return self.variance.values[np.asarray(Y_metadata["output_index"]).flatten()]

    def exact_inference_gradients(self, dL_dKdiag, Y_metadata=None):
        return np.asarray(dL_dKdiag).reshape(-1)[np.asarray(Y_metadata["output_index"]).flatten()]

    def predictive_values(self, mu, var, full_cov=False, Y_metadata=None):
        s = self.variance.values[np.asarray(Y_metadata["output_index"]).flatten()]
        if full_cov:
            return mu, var + np.eye(var.shape[0]) * s
        return mu, var + s[:, None]

    def predictive_quantiles(self, mu, var, quantiles, Y_metadata=None):
        """(reference `gaussian.py:375-377`)"""
        from scipy import stats
        s = self.variance.values[np.asarray(Y_metadata["output_index"]).flatten()]
        return [stats.norm.ppf(q / 100.) * np.sqrt(var + s[:, None]) + mu for q in quantiles]

    def to_dict(self):
        return {"class": "GPy.likelihoods.HeteroscedasticGaussian", "name": self.name,
                "variance": self.variance.values.tolist()}


class MixedNoise(Parameterized):
    """One Gaussian likelihood per output (reference `GPy/likelihoods/mixed_noise.py:15-100`): the sub-likelihoods are linked,
    so their variances are this likelihood's parameters in list order.  `gaussian_variance` hands the length-N noise vector
    (the variance of each row's output, `Y_metadata['output_index']`) to the inference call and the noise gradients are the
    per-output sums of diag(dL_dK), which the device returns as an N-vector.  Only Gaussian sub-likelihoods."""

    def __init__(self, likelihoods_list, name="mixed_noise"):
        super(MixedNoise, self).__init__(name)
        if not all(isinstance(l, Gaussian) and not isinstance(l, HeteroscedasticGaussian) for l in likelihoods_list):
            raise NotImplementedError("MixedNoise on the MI355X path takes Gaussian likelihoods only")
        self.link_parameters(*likelihoods_list)
        self.likelihoods_list = likelihoods_list
        self.log_concave = False

    def _index(self, Y_metadata):
        return np.asarray(Y_metadata["output_index"]).flatten().astype(np.int_)

    def _variances(self):
        return np.array([float(l.variance.values[0]) for l in self.likelihoods_list])

    def gaussian_variance(self, Y_metadata):
        """(reference `mixed_noise.py:24-30`)"""
        return self._variances()[self._index(Y_metadata)]

    def betaY(self, Y, Y_metadata):
        return Y / self.gaussian_variance(Y_metadata=Y_metadata)[:, None]

    def update_gradients(self, gradients):
        g = np.asarray(gradients, dtype=float).ravel()
        for lik, gj in zip(self.likelihoods_list, g):
            lik.update_gradients(gj)

    def exact_inference_gradients(self, dL_dKdiag, Y_metadata):
        """(reference `mixed_noise.py:39-42`): per-output sums of diag(dL_dK)"""
        return np.bincount(self._index(Y_metadata), weights=np.asarray(dL_dKdiag, dtype=float).reshape(-1),
                           minlength=len(self.likelihoods_list)).astype(float)

    def predictive_values(self, mu, var, full_cov=False, Y_metadata=None):
        """(reference `mixed_noise.py:44-51`; the caller's var is not modified)"""
        s = self.gaussian_variance(Y_metadata)
        if full_cov:
            return mu, var + np.diag(s)
        return mu, var + s.reshape(np.shape(var)[0], -1)

    def predictive_variance(self, mu, sigma, Y_metadata):
        """(reference `mixed_noise.py:53-55`)"""
        return self.gaussian_variance(Y_metadata) + sigma ** 2

    def predictive_quantiles(self, mu, var, quantiles, Y_metadata):
        """(reference `mixed_noise.py:57-65`): each output's quantiles from its own likelihood"""
        ind = self._index(Y_metadata)
        mu, var = np.asarray(mu), np.asarray(var)
        Q = np.zeros((mu.size, len(quantiles)))
        for j in np.unique(ind):
            q = self.likelihoods_list[j].predictive_quantiles(mu[ind == j, :], var[ind == j, :], quantiles)
            Q[ind == j, :] = np.hstack(q)
        return [q[:, None] for q in Q.T]

    def log_predictive_density(self, y_test, mu_star, var_star, Y_metadata=None):
        """independent Gaussian predictive densities with each row's own noise variance"""
        v = np.asarray(var_star) + self.gaussian_variance(Y_metadata)[:, None]
        return -0.5 * np.log(2 * np.pi) - 0.5 * np.log(v) - 0.5 * np.square(y_test - mu_star) / v

    def samples(self, gp, Y_metadata):
        """(reference `mixed_noise.py:67-84`)"""
        gp = np.asarray(gp)
        Ysim = np.zeros(gp.shape)
        ind = self._index(Y_metadata)
        for j in np.unique(ind):
            flt = ind == j
            Ysim[flt, :] = gp[flt, :] + np.sqrt(float(self.likelihoods_list[j].variance.values[0])) * np.random.normal(
                size=gp[flt, :].shape)
        return Ysim

    def to_dict(self):
        """(reference `mixed_noise.py:86-100`)"""
        return {"name": self.name, "class": "GPy.likelihoods.MixedNoise",
                "likelihoods_list": [l.to_dict() for l in self.likelihoods_list]}


from . import link_functions  # noqa: E402  (GPy.likelihoods.link_functions)


_SQUARE_LIMIT = np.sqrt(np.finfo(np.float64).max)
_CUBE_LIMIT = np.nextafter(np.finfo(np.float64).max ** (1 / 3.0), -np.inf)


class Likelihood(Parameterized):
    """What the non-Gaussian likelihoods share (reference `GPy/likelihoods/likelihood.py:17-47,551-732`): a link function, the
    derivatives in f composed from the subclass's derivatives in lambda = link(f) and the link's by the chain rule (Faa di Bruno;
    `util/misc.py` chain_1..3, which clip the link's slope before squaring and cubing it), and `_laplace_gradients`, the
    derivatives with respect to the likelihood's own parameters that the Laplace approximation asks for.  A subclass supplies
    `logpdf_link` .. `d3logpdf_dlink3` and, if it has parameters, `dlogpdf_link_dtheta`, `dlogpdf_dlink_dtheta` and
    `d2logpdf_dlink2_dtheta` (each `size` x N x 1, in link order)."""

    def __init__(self, gp_link, name):
        super(Likelihood, self).__init__(name)
        assert isinstance(gp_link, link_functions.GPTransformation), "gp_link is not a valid GPTransformation."
        self.gp_link = gp_link
        self.log_concave = False
        self.is_fixed = False

    def update_gradients(self, grad):
        pass

    def exact_inference_gradients(self, dL_dKdiag, Y_metadata=None):
        return np.zeros(self.size)

    def conditional_mean(self, gp):
        raise NotImplementedError

    def conditional_variance(self, gp):
        raise NotImplementedError

    def _identity(self):
        return isinstance(self.gp_link, link_functions.Identity)

    # ---- in terms of f: Faa di Bruno (reference `likelihood.py:551-652`, `util/misc.py` chain_1..3) ----------------------
    def logpdf(self, f, y, Y_metadata=None):
        return self.logpdf_link(self.gp_link.transf(f), y)

    def dlogpdf_df(self, f, y, Y_metadata=None):
        if self._identity():
            return self.dlogpdf_dlink(f, y)
        return self.dlogpdf_dlink(self.gp_link.transf(f), y) * self.gp_link.dtransf_df(f)

    def d2logpdf_df2(self, f, y, Y_metadata=None):
        if self._identity():
            return self.d2logpdf_dlink2(f, y)
        lam, d1 = self.gp_link.transf(f), self.gp_link.dtransf_df(f)
        return (self.d2logpdf_dlink2(lam, y) * np.clip(d1, -np.inf, _SQUARE_LIMIT) ** 2
                + self.dlogpdf_dlink(lam, y) * self.gp_link.d2transf_df2(f))

    def d3logpdf_df3(self, f, y, Y_metadata=None):
        if self._identity():
            return self.d3logpdf_dlink3(f, y)
        lam, d1, d2 = self.gp_link.transf(f), self.gp_link.dtransf_df(f), self.gp_link.d2transf_df2(f)
        return (self.d3logpdf_dlink3(lam, y) * np.clip(d1, -np.inf, _CUBE_LIMIT) ** 3 + 3.0 * self.d2logpdf_dlink2(lam, y) * d1 * d2
                + self.dlogpdf_dlink(lam, y) * self.gp_link.d3transf_df3(f))

    # ---- in terms of the likelihood's parameters (reference `likelihood.py:655-732`) -------------------------------------
    def _no_parameters(self, f):
        f = np.asarray(f)
        return np.zeros((0,) + f.shape)

    def dlogpdf_dtheta(self, f, y, Y_metadata=None):
        if self.size == 0:
            return self._no_parameters(f)
        return np.asarray(self.dlogpdf_link_dtheta(self.gp_link.transf(f), y))

    def dlogpdf_df_dtheta(self, f, y, Y_metadata=None):
        if self.size == 0:
            return self._no_parameters(f)
        g = np.asarray(self.dlogpdf_dlink_dtheta(self.gp_link.transf(f), y))
        return g if self._identity() else g * self.gp_link.dtransf_df(f)[None]

    def d2logpdf_df2_dtheta(self, f, y, Y_metadata=None):
        if self.size == 0:
            return self._no_parameters(f)
        lam = self.gp_link.transf(f)
        h = np.asarray(self.d2logpdf_dlink2_dtheta(lam, y))
        if self._identity():
            return h
        d1 = np.clip(self.gp_link.dtransf_df(f), -np.inf, _SQUARE_LIMIT)
        return h * (d1 ** 2)[None] + np.asarray(self.dlogpdf_dlink_dtheta(lam, y)) * self.gp_link.d2transf_df2(f)[None]

    def _laplace_gradients(self, f, y, Y_metadata=None):
        """(dlogpdf_dtheta, dlogpdf_df_dtheta, d2logpdf_df2_dtheta), each `size` x N x 1 with the parameters in link order
        (reference `likelihood.py:721-732`)"""
        out = (self.dlogpdf_dtheta(f, y, Y_metadata=Y_metadata), self.dlogpdf_df_dtheta(f, y, Y_metadata=Y_metadata),
               self.d2logpdf_df2_dtheta(f, y, Y_metadata=Y_metadata))
        assert all(a.shape[0] == self.size for a in out)
        return out

    @staticmethod
    def _gh_points(T=20):
        """the Gauss-Hermite rule of the reference (`likelihood.py:229-233`: 20 points)"""
        return np.polynomial.hermite.hermgauss(T)

    def variational_expectations(self, Y, m, v, gh_points=None, Y_metadata=None):
        """E_q[log p(y | f)] for q(f) = N(m, v) and its derivatives in m and v by Gauss-Hermite quadrature (reference
        `likelihood.py:358-411`): (F, dF_dmu, dF_dv, dF_dtheta); dF_dtheta is `size` x N x L, or None without parameters.
        Y, m and v have the same shape."""
        gh_x, gh_w = self._gh_points() if gh_points is None else gh_points
        m, v, Y = np.asarray(m), np.asarray(v), np.asarray(Y)
        shape = m.shape
        m, v, Y = m.ravel(), v.ravel(), Y.ravel()
        X = gh_x[None, :] * np.sqrt(2. * v[:, None]) + m[:, None]          # data along the first axis, nodes along the second
        logp = self.logpdf(X, Y[:, None], Y_metadata=Y_metadata)
        dlogp_dx = self.dlogpdf_df(X, Y[:, None], Y_metadata=Y_metadata)
        d2logp_dx2 = self.d2logpdf_df2(X, Y[:, None], Y_metadata=Y_metadata)
        F = np.dot(logp, gh_w) / np.sqrt(np.pi)
        dF_dm = np.dot(dlogp_dx, gh_w) / np.sqrt(np.pi)
        dF_dv = np.dot(d2logp_dx2, gh_w) / np.sqrt(np.pi) / 2.
        if not (np.all(np.isfinite(dF_dv)) and np.all(np.isfinite(dF_dm))):
            raise FloatingPointError("variational_expectations: the quadrature gave a non-finite derivative")
        dF_dtheta = None
        if self.size:
            dF_dtheta = np.dot(self.dlogpdf_dtheta(X, Y[:, None], Y_metadata=Y_metadata), gh_w) / np.sqrt(np.pi)
            dF_dtheta = dF_dtheta.reshape(self.size, shape[0], shape[1])
        return F.reshape(*shape), dF_dm.reshape(*shape), dF_dv.reshape(*shape), dF_dtheta

    def predictive_values(self, mu, var, full_cov=False, Y_metadata=None):
        """(reference `likelihood.py:734-755`)"""
        pred_mean = self.predictive_mean(mu, var, Y_metadata=Y_metadata)
        return pred_mean, self.predictive_variance(mu, var, pred_mean, Y_metadata=Y_metadata)

    def to_dict(self):
        return {"class": "GPy.likelihoods." + type(self).__name__, "name": self.name, "gp_link_dict": self.gp_link.to_dict()}


class Bernoulli(Likelihood):
    """Bernoulli likelihood p(y | f) = lambda(f)^y (1 - lambda(f))^(1 - y), y in {0, 1} (reference
    `GPy/likelihoods/bernoulli.py:9-273`), with the derivatives in f that the Laplace approximation needs, composed from
    the derivatives in lambda and the link's by the chain rule in `Likelihood` (reference `likelihood.py:551-652`).  No parameters (`size == 0`);
    with the probit link it is log-concave.  The probabilities are clipped where the reference clips them (1e-9), so values far
    in the tails agree with it."""

    def __init__(self, gp_link=None, name="Bernoulli"):
        super(Bernoulli, self).__init__(link_functions.Probit() if gp_link is None else gp_link, name)
        self.log_concave = isinstance(self.gp_link, link_functions.Probit)

    @staticmethod
    def check_targets(Y):
        """Y must hold zeros and ones only (the assertion of reference `bernoulli.py:53-55`)."""
        Y = np.asarray(Y)
        assert np.count_nonzero(Y == 1) + np.count_nonzero(Y == 0) == Y.size, \
            "Bernoulli likelihood is meant to be used only with outputs in {0, 1}."
        return Y

    # ---- EP (reference `bernoulli.py:59-92`) -----------------------------------------------------------------------------
    def _ep_sign(self, Y_i):
        Y_i = np.asarray(Y_i, dtype=np.float64)
        if not np.all((Y_i == 1) | (Y_i == 0) | (Y_i == -1)):
            raise ValueError("bad value for Bernoulli observation (0, 1)")
        return np.where(Y_i == 1, 1.0, -1.0)

    def log_moments_match_ep(self, Y_i, tau_i, v_i):
        """(log Z_hat, mu_hat, sigma2_hat) of the tilted distribution of a cavity N(v / tau, 1 / tau), scalars or arrays.  With
        z = sign v / sqrt(tau^2 + tau): log Z_hat = log Phi(z) and phi(z) / Phi(z) from their definitions, through the scaled
        complementary error function where Phi underflows (z < 0), so both hold over the whole real line."""
        from scipy import special
        if not isinstance(self.gp_link, link_functions.Probit):
            raise NotImplementedError("exact EP moment matching on this backend needs the probit link, not %s"
                                      % type(self.gp_link).__name__)
        sign = self._ep_sign(Y_i)
        tau_i, v_i = np.asarray(tau_i, dtype=np.float64), np.asarray(v_i, dtype=np.float64)
        q = tau_i ** 2 + tau_i
        z = sign * v_i / np.sqrt(q)
        zn = np.minimum(z, 0.0)
        with np.errstate(over="ignore", under="ignore"):
            ratio = np.where(z < 0.0, np.sqrt(2.0 / np.pi) / special.erfcx(-zn / np.sqrt(2.0)),
                             np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi) / special.ndtr(np.maximum(z, 0.0)))
        log_Z_hat = special.log_ndtr(z)
        mu_hat = v_i / tau_i + sign * ratio / np.sqrt(q)
        sigma2_hat = 1.0 / tau_i - (ratio / q) * (z + ratio)
        return log_Z_hat, mu_hat, sigma2_hat

    def moments_match_ep(self, Y_i, tau_i, v_i, Y_metadata_i=None):
        """(Z_hat, mu_hat, sigma2_hat) as the reference returns them (`bernoulli.py:92`)"""
        log_Z_hat, mu_hat, sigma2_hat = self.log_moments_match_ep(Y_i, tau_i, v_i)
        return np.exp(log_Z_hat), mu_hat, sigma2_hat

    def ep_gradients(self, Y, cav_tau, cav_v, dL_dKdiag, Y_metadata=None, quad_mode="gh", boost_grad=1.):
        """no parameters, no gradients (reference `likelihood.py:227-228` for `size == 0`)"""
        return np.zeros(0)

    def variational_expectations(self, Y, m, v, gh_points=None, Y_metadata=None):
        """(reference `bernoulli.py:94-115`): the probit link's quadrature on y f, with Phi clipped to [1e-9, 1 - 1e-9]"""
        if not isinstance(self.gp_link, link_functions.Probit):
            raise NotImplementedError("variational_expectations of a Bernoulli likelihood needs the probit link, not %s"
                                      % type(self.gp_link).__name__)
        gh_x, gh_w = self._gh_points() if gh_points is None else gh_points
        gh_w = gh_w / np.sqrt(np.pi)
        m, v, Y = np.asarray(m), np.asarray(v), np.asarray(Y)
        shape = m.shape
        m, v, Y = m.ravel(), v.ravel(), Y.ravel()
        Ysign = np.where(Y == 1, 1, -1)
        X = gh_x[None, :] * np.sqrt(2. * v[:, None]) + (m * Ysign)[:, None]
        p = np.clip(link_functions.std_norm_cdf(X), 1e-9, 1. - 1e-9)
        NoverP = link_functions.std_norm_pdf(X) / p
        F = np.log(p).dot(gh_w)
        dF_dm = (NoverP * Ysign[:, None]).dot(gh_w)
        dF_dv = -0.5 * (NoverP ** 2 + NoverP * X).dot(gh_w)
        return F.reshape(*shape), dF_dm.reshape(*shape), dF_dv.reshape(*shape), None

    # ---- in terms of lambda = link(f) (reference `bernoulli.py:138-249`) -------------------------------------------------
    def pdf_link(self, inv_link_f, y, Y_metadata=None):
        return np.where(y == 1, inv_link_f, 1.0 - inv_link_f)

    def logpdf_link(self, inv_link_f, y, Y_metadata=None):
        return np.log(np.clip(self.pdf_link(inv_link_f, y), 1e-9, np.inf))

    def dlogpdf_dlink(self, inv_link_f, y, Y_metadata=None):
        lam = np.clip(inv_link_f, 1e-9, 1.0 - 1e-9)
        return 1.0 / np.where(y == 1, lam, -(1.0 - lam))

    def d2logpdf_dlink2(self, inv_link_f, y, Y_metadata=None):
        return -1.0 / np.square(np.clip(self.pdf_link(inv_link_f, y), 1e-9, 1e9))

    def d3logpdf_dlink3(self, inv_link_f, y, Y_metadata=None):
        with np.errstate(divide="ignore"):
            return np.where(y == 1, 2.0 / inv_link_f ** 3, -2.0 / (1.0 - inv_link_f) ** 3)

    # ---- prediction (reference `bernoulli.py:120-136,251-270`, `likelihood.py:734-755`) ---------------------------------
    def predictive_mean(self, mu, variance, Y_metadata=None):
        if not isinstance(self.gp_link, link_functions.Probit):
            raise NotImplementedError("predictive_mean in closed form needs the probit link")
        return link_functions.std_norm_cdf(mu / np.sqrt(1.0 + variance))

    def predictive_variance(self, mu, variance, pred_mean=None, Y_metadata=None):
        return np.nan                                      # as the reference returns it for the probit link

    def predictive_quantiles(self, mu, var, quantiles, Y_metadata=None):
        p = self.predictive_mean(mu, var)
        return [np.asarray(p > (q / 100.0), dtype=np.int32) for q in quantiles]

    def samples(self, gp, Y_metadata=None):
        gp = np.asarray(gp)
        return np.random.binomial(np.ones(gp.size, dtype=int), self.gp_link.transf(gp.ravel())).reshape(gp.shape)


class StudentT(Likelihood):
    """Student-t likelihood with `deg_free` degrees of freedom and squared scale `t_scale2` around lambda(f) (reference
    `GPy/likelihoods/student_t.py:16-319`; Bayesian Data Analysis' nomenclature):

        log p(y | lambda) = lgamma((v + 1) / 2) - lgamma(v / 2) - log(sigma2 v pi) / 2 - (v + 1) / 2 log(1 + e^2 / (v sigma2)),  e = y - lambda

    The parameters are `t_scale2` then `deg_free` in link order, both positive.  It is not log-concave: the Laplace
    approximation clips W from below (reference `laplace.py:319-321`)."""

    def __init__(self, gp_link=None, deg_free=5, sigma2=2, name="Student_T"):
        super(StudentT, self).__init__(link_functions.Identity() if gp_link is None else gp_link, name)
        self.sigma2 = Param("t_scale2", float(sigma2))          # a squared scale, not a noise variance
        self.v = Param("deg_free", float(deg_free))
        self.link_parameter(self.sigma2)
        self.link_parameter(self.v)
        self.log_concave = False

    @property
    def deg_free(self):
        return self.v

    def _sv(self):
        return float(self.sigma2.values[0]), float(self.v.values[0])

    def update_gradients(self, grads):
        """in link order (reference `student_t.py:41-47`)"""
        self.sigma2.gradient = grads[0]
        self.v.gradient = grads[1]

    # ---- in terms of lambda = link(f) (reference `student_t.py:76-171`) --------------------------------------------------
    def logpdf_link(self, inv_link_f, y, Y_metadata=None):
        from scipy.special import gammaln
        s2, v = self._sv()
        e = y - inv_link_f
        return (gammaln((v + 1) * 0.5) - gammaln(v * 0.5) - 0.5 * np.log(s2 * v * np.pi)
                - 0.5 * (v + 1) * np.log(1 + (1 / v) * ((e ** 2) / s2)))

    def dlogpdf_dlink(self, inv_link_f, y, Y_metadata=None):
        s2, v = self._sv()
        e = y - inv_link_f
        return ((v + 1) * e) / (v * s2 + e ** 2)

    def d2logpdf_dlink2(self, inv_link_f, y, Y_metadata=None):
        s2, v = self._sv()
        e = y - inv_link_f
        return ((v + 1) * (e ** 2 - v * s2)) / ((s2 * v + e ** 2) ** 2)

    def d3logpdf_dlink3(self, inv_link_f, y, Y_metadata=None):
        s2, v = self._sv()
        e = y - inv_link_f
        return -(2 * (v + 1) * (-e) * (e ** 2 - 3 * v * s2)) / ((e ** 2 + s2 * v) ** 3)

    # ---- in terms of t_scale2 (reference `student_t.py:173-237`) and deg_free (`:239-268`) --------------------------------
    def dlogpdf_link_dvar(self, inv_link_f, y, Y_metadata=None):
        s2, v = self._sv()
        e2 = np.square(y - inv_link_f)
        return v * (e2 - s2) / (2 * s2 * (s2 * v + e2))

    def dlogpdf_dlink_dvar(self, inv_link_f, y, Y_metadata=None):
        s2, v = self._sv()
        e = y - inv_link_f
        return (v * (v + 1) * (-e)) / ((s2 * v + e ** 2) ** 2)

    def d2logpdf_dlink2_dvar(self, inv_link_f, y, Y_metadata=None):
        s2, v = self._sv()
        e = y - inv_link_f
        return (v * (v + 1) * (s2 * v - 3 * (e ** 2))) / ((s2 * v + (e ** 2)) ** 3)

    def dlogpdf_link_dv(self, inv_link_f, y, Y_metadata=None):
        from scipy.special import psi
        s2, v = self._sv()
        e2 = np.square(y - inv_link_f)
        d = 0.5 * psi(0.5 * (v + 1)) - 0.5 * psi(0.5 * v) - 1.0 / (2 * v)
        d = d + 0.5 * (v + 1) * e2 / (v * (e2 + s2 * v))
        return d - 0.5 * np.log1p(e2 / (s2 * v))

    def dlogpdf_dlink_dv(self, inv_link_f, y, Y_metadata=None):
        s2, v = self._sv()
        e = y - inv_link_f
        e2 = np.square(e)
        return e * (e2 - s2) / (e2 + s2 * v) ** 2

    def d2logpdf_dlink2_dv(self, inv_link_f, y, Y_metadata=None):
        s2, v = self._sv()
        e2 = np.square(y - inv_link_f)
        q = e2 + s2 * v
        return (-s2 * (v + 1) + e2 - s2 * v) / q ** 2 - 2 * s2 * (v + 1) * (e2 - s2 * v) / q ** 3

    def dlogpdf_link_dtheta(self, f, y, Y_metadata=None):
        return np.array((self.dlogpdf_link_dvar(f, y), self.dlogpdf_link_dv(f, y)))

    def dlogpdf_dlink_dtheta(self, f, y, Y_metadata=None):
        return np.array((self.dlogpdf_dlink_dvar(f, y), self.dlogpdf_dlink_dv(f, y)))

    def d2logpdf_dlink2_dtheta(self, f, y, Y_metadata=None):
        return np.array((self.d2logpdf_dlink2_dvar(f, y), self.d2logpdf_dlink2_dv(f, y)))

    # ---- prediction (reference `student_t.py:285-319`, `likelihood.py:440-497`) ------------------------------------------
    def conditional_mean(self, gp):
        return self.gp_link.transf(gp)

    def conditional_variance(self, gp):
        """v / (v - 2), as the reference states it (`student_t.py:302-303`: without the squared scale)"""
        v = self._sv()[1]
        return v / (v - 2.0)

    def predictive_mean(self, mu, sigma, Y_metadata=None):
        return self.gp_link.transf(mu)

    def predictive_variance(self, mu, variance, predictive_mean=None, Y_metadata=None):
        """E[V(y* | f*)] + V[E(y* | f*)] over f* ~ N(mu, variance) (reference `likelihood.py:440-497`, which integrates
        numerically): with the identity link the first term is the constant `conditional_variance` and the second is
        `variance`.  It does not exist for deg_free <= 2 (NaN, `student_t.py:289-293`)."""
        mu = np.asarray(mu, dtype=np.float64)
        if self._sv()[1] <= 2.0:
            return np.full(mu.shape, np.nan)
        if not self._identity():
            raise NotImplementedError("predictive_variance in closed form needs the identity link")
        return self.conditional_variance(mu) + np.asarray(variance, dtype=np.float64)

    def samples(self, gp, Y_metadata=None):
        from scipy import stats
        gp = np.asarray(gp)
        s2, v = self._sv()
        return stats.t.rvs(v, loc=self.gp_link.transf(gp.ravel()), scale=np.sqrt(s2), size=gp.size).reshape(gp.shape)

    def to_dict(self):
        return dict(super(StudentT, self).to_dict(), deg_free=self.v.values.tolist(), t_scale2=self.sigma2.values.tolist())


class Poisson(Likelihood):
    """Poisson likelihood p(y | lambda) = lambda^y exp(-lambda) / y!, y in {0, 1, 2, ...} (reference
    `GPy/likelihoods/poisson.py:11-152`); the default link is `Log`, with which it is log-concave
    (d2 log p / df2 = -exp(f)).  No parameters."""

    def __init__(self, gp_link=None, name="Poisson"):
        super(Poisson, self).__init__(link_functions.Log() if gp_link is None else gp_link, name)
        self.log_concave = isinstance(self.gp_link, link_functions.Log)

    @staticmethod
    def check_targets(Y):
        """Y must hold non-negative whole numbers (the note of reference `poisson.py:18-19`)."""
        Y = np.asarray(Y)
        assert np.count_nonzero((Y >= 0) & (Y == np.floor(Y))) == Y.size, \
            "Poisson likelihood is meant to be used only with outputs in {0, 1, 2, ...}."
        return Y

    # ---- in terms of lambda = link(f) (reference `poisson.py:52-127`) ----------------------------------------------------
    def logpdf_link(self, link_f, y, Y_metadata=None):
        from scipy.special import gammaln
        return -link_f + y * np.log(link_f) - gammaln(y + 1)

    def dlogpdf_dlink(self, link_f, y, Y_metadata=None):
        return y / link_f - 1

    def d2logpdf_dlink2(self, link_f, y, Y_metadata=None):
        return -y / (link_f ** 2)

    def d3logpdf_dlink3(self, link_f, y, Y_metadata=None):
        return 2 * y / (link_f) ** 3

    # ---- prediction (reference `poisson.py:129-152`, `likelihood.py:413-497`) --------------------------------------------
    def conditional_mean(self, gp):
        return self.gp_link.transf(gp)

    def conditional_variance(self, gp):
        return self.gp_link.transf(gp)

    def _log_link_only(self, what):
        if not isinstance(self.gp_link, link_functions.Log):
            raise NotImplementedError("%s in closed form needs the log link" % what)

    def predictive_mean(self, mu, variance, Y_metadata=None):
        """E[exp(f*)] = exp(mu + v / 2) for f* ~ N(mu, v): the log-normal mean (the reference integrates numerically,
        `likelihood.py:413-438`)"""
        self._log_link_only("predictive_mean")
        return np.exp(np.asarray(mu, dtype=np.float64) + 0.5 * np.asarray(variance, dtype=np.float64))

    def predictive_variance(self, mu, variance, predictive_mean=None, Y_metadata=None):
        """E[V(y* | f*)] + V[E(y* | f*)] = E + (exp(v) - 1) exp(2 mu + v) (`likelihood.py:440-497` in closed form)"""
        self._log_link_only("predictive_variance")
        mu, v = np.asarray(mu, dtype=np.float64), np.asarray(variance, dtype=np.float64)
        return np.exp(mu + 0.5 * v) + np.expm1(v) * np.exp(2.0 * mu + v)

    def samples(self, gp, Y_metadata=None):
        gp = np.asarray(gp)
        return np.random.poisson(self.gp_link.transf(gp.ravel())).reshape(gp.shape)
