"""NumPy restatement of what `BayesianGPLVM` adds to the uncertain-input sparse fit of tests/psi_np.py: the KL term of the
standard normal prior and its gradients (reference `variational.py:29-37`), the bound and the gradients of q(X)
(`bayesian_gplvm.py:84-100`), and prediction at uncertain points (`posterior.py:249-269`).  Every function takes a dtype:
float64, or long double for the references the device is judged against."""
import numpy as np

import psi_np as P


def kl(mu, S, dtype=np.float64):
    """KL(q || N(0, I)), dKL/dmu, dKL/dS"""
    mu, S = np.asarray(mu, dtype=dtype), np.asarray(S, dtype=dtype)
    return 0.5 * ((mu * mu).sum() + (S - np.log(S)).sum()) - dtype(0.5) * mu.size, mu, 0.5 * (1 - 1 / S)


def bound(var, ls, ARD, white, Z, mu, S, Y, noise, dtype=np.float64):
    """`P.vardtc_uncertain` plus: bound = lml - KL, Xmean_grad = dmu - mu, Xvar_grad = dS - (1 - 1/S)/2, woodbury_inv"""
    v = P.vardtc_uncertain(var, ls, ARD, white, Z, mu, S, Y, noise, dtype=dtype)
    k, gm, gs = kl(mu, S, dtype)
    v.update(KL=k, bound=v["lml"] - k, Xmean_grad=v["dmu"] - gm, Xvar_grad=v["dS"] - gs,
             woodbury_inv=woodbury_inv(var, ls, white, Z, mu, S, noise, dtype))
    return v


def woodbury_inv(var, ls, white, Z, mu, S, noise, dtype=np.float64):
    """Lm^-T (I - B^-1) Lm^-1 (reference `var_dtc.py:206-210`)"""
    v, l2, Zd, _, _ = P._prep(var, ls, Z, mu, S, dtype)
    M = Zd.shape[0]
    beta = 1 / max(dtype(noise), dtype(1e-8))
    psi2 = P.psi_stats(var, ls, Z, mu, S, None, dtype)[2]
    I = np.eye(M, dtype=dtype)
    Lmi = P._tri_inv(P._chol(P._rbf_K(v, l2, Zd) + (dtype(sum(white)) + dtype(1e-8)) * I))
    LBi = P._tri_inv(P._chol(I + Lmi @ (beta * psi2) @ Lmi.T))
    return Lmi.T @ (I - LBi.T @ LBi) @ Lmi


def predict_uncertain(var, ls, white, Z, wv, Winv, mu_new, S_new, dtype=np.float64, clip=True):
    """(mean (N* x Dy), var (N* x Dy), psi0*) at q(x*) = N(mu_new, diag S_new) for RBF(var, ls) + White parts, given the
    posterior's woodbury_vector and woodbury_inv: row by row, no N* x M x M array"""
    v, l2, Zd, mud, Sd = P._prep(var, ls, Z, mu_new, S_new, dtype)
    la, W = np.asarray(wv, dtype=dtype), np.asarray(Winv, dtype=dtype)
    psi0 = v + dtype(sum(white))
    mean, out = np.empty((mud.shape[0], la.shape[1]), dtype=dtype), np.empty((mud.shape[0], la.shape[1]), dtype=dtype)
    for n in range(mud.shape[0]):
        p1, p2 = P.psi1_row(v, l2, Zd, mud[n], Sd[n]), P.psi2_row(v, l2, Zd, mud[n], Sd[n])
        mean[n] = p1 @ la
        out[n] = psi0 + ((p2 @ la) * la).sum(0) - (p2 * W).sum() - mean[n] ** 2
    if clip:
        out = np.maximum(out, dtype(1e-15))
    return mean, out, psi0


# ---- the shape edges of k_psi2n_contract (tests/test_gpu_bgplvm.py; their float64 distance is measured in
# tests/test_oracle_bgplvm.py): (M, Mn, Q, Dy, White variances) ---------------------------------------------------------------
EDGE_CASES = [(1, 1, 1, 1, ()), (15, 63, 1, 1, (0.3,)), (17, 65, 2, 3, (0.3,)), (65, 65, 3, 3, (0.3,)), (130, 63, 2, 1, (0.3,)),
              (8, 2051, 2, 3, (0.3,)), (17, 65, 33, 1, (0.3,)), (15, 63, 40, 3, (0.3,)), (17, 33, 20, 1, (0.3,)),
              (33, 17, 2, 4, (0.3,)), (17, 33, 3, 5, ())]


def edge_id(c):
    return "M%d_Mn%d_Q%d_Dy%d%s" % (c[0], c[1], c[2], c[3], "_white" if c[4] else "")


def edge_problem(c):
    """a seeded fit (training inputs, Y, Z, kernel, noise) and new uncertain points for one edge case, in the fixtures' range
    (|mu| <= 3, S in [0.05, 1]); beyond three dimensions the lengthscales grow with sqrt(Q) so that psi2 stays away from 0"""
    M, Mn, Q, Dy, white = c
    r = np.random.default_rng(1000 + 7 * M + 3 * Mn + Q + Dy)
    N = max(40, 2 * M)
    mu = r.uniform(-3, 3, (N, Q))
    Y = np.sin(mu.sum(1, keepdims=True) / np.sqrt(Q) + 0.7 * np.arange(Dy)[None, :]) + 0.1 * r.standard_normal((N, Dy))
    ls = r.uniform(0.8, 1.8, Q) * (np.sqrt(Q) if Q > 3 else 1.0)
    return dict(var=1.3, ls=ls, ARD=True, white=list(white), Z=r.uniform(-3, 3, (M, Q)), mu=mu, S=r.uniform(0.05, 1.0, (N, Q)),
                Y=Y, noise=0.05, mu_new=r.uniform(-3, 3, (Mn, Q)), S_new=r.uniform(0.05, 1.0, (Mn, Q)))


def example_data(seed=0, n_per=30, Dy=12):
    """the data of examples/bgplvm.py: three clusters on a 2-D latent manifold, embedded non-linearly in Dy dimensions"""
    r = np.random.default_rng(seed)
    centres = np.array([[-1.5, -1.0], [1.5, -0.5], [0.0, 1.6]])
    labels = np.repeat(np.arange(3), n_per)
    t = centres[labels] + 0.35 * r.standard_normal((3 * n_per, 2))
    A, B = r.standard_normal((2, Dy)), r.standard_normal((2, Dy))
    Y = np.sin(t @ A) + 0.5 * np.tanh(t @ B) * (t[:, :1] * t[:, 1:]) + 0.05 * r.standard_normal((3 * n_per, Dy))
    return Y, labels, t
