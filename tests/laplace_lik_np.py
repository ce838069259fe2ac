"""NumPy restatement (dense, `mdot` form) of the Laplace approximation with a likelihood that has parameters, on top of
tests/laplace_np.py: the mode search with W clipped for a likelihood that is not log-concave (reference `laplace.py:319-321`)
and the likelihood-parameter gradient of the approximate log marginal (`laplace.py:276-299`),

    dL_dthetaL_i = sum dlogpdf_dtheta_i + 0.5 diag(Ki_W_i) . d2logpdf_df2_dtheta_i + dL_dfhat^T (I - K K_Wi_i) K dlogpdf_df_dtheta_i

formed with the dense N x N matrices as the reference forms it.  `implicit_vector` is the dense form of what
`mi355gp_laplace_implicit` returns.  Fixtures: tests/golden/laplace_lik (tools/make_golden_laplace_lik.py).  Shared by the
CPU and the GPU tests."""
import os

import numpy as np

import laplace_np as LP
import mlp_np as P
import gpy_amd

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "laplace_lik")
# standing tolerances of tests/test_gpu_laplace.py for the same quantities (tests/laplace_np.py STANDING); the likelihood's
# predictive mean and variance stand with the other predictions.  dL_dthetaL has no standing value: 10 x its stored floor,
# and where that floor is 0 (the reference's two runs stopped at the same iterate) 10 x the stored forward rounding-error bound
# of the reference's own evaluation (tools/make_golden_laplace_lik.py explains both)
STANDING = {"lml": 1e-10, "f_hat": 1e-9, "Ki_fhat": 1e-9, "dtheta": 1e-8, "pred_mu": 1e-9, "pred_var": 1e-9,
            "pred_ymean": 1e-9, "pred_yvar": 1e-9, "dL_dthetaL": 0.0}
NOT_CASES = ("likelihood_values.npz", "robust_toy_optimize.npz")
CASES = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz") and f not in NOT_CASES) if os.path.isdir(GOLDEN) else []


def make_likelihood(g):
    """the gpy_amd likelihood of a fixture (its `lik` string: 'studentt' with `lik_theta` = [t_scale2, deg_free], or 'poisson')"""
    if str(g["lik"]) == "studentt":
        return gpy_amd.StudentT(deg_free=float(g["lik_theta"][1]), sigma2=float(g["lik_theta"][0]))
    return gpy_amd.Poisson()


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    g = {k: z[k] for k in z.files}
    g["specs"] = P.load_specs(g["specs"])
    g["tol"] = {q: max(STANDING[q], 10.0 * float(g["ref_floor_" + q])) for q in STANDING}
    g["tol"]["dL_dthetaL"] = 10.0 * max(float(g["ref_floor_dL_dthetaL"]), float(g["ref_rounding_dL_dthetaL"]))
    if str(g["lik"]) == "poisson":
        # the reference integrates the predictive moments numerically and the package uses the closed form: 10 x the
        # difference the generator measured between the two on the CPU, never less than 1e-12 (relative)
        for q in ("pred_ymean", "pred_yvar"):
            g["tol"][q] = max(1e-12, 10.0 * float(g["closed_form_diff_" + q]))
    g["check_y_prediction"] = "predictive check dropped" not in str(g["note"])
    return g


def clipped_W(lik, f, y):
    W = -lik.d2logpdf_df2(f, y)
    return W if lik.log_concave else np.clip(W, 1e-6, 1e+30)


def find_mode(K, Y, lik, tol=1e-10, max_iter=100, polish=0):
    """laplace_np.find_mode with W clipped where the likelihood is not log-concave; `polish` further full Newton steps"""
    y = Y[:, 0]
    Ki_f, f = np.zeros_like(y), np.zeros_like(y)

    def obj(Ki_f, f):
        return -0.5 * np.dot(Ki_f, f) + np.sum(lik.logpdf(f, y))
    diff, it = np.inf, 0
    while diff > tol and it < max_iter:
        W = clipped_W(lik, f, y)
        a, Ka, _ = LP.newton(K, W, W * f + lik.dlogpdf_df(f, y))
        dKi_f, Kd = a - Ki_f, Ka - f
        s = LP.line_step(obj, Ki_f, f, dKi_f, Kd)
        new = (Ki_f + s * dKi_f, f + s * Kd)
        diff = abs(obj(*new) - obj(Ki_f, f))
        Ki_f, f = new
        it += 1
    for _ in range(polish):
        W = clipped_W(lik, f, y)
        Ki_f, f, _ = LP.newton(K, W, W * f + lik.dlogpdf_df(f, y))
    return f, Ki_f, it


def implicit_vector(K, K_Wi_i, dL_dfhat):
    """s = K (u - K_Wi_i K u) with u = dL_dfhat: s . g = dL_dfhat^T (I - K K_Wi_i) K g for every g (K, K_Wi_i symmetric)"""
    Ku = K @ dL_dfhat
    return K @ (dL_dfhat - K_Wi_i @ Ku)


def dL_dthetaL(lik, K, f, y, diag_Ki_W_i, K_Wi_i, dL_dfhat):
    """the reference's loop over the likelihood's parameters (`laplace.py:279-296`), dense"""
    dlik, dlik_grad, dlik_hess = lik._laplace_gradients(f[:, None], y[:, None])
    I_KW_i = np.eye(K.shape[0]) - K @ K_Wi_i
    out = np.zeros(lik.size)
    for i in range(lik.size):
        explicit = np.sum(dlik[i]) + 0.5 * np.sum(diag_Ki_W_i * dlik_hess[i][:, 0])
        dfhat_dthetaL = I_KW_i @ (K @ dlik_grad[i])
        out[i] = explicit + float(dL_dfhat @ dfhat_dthetaL[:, 0])
    return out


def inference(specs, X, Y, lik, tol=1e-10, max_iter=100, polish=0):
    """dict(lml, f_hat, Ki_fhat, dtheta, dL_dthetaL, woodbury_inv, ...) for the kernel of `specs` and the likelihood `lik`"""
    K, dKs = LP.expr(specs, X)
    y = Y[:, 0]
    f, Ki_f, it = find_mode(K, Y, lik, tol, max_iter, polish)
    W = clipped_W(lik, f, y)
    dKiWi, logdet, K_Wi_i = LP.finish(K, W)
    lml = -0.5 * np.dot(Ki_f, f) + np.sum(lik.logpdf(f, y)) - 0.5 * logdet
    dL_dfhat = -0.5 * dKiWi * (-lik.d3logpdf_df3(f, y))
    G = LP.dL_dK_sym(K, Ki_f, dL_dfhat, K_Wi_i)
    return dict(lml=lml, f_hat=f[:, None], Ki_fhat=Ki_f[:, None], woodbury_inv=K_Wi_i, W=W, iterations=it, K=K,
                dtheta=np.array([np.sum(G * dK) for dK in dKs]), diag_Ki_W_i=dKiWi, dL_dfhat=dL_dfhat,
                dL_dthetaL=dL_dthetaL(lik, K, f, y, dKiWi, K_Wi_i, dL_dfhat))


def figures(g, got):
    fig = {q: (abs(got[q] - g[q]) / abs(g[q]) if q == "lml" else LP.rel(got[q], g[q])) for q in got}
    print({q: "%.1e (tol %.1e)" % (fig[q], g["tol"][q]) for q in fig})
    return fig
