/* mi355gp.h -- C-ABI of libmi355gp.so: the MI355X-native (gfx950, hand-written HIP) exact-GP backend.
 *
 * GPy has no FFI: its hot path is three Python call signatures.  This header is the
 * boundary a maintainer binds with ctypes; every entry point names the
 * reference function(s) it replaces (paths relative to the GPy checkout).
 *
 * Conventions
 *   - all matrices fp64; host arrays are C-contiguous (row-major) unless a `fortran_order` flag says otherwise
 *   - return value: 0 = OK; >0 = LAPACK-style `info` (1-based index of the first non-positive pivot of the
 *     Cholesky factorisation); <0 = argument / HIP error, text via mi355gp_last_error()
 *   - `kind`: covariance function, `ard`: 0 = one lengthscale, 1 = one per input dimension
 *   - `theta` = [variance, lengthscale (1 or D values)]  (the order GPy links them: kern/src/stationary.py:78-81)
 *   - gradient outputs use the same order; values/gradients are untransformed (paramz applies Logexp outside)
 *   - one context = one device + one data set (X, Y); contexts are independent, not thread-safe individually
 */
#ifndef MI355GP_H
#define MI355GP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi355gp_ctx mi355gp_ctx;

enum { MI355GP_RBF = 0, MI355GP_MATERN52 = 1, MI355GP_MATERN32 = 2, MI355GP_EXPONENTIAL = 3,
       MI355GP_WHITE = 4, MI355GP_BIAS = 5 /* static kernels, only as parts of a sum (kern/src/static.py:63-98,151-173) */,
       MI355GP_RATQUAD = 6, MI355GP_STDPERIODIC = 7, MI355GP_COREGIONALIZE = 8, MI355GP_LINEAR = 9,
       MI355GP_MLP = 10, MI355GP_POLY = 11, MI355GP_COSINE = 12, MI355GP_SINC = 13, MI355GP_EXPQUADCOSINE = 14 };

/* The exact-GP entry points (single kind and part lists; not the sparse or grid paths) also take
 *   MI355GP_RATQUAD      k = var (1 + r^2/2)^-power (kern/src/stationary.py:747-802, GPy.kern.RatQuad);
 *                        theta = [variance, lengthscale (1, or n_active if ard), power]  (link order :757-760)
 *   MI355GP_STDPERIODIC  k = var exp(-1/2 sum_q (sin(pi (x_q - x'_q) / T_q) / l_q)^2) (kern/src/standard_periodic.py:15-133,
 *                        GPy.kern.StdPeriodic); theta = [variance, period (1 or n_active), lengthscale (1 or n_active)]
 *                        (:56-94); `ard` is a bitmask: bit 0 = ARD1 (one period per dimension), bit 1 = ARD2 (one
 *                        lengthscale per dimension)
 * Gradients come back in theta order.  Both have K(x, x) = variance.  Period, lengthscale and power must be positive. */

/* The exact-GP part-list entry points (mi355gp_exact_inference_sum, mi355gp_exact_studentt_sum, mi355gp_predict_sum,
 * mi355gp_covariance_between_points) and the stateless mi355gp_kern_K / mi355gp_update_gradients_full also take
 *   MI355GP_COREGIONALIZE  k(x, x') = B[idx][idx'] (kern/src/coregionalize.py:82-157, GPy.kern.Coregionalize), idx = the value
 *                          of ONE input column holding the output index (n_active must be 1; the stateless entry points take
 *                          that column itself, D = 1).  `ard` carries the number of outputs P, 1 <= P <= 16 (StdPeriodic
 *                          reuses `ard` as well, as a bitmask).  theta = B, P x P row-major, symmetric (the host passes
 *                          0.5 (B + B^T), B = W W^T + diag(kappa), :80-81).  Every index must be an integer in [0, P):
 *                          anything else is an error return naming the value, never a clamp.
 *                          Gradients come back as S, P x P row-major in theta order: S[a][b] = sum over rows i with idx_i = a
 *                          and columns j with idx_j = b of dL_dK_ij (times the term's other factors).  The host turns S into
 *                          dkappa = diag(S), dW = (S + S^T) W (:110-128).  Usually a factor of a product term (ICM / LCM);
 *                          the single-kind entry points, mi355gp_kern_Kdiag, mi355gp_predictive_gradients_sum and the sparse
 *                          and grid paths reject it. */

/* The exact-GP entry points (single kind and part lists), mi355gp_predictive_gradients_sum and the stateless mi355gp_kern_K /
 * mi355gp_update_gradients_full / mi355gp_gradients_X also take
 *   MI355GP_LINEAR         k(x, x') = sum_q var_q x_q x'_q (kern/src/linear.py:13-85, GPy.kern.Linear), alone, as a summand or as
 *                          a factor of a product term.  theta = the variances in GPy's order (:34-51): one value (ard = 0) or
 *                          one per active dimension (ard = 1); every one must be positive.  Gradients come back in theta
 *                          order (:87-98).  Not stationary: K(x, x) = sum_q var_q x_q^2 depends on the point (:84-85), so
 *                          prediction variances take Kdiag per point and mi355gp_kern_Kdiag (no X argument) rejects the kind;
 *                          dK/dx = var_q x'_q (:108-114) and dKdiag/dx = 2 var_q x_q enter mi355gp_predictive_gradients_sum.
 *                          The sparse and grid paths reject it. */

/* The same entry points take the two other dot-product kinds of GPy, functions of x.x', x.x and x'.x' alone:
 *   MI355GP_MLP            the arc-sine / neural-network kernel (kern/src/mlp.py:48-64, GPy.kern.MLP):
 *                            k(x, x') = var (2/pi) asin( s / sqrt((p + 1)(p' + 1)) ),  s = sum_q w_q x_q x'_q + b,
 *                            p = sum_q w_q x_q^2 + b (p' likewise from x').
 *                          theta = [variance, weight_variance (1, or n_active if ard), bias_variance] in GPy's link order
 *                          (:36-45), every one positive; gradients come back in theta order (:98-123).  Not stationary:
 *                          K(x, x) = var (2/pi) asin(p / (p + 1)) depends on the point (:61-64).  dK/dx (:124-130) serves
 *                          mi355gp_gradients_X (X2 == NULL: the weights c + c^T of :124-127) and, with dKdiag/dx (:133-147),
 *                          mi355gp_predictive_gradients_sum.
 *   MI355GP_POLY           the polynomial kernel (kern/src/poly.py:15-49, GPy.kern.Poly): k(x, x') = var (a x.x' + c)^order.
 *                          theta = [variance, scale, bias, order], the first three positive, order >= 1 and fixed (no
 *                          parameter: its gradient slot is written as 0 so that theta and dtheta have the same length).
 *                          A negative base follows C pow().  The reference has no gradients_X for it (:45-49):
 *                          mi355gp_gradients_X and mi355gp_predictive_gradients_sum reject the kind.
 * Both alone, as a summand or as a factor of a product term.  mi355gp_kern_Kdiag (no X argument) and the sparse and grid
 * paths reject both. */

/* The exact-GP entry points (single kind and part lists, the Laplace / EP session included), mi355gp_predictive_gradients_sum
 * and the stateless mi355gp_kern_K / mi355gp_kern_Kdiag / mi355gp_update_gradients_full / mi355gp_gradients_X also take the
 * three oscillating stationary kinds, functions of the scaled distance r = sqrt(sum_q ((x_q - x'_q) / l_q)^2) alone:
 *   MI355GP_COSINE         k = var cos r (kern/src/stationary.py:664-680, GPy.kern.Cosine)
 *   MI355GP_SINC           k = var sinc(2 r) = var sin(2 pi r) / (2 pi r), 1 at r = 0 (:717-743, GPy.kern.Sinc)
 *   MI355GP_EXPQUADCOSINE  k = var exp(-2 pi^2 r^2) cos(2 pi r / T), one component of the spectral-mixture kernel (:682-713,
 *                          GPy.kern.ExpQuadCosine)
 * theta = [variance, lengthscale (1, or n_active if ard)] for Cosine and Sinc, [variance, lengthscale..., period] for
 * ExpQuadCosine (link order :692-695); every value must be positive.  Gradients come back in theta order (the period's from
 * :703-709).  K(x, x) = variance; dK/dr / r is taken as 0 at r = 0 (the _inv_dist convention, :225-232), so coinciding points
 * add nothing to the lengthscale and X gradients.  Alone, as a summand or as a factor of a product term.  The kinds are positive
 * definite over ONE input dimension only (cos |x - x'| is not for D > 1): give them one active column.  The sparse, grid and
 * psi-statistics paths reject all three. */

/* One part of a sum-of-products kernel expression (GPy.kern.Add, kern/src/add.py:58-84; GPy.kern.Prod,
 * kern/src/prod.py:58-99).  theta = [variance, lengthscale (1, or n_active if ard)] (static kinds: [variance]);
 * active_dims: the input columns this part acts on (kern/src/kern.py:49-53,112-117), NULL / n_active == 0 = all columns.
 * term: 0 = the part is a summand of its own; parts sharing the same NONZERO term id are multiplied element-wise and
 * their product is one summand: K = sum_t prod_{f in t} k_f.  Gradients come back per part, in part order. */
typedef struct {
    int kind;
    int ard;
    int n_active;
    const int* active_dims;
    const double* theta;
    int term;
} mi355gp_part;

/* which device-resident matrix mi355gp_fetch() materialises on the host (all N x N) */
enum {
    MI355GP_FETCH_L = 0,      /* Cholesky factor of Ky, strict upper triangle zero  (Posterior.woodbury_chol) */
    MI355GP_FETCH_KINV = 1,   /* Ky^-1, symmetric                                    (Posterior.woodbury_inv)  */
    MI355GP_FETCH_DLDK = 2,   /* dL_dK = 0.5*(alpha alpha^T - Dy*Ky^-1), symmetric   (grad_dict['dL_dK'])      */
    MI355GP_FETCH_K = 3       /* K(X,X) without noise/jitter, symmetric              (Posterior._K)            */
};

/* out_scalars[] layout of mi355gp_exact_inference / mi355gp_inference_given_K */
enum {
    MI355GP_OUT_LML = 0,        /* log marginal likelihood (without Z_tilde)            */
    MI355GP_OUT_LOGDET = 1,     /* log det Ky                                           */
    MI355GP_OUT_DATAFIT = 2,    /* sum(alpha * R)                                       */
    MI355GP_OUT_DNOISE = 3,     /* dL/d sigma_n^2 = trace(dL_dK)                        */
    MI355GP_OUT_TRKINV = 4,     /* trace(Ky^-1)                                         */
    MI355GP_NUM_OUT = 8
};

/* stage_ms[] layout (hipEvent timings of the last inference call, milliseconds).  Passing stage_ms makes the call run plain
 * launches: below N = 6144 a context otherwise replays its factorisation region (potrf, trtri, alpha solve, lauum) from a hipGraph
 * captured at its second evaluation (MI355GP_GRAPH=0 disables it), and graph nodes carry no timing events. */
enum {
    MI355GP_T_KBUILD = 0, MI355GP_T_POTRF = 1, MI355GP_T_TRTRI = 2, MI355GP_T_LAUUM = 3,
    MI355GP_T_SOLVE = 4, MI355GP_T_GRAD = 5, MI355GP_T_TOTAL = 6, MI355GP_NUM_T = 8
};

/* ---- library / device ------------------------------------------------------------------------- */
const char* mi355gp_last_error(void);
const char* mi355gp_version(void);
int mi355gp_device_count(int* count);
/* hipDeviceSynchronize on `device`: everything the library has enqueued there is complete on return.  (Every compute entry
   point already returns after its own stream has drained; this is the device-wide fence a timing harness brackets a region
   with -- bench.py -- without importing a second HIP runtime user into the process.) */
int mi355gp_device_synchronize(int device);

/* ---- context ------------------------------------------------------------------------------------ */
int mi355gp_create(int device, mi355gp_ctx** ctx);
int mi355gp_destroy(mi355gp_ctx* ctx);

/* Uploads the training set once (X is constant across optimiser iterations: core/gp.py:44-60).
 * X: N x D, R: N x Dy (= Y - mean_function.f(X), exact_gaussian_inference.py:42-50). */
int mi355gp_set_data(mi355gp_ctx* ctx, const double* X, int64_t N, int D, const double* R, int Dy);
/* replaces only the targets (same N, Dy) */
int mi355gp_set_targets(mi355gp_ctx* ctx, const double* R, int Dy);

/* ---- kernel functions (replace Stationary.K / Kdiag / update_gradients_full) ------------------------ */
/* K(X, X2) -> K_out (N x M, row-major).  X2 == NULL: symmetric case (M = N, exact `variance` on the diagonal).
 * Replaces kern/src/stationary.py:105-168 (+ K_of_r: rbf.py:51-52, stationary.py:382-383,488-489,585-586). */
int mi355gp_kern_K(int device, int kind, int ard, const double* theta, const double* X, int64_t N,
                   const double* X2, int64_t M, int D, double* K_out);
/* Kdiag(X) (kern/src/stationary.py:170-173) */
int mi355gp_kern_Kdiag(int kind, const double* theta, int64_t N, double* out);
/* dL/dtheta from a caller-supplied dL_dK (N x M, row-major, need not be symmetric).
 * Replaces Stationary.update_gradients_full (kern/src/stationary.py:193-243) incl. the native
 * lengthscale_grads loop (kern/src/stationary_cython.pyx:53-62).  dtheta_out: 1 + (ard ? D : 1); RatQuad / StdPeriodic:
 * as long as their theta (RatQuad.update_gradients_full stationary.py:790-798, StdPeriodic standard_periodic.py:501-526). */
int mi355gp_update_gradients_full(int device, int kind, int ard, const double* theta, const double* dL_dK,
                                  const double* X, int64_t N, const double* X2, int64_t M, int D,
                                  double* dtheta_out);

/* dL/dX (N x D) from dL_dK (N x M): Stationary.gradients_X (kern/src/stationary.py:245-252,330-358, native loop
 * kern/src/stationary_utils.c:1-14).  X2 == NULL: the symmetric form (tmp + tmp^T against X itself).  Any D (the reductions run in groups of 32 dimensions).
 * StdPeriodic: StdPeriodic.gradients_X (kern/src/standard_periodic.py:574-580), a row reduction over X2. */
int mi355gp_gradients_X(int device, int kind, int ard, const double* theta, const double* dL_dK, const double* X,
                        int64_t N, const double* X2, int64_t M, int D, double* out);

/* ---- the fused hot path ---------------------------------------------------------------------------- */
/* One GP.parameters_changed (core/gp.py:278-280) with everything N x N resident in HBM:
 *   K = kern.K(X); Ky = K + (noise + jitter + extra_jitter) I; L = chol(Ky); alpha = Ky^-1 R;
 *   LML; Ky^-1; dL_dK (never materialised); dL/dtheta; dL/dnoise; diag(dL_dK).
 * Replaces ExactGaussianInference.inference (inference/latent_function_inference/exact_gaussian_inference.py:37-74),
 * pdinv/jitchol/dpotrs/dpotri/dtrtri/tdot/symmetrify (util/linalg.py:56-75,116-145,193-227,299-379),
 * Gaussian.exact_inference_gradients (likelihoods/gaussian.py:78-79) and
 * Stationary.update_gradients_full (kern/src/stationary.py:193-243) applied to that dL_dK.
 *   noise: noise_len == 1 (homoscedastic) or N values; jitter: the reference's 1e-8 (exact_gaussian_inference.py:56);
 *   extra_jitter: the jitchol ladder term (util/linalg.py:66-72), 0 on the first attempt;
 *   out_scalars[MI355GP_NUM_OUT]; alpha_out (N x Dy) / dtheta_out / diag_dLdK_out (N) / stage_ms[MI355GP_NUM_T] may be NULL.
 * Returns info > 0 when Ky is not positive definite (the caller runs the ladder). */
int mi355gp_exact_inference(mi355gp_ctx* ctx, int kind, int ard, const double* theta,
                            const double* noise, int64_t noise_len, double jitter, double extra_jitter,
                            double* out_scalars, double* alpha_out, double* dtheta_out,
                            double* diag_dLdK_out, double* stage_ms);

/* The same evaluation for a SUM of kernels: Ky = sum_p K_p(X) + (noise + jitter) I.  dtheta_out is the concatenation of the
 * parts' gradients, each [variance, lengthscale(s)] ([variance] for White / Bias), in part order -- the order
 * GPy's Add links its parts (kern/src/add.py:24-45). */
int mi355gp_exact_inference_sum(mi355gp_ctx* ctx, int nparts, const mi355gp_part* parts, const double* noise,
                                int64_t noise_len, double jitter, double extra_jitter, double* out_scalars,
                                double* alpha_out, double* dtheta_out, double* diag_dLdK_out, double* stage_ms);

/* Student-t PROCESS inference (ExactStudentTInference.inference, exact_studentt_inference.py:20-52) for a sum of parts:
 * Ky = K + jitter I (the reference's 1e-8), dL_dK = 0.5 ((nu+N)/(nu+beta-2) alpha alpha^T - Dy Ky^-1), beta = sum(alpha*R).
 * out_scalars: [LML] Student-t log marginal, [LOGDET], [DATAFIT] = beta, [5] = (nu+N)/(nu+beta-2) (dL_dm = that * alpha). */
int mi355gp_exact_studentt_sum(mi355gp_ctx* ctx, int nparts, const mi355gp_part* parts, double nu, double jitter,
                               double extra_jitter, double* out_scalars, double* alpha_out, double* dtheta_out,
                               double* stage_ms);

/* Same with a caller-supplied covariance matrix (the `K=` argument of ExactGaussianInference.inference,
 * exact_gaussian_inference.py:52-53; used by EP and by foreign kernels).  K_host: N x N row-major. No dtheta. */
int mi355gp_inference_given_K(mi355gp_ctx* ctx, const double* K_host, const double* noise, int64_t noise_len,
                              double jitter, double extra_jitter, double* out_scalars, double* alpha_out,
                              double* diag_dLdK_out, double* stage_ms);

/* Lazy materialisation of a device-resident N x N result of the last inference call. */
int mi355gp_fetch(mi355gp_ctx* ctx, int which, double* out, int fortran_order);

/* Posterior prediction on device (PosteriorExact._raw_predict, inference/latent_function_inference/posterior.py:273-302):
 * mu (M x Dy) = K(Xnew,X) alpha; full_cov == 0: var (M) = Kdiag - sum((L^-1 Kx)^2, 0); else var (M x M). */
int mi355gp_predict(mi355gp_ctx* ctx, int kind, int ard, const double* theta, const double* Xnew, int64_t M,
                    double* mu_out, double* var_out, int full_cov);

/* the same for a sum kernel (White parts contribute to Kdiag only, as GPy's White.K(X, X2) = 0: static.py:77-81) */
int mi355gp_predict_sum(mi355gp_ctx* ctx, int nparts, const mi355gp_part* parts, const double* Xnew, int64_t M,
                        double* mu_out, double* var_out, int full_cov);

/* GP.predictive_gradients (core/gp.py:418-474) for a sum of stationary (+ White / Bias) parts, no product terms, any D:
 *   dmu_out  (M x D x Dy, row-major)  d mean[m][d] / d Xnew[m][q] = kern.gradients_X(woodbury_vector[:, d]^T, Xnew, X)  (:448-451)
 *   dvar_out (M x D)                  d var[m]    / d Xnew[m][q] = gradients_X_diag (0 for stationary kernels,
 *                                     stationary.py:360-361) + kern.gradients_X(-2 K(Xnew, X) Ky^-1, Xnew, X)           (:454,462-465)
 * Ky^-1 K(X, Xnew) is formed on the device as X^T (X K(X, Xnew)) with X = L^-1 from the last inference call; nothing N x N or
 * N x M crosses PCIe.  Either output may be NULL. */
int mi355gp_predictive_gradients_sum(mi355gp_ctx* ctx, int nparts, const mi355gp_part* parts, const double* Xnew, int64_t M,
                                     double* dmu_out, double* dvar_out);

/* ---- Laplace approximation for a non-Gaussian likelihood (one output column) ---------------------------------------------
 * The N x N work of Laplace.inference (inference/latent_function_inference/laplace.py:122-353) as a session on an exact
 * context; the likelihood's derivatives are O(N) host work and travel as vectors, nothing N x N crosses PCIe.  Call order:
 * begin, newton (once per iteration of the mode search), finish, gradients, then predict / fetch as often as needed.  Any
 * exact / Student-t / given-K evaluation on the context ends the session (and the other way round); both give their usual
 * bits afterwards.  The first begin of a context allocates a fourth N x N buffer for K and the session's vectors. */
/* K = kern.K(X) for the part list (laplace.py:129; add.py:58-72, prod.py:58-65): no noise, no jitter, the exact Kdiag on the
 * diagonal; resident until the next begin / set_data. */
int mi355gp_laplace_begin(mi355gp_ctx* ctx, int nparts, const mi355gp_part* parts);
/* One iteration of rasm_mode (laplace.py:184-199) for W = -d2logpdf_df2(f) (N, finite, >= 0) and b = W f + dlogpdf_df(f):
 * B = I + W^1/2 K W^1/2 + extra_jitter I, its Cholesky factor and inverse factor (_compute_B_statistics, :333-338, without
 * the N^3 products), a_out = b - W^1/2 B^-1 W^1/2 K b (the full-step Ki_f, :195-198), Ka_out = K a_out -- f_trial =
 * K (Ki_f + s dKi_f) is linear in the step s, so the line search (:202-208) is host work on these two vectors -- and
 * *logdet_out (optional) = 2 sum log diag L_B.  Returns info > 0 when B is not positive definite (the caller runs jitchol's
 * ladder through extra_jitter, util/linalg.py:56-75). */
int mi355gp_laplace_newton(mi355gp_ctx* ctx, const double* W, const double* b, double extra_jitter, double* a_out,
                           double* Ka_out, double* logdet_out);
/* The B statistics at the mode (laplace.py:247, :333-351) for W at f_hat: diagKiWi_out (N) = diag(K - K K_Wi_i K) =
 * Kdiag - colsumsq(L_B^-1 W^1/2 K) (:347-348), *logdet_out = logdet_I_KW (:351); B^-1 stays resident for gradients / fetch. */
int mi355gp_laplace_finish(mi355gp_ctx* ctx, const double* W, double extra_jitter, double* diagKiWi_out, double* logdet_out);
/* Kernel gradients at the mode (laplace.py:257-272 with kern.update_gradients_full applied to that dL_dK): Ki_f = Ki_fhat,
 * dL_dfhat = -0.5 diag(Ki_W_i) dW_df (both N).  dL_dK = 0.5 (Ki_f Ki_f^T - K_Wi_i) + Ki_f dL_dfhat^T (I - K K_Wi_i) is formed
 * on the device in its symmetrised form (every dK/dtheta is symmetric, so the gradients are the same) and reduced per part;
 * dtheta_out as in mi355gp_exact_inference_sum.  Afterwards mi355gp_fetch gives MI355GP_FETCH_DLDK = that symmetrised
 * dL_dK, MI355GP_FETCH_KINV = K_Wi_i = W^1/2 B^-1 W^1/2 (the posterior's woodbury_inv, :338) and MI355GP_FETCH_K = K;
 * MI355GP_FETCH_L is an error (there is no Cholesky factor of Ky). */
int mi355gp_laplace_gradients(mi355gp_ctx* ctx, const double* Ki_f, const double* dL_dfhat, double* dtheta_out);
/* The implicit term of the likelihood-parameter gradients at the mode (laplace.py:276-299).  The reference forms, per
 * likelihood parameter i, dfhat_dthetaL = (I - K K_Wi_i) K g_i with g_i = d(dlogpdf_df)/dthetaL_i (:293) and then
 * dL_dfhat^T dfhat_dthetaL (:295).  K and K_Wi_i are symmetric, so that scalar is s^T g_i with the one vector
 *   s_out (N) = K u,  u = dL_dfhat - K_Wi_i K dL_dfhat  (the u of mi355gp_laplace_gradients, formed by the same code),
 * whatever the number of parameters: the products with g_i are O(N) host work.  Two N-vectors cross PCIe, nothing N x N.
 * Needs mi355gp_laplace_finish; may be called before or after mi355gp_laplace_gradients and leaves every matrix of the
 * session (K, B^-1, a resident dL_dK) as it is.  Fixed-order reductions: the same input gives the same bytes. */
int mi355gp_laplace_implicit(mi355gp_ctx* ctx, const double* dL_dfhat, double* s_out);
/* Posterior._raw_predict for Posterior(woodbury_vector = Ki_fhat, woodbury_inv = K_Wi_i, K) (posterior.py:198-262 as built at
 * laplace.py:146): mu_out (M) = K(Xnew, X) wv; full_cov == 0: var_out (M) = Kdiag(Xnew) - colsumsq(L_B^-1 W^1/2 K(X, Xnew)),
 * else M x M.  `parts` = the kernel of the session; needs mi355gp_laplace_finish. */
int mi355gp_laplace_predict(mi355gp_ctx* ctx, int nparts, const mi355gp_part* parts, const double* Xnew, int64_t M,
                            const double* wv, double* mu_out, double* var_out, int full_cov);

/* ---- Expectation propagation inside a Laplace session (one output column, zero prior mean) -----------------------------------
 * The two parts of EP.expectation_propagation (inference/latent_function_inference/expectation_propagation.py:279-310) that are
 * EP and nothing else; they need mi355gp_laplace_begin (K resident).  After convergence the session's own calls give the rest
 * with W = tau_tilde, b = v_tilde: mi355gp_laplace_newton returns alpha (:386-387), mu and log det B (:367), then
 * mi355gp_laplace_finish, mi355gp_laplace_gradients(Ki_f = alpha, dL_dfhat = 0) (dL_dK = 0.5 (alpha alpha^T - Wi), :393) and
 * mi355gp_laplace_predict (PosteriorEP._raw_predict, posterior.py:305-336). */
enum { MI355GP_EP_BERNOULLI_PROBIT = 0 };
/* posteriorParams._recompute (:129-143): B = I + S^1/2 K S^1/2 + extra_jitter I with S = diag(tau) (N, finite, >= 0), its factor
 * (info > 0 when not positive definite, as mi355gp_laplace_newton), mu_out (N) = K alpha with alpha = v - S^1/2 B^-1 S^1/2 K v,
 * sigdiag_out (N) = diag(Sigma) + add_diag, *logdet_out (optional) = 2 sum log diag L_B.  want_sigma != 0: the full symmetric
 * Sigma = K - V^T V, V = L_B^-1 S^1/2 K (:136-137), is formed in one of the session's work buffers with add_diag on its diagonal
 * (the 1e-7 of _init_approximations, :319, :326) and stays resident, with mu, for mi355gp_ep_sweep; any other session call
 * overwrites it.  want_sigma == 0: only the diagonal, Kdiag - colsumsq(V).  tau = v = 0 gives Sigma = K + add_diag I, mu = 0
 * (the cold start of :316-321).  *ms_out (optional): device time of the enqueued work between two events. */
int mi355gp_ep_recompute(mi355gp_ctx* ctx, const double* tau, const double* v, double extra_jitter, double add_diag,
                         int want_sigma, double* mu_out, double* sigdiag_out, double* logdet_out, double* ms_out);
/* One pass of _local_updates (:330-351) with parallel_updates=False over the sites in `order` (N, a permutation of 0 .. N-1), on
 * the device: cavity (:27-29), moment matching of likelihood `lik` (MI355GP_EP_BERNOULLI_PROBIT: bernoulli.py:73-79, carried
 * as log Z_hat), site update with fractional power eta, damping delta and the clamp of tau at machine epsilon (:52-68), rank-one
 * update of mu and Sigma (:101-105).  ysign (N): +1 / -1 per row.  tau, v (N): in / out.  cav_tau_out, cav_v_out, logZhat_out
 * (N, by site), mu_out, sigdiag_out (N, after the sweep).  2 N launches on the context's stream, no host synchronisation inside;
 * the same inputs give the same bits.  Needs mi355gp_ep_recompute with want_sigma as the last session call (or a sweep). */
int mi355gp_ep_sweep(mi355gp_ctx* ctx, int lik, const int64_t* order, const double* ysign, double eta, double delta, double* tau,
                     double* v, double* cav_tau_out, double* cav_v_out, double* logZhat_out, double* mu_out, double* sigdiag_out,
                     double* ms_out);

/* Posterior covariance between two point sets (Posterior.covariance_between_points, posterior.py:109-130) */
int mi355gp_covariance_between_points(mi355gp_ctx* ctx, int nparts, const mi355gp_part* parts, const double* X1,
                                      int64_t M1, const double* X2, int64_t M2, double* out);

/* ---- standalone dense routines (dpotrf / dpotri equivalents; also what bench.py times in isolation) --- */
/* In-place lower Cholesky of a host matrix (row-major N x N, lower triangle read), strict upper zeroed on return.
 * Replaces lapack.dpotrf(A, lower=1) (util/linalg.py:58).  ms (optional): device time of the factorisation. */
int mi355gp_potrf(int device, double* A, int64_t N, double* ms);
/* Ainv (symmetric, full) from A; replaces pdinv's dpotrf+dpotri+symmetrify (util/linalg.py:193-214). */
int mi355gp_pdinv(int device, const double* A, int64_t N, double* Ainv, double* L_out, double* logdet, double* ms);
/* the same with the third member of GPy's pdinv tuple, Li = L^-1 (dtrtri, linalg.py:207): (Ai, L, Li, logdet) */
int mi355gp_pdinv_full(int device, const double* A, int64_t N, double* Ainv, double* L_out, double* Li_out, double* logdet,
                       double* ms);

/* Options of ONE context, set through the ABI (the MI355GP_* environment variables of DESIGN.md 6e only provide the
 * process-wide DEFAULTS that a context starts from; an option set here survives mi355gp_set_data).
 * PROFILE: bracket launches of the factorisation kernels with hipEvents on the launching stream (adds ~2 us per timed
 *   launch).  value 0 = off, 1 = all families, otherwise (bitmask of 1 << MI355GP_PF_*) << 1;
 * LOOKAHEAD: 1 (default) factor panel k+1 on a second, high-priority stream while the trailing update of step k still
 *   runs; 0 = everything in order on one stream (reference schedule);
 * the schedule switches (value -1 = back to the process default): TRI_OVERLAP 0/1 inverse of the leading block underneath
 *   potrf; TRI_MIN_NT smallest number of 128-tiles for that overlap (and for PART1_ON_PANEL); TRI_H leading tiles inverted
 *   early (0 = time model); TRI_WGS workgroups of the early T21 instance (0 = CU share); TRI_HALF 0/1 allow the
 *   two-shader-engine side stream; PART1_ON_PANEL 0/1; NBO outer panel width (multiple of 128, 0 = default 512);
 *   SOLVE_OVERLAP 0/1 alpha underneath lauum; DIAG_EXCL_FIRST 0/1; GRAPH 0/1 hipGraph replay of the factorisation region
 *   below the overlap threshold; PERSIST 0/1 the single-launch dataflow Cholesky for small N. */
enum { MI355GP_OPT_PROFILE = 0, MI355GP_OPT_LOOKAHEAD = 1, MI355GP_OPT_TRI_OVERLAP = 2, MI355GP_OPT_TRI_MIN_NT = 3,
       MI355GP_OPT_TRI_H = 4, MI355GP_OPT_TRI_WGS = 5, MI355GP_OPT_TRI_HALF = 6, MI355GP_OPT_PART1_ON_PANEL = 7,
       MI355GP_OPT_NBO = 8, MI355GP_OPT_SOLVE_OVERLAP = 9, MI355GP_OPT_DIAG_EXCL_FIRST = 10, MI355GP_OPT_GRAPH = 11,
       MI355GP_OPT_PERSIST = 12, MI355GP_OPT_AGG2 = 13, MI355GP_OPT_PERSIST_TEST = 14, MI355GP_OPT_PERSIST_ABORTS = 15,
       MI355GP_OPT_PERSIST_SKIP = 16, MI355GP_OPT_PERSIST_SCHED = 17, MI355GP_OPT_NUM = 18 };
/* MI355GP_OPT_PERSIST_TEST: test hook, consumed by the NEXT persistent launch of the context: 1 = the launch waits for one
   workgroup more than it has (called off at the co-residency gate, matrix untouched), 2 = the chain workgroup aborts after the
   gate (dirty abort, matrix rebuilt), 3 = the first gate kernel of the early inverse underneath the launch gives up at once (what
   its 20 ms limit does on a GPU shared with something heavy: the evaluation is marked aborted because the kernels behind the gate
   read unfinished rows); either way the evaluation is redone on the launch-per-step schedule inside the same call.
   MI355GP_OPT_PERSIST_ABORTS / _SKIP: read-only (mi355gp_get_option): persistent launches of this context that did not
   complete / evaluations that still stay on the launch-per-step schedule because of the last one.
   MI355GP_OPT_PERSIST_SCHED: read-only: the schedule of a small factorisation this context has settled on, by its own timing of
   the two or by an explicit PERSIST option: 0 = not decided yet (the first evaluations),
   1 = the persistent launch, 2 = launches (this box runs them faster, or PERSIST = 0). */
int mi355gp_set_option(mi355gp_ctx* ctx, int option, int value);
/* the value in effect for a schedule switch (options above MI355GP_OPT_PROFILE) */
int mi355gp_get_option(mi355gp_ctx* ctx, int option, int* value);
/* kernel families of mi355gp_get_profile */
enum { MI355GP_PF_UPDATE = 0 /* k_update_nt<4,true>: trailing update of potrf on 128 x 128 tiles */, MI355GP_PF_TRTRI = 1, MI355GP_PF_LAUUM = 2,
       MI355GP_PF_DIAG = 3 /* k_diag128 */, MI355GP_PF_TRSM = 4 /* k_trsm128 */,
       MI355GP_PF_UPDATE64 = 5 /* k_update_nt64: the same update on 64 x 64 tiles (launches of few tiles) */,
       MI355GP_PF_PERSIST = 6 /* k_potrf_persist: the whole factorisation of a small matrix as one persistent launch */,
       MI355GP_PF_TRTRI_EARLY = 7 /* the part of the triangular inverse that runs on the CU-masked side stream UNDERNEATH potrf
                                     (inverse of the leading block + its share of T21 = L21 X11): elapsed time on that stream;
                                     MI355GP_PF_TRTRI is the part exposed after potrf, and carries the flops of both */,
       MI355GP_PF_NUM = 8 };
/* Per family, for the last inference call made with PROFILE on: summed launch durations (ms), summed ALGORITHMIC
 * flops of those launches, launch count.  Arrays of MI355GP_PF_NUM. */
int mi355gp_get_profile(mi355gp_ctx* ctx, double* ms, double* flops, int* launches);

/* ---- optional multi-GPU mode: 2D block-cyclic factorisation on a Pr x Pc process grid ---------------------------
 * (north_star config 4; no GPy counterpart -- GPy's only parallel code is the mpi4py sparse GP,
 *  inference/latent_function_inference/var_dtc_parallel.py).  One process per GPU; rank = pr*Pc + pc.
 * Rank 0 obtains a 128-byte RCCL id with mi355gp_grid_unique_id and ships it to the others by any host channel
 * (bench.py / gpy_amd/grid.py use torch.distributed or a file); every rank then calls mi355gp_grid_create with it.
 * id128 == NULL selects the LOOPBACK transport: all Pr*Pc logical ranks live in this process on `device`
 * (correctness testing on one GPU); `rank` is ignored then.  nb: tile edge, multiple of 128. */
typedef struct mi355gp_grid mi355gp_grid;
int mi355gp_grid_unique_id(void* id128);
int mi355gp_grid_create(int device, int rank, int world, int Pr, int Pc, int nb, const void* id128, mi355gp_grid** out);
int mi355gp_grid_destroy(mi355gp_grid* g);
/* every rank passes the full X (N x D) and R (N x Dy) */
int mi355gp_grid_set_data(mi355gp_grid* g, const double* X, int64_t N, int D, const double* R, int Dy);
/* same contract and outputs as mi355gp_exact_inference; results are replicated on every rank.  Collective.
 * stage_ms: KBUILD, POTRF (= the whole one-pass factorisation + inversion), SOLVE, GRAD, TOTAL. */
int mi355gp_grid_exact_inference(mi355gp_grid* g, int kind, int ard, const double* theta, const double* noise,
                                 int64_t noise_len, double jitter, double extra_jitter, double* out_scalars,
                                 double* alpha_out, double* dtheta_out, double* diag_dLdK_out, double* stage_ms);
/* tiles owned by this process's ranks, written at their global position of an N x N row-major array (lower triangle);
 * which = MI355GP_FETCH_L or MI355GP_FETCH_LINV */
#define MI355GP_FETCH_LINV 100
int mi355gp_grid_fetch(mi355gp_grid* g, int which, double* out);
/* Schedule options of one grid (every rank must set the same values; takes effect at the next inference call).
 *   MI355GP_GRID_OPT_LOOKAHEAD: 1 = critical path one group ahead on a second stream (default), 0 = in order on one stream
 *   MI355GP_GRID_OPT_G        : steps per group of the two-level blocked factorisation: tiles beyond the group receive the
 *                               group's panels in ONE pass with K = G * nb (default 1 = one rank-nb update per step; measured best on the loopback grid)
 *   MI355GP_GRID_OPT_GW       : steps per update of Kinv = X^T X; default 4; 0 = one deep-K pass after the last step
 *   MI355GP_GRID_OPT_CHECK_SEQ: 1 = after every evaluation compare, inside every communicator, the members' logs of the
 *                               collectives they enqueued (operation, root, size, in order): RCCL matches collectives by order,
 *                               so a divergence is a dead-lock or a wrong panel in waiting; error -7 names the ranks
 * value -1 restores the process default (environment MI355GP_GRID_LOOKAHEAD / _G / _GW / _CHECK_SEQ, else the built-in one). */
enum { MI355GP_GRID_OPT_LOOKAHEAD = 0, MI355GP_GRID_OPT_G = 1, MI355GP_GRID_OPT_GW = 2, MI355GP_GRID_OPT_CHECK_SEQ = 3,
       MI355GP_GRID_OPT_NUM = 4 };
int mi355gp_grid_set_option(mi355gp_grid* g, int option, int value);
int mi355gp_grid_get_option(mi355gp_grid* g, int option, int* value);
/* The collective log of the LAST evaluation of logical rank `rank` (loopback transport: any rank of the grid; one rank per
 * process: the caller's own): out9 = [collectives on the world / row / column communicator, then per communicator an FNV-1a hash
 * over (operation, root, doubles) as (high 32 bits, low 32 bits)]. */
int mi355gp_grid_coll_log(mi355gp_grid* g, int rank, double* out9);
/* ---- sparse GP (VarDTC) path: BASELINE config 5 -----------------------------------------------------------------
 * One SparseGP.parameters_changed (core/sparse_gp.py:76-119) for certain inputs and a homoscedastic Gaussian likelihood:
 * VarDTC.inference (inference/latent_function_inference/var_dtc.py:66-215, helpers :217-276) + the kernel and
 * inducing-input gradient assembly of SparseGP._update_gradients (sparse_gp.py:108-118), streamed over row chunks of X
 * like the reference's own VarDTC_minibatch (var_dtc_parallel.py:72-133).  X: N x D, Y: N x Dy, Z: M x D.
 *   out_scalars: [0] log marginal likelihood, [1] dL/d(noise variance), [2] trace(A), [3] data_fit,
 *                [4] sum(log diag LB), [5] beta
 *   dtheta_out: 1 + (ard ? D : 1) (variance, lengthscales; diag + Knm + Kmm terms summed as sparse_gp.py:110-115)
 *   dZ_out: M x D = gradients_X(dL_dKmm, Z) + gradients_X(dL_dKnm^T, Z, X) (sparse_gp.py:116-118)
 *   wv_out (optional): woodbury_vector M x Dy;  stage_ms (optional, 4): pass 1, M x M algebra, pass 2, total
 * Returns info > 0 if Kmm or B is not positive definite (the caller runs the jitchol ladder via extra_jitter). */
typedef struct mi355gp_sparse mi355gp_sparse;
int mi355gp_sparse_create(int device, mi355gp_sparse** out);
int mi355gp_sparse_destroy(mi355gp_sparse* s);
int mi355gp_sparse_set_data(mi355gp_sparse* s, const double* X, int64_t N, int D, const double* Y, int Dy);
int mi355gp_vardtc_inference(mi355gp_sparse* s, int kind, int ard, const double* theta, const double* Z, int64_t M,
                             double noise_var, double extra_jitter, double* out_scalars, double* dtheta_out,
                             double* dZ_out, double* wv_out, double* stage_ms);
/* The same evaluation for a SUM of kernel parts (GPy.kern.Add of stationary / White / Bias kernels with active_dims,
 * kern/src/add.py:58-88, static.py:63-98,151-173; product terms are not accepted here), scalar OR per-point noise
 * variances (heteroscedastic precision: var_dtc.py:78-86,126-129,224-226,240-256,267-269; any Dy) and targets
 * R = Y - mean_function.f(X) uploaded by mi355gp_sparse_set_data (var_dtc.py:73-76,88-89).
 *   noise: noise_len == 1 or N (the rows of this context) noise VARIANCES
 *   out_scalars: as above; [1] (dL/d noise variance) only for noise_len == 1
 *   dtheta_out: concatenation over the parts, each [variance, lengthscale(s)] ([variance] for White / Bias)
 *   dnoise_rows_out (N x Dy, required for noise_len == N): dL_dR per point and output column = what
 *                                likelihood.exact_inference_gradients receives (var_dtc.py:240-256 as written there)
 *   dLdm_out (optional, N x Dy): dL_dm = beta R - K(X, Z) woodbury_vector (var_dtc.py:148; SparseGP hands it to
 *                                mean_function.update_gradients, sparse_gp.py:84-85) */
int mi355gp_vardtc_inference_sum(mi355gp_sparse* s, int nparts, const mi355gp_part* parts, const double* Z, int64_t M,
                                 const double* noise, int64_t noise_len, double extra_jitter, double* out_scalars,
                                 double* dtheta_out, double* dZ_out, double* wv_out, double* dnoise_rows_out,
                                 double* dLdm_out, double* stage_ms);
/* Uncertain inputs q(x_n) = N(X_n, diag S_n) (SparseGPRegression(X, Y, X_variance=S), var_dtc.py with psi statistics,
 * kern/src/psi_comp/rbf_psi_comp.py).  S: N x D, the shape of set_data's X (then read as the means); every entry positive and
 * finite, checked on the host before any launch.  set_data discards S. */
int mi355gp_sparse_set_input_variance(mi355gp_sparse* s, const double* S, int64_t N, int D);
/* Replaces the inputs of set_data and nothing else: X (N x D, the means when the inputs are uncertain) and, with S != NULL, the
 * input variances.  Y and everything sized by Y stay resident: this is the upload of one Bayesian GPLVM step, where every mean
 * and variance of q(X) changes and Y (N x Dy, the wide matrix) does not.  N, D must be set_data's; S is validated as
 * mi355gp_sparse_set_input_variance validates it; a row-sharded context is refused; the last result is forgotten. */
int mi355gp_sparse_set_inputs(mi355gp_sparse* s, const double* X, const double* S, int64_t N, int D);
/* One evaluation with uncertain inputs: one RBF part (iso or ARD, any active_dims) alone or summed with White parts; ONE
 * noise variance (noise_len == 1).  Anything else -- a Bias part, a second RBF, a product, per-point noise, a row-sharded
 * context, no input variances -- is refused with an error that names it.  out_scalars, dtheta_out, dZ_out, wv_out, stage_ms
 * as mi355gp_vardtc_inference_sum; dmu_out / dS_out (optional, N x D): gradients with respect to the inputs' means and
 * variances.  The context ends in the state of a certain-input call: mi355gp_sparse_predict and mi355gp_sparse_fetch work
 * (mi355gp_sparse_fetch_dLdKnm does not: dL_dpsi1 / dL_dpsi2 take dL_dKnm's place).  Two calls give the same bits. */
int mi355gp_vardtc_inference_uncertain(mi355gp_sparse* s, int nparts, const mi355gp_part* parts, const double* Z, int64_t M,
                                       const double* noise, int64_t noise_len, double extra_jitter, double* out_scalars,
                                       double* dtheta_out, double* dZ_out, double* wv_out, double* dmu_out, double* dS_out,
                                       double* stage_ms);
/* Sparse posterior prediction on the device (Posterior._raw_predict, inference/latent_function_inference/posterior.py:198-262,
 * for the (woodbury_inv, woodbury_vector) posterior of var_dtc.py:213): mu (Mn x Dy) = K(X*, Z) woodbury_vector;
 * full_cov == 0: var (Mn) = Kdiag - sum(Kx * (woodbury_inv Kx), 0), clipped at 1e-15 (posterior.py:248); else Mn x Mn.
 * `parts` = the kernel of the last inference call. */
int mi355gp_sparse_predict(mi355gp_sparse* s, int nparts, const mi355gp_part* parts, const double* Xnew, int64_t Mn,
                           double* mu_out, double* var_out, int full_cov);
/* Prediction at UNCERTAIN new points q(x*) = N(mu_new, diag S_new) (Posterior._raw_predict with a VariationalPosterior,
 * posterior.py:249-269, full_cov = False): mean_out (Mn x Dy) = psi1* woodbury_vector; var_out (optional, Mn x Dy)
 * = psi0* + sum_mo psi2n*[m][o] (lam[m][d] lam[o][d] - woodbury_inv[m][o]) - mean^2, clipped at 1e-15.  `parts` = the kernel
 * of the last VarDTC call (certain or uncertain inputs), one RBF part alone or with White parts; anything else, a context
 * without a result, an SVGP result, a row-sharded context and a non-positive S entry are refused by name.  Neither an
 * Mn x M x M array nor Dy M x M matrices are formed; two calls give the same bits. */
int mi355gp_sparse_predict_uncertain(mi355gp_sparse* s, int nparts, const mi355gp_part* parts, const double* mu_new,
                                     const double* S_new, int64_t Mn, double* mean_out, double* var_out);
/* Time of the last mi355gp_sparse_predict_uncertain call's stream work (HIP events on the launching stream), milliseconds. */
int mi355gp_sparse_get_predict_ms(mi355gp_sparse* s, double* ms_out);
/* Rows [row0, row0 + nrows) of dL_dKnm (nrows x M, row-major) of the last call -- the matrix SparseGP._update_gradients
 * hands to a foreign kernel's update_gradients_full / gradients_X (core/sparse_gp.py:108-118).  It is never resident as a
 * whole (3.3 GB at config 5): the caller walks it in row blocks. */
int mi355gp_sparse_fetch_dLdKnm(mi355gp_sparse* s, int64_t row0, int64_t nrows, double* out);
/* Row-sharded multi-GPU mode (the reference's MPI design, var_dtc_parallel.py:121-130,387-394): every rank holds a
 * slice of the rows of (X, Y); psi2/psi1Y after pass 1 and the gradient sums after pass 2 are all-reduced over RCCL,
 * the M x M algebra is replicated.  Call on every rank before set_data (id128: mi355gp_grid_unique_id on rank 0). */
int mi355gp_sparse_attach_comm(mi355gp_sparse* s, int rank, int world, const void* id128);
/* The same mode over the LOOPBACK transport: `world` contexts of ONE process (one host thread each) that name the same
 * group_key rendezvous for every exchange step and are summed in rank order -- world > 1 on a single GPU (tests). */
int mi355gp_sparse_attach_loopback(mi355gp_sparse* s, int rank, int world, int group_key);
/* M x M results of the last call: 0 dL_dKmm, 1 woodbury_inv (var_dtc.py:206-210), 2 Lm, 3 Kmm (+1e-8 I; after
 * mi355gp_pep_inference: + that call's jitter), 4 psi2, 5 dL_dpsi2_beta (var_dtc.py:220; 4 and 5: VarDTC results only) */
int mi355gp_sparse_fetch(mi355gp_sparse* s, int which, double* out);
/* Launch timing of the two MFMA kernels of the last mi355gp_vardtc_inference_sum call (hipEvent pairs on the launching
 * stream, recorded on every call): out6 = [T = Kfu dL_dpsi2 GEMM: summed ms, algorithmic flops (2 rows M^2), launches,
 * split-K Gram psi2: summed ms, algorithmic flops (rows M^2, lower half), launches]. */
int mi355gp_sparse_get_profile(mi355gp_sparse* s, double* out6);

/* ---- SVGP on the sparse context: minibatches and non-Gaussian likelihoods (Hensman et al. 2013, 2015) -------------------
 * One SVGP.inference (inference/latent_function_inference/svgp.py:10-121) + SVGP.parameters_changed (core/svgp.py:54-71) for
 * certain inputs and a zero mean function is a two-call session around the likelihood's quadrature
 * (likelihood.variational_expectations, svgp.py:77), which stays with the caller: forward -> quadrature -> backward.
 * q(u_d) = N(m_d, L_d L_d^T) for d < L latent functions, 1 <= L <= 16; M inducing points.  Accepted parts: those of
 * mi355gp_vardtc_inference_sum.  A row-sharded context and a context holding input variances are refused.  All reductions run
 * in a fixed order: two sessions on the same inputs give the same bytes.  After an SVGP call mi355gp_sparse_fetch,
 * mi355gp_sparse_fetch_dLdKnm and mi355gp_sparse_predict (they describe VarDTC's result) are refused until the next VarDTC or
 * PEP call.
 *
 * mi355gp_svgp_forward replaces svgp.py:12-56: Kmm = K(Z) with NO 1e-8 term (svgp.py:37, unlike var_dtc.py:93), Lm, Kmm^-1,
 * S_d, S_d^-1, Kmm^-1 m, the KL term (:54-56), and over the context's row chunks A^T = K(X, Z) Kmm^-1, mu = A^T m,
 * v[n,d] = sum_j (A^T L_d)[n,j]^2 + Kdiag - sum_j A^T[n,j] K(X, Z)[n,j] (:45-51).
 *   q_mean: M x L row-major;  q_chol: L matrices M x M row-major whose lower triangles are the L_d (svgp.py:16)
 *   mu_out, v_out: N x L;  scalars_out[2 + L]: [0] KL, [1] log det Kmm, [2 + d] log det S_d;  stage_ms[3] may be NULL
 * Returns LAPACK-style info > 0 when Kmm is not positive definite: retry with extra_jitter as jitchol does (util/linalg.py:56-75). */
int mi355gp_svgp_forward(mi355gp_sparse* s, int nparts, const mi355gp_part* parts, const double* Z, int64_t M, const double* q_mean,
                         const double* q_chol, int L, double extra_jitter, double* mu_out, double* v_out, double* scalars_out,
                         double* stage_ms);
/* mi355gp_svgp_backward replaces svgp.py:84-117 and core/svgp.py:57-65 after a forward call on the same data.  dF_dmu, dF_dv:
 * N x L, already multiplied by batch_scale (svgp.py:80); the weights dF_dv are signed.
 *   dtheta_out: the parts' parameter gradients concatenated (dL_dKmm, dL_dKmn and dL_dKdiag terms summed, core/svgp.py:58-63)
 *   dZ_out: M x D (core/svgp.py:65);  dm_out: M x L = dL_dm (svgp.py:112);  dchol_out: L x M x M, the lower triangle of
 *   dL_dchol_d = 2 dL_dS_d L_d (svgp.py:114), zero above the diagonal;  stage_ms[3] may be NULL */
int mi355gp_svgp_backward(mi355gp_sparse* s, const double* dF_dmu, const double* dF_dv, double* dtheta_out, double* dZ_out,
                          double* dm_out, double* dchol_out, double* stage_ms);
/* mi355gp_svgp_predict replaces Posterior._raw_predict (posterior.py:220-248) for Posterior(mean = m, cov = S) of svgp.py:121 after
 * a forward call: woodbury_vector = Kmm^-1 m and woodbury_inv_d = Kmm^-1 - Kmm^-1 S_d Kmm^-1 (posterior.py:190-209) stay resident.
 *   mu_out: Mn x L;  var_out (may be NULL): Mn x L clipped at 1e-15, or Mn x Mn x L with full_cov (posterior.py:233-248)
 *   wv_out (M x L) / winv_out (L x M x M) may be NULL: the Woodbury quantities themselves; Mn == 0 fetches only them. */
int mi355gp_svgp_predict(mi355gp_sparse* s, int nparts, const mi355gp_part* parts, const double* Xnew, int64_t Mn, int full_cov,
                         double* mu_out, double* var_out, double* wv_out, double* winv_out);

/* ---- FITC and power EP (PEP) on the sparse context: the sparse methods for a Gaussian likelihood beside VarDTC -------------
 * One PEP.inference (inference/latent_function_inference/pep.py:23-93; Bui, Yan and Turner, arXiv:1605.07066) and the
 * certain-input branch of SparseGP._update_gradients (core/sparse_gp.py:108-119).  alpha = 1 is FITC.inference
 * (fitc.py:21-88, Snelson and Ghahramani: the same arithmetic line for line); alpha -> 0 approaches VarDTC.
 *   sigma*_n = noise + alpha (Kdiag_n - |Lm^-1 k_n|^2), beta* = 1 / sigma* (pep.py:44-46), A = I + Lm^-1 Kuf diag(beta*) Kfu Lm^-T
 *   (:49), b, v, P (:53-59), the log marginal (:64-68), dL_dR (:70-72), dL_dKmm (:75-78), dL_dKnm (:81-84), dL_dKdiag = alpha dL_dR
 *   and dL_dthetaL = sum dL_dR + (1 - alpha) / alpha N / (2 noise) (:86-88).
 * Arguments as mi355gp_vardtc_inference_sum, with ONE noise variance and
 *   alpha in (0, 1];  jitter: the WHOLE term added to Kmm's diagonal, the classes' const_jitter = 1e-6 (pep.py:17, fitc.py:17;
 *   not VarDTC's 1e-8) plus the jitchol ladder's term;
 *   out_scalars[MI355GP_NUM_OUT]: [0] log marginal, [1] dL_dthetaL, [2] sum dL_dR, [3] |b|^2, [4] sum log diag LA, [5] sum log beta*;
 *   dtheta_out (concatenated over the parts), dZ_out (M x D), wv_out (M), dLdR_out (N: dL_dKdiag = alpha times it) and
 *   stage_ms[4] (pass 1, M x M, pass 2, total; HIP events on the launching stream) may be NULL.
 * Accepted parts: those of mi355gp_vardtc_inference_sum.  Refused with an error that names it: alpha outside (0, 1], more than
 * one output column (the reference's v.reshape(-1, 1)), a row-sharded context, a context holding input variances, and a
 * sigma*_n that is not positive -- rounding can do that when the noise is tiny and a point sits on an inducing input; the
 * check runs on the host between the passes (mi355gp_pep_check_sigma) and names the row.  Returns LAPACK-style info > 0 when Kmm
 * or A is not positive definite (the caller raises the jitter).  Every reduction has a fixed order: two calls give the same bytes.
 * The result lies where VarDTC's does: mi355gp_sparse_predict and mi355gp_sparse_fetch (0 dL_dKmm, 1 woodbury_inv = Kmm^-1 - P,
 * 2 Lm, 3 Kmm with THIS call's jitter; 4 and 5 do not exist and are refused) work on it unchanged, and
 * mi355gp_sparse_fetch_dLdKnm serves PEP's rows (pep.py:81-84).  A later VarDTC or SVGP call replaces it, and the reverse. */
int mi355gp_pep_inference(mi355gp_sparse* s, int nparts, const mi355gp_part* parts, const double* Z, int64_t M,
                          double noise_variance, double alpha, double jitter, double* out_scalars, double* dtheta_out,
                          double* dZ_out, double* wv_out, double* dLdR_out, double* stage_ms);
/* The host's check of sigma*_n (pep.py:44) for rows [row0, row0 + n): 0, or -8 and an error naming the first row whose
 * sigma* is not positive (NaN included).  Reads no device state; noise_variance and alpha only word the message. */
int mi355gp_pep_check_sigma(const double* sigma, int64_t n, int64_t row0, double noise_variance, double alpha);

/* ---- psi-statistics of the RBF kernel for Gaussian inputs q(x_n) = N(mu_n, diag S_n) (kern/src/psi_comp/rbf_psi_comp.py) ----
 * Stateless, like mi355gp_kern_K.  lengthscale: D entries if ard, else one.  Z: M x D, mu / S: N x D row-major; every S
 * entry must be positive and finite (checked on the host before any launch); D <= 64.
 * psi1_out (N x M) and psi2_out (M x M, = sum_n w_n psi2n; weights NULL: w_n = 1) may each be NULL.  The sum over n is
 * combined in a fixed order: two calls give the same bits. */
int mi355gp_rbf_psi(int device, double variance, const double* lengthscale, int ard, const double* Z, int64_t M,
                    const double* mu, const double* S, int64_t N, int D, const double* weights, double* psi1_out,
                    double* psi2_out);
/* The five outputs of psiDerivativecomputations (rbf_psi_comp.py:70-133) from dL_dpsi0 (N), dL_dpsi1 (N x M) and dL_dpsi2
 * (M x M, symmetrised inside), each of which may be NULL: dvar_out (1), dl_out (D if ard, else 1), dZ_out (M x D),
 * dmu_out and dS_out (N x D).  psi2n is recomputed tile by tile; no N x M x M array exists. */
int mi355gp_rbf_psi_grad(int device, double variance, const double* lengthscale, int ard, const double* Z, int64_t M,
                         const double* mu, const double* S, int64_t N, int D, const double* weights, const double* dL_dpsi0,
                         const double* dL_dpsi1, const double* dL_dpsi2, double* dvar_out, double* dl_out, double* dZ_out,
                         double* dmu_out, double* dS_out);

#ifdef __cplusplus
}
#endif
#endif
