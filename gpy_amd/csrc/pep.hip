// pep.hip -- FITC and power-EP (PEP) sparse inference for a Gaussian likelihood on the sparse context.
// Replaces, for certain inputs, one output column, one noise variance and a zero mean function,
//   PEP.inference                    GPy/inference/latent_function_inference/pep.py:23-93
//   FITC.inference                   GPy/inference/latent_function_inference/fitc.py:21-88   (pep.py with alpha = 1, line for line)
//   SparseGP._update_gradients       GPy/core/sparse_gp.py:108-119  (certain-input branch)
// One evaluation is two passes over the context's row chunks; no N x M array outlives a chunk.  With Lm = chol(Kmm),
// Xm = Lm^-1 and the whitened rows w_n = Xm k_n (W = Kfu Xm^T):
//   pass 1   Kmm (jitter 1e-6, pep.py:19,36-37), Lm, Xm first: beta* needs them.  Per chunk: Kfu, W (MFMA), one row kernel
//            (q_n = |w_n|^2, sigma*_n, beta*_n, log beta*_n, pep.py:44-46; the row times sqrt(beta*_n)), the split-K Gram
//            A - I += sum_n beta*_n w_n w_n^T (pep.py:49-51) and W^T (beta* y) (:53).
//   M x M    LA = chol(A), b = LA^-1 W^T (beta* y), w = LA^-T b, v = Xm^T w (pep.py:52-57), A^-1, G = A^-1 Xm,
//            woodbury_inv = Kmm^-1 - P = Xm^T (I - A^-1) Xm (:58-59,87-88)
//   pass 2   Kfu and W again (a single chunk: still resident), C1 = W G (row n: (P k_n)^T), C2 = W Xm (row n: (Kmm^-1 k_n)^T) --
//            2.5 N M^2 products with W's half -- one row kernel (dL_dR_n, pep.py:70-72, and the row of dL_dKnm, :81-84, in place),
//            the kernels' reductions of those rows, and the signed weighted Gram sum_n dL_dR_n a_n a_n^T (:77-79)
// Every reduction over rows, chunks and splits has a fixed order (no floating-point atomics): two calls give the same bytes.
// Padding convention as in svgp.hip: Lm, Xm, A and A^-1 carry the identity in the padding block, the columns >= M of every
// chunk buffer and the entries >= M of every vector are zero.
#include <cmath>
#include <vector>

#include "sparse_ctx.h"

struct PepState {
    long mp = 0, chunk = 0, n = 0;
    double alpha = 1.0, jitter = 1e-6;
    DevBuf C1, C2, S, rowStat, red;        // chunk x mp (twice), mp x mp, [sigma* | log beta*] (2 n), 2
};

void pep_release(mi355gp_sparse* s) {
    delete s->pep;
    s->pep = nullptr;
    s->pep_result = false;
}

static int pep_state(mi355gp_sparse* s) {
    PepState* pp = s->pep;
    if (pp && pp->mp == s->mp && pp->chunk == s->chunk && pp->n == s->n) return 0;
    pep_release(s);
    pp = new PepState();
    s->pep = pp;
    pp->mp = s->mp;
    pp->chunk = s->chunk;
    pp->n = s->n;
    HIP_CHECK(pp->C1.alloc((size_t)s->chunk * s->mp));
    HIP_CHECK(pp->C2.alloc((size_t)s->chunk * s->mp));
    HIP_CHECK(pp->S.alloc((size_t)s->mp * s->mp));
    HIP_CHECK(pp->rowStat.alloc((size_t)2 * s->n));
    HIP_CHECK(pp->red.alloc(2));
    return 0;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------
// sum of the split-K partial Grams (lower tiles) mirrored onto the upper triangle, in the order of the splits
__global__ void k_pep_sym_splits(const double* __restrict__ part, long mp, int nsplit, double* __restrict__ out) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= mp) return;
    const long a = (i >= j) ? i : j, b = (i >= j) ? j : i;
    double v = 0.0;
    for (int k = 0; k < nsplit; ++k) v += part[(long)k * mp * mp + a * mp + b];
    out[i * mp + j] = v;
}

// Pass 1, one wave per chunk row, W read once (pep.py:44-46,49):
//   q = |w_n|^2, sigma* = s2 + alpha (Knn - q), beta* = 1 / sigma*;  Out[n][:] = sqrt(beta*) w_n;  V[n] = beta* y_n
// Knn = knn for every row, or kd[n] where a per-point diagonal is given.
// A sigma* that is not positive leaves beta* = 0 behind (the row drops out of every sum) and sigma* itself for the host's
// check, which ends the call: nothing downstream sees a NaN.  Rows [rows, rows_pad) of Out are zeroed for the Gram.
__global__ __launch_bounds__(256) void k_pep_rows1(const double* __restrict__ W, long ld, long rows, long rows_pad,
                                                   const double* __restrict__ y, double s2, double alpha, double knn,
                                                   const double* __restrict__ kd, double* __restrict__ sigma, double* __restrict__ logb,
                                                   double* __restrict__ beta, double* __restrict__ V,
                                                   double* __restrict__ Out) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= rows_pad) return;
    double* o = Out + i * ld;
    if (i >= rows) {
        for (long j = lane; j < ld; j += 64) o[j] = 0.0;
        return;
    }
    const double* w = W + i * ld;
    double q = 0.0;
    for (long j = lane; j < ld; j += 64) q = fma(w[j], w[j], q);
    for (int off = 32; off > 0; off >>= 1) q += __shfl_xor(q, off);
    const double sg = s2 + alpha * ((kd ? kd[i] : knn) - q);
    const bool ok = sg > 0.0;
    const double b = ok ? 1.0 / sg : 0.0, sb = sqrt(b);
    for (long j = lane; j < ld; j += 64) o[j] = sb * w[j];
    if (lane == 0) {
        sigma[i] = sg;
        logb[i] = ok ? -log(sg) : 0.0;
        beta[i] = b;
        V[i] = b * y[i];
    }
}

// Pass 2, one wave per chunk row, the rows of Kfu, C1 = (P k_n)^T and C2 = (Kmm^-1 k_n)^T read once (the second sweep hits
// the cache):  p = k_n^T P k_n, t = k_n^T v,
//   dL_dR_n = beta*^2 (p - (1 + c) / beta* + y^2 - 2 y t + t^2) / 2                                     (pep.py:70-72)
//   C1[n][:] = beta* ((y - t) v^T - (P k_n)^T) - 2 alpha dL_dR_n (Kmm^-1 k_n)^T = dL_dKnm[n][:]          (pep.py:81-84)
//   U[n][:]  = dL_dR_n (Kmm^-1 k_n)^T                     (the signed rows of the weighted Gram, pep.py:77-79)
// Rows [rows, rows_pad): C1 is zero already (Kfu's rows are), U is zeroed.
__global__ __launch_bounds__(256) void k_pep_rows2(const double* __restrict__ Kfu, double* __restrict__ C1,
                                                   const double* __restrict__ C2, double* __restrict__ U, long ld, long rows,
                                                   long rows_pad, long m, const double* __restrict__ y,
                                                   const double* __restrict__ beta, const double* __restrict__ v, double alpha,
                                                   double c, double* __restrict__ dR) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= rows_pad) return;
    double* u = U + i * ld;
    if (i >= rows) {
        for (long j = lane; j < ld; j += 64) u[j] = 0.0;
        return;
    }
    const double* k = Kfu + i * ld;
    double* c1 = C1 + i * ld;
    const double* c2 = C2 + i * ld;
    double p = 0.0, t = 0.0;
    for (long j = lane; j < m; j += 64) {
        const double kj = k[j];
        p = fma(kj, c1[j], p);
        t = fma(kj, v[j], t);
    }
    for (int off = 32; off > 0; off >>= 1) {
        p += __shfl_xor(p, off);
        t += __shfl_xor(t, off);
    }
    const double b = beta[i], yn = y[i];
    // (beta* = 0 marks a row whose sigma* was not positive: the call is ending with an error, the row contributes zeros)
    const double r = (b > 0.0) ? 0.5 * b * b * (((p - (1.0 + c) / b) + yn * yn) - 2.0 * yn * t + t * t) : 0.0;
    const double f = b * (yn - t), g = 2.0 * alpha * r;
    for (long j = lane; j < ld; j += 64) {
        const bool in = j < m;
        const double a = c2[j];
        c1[j] = in ? (f * v[j] - b * c1[j]) - g * a : 0.0;
        u[j] = in ? r * a : 0.0;
    }
    if (lane == 0) dR[i] = r;
}

// S[i][j] = G[i][j] * S[i][j] for i < rows, j < m, 0 in the padding: this chunk's rows of dL_dKnm times the other factors'
// covariance (prod.py:86-99), the weights one factor of a product sees
__global__ void k_pep_weights_times(const double* __restrict__ G, double* __restrict__ S, long ld, long rows, long rows_pad, long m) {
    const long j = (long)blockIdx.y * blockDim.x + threadIdx.x, i = blockIdx.x;
    if (j >= ld || i >= rows_pad) return;
    S[i * ld + j] = (i < rows && j < m) ? G[i * ld + j] * S[i * ld + j] : 0.0;
}

// dL_dKmm = (Kmm^-1 - v v^T - P) / 2 + alpha Kmm^-1 Kuf diag(dL_dR) Kfu Kmm^-1 (pep.py:75-79) over the leading m x m, 0 in the
// padding; Winv = Kmm^-1 - P, Sg = sum_n dL_dR_n a_n a_n^T (its two halves averaged: the GEMM rounds them apart)
__global__ void k_pep_dLdKmm(const double* __restrict__ Winv, const double* __restrict__ v, const double* __restrict__ Sg,
                             double alpha, long mp, long m, double* __restrict__ out) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= mp) return;
    double r = 0.0;
    if (i < m && j < m) r = 0.5 * (Winv[i * mp + j] - v[i] * v[j]) + alpha * (0.5 * (Sg[i * mp + j] + Sg[j * mp + i]));
    out[i * mp + j] = r;
}

// out[0] = sum_i log LA_ii, out[1] = |b|^2 over i < m, one block, a fixed order (pep.py:65,67)
__global__ __launch_bounds__(256) void k_pep_mm_scalars(const double* __restrict__ LA, const double* __restrict__ b, long mp, long m,
                                                        double* __restrict__ out) {
    __shared__ double red[2][256];
    const int t = threadIdx.x;
    double s0 = 0.0, s1 = 0.0;
    for (long i = t; i < m; i += 256) {
        s0 += log(LA[i * mp + i]);
        s1 = fma(b[i], b[i], s1);
    }
    red[0][t] = s0;
    red[1][t] = s1;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (t < k) {
            red[0][t] += red[0][t + k];
            red[1][t] += red[1][t + k];
        }
        __syncthreads();
    }
    if (t < 2) out[t] = red[t][0];
}

// ---- phases ----------------------------------------------------------------------------------------------------------------
// rows a chunk buffer is zeroed / scaled to: what the tile GEMMs (128) and the split-K Gram (16 per split) read
static long pep_rows_pad(const mi355gp_sparse* s, long rc) {
    const long a = round_up(rc, NB), b = round_up(rc, 16L * s->splitk);
    return a > b ? a : b;
}

// Kfu of rows [r0, r0 + rc) (zero in the padding) into s->Kfu and the whitened rows W = Kfu Xm^T into s->T
static int pep_chunk_W(mi355gp_sparse* s, long r0, long rc) {
    const long mp = s->mp, rcp = round_up(rc, NB);
    if (int rc2 = sparse_cross_rows(s, r0, rc, 0, pep_rows_pad(s, rc), nullptr)) return rc2;
    launch_gemm(s->st, 0, 0, rcp, mp, mp, s->Kfu, mp, s->Xm, mp, s->T, mp, 1.0, 0.0);
    return 0;
}

// The pass-2 products and row kernel of one chunk whose Kfu / W are in place: leaves the chunk's rows of dL_dKnm in C1, the
// signed rows in s->T (W is spent) and dL_dR in s->dRowR
static void pep_chunk_rows2(mi355gp_sparse* s, long r0, long rc) {
    PepState* pp = s->pep;
    hipStream_t st = s->st;
    const long mp = s->mp, rcp = round_up(rc, NB);
    launch_gemm(st, 0, 1, rcp, mp, mp, s->T, mp, s->Q2, mp, pp->C1, mp, 1.0, 0.0);        // W (A^-1 Xm): rows (P k_n)^T
    launch_gemm(st, 0, 1, rcp, mp, mp, s->T, mp, s->Xm, mp, pp->C2, mp, 1.0, 0.0);        // W Xm: rows (Kmm^-1 k_n)^T
    hipLaunchKernelGGL(k_pep_rows2, dim3((unsigned)((rcp + 3) / 4)), dim3(256), 0, st, s->Kfu, pp->C1, pp->C2, s->T, mp, rc, rcp, s->m,
                       s->dY + r0, s->dBeta + r0, s->vvec, pp->alpha, (1.0 - pp->alpha) / pp->alpha, s->dRowR + r0);
}

extern "C" {

// The host's check of sigma*_n = s2 + alpha (Knn_n - q_n) (pep.py:44; fitc.py:41) for rows [row0, row0 + n): in exact
// arithmetic it is at least s2 > 0, rounding can take it below zero when the noise is tiny and a point sits on an inducing
// input.  0, or -8 with an error that names the first such row (a NaN counts).  Reads no device state.
int mi355gp_pep_check_sigma(const double* sigma, int64_t n, int64_t row0, double noise_variance, double alpha) {
    ARG_CHECK(sigma && n >= 0, "mi355gp_pep_check_sigma: bad arguments");
    for (int64_t i = 0; i < n; ++i)
        if (!(sigma[i] > 0.0)) {
            mi355gp_set_error("mi355gp_pep_inference: sigma* of row %lld is %g, not positive (noise variance %g, alpha %g: "
                              "noise + alpha (Kdiag - |Lm^-1 k_n|^2), pep.py:44); raise the noise variance or the jitter",
                              (long long)(row0 + i), sigma[i], noise_variance, alpha);
            return -8;
        }
    return 0;
}

// One PEP.inference (pep.py:23-93; alpha = 1: FITC.inference, fitc.py:21-88) and the certain-input branch of
// SparseGP._update_gradients (sparse_gp.py:108-119); see mi355gp.h.
int mi355gp_pep_inference(mi355gp_sparse* s, int nparts, const mi355gp_part* parts, const double* Z, int64_t M,
                          double noise_variance, double alpha, double jitter, double* out_scalars, double* dtheta_out,
                          double* dZ_out, double* wv_out, double* dLdR_out, double* stage_ms) {
    const char* where = "mi355gp_pep_inference";
    if (!s || s->n <= 0) PART_FAIL("%s: set_data first", where);
    ARG_CHECK(parts && Z && M > 0 && out_scalars, "mi355gp_pep_inference: bad arguments");
    if (!(alpha > 0.0 && alpha <= 1.0)) PART_FAIL("%s: alpha = %g is outside (0, 1] (1 is FITC; VarDTC is the limit alpha -> 0)", where, alpha);
    if (s->Dy != 1)
        PART_FAIL("%s: %d output columns; PEP / FITC take one (the reference's v.reshape(-1, 1), pep.py:57, fitc.py:54)", where, s->Dy);
    if (sharded(s)) PART_FAIL("%s: a row-sharded context is not supported by PEP / FITC", where);
    if (s->dSvar) PART_FAIL("%s: the context holds input variances; PEP / FITC take certain inputs (mi355gp_sparse_set_data discards them)", where);
    if (!(noise_variance > 0.0) || !(jitter >= 0.0)) PART_FAIL("%s: noise variance %g, jitter %g: the first must be positive, the second not negative", where, noise_variance, jitter);
    EngineShared gate(s->device);
    if (int rc = sparse_open(s, nparts, parts, M)) return rc;
    if (int rc = pep_state(s)) return rc;
    PepState* pp = s->pep;
    pp->alpha = alpha;
    pp->jitter = jitter;
    hipStream_t st = s->st;
    const long n = s->n, m = s->m, mp = s->mp, chunk = s->chunk;
    const double c = (1.0 - alpha) / alpha;
    const bool one_chunk = (n <= chunk);
    s->mfma_prof.on = false;
    s->beta_scalar = 0.0;
    if (int rc = sparse_start(s, Z, nullptr, 0)) return rc;
    // Knn = kern.Kdiag(X) (pep.py:38): a constant, or by point in s->dKd
    const double knn = s->diag_pt ? 0.0 : expression_kdiag(s->parts, s->terms);
    if (s->diag_pt)
        if (int rc = sparse_kdiag_data(s, nullptr, nullptr)) return rc;
    double* sigma = pp->rowStat;
    double* logb = pp->rowStat + n;
    // ---- pass 1 ------------------------------------------------------------------------------------------------------------------
    // Kmm = K(Z) + jitter I (pep.py:36-37), Lm = jitchol(Kmm) (:40), Xm = Lm^-1
    auto rebuild_kmm = [&]() { build_kmm(s, s->Lm, s->T1, jitter, /*lower_only=*/1, st); };
    rebuild_kmm();
    if (int rc = potrf_checked(st, s->Lm, s->Xm, s->Tm, nullptr, mp, &s->ws, &s->h_info[0], rebuild_kmm)) return rc;
    HIP_CHECK(hipMemsetAsync(s->psi1Y, 0, sizeof(double) * mp, st));
    int nch = 0;
    for (long r0 = 0; r0 < n; r0 += chunk, ++nch) {
        const long rc = (n - r0 < chunk) ? (n - r0) : chunk;
        const long rz = pep_rows_pad(s, rc);
        if (int rc2 = pep_chunk_W(s, r0, rc)) return rc2;
        // LiUT = Lm^-1 Kuf (pep.py:42), sigma_star, beta_star (:44-45), the rows scaled for A (:49-50)
        hipLaunchKernelGGL(k_pep_rows1, dim3((unsigned)((rz + 3) / 4)), dim3(256), 0, st, s->T, mp, rc, rz, s->dY + r0, noise_variance,
                           alpha, knn, s->diag_pt ? s->dKd + r0 : nullptr, sigma + r0, logb + r0, s->dBeta + r0, s->dV + r0, pp->C1);
        launch_gram_splitk(st, pp->C1, mp, round_up(rc, 16L * s->splitk), mp, s->splitk, nch > 0, s->psi2part);
        // URiy = Kuf (beta* y) in the whitened basis (pep.py:53)
        const int ns = launch_colreduce_multi(st, s->T, mp, rc, mp, s->dV + r0, 1, 1, 1, 0, s->colPart);
        launch_sum_splits(st, s->colPart, mp, ns, 1, s->psi1Y);
    }
    hipLaunchKernelGGL(k_pep_sym_splits, grid2d(mp, mp), dim3(256), 0, st, s->psi2part, mp, s->splitk, s->Amat);      // A - I
    HIP_CHECK(hipEventRecord(s->ev[1], st));
    // the host's look at pass 1: Kmm's factorisation (info > 0: the caller adds jitter) and every sigma*
    std::vector<double> hstat((size_t)2 * n);
    HIP_CHECK(hipMemcpyAsync(hstat.data(), pp->rowStat, sizeof(double) * 2 * n, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    if (s->h_info[0] > 0) return s->h_info[0] > m ? (int)m : s->h_info[0];
    if (int rc = mi355gp_pep_check_sigma(hstat.data(), n, 0, noise_variance, alpha)) return rc;
    // ---- M x M -------------------------------------------------------------------------------------------------------------------
    // A = I + LiUT diag(beta*) LiUT^T, LA = jitchol(A) (pep.py:49-52); XB = LA^-1, Bi = A^-1 (lower tiles)
    auto build_A = [&]() { launch_mm_axpby(st, s->Amat, 1.0, nullptr, 0.0, 1.0, mp, s->LB); };
    build_A();
    if (int rc = potrf_checked(st, s->LB, s->XB, s->Tm, s->Bi, mp, &s->ws, &s->h_info[1], build_A)) return rc;
    // b = LA^-1 Lm^-1 URiy (pep.py:54-55), w = LA^-T b, v = Lm^-T w = woodbury_vector (:56-57,91)
    launch_trmv_lower(st, s->XB, mp, mp, s->psi1Y, 1, s->cvec);
    launch_trmv_lower_T(st, s->XB, mp, mp, s->cvec, 1, s->wvec, s->trmvPart);
    launch_trmv_lower_T(st, s->Xm, mp, mp, s->wvec, 1, s->vvec, s->trmvPart);
    // P = Lm^-T A^-1 Lm^-1 (pep.py:58-59) is never formed: pass 2 reads G = A^-1 Xm (P k_n = Xm^T A^-1 w_n), and
    // woodbury_inv = Kmm^-1 - P = Xm^T (I - A^-1) Xm (:87-88) is built as mi355gp_sparse_fetch builds VarDTC's
    launch_mm_sym(st, s->Bi, mp, s->E);
    launch_gemm(st, 0, 1, mp, mp, mp, s->E, mp, s->Xm, mp, s->Q2, mp, 1.0, 0.0);
    launch_mm_axpby(st, s->E, -1.0, nullptr, 0.0, 1.0, mp, s->E);
    launch_gemm(st, 1, 1, mp, mp, mp, s->Xm, mp, s->E, mp, s->T1, mp, 1.0, 0.0);
    launch_gemm(st, 0, 1, mp, mp, mp, s->T1, mp, s->Xm, mp, s->Winv, mp, 1.0, 0.0);
    hipLaunchKernelGGL(k_pep_mm_scalars, dim3(1), dim3(256), 0, st, s->LB, s->cvec, mp, m, pp->red);
    HIP_CHECK(hipEventRecord(s->ev[2], st));
    // ---- pass 2 ------------------------------------------------------------------------------------------------------------------
    if (int rc = sparse_rows_gradients_reset(s)) return rc;
    nch = 0;
    for (long r0 = 0; r0 < n; r0 += chunk, ++nch) {
        const long rc = (n - r0 < chunk) ? (n - r0) : chunk;
        const long rcp = round_up(rc, NB);
        if (!one_chunk)                                       // a single chunk: Kfu and W are still resident from pass 1
            if (int rc2 = pep_chunk_W(s, r0, rc)) return rc2;
        pep_chunk_rows2(s, r0, rc);
        // Kmm^-1 Kuf diag(dL_dR) Kfu Kmm^-1 (pep.py:77-79): signed weights, so the rows are weighted once, not by square roots
        launch_gemm(st, 1, 1, mp, mp, rcp, pp->C2, mp, s->T, mp, pp->S, mp, 1.0, nch > 0 ? 1.0 : 0.0);
        // update_gradients_full(dL_dKnm, X, Z) and gradients_X(dL_dKnm^T, Z, X) (sparse_gp.py:111-118): no rank term, the rows
        // are complete; the Kfu buffer is scratch from here on
        const RankTerm none{nullptr, nullptr, 0, 0.0, 1.0, nullptr};
        sparse_rows_gradients(s, rc, pp->C1, s->Kfu, none, [&]() {
            hipLaunchKernelGGL(k_pep_weights_times, dim3((unsigned)rcp, (unsigned)((mp + 255) / 256)), dim3(256), 0, st, pp->C1, s->Kfu,
                               mp, rc, rcp, m);
        });
    }
    hipLaunchKernelGGL(k_pep_dLdKmm, grid2d(mp, mp), dim3(256), 0, st, s->Winv, s->vvec, pp->S, alpha, mp, m, s->dLdKmm);
    sparse_kmm_gradients(s);
    // a per-point diagonal: update_gradients_diag's sums against w_n = dL_dR_n (times alpha on the host, pep.py:85)
    std::vector<double> dsums;
    if (s->diag_pt)
        if (int rc = sparse_kdiag(s, s->dX, n, s->dRowR, nullptr, &dsums)) return rc;
    HIP_CHECK(hipEventRecord(s->ev[3], st));
    // ---- small results to the host -----------------------------------------------------------------------------------------------
    KernGrads kg;
    std::vector<double> hdR((size_t)n);
    double red[2] = {0.0, 0.0};
    if (int rc = sparse_fetch_gradients(s, true, &kg)) return rc;
    HIP_CHECK(hipMemcpyAsync(hdR.data(), s->dRowR, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(red, pp->red, sizeof(red), hipMemcpyDeviceToHost, st));
    if (wv_out) HIP_CHECK(hipMemcpyAsync(wv_out, s->vvec, sizeof(double) * m, hipMemcpyDeviceToHost, st));
    if (int rc = sparse_finish(s, 3, stage_ms)) return rc;      // (info > 0: A not positive definite, the caller adds jitter)
    // the sums over rows, in row order
    double sum_logb = 0.0, sum_byy = 0.0, sum_dR = 0.0;
    for (long i = 0; i < n; ++i) {
        sum_logb += hstat[(size_t)(n + i)];
        sum_byy += s->rowYY[(size_t)i] / hstat[(size_t)i];
        sum_dR += hdR[(size_t)i];
    }
    // log_marginal (pep.py:64-68) and dL_dthetaL (:86)
    const double nd = (double)n;
    for (int i = 0; i < MI355GP_NUM_OUT; ++i) out_scalars[i] = 0.0;
    out_scalars[0] = -0.5 * nd * log(2.0 * M_PI) - red[0] + 0.5 * (1.0 + c) * sum_logb - 0.5 * sum_byy + 0.5 * red[1] +
                     0.5 * c * nd * log(noise_variance);
    out_scalars[1] = sum_dR + 0.5 * c * nd / noise_variance;
    out_scalars[2] = sum_dR;
    out_scalars[3] = red[1];
    out_scalars[4] = red[0];
    out_scalars[5] = sum_logb;
    if (dLdR_out)
        for (long i = 0; i < n; ++i) dLdR_out[i] = hdR[(size_t)i];
    // update_gradients_diag(dL_dKdiag = alpha dL_dR) (pep.py:85, sparse_gp.py:110)
    if (s->diag_pt) sparse_diag_dtheta(s, dsums, alpha, &kg.ddiag);
    sparse_assemble_gradients(s, kg, alpha * sum_dR, dtheta_out, dZ_out);
    s->have_result = s->winv_ok = true;
    s->uncertain_result = false;
    s->pep_result = true;
    s->kmm_jitter = jitter;
    return 0;
}

}  // extern "C"

// Rows [row0, row0 + nrows) of dL_dKnm (pep.py:81-84) of the last PEP call, formed again as pass 2 forms them (the caller,
// mi355gp_sparse_fetch_dLdKnm, holds the gate and has checked the range)
int pep_fetch_dLdKnm(mi355gp_sparse* s, long row0, long nrows, double* out) {
    PepState* pp = s->pep;
    ARG_CHECK(pp && s->pep_result, "mi355gp_sparse_fetch_dLdKnm: no PEP result on this context");
    hipStream_t st = s->st;
    if (int rc = pep_chunk_W(s, row0, nrows)) return rc;
    pep_chunk_rows2(s, row0, nrows);
    HIP_CHECK(hipMemcpy2DAsync(out, sizeof(double) * s->m, pp->C1, sizeof(double) * s->mp, sizeof(double) * s->m, nrows,
                               hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    return 0;
}
