// svgp.hip -- stochastic variational GP (SVGP) inference on the sparse context: minibatches and non-Gaussian likelihoods.
// Replaces, for certain inputs and a zero mean function,
//   SVGP.inference                   GPy/inference/latent_function_inference/svgp.py:10-121
//   SVGP.parameters_changed          GPy/core/svgp.py:54-71  (kernel and inducing-input gradients from dL_dKmm / dL_dKmn / dL_dKdiag)
//   Posterior._raw_predict           GPy/inference/latent_function_inference/posterior.py:198-262 (the mean / cov form, :79-107)
// as a two-call session around the likelihood's quadrature, which stays on the host (variational_expectations: O(N L)):
//   forward   M x M: Kmm (no 1e-8 term, svgp.py:37), Lm, Kmm^-1, S_d = L_d L_d^T, S_d^-1, Kmm^-1 m, the KL term
//             rows : per chunk Kfu, A^T = Kfu Kmm^-1 (MFMA), A^T L_d (MFMA), one row-reduction kernel -> mu, v
//   backward  rows : per chunk A dF_dmu, the weighted Grams A diag(dF_dv_d) A^T (MFMA, signed weights), this chunk's rows of
//                    dL_dKmn (MFMA) and their theta sums / H^T [X~ | 1] column sums through the sparse path's gradient kernels
//             M x M: dL_dKmm, dL_dm, dL_dchol, the Kmm part of the theta and Z gradients
// All reductions run in a fixed order (no floating-point atomics): two calls on the same inputs give the same bytes.
// Padding convention (M padded to mp = a multiple of 128): Kmm, Kmm^-1, L_d, S_d and S_d^-1 carry the identity in the padding
// block, m and the columns >= M of every chunk buffer are zero; products of such matrices keep the two blocks apart.
#include <cmath>
#include <cstring>
#include <vector>

#include "sparse_ctx.h"

#define SVGP_LMAX 16

struct SvgpState {
    int L = 0;
    long mp = 0, chunk = 0, n = 0;
    bool fwd_ok = false, winv_ok = false;
    DevBuf Kmmi, Ld, Sd, Si, AdvA, Tq, Wd, U, qm, Kmmim, Admu, colPart, rowPart, red, dMu, dVv, dFmu, dFv, dQ;
    int h_info[SVGP_LMAX] = {};   // LAPACK-style info of the L factorisations of S_d (targets of async copies)
};

void svgp_release(mi355gp_sparse* s) {
    delete s->svgp;
    s->svgp = nullptr;
    s->svgp_result = false;
}

// ---- kernels (the elementwise M x M ones are sparse.hip's: launch_mm_sym, launch_mm_axpby) ---------------------------
// out = sum_d A_d in the order d = 0 .. L-1
__global__ void k_svgp_sum_lat(const double* __restrict__ A, int L, long mp, double* __restrict__ out) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= mp) return;
    double v = 0.0;
    for (int d = 0; d < L; ++d) v += A[(long)d * mp * mp + i * mp + j];
    out[i * mp + j] = v;
}
// one wave per row: out[i][l] = sum_j A[i][j] x[j][l]   (A mp x mp, x mp x L zero in the padding)
__global__ __launch_bounds__(256) void k_svgp_matvec(const double* __restrict__ A, long mp, const double* __restrict__ x, int L,
                                                     double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= mp) return;
    const double* ar = A + i * mp;
    for (int l = 0; l < L; ++l) {
        double a = 0.0;
        for (long j = lane; j < mp; j += 64) a = fma(ar[j], x[j * L + l], a);
        for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off);
        if (lane == 0) out[i * L + l] = a;
    }
}
// the KL term's sums (svgp.py:55), one block per row i < m: rowpart[i] = {sum_j Kmmi_ij S_d,ij (d < L), m_id (Kmmi m)_id (d < L),
// log Lm_ii}; launch_reduce_partials adds the rows in a fixed order
__global__ __launch_bounds__(256) void k_svgp_kl_rows(const double* __restrict__ Kmmi, const double* __restrict__ Sd,
                                                      const double* __restrict__ Lm, const double* __restrict__ qm,
                                                      const double* __restrict__ Kmmim, int L, long mp, long m,
                                                      double* __restrict__ rowpart) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    const long i = blockIdx.x;
    const int stride = 2 * L + 1;
    for (int d = 0; d < L; ++d) {
        const double* S = Sd + (long)d * mp * mp;
        double a = 0.0;
        for (long j = t; j < m; j += 256) a = fma(Kmmi[i * mp + j], S[i * mp + j], a);
        red[t] = a;
        __syncthreads();
        for (int k = 128; k > 0; k >>= 1) {
            if (t < k) red[t] += red[t + k];
            __syncthreads();
        }
        if (t == 0) rowpart[i * stride + d] = red[0];
        __syncthreads();
    }
    if (t == 0) {
        for (int d = 0; d < L; ++d) rowpart[i * stride + L + d] = qm[i * L + d] * Kmmim[i * L + d];
        rowpart[i * stride + 2 * L] = log(Lm[i * mp + i]);
    }
}
// The three row reductions of svgp.py:45-51 in one pass, one wave per chunk row, 16-byte loads (ld % 2 == 0, the padding
// columns of At / U / Kfu and the padding rows of qm are zero):
//   first latent (d == 0):  mu[i][:] = sum_j At[i][j] m[j][:],  q[i] = sum_j At[i][j] Kfu[i][j]  (kept for the other latents)
//   every latent:           v[i][d] = sum_j U[i][j]^2 + kdiag - q[i],   U = A^T L_d   (kdiag: kd[i] where a vector is given)
__global__ __launch_bounds__(256) void k_svgp_rowstats(const double* __restrict__ At, const double* __restrict__ Kfu,
                                                       const double* __restrict__ U, long ld, long rows,
                                                       const double* __restrict__ qm, int L, int d, double kdiag,
                                                       const double* __restrict__ kd, double* __restrict__ mu, double* __restrict__ q, double* __restrict__ v) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= rows) return;
    const double2* ur = reinterpret_cast<const double2*>(U + i * ld);
    double ss = 0.0;
    for (long j = lane; j < ld / 2; j += 64) {
        const double2 u = ur[j];
        ss = fma(u.x, u.x, ss);
        ss = fma(u.y, u.y, ss);
    }
    for (int off = 32; off > 0; off >>= 1) ss += __shfl_down(ss, off);
    double qq = 0.0;
    if (d == 0) {
        const double2* ar = reinterpret_cast<const double2*>(At + i * ld);
        const double2* kr = reinterpret_cast<const double2*>(Kfu + i * ld);
        double acc[SVGP_LMAX];
#pragma unroll
        for (int l = 0; l < SVGP_LMAX; ++l) acc[l] = 0.0;
        for (long j = lane; j < ld / 2; j += 64) {
            const double2 a = ar[j], k = kr[j];
            qq = fma(a.x, k.x, qq);
            qq = fma(a.y, k.y, qq);
            const double* m0 = qm + 2 * j * L;
#pragma unroll
            for (int l = 0; l < SVGP_LMAX; ++l)
                if (l < L) acc[l] = fma(a.y, m0[L + l], fma(a.x, m0[l], acc[l]));
        }
        for (int off = 32; off > 0; off >>= 1) qq += __shfl_down(qq, off);
#pragma unroll
        for (int l = 0; l < SVGP_LMAX; ++l)
            if (l < L) {
                double a = acc[l];
                for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off);
                if (lane == 0) mu[i * L + l] = a;
            }
        if (lane == 0) q[i] = qq;
    } else if (lane == 0) {
        qq = q[i];
    }
    if (lane == 0) v[i * L + d] = (ss + (kd ? kd[i] : kdiag)) - qq;
}
// U[i][j] = w[i][d] * At[i][j] for i < rows, 0 for rows <= i < rows_pad   (Adv_d of svgp.py:85, N x M; the weights are signed)
__global__ void k_svgp_weight_rows(const double* __restrict__ At, long ld, long rows, long rows_pad, const double* __restrict__ w,
                                   int L, int d, double* __restrict__ U) {
    const long j = (long)blockIdx.y * blockDim.x + threadIdx.x, i = blockIdx.x;
    if (j >= ld || i >= rows_pad) return;
    U[i * ld + j] = (i < rows) ? w[i * L + d] * At[i * ld + j] : 0.0;
}
// W[i][j] = (G[i][j] + sum_d Y[i][d] V[j][d]) * W[i][j] for i < rows, j < m; 0 in the padding: this chunk's rows of dL_dKmn times
// the other factors' covariance (prod.py:86-99), the weights one factor of a product sees
__global__ void k_svgp_weights_times(const double* __restrict__ G, double* __restrict__ W, long ld, long rows, long rows_pad,
                                     long m, const double* __restrict__ Y, const double* __restrict__ V, int L) {
    const long j = (long)blockIdx.y * blockDim.x + threadIdx.x, i = blockIdx.x;
    if (j >= ld || i >= rows_pad) return;
    double g = 0.0;
    if (i < rows && j < m) {
        double yv = 0.0;
        for (int d = 0; d < L; ++d) yv = fma(Y[i * L + d], V[j * L + d], yv);
        g = (G[i * ld + j] + yv) * W[i * ld + j];
    }
    W[i * ld + j] = g;
}
// dL_dKmm = dF_dKmm - dKL_dKmm (svgp.py:60,89-91,112) over the leading m x m, 0 in the padding:
//   F = -Admu Kmmim^T + sum_d AdvA_d - tmp - tmp^T,  dF_dKmm = (F + F^T) / 2,  tmp = (sum_d AdvA_d S_d) Kmmi
//   dKL_dKmm = L Kmmi / 2 - Kmmi (sum_d S_d) Kmmi / 2 - Kmmim Kmmim^T / 2
__global__ void k_svgp_dLdKmm(const double* __restrict__ sumA, const double* __restrict__ tmp, const double* __restrict__ Kmmi,
                              const double* __restrict__ KSK, const double* __restrict__ Admu, const double* __restrict__ Kmmim,
                              int L, long mp, long m, double* __restrict__ out) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= mp) return;
    double v = 0.0;
    if (i < m && j < m) {
        double am_ij = 0.0, am_ji = 0.0, kk = 0.0;
        for (int d = 0; d < L; ++d) {
            am_ij = fma(Admu[i * L + d], Kmmim[j * L + d], am_ij);
            am_ji = fma(Admu[j * L + d], Kmmim[i * L + d], am_ji);
            kk = fma(Kmmim[i * L + d], Kmmim[j * L + d], kk);
        }
        const double t2 = tmp[i * mp + j] + tmp[j * mp + i];
        const double f_ij = ((sumA[i * mp + j] - am_ij) - t2), f_ji = ((sumA[j * mp + i] - am_ji) - t2);
        const double dkl = 0.5 * (double)L * Kmmi[i * mp + j] - 0.5 * KSK[i * mp + j] - 0.5 * kk;
        v = 0.5 * (f_ij + f_ji) - dkl;
    }
    out[i * mp + j] = v;
}

// ---- state -----------------------------------------------------------------------------------------------------------
static int svgp_state(mi355gp_sparse* s, int L) {
    SvgpState* sv = s->svgp;
    if (sv && sv->L == L && sv->mp == s->mp && sv->chunk == s->chunk && sv->n == s->n) return 0;
    svgp_release(s);
    sv = new SvgpState();
    s->svgp = sv;
    sv->L = L;
    sv->mp = s->mp;
    sv->chunk = s->chunk;
    sv->n = s->n;
    const size_t mm = (size_t)s->mp * s->mp;
    const long nv = (s->D + 1 > L ? s->D + 1 : L);
    HIP_CHECK(sv->Kmmi.alloc(mm));
    HIP_CHECK(sv->Ld.alloc(mm * L));
    HIP_CHECK(sv->Sd.alloc(mm * L));
    HIP_CHECK(sv->Si.alloc(mm * L));
    HIP_CHECK(sv->AdvA.alloc(mm * L));
    HIP_CHECK(sv->Tq.alloc(mm * L));
    HIP_CHECK(sv->U.alloc((size_t)s->chunk * s->mp));
    HIP_CHECK(sv->qm.alloc((size_t)s->mp * L));
    HIP_CHECK(sv->Kmmim.alloc((size_t)s->mp * L));
    HIP_CHECK(sv->Admu.alloc((size_t)s->mp * L));
    HIP_CHECK(sv->colPart.alloc((size_t)64 * s->mp * nv));
    HIP_CHECK(sv->rowPart.alloc((size_t)s->mp * (2 * L + 1)));
    HIP_CHECK(sv->red.alloc(2 * L + 1));
    HIP_CHECK(sv->dMu.alloc((size_t)s->n * L));
    HIP_CHECK(sv->dVv.alloc((size_t)s->n * L));
    HIP_CHECK(sv->dFmu.alloc((size_t)s->n * L));
    HIP_CHECK(sv->dFv.alloc((size_t)s->n * L));
    HIP_CHECK(sv->dQ.alloc((size_t)s->n));
    return 0;
}

// Kfu chunk (zero in the padding) and A^T = Kfu Kmm^-1 of rows [r0, r0 + rc) into s->Kfu / s->T
static int svgp_chunk_A(mi355gp_sparse* s, long r0, long rc) {
    SvgpState* sv = s->svgp;
    hipStream_t st = s->st;
    const long mp = s->mp, rcp = round_up(rc, NB);
    if (int rc2 = sparse_cross_rows(s, r0, rc, 0, rcp, nullptr)) return rc2;
    launch_gemm(st, 0, 1, rcp, mp, mp, s->Kfu, mp, sv->Kmmi, mp, s->T, mp, 1.0, 0.0);
    return 0;
}

static int svgp_common_checks(const mi355gp_sparse* s, const char* where) {
    if (!s || s->n <= 0) PART_FAIL("%s: set_data first", where);
    if (sharded(s)) PART_FAIL("%s: a row-sharded context is not supported by SVGP", where);
    if (s->dSvar) PART_FAIL("%s: the context holds input variances; SVGP takes certain inputs (mi355gp_sparse_set_data discards them)", where);
    return 0;
}

extern "C" {

// One SVGP.inference up to the likelihood's quadrature (svgp.py:12-56): q(u_d) = N(m_d, L_d L_d^T), d < L.
//   q_mean: M x L row-major; q_chol: L matrices M x M row-major, the lower triangle read (svgp.py:16, choleskies.flat_to_triang)
//   mu_out, v_out: N x L, the marginal means and variances of q(f) (svgp.py:45-51)
//   scalars_out[2 + L]: [0] the KL term (svgp.py:54-56), [1] log det Kmm, [2 + d] log det S_d
//   stage_ms[3] (optional): M x M phase, row phase, total
// Returns 0, LAPACK-style info > 0 when Kmm is not positive definite (the caller retries with extra_jitter as jitchol does,
// util/linalg.py:56-75) or a negative error.
int mi355gp_svgp_forward(mi355gp_sparse* s, int nparts, const mi355gp_part* parts, const double* Z, int64_t M, const double* q_mean,
                         const double* q_chol, int L, double extra_jitter, double* mu_out, double* v_out, double* scalars_out,
                         double* stage_ms) {
    if (int rc = svgp_common_checks(s, "mi355gp_svgp_forward")) return rc;
    if (L < 1 || L > SVGP_LMAX) PART_FAIL("mi355gp_svgp_forward: %d latent functions; between 1 and %d are supported", L, SVGP_LMAX);
    ARG_CHECK(parts && Z && M > 0 && q_mean && q_chol && mu_out && v_out && scalars_out, "mi355gp_svgp_forward: bad arguments");
    EngineShared gate(s->device);
    if (int rc = sparse_open(s, nparts, parts, M)) return rc;
    if (int rc = svgp_state(s, L)) return rc;
    SvgpState* sv = s->svgp;
    sv->fwd_ok = sv->winv_ok = false;
    hipStream_t st = s->st;
    const long n = s->n, m = s->m, mp = s->mp, chunk = s->chunk;
    const size_t mm = (size_t)mp * mp;
    s->mfma_prof.on = false;
    // q(u): m zero padded, L_d with the identity in the padding block; log det S_d = 2 sum log |L_d,ii| (svgp.py:23)
    std::vector<double> hqm((size_t)mp * L, 0.0), hld(mm * L, 0.0), logdetS((size_t)L, 0.0);
    for (long i = 0; i < m; ++i)
        for (int d = 0; d < L; ++d) hqm[(size_t)i * L + d] = q_mean[i * L + d];
    for (int d = 0; d < L; ++d) {
        double* dst = hld.data() + (size_t)d * mm;
        const double* src = q_chol + (size_t)d * m * m;
        for (long i = 0; i < m; ++i) {
            for (long j = 0; j <= i; ++j) dst[i * mp + j] = src[i * m + j];
            logdetS[(size_t)d] += 2.0 * log(fabs(src[i * m + i]));
        }
        for (long i = m; i < mp; ++i) dst[i * mp + i] = 1.0;
    }
    HIP_CHECK(hipMemcpyAsync(sv->qm, hqm.data(), sizeof(double) * mp * L, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(sv->Ld, hld.data(), sizeof(double) * mm * L, hipMemcpyHostToDevice, st));
    if (int rc = sparse_start(s, Z, nullptr, 0)) return rc;
    // ---- M x M phase -------------------------------------------------------------------------------------------------------
    // Kmm = K(Z) (+ the ladder's jitter only, svgp.py:37,40), Lm = chol, Xm = Lm^-1, Kmm^-1 = Xm^T Xm (svgp.py:40-42)
    auto rebuild_kmm = [&]() { build_kmm(s, s->Lm, s->T1, extra_jitter, /*lower_only=*/1, st); };
    rebuild_kmm();
    if (int rc = potrf_checked(st, s->Lm, s->Xm, s->Tm, s->Bi, mp, &s->ws, &s->h_info[0], rebuild_kmm)) return rc;
    launch_mm_sym(st, s->Bi, mp, sv->Kmmi);
    // S_d = L_d L_d^T (svgp.py:19-20) and S_d^-1 (svgp.py:22) through its own factorisation
    for (int d = 0; d < L; ++d) {
        double* Ld = sv->Ld + (size_t)d * mm;
        double* Sd = sv->Sd + (size_t)d * mm;
        launch_gemm(st, 0, 0, mp, mp, mp, Ld, mp, Ld, mp, Sd, mp, 1.0, 0.0);
        auto rebuild_s = [&]() { (void)hipMemcpyAsync(s->LB, Sd, sizeof(double) * mm, hipMemcpyDeviceToDevice, st); };
        rebuild_s();
        sv->h_info[d] = 0;
        if (int rc = potrf_checked(st, s->LB, s->XB, s->Tm, s->P, mp, &s->ws, &sv->h_info[d], rebuild_s)) return rc;
        launch_mm_sym(st, s->P, mp, sv->Si + (size_t)d * mm);
    }
    // Kmm^-1 m (svgp.py:54) and the sums of the KL term (svgp.py:55)
    hipLaunchKernelGGL(k_svgp_matvec, dim3((unsigned)((mp + 3) / 4)), dim3(256), 0, st, sv->Kmmi, mp, sv->qm, L, sv->Kmmim);
    hipLaunchKernelGGL(k_svgp_kl_rows, dim3((unsigned)m), dim3(256), 0, st, sv->Kmmi, sv->Sd, s->Lm, sv->qm, sv->Kmmim, L, mp, m,
                       sv->rowPart);
    launch_reduce_partials(st, sv->rowPart, (int)m, 2 * L + 1, sv->red);
    HIP_CHECK(hipEventRecord(s->ev[1], st));
    // ---- row phase: mu = A^T m, v_d = diag(A^T S_d A) + Kdiag - diag(A^T Kmn) (svgp.py:45-51) ------------------------------
    const double kdiag = s->diag_pt ? 0.0 : expression_kdiag(s->parts, s->terms);
    if (s->diag_pt)                                            // Kdiag by point, in s->dKd
        if (int rc = sparse_kdiag_data(s, nullptr, nullptr)) return rc;
    for (long r0 = 0; r0 < n; r0 += chunk) {
        const long rc = (n - r0 < chunk) ? (n - r0) : chunk;
        const long rcp = round_up(rc, NB);
        if (int rc2 = svgp_chunk_A(s, r0, rc)) return rc2;
        for (int d = 0; d < L; ++d) {
            launch_gemm(st, 0, 1, rcp, mp, mp, s->T, mp, sv->Ld + (size_t)d * mm, mp, sv->U, mp, 1.0, 0.0);
            hipLaunchKernelGGL(k_svgp_rowstats, dim3((unsigned)((rc + 3) / 4)), dim3(256), 0, st, s->T, s->Kfu, sv->U, mp, rc, sv->qm, L,
                               d, kdiag, s->diag_pt ? s->dKd + r0 : nullptr, sv->dMu + r0 * L, sv->dQ + r0, sv->dVv + r0 * L);
        }
    }
    HIP_CHECK(hipEventRecord(s->ev[2], st));
    std::vector<double> red((size_t)(2 * L + 1));
    HIP_CHECK(hipMemcpyAsync(mu_out, sv->dMu, sizeof(double) * n * L, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(v_out, sv->dVv, sizeof(double) * n * L, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(red.data(), sv->red, sizeof(double) * (2 * L + 1), hipMemcpyDeviceToHost, st));
    if (int rc = sparse_finish(s, 2, stage_ms)) return rc;      // (info > 0: Kmm not positive definite, the caller adds jitter)
    for (int d = 0; d < L; ++d)
        if (sv->h_info[d] > 0 || !std::isfinite(logdetS[(size_t)d])) {
            mi355gp_set_error("mi355gp_svgp_forward: Cholesky representation unstable: S_%d = L_%d L_%d^T is not positive definite "
                              "(info %d; svgp.py:25-26)", d, d, d, sv->h_info[d]);
            return -7;
        }
    const double logdetKmm = 2.0 * red[(size_t)(2 * L)];
    double KL = 0.0;
    for (int d = 0; d < L; ++d)                                              // svgp.py:55-56
        KL += -0.5 * logdetS[(size_t)d] - 0.5 * (double)m + 0.5 * logdetKmm + 0.5 * red[(size_t)d] + 0.5 * red[(size_t)(L + d)];
    scalars_out[0] = KL;
    scalars_out[1] = logdetKmm;
    for (int d = 0; d < L; ++d) scalars_out[2 + d] = logdetS[(size_t)d];
    sv->fwd_ok = true;
    s->svgp_result = true;
    return 0;
}

// The rest of SVGP.inference (svgp.py:84-117) and of SVGP.parameters_changed (core/svgp.py:57-65) from the likelihood's
// dF_dmu, dF_dv (N x L, already multiplied by batch_scale, svgp.py:80):
//   dtheta_out: the parts' parameter gradients, concatenated (dL_dKmm + dL_dKmn + dL_dKdiag terms summed, core/svgp.py:58-63)
//   dZ_out: M x D = gradients_X(dL_dKmm, Z) + gradients_X(dL_dKmn, Z, X) (core/svgp.py:65)
//   dm_out: M x L = dL_dm (svgp.py:99,112);  dchol_out: L x M x M, dL_dchol_d = 2 dL_dS_d L_d, lower triangle (svgp.py:114)
//   stage_ms[3] (optional): row phase, M x M phase, total
int mi355gp_svgp_backward(mi355gp_sparse* s, const double* dF_dmu, const double* dF_dv, double* dtheta_out, double* dZ_out,
                          double* dm_out, double* dchol_out, double* stage_ms) {
    if (int rc = svgp_common_checks(s, "mi355gp_svgp_backward")) return rc;
    ARG_CHECK(s->svgp_result && s->svgp && s->svgp->fwd_ok,
              "mi355gp_svgp_backward: no mi355gp_svgp_forward result on this context's data: run mi355gp_svgp_forward first");
    ARG_CHECK(dF_dmu && dF_dv, "mi355gp_svgp_backward: bad arguments");
    HIP_CHECK(hipSetDevice(s->device));
    EngineShared gate(s->device);
    SvgpState* sv = s->svgp;
    hipStream_t st = s->st;
    const long n = s->n, m = s->m, mp = s->mp, chunk = s->chunk;
    const int L = sv->L;
    const size_t mm = (size_t)mp * mp;
    HIP_CHECK(hipMemcpyAsync(sv->dFmu, dF_dmu, sizeof(double) * n * L, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(sv->dFv, dF_dv, sizeof(double) * n * L, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipEventRecord(s->ev[0], st));
    // tmp_d = 2 (S_d Kmmi - I) (svgp.py:92-93; zero in the padding block)
    for (int d = 0; d < L; ++d) {
        launch_gemm(st, 0, 1, mp, mp, mp, sv->Sd + (size_t)d * mm, mp, sv->Kmmi, mp, s->E, mp, 1.0, 0.0);
        launch_mm_axpby(st, s->E, 2.0, nullptr, 0.0, -2.0, mp, sv->Tq + (size_t)d * mm);
    }
    if (int rc = sparse_rows_gradients_reset(s)) return rc;
    HIP_CHECK(hipMemsetAsync(sv->Admu, 0, sizeof(double) * mp * L, st));
    // ---- row phase -----------------------------------------------------------------------------------------------------------
    const bool one_chunk = (n <= chunk);                      // A^T of a single chunk is still resident in s->T
    int nch = 0;
    for (long r0 = 0; r0 < n; r0 += chunk, ++nch) {
        const long rc = (n - r0 < chunk) ? (n - r0) : chunk;
        const long rcp = round_up(rc, NB);
        if (!one_chunk)
            if (int rc2 = svgp_chunk_A(s, r0, rc)) return rc2;
        const double* At = s->T;
        double* G = s->Kfu;                                   // this chunk's rows of dL_dKmn without the rank-L term (N x M)
        // A dF_dmu (svgp.py:86)
        const int nsm = launch_colreduce_multi(st, At, mp, rc, mp, sv->dFmu + r0 * L, L, 1, L, 0, sv->colPart);
        launch_sum_splits(st, sv->colPart, mp * L, nsm, 1, sv->Admu);
        for (int d = 0; d < L; ++d) {
            // Adv_d = A diag(dF_dv_d) (svgp.py:85), AdvA_d += Adv_d A^T (:88), G += Adv_d^T tmp_d (:96-97)
            hipLaunchKernelGGL(k_svgp_weight_rows, dim3((unsigned)rcp, (unsigned)((mp + 255) / 256)), dim3(256), 0, st, At, mp, rc, rcp,
                               sv->dFv + r0 * L, L, d, sv->U);
            launch_gemm(st, 1, 1, mp, mp, rcp, At, mp, sv->U, mp, sv->AdvA + (size_t)d * mm, mp, 1.0, nch > 0 ? 1.0 : 0.0);
            launch_gemm(st, 0, 1, rcp, mp, mp, sv->U, mp, sv->Tq + (size_t)d * mm, mp, G, mp, 1.0, d > 0 ? 1.0 : 0.0);
        }
        // dL_dKmn = (Kmmi m) dF_dmu^T + G (svgp.py:95): the rank-L term is formed inside the gradient pass
        const RankTerm rk{sv->dFmu + r0 * L, sv->Kmmim, L, 1.0, 1.0, nullptr};
        sparse_rows_gradients(s, rc, G, sv->U, rk, [&]() {
            hipLaunchKernelGGL(k_svgp_weights_times, dim3((unsigned)rcp, (unsigned)((mp + 255) / 256)), dim3(256), 0, st, G, sv->U, mp,
                               rc, rcp, m, sv->dFmu + r0 * L, sv->Kmmim, L);
        });
    }
    HIP_CHECK(hipEventRecord(s->ev[1], st));
    // ---- M x M phase ---------------------------------------------------------------------------------------------------------
    // sumA = sum_d AdvA_d (in Amat), tmp = (sum_d AdvA_d S_d) Kmmi (svgp.py:89, in T1), KSK = Kmmi (sum_d S_d) Kmmi (svgp.py:60, in Q2)
    hipLaunchKernelGGL(k_svgp_sum_lat, grid2d(mp, mp), dim3(256), 0, st, sv->AdvA, L, mp, s->Amat);
    for (int d = 0; d < L; ++d)
        launch_gemm(st, 0, 1, mp, mp, mp, sv->AdvA + (size_t)d * mm, mp, sv->Sd + (size_t)d * mm, mp, s->E, mp, 1.0, d > 0 ? 1.0 : 0.0);
    launch_gemm(st, 0, 1, mp, mp, mp, s->E, mp, sv->Kmmi, mp, s->T1, mp, 1.0, 0.0);
    hipLaunchKernelGGL(k_svgp_sum_lat, grid2d(mp, mp), dim3(256), 0, st, sv->Sd, L, mp, s->E);
    launch_gemm(st, 0, 1, mp, mp, mp, sv->Kmmi, mp, s->E, mp, s->P, mp, 1.0, 0.0);
    launch_gemm(st, 0, 1, mp, mp, mp, s->P, mp, sv->Kmmi, mp, s->Q2, mp, 1.0, 0.0);
    hipLaunchKernelGGL(k_svgp_dLdKmm, grid2d(mp, mp), dim3(256), 0, st, s->Amat, s->T1, sv->Kmmi, s->Q2, sv->Admu, sv->Kmmim, L, mp, m,
                       s->dLdKmm);
    // dL_dchol_d = 2 dL_dS_d L_d, dL_dS_d = AdvA_d - (Kmmi - S_d^-1) / 2 (svgp.py:59,100,112,114), into Tq (tmp_d is spent)
    for (int d = 0; d < L; ++d) {
        launch_mm_axpby(st, sv->Kmmi, -0.5, sv->Si + (size_t)d * mm, 0.5, 0.0, mp, s->E);
        launch_mm_axpby(st, sv->AdvA + (size_t)d * mm, 1.0, s->E, 1.0, 0.0, mp, s->P);
        launch_gemm(st, 0, 1, mp, mp, mp, s->P, mp, sv->Ld + (size_t)d * mm, mp, sv->Tq + (size_t)d * mm, mp, 2.0, 0.0);
    }
    sparse_kmm_gradients(s);
    // a per-point diagonal: update_gradients_diag's sums against w_n = dL_dKdiag_n = sum_d dF_dv[n][d] (svgp.py:117)
    std::vector<double> dsums, wrow;
    if (s->diag_pt) {
        wrow.assign((size_t)n, 0.0);
        for (long i = 0; i < n; ++i)
            for (int d = 0; d < L; ++d) wrow[(size_t)i] += dF_dv[i * L + d];
        HIP_CHECK(s->diagW.need((size_t)n));
        HIP_CHECK(hipMemcpyAsync(s->diagW, wrow.data(), sizeof(double) * n, hipMemcpyHostToDevice, st));
        if (int rc = sparse_kdiag(s, s->dX, n, s->diagW, nullptr, &dsums)) return rc;
    }
    HIP_CHECK(hipEventRecord(s->ev[2], st));
    // ---- small results to the host ------------------------------------------------------------------------------------------
    KernGrads kg;
    std::vector<double> admu((size_t)mp * L), kmmim((size_t)mp * L);
    if (int rc = sparse_fetch_gradients(s, true, &kg)) return rc;
    HIP_CHECK(hipMemcpyAsync(admu.data(), sv->Admu, sizeof(double) * mp * L, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(kmmim.data(), sv->Kmmim, sizeof(double) * mp * L, hipMemcpyDeviceToHost, st));
    if (dchol_out)
        for (int d = 0; d < L; ++d)
            HIP_CHECK(hipMemcpy2DAsync(dchol_out + (size_t)d * m * m, sizeof(double) * m, sv->Tq + (size_t)d * mm, sizeof(double) * mp,
                                       sizeof(double) * m, m, hipMemcpyDeviceToHost, st));
    if (int rc = sparse_finish(s, 2, stage_ms)) return rc;
    if (dchol_out)                                              // the lower triangle is the gradient (choleskies.triang_to_flat)
        for (int d = 0; d < L; ++d)
            for (long i = 0; i < m; ++i)
                for (long j = i + 1; j < m; ++j) dchol_out[(size_t)d * m * m + i * m + j] = 0.0;
    if (dm_out)                                                 // dL_dm = A dF_dmu - Kmmi m (svgp.py:58,99,112)
        for (long i = 0; i < m * L; ++i) dm_out[i] = admu[(size_t)i] - kmmim[(size_t)i];
    // dL_dKdiag = dF_dv.sum(1) (svgp.py:117): update_gradients_diag gives its sum to every part's variance
    double sum_dv = 0.0;
    for (long i = 0; i < n * L; ++i) sum_dv += dF_dv[i];
    if (s->diag_pt) sparse_diag_dtheta(s, dsums, 1.0, &kg.ddiag);
    sparse_assemble_gradients(s, kg, sum_dv, dtheta_out, dZ_out);             // (core/svgp.py:58-65)
    return 0;
}

// woodbury_inv_d = Kmmi - Kmmi S_d Kmmi (posterior.py:95-107 for the mean / cov form), once per forward call
static int svgp_ensure_winv(mi355gp_sparse* s) {
    SvgpState* sv = s->svgp;
    if (sv->winv_ok) return 0;
    hipStream_t st = s->st;
    const long mp = s->mp;
    const size_t mm = (size_t)mp * mp;
    if (!sv->Wd.p) HIP_CHECK(sv->Wd.alloc(mm * sv->L));
    for (int d = 0; d < sv->L; ++d) {
        launch_gemm(st, 0, 1, mp, mp, mp, sv->Kmmi, mp, sv->Sd + (size_t)d * mm, mp, s->E, mp, 1.0, 0.0);
        launch_gemm(st, 0, 1, mp, mp, mp, s->E, mp, sv->Kmmi, mp, s->P, mp, 1.0, 0.0);
        launch_mm_axpby(st, sv->Kmmi, 1.0, s->P, -1.0, 0.0, mp, sv->Wd + (size_t)d * mm);
    }
    sv->winv_ok = true;
    return 0;
}

// Posterior._raw_predict (posterior.py:198-262) for the posterior of the last mi355gp_svgp_forward on this context:
// woodbury_vector = Kmm^-1 m and woodbury_inv_d = Kmm^-1 - Kmm^-1 S_d Kmm^-1 stay resident.
//   mu_out: Mn x L;  var_out (optional): Mn x L, or Mn x Mn x L with full_cov (one latent after the other, posterior.py:218-246)
// wv_out (optional, M x L) / winv_out (optional, L x M x M): the two Woodbury quantities themselves.
// The kernel (parts) must be the one of the forward call.
int mi355gp_svgp_predict(mi355gp_sparse* s, int nparts, const mi355gp_part* parts, const double* Xnew, int64_t Mn, int full_cov,
                         double* mu_out, double* var_out, double* wv_out, double* winv_out) {
    if (int rc = svgp_common_checks(s, "mi355gp_svgp_predict")) return rc;
    ARG_CHECK(s->svgp_result && s->svgp && s->svgp->fwd_ok,
              "mi355gp_svgp_predict: no mi355gp_svgp_forward result on this context's data: run mi355gp_svgp_forward first");
    ARG_CHECK((Xnew && Mn > 0 && mu_out) || (Mn == 0 && (wv_out || winv_out)), "mi355gp_svgp_predict: bad arguments");
    HIP_CHECK(hipSetDevice(s->device));
    EngineShared gate(s->device);
    SvgpState* sv = s->svgp;
    hipStream_t st = s->st;
    const long m = s->m, mp = s->mp, L = sv->L;
    const size_t mm = (size_t)mp * mp;
    if (var_out || winv_out)
        if (int rc = svgp_ensure_winv(s)) return rc;
    if (wv_out) {
        std::vector<double> h((size_t)mp * L);
        HIP_CHECK(hipMemcpy(h.data(), sv->Kmmim, sizeof(double) * mp * L, hipMemcpyDeviceToHost));
        memcpy(wv_out, h.data(), sizeof(double) * m * L);
    }
    if (winv_out) {
        for (long d = 0; d < L; ++d)
            HIP_CHECK(hipMemcpy2DAsync(winv_out + (size_t)d * m * m, sizeof(double) * m, sv->Wd + (size_t)d * mm, sizeof(double) * mp,
                                       sizeof(double) * m, m, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
    }
    if (Mn == 0) return 0;
    if (int rc = prepare_sparse_parts(s, nparts, parts)) return rc;
    scale_for_parts(s, s->dZ, m, mp, true);
    NewPoints q;
    if (int rc = sparse_newpoints(s, Xnew, Mn, full_cov && var_out, sv->Kmmim, (int)L, "mi355gp_svgp_predict", &q)) return rc;   // mu = Kx^T Kmmi m
    HIP_CHECK(hipMemcpyAsync(mu_out, q.Mu, sizeof(double) * Mn * L, hipMemcpyDeviceToHost, st));
    if (var_out) {
        std::vector<double> hv(full_cov ? (size_t)Mn * Mn : (size_t)Mn);
        for (long d = 0; d < L; ++d) {                            // one latent after the other, the host interleaving each
            if (int rc = sparse_newpoints_var(s, &q, sv->Wd + (size_t)d * mm, full_cov != 0, /*keep_kss=*/true)) return rc;
            if (!full_cov) {
                HIP_CHECK(hipMemcpyAsync(hv.data(), q.var, sizeof(double) * Mn, hipMemcpyDeviceToHost, st));
                HIP_CHECK(hipStreamSynchronize(st));
                for (int64_t i = 0; i < Mn; ++i) var_out[i * L + d] = hv[(size_t)i] < 1e-15 ? 1e-15 : hv[(size_t)i];   // posterior.py:248
            } else {
                HIP_CHECK(hipMemcpy2DAsync(hv.data(), sizeof(double) * Mn, q.var, sizeof(double) * q.mnp, sizeof(double) * Mn, Mn,
                                           hipMemcpyDeviceToHost, st));
                HIP_CHECK(hipStreamSynchronize(st));
                for (int64_t i = 0; i < Mn * Mn; ++i) var_out[i * L + d] = hv[(size_t)i];
            }
        }
    }
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
