// psi_lin.hip -- what the uncertain-input fit needs on top of the certain-input passes for a Linear part, and on top of the RBF
// psi kernels for Bias parts (linear_psi_comp.py, static.py:133-189, add.py:147-266; the algebra: DESIGN.md 6r).  Everything
// here is M x M, M x D or rows x D sized; the one pass over N x M weights is k_grad_rows_lin (kern_sparse.hip).  Every sum
// has a fixed order, there are no atomics.  Also the stand-alone probe of the row kernel (include/mi355gp_debug_psi_lin.h).
#include <vector>

#include "../../include/mi355gp.h"
#include "../../include/mi355gp_debug_psi_lin.h"
#include "internal.h"
#include "psi.h"

// psi2[i][j] += sum_q (il_q^4 s_q) z_iq z_jq, i, j < m: the Z diag(variance^2 s) Z^T term of a Linear part (il = sqrt(variance),
// s = sums[0 .. D) the column sums of the input variances)
__global__ void k_psi2_rank_add(const double* __restrict__ Z, const double* __restrict__ il, const double* __restrict__ sums, long m,
                                int D, double* __restrict__ psi2, long ld) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= m) return;
    double a = 0.0;
    for (int q = 0; q < D; ++q) {
        const double v = il[q] * il[q];
        a = fma(v * v * sums[q] * Z[i * D + q], Z[j * D + q], a);
    }
    psi2[i * ld + j] += a;
}

// out[i][q] = sum_{j < m} A[j][i] Z[j][q]  (A symmetric in its leading m x m: A Z, read along rows)
__global__ void k_mm_times_z(const double* __restrict__ A, long ld, const double* __restrict__ Z, long m, int D,
                             double* __restrict__ out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int q = blockIdx.y;
    if (i >= m) return;
    double a = 0.0;
    for (long j = 0; j < m; ++j) a = fma(A[j * ld + i], Z[j * D + q], a);
    out[i * D + q] = a;
}

// out[j] = scale sum_{i < m} A[i][j], j < m
__global__ void k_mm_colsums(const double* __restrict__ A, long ld, long m, double scale, double* __restrict__ out) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    double a = 0.0;
    for (long i = 0; i < m; ++i) a += A[i * ld + j];
    out[j] = scale * a;
}

// psi2[i][j] += b (c_i + c_j) + nb2, i, j < m: Bias against the psi1 column sums c of the input-dependent part, and against itself
__global__ void k_psi2_bias_add(double* __restrict__ psi2, long ld, long m, const double* __restrict__ c, double b, double nb2) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= m) return;
    psi2[i * ld + j] += fma(b, c[i] + c[j], nb2);
}

// psi1Y[j][d] += b vs[d], j < m: psi1^T V of a constant psi1
__global__ void k_psi1y_bias_add(double* __restrict__ psi1Y, long m, int Dy, const double* __restrict__ vs, double b) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m * Dy) return;
    psi1Y[k] = fma(b, vs[k % Dy], psi1Y[k]);
}

// var[n][d] = max(base[n] + sum_q S[n][q] g[d][q], 1e-15): the Linear predictive variance at uncertain points from the
// certain-input one at the means (base, not clipped)
__global__ void k_lin_predvar(const double* __restrict__ base, const double* __restrict__ S, const double* __restrict__ g, long rows,
                              int D, int Dy, double* __restrict__ var) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= rows * Dy) return;
    const long n = k / Dy;
    const int d = (int)(k - n * Dy);
    double a = base[n];
    for (int q = 0; q < D; ++q) a = fma(S[n * D + q], g[d * D + q], a);
    var[k] = a > 1e-15 ? a : 1e-15;
}

// Bias parts in the prediction at uncertain points of an RBF part: mean[n][d] += bsl[d];  C[n][d] (optional, rows x (Dy + 1))
// += sum_m psi1[n][m] u[m][d] + cst[d]
__global__ void k_psi_bias_pred(const double* __restrict__ psi1, long ldp, const double* __restrict__ u, const double* __restrict__ cst,
                                const double* __restrict__ bsl, long rows, long m, int Dy, double* __restrict__ C,
                                double* __restrict__ mean) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= rows * Dy) return;
    const long n = k / Dy;
    const int d = (int)(k - n * Dy);
    mean[k] += bsl[d];
    if (!C) return;
    double a = cst[d];
    for (long j = 0; j < m; ++j) a = fma(psi1[n * ldp + j], u[j * Dy + d], a);
    C[n * (Dy + 1) + d] += a;
}

static inline dim3 grid_mm(long m) { return dim3((unsigned)((m + 255) / 256), (unsigned)m); }

void launch_psi2_rank_add(hipStream_t st, const double* Z, const double* il, const double* sums, long m, int D, double* psi2, long ld) {
    hipLaunchKernelGGL(k_psi2_rank_add, grid_mm(m), dim3(256), 0, st, Z, il, sums, m, D, psi2, ld);
}
void launch_mm_times_z(hipStream_t st, const double* A, long ld, const double* Z, long m, int D, double* out) {
    hipLaunchKernelGGL(k_mm_times_z, dim3((unsigned)((m + 255) / 256), (unsigned)D), dim3(256), 0, st, A, ld, Z, m, D, out);
}
void launch_mm_colsums(hipStream_t st, const double* A, long ld, long m, double scale, double* out) {
    hipLaunchKernelGGL(k_mm_colsums, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, A, ld, m, scale, out);
}
void launch_psi2_bias_add(hipStream_t st, double* psi2, long ld, long m, const double* c, double b, double nb2) {
    hipLaunchKernelGGL(k_psi2_bias_add, grid_mm(m), dim3(256), 0, st, psi2, ld, m, c, b, nb2);
}
void launch_psi1y_bias_add(hipStream_t st, double* psi1Y, long m, int Dy, const double* vs, double b) {
    hipLaunchKernelGGL(k_psi1y_bias_add, dim3((unsigned)((m * Dy + 255) / 256)), dim3(256), 0, st, psi1Y, m, Dy, vs, b);
}
void launch_lin_predvar(hipStream_t st, const double* base, const double* S, const double* g, long rows, int D, int Dy, double* var) {
    hipLaunchKernelGGL(k_lin_predvar, dim3((unsigned)((rows * Dy + 255) / 256)), dim3(256), 0, st, base, S, g, rows, D, Dy, var);
}
void launch_psi_bias_pred(hipStream_t st, const double* psi1, long ldp, const double* u, const double* cst, const double* bsl, long rows,
                          long m, int Dy, double* C, double* mean) {
    hipLaunchKernelGGL(k_psi_bias_pred, dim3((unsigned)((rows * Dy + 255) / 256)), dim3(256), 0, st, psi1, ldp, u, cst, bsl, rows, m, Dy, C,
                       mean);
}

extern "C" {

// The row kernel on its own (see the header): everything is uploaded, scaled as the sparse context scales it, run once and
// fetched.  fused != 0: k_grad_rows_lin with the weights formed on the fly (D <= 16); 0: the weights in memory, then the plain kernel.
int mi355gp_dbg_psi_lin_rows(int device, int fused, const double* W, const double* Y, const double* V, const double* rowscale,
                               double beta, double gscale, const double* X, const double* Z, const double* variances, double c0,
                               int64_t rows, int64_t M, int D, int Dy, double* out, int reps, double* ms_out) {
    ARG_CHECK(W && X && Z && variances && out && rows > 0 && M > 0 && D >= 1 && D <= 64, "mi355gp_dbg_psi_lin_rows: bad arguments");
    ARG_CHECK(!Y || (V && Dy >= 1), "mi355gp_dbg_psi_lin_rows: a rank term needs Y (rows x Dy), V (M x Dy) and Dy >= 1");
    ARG_CHECK(!fused || D <= 16, "mi355gp_dbg_psi_lin_rows: the fused row kernel takes at most 16 input dimensions");
    HIP_CHECK(hipSetDevice(device));
    EngineShared gate(device);
    hipStream_t st = nullptr;
    const long ldw = round_up(M, 4);
    std::vector<double> il((size_t)D), wp((size_t)rows * ldw, 0.0);
    for (int q = 0; q < D; ++q) {
        ARG_CHECK(variances[q] >= 0.0, "mi355gp_dbg_psi_lin_rows: negative variance");
        il[(size_t)q] = std::sqrt(variances[q]);
    }
    for (long i = 0; i < rows; ++i)
        for (long j = 0; j < M; ++j) wp[(size_t)(i * ldw + j)] = W[i * M + j];
    DevBuf dW, dY, dV, dRs, dX, dZ, dIl, dXt, dZt, dG, dOut;
    HIP_CHECK(dW.alloc(wp.size()));
    HIP_CHECK(dX.alloc(rows * D));
    HIP_CHECK(dZ.alloc(M * D));
    HIP_CHECK(dIl.alloc(D));
    HIP_CHECK(dXt.alloc(rows * D));
    HIP_CHECK(dZt.alloc(M * D));
    HIP_CHECK(dOut.alloc(rows * D));
    HIP_CHECK(hipMemcpy(dW, wp.data(), sizeof(double) * wp.size(), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dX, X, sizeof(double) * rows * D, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dZ, Z, sizeof(double) * M * D, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dIl, il.data(), sizeof(double) * D, hipMemcpyHostToDevice));
    RankTerm rk{nullptr, nullptr, 0, 0.0, 1.0, nullptr};
    if (Y) {
        HIP_CHECK(dY.alloc(rows * Dy));
        HIP_CHECK(dV.alloc(M * Dy));
        HIP_CHECK(hipMemcpy(dY, Y, sizeof(double) * rows * Dy, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dV, V, sizeof(double) * M * Dy, hipMemcpyHostToDevice));
        if (rowscale) {
            HIP_CHECK(dRs.alloc(rows));
            HIP_CHECK(hipMemcpy(dRs, rowscale, sizeof(double) * rows, hipMemcpyHostToDevice));
        }
        rk = RankTerm{dY, dV, Dy, beta, gscale, rowscale ? (const double*)dRs : nullptr};
    }
    launch_scale_inputs(st, dX, rows, D, dIl, 1, dXt, rows);
    launch_scale_inputs(st, dZ, M, D, dIl, 1, dZt, M);
    const double* g = dW;
    if (!fused && Y) {
        HIP_CHECK(dG.alloc(wp.size()));
        launch_form_rank_weights(st, dW, ldw, rows, M, rk, dG);
        g = dG;
    }
    auto once = [&]() {
        if (fused) launch_grad_rows_lin(st, dXt, rows, rows, D, dZt, M, M, dW, ldw, rk, dIl, c0, dOut);
        else launch_rows_lin_plain(st, dXt, rows, rows, D, dZt, M, M, g, ldw, dIl, c0, dOut);
    };
    once();
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    if (ms_out && reps >= 1) {
        hipEvent_t e0, e1;
        HIP_CHECK(hipEventCreate(&e0));
        HIP_CHECK(hipEventCreate(&e1));
        for (int k = 0; k < reps; ++k) {
            HIP_CHECK(hipEventRecord(e0, st));
            once();
            HIP_CHECK(hipEventRecord(e1, st));
            HIP_CHECK(hipEventSynchronize(e1));
            float ms = 0.0f;
            HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
            ms_out[k] = (double)ms;
        }
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
    }
    HIP_CHECK(hipMemcpy(out, dOut, sizeof(double) * rows * D, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
