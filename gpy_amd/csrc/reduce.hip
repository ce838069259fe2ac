// reduce.hip -- the reductions, triangular solves and fetch helpers that stage no input slabs: the fixed-order combine of the
// gradient records, alpha = X^T (X R), the scalars of an evaluation, host-shaped views of padded matrices, column and row
// reductions of the prediction and sparse paths, row scalings.
#include <cstdint>

#include "internal.h"

// out[0] = (nu + n) / (nu + beta - 2) with beta = scal[0] = sum(alpha * R)   (exact_studentt_inference.py:46,51)
__global__ void k_studentt_scale(const double* __restrict__ scal, double nu, double n, double* __restrict__ out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) out[0] = (nu + n) / (nu + scal[0] - 2.0);
}
void launch_studentt_scale(hipStream_t st, const double* scal, double nu, long n, double* out) {
    hipLaunchKernelGGL(k_studentt_scale, dim3(1), dim3(64), 0, st, scal, nu, (double)n, out);
}

// out[c] = sum_b partials[b][c], fixed order (bit-reproducible run to run)
__global__ void k_reduce_partials(const double* __restrict__ partials, int nblocks, int stride,
                                  double* __restrict__ out) {
    __shared__ double red[256];
    const int c = blockIdx.x, t = threadIdx.x;
    double s = 0.0;
    for (int b = t; b < nblocks; b += 256) s += partials[(long)b * stride + c];
    red[t] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (t < k) red[t] += red[t + k];
        __syncthreads();
    }
    if (t == 0) out[c] = red[0];
}

void launch_reduce_partials(hipStream_t st, const double* partials, int nblocks, int stride, double* out) {
    hipLaunchKernelGGL(k_reduce_partials, dim3(stride), dim3(256), 0, st, partials, nblocks, stride, out);
}

// ------------------------------------------------------------------------------------------------
// alpha = X^T (X R) with X = L^-1 lower triangular (replaces lapack.dpotrs, GPy/util/linalg.py:116-125).
// pass 1: one wave per row, y_i = sum_{j<=i} X_ij R_j
template <int DC>
__global__ __launch_bounds__(256) void k_trmv_rows(const double* __restrict__ X, long ld, long n,
                                                   const double* __restrict__ R, int Dy, int d0,
                                                   double* __restrict__ y) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    double acc[DC];
#pragma unroll
    for (int d = 0; d < DC; ++d) acc[d] = 0.0;
    const double* xr = X + i * ld;
    // eight 512-byte row segments in flight per wave (one load per lane and segment was one load in flight: 0.4-0.8 TB/s, and the
    // pass sits on the CUs X^T X wants); the sums run in the same order as before: the same bits
    long j = lane;
    for (; j + 7 * 64 <= i; j += 8 * 64) {
        double x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = xr[j + u * 64];
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int d = 0; d < DC; ++d)
                if (d0 + d < Dy) acc[d] = fma(x[u], R[(j + u * 64) * Dy + d0 + d], acc[d]);
    }
    for (; j <= i; j += 64) {
        const double x = xr[j];
#pragma unroll
        for (int d = 0; d < DC; ++d)
            if (d0 + d < Dy) acc[d] = fma(x, R[j * Dy + d0 + d], acc[d]);
    }
#pragma unroll
    for (int d = 0; d < DC; ++d) {
        double v = acc[d];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
        if (lane == 0 && d0 + d < Dy) y[i * Dy + d0 + d] = v;
    }
}

// pass 2: partial column sums over chunks of `crows` rows: part[chunk][j][d] = sum_{i in chunk, i>=j} X_ij y_i
// (crows = 64 up to N = 16384: four times as many, four times shorter blocks than with 256 -- at N = 4096 the pass took
//  300 us on 256 blocks of 256 sequential row steps and was as long as the X^T X it is meant to hide under)
int trmv_chunk_rows(long n) { return n <= 16384 ? 64 : 256; }
template <int DC>
__global__ __launch_bounds__(256) void k_trmv_cols(const double* __restrict__ X, long ld, long n,
                                                   const double* __restrict__ y, int Dy, int d0,
                                                   double* __restrict__ part, int crows) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    const long c = blockIdx.y;
    const long ibeg = c * crows, iend = (ibeg + crows < n) ? ibeg + crows : n;
    if ((long)blockIdx.x * 256 >= iend) return;   // whole block above the diagonal band: no contribution
    double acc[DC];
#pragma unroll
    for (int d = 0; d < DC; ++d) acc[d] = 0.0;
    if (j < n) {
        // the rows of the chunk eight at a time (eight independent loads in flight per thread instead of one); rows above the
        // diagonal are skipped by predicate, the sums run in the same order as before: the same bits
        long i = ibeg;
        for (; i + 8 <= iend; i += 8) {
            double x[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) x[u] = (i + u >= j) ? X[(i + u) * ld + j] : 0.0;
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (i + u >= j) {
#pragma unroll
                    for (int d = 0; d < DC; ++d)
                        if (d0 + d < Dy) acc[d] = fma(x[u], y[(i + u) * Dy + d0 + d], acc[d]);
                }
        }
        for (i = (i > j ? i : j); i < iend; ++i) {
            const double x = X[i * ld + j];
#pragma unroll
            for (int d = 0; d < DC; ++d)
                if (d0 + d < Dy) acc[d] = fma(x, y[i * Dy + d0 + d], acc[d]);
        }
#pragma unroll
        for (int d = 0; d < DC; ++d)
            if (d0 + d < Dy) part[(c * n + j) * Dy + d0 + d] = acc[d];
    }
}

__global__ void k_trmv_finish(const double* __restrict__ part, long n, int Dy, long nchunks,
                              double* __restrict__ alpha, int crows) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * Dy) return;
    const long j = idx / Dy;
    double s = 0.0;
    long c = j / crows;
    for (; c + 8 <= nchunks; c += 8) {                       // eight partials in flight (was: one dependent load per chunk)
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = part[(c + u) * n * Dy + idx];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; c < nchunks; ++c) s += part[c * n * Dy + idx];
    alpha[idx] = s;
}

void launch_tri_matvec(hipStream_t st, const double* X, long ld, long n, const double* R, int Dy, double* tmp,
                       double* alpha, double* partials) {
    const int crows = trmv_chunk_rows(n);
    const long nchunks = (n + crows - 1) / crows, ncolb = (n + 255) / 256;
    for (int d0 = 0; d0 < Dy; d0 += 4)
        hipLaunchKernelGGL((k_trmv_rows<4>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, X, ld, n, R, Dy, d0, tmp);
    for (int d0 = 0; d0 < Dy; d0 += 4)
        hipLaunchKernelGGL((k_trmv_cols<4>), dim3((unsigned)ncolb, (unsigned)nchunks), dim3(256), 0, st, X, ld, n,
                           tmp, Dy, d0, partials, crows);
    hipLaunchKernelGGL(k_trmv_finish, dim3((unsigned)((n * Dy + 255) / 256)), dim3(256), 0, st, partials, n, Dy,
                       nchunks, alpha, crows);
}

// ------------------------------------------------------------------------------------------------
// out3[0] = sum alpha*R ; out3[1] = sum alpha^2 ; out3[2] = trace(W) ; out3[3] = 2*sum(logsum)
// diag_out[i] = 0.5*(sum_d alpha_id^2 - Dy*W_ii)   (= diag(dL_dK), exact_gaussian_inference.py:70-72)
__global__ __launch_bounds__(1024) void k_scalars(const double* __restrict__ alpha, const double* __restrict__ R,
                                                  const double* __restrict__ W, long ldw, long n, int Dy,
                                                  const double* __restrict__ logsum, long nblk,
                                                  double* __restrict__ out4, double* __restrict__ diag_out,
                                                  const int* __restrict__ info) {
    __shared__ double red[4][1024];
    const int t = threadIdx.x;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (long i = t; i < n; i += 1024) {
        double a2 = 0.0;
        for (int d = 0; d < Dy; ++d) {
            const double a = alpha[i * Dy + d];
            s0 = fma(a, R[i * Dy + d], s0);
            a2 = fma(a, a, a2);
        }
        s1 += a2;
        const double w = W ? W[i * ldw + i] : 0.0;
        s2 += w;
        if (diag_out) diag_out[i] = 0.5 * (a2 - (double)Dy * w);
    }
    for (long b = t; b < nblk; b += 1024) s3 += logsum[b];
    red[0][t] = s0; red[1][t] = s1; red[2][t] = s2; red[3][t] = s3;
    __syncthreads();
    for (int k = 512; k > 0; k >>= 1) {
        if (t < k) {
            red[0][t] += red[0][t + k]; red[1][t] += red[1][t + k];
            red[2][t] += red[2][t + k]; red[3][t] += red[3][t + k];
        }
        __syncthreads();
    }
    if (t == 0) {
        out4[0] = red[0][0]; out4[1] = red[1][0]; out4[2] = red[2][0]; out4[3] = 2.0 * red[3][0];
        if (info) out4[6] = (double)info[0];      // the factorisation's LAPACK-style info rides along with the scalars
    }
}

void launch_scalars(hipStream_t st, const double* alpha, const double* R, const double* W, long ldw, long n,
                       int Dy, const double* logsum, long nblk, double* out4, double* diag_out, const int* info) {
    hipLaunchKernelGGL(k_scalars, dim3(1), dim3(1024), 0, st, alpha, R, W, ldw, n, Dy, logsum, nblk, out4, diag_out, info);
}

// ------------------------------------------------------------------------------------------------
// dense host-shaped views of padded device matrices (lazy fetch path; PCIe-bound, not on the hot loop)
__global__ void k_extract(const double* __restrict__ A, long ld, long n, int mode, const double* __restrict__ alpha,
                          int Dy, double* __restrict__ out, int transpose, const double* __restrict__ aa_scale) {
    const long nbx = (n + 255) / 256;
    const long i = blockIdx.x / nbx;
    const long j = (blockIdx.x - i * nbx) * 256 + threadIdx.x;
    if (j >= n) return;
    double v;
    if (mode == 0) {
        v = (j <= i) ? A[i * ld + j] : 0.0;
    } else {
        const long hi = i > j ? i : j, lo = i > j ? j : i;
        v = A[hi * ld + lo];
        if (mode == 2) {
            double aa = 0.0;
            for (int d = 0; d < Dy; ++d) aa = fma(alpha[i * Dy + d], alpha[j * Dy + d], aa);
            // Student-t process: the alpha alpha^T term carries (nu+N)/(nu+beta-2) (exact_studentt_inference.py:46)
            v = 0.5 * ((aa_scale ? aa_scale[0] : 1.0) * aa - (double)Dy * v);
        }
    }
    if (transpose) out[j * n + i] = v; else out[i * n + j] = v;
}

void launch_extract(hipStream_t st, const double* A, long ld, long n, int mode, const double* alpha, int Dy,
                    double* out, int transpose, const double* aa_scale) {
    hipLaunchKernelGGL(k_extract, dim3((unsigned)(((n + 255) / 256) * n)), dim3(256), 0, st, A, ld, n, mode, alpha, Dy,
                       out, transpose, aa_scale);
}

// A (npad x npad) <- dense src (n x n) + diag(noise + jit); identity in the padding
__global__ void k_pad_from_dense(const double* __restrict__ src, long n, double* __restrict__ A, long npad,
                                 const double* __restrict__ noise, long noise_len, double jit) {
    const long nbx = (npad + 255) / 256;
    const long i = blockIdx.x / nbx;
    const long j = (blockIdx.x - i * nbx) * 256 + threadIdx.x;
    if (j >= npad) return;
    double v;
    if (i < n && j < n) {
        v = src[i * n + j];
        if (i == j) v += (noise ? noise[noise_len > 1 ? i : 0] : 0.0) + jit;
    } else {
        v = (i == j) ? 1.0 : 0.0;
    }
    A[i * npad + j] = v;
}

void launch_pad_from_dense(hipStream_t st, const double* src, long n, double* A, long npad, const double* noise,
                           long noise_len, double jit) {
    hipLaunchKernelGGL(k_pad_from_dense, dim3((unsigned)(((npad + 255) / 256) * npad)), dim3(256), 0, st, src, n, A,
                       npad, noise, noise_len, jit);
}

// ------------------------------------------------------------------------------------------------
// Column reductions for prediction: 64 columns per block, 4 row groups per column, fixed-order combine.
__global__ __launch_bounds__(256) void k_col_reduce(const double* __restrict__ M, long ld, long rows, long cols,
                                                    const double* __restrict__ v, int Dy, int d, double c0, int mode,
                                                    double* __restrict__ out) {
    __shared__ double red[4][64];
    const int tx = threadIdx.x & 63, g = threadIdx.x >> 6;
    const long j = (long)blockIdx.x * 64 + tx;
    double s = 0.0;
    if (j < cols) {
        for (long i = g; i < rows; i += 4) {
            const double x = M[i * ld + j];
            s = (mode == 0) ? fma(x, v[i * Dy + d], s) : fma(x, x, s);
        }
    }
    red[g][tx] = s;
    __syncthreads();
    if (g == 0 && j < cols) {
        const double tot = (red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx]);
        if (mode == 0) out[j * Dy + d] = tot; else out[j] = c0 - tot;
    }
}

void launch_col_reduce(hipStream_t st, const double* M, long ld, long rows, long cols, const double* v, int Dy,
                       double c0, int mode, double* out) {
    const unsigned nb = (unsigned)((cols + 63) / 64);
    if (mode == 0) {
        for (int d = 0; d < Dy; ++d)
            hipLaunchKernelGGL(k_col_reduce, dim3(nb), dim3(256), 0, st, M, ld, rows, cols, v, Dy, d, c0, 0, out);
    } else {
        hipLaunchKernelGGL(k_col_reduce, dim3(nb), dim3(256), 0, st, M, ld, rows, cols, v, 1, 0, c0, 1, out);
    }
}

// y = X r (lower-triangular X) and a = X^T y as separate products (sparse path: LB^-1 Lm^-1 psi1Y etc.)
void launch_trmv_lower(hipStream_t st, const double* X, long ld, long n, const double* R, int Dy, double* y) {
    for (int d0 = 0; d0 < Dy; d0 += 4)
        hipLaunchKernelGGL((k_trmv_rows<4>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, X, ld, n, R, Dy, d0, y);
}
void launch_trmv_lower_T(hipStream_t st, const double* X, long ld, long n, const double* y, int Dy, double* out,
                         double* partials) {
    const int crows = trmv_chunk_rows(n);
    const long nchunks = (n + crows - 1) / crows, ncolb = (n + 255) / 256;
    for (int d0 = 0; d0 < Dy; d0 += 4)
        hipLaunchKernelGGL((k_trmv_cols<4>), dim3((unsigned)ncolb, (unsigned)nchunks), dim3(256), 0, st, X, ld, n, y,
                           Dy, d0, partials, crows);
    hipLaunchKernelGGL(k_trmv_finish, dim3((unsigned)((n * Dy + 255) / 256)), dim3(256), 0, st, partials, n, Dy,
                       nchunks, out, crows);
}

// ------------------------------------------------------------------------------------------------
// Row reductions of the sparse path over a resident chunk: s[i][d] = sum_j K[i][j] v[j][d] (= K(X, Z) woodbury_vector:
// dL_dm = V - s, var_dtc.py:148) and t[i] = sum_j K[i][j] T[i][j] (the per-point noise gradient, var_dtc.py:240-256).
__global__ __launch_bounds__(256) void k_rowdots(const double* __restrict__ K, const double* __restrict__ T, long ld,
                                                 long rows, long m, const double* __restrict__ v, int Dy,
                                                 double* __restrict__ out_s, double* __restrict__ t_out) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= rows) return;
    const double* kr = K + i * ld;
    double t = 0.0;
    if (t_out) {
        const double* tr = T + i * ld;
        for (long j = lane; j < m; j += 64) t = fma(kr[j], tr[j], t);
        for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off);
        if (lane == 0) t_out[i] = t;
    }
    if (out_s) {
        for (int d = 0; d < Dy; ++d) {
            double a = 0.0;
            for (long j = lane; j < m; j += 64) a = fma(kr[j], v[j * Dy + d], a);
            for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off);
            if (lane == 0) out_s[i * Dy + d] = a;
        }
    }
}
void launch_rowdots(hipStream_t st, const double* K, const double* T, long ld, long rows, long m, const double* v, int Dy,
                    double* out_s, double* t_out) {
    if (rows <= 0) return;
    hipLaunchKernelGGL(k_rowdots, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, K, T, ld, rows, m, v, Dy, out_s, t_out);
}

__global__ void k_rowscale_sqrt(const double* __restrict__ M, long ld, long rows, long cols, const double* __restrict__ w,
                                double* __restrict__ Out) {
    const long j = (long)blockIdx.y * blockDim.x + threadIdx.x, i = blockIdx.x;
    if (j >= cols || i >= rows) return;
    Out[i * ld + j] = M[i * ld + j] * sqrt(w[i]);
}
void launch_rowscale_sqrt(hipStream_t st, const double* M, long ld, long rows, long cols, const double* w, double* Out) {
    if (rows <= 0) return;
    hipLaunchKernelGGL(k_rowscale_sqrt, dim3((unsigned)rows, (unsigned)((cols + 255) / 256)), dim3(256), 0, st, M, ld, rows,
                       cols, w, Out);
}

// M[i][j] * s[i] (inverse: / s[i]) into Out (may alias M), rows x cols (ld shared): the signed form of launch_rowscale_sqrt
__global__ void k_rowscale(const double* __restrict__ M, long ld, long rows, long cols, const double* __restrict__ s, int inverse,
                           double* __restrict__ Out) {
    const long j = (long)blockIdx.y * blockDim.x + threadIdx.x, i = blockIdx.x;
    if (j >= cols || i >= rows) return;
    Out[i * ld + j] = inverse ? M[i * ld + j] / s[i] : M[i * ld + j] * s[i];
}
void launch_rowscale(hipStream_t st, const double* M, long ld, long rows, long cols, const double* s, int inverse, double* Out) {
    if (rows <= 0) return;
    hipLaunchKernelGGL(k_rowscale, dim3((unsigned)rows, (unsigned)((cols + 255) / 256)), dim3(256), 0, st, M, ld, rows, cols, s,
                       inverse, Out);
}
