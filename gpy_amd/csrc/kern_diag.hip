// kern_diag.hip -- the per-point diagonal of a kernel expression (add.py:74-79, prod.py:67-71, linear.py:84-85,100-105,
// coregionalize.py:106-107,145-151) over the
// rows of a resident row-major point set: kd_n = sum over terms of the product of the factors' diagonals at x_n, and for a
// weight vector w the sums that update_gradients_diag and the sparse bounds need.  One thread per row; a block's sums are
// reduced by a fixed tree, the blocks' records are added in block order by one more launch (no floating-point atomics).
#include "../../include/mi355gp.h"
#include "internal.h"

// fixed-tree sum of one value per thread; the result is valid in thread 0
__device__ __forceinline__ double kdiag_block_sum(double* red, int t, double v) {
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (t < k) red[t] += red[t + k];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(256) void k_kdiag_rows(DiagDesc ds, const double* __restrict__ X, long n, int D,
                                                    const double* __restrict__ coef, const double* __restrict__ w,
                                                    double* __restrict__ kd_out, double* __restrict__ partials) {
    __shared__ double sd[KDIAG_MAX_PARTS][256];        // the parts' diagonals at this thread's row
    __shared__ double red[256];
    const int t = threadIdx.x;
    const long i = (long)blockIdx.x * 256 + t;
    const bool valid = i < n;
    const double* x = X + (valid ? i : 0) * D;
    for (int p = 0; p < ds.nparts; ++p) {
        double d = ds.var[p];
        if (ds.by_point[p] == 1) {
            d = 0.0;
            for (int q = 0; q < D; ++q) d = fma(coef[p * D + q], x[q] * x[q], d);
        } else if (ds.by_point[p] == 2) {                // diag(B) at the row's output; an index outside [0, P) reads nothing: NaN
            const int a = coreg_idx(x[ds.ccol[p]], ds.cP[p]);
            d = a >= 0 ? coef[ds.nparts * D + p * KDIAG_MAX_OUT + a] : __builtin_nan("");
        }
        sd[p][t] = d;
    }
    double kd = 0.0;
    for (int tm = 0; tm < ds.nterms; ++tm) {
        double v = 1.0;
        for (int k = ds.tstart[tm]; k < ds.tstart[tm + 1]; ++k) v *= sd[ds.tpart[k]][t];
        kd += v;
    }
    if (kd_out && valid) kd_out[i] = kd;
    if (!w) return;                                      // (the same for every thread)
    const double wv = valid ? w[i] : 0.0;
    const int W = ds.width;
    double* rec = partials + (long)blockIdx.x * kdiag_slots(ds.nparts, W);
    double s = kdiag_block_sum(red, t, wv * kd);
    if (t == 0) rec[0] = s;
    s = kdiag_block_sum(red, t, wv * wv * kd);
    if (t == 0) rec[1] = s;
    for (int p = 0; p < ds.nparts; ++p) {
        double o = wv;                                   // the weight times the other factors of p's term
        const int tm = ds.tix[p];
        for (int k = ds.tstart[tm]; k < ds.tstart[tm + 1]; ++k)
            if (ds.tpart[k] != p) o *= sd[ds.tpart[k]][t];
        double* out = rec + 2 + p * W;
        if (!ds.by_point[p]) {
            s = kdiag_block_sum(red, t, o);
            if (t == 0) {
                out[0] = s;
                for (int q = 1; q < W; ++q) out[q] = 0.0;
            }
        } else if (ds.by_point[p] == 1) {
            for (int q = 0; q < D; ++q) {
                s = kdiag_block_sum(red, t, o * (x[q] * x[q]));
                if (t == 0) out[q] = s;
            }
            if (t == 0)
                for (int q = D; q < W; ++q) out[q] = 0.0;
        } else {
            // the per-output buckets (coregionalize.py:145-151): the rows of output a alone; a row whose index is no output
            // poisons bucket 0, as the bucketed gradient pass does
            const int P = ds.cP[p], a = coreg_idx(x[ds.ccol[p]], P);
            for (int q = 0; q < P; ++q) {
                double v = (a == q) ? o : 0.0;
                if (q == 0 && a < 0 && valid) v = __builtin_nan("");
                s = kdiag_block_sum(red, t, v);
                if (t == 0) out[q] = s;
            }
            if (t == 0)
                for (int q = P; q < W; ++q) out[q] = 0.0;
        }
    }
}

// out[s] = sum over the blocks, in block order, of partials[b][s]
__global__ void k_kdiag_combine(const double* __restrict__ partials, long nblk, int S, double* __restrict__ out) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    double a = 0.0;
    for (long b = 0; b < nblk; ++b) a += partials[b * S + s];
    out[s] = a;
}

// Gaussian rows q(x_n) = N(mu_n, diag S_n): the column sums a Linear part's psi0 = sum_q variance_q (mu_q^2 + S_q) and its
// psi2 need -- rec[q] = sum_n S_nq, rec[D + q] = sum_n mu_nq^2 -- one record of 2 D doubles per block, as above
__global__ __launch_bounds__(256) void k_kdiag_var_rows(const double* __restrict__ mu, const double* __restrict__ S, long n, int D,
                                                        double* __restrict__ partials) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    const long i = (long)blockIdx.x * 256 + t;
    const bool valid = i < n;
    double* rec = partials + (long)blockIdx.x * 2 * D;
    for (int q = 0; q < D; ++q) {
        const double sv = valid ? S[i * D + q] : 0.0, x = valid ? mu[i * D + q] : 0.0;
        double s = kdiag_block_sum(red, t, sv);
        if (t == 0) rec[q] = s;
        s = kdiag_block_sum(red, t, x * x);
        if (t == 0) rec[D + q] = s;
    }
}

void launch_kdiag_var_sums(hipStream_t st, const double* mu, const double* S, long n, int D, double* partials, double* sums_out) {
    const long nblk = kdiag_blocks(n);
    hipLaunchKernelGGL(k_kdiag_var_rows, dim3((unsigned)nblk), dim3(256), 0, st, mu, S, n, D, partials);
    hipLaunchKernelGGL(k_kdiag_combine, dim3((unsigned)((2 * D + 255) / 256)), dim3(256), 0, st, partials, nblk, 2 * D, sums_out);
}

void launch_kdiag(hipStream_t st, const DiagDesc& ds, const double* X, long n, int D, const double* coef, const double* w,
                  double* kd_out, double* partials, double* sums_out) {
    const long nblk = kdiag_blocks(n);
    hipLaunchKernelGGL(k_kdiag_rows, dim3((unsigned)nblk), dim3(256), 0, st, ds, X, n, D, coef, w, kd_out, partials);
    if (!w) return;
    const int S = kdiag_slots(ds.nparts, ds.width);
    hipLaunchKernelGGL(k_kdiag_combine, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, partials, nblk, S, sums_out);
}
