// kern_sparse.hip -- the streaming sparse path's covariance passes: K(X_chunk, Z) with the column reduction fused in
// (k_kbuild_cols), the gradient pass with the column reductions fused in (k_grad_cols, k_grad_cols_mfma; k_grad_cols_lin for a
// Linear part), and the column reductions over a resident chunk with their fixed-order combine (k_colreduce_multi, k_sum_splits).
#include <cstdint>
#include <cstdlib>

#include "../../include/mi355gp.h"
#include "internal.h"
#include "kern_tile.h"

// K(X_chunk, Z) of the streaming sparse path (var_dtc.py:123) WITH the column reduction psi1^T V = sum_i K[i][j] V[i][d]
// (var_dtc_parallel.py:91-116) fused in: block = (column tile, row split) as in k_grad_cols; the Z slab of the column tile is
// staged once per block, every 64 x 64 tile of K is stored as 32-byte row vectors and its contribution to the column sums stays
// in registers across the block's row tiles.  The separate pass re-read the whole 3.3 GB chunk for it (k_colreduce_multi: 0.58 ms
// at configuration 5).  One plain stationary part only (no accumulation, no product): sums of kernels keep the two-pass form.
// Partials [split][column][d] are combined in fixed order by launch_sum_splits: bit reproducible.
#define KBC_DY 4
__global__ __launch_bounds__(256) void k_kbuild_cols(KernParams kp, const double* __restrict__ Xt1, long ld1, long n,
                                                     const double* __restrict__ Xt2, long ld2, long m, double* __restrict__ out,
                                                     long ldo, const double* __restrict__ V, int Dy, int ntc, int ntr,
                                                     int tiles_per_split, double* __restrict__ colpart, long mcols) {
    __shared__ __attribute__((aligned(16))) double si[KDC * KT];
    __shared__ __attribute__((aligned(16))) double sj[KDC * KTJ];
    __shared__ double sv[KT * KBC_DY];
    __shared__ double red[256];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int tj = blockIdx.x % ntc, split = blockIdx.x / ntc;
    const long j0 = (long)tj * KT;
    const int D = kp.D;                                   // <= KDC
    double csum[4][KBC_DY];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int d = 0; d < KBC_DY; ++d) csum[b][d] = 0.0;
    stage_xj(Xt2, ld2, j0, 0, D, sj, t);
    const bool fullcols = j0 + KT <= m;
    const int ti_end = ((split + 1) * tiles_per_split < ntr) ? (split + 1) * tiles_per_split : ntr;
    for (int ti = split * tiles_per_split; ti < ti_end; ++ti) {
        const long i0 = (long)ti * KT;
        __syncthreads();                                  // the previous tile's reads of si / sv are done
        stage_x(Xt1, ld1, i0, 0, D, si, t);
        if (t < KT * Dy) {
            const long i = i0 + t / Dy;
            sv[(t / Dy) * KBC_DY + t % Dy] = (i < n) ? V[i * Dy + t % Dy] : 0.0;
        }
        __syncthreads();
        double r2[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) r2[a][b] = 0.0;
        accum_r2(si, sj, D, ty, tx, r2);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const long i = i0 + ty * 4 + a;
            d4 o;
#pragma unroll
            for (int b = 0; b < 4; ++b) o[b] = (i < n && j0 + tx * 4 + b < m) ? cov_k(kp.kind, kp.variance, r2[a][b], false) : 0.0;
            if (i < n) {
                if (fullcols) *reinterpret_cast<d4*>(out + i * ldo + j0 + tx * 4) = o;
                else
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if (j0 + tx * 4 + b < m) out[i * ldo + j0 + tx * 4 + b] = o[b];
            }
#pragma unroll
            for (int d = 0; d < KBC_DY; ++d) {
                if (d < Dy) {
                    const double v = sv[(ty * 4 + a) * KBC_DY + d];
#pragma unroll
                    for (int b = 0; b < 4; ++b) csum[b][d] = fma(o[b], v, csum[b][d]);
                }
            }
        }
    }
    // column partials of this block: over the 16 row groups (ty) in fixed order
    double* cp = colpart + (long)split * mcols * Dy;
#pragma unroll
    for (int d = 0; d < KBC_DY; ++d) {
        if (d < Dy) {
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                __syncthreads();
                red[ty * 16 + tx] = csum[b][d];
                __syncthreads();
                if (ty == 0) {
                    double sacc = 0.0;
                    for (int r = 0; r < 16; ++r) sacc += red[r * 16 + tx];
                    const long j = j0 + tx * 4 + b;
                    if (j < mcols) cp[j * Dy + d] = sacc;
                }
            }
        }
    }
}

// returns the number of row splits (colpart: nsplit * mcols * Dy doubles), 0 if the fused form does not apply
int launch_kbuild_cols(hipStream_t st, KernParams kp, const double* Xt1, long ld1, long n, const double* Xt2, long ld2, long m,
                       long mcols, double* Kout, long ldk, const double* V, int Dy, double* colpart) {
    if (kp.D > KDC || kp.kind > MI355GP_EXPONENTIAL || Dy > KBC_DY || Dy < 1 || ldk % 4 != 0 || ((uintptr_t)Kout & 31) != 0) return 0;
    const int ntr = (int)((n + KT - 1) / KT), ntc = (int)((mcols + KT - 1) / KT);
    int nsplit = 2048 / ntc;
    if (nsplit > 64) nsplit = 64;
    if (nsplit > ntr) nsplit = ntr;
    if (nsplit < 1) nsplit = 1;
    const int tps = (ntr + nsplit - 1) / nsplit;
    nsplit = (ntr + tps - 1) / tps;
    hipLaunchKernelGGL(k_kbuild_cols, dim3((unsigned)(ntc * nsplit)), dim3(256), 0, st, kp, Xt1, ld1, n, Xt2, ld2, m, Kout, ldk, V, Dy,
                       ntc, ntr, tps, colpart, mcols);
    return nsplit;
}


// ------------------------------------------------------------------------------------------------
// Gradient pass of the sparse path with the column reductions fused in (D <= 16): besides the theta partials of k_grad,
// every block accumulates  HX[j][c] = sum_i H[i][j] * x~[i][c]  (c < D) and the column sums of H (c = D) for its 64
// columns over ITS range of row tiles -- H = dL_dKnm * (dK/dr)/r never goes to memory (the separate pass wrote and
// re-read the 3.3 GB chunk).  Block = (column tile, row split); partial sums per split are combined in fixed order by
// launch_sum_splits, so the result stays bit-reproducible.  G: n x m weights, optionally formed on the fly (RankTerm).
#ifdef MI355GP_DIAG   // the VALU-only form (18 % of the issue rate at configuration 5): kept for A/B in the diagnostics build
template <bool ARD>
__global__ __launch_bounds__(256) void k_grad_cols(KernParams kp, const double* __restrict__ Xt1, long ld1, long n,
                                                   const double* __restrict__ Xt2, long ld2, long m,
                                                   const double* __restrict__ G, long ldg, RankTerm rk, int ntc,
                                                   int ntr, int tiles_per_split, double* __restrict__ partials,
                                                   double* __restrict__ colpart, long mcols, int nv) {
    constexpr int NVMAX = 17;
    __shared__ __attribute__((aligned(16))) double si[KDC * KT];
    __shared__ __attribute__((aligned(16))) double sj[KDC * KTJ];
    double* red = block_red();
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int tj = blockIdx.x % ntc, split = blockIdx.x / ntc;
    const long j0 = (long)tj * KT;
    const int D = kp.D;                                   // <= 16: one staging pass holds every dimension
    double a_var = 0.0, a_iso = 0.0;
    double a_q[NVMAX - 1];
    double hc[4][NVMAX];
#pragma unroll
    for (int q = 0; q < NVMAX - 1; ++q) a_q[q] = 0.0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int c = 0; c < NVMAX; ++c) hc[b][c] = 0.0;
    const int ti_end = ((split + 1) * tiles_per_split < ntr) ? (split + 1) * tiles_per_split : ntr;
    for (int ti = split * tiles_per_split; ti < ti_end; ++ti) {
        const long i0 = (long)ti * KT;
        double r2[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) r2[a][b] = 0.0;
        __syncthreads();
        stage_x(Xt1, ld1, i0, 0, D, si, t);
        stage_xj(Xt2, ld2, j0, 0, D, sj, t);
        __syncthreads();
        accum_r2(si, sj, D, ty, tx, r2);
        double gT[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const long i = i0 + ty * 4 + a;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const long j = j0 + tx * 4 + b;
                double g = 0.0;
                if (i < n && j < m) {
                    g = G[i * ldg + j];
                    if (rk.Y) {
                        double yv = 0.0;
                        for (int d = 0; d < rk.Dy; ++d) yv = fma(rk.Y[i * rk.Dy + d], rk.V[j * rk.Dy + d], yv);
                        g = fma(rk.gscale, g, rk.beta * yv);
                        if (rk.rowscale) g *= rk.rowscale[i];
                    }
                }
                const CovVal c = cov_all(kp.kind, kp.variance, r2[a][b], false);
                a_var = fma(g, c.k, a_var);
                if (!ARD) a_iso = fma(g, c.dk_r, a_iso);
                gT[a][b] = g * c.dk_or;
            }
        }
#pragma unroll
        for (int q = 0; q < NVMAX - 1; ++q) {
            if (q < D) {
                const d4 xi = *reinterpret_cast<const d4*>(si + q * KT + ty * 4);
                if (ARD) {
                    const d4 xj = ld_xj(sj, q, tx);
                    double sacc = 0.0;
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int b = 0; b < 4; ++b) {
                            const double d = xi[a] - xj[b];
                            sacc = fma(gT[a][b], d * d, sacc);
                        }
                    a_q[q] += sacc;
                }
#pragma unroll
                for (int b = 0; b < 4; ++b)
#pragma unroll
                    for (int a = 0; a < 4; ++a) hc[b][q] = fma(gT[a][b], xi[a], hc[b][q]);
            }
        }
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int a = 0; a < 4; ++a) hc[b][NVMAX - 1] += gT[a][b];     // column sums (the "ones" column, stored at c = D)
    }
    // theta partials of this block
    double* out = partials + (long)blockIdx.x * GP_STRIDE;
    const double sv = block_sum(t, a_var);
    if (t == 0) out[0] = sv;
    if (!ARD) {
        const double sl = block_sum(t, a_iso);
        if (t == 0) out[1] = sl;
    } else {
#pragma unroll
        for (int q = 0; q < NVMAX - 1; ++q) {
            if (q < D) {
                const double sq = block_sum(t, a_q[q]);
                if (t == 0) out[2 + q] = sq;
            }
        }
    }
    // column partials: sum over the 16 row groups (ty) in fixed order, one (b, c) pair at a time
    double* cp = colpart + (long)split * mcols * nv;
#pragma unroll
    for (int c = 0; c < NVMAX; ++c) {
        const int cdst = (c == NVMAX - 1) ? D : c;
        if (c < D || c == NVMAX - 1) {
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                __syncthreads();
                red[ty * 16 + tx] = hc[b][c];
                __syncthreads();
                if (ty == 0) {
                    double sacc = 0.0;
                    for (int r = 0; r < 16; ++r) sacc += red[r * 16 + tx];
                    const long j = j0 + tx * 4 + b;
                    if (j < mcols) cp[j * nv + cdst] = (j < m) ? sacc : 0.0;
                }
            }
        }
    }
}
#endif   // MI355GP_DIAG


// The same pass with the column reductions on the MATRIX pipe.  k_grad_cols keeps hc[4][17] per thread (136 VGPRs of accumulators:
// 256 VGPRs in all, ONE workgroup per CU, 18 % of the issue rate at configuration 5).  Here the tile H = dL_dKnm * (dK/dr)/r goes
// to LDS once and  HX[j][c] += sum_i H[i][j] x~[i][c]  is a 64 x 16 x 64 product per tile on v_mfma_f64_16x16x4 (wave w: columns
// 16 w .. 16 w + 15; A operand H^T from the LDS tile, B operand from a row-major copy of the x~ slab): 4 accumulator VGPR pairs
// instead of 68, no cross-thread reduction (every (j, c) lives in one lane) and the same fp64 pipe time as the FMAs it replaces
// (MFMA and VALU fp64 share the pipe) -- the gain is occupancy.  The column SUMS of H (the "ones" column) stay on the
// VALU (4 partial sums per thread, reduced once per block).  Rows in fixed order per block: bit reproducible.
#define GC_DY 4                                     // output columns the rank term keeps in registers (more: per-element loads)
#define GC_HS 80                                    // row stride (doubles) of the LDS H tile: rows 128 B apart in bank space
template <bool ARD>
__global__ __launch_bounds__(256, 2) void k_grad_cols_mfma(KernParams kp, const double* __restrict__ Xt1, long ld1, long n,
                                                           const double* __restrict__ Xt2, long ld2, long m,
                                                           const double* __restrict__ G, long ldg, RankTerm rk, int ntc,
                                                           int ntr, int tiles_per_split, double* __restrict__ partials,
                                                           double* __restrict__ colpart, long mcols, int nv) {
    constexpr int DM = 16;                               // D <= 16
    __shared__ __attribute__((aligned(16))) double si[DM * KT];
    __shared__ __attribute__((aligned(16))) double sj[DM * KTJ];
    __shared__ __attribute__((aligned(16))) double sit[KT * 18];   // x~ slab row-major [i][c], stride 18: the B operand
    __shared__ __attribute__((aligned(16))) double sh[KT * GC_HS];
    double* red = block_red();
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4, lane = t & 63, w = t >> 6;
    const int tj = blockIdx.x % ntc, split = blockIdx.x / ntc;
    const long j0 = (long)tj * KT;
    const int D = kp.D;
    double a_var = 0.0, a_iso = 0.0;
    double a_q[DM];
    double csum[4] = {0.0, 0.0, 0.0, 0.0};
    d4 hx = {0.0, 0.0, 0.0, 0.0};                        // HX[j = 16 w + (lane >> 4) + 4 r][c = lane & 15]
#pragma unroll
    for (int q = 0; q < DM; ++q) a_q[q] = 0.0;
    for (int idx = t; idx < KT * 18; idx += 256) sit[idx] = 0.0;      // columns c >= D stay zero
    // this thread's four columns: are all of them there (vector loads of the weights), and the rank term's column values
    const bool vec4 = (j0 + tx * 4 + 3 < m) && (ldg % 4 == 0) && ((reinterpret_cast<unsigned long long>(G) & 31ull) == 0);
    const bool rkfast = rk.Y != nullptr && rk.Dy <= GC_DY;
    double vcol[4][GC_DY];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int d = 0; d < GC_DY; ++d)
            vcol[b][d] = (rkfast && d < rk.Dy && j0 + tx * 4 + b < m) ? rk.V[(j0 + tx * 4 + b) * rk.Dy + d] : 0.0;
    const int ti_end = ((split + 1) * tiles_per_split < ntr) ? (split + 1) * tiles_per_split : ntr;
    for (int ti = split * tiles_per_split; ti < ti_end; ++ti) {
        const long i0 = (long)ti * KT;
        double r2[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) r2[a][b] = 0.0;
        __syncthreads();                                 // the previous tile's MFMA reads of sh / sit are done
        for (int idx = t; idx < D * KT; idx += 256) {
            const int q = idx >> 6, ii = idx & 63;
            const double v = Xt1[(long)q * ld1 + i0 + ii];
            si[q * KT + ii] = v;
            sit[ii * 18 + q] = v;
        }
        stage_xj(Xt2, ld2, j0, 0, D, sj, t);
        __syncthreads();
        accum_r2(si, sj, D, ty, tx, r2);
        double gT[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const long i = i0 + ty * 4 + a;
            // the weights of this row: one 32-byte load when the four columns exist (the scalar loads it replaces touched every
            // cache line four times), the rank term's row values once per row (they used to be fetched per element)
            d4 gv = {0.0, 0.0, 0.0, 0.0};
            double yrow[GC_DY], rs = 1.0;
            if (i < n) {
                if (vec4) gv = *reinterpret_cast<const d4*>(G + i * ldg + j0 + tx * 4);
                else
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if (j0 + tx * 4 + b < m) gv[b] = G[i * ldg + j0 + tx * 4 + b];
                if (rk.Y && rkfast) {
#pragma unroll
                    for (int d = 0; d < GC_DY; ++d) yrow[d] = (d < rk.Dy) ? rk.Y[i * rk.Dy + d] : 0.0;
                    if (rk.rowscale) rs = rk.rowscale[i];
                }
            }
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const long j = j0 + tx * 4 + b;
                double g = 0.0;
                if (i < n && j < m) {
                    g = gv[b];
                    if (rk.Y) {
                        double yv = 0.0;
                        if (rkfast) {
#pragma unroll
                            for (int d = 0; d < GC_DY; ++d)
                                if (d < rk.Dy) yv = fma(yrow[d], vcol[b][d], yv);
                        } else {
                            for (int d = 0; d < rk.Dy; ++d) yv = fma(rk.Y[i * rk.Dy + d], rk.V[j * rk.Dy + d], yv);
                        }
                        g = fma(rk.gscale, g, rk.beta * yv);
                        if (rk.rowscale) g *= rkfast ? rs : rk.rowscale[i];
                    }
                }
                const CovVal c = cov_all(kp.kind, kp.variance, r2[a][b], false);
                a_var = fma(g, c.k, a_var);
                if (!ARD) a_iso = fma(g, c.dk_r, a_iso);
                gT[a][b] = g * c.dk_or;
                csum[b] += gT[a][b];
            }
            *reinterpret_cast<d4*>(sh + (ty * 4 + a) * GC_HS + tx * 4) = (d4){gT[a][0], gT[a][1], gT[a][2], gT[a][3]};
        }
        if (ARD) {
#pragma unroll
            for (int q = 0; q < DM; ++q) {
                if (q < D) {
                    const d4 xi = *reinterpret_cast<const d4*>(si + q * KT + ty * 4);
                    const d4 xj = ld_xj(sj, q, tx);
                    double sacc = 0.0;
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int b = 0; b < 4; ++b) {
                            const double d = xi[a] - xj[b];
                            sacc = fma(gT[a][b], d * d, sacc);
                        }
                    a_q[q] += sacc;
                }
            }
        }
        __syncthreads();                                 // the H tile is complete
        // HX[16 w .., :] += H[:, 16 w ..]^T x~ : k = 4 s + (lane >> 4) over the 64 rows of the tile
        const double* ha = sh + (lane >> 4) * GC_HS + 16 * w + (lane & 15);
        const double* xb = sit + (lane >> 4) * 18 + (lane & 15);
#pragma unroll
        for (int s4 = 0; s4 < 16; ++s4) hx = mfma_f64(ha[4 * s4 * GC_HS], xb[4 * s4 * 18], hx);
    }
    // theta partials of this block
    double* out = partials + (long)blockIdx.x * GP_STRIDE;
    const double sv = block_sum(t, a_var);
    if (t == 0) out[0] = sv;
    if (!ARD) {
        const double sl = block_sum(t, a_iso);
        if (t == 0) out[1] = sl;
    } else {
#pragma unroll
        for (int q = 0; q < DM; ++q) {
            if (q < D) {
                const double sq = block_sum(t, a_q[q]);
                if (t == 0) out[2 + q] = sq;
            }
        }
    }
    double* cp = colpart + (long)split * mcols * nv;
    // HX: every (j, c) is one accumulator register
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long j = j0 + 16 * w + (lane >> 4) + 4 * r;
        const int c = lane & 15;
        if (c < D && j < mcols) cp[j * nv + c] = (j < m) ? hx[r] : 0.0;
    }
    // column sums of H: over the 16 row groups (ty) in fixed order
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        __syncthreads();
        red[ty * 16 + tx] = csum[b];
        __syncthreads();
        if (ty == 0) {
            double sacc = 0.0;
            for (int r = 0; r < 16; ++r) sacc += red[r * 16 + tx];
            const long j = j0 + tx * 4 + b;
            if (j < mcols) cp[j * nv + D] = (j < m) ? sacc : 0.0;
        }
    }
}

// returns the number of row splits (colpart holds nsplit * mcols * (D+1) doubles, partials ntc*nsplit blocks); 0 if the
// fused form does not apply (D > 16)
int launch_grad_cols(hipStream_t st, KernParams kp, const double* Xt1, long ld1, long n, const double* Xt2, long ld2,
                     long m, long mcols, const double* G, long ldg, RankTerm rk, double* partials, double* colpart,
                     int* nblocks_out) {
    if (kp.D > 16) return 0;
    const int ntr = (int)((n + KT - 1) / KT), ntc = (int)((mcols + KT - 1) / KT);
    int nsplit = 2048 / ntc;
    if (nsplit > 64) nsplit = 64;
    if (nsplit > ntr) nsplit = ntr;
    if (nsplit < 1) nsplit = 1;
    const int tps = (ntr + nsplit - 1) / nsplit;
    nsplit = (ntr + tps - 1) / tps;
    const int nb = ntc * nsplit;
    static const int use_mfma = [] { const char* e = DIAG_ENV("GRAD_COLS_MFMA"); return (e && *e) ? atoi(e) : 1; }();
    if (use_mfma) {
        if (kp.ard)
            hipLaunchKernelGGL((k_grad_cols_mfma<true>), dim3(nb), dim3(256), 0, st, kp, Xt1, ld1, n, Xt2, ld2, m, G, ldg, rk, ntc,
                               ntr, tps, partials, colpart, mcols, kp.D + 1);
        else
            hipLaunchKernelGGL((k_grad_cols_mfma<false>), dim3(nb), dim3(256), 0, st, kp, Xt1, ld1, n, Xt2, ld2, m, G, ldg, rk, ntc,
                               ntr, tps, partials, colpart, mcols, kp.D + 1);
        *nblocks_out = nb;
        return nsplit;
    }
#ifdef MI355GP_DIAG
    if (kp.ard)
        hipLaunchKernelGGL((k_grad_cols<true>), dim3(nb), dim3(256), 0, st, kp, Xt1, ld1, n, Xt2, ld2, m, G, ldg, rk, ntc, ntr,
                           tps, partials, colpart, mcols, kp.D + 1);
    else
        hipLaunchKernelGGL((k_grad_cols<false>), dim3(nb), dim3(256), 0, st, kp, Xt1, ld1, n, Xt2, ld2, m, G, ldg, rk, ntc, ntr,
                           tps, partials, colpart, mcols, kp.D + 1);
#endif
    *nblocks_out = nb;
    return nsplit;
}

// ------------------------------------------------------------------------------------------------
// The pass for a term that is exactly one stationary factor times one Coregionalize factor (what util.multioutput.ICM builds;
// D <= 16, P <= 16): k_grad_cols_mfma with the lookup B[a_i][b_j] folded in.  The product route (sparse_rows_gradients) builds
// the other factor's covariance, multiplies dL_dKnm up in memory, runs the gradient kernel with H written and the column
// reduction, per factor: about eight passes over a chunk x M array.  Here the chunk's rows of W are read once, dL_dKnm is
// formed on the fly from the RankTerm (rowscale included: MixedNoise gives per-point precisions) and nothing of chunk x M is
// written.  From ONE evaluation of c = cov_all(r^2) per element:
//   the stationary factor's theta record from  g B[a][b] c            (a_var, a_iso / a_q as in k_grad_cols_mfma),
//   HX = H^T [x~ | 1] with H = g B[a][b] c.dk_or                      (v_mfma_f64_16x16x4, the ones column on the VALU),
//   the Coregionalize factor's buckets  S[a][b] += g c.k              (the weights of update_gradients_full: dL_dK times the
//                                                                      OTHER factor's covariance, prod.py:86-99).
// B lives in LDS; the tile's row and column output indices are read from the Coregionalize part's own scaled copies (Ct1 / Ct2:
// they hold the index column alone) into LDS as integers, with the masks of the outputs present.  Per tile and present pair
// (a, b), in a fixed order, every thread sums its matching elements and a fixed wave / block tree adds them into the block's LDS
// record, as k_grad_coreg does: rows sorted by output give ONE pair, one block reduction, in nearly every tile; a tile with
// many pairs is right all the same.  The block's S goes to spart + block * P * P (combine: launch_reduce_partials, block order).
// An index that is no output never reads outside B: its elements count as NaN and the block's record is poisoned.
// LDS: k_grad_cols_mfma's 68.6 KB (si 8, sj 9, sit 9, sh 40, red 2) + B 2 KB + S 2 KB + two index arrays 0.5 KB = 73 KB: two
// workgroups per CU (160 KB) as that kernel has; __launch_bounds__(256, 2) holds the registers to the same budget.
template <bool ARD>
__global__ __launch_bounds__(256, 2) void k_grad_cols_icm(KernParams kp, KernParams kc, const double* __restrict__ Xt1, long ld1, long n,
                                                          const double* __restrict__ Xt2, long ld2, long m,
                                                          const double* __restrict__ Ct1, long ldc1,
                                                          const double* __restrict__ Ct2, long ldc2,
                                                          const double* __restrict__ G, long ldg, RankTerm rk, int ntc, int ntr,
                                                          int tiles_per_split, double* __restrict__ partials,
                                                          double* __restrict__ colpart, long mcols, int nv,
                                                          double* __restrict__ spart) {
    constexpr int DM = 16;                               // D <= 16
    __shared__ __attribute__((aligned(16))) double si[DM * KT];
    __shared__ __attribute__((aligned(16))) double sj[DM * KTJ];
    __shared__ __attribute__((aligned(16))) double sit[KT * 18];   // x~ slab row-major [i][c], stride 18: the B operand
    __shared__ __attribute__((aligned(16))) double sh[KT * GC_HS];
    __shared__ double sB[COREG_PMAX * COREG_PMAX], sacc[COREG_PMAX * COREG_PMAX];
    __shared__ int sa[KT], sb[KT];
    __shared__ unsigned smask[2];
    __shared__ double redS[4];
    double* red = block_red();
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4, lane = t & 63, w = t >> 6;
    const int tj = blockIdx.x % ntc, split = blockIdx.x / ntc;
    const long j0 = (long)tj * KT;
    const int D = kp.D, P = kc.ard;
    double a_var = 0.0, a_iso = 0.0;
    double a_q[DM];
    double csum[4] = {0.0, 0.0, 0.0, 0.0};
    d4 hx = {0.0, 0.0, 0.0, 0.0};                        // HX[j = 16 w + (lane >> 4) + 4 r][c = lane & 15]
    bool poisoned = false;                               // (thread 0) an index outside [0, P) was met
#pragma unroll
    for (int q = 0; q < DM; ++q) a_q[q] = 0.0;
    for (int idx = t; idx < KT * 18; idx += 256) sit[idx] = 0.0;      // columns c >= D stay zero
    for (int k = t; k < P * P; k += 256) {
        sB[k] = kc.pw[k];
        sacc[k] = 0.0;
    }
    if (w == 1) {                                        // the column tile's outputs: the same for every row tile of this block
        const long j = j0 + lane;
        int v = -2;                                      // -2: padding (no element), -1: an invalid index
        if (j < m) v = coreg_idx(Ct2[(long)kc.col * ldc2 + j], P);
        unsigned bit = (v >= 0) ? (1u << v) : (v == -1 ? (1u << COREG_PMAX) : 0u);
        for (int off = 32; off > 0; off >>= 1) bit |= (unsigned)__shfl_xor((int)bit, off);
        sb[lane] = v;
        if (lane == 0) smask[1] = bit;
    }
    const bool vec4 = (j0 + tx * 4 + 3 < m) && (ldg % 4 == 0) && ((reinterpret_cast<unsigned long long>(G) & 31ull) == 0);
    const bool rkfast = rk.Y != nullptr && rk.Dy <= GC_DY;
    double vcol[4][GC_DY];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int d = 0; d < GC_DY; ++d)
            vcol[b][d] = (rkfast && d < rk.Dy && j0 + tx * 4 + b < m) ? rk.V[(j0 + tx * 4 + b) * rk.Dy + d] : 0.0;
    const int ti_end = ((split + 1) * tiles_per_split < ntr) ? (split + 1) * tiles_per_split : ntr;
    for (int ti = split * tiles_per_split; ti < ti_end; ++ti) {
        const long i0 = (long)ti * KT;
        double r2[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) r2[a][b] = 0.0;
        __syncthreads();                                 // the previous tile's reads of sh / sit / sa / smask are done
        for (int idx = t; idx < D * KT; idx += 256) {
            const int q = idx >> 6, ii = idx & 63;
            const double v = Xt1[(long)q * ld1 + i0 + ii];
            si[q * KT + ii] = v;
            sit[ii * 18 + q] = v;
        }
        stage_xj(Xt2, ld2, j0, 0, D, sj, t);
        if (w == 0) {                                    // the row tile's outputs
            const long i = i0 + lane;
            int v = -2;
            if (i < n) v = coreg_idx(Ct1[(long)kc.col * ldc1 + i], P);
            unsigned bit = (v >= 0) ? (1u << v) : (v == -1 ? (1u << COREG_PMAX) : 0u);
            for (int off = 32; off > 0; off >>= 1) bit |= (unsigned)__shfl_xor((int)bit, off);
            sa[lane] = v;
            if (lane == 0) smask[0] = bit;
        }
        __syncthreads();
        accum_r2(si, sj, D, ty, tx, r2);
        const unsigned rm = smask[0], cm = smask[1];
        if (t == 0 && ((rm | cm) >> COREG_PMAX)) poisoned = true;
        int ra[4], cb[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) ra[a] = sa[ty * 4 + a];
#pragma unroll
        for (int b = 0; b < 4; ++b) cb[b] = sb[tx * 4 + b];
        double gT[4][4], sw[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const long i = i0 + ty * 4 + a;
            d4 gv = {0.0, 0.0, 0.0, 0.0};
            double yrow[GC_DY], rs = 1.0;
            if (i < n) {
                if (vec4) gv = *reinterpret_cast<const d4*>(G + i * ldg + j0 + tx * 4);
                else
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if (j0 + tx * 4 + b < m) gv[b] = G[i * ldg + j0 + tx * 4 + b];
                if (rk.Y && rkfast) {
#pragma unroll
                    for (int d = 0; d < GC_DY; ++d) yrow[d] = (d < rk.Dy) ? rk.Y[i * rk.Dy + d] : 0.0;
                    if (rk.rowscale) rs = rk.rowscale[i];
                }
            }
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const long j = j0 + tx * 4 + b;
                double g = 0.0, bij = 0.0;
                if (i < n && j < m) {
                    g = gv[b];
                    if (rk.Y) {
                        double yv = 0.0;
                        if (rkfast) {
#pragma unroll
                            for (int d = 0; d < GC_DY; ++d)
                                if (d < rk.Dy) yv = fma(yrow[d], vcol[b][d], yv);
                        } else {
                            for (int d = 0; d < rk.Dy; ++d) yv = fma(rk.Y[i * rk.Dy + d], rk.V[j * rk.Dy + d], yv);
                        }
                        g = fma(rk.gscale, g, rk.beta * yv);
                        if (rk.rowscale) g *= rkfast ? rs : rk.rowscale[i];
                    }
                    bij = (ra[a] >= 0 && cb[b] >= 0) ? sB[ra[a] * P + cb[b]] : __builtin_nan("");
                }
                const CovVal c = cov_all(kp.kind, kp.variance, r2[a][b], false);
                const double gb = g * bij;               // the weight the stationary factor sees (prod.py:86-99)
                sw[a][b] = g * c.k;                      // ... and the one the Coregionalize factor sees
                a_var = fma(gb, c.k, a_var);
                if (!ARD) a_iso = fma(gb, c.dk_r, a_iso);
                gT[a][b] = gb * c.dk_or;
                csum[b] += gT[a][b];
            }
            *reinterpret_cast<d4*>(sh + (ty * 4 + a) * GC_HS + tx * 4) = (d4){gT[a][0], gT[a][1], gT[a][2], gT[a][3]};
        }
        if (ARD) {
#pragma unroll
            for (int q = 0; q < DM; ++q) {
                if (q < D) {
                    const d4 xi = *reinterpret_cast<const d4*>(si + q * KT + ty * 4);
                    const d4 xj = ld_xj(sj, q, tx);
                    double sacc_q = 0.0;
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int b = 0; b < 4; ++b) {
                            const double d = xi[a] - xj[b];
                            sacc_q = fma(gT[a][b], d * d, sacc_q);
                        }
                    a_q[q] += sacc_q;
                }
            }
        }
        __syncthreads();                                 // the H tile is complete
        const double* ha = sh + (lane >> 4) * GC_HS + 16 * w + (lane & 15);
        const double* xb = sit + (lane >> 4) * 18 + (lane & 15);
#pragma unroll
        for (int s4 = 0; s4 < 16; ++s4) hx = mfma_f64(ha[4 * s4 * GC_HS], xb[4 * s4 * 18], hx);
        // the buckets: every present pair in a fixed order (the masks are the block's: the loop is uniform)
        for (unsigned rmm = rm & ((1u << COREG_PMAX) - 1); rmm; rmm &= rmm - 1) {
            const int pa = __ffs(rmm) - 1;
            for (unsigned cmm = cm & ((1u << COREG_PMAX) - 1); cmm; cmm &= cmm - 1) {
                const int pb = __ffs(cmm) - 1;
                double v = 0.0;
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if (ra[a] == pa && cb[b] == pb) v += sw[a][b];
                for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
                if (lane == 0) redS[w] = v;
                __syncthreads();
                if (t == 0) sacc[pa * P + pb] += (redS[0] + redS[1]) + (redS[2] + redS[3]);
                __syncthreads();
            }
        }
    }
    // theta partials of this block
    double* out = partials + (long)blockIdx.x * GP_STRIDE;
    const double sv = block_sum(t, a_var);
    if (t == 0) out[0] = sv;
    if (!ARD) {
        const double sl = block_sum(t, a_iso);
        if (t == 0) out[1] = sl;
    } else {
#pragma unroll
        for (int q = 0; q < DM; ++q) {
            if (q < D) {
                const double sq = block_sum(t, a_q[q]);
                if (t == 0) out[2 + q] = sq;
            }
        }
    }
    double* cp = colpart + (long)split * mcols * nv;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long j = j0 + 16 * w + (lane >> 4) + 4 * r;
        const int c = lane & 15;
        if (c < D && j < mcols) cp[j * nv + c] = (j < m) ? hx[r] : 0.0;
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        __syncthreads();
        red[ty * 16 + tx] = csum[b];
        __syncthreads();
        if (ty == 0) {
            double sacc_c = 0.0;
            for (int r = 0; r < 16; ++r) sacc_c += red[r * 16 + tx];
            const long j = j0 + tx * 4 + b;
            if (j < mcols) cp[j * nv + D] = (j < m) ? sacc_c : 0.0;
        }
    }
    __syncthreads();
    if (t == 0 && poisoned) sacc[0] = __builtin_nan("");
    __syncthreads();
    double* so = spart + (long)blockIdx.x * P * P;
    for (int k = t; k < P * P; k += 256) so[k] = sacc[k];
}

// Whether the pass applies (the one list of its conditions: the caller asks before it decides on a route) ...
// ... and the launch: returns the number of row splits (0, with nothing launched, where it does not apply); *nblocks_out <= 2048
// blocks have written a GP_STRIDE record to partials and a P x P record to spart, colpart holds nsplit * mcols * (D + 1) doubles
bool grad_cols_icm_applies(int D, int P, long mcols) {
    return D <= 16 && P >= 1 && P <= COREG_PMAX && (mcols + KT - 1) / KT <= 2048;      // (spart and partials hold 2048 block records)
}
int launch_grad_cols_icm(hipStream_t st, KernParams kp, KernParams kc, const double* Xt1, long ld1, long n, const double* Xt2, long ld2,
                         long m, long mcols, const double* Ct1, long ldc1, const double* Ct2, long ldc2, const double* G, long ldg,
                         RankTerm rk, double* partials, double* colpart, double* spart, int* nblocks_out) {
    if (!grad_cols_icm_applies(kp.D, kc.ard, mcols)) return 0;
    const int ntr = (int)((n + KT - 1) / KT), ntc = (int)((mcols + KT - 1) / KT);
    int nsplit = 2048 / ntc;
    if (nsplit > 64) nsplit = 64;
    if (nsplit > ntr) nsplit = ntr;
    if (nsplit < 1) nsplit = 1;
    const int tps = (ntr + nsplit - 1) / nsplit;
    nsplit = (ntr + tps - 1) / tps;
    const int nb = ntc * nsplit;
    if (kp.ard)
        hipLaunchKernelGGL((k_grad_cols_icm<true>), dim3(nb), dim3(256), 0, st, kp, kc, Xt1, ld1, n, Xt2, ld2, m, Ct1, ldc1, Ct2, ldc2, G,
                           ldg, rk, ntc, ntr, tps, partials, colpart, mcols, kp.D + 1, spart);
    else
        hipLaunchKernelGGL((k_grad_cols_icm<false>), dim3(nb), dim3(256), 0, st, kp, kc, Xt1, ld1, n, Xt2, ld2, m, Ct1, ldc1, Ct2, ldc2, G,
                           ldg, rk, ntc, ntr, tps, partials, colpart, mcols, kp.D + 1, spart);
    *nblocks_out = nb;
    return nsplit;
}

// The pass for a Linear part (kind 9, linear.py:87-114; D <= 16).  K = sum_q x~_iq z~_jq with x~ = sqrt(variance_q) x, so the whole
// row-side gradient is the skinny product  HX[j][q] = sum_i g[i][j] x~[i][q]  of the weights themselves: dL/dvariance_q =
// sum_j z~_jq HX[j][q] / variance_q and dL/dZ_jq = sqrt(variance_q) HX[j][q], both finished on the host from HX and the scaled Z.
// No covariance is evaluated, the Z slab is not staged and there is no ones column.  Block = (column tile, row split), the
// weights formed on the fly and the 64 x 16 x 64 product per tile on v_mfma_f64_16x16x4 exactly as in k_grad_cols_mfma (the
// weight formation is that kernel's, repeated here so that its code stays as measured).
__global__ __launch_bounds__(256, 2) void k_grad_cols_lin(const double* __restrict__ Xt1, long ld1, long n, int D, long m,
                                                          const double* __restrict__ G, long ldg, RankTerm rk, int ntc, int ntr,
                                                          int tiles_per_split, double* __restrict__ colpart, long mcols) {
    __shared__ __attribute__((aligned(16))) double sit[KT * 18];   // x~ slab row-major [i][c], stride 18: the B operand
    __shared__ __attribute__((aligned(16))) double sh[KT * GC_HS];  // the tile of weights: the A operand
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4, lane = t & 63, w = t >> 6;
    const int tj = blockIdx.x % ntc, split = blockIdx.x / ntc;
    const long j0 = (long)tj * KT;
    d4 hx = {0.0, 0.0, 0.0, 0.0};                        // HX[j = 16 w + (lane >> 4) + 4 r][c = lane & 15]
    for (int idx = t; idx < KT * 18; idx += 256) sit[idx] = 0.0;      // columns c >= D stay zero
    const bool vec4 = (j0 + tx * 4 + 3 < m) && (ldg % 4 == 0) && ((reinterpret_cast<unsigned long long>(G) & 31ull) == 0);
    const bool rkfast = rk.Y != nullptr && rk.Dy <= GC_DY;
    double vcol[4][GC_DY];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int d = 0; d < GC_DY; ++d)
            vcol[b][d] = (rkfast && d < rk.Dy && j0 + tx * 4 + b < m) ? rk.V[(j0 + tx * 4 + b) * rk.Dy + d] : 0.0;
    const int ti_end = ((split + 1) * tiles_per_split < ntr) ? (split + 1) * tiles_per_split : ntr;
    for (int ti = split * tiles_per_split; ti < ti_end; ++ti) {
        const long i0 = (long)ti * KT;
        __syncthreads();                                 // the previous tile's MFMA reads of sh / sit are done
        for (int idx = t; idx < D * KT; idx += 256) {
            const int q = idx >> 6, ii = idx & 63;
            sit[ii * 18 + q] = Xt1[(long)q * ld1 + i0 + ii];
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const long i = i0 + ty * 4 + a;
            d4 gv = {0.0, 0.0, 0.0, 0.0};
            double yrow[GC_DY], rs = 1.0;
            if (i < n) {
                if (vec4) gv = *reinterpret_cast<const d4*>(G + i * ldg + j0 + tx * 4);
                else
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if (j0 + tx * 4 + b < m) gv[b] = G[i * ldg + j0 + tx * 4 + b];
                if (rk.Y && rkfast) {
#pragma unroll
                    for (int d = 0; d < GC_DY; ++d) yrow[d] = (d < rk.Dy) ? rk.Y[i * rk.Dy + d] : 0.0;
                    if (rk.rowscale) rs = rk.rowscale[i];
                }
            }
            d4 go = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const long j = j0 + tx * 4 + b;
                double g = 0.0;
                if (i < n && j < m) {
                    g = gv[b];
                    if (rk.Y) {
                        double yv = 0.0;
                        if (rkfast) {
#pragma unroll
                            for (int d = 0; d < GC_DY; ++d)
                                if (d < rk.Dy) yv = fma(yrow[d], vcol[b][d], yv);
                        } else {
                            for (int d = 0; d < rk.Dy; ++d) yv = fma(rk.Y[i * rk.Dy + d], rk.V[j * rk.Dy + d], yv);
                        }
                        g = fma(rk.gscale, g, rk.beta * yv);
                        if (rk.rowscale) g *= rkfast ? rs : rk.rowscale[i];
                    }
                }
                go[b] = g;
            }
            *reinterpret_cast<d4*>(sh + (ty * 4 + a) * GC_HS + tx * 4) = go;
        }
        __syncthreads();                                 // the tile of weights and the x~ slab are complete
        // HX[16 w .., :] += g[:, 16 w ..]^T x~ : k = 4 s + (lane >> 4) over the 64 rows of the tile
        const double* ha = sh + (lane >> 4) * GC_HS + 16 * w + (lane & 15);
        const double* xb = sit + (lane >> 4) * 18 + (lane & 15);
#pragma unroll
        for (int s4 = 0; s4 < 16; ++s4) hx = mfma_f64(ha[4 * s4 * GC_HS], xb[4 * s4 * 18], hx);
    }
    double* cp = colpart + (long)split * mcols * D;      // every (j, c) is one accumulator register
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long j = j0 + 16 * w + (lane >> 4) + 4 * r;
        const int c = lane & 15;
        if (c < D && j < mcols) cp[j * D + c] = (j < m) ? hx[r] : 0.0;
    }
}

int launch_grad_cols_lin(hipStream_t st, const double* Xt1, long ld1, long n, int D, long m, long mcols, const double* G, long ldg,
                         RankTerm rk, double* colpart) {
    if (D > 16) return 0;
    const int ntr = (int)((n + KT - 1) / KT), ntc = (int)((mcols + KT - 1) / KT);
    int nsplit = 2048 / ntc;                             // the splits of launch_grad_cols
    if (nsplit > 64) nsplit = 64;
    if (nsplit > ntr) nsplit = ntr;
    if (nsplit < 1) nsplit = 1;
    const int tps = (ntr + nsplit - 1) / nsplit;
    nsplit = (ntr + tps - 1) / tps;
    hipLaunchKernelGGL(k_grad_cols_lin, dim3((unsigned)(ntc * nsplit)), dim3(256), 0, st, Xt1, ld1, n, D, m, G, ldg, rk, ntc, ntr, tps,
                       colpart, mcols);
    return nsplit;
}

// The row-side counterpart for a Linear part under uncertain inputs (D <= 16): the gradient with respect to the rows themselves,
//   out[i][q] = il_q (sum_j g[i][j] z~[j][q] + c0 x~[i][q]),     il_q = sqrt(variance_q), z~ = il z, x~ = il x,
// which is d/dmu_iq of sum g K(mu, Z) + (c0 / 2) sum_i Kdiag(mu_i): the tall-skinny product (rows x m) (m x D).  A workgroup owns
// 64 rows and walks the column tiles in order; the weights are formed on the fly exactly as k_grad_cols_lin forms them (no
// rows x m array is written), the z~ slab of the tile is staged in LDS (zero past m and past D) and every wave multiplies its
// 16 rows on v_mfma_f64_16x16x4.  One accumulator per output, summed over j in a fixed order: no atomics, the same bytes on
// every call.  The kernel reads the chunk's weights once and is bound by that read.
__global__ __launch_bounds__(256, 2) void k_grad_rows_lin(const double* __restrict__ Xt1, long ld1, long n, int D,
                                                          const double* __restrict__ Xt2, long ld2, long m,
                                                          const double* __restrict__ G, long ldg, RankTerm rk,
                                                          const double* __restrict__ il, double c0, double* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) double szt[KT * 18];   // z~ slab row-major [j][c], stride 18: the B operand
    __shared__ __attribute__((aligned(16))) double sh[KT * GC_HS];  // the tile of weights [i][j]: the A operand
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4, lane = t & 63, w = t >> 6;
    const long i0 = (long)blockIdx.x * KT;
    const int ntc = (int)((m + KT - 1) / KT);
    d4 acc = {0.0, 0.0, 0.0, 0.0};                       // out[i = i0 + 16 w + (lane >> 4) + 4 r][c = lane & 15]
    for (int idx = t; idx < KT * 18; idx += 256) szt[idx] = 0.0;      // columns c >= D stay zero
    const bool rkfast = rk.Y != nullptr && rk.Dy <= GC_DY;
    double yrow[4][GC_DY], rs[4];                        // the block's rows do not change: their rank-term rows once
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const long i = i0 + ty * 4 + a;
        rs[a] = 1.0;
#pragma unroll
        for (int d = 0; d < GC_DY; ++d) yrow[a][d] = (rkfast && i < n && d < rk.Dy) ? rk.Y[i * rk.Dy + d] : 0.0;
        if (rkfast && i < n && rk.rowscale) rs[a] = rk.rowscale[i];
    }
    for (int tj = 0; tj < ntc; ++tj) {
        const long j0 = (long)tj * KT;
        __syncthreads();                                 // the previous tile's MFMA reads of sh / szt are done
        for (int idx = t; idx < D * KT; idx += 256) {
            const int q = idx >> 6, jj = idx & 63;
            szt[jj * 18 + q] = (j0 + jj < m) ? Xt2[(long)q * ld2 + j0 + jj] : 0.0;
        }
        const bool vec4 = (j0 + tx * 4 + 3 < m) && (ldg % 4 == 0) && ((reinterpret_cast<unsigned long long>(G) & 31ull) == 0);
        double vcol[4][GC_DY];
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int d = 0; d < GC_DY; ++d)
                vcol[b][d] = (rkfast && d < rk.Dy && j0 + tx * 4 + b < m) ? rk.V[(j0 + tx * 4 + b) * rk.Dy + d] : 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const long i = i0 + ty * 4 + a;
            d4 gv = {0.0, 0.0, 0.0, 0.0};
            if (i < n) {
                if (vec4) gv = *reinterpret_cast<const d4*>(G + i * ldg + j0 + tx * 4);
                else
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if (j0 + tx * 4 + b < m) gv[b] = G[i * ldg + j0 + tx * 4 + b];
            }
            d4 go = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const long j = j0 + tx * 4 + b;
                double g = 0.0;
                if (i < n && j < m) {
                    g = gv[b];
                    if (rk.Y) {
                        double yv = 0.0;
                        if (rkfast) {
#pragma unroll
                            for (int d = 0; d < GC_DY; ++d)
                                if (d < rk.Dy) yv = fma(yrow[a][d], vcol[b][d], yv);
                        } else {
                            for (int d = 0; d < rk.Dy; ++d) yv = fma(rk.Y[i * rk.Dy + d], rk.V[j * rk.Dy + d], yv);
                        }
                        g = fma(rk.gscale, g, rk.beta * yv);
                        if (rk.rowscale) g *= rkfast ? rs[a] : rk.rowscale[i];
                    }
                }
                go[b] = g;
            }
            *reinterpret_cast<d4*>(sh + (ty * 4 + a) * GC_HS + tx * 4) = go;
        }
        __syncthreads();                                 // the tile of weights and the z~ slab are complete
        // out[16 w .., :] += g[16 w .., :] z~ : k = 4 s + (lane >> 4) over the 64 columns of the tile
        const double* ha = sh + (16 * w + (lane & 15)) * GC_HS + (lane >> 4);
        const double* zb = szt + (lane >> 4) * 18 + (lane & 15);
#pragma unroll
        for (int s4 = 0; s4 < 16; ++s4) acc = mfma_f64(ha[4 * s4], zb[4 * s4 * 18], acc);
    }
    const int c = lane & 15;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long i = i0 + 16 * w + (lane >> 4) + 4 * r;
        if (c < D && i < n) out[i * D + c] = il[c] * fma(c0, Xt1[(long)c * ld1 + i], acc[r]);
    }
}

// the same from weights in memory (any D up to 64; the fallback of the fused kernel, as on the column side): one thread per
// output, j in order
__global__ __launch_bounds__(256) void k_rows_lin_plain(const double* __restrict__ Xt1, long ld1, long n, int D,
                                                        const double* __restrict__ Xt2, long ld2, long m,
                                                        const double* __restrict__ g, long ldg, const double* __restrict__ il,
                                                        double c0, double* __restrict__ out) {
    const int q = threadIdx.x & 63;
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n || q >= D) return;
    double a = 0.0;
    for (long j = 0; j < m; ++j) a = fma(g[i * ldg + j], Xt2[(long)q * ld2 + j], a);
    out[i * D + q] = il[q] * fma(c0, Xt1[(long)q * ld1 + i], a);
}

int launch_grad_rows_lin(hipStream_t st, const double* Xt1, long ld1, long n, int D, const double* Xt2, long ld2, long m,
                         const double* G, long ldg, RankTerm rk, const double* il, double c0, double* out) {
    if (D > 16) return 0;
    hipLaunchKernelGGL(k_grad_rows_lin, dim3((unsigned)((n + KT - 1) / KT)), dim3(256), 0, st, Xt1, ld1, n, D, Xt2, ld2, m, G, ldg, rk,
                       il, c0, out);
    return 1;
}
void launch_rows_lin_plain(hipStream_t st, const double* Xt1, long ld1, long n, int D, const double* Xt2, long ld2, long m,
                           const double* g, long ldg, const double* il, double c0, double* out) {
    hipLaunchKernelGGL(k_rows_lin_plain, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, Xt1, ld1, n, D, Xt2, ld2, m, g, ldg, il, c0,
                       out);
}

// out[i][j] = rowscale_i (gscale G[i][j] + beta sum_d Y[i][d] V[j][d]) for j < m, 0 for m <= j < ld: the weights of a RankTerm in
// memory, in the arithmetic of the fused passes
__global__ void k_form_rank_weights(const double* __restrict__ G, long ld, long rows, long m, RankTerm rk, double* __restrict__ out) {
    const long j = (long)blockIdx.y * blockDim.x + threadIdx.x, i = blockIdx.x;
    if (j >= ld || i >= rows) return;
    double g = 0.0;
    if (j < m) {
        double yv = 0.0;
        for (int d = 0; d < rk.Dy; ++d) yv = fma(rk.Y[i * rk.Dy + d], rk.V[j * rk.Dy + d], yv);
        g = fma(rk.gscale, G[i * ld + j], rk.beta * yv);
        if (rk.rowscale) g *= rk.rowscale[i];
    }
    out[i * ld + j] = g;
}
void launch_form_rank_weights(hipStream_t st, const double* G, long ld, long rows, long m, RankTerm rk, double* out) {
    hipLaunchKernelGGL(k_form_rank_weights, dim3((unsigned)rows, (unsigned)((ld + 255) / 256)), dim3(256), 0, st, G, ld, rows, m, rk, out);
}

// out[j][c] = sum_i M[i][j] * V(i, c), c < nv <= 33.  V(i, c) = V[i*sr + c*sc] for c < nvt, 1 for c == nvt (the column
// sums): sr = 1, sc = ld for a dimension-major input, sr = Dy, sc = 1 for a row-major (rows x Dy) one.  One thread per column, 4 row groups per block, optional row split over blockIdx.y with a
// fixed-order combine by the caller (partials [split][cols][nv]).
template <int NV>
__global__ __launch_bounds__(256) void k_colreduce_multi(const double* __restrict__ M, long ld, long rows, long cols,
                                                         const double* __restrict__ V, long sr, long sc, int nvt,
                                                         int nv, double* __restrict__ part, int nv_total, int c_off) {
    __shared__ double sv[NV][256];
    __shared__ double red[4][64];
    const int tx = threadIdx.x & 63, g = threadIdx.x >> 6;
    const long j = (long)blockIdx.x * 64 + tx;
    const long rs = (rows + gridDim.y - 1) / gridDim.y;
    const long r0 = (long)blockIdx.y * rs, r1 = (r0 + rs < rows) ? r0 + rs : rows;
    double acc[NV];
#pragma unroll
    for (int c = 0; c < NV; ++c) acc[c] = 0.0;
    for (long ib = r0; ib < r1; ib += 256) {
        __syncthreads();
        for (int c = 0; c < nv; ++c) {
            const long i = ib + threadIdx.x;
            sv[c][threadIdx.x] = (i < r1) ? ((c < nvt) ? V[i * sr + (long)c * sc] : 1.0) : 0.0;
        }
        __syncthreads();
        const long iend = (ib + 256 < r1) ? 256 : (r1 - ib);
        if (j < cols) {
            for (long ii = g; ii < iend; ii += 4) {
                const double x = M[(ib + ii) * ld + j];
#pragma unroll
                for (int c = 0; c < NV; ++c)
                    if (c < nv) acc[c] = fma(x, sv[c][ii], acc[c]);
            }
        }
    }
    double* out = part + ((long)blockIdx.y * cols) * nv_total + c_off;   // this launch fills columns [c_off, c_off + nv) of nv_total
#pragma unroll
    for (int c = 0; c < NV; ++c) {
        if (c >= nv) break;
        __syncthreads();
        red[g][tx] = acc[c];
        __syncthreads();
        if (g == 0 && j < cols) out[j * nv_total + c] = (red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx]);
    }
}

// part must hold nsplit * cols * nv doubles (nv = nvt + ones); returns nsplit.  More than 32 V columns (input dimension
// D > 32 in gradients_X / the sparse path's dL/dZ, stationary.py:330-358 has no such limit) run as several launches of at
// most 32 columns each that fill their own column range of the same [split][cols][nv] partials; the all-ones column rides
// with the last one.
int launch_colreduce_multi(hipStream_t st, const double* M, long ld, long rows, long cols, const double* V, long sr,
                           long sc, int nvt, int ones, double* part) {
    const int nv_total = nvt + (ones ? 1 : 0);
    // 64 columns per block: the row split supplies the parallelism (>= 2048 blocks for a 32k x 2k panel)
    int nsplit = (int)((rows + 511) / 512);
    if (nsplit < 1) nsplit = 1;
    if (nsplit > 64) nsplit = 64;
    const dim3 grid((unsigned)((cols + 63) / 64), (unsigned)nsplit);
    int c0 = 0;
    do {
        const int nvc = nvt - c0 < 32 ? nvt - c0 : 32;                 // V columns of this launch
        const bool lastc = c0 + nvc >= nvt;
        const int nv = nvc + ((lastc && ones) ? 1 : 0);                // <= 33
        const double* Vc = V + (long)c0 * sc;
        if (nv <= 9)
            hipLaunchKernelGGL((k_colreduce_multi<9>), grid, dim3(256), 0, st, M, ld, rows, cols, Vc, sr, sc, nvc, nv, part, nv_total, c0);
        else if (nv <= 17)
            hipLaunchKernelGGL((k_colreduce_multi<17>), grid, dim3(256), 0, st, M, ld, rows, cols, Vc, sr, sc, nvc, nv, part, nv_total, c0);
        else
            hipLaunchKernelGGL((k_colreduce_multi<33>), grid, dim3(256), 0, st, M, ld, rows, cols, Vc, sr, sc, nvc, nv, part, nv_total, c0);
        c0 += nvc;
    } while (c0 < nvt);
    return nsplit;
}

// dst[i] (+)= sum_s src[s*cnt + i]  (fixed order)
__global__ void k_sum_splits(const double* __restrict__ src, long cnt, int nsplit, int accumulate,
                             double* __restrict__ dst) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cnt) return;
    double s = accumulate ? dst[i] : 0.0;
    for (int k = 0; k < nsplit; ++k) s += src[(long)k * cnt + i];
    dst[i] = s;
}
void launch_sum_splits(hipStream_t st, const double* src, long cnt, int nsplit, int accumulate, double* dst) {
    hipLaunchKernelGGL(k_sum_splits, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, src, cnt, nsplit, accumulate,
                       dst);
}
