// kern.hip -- covariance assembly (Stationary.K), the fused dL/dK -> dL/dtheta reduction
// (Stationary.update_gradients_full), the alpha products and the fetch helpers.
// Reference: GPy/kern/src/stationary.py:105-168,193-243; rbf.py:51-52,177-178; stationary.py:382-386,
// 488-492,585-589; stationary_cython.pyx:53-62; inference/.../exact_gaussian_inference.py:55-72.
//
// These stages are HBM-bound (8 N^2 bytes written by the build, 4 N^2 read by the gradient pass over the
// lower triangle of Ky^-1): inputs are pre-scaled by 1/lengthscale and stored dimension-major so a 64-point
// slab of every dimension is one coalesced 512-byte read, X tiles live in LDS, and K is recomputed from X
// inside the gradient pass instead of being re-read from memory.
#include <cstdint>
#include <cstdlib>

#include "../../include/mi355gp.h"
#include "grad_policy.h"
#include "internal.h"

#define KT 64      // covariance tile edge
#define KDC 32     // input dimensions staged per LDS chunk

struct CovVal {
    double k;        // K(r)
    double dk_r;     // dK/dr * r
    double dk_or;    // dK/dr / r   (0 where r == 0 for the exponential kernel)
};

// kinds 4 / 5 are the static kernels of GPy/kern/src/static.py: White (variance on coinciding points of the symmetric
// case, :77-81) and Bias (constant, :165-167); `same` = the entry is a diagonal entry of a symmetric evaluation.
__device__ __forceinline__ double cov_k(int kind, double var, double r2, bool same = false) {
    if (kind == MI355GP_WHITE) return same ? var : 0.0;
    if (kind == MI355GP_BIAS) return var;
    if (kind == MI355GP_RBF) return var * exp(-0.5 * r2);
    const double r = sqrt(r2);
    if (kind == MI355GP_MATERN52) {
        const double s5r = 2.2360679774997896964 * r;
        return var * (1.0 + s5r + (5.0 / 3.0) * r2) * exp(-s5r);
    }
    if (kind == MI355GP_MATERN32) {
        const double s3r = 1.7320508075688772935 * r;
        return var * (1.0 + s3r) * exp(-s3r);
    }
    return var * exp(-r);
}

__device__ __forceinline__ CovVal cov_all(int kind, double var, double r2, bool same = false) {
    CovVal c;
    if (kind >= MI355GP_WHITE) {
        c.k = (kind == MI355GP_BIAS || same) ? var : 0.0;
        c.dk_r = 0.0;
        c.dk_or = 0.0;
        return c;
    }
    if (kind == MI355GP_RBF) {
        c.k = var * exp(-0.5 * r2);
        c.dk_r = -r2 * c.k;
        c.dk_or = -c.k;
        return c;
    }
    const double r = sqrt(r2);
    if (kind == MI355GP_MATERN52) {
        const double s5r = 2.2360679774997896964 * r;
        const double e = var * exp(-s5r);
        c.k = (1.0 + s5r + (5.0 / 3.0) * r2) * e;
        c.dk_or = -(5.0 / 3.0) * (1.0 + s5r) * e;
        c.dk_r = c.dk_or * r2;
        return c;
    }
    if (kind == MI355GP_MATERN32) {
        const double s3r = 1.7320508075688772935 * r;
        const double e = var * exp(-s3r);
        c.k = (1.0 + s3r) * e;
        c.dk_or = -3.0 * e;
        c.dk_r = c.dk_or * r2;
        return c;
    }
    c.k = var * exp(-r);
    c.dk_r = -r * c.k;
    c.dk_or = (r != 0.0) ? -c.k / r : 0.0;
    return c;
}

// ------------------------------------------------------------------------------------------------
// Xt[q][i] = X[i][q] / l_q, zero for i in [n, ldx)
__global__ void k_scale_inputs(const double* __restrict__ X, long n, int D, const double* __restrict__ inv_ls,
                               int ard, double* __restrict__ Xt, long ldx) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)D * ldx) return;
    const int q = (int)(idx / ldx);
    const long i = idx - (long)q * ldx;
    Xt[idx] = (i < n) ? X[i * D + q] * inv_ls[ard ? q : 0] : 0.0;
}

void launch_scale_inputs(hipStream_t st, const double* X, long n, int D, const double* inv_ls, int ard,
                         double* Xt, long ldx) {
    const long total = (long)D * ldx;
    hipLaunchKernelGGL(k_scale_inputs, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, X, n, D, inv_ls,
                       ard, Xt, ldx);
}

// Stage rows [i0, i0+64) of dims [q0, q0+qc) of a dimension-major input into LDS s[q][64].
__device__ __forceinline__ void stage_x(const double* __restrict__ Xt, long ldx, long i0, int q0, int qc,
                                        double* s, int t) {
    for (int idx = t; idx < qc * KT; idx += 256) {
        const int q = idx >> 6, ii = idx & 63;
        s[q * KT + ii] = Xt[(long)(q0 + q) * ldx + i0 + ii];
    }
}

// The COLUMN-side slab is stored permuted with rows of KTJ doubles: element ii = 4 tx + b of dimension q sits at
// q KTJ + 40 (b >> 1) + 2 tx + (b & 1).  A thread's four values are then two 16-byte reads whose 16 lanes of a ds_read_b128
// lane group cover 256 contiguous bytes: conflict-free.  In the natural layout (4 tx + b) the two reads of a lane are 32 bytes
// apart and lanes tx, tx + 8 of a group land on the same banks (2-way on every read of the slab: the 28 % of LDS cycles that
// SQ_LDS_BANK_CONFLICT showed for k_grad / k_kbuild).  The offset of the second half (40, not 32) keeps the 64-bit stores of
// the staging pass conflict-free as well (ds_write_b64: groups of 16 consecutive lanes, banks modulo 32 dwords).
#define KTJ 72
__device__ __forceinline__ int xj_pos(int ii) { return 40 * ((ii >> 1) & 1) + 2 * (ii >> 2) + (ii & 1); }
__device__ __forceinline__ void stage_xj(const double* __restrict__ Xt, long ldx, long i0, int q0, int qc, double* s, int t) {
    for (int idx = t; idx < qc * KT; idx += 256) {
        const int q = idx >> 6, ii = idx & 63;
        s[q * KTJ + xj_pos(ii)] = Xt[(long)(q0 + q) * ldx + i0 + ii];
    }
}
__device__ __forceinline__ d4 ld_xj(const double* sj, int q, int tx) {
    const d2 lo = *reinterpret_cast<const d2*>(sj + q * KTJ + 2 * tx);
    const d2 hi = *reinterpret_cast<const d2*>(sj + q * KTJ + 40 + 2 * tx);
    return d4{lo[0], lo[1], hi[0], hi[1]};
}

// r2[a][b] += sum_q (xi[q][ty*4+a] - xj[q][tx*4+b])^2
__device__ __forceinline__ void accum_r2(const double* si, const double* sj, int qc, int ty, int tx,
                                         double (&r2)[4][4]) {
    for (int q = 0; q < qc; ++q) {
        const d4 xi = *reinterpret_cast<const d4*>(si + q * KT + ty * 4);
        const d4 xj = ld_xj(sj, q, tx);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const double d = xi[a] - xj[b];
                r2[a][b] = fma(d, d, r2[a][b]);
            }
    }
}

// ------------------------------------------------------------------------------------------------
// Covariance assembly.  SYM: Ky = K + diag(noise + jit) into the padded npad x npad buffer (identity in the
// padding), optionally lower 64-tiles only.  !SYM: rectangular K(X1, X2) into a dense n x m buffer.
// Every kind has a kernel of its own (k_kbuild below for the stationary and static kinds, the others in their sections
// further down) that holds only what is the kind's: what it stages, what it accumulates over the staged slabs, how an
// element follows from the sums.  The rest is one skeleton of inlined helpers: kbuild_tile, stage_chunk, kbuild_pad
// and kbuild_store_row.  Inlining keeps every instantiation's code to what its kind needs.
struct KbuildArgs {
    KernParams kp;
    const double* Xt1;                 // row side: dimension-major inputs [D][ld1], n points
    long ld1, n;
    const double* Xt2;                 // column side, m points
    long ld2, m;
    double* out;
    long ldo, nrows_out;
    const double* noise;
    long noise_len;
    double jit;
    int lower_only, add_diag, ntc, accumulate;
    int diag_same;                     // the stationary kernel only (White): a rectangular evaluation of coinciding points
    const double* mul;                 // (may alias out): element-wise multiplier with out's layout -- product kernels
                                       // (GPy/kern/src/prod.py:58-65)
};

// The origin of this block's tile; false: nothing to do (an upper tile of a lower_only build)
template <bool SYM>
__device__ __forceinline__ bool kbuild_tile(const KbuildArgs& A, long& i0, long& j0) {
    const long ti = blockIdx.x / A.ntc, tj = blockIdx.x % A.ntc;
    i0 = ti * KT;
    j0 = tj * KT;
    return !(SYM && A.lower_only && tj > ti);
}

__device__ __forceinline__ void zero_tile(double (&s)[4][4]) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) s[a][b] = 0.0;
}

// Chunk q0 of the dimensions: both slabs of the tile at (i0, j0) go to LDS between two barriers.  Returns the number of
// dimensions staged; the kind's accumulate step over them follows.
__device__ __forceinline__ int stage_chunk(int D, int q0, const double* __restrict__ Xt1, long ld1, long i0,
                                           const double* __restrict__ Xt2, long ld2, long j0, double* si, double* sj, int t) {
    const int qc = (D - q0 < KDC) ? (D - q0) : KDC;
    __syncthreads();
    stage_x(Xt1, ld1, i0, q0, qc, si, t);
    stage_xj(Xt2, ld2, j0, q0, qc, sj, t);
    __syncthreads();
    return qc;
}

// what an element outside n x m holds: the identity in the padding of a fresh symmetric build, nothing otherwise
template <bool SYM>
__device__ __forceinline__ double kbuild_pad(const KbuildArgs& A, long i, long j) {
    return (SYM && i == j && !A.accumulate) ? 1.0 : 0.0;
}

// Row i of a thread's 4 x 4 elements, v[b] = element (i, j0 + tx * 4 + b), goes out: times mul, plus noise + jitter on the
// diagonal, plus what is there (accumulate); one 32-byte store into the padded symmetric buffer, scalar stores otherwise.
template <bool SYM>
__device__ __forceinline__ void kbuild_store_row(const KbuildArgs& A, long i, long j0, int tx, const double (&v)[4]) {
    if (SYM) {
        if (i < A.nrows_out) {
            d4* p = reinterpret_cast<d4*>(A.out + i * A.ldo + j0 + tx * 4);
            d4 o = (d4){v[0], v[1], v[2], v[3]};
            if (A.mul) o *= *reinterpret_cast<const d4*>(A.mul + i * A.ldo + j0 + tx * 4);
            if (A.add_diag && i < A.n) {                      // noise + jitter enter once, outside any product
                const long d = i - (j0 + tx * 4);
                if (d >= 0 && d < 4) o[d] += A.noise[A.noise_len > 1 ? i : 0] + A.jit;
            }
            if (A.accumulate) o += *p;                       // sum kernels (GPy/kern/src/add.py:58-72): K += K_part
            *p = o;
        }
    } else if (i < A.n) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const long j = j0 + tx * 4 + b;
            if (j < A.m) {
                const double w = A.mul ? v[b] * A.mul[i * A.ldo + j] : v[b];
                A.out[i * A.ldo + j] = A.accumulate ? A.out[i * A.ldo + j] + w : w;
            }
        }
    }
}

// The stationary kinds and the static ones.  White puts its variance on coinciding points: the diagonal of a symmetric
// build, and of a rectangular one that says so (diag_same).  The one kernel that takes KbuildArgs' fields as parameters of
// its own: `__restrict__` on them is worth a wait less in the epilogue of the kernel that the benchmark times.
template <bool SYM>
__global__ __launch_bounds__(256) void k_kbuild(KernParams kp, const double* __restrict__ Xt1, long ld1, long n,
                                                const double* __restrict__ Xt2, long ld2, long m,
                                                double* __restrict__ out, long ldo, long nrows_out,
                                                const double* __restrict__ noise, long noise_len, double jit,
                                                int lower_only, int add_diag, int ntc, int accumulate, int diag_same,
                                                const double* mul) {
    const KbuildArgs A{kp,    Xt1,        ld1,      n,   Xt2,        ld2,       m,  out, ldo, nrows_out, noise, noise_len,
                       jit,   lower_only, add_diag, ntc, accumulate, diag_same, mul};
    __shared__ __attribute__((aligned(16))) double si[KDC * KT];
    __shared__ __attribute__((aligned(16))) double sj[KDC * KTJ];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    long i0, j0;
    if (!kbuild_tile<SYM>(A, i0, j0)) return;
    double r2[4][4];
    zero_tile(r2);
    if (i0 < A.n && j0 < A.m)
        for (int q0 = 0; q0 < A.kp.D; q0 += KDC)
            accum_r2(si, sj, stage_chunk(A.kp.D, q0, A.Xt1, A.ld1, i0, A.Xt2, A.ld2, j0, si, sj, t), ty, tx, r2);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const long i = i0 + ty * 4 + a;
        double v[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const long j = j0 + tx * 4 + b;
            if (i < A.n && j < A.m) v[b] = cov_k(A.kp.kind, A.kp.variance, r2[a][b], (SYM || A.diag_same) && i == j);
            else v[b] = kbuild_pad<SYM>(A, i, j);
        }
        kbuild_store_row<SYM>(A, i, j0, tx, v);
    }
}



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
// Gradient reduction.  For every (i, j): g = weight * dL_dK[i][j];
//   acc_var += g*K ; acc_iso += g*(dK/dr*r) ; acc_q += g*(dK/dr / r)*(x~_iq - x~_jq)^2   (x~ = x / l)
// FUSED: dL_dK = 0.5*(alpha_i . alpha_j - Dy*W_ij) from the lower triangle of W (off-diagonal weight 2).
// else : dL_dK read from G (n x m).
// Per-block partials [2 + 32]: [0] var, [1] iso, [2+q] lengthscale dims q_off..q_off+31.
// As for the assembly, every kind has a kernel of its own (k_grad below, the others in their sections) around shared inlined
// pieces: grad_tile, stage_chunk / restage, grad_weight, store_h and block_sum.

// Tile `tile` of a pass: FUSED walks the lower triangle row by row, else every tile of ntc tile columns
template <bool FUSED>
__device__ __forceinline__ void grad_tile(long tile, int ntc, long& ti, long& tj) {
    if (FUSED) {   // lower-triangular enumeration
        ti = (long)((sqrt(8.0 * (double)tile + 1.0) - 1.0) * 0.5);
        while (ti * (ti + 1) / 2 > tile) --ti;
        while ((ti + 1) * (ti + 2) / 2 <= tile) ++ti;
        tj = tile - ti * (ti + 1) / 2;
    } else {
        ti = tile / ntc;
        tj = tile - ti * ntc;
    }
}

// D > 32: bring the qcnt dimensions from q_off, the ones this launch reduces, back into LDS unless they are what is there
__device__ __forceinline__ void restage(int last_q0, int q_off, int qcnt, const double* __restrict__ Xt1, long ld1, long i0,
                                        const double* __restrict__ Xt2, long ld2, long j0, double* si, double* sj, int t) {
    if (last_q0 != q_off) {
        __syncthreads();
        stage_x(Xt1, ld1, i0, q_off, qcnt, si, t);
        stage_xj(Xt2, ld2, j0, q_off, qcnt, sj, t);
        __syncthreads();
    }
}

// The weight dL_dK of element (i, j), 0 outside n x m.
//   FUSED: 0.5 (sc * alpha_i . alpha_j - Dy * W_ij) from the lower triangle of W = Ky^-1 (G), j <= i only; sc = 1 for the Gaussian
//          process, (nu+N)/(nu+beta-2) for the Student-t process (exact_studentt_inference.py:46).  With TWICE an element below
//          the diagonal counts for its mirror image as well.
//   else : G[i][j].
//   Mul  : factor of a product kernel -- dL_dK times the other factors' covariances (prod.py:86-99).  !TWICE (Coregionalize, which
//          completes symmetrically on its own) takes it on the elements j <= i of the fused form alone.
template <bool FUSED, bool TWICE>
__device__ __forceinline__ double grad_weight(long i, long j, long n, long m, const double* __restrict__ G, long ldg,
                                              const double* __restrict__ alpha, int Dy, double sc,
                                              const double* __restrict__ Mul, long ldm) {
    double g = 0.0;
    if (i < n && j < m) {
        if (FUSED) {
            if (j <= i) {
                double aa = 0.0;
                for (int d = 0; d < Dy; ++d) aa = fma(alpha[i * Dy + d], alpha[j * Dy + d], aa);
                g = 0.5 * (sc * aa - (double)Dy * G[i * ldg + j]);
                if (TWICE) {
                    if (j < i) g *= 2.0;
                } else if (Mul) {
                    g *= Mul[i * ldm + j];
                }
            }
        } else {
            g = G[i * ldg + j];
        }
        if (TWICE && Mul) g *= Mul[i * ldm + j];
    }
    return g;
}

// A weight of the gradients_X reductions goes out: Hout[i][j] = h inside n x m.  MASKED: 0 where key == 0 -- for
// H = dL_dK * (dK/dr)/r (stationary.py:330-346) and key = r^2 that is `_inv_dist` (:225-232): a coincident pair gives
// exactly nothing, not x H - H x to rounding.
template <bool MASKED>
__device__ __forceinline__ void store_h(double* __restrict__ Hout, long ldh, long i, long j, long n, long m, double key, double h) {
    if (i < n && j < m) Hout[i * ldh + j] = (MASKED && key == 0.0) ? 0.0 : h;
}

// 256 doubles of LDS: block_sum's scratch, free for a kernel's own fixed-order reductions between two calls
__device__ __forceinline__ double* block_red() {
    __shared__ double red[256];
    return red;
}

// deterministic sum of v over the block's 256 threads
__device__ __forceinline__ double block_sum(int t, double v) {
    double* red = block_red();
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    return red[0];
}

template <bool FUSED, bool ARD>
__global__ __launch_bounds__(256) void k_grad(KernParams kp, const double* __restrict__ Xt1, long ld1, long n,
                                              const double* __restrict__ Xt2, long ld2, long m,
                                              const double* __restrict__ G, long ldg,
                                              const double* __restrict__ alpha, int Dy, int q_off,
                                              long ntiles, int ntc, double* __restrict__ partials,
                                              double* __restrict__ Hout = nullptr, long ldh = 0, int diag_same = 0,
                                              const double* __restrict__ aa_scale = nullptr,
                                              const double* __restrict__ Mul = nullptr, long ldm = 0,
                                              RankTerm rk = RankTerm{nullptr, nullptr, 0, 0.0, 1.0, nullptr}) {
    __shared__ __attribute__((aligned(16))) double si[KDC * KT];
    __shared__ __attribute__((aligned(16))) double sj[KDC * KTJ];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    double a_var = 0.0, a_iso = 0.0;
    double a_q[KDC];
#pragma unroll
    for (int q = 0; q < KDC; ++q) a_q[q] = 0.0;
    const int qcnt = ARD ? ((kp.D - q_off < KDC) ? (kp.D - q_off) : KDC) : 0;
    const double sc = (FUSED && aa_scale) ? aa_scale[0] : 1.0;

    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        long ti, tj;
        grad_tile<FUSED>(tile, ntc, ti, tj);
        const long i0 = ti * KT, j0 = tj * KT;
        double r2[4][4];
        zero_tile(r2);
        int last_q0 = -1;
        for (int q0 = 0; q0 < kp.D; last_q0 = q0, q0 += KDC)
            accum_r2(si, sj, stage_chunk(kp.D, q0, Xt1, ld1, i0, Xt2, ld2, j0, si, sj, t), ty, tx, r2);
        // weights * dL_dK, then the covariance factors
        double gT[4][4];   // g * dK/dr / r
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const long i = i0 + ty * 4 + a;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const long j = j0 + tx * 4 + b;
                double g = 0.0;   // grad_weight<FUSED, true> with the rank term, spelt out: see there
                if (i < n && j < m) {
                    if (FUSED) {
                        if (j <= i) {
                            double aa = 0.0;
                            for (int d = 0; d < Dy; ++d) aa = fma(alpha[i * Dy + d], alpha[j * Dy + d], aa);
                            g = 0.5 * (sc * aa - (double)Dy * G[i * ldg + j]);
                            if (j < i) g *= 2.0;
                        }
                    } else {
                        g = G[i * ldg + j];
                        if (rk.Y) {   // dL_dKnm = gscale * G + beta * Y v^T formed on the fly (var_dtc.py:219,233)
                            double yv = 0.0;
                            for (int d = 0; d < rk.Dy; ++d) yv = fma(rk.Y[i * rk.Dy + d], rk.V[j * rk.Dy + d], yv);
                            g = fma(rk.gscale, g, rk.beta * yv);
                            if (rk.rowscale) g *= rk.rowscale[i];   // per-point precision (var_dtc.py:224-226)
                        }
                    }
                    if (Mul) g *= Mul[i * ldm + j];
                }
                const CovVal c = cov_all(kp.kind, kp.variance, r2[a][b], (FUSED || diag_same) && i == j);
                a_var = fma(g, c.k, a_var);
                if (!ARD) a_iso = fma(g, c.dk_r, a_iso);
                gT[a][b] = g * c.dk_or;
            }
        }
        if (!FUSED && Hout) {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) store_h<true>(Hout, ldh, i0 + ty * 4 + a, j0 + tx * 4 + b, n, m, r2[a][b], gT[a][b]);
        }
        if (ARD) {
            restage(last_q0, q_off, qcnt, Xt1, ld1, i0, Xt2, ld2, j0, si, sj, t);
#pragma unroll
            for (int q = 0; q < KDC; ++q) {
                if (q < qcnt) {
                    const d4 xi = *reinterpret_cast<const d4*>(si + q * KT + ty * 4);
                    const d4 xj = ld_xj(sj, q, tx);
                    double s = 0.0;
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int b = 0; b < 4; ++b) {
                            const double d = xi[a] - xj[b];
                            s = fma(gT[a][b], d * d, s);
                        }
                    a_q[q] += s;
                }
            }
        }
    }
    // deterministic block reduction -> partials[blockIdx][...]
    double* out = partials + (long)blockIdx.x * GP_STRIDE;
    const double sv = block_sum(t, a_var);
    if (t == 0) out[0] = sv;
    if (!ARD) {
        const double sl = block_sum(t, a_iso);
        if (t == 0) out[1] = sl;
    } else {
#pragma unroll
        for (int q = 0; q < KDC; ++q) {
            if (q < qcnt) {
                const double sq = block_sum(t, a_q[q]);
                if (t == 0) out[2 + q] = sq;
            }
        }
    }
}

// k_grad<true, true> of the plain stationary kinds with less fp64 issue per tile (grad_policy.h says which launches take it).
//   * Interior tiles (strictly below the diagonal, all 64 rows inside n) need no bounds or triangle test: alpha is read once per
//     thread row and column, the weights of a thread row are ONE 32-byte load, every element counts twice.  Diagonal and edge tiles
//     form their weights as k_grad does.
//   * r^2, K and the variance sum keep k_grad's direct form (x~_i - x~_j)^2: exact zeros for duplicates.
//   * The per-dimension reduction  a_q += sum_ij T_ij (x~_iq - x~_jq)^2,  T = g (dK/dr)/r  (48 fp64 instructions per thread and
//     dimension as sub + mul + fma per pair), is expanded about a per-tile centre c_q = x~_{j0,q}, u = x~_i - c, v = x~_j - c:
//         sum_i u_iq (u_iq R_i - 2 P_iq) + sum_j v_jq^2 C_j,    R = row sums of T, C = column sums, P = T V  (64 x 64 x qpad)
//     with P on v_mfma_f64_16x16x4: wave w owns rows 16 w .. 16 w + 15 (its four ty), q in blocks of 16, 32 MFMAs per tile and wave
//     at D = 32.  T reaches the A operand through a per-wave LDS scratch, one of the thread's four columns at a time (16 columns:
//     8.5 KB for the block); MFMA row m reads scratch row 4 (m & 3) + (m >> 2), so that accumulator register r of lane (ty, tx) is
//     P[4 ty + r][16 qb + tx]: the thread's OWN rows, and R needs no more than the sum over the 16 lanes of a row group.  The centring
//     is applied as the operands leave LDS (the slabs stay as the r^2 pass needs them: one staging), so u, v are differences of
//     points of ONE tile and the expansion cancels at the tile's spread, not at the data's offset from the origin.
//   * Two accumulators per lane (q = tx, 16 + tx) replace a_q[32]; every sum runs in a fixed order: bit reproducible.
//   * The kind is a template parameter: 167 VGPRs and three waves per SIMD without a spill (254 with the kind at run time).
// Slab row strides 66 / 74 (not 64 / 72): lanes that differ in q (the MFMA's B operand, the u and v reads) fall on different banks.
// LDS: 16.5 + 18.5 + 8.5 + 2 + 2 = 47.5 KB, three blocks per CU.
#define TG_SI 66
#define TG_SJ 74
#define TG_AS 17
__device__ __forceinline__ int tg_stage(int D, int q0, const double* __restrict__ Xt, long ldx, long i0, long j0, double* si,
                                        double* sj, int t) {
    const int qc = (D - q0 < KDC) ? (D - q0) : KDC;
    const int qpad = (qc + 15) & ~15;                    // dimensions up to the next multiple of 16 are zeros: the MFMA's q blocks
    __syncthreads();
    for (int idx = t; idx < qpad * KT; idx += 256) {
        const int q = idx >> 6, ii = idx & 63;
        const bool in = q < qc;
        si[q * TG_SI + ii] = in ? Xt[(long)(q0 + q) * ldx + i0 + ii] : 0.0;
        sj[q * TG_SJ + xj_pos(ii)] = in ? Xt[(long)(q0 + q) * ldx + j0 + ii] : 0.0;
    }
    __syncthreads();
    return qc;
}

template <int KIND>
__global__ __launch_bounds__(256, 3) void k_grad_tilegemm(KernParams kp, const double* __restrict__ Xt, long ldx, long n,
                                                          const double* __restrict__ W, long ldw,
                                                          const double* __restrict__ alpha, int Dy, int q_off, long ntiles,
                                                          double* __restrict__ partials, const double* __restrict__ aa_scale) {
    __shared__ __attribute__((aligned(16))) double si[KDC * TG_SI];
    __shared__ __attribute__((aligned(16))) double sj[KDC * TG_SJ];
    __shared__ double sa[4 * 16 * TG_AS];                 // per wave: 16 rows x 16 columns of T
    __shared__ __attribute__((aligned(16))) double scs[4 * KT];   // per wave: the column sums of its 16 rows
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4, w = t >> 6, kk = ty & 3;
    const int qcnt = (kp.D - q_off < KDC) ? (kp.D - q_off) : KDC;
    const bool two = qcnt > 16;                           // a second block of 16 dimensions
    const double sc = aa_scale ? aa_scale[0] : 1.0;
    double* saw = sa + w * 16 * TG_AS;
    const int arow = (4 * (tx & 3) + (tx >> 2)) * TG_AS + kk;
    double a_var = 0.0, acc0 = 0.0, acc1 = 0.0;

    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        long ti, tj;
        grad_tile<true>(tile, 0, ti, tj);
        const long i0 = ti * KT, j0 = tj * KT;
        double r2[4][4];
        zero_tile(r2);
        int last_q0 = -1;
        for (int q0 = 0; q0 < kp.D; last_q0 = q0, q0 += KDC) {
            const int qc = tg_stage(kp.D, q0, Xt, ldx, i0, j0, si, sj, t);
            for (int q = 0; q < qc; ++q) {
                const d2 xa = *reinterpret_cast<const d2*>(si + q * TG_SI + ty * 4);
                const d2 xb = *reinterpret_cast<const d2*>(si + q * TG_SI + ty * 4 + 2);
                const double xi[4] = {xa[0], xa[1], xb[0], xb[1]};
                const d2 lo = *reinterpret_cast<const d2*>(sj + q * TG_SJ + 2 * tx);
                const d2 hi = *reinterpret_cast<const d2*>(sj + q * TG_SJ + 40 + 2 * tx);
                const double xj[4] = {lo[0], lo[1], hi[0], hi[1]};
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const double d = xi[a] - xj[b];
                        r2[a][b] = fma(d, d, r2[a][b]);
                    }
            }
        }
        // T = g (dK/dr)/r and the variance sum
        double gT[4][4];
        if (tj < ti && i0 + KT <= n) {
            const long ib = i0 + ty * 4, jb = j0 + tx * 4;
            if (Dy == 1) {
                double ai[4], aj[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) ai[a] = alpha[ib + a], aj[a] = alpha[jb + a];
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) gT[a][b] = fma(ai[a], aj[b], 0.0);
            } else {
                zero_tile(gT);
                for (int d = 0; d < Dy; ++d) {
                    double ai[4], aj[4];
#pragma unroll
                    for (int a = 0; a < 4; ++a) ai[a] = alpha[(ib + a) * Dy + d], aj[a] = alpha[(jb + a) * Dy + d];
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int b = 0; b < 4; ++b) gT[a][b] = fma(ai[a], aj[b], gT[a][b]);
                }
            }
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const d4 wv = *reinterpret_cast<const d4*>(W + (ib + a) * ldw + jb);
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    double g = 0.5 * (sc * gT[a][b] - (double)Dy * wv[b]);
                    g *= 2.0;
                    const CovVal c = cov_all(KIND, kp.variance, r2[a][b], false);
                    a_var = fma(g, c.k, a_var);
                    gT[a][b] = g * c.dk_or;
                }
            }
        } else {
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const long i = i0 + ty * 4 + a;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const long j = j0 + tx * 4 + b;
                    double g = 0.0;
                    if (i < n && j <= i) {
                        double aa = 0.0;
                        for (int d = 0; d < Dy; ++d) aa = fma(alpha[i * Dy + d], alpha[j * Dy + d], aa);
                        g = 0.5 * (sc * aa - (double)Dy * W[i * ldw + j]);
                        if (j < i) g *= 2.0;
                    }
                    const CovVal c = cov_all(KIND, kp.variance, r2[a][b], i == j);
                    a_var = fma(g, c.k, a_var);
                    gT[a][b] = g * c.dk_or;
                }
            }
        }
        // bring the dimensions this launch reduces back (D > 32)
        if (last_q0 != q_off) tg_stage(kp.D, q_off, Xt, ldx, i0, j0, si, sj, t);
        // R: over the 16 lanes of the row group; C: over the wave's four row groups here, over the waves below
        double R[4], C[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            R[a] = (gT[a][0] + gT[a][1]) + (gT[a][2] + gT[a][3]);
            C[a] = (gT[0][a] + gT[1][a]) + (gT[2][a] + gT[3][a]);
        }
#pragma unroll
        for (int m = 1; m < 16; m <<= 1)
#pragma unroll
            for (int a = 0; a < 4; ++a) R[a] += __shfl_xor(R[a], m);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            C[b] += __shfl_xor(C[b], 16);
            C[b] += __shfl_xor(C[b], 32);
        }
        if (kk == 0) {
            *reinterpret_cast<d2*>(scs + w * KT + 4 * tx) = (d2){C[0], C[1]};
            *reinterpret_cast<d2*>(scs + w * KT + 4 * tx + 2) = (d2){C[2], C[3]};
        }
        // P = T V: column 4 tx' + b of the tile is k index tx' of chunk b
        const double c0 = sj[tx * TG_SJ], c1 = two ? sj[(16 + tx) * TG_SJ] : 0.0;   // the centre: column point 0 (xj_pos(0) = 0)
        d4 P0 = {0.0, 0.0, 0.0, 0.0}, P1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int b = 0; b < 4; ++b) {
#pragma unroll
            for (int a = 0; a < 4; ++a) saw[(4 * kk + a) * TG_AS + tx] = gT[a][b];
            __builtin_amdgcn_wave_barrier();
            const double* vb = sj + tx * TG_SJ + 40 * (b >> 1) + (b & 1) + 2 * kk;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const double av = saw[arow + 4 * s];
                P0 = mfma_f64(av, vb[8 * s] - c0, P0);
                if (two) P1 = mfma_f64(av, vb[16 * TG_SJ + 8 * s] - c1, P1);
            }
            __builtin_amdgcn_wave_barrier();
        }
        __syncthreads();                                     // the waves' column sums are there
        // the thread's share: dimensions tx (and 16 + tx), rows 4 ty .. + 3 (its own), columns 4 ty .. + 3
        double Cs[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) Cs[b] = scs[4 * ty + b];
#pragma unroll
        for (int ww = 1; ww < 4; ++ww)
#pragma unroll
            for (int b = 0; b < 4; ++b) Cs[b] += scs[ww * KT + 4 * ty + b];
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            if (qb == 0 || two) {
                const int q = 16 * qb + tx;
                const double c = qb ? c1 : c0;
                const d4 P = qb ? P1 : P0;
                const d2 ua = *reinterpret_cast<const d2*>(si + q * TG_SI + ty * 4);
                const d2 ub = *reinterpret_cast<const d2*>(si + q * TG_SI + ty * 4 + 2);
                const d2 va = *reinterpret_cast<const d2*>(sj + q * TG_SJ + 2 * ty);
                const d2 vc = *reinterpret_cast<const d2*>(sj + q * TG_SJ + 40 + 2 * ty);
                const double u[4] = {ua[0] - c, ua[1] - c, ub[0] - c, ub[1] - c};
                const double v[4] = {va[0] - c, va[1] - c, vc[0] - c, vc[1] - c};
                double s = 0.0;
#pragma unroll
                for (int a = 0; a < 4; ++a) s = fma(u[a], fma(u[a], R[a], -2.0 * P[a]), s);
#pragma unroll
                for (int b = 0; b < 4; ++b) s = fma(v[b] * v[b], Cs[b], s);
                if (qb) acc1 += s;
                else acc0 += s;
            }
        }
    }
    // deterministic block reduction -> partials[blockIdx][...]: dimension 16 qb + tx over the 16 row groups in order
    double* out = partials + (long)blockIdx.x * GP_STRIDE;
    const double sv = block_sum(t, a_var);
    if (t == 0) out[0] = sv;
    double* red = block_red();
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
        if (qb == 0 || two) {
            __syncthreads();
            red[t] = qb ? acc1 : acc0;
            __syncthreads();
            if (t < 16 && 16 * qb + t < qcnt) {
                double s = 0.0;
                for (int r = 0; r < 16; ++r) s += red[r * 16 + t];
                out[2 + 16 * qb + t] = s;
            }
        }
    }
}

static int pick_grad_blocks(long ntiles) { return (int)((ntiles < 2048) ? ntiles : 2048); }

int grad_num_blocks(long n) {
    const long nt = (n + KT - 1) / KT;
    return pick_grad_blocks(nt * (nt + 1) / 2);
}

int grad_generic_num_blocks(long n, long m) {
    return pick_grad_blocks(((n + KT - 1) / KT) * ((m + KT - 1) / KT));
}

// One launch per group of 32 dimensions for a kind that reduces per dimension (ARD), one launch otherwise: launch(q_off, part,
// h) with the records of group gidx at part = partials + gidx * nb * GP_STRIDE.  Hout may alias G (in place), which every
// launch reads: only the LAST group's launch gets it as h.
template <class Launch>
static void for_each_group(int D, bool perdim, int nb, double* partials, double* Hout, Launch launch) {
    if (!perdim) {
        launch(0, partials, Hout);
        return;
    }
    for (int q_off = 0, gidx = 0; q_off < D; q_off += KDC, ++gidx)
        launch(q_off, partials + (long)gidx * nb * GP_STRIDE, (q_off + KDC >= D) ? Hout : nullptr);
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

// out[0] = (nu + n) / (nu + beta - 2) with beta = scal[0] = sum(alpha * R)   (exact_studentt_inference.py:46,51)
__global__ void k_studentt_scale(const double* __restrict__ scal, double nu, double n, double* __restrict__ out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) out[0] = (nu + n) / (nu + scal[0] - 2.0);
}
void launch_studentt_scale(hipStream_t st, const double* scal, double nu, long n, double* out) {
    hipLaunchKernelGGL(k_studentt_scale, dim3(1), dim3(64), 0, st, scal, nu, (double)n, out);
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

// ------------------------------------------------------------------------------------------------
// RatQuad (kind 6, stationary.py:747-802) and StdPeriodic (kind 7, standard_periodic.py:15-580).
// Their own kernels (templates on the kind) around the shared skeleton: the accumulate step and the element are what differs.
//   RatQuad:     K = var exp(-a log1p(r^2 / 2)),  dK/dr / r = -a K / (1 + r^2 / 2),  dK/da = -K log1p(r^2 / 2)
//                (inputs scaled by 1 / l as for the other stationary kinds)
//   StdPeriodic: K = var exp(-1/2 sum_q (sin(Delta_q) / l_q)^2),  Delta_q = pi (x_iq - x_jq) / T_q
//                (inputs staged UNSCALED: Delta is formed from the difference of the raw coordinates, so calendar-year
//                inputs keep their precision; pi / T_q and 1 / l_q are applied per dimension in the pair loop)

__device__ __forceinline__ void ratquad_all(double var, double a, double r2, double& k, double& dk_or, double& dk_a) {
    const double h = 0.5 * r2;
    const double lg = log1p(h);
    k = var * exp(-a * lg);
    dk_or = -a * k / (1.0 + h);
    dk_a = -k * lg;
}

// Cosine (kind 12, stationary.py:664-680), Sinc (kind 13, :717-743) and ExpQuadCosine (kind 14, :682-713): functions of the
// scaled distance r = sqrt(s) alone, in the kernels of RatQuad (inputs scaled by 1 / l).  Each helper returns K and (dK/dr) / r
// from ONE sincos evaluation; (dK/dr) / r is 0 at r = 0, the reference's _inv_dist convention (:225-232).  The arguments of
// Sinc and ExpQuadCosine are multiples of pi: sincospi reduces 2 r and 2 r / T exactly instead of a product with a rounded pi.
//   Cosine:        K = var cos r,                           dK/dr = -var sin r
//   Sinc:          K = var sinc(2 r) = var sin(2 pi r) / (2 pi r),  dK/dr = var (cos(2 pi r) - sinc(2 r)) / r
//   ExpQuadCosine: K = var E cos(2 pi r / T), E = exp(-2 pi^2 r^2),  dK/dr = -4 pi^2 r K - var (2 pi / T) E sin(2 pi r / T),
//                  dK/dT = var (2 pi r / T^2) E sin(2 pi r / T)     (kp.power carries T)
#define OSC_2PI2 (2.0 * M_PI * M_PI)
#define OSC_4PI2 (4.0 * M_PI * M_PI)

__device__ __forceinline__ void cosine_all(double var, double s, double& k, double& dk_or) {
    const double r = sqrt(s);
    double sn, cs;
    sincos(r, &sn, &cs);
    k = var * cs;
    dk_or = (r > 0.0) ? -var * sn / r : 0.0;
}

// cos t - sin t / t = sum_{k >= 1} (-1)^k 2k / (2k + 1)! u^k in u = t^2 = 4 pi^2 s.  Below u = 1 the difference of the two
// rounded values would cancel (the reference switches to its leading term -u / 3 below r = 1e-5, :733-743); ten terms leave a
// truncation of 22 / 23! < 1e-21 there.
__device__ __forceinline__ double sinc_diff_series(double u) {
    double p = 20.0 / 51090942171709440000.0;                  // 20 / 21!
    p = fma(p, u, -18.0 / 121645100408832000.0);               // 18 / 19!
    p = fma(p, u, 16.0 / 355687428096000.0);                   // 16 / 17!
    p = fma(p, u, -14.0 / 1307674368000.0);                    // 14 / 15!
    p = fma(p, u, 12.0 / 6227020800.0);                        // 12 / 13!
    p = fma(p, u, -10.0 / 39916800.0);                         // 10 / 11!
    p = fma(p, u, 8.0 / 362880.0);                             // 8 / 9!
    p = fma(p, u, -6.0 / 5040.0);                              // 6 / 7!
    p = fma(p, u, 4.0 / 120.0);                                // 4 / 5!
    p = fma(p, u, -2.0 / 6.0);                                 // 2 / 3!
    return p;                                                  // (cos t - sin t / t) / u
}

__device__ __forceinline__ void sinc_all(double var, double s, double& k, double& dk_or) {
    const double x = 2.0 * sqrt(s), u = OSC_4PI2 * s;
    double sn, cs;
    sincospi(x, &sn, &cs);
    const double snc = (x > 0.0) ? sn / (M_PI * x) : 1.0;
    k = var * snc;
    // (dK/dr) / r = var (cos t - sinc) / r^2 = 4 pi^2 var (cos t - sinc) / u
    if (u < 1.0) dk_or = (s > 0.0) ? OSC_4PI2 * var * sinc_diff_series(u) : 0.0;
    else dk_or = var * (cs - snc) / s;
}

__device__ __forceinline__ void eqc_all(double var, double T, double s, double& k, double& dk_or, double& dk_T) {
    const double r = sqrt(s), e = var * exp(-OSC_2PI2 * s);
    double sn, cs;
    sincospi(2.0 * r / T, &sn, &cs);
    const double w = 2.0 * M_PI / T * e * sn;                  // var (2 pi / T) E sin(2 pi r / T)
    k = e * cs;
    dk_or = (r > 0.0) ? -OSC_4PI2 * k - w / r : 0.0;
    dk_T = w * r / T;
}

// K, (dK/dr) / r and the derivative by the kind's scalar parameter (RatQuad: power, ExpQuadCosine: period; 0 otherwise)
template <int KIND>
__device__ __forceinline__ void ext_all(const KernParams& kp, double s, double& k, double& dk_or, double& dk_p) {
    if (KIND == MI355GP_RATQUAD) {
        ratquad_all(kp.variance, kp.power, s, k, dk_or, dk_p);
    } else if (KIND == MI355GP_COSINE) {
        cosine_all(kp.variance, s, k, dk_or);
        dk_p = 0.0;
    } else if (KIND == MI355GP_SINC) {
        sinc_all(kp.variance, s, k, dk_or);
        dk_p = 0.0;
    } else {
        eqc_all(kp.variance, kp.power, s, k, dk_or, dk_p);
    }
}

// s[a][b] += sum_q (sin(pi / T_q (xi[q][ty*4+a] - xj[q][tx*4+b])) / l_q)^2 over the staged dimensions q0 .. q0 + qc
__device__ __forceinline__ void accum_per(const double* si, const double* sj, const double* __restrict__ pw, int D, int q0, int qc,
                                          int ty, int tx, double (&s)[4][4]) {
    for (int q = 0; q < qc; ++q) {
        const double pt = pw[q0 + q], il = pw[D + q0 + q];
        const d4 xi = *reinterpret_cast<const d4*>(si + q * KT + ty * 4);
        const d4 xj = ld_xj(sj, q, tx);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const double sn = sin((xi[a] - xj[b]) * pt) * il;
                s[a][b] = fma(sn, sn, s[a][b]);
            }
    }
}

template <int KIND>
__device__ __forceinline__ void accum_ext(const double* si, const double* sj, const KernParams& kp, int q0, int qc, int ty, int tx,
                                          double (&s)[4][4]) {
    if (KIND != MI355GP_STDPERIODIC) accum_r2(si, sj, qc, ty, tx, s);
    else accum_per(si, sj, kp.pw, kp.D, q0, qc, ty, tx, s);
}

template <int KIND>
__device__ __forceinline__ double ext_k(const KernParams& kp, double s) {
    if (KIND == MI355GP_RATQUAD) return kp.variance * exp(-kp.power * log1p(0.5 * s));
    if (KIND == MI355GP_COSINE) return kp.variance * cos(sqrt(s));
    if (KIND == MI355GP_SINC) {
        const double x = 2.0 * sqrt(s);
        return kp.variance * ((x > 0.0) ? sinpi(x) / (M_PI * x) : 1.0);
    }
    if (KIND == MI355GP_EXPQUADCOSINE) return kp.variance * exp(-OSC_2PI2 * s) * cospi(2.0 * sqrt(s) / kp.power);
    return kp.variance * exp(-0.5 * s);
}

// Covariance assembly for these kinds: no White-like diagonal in any.
template <bool SYM, int KIND>
__global__ __launch_bounds__(256) void k_kbuild_ext(KbuildArgs A) {
    __shared__ __attribute__((aligned(16))) double si[KDC * KT];
    __shared__ __attribute__((aligned(16))) double sj[KDC * KTJ];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    long i0, j0;
    if (!kbuild_tile<SYM>(A, i0, j0)) return;
    double s[4][4];
    zero_tile(s);
    if (i0 < A.n && j0 < A.m)
        for (int q0 = 0; q0 < A.kp.D; q0 += KDC)
            accum_ext<KIND>(si, sj, A.kp, q0, stage_chunk(A.kp.D, q0, A.Xt1, A.ld1, i0, A.Xt2, A.ld2, j0, si, sj, t), ty, tx, s);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const long i = i0 + ty * 4 + a;
        double v[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const long j = j0 + tx * 4 + b;
            if (i < A.n && j < A.m) v[b] = ext_k<KIND>(A.kp, s[a][b]);
            else v[b] = kbuild_pad<SYM>(A, i, j);
        }
        kbuild_store_row<SYM>(A, i, j0, tx, v);
    }
}

// Gradient pass of k_grad for these kinds, one launch per group of 32 dimensions (q_off).  Record A [GP_STRIDE] per block:
//   [0] sum g K, RatQuad [1] sum g dK/dr r (isotropic) or [2 + q] sum g (dK/dr / r) (x~_iq - x~_jq)^2 (ARD)
//   (Cosine, Sinc and ExpQuadCosine as RatQuad; record B [0] of ExpQuadCosine: sum g dK/dperiod, none for the other two),
//   StdPeriodic [2 + q] sum g K sin(D_q) cos(D_q) D_q (period);
// record B at partB: RatQuad [0] sum g dK/dpower, StdPeriodic [2 + q] sum g K sin^2(D_q) (lengthscale).
// StdPeriodic always reduces per dimension; the host applies 1 / (T_q l_q^2), 1 / l_q^3 and sums the isotropic cases.
template <bool FUSED, int KIND>
__global__ __launch_bounds__(256) void k_grad_ext(KernParams kp, const double* __restrict__ Xt1, long ld1, long n,
                                                  const double* __restrict__ Xt2, long ld2, long m,
                                                  const double* __restrict__ G, long ldg,
                                                  const double* __restrict__ alpha, int Dy, int q_off,
                                                  long ntiles, int ntc, double* __restrict__ partA, double* __restrict__ partB,
                                                  double* __restrict__ Hout, long ldh, const double* __restrict__ aa_scale,
                                                  const double* __restrict__ Mul, long ldm) {
    constexpr bool PER = (KIND == MI355GP_STDPERIODIC);
    constexpr bool SCALAR = (KIND == MI355GP_RATQUAD || KIND == MI355GP_EXPQUADCOSINE);   // a scalar parameter: record B [0]
    __shared__ __attribute__((aligned(16))) double si[KDC * KT];
    __shared__ __attribute__((aligned(16))) double sj[KDC * KTJ];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const bool perdim = PER || kp.ard;
    double a_var = 0.0, a_iso = 0.0, a_pow = 0.0;
    double a1[KDC], a2[PER ? KDC : 1];
#pragma unroll
    for (int q = 0; q < KDC; ++q) a1[q] = 0.0;
#pragma unroll
    for (int q = 0; q < (PER ? KDC : 1); ++q) a2[q] = 0.0;
    const int qcnt = perdim ? ((kp.D - q_off < KDC) ? (kp.D - q_off) : KDC) : 0;
    const double sc = (FUSED && aa_scale) ? aa_scale[0] : 1.0;

    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        long ti, tj;
        grad_tile<FUSED>(tile, ntc, ti, tj);
        const long i0 = ti * KT, j0 = tj * KT;
        double s[4][4];
        zero_tile(s);
        int last_q0 = -1;
        for (int q0 = 0; q0 < kp.D; last_q0 = q0, q0 += KDC)
            accum_ext<KIND>(si, sj, kp, q0, stage_chunk(kp.D, q0, Xt1, ld1, i0, Xt2, ld2, j0, si, sj, t), ty, tx, s);
        double gw[4][4];   // functions of r: g dK/dr / r;  StdPeriodic: g K
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const long i = i0 + ty * 4 + a;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const long j = j0 + tx * 4 + b;
                const double g = grad_weight<FUSED, true>(i, j, n, m, G, ldg, alpha, Dy, sc, Mul, ldm);
                if (PER) {
                    const double k = kp.variance * exp(-0.5 * s[a][b]);
                    a_var = fma(g, k, a_var);
                    gw[a][b] = g * k;
                } else {
                    double k, dk_or, dk_a;
                    ext_all<KIND>(kp, s[a][b], k, dk_or, dk_a);
                    a_var = fma(g, k, a_var);
                    if (SCALAR) a_pow = fma(g, dk_a, a_pow);
                    if (!kp.ard) a_iso = fma(g, dk_or * s[a][b], a_iso);
                    gw[a][b] = g * dk_or;
                }
            }
        }
        // functions of r: H = dL_dK (dK/dr) / r as in k_grad (0 at r = 0); StdPeriodic has its own dK/dx pass (k_periodic_gradx)
        if (!PER && !FUSED && Hout) {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) store_h<true>(Hout, ldh, i0 + ty * 4 + a, j0 + tx * 4 + b, n, m, s[a][b], gw[a][b]);
        }
        if (qcnt > 0) {
            restage(last_q0, q_off, qcnt, Xt1, ld1, i0, Xt2, ld2, j0, si, sj, t);
#pragma unroll
            for (int q = 0; q < KDC; ++q) {
                if (q < qcnt) {
                    const d4 xi = *reinterpret_cast<const d4*>(si + q * KT + ty * 4);
                    const d4 xj = ld_xj(sj, q, tx);
                    if (PER) {
                        const double pt = kp.pw[q_off + q];
                        double s1 = 0.0, s2 = 0.0;
#pragma unroll
                        for (int a = 0; a < 4; ++a)
#pragma unroll
                            for (int b = 0; b < 4; ++b) {
                                const double dl = (xi[a] - xj[b]) * pt;
                                double sn, cs;
                                sincos(dl, &sn, &cs);
                                s1 = fma(gw[a][b], sn * cs * dl, s1);
                                s2 = fma(gw[a][b], sn * sn, s2);
                            }
                        a1[q] += s1;
                        a2[PER ? q : 0] += s2;
                    } else {
                        double s1 = 0.0;
#pragma unroll
                        for (int a = 0; a < 4; ++a)
#pragma unroll
                            for (int b = 0; b < 4; ++b) {
                                const double d = xi[a] - xj[b];
                                s1 = fma(gw[a][b], d * d, s1);
                            }
                        a1[q] += s1;
                    }
                }
            }
        }
    }
    double* outA = partA + (long)blockIdx.x * GP_STRIDE;
    double* outB = partB + (long)blockIdx.x * GP_STRIDE;
    const double sv = block_sum(t, a_var);
    if (t == 0) outA[0] = sv;
    if (!PER) {
        if (SCALAR) {
            const double sp = block_sum(t, a_pow);
            if (t == 0) outB[0] = sp;
        }
        if (!kp.ard) {
            const double sl = block_sum(t, a_iso);
            if (t == 0) outA[1] = sl;
        }
    }
#pragma unroll
    for (int q = 0; q < KDC; ++q) {
        if (q < qcnt) {
            const double s1 = block_sum(t, a1[q]);
            if (t == 0) outA[2 + q] = s1;
            if (PER) {
                const double s2 = block_sum(t, a2[PER ? q : 0]);
                if (t == 0) outB[2 + q] = s2;
            }
        }
    }
}

// (the signature every family's gradient launcher has: the arguments of the kernels but q_off, which for_each_group supplies)
static void launch_grad_ext(hipStream_t st, bool fused, KernParams kp, const double* Xt1, long ld1, long n, const double* Xt2,
                            long ld2, long m, const double* G, long ldg, const double* alpha, int Dy, long ntiles, int ntc,
                            double* partials, double* Hout, long ldh, const double* aa_scale, const double* Mul, long ldm) {
    const int nb = pick_grad_blocks(ntiles);
    const dim3 g((unsigned)nb), b(256);
    const bool per = kp.kind == MI355GP_STDPERIODIC;
    const long offB = (long)((kp.D + KDC - 1) / KDC) * nb * GP_STRIDE;      // the second records follow every group's first
    for_each_group(kp.D, per || kp.ard, nb, partials, Hout, [&](int q_off, double* pa, double* h) {
#define GRAD_EXT(F, K)                                                                                                           \
    hipLaunchKernelGGL((k_grad_ext<F, K>), g, b, 0, st, kp, Xt1, ld1, n, Xt2, ld2, m, G, ldg, alpha, Dy, q_off, ntiles, ntc, pa, \
                       pa + offB, h, ldh, aa_scale, Mul, ldm)
        if (per) {
            if (fused) GRAD_EXT(true, MI355GP_STDPERIODIC);
            else GRAD_EXT(false, MI355GP_STDPERIODIC);
        } else if (kp.kind == MI355GP_COSINE) {
            if (fused) GRAD_EXT(true, MI355GP_COSINE);
            else GRAD_EXT(false, MI355GP_COSINE);
        } else if (kp.kind == MI355GP_SINC) {
            if (fused) GRAD_EXT(true, MI355GP_SINC);
            else GRAD_EXT(false, MI355GP_SINC);
        } else if (kp.kind == MI355GP_EXPQUADCOSINE) {
            if (fused) GRAD_EXT(true, MI355GP_EXPQUADCOSINE);
            else GRAD_EXT(false, MI355GP_EXPQUADCOSINE);
        } else {
            if (fused) GRAD_EXT(true, MI355GP_RATQUAD);
            else GRAD_EXT(false, MI355GP_RATQUAD);
        }
#undef GRAD_EXT
    });
}

// StdPeriodic dK/dx as a row reduction (see internal.h).  Block = 64 rows x 4 column lanes; the block walks every 64-column
// tile, the covariance of each pair is formed over all dimensions first (chunks of 32), then the dimensions of the group
// q_off .. q_off + 31 are accumulated.  The four lanes of a row are combined in fixed order: bit reproducible.
__global__ __launch_bounds__(256) void k_periodic_gradx(KernParams kp, const double* __restrict__ Xt1, long ld1, long n,
                                                        const double* __restrict__ Xt2, long ld2, long m,
                                                        const double* __restrict__ W, long ldw, int wt, int q_off,
                                                        double* __restrict__ out) {
    __shared__ double si[KDC * KT];
    __shared__ double sj[KDC * KT];
    __shared__ double red[4][KT];
    const int t = threadIdx.x, r = t & 63, l = t >> 6;
    const long i0 = (long)blockIdx.x * KT, i = i0 + r;
    const int qcnt = (kp.D - q_off < KDC) ? (kp.D - q_off) : KDC;
    const double* __restrict__ pt = kp.pw;
    const double* __restrict__ il = kp.pw + kp.D;
    double acc[KDC];
#pragma unroll
    for (int q = 0; q < KDC; ++q) acc[q] = 0.0;
    for (long j0 = 0; j0 < m; j0 += KT) {
        double s[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) s[c] = 0.0;
        int last_q0 = -1;
        for (int q0 = 0; q0 < kp.D; q0 += KDC) {
            const int qc = (kp.D - q0 < KDC) ? (kp.D - q0) : KDC;
            __syncthreads();
            stage_x(Xt1, ld1, i0, q0, qc, si, t);
            stage_x(Xt2, ld2, j0, q0, qc, sj, t);
            __syncthreads();
            for (int q = 0; q < qc; ++q) {
                const double xi = si[q * KT + r], p = pt[q0 + q], w = il[q0 + q];
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    const double sn = sin((xi - sj[q * KT + 4 * c + l]) * p) * w;
                    s[c] = fma(sn, sn, s[c]);
                }
            }
            last_q0 = q0;
        }
        // weights W(i, j) K(i, j)
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const long j = j0 + 4 * c + l;
            double wk = 0.0;
            if (i < n && j < m) wk = (wt ? W[j * ldw + i] : W[i * ldw + j]) * kp.variance * exp(-0.5 * s[c]);
            s[c] = wk;
        }
        if (last_q0 != q_off) {
            __syncthreads();
            stage_x(Xt1, ld1, i0, q_off, qcnt, si, t);
            stage_x(Xt2, ld2, j0, q_off, qcnt, sj, t);
            __syncthreads();
        }
#pragma unroll
        for (int q = 0; q < KDC; ++q) {
            if (q < qcnt) {
                const double xi = si[q * KT + r], p = pt[q_off + q];
                double a = 0.0;
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    double sn, cs;
                    sincos((xi - sj[q * KT + 4 * c + l]) * p, &sn, &cs);
                    a = fma(s[c], 2.0 * sn * cs, a);
                }
                acc[q] += a;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < KDC; ++q) {
        if (q < qcnt) {
            __syncthreads();
            red[l][r] = acc[q];
            __syncthreads();
            if (l == 0 && i < n) out[i * kp.D + q_off + q] = (red[0][r] + red[1][r]) + (red[2][r] + red[3][r]);
        }
    }
}

void launch_periodic_gradx(hipStream_t st, KernParams kp, const double* Xt1, long ld1, long n, const double* Xt2, long ld2,
                           long m, const double* W, long ldw, int wt, double* out) {
    const unsigned nbr = (unsigned)((n + KT - 1) / KT);
    for (int q_off = 0; q_off < kp.D; q_off += KDC)
        hipLaunchKernelGGL(k_periodic_gradx, dim3(nbr), dim3(256), 0, st, kp, Xt1, ld1, n, Xt2, ld2, m, W, ldw, wt, q_off, out);
}

// ------------------------------------------------------------------------------------------------
// Coregionalize (kind 8, coregionalize.py:82-157): k(x, x') = B[idx][idx'], idx = the value of input row kp.col of Xt (staged
// unscaled), B = kp.pw (P x P row-major, P = kp.ard <= 16).  The host validates every index before a launch; an index that is
// not an integer in [0, P) still never reads outside B here: it yields NaN (K-build) or poisons the block's record (gradient).
#define COREG_PMAX 16

__device__ __forceinline__ int coreg_idx(double x, int P) {
    const int a = (int)x;
    return ((double)a == x && a >= 0 && a < P) ? a : -1;
}

// Covariance assembly: the skeleton's tile decode and row epilogue around a lookup -- nothing to accumulate.  B lives in LDS
// once per block, the tile's row / column indices as integers.  The diagonal is what B gives.
template <bool SYM>
__global__ __launch_bounds__(256) void k_kbuild_coreg(KbuildArgs A) {
    __shared__ double sB[COREG_PMAX * COREG_PMAX];
    __shared__ int sa[KT], sb[KT];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    long i0, j0;
    if (!kbuild_tile<SYM>(A, i0, j0)) return;
    const int P = A.kp.ard;
    for (int k = t; k < P * P; k += 256) sB[k] = A.kp.pw[k];
    if (t < KT) {
        const long i = i0 + t;
        sa[t] = (i < A.n) ? coreg_idx(A.Xt1[(long)A.kp.col * A.ld1 + i], P) : 0;
    } else if (t < 2 * KT) {
        const long j = j0 + (t - KT);
        sb[t - KT] = (j < A.m) ? coreg_idx(A.Xt2[(long)A.kp.col * A.ld2 + j], P) : 0;
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const long i = i0 + ty * 4 + a;
        const int ia = sa[ty * 4 + a];
        double v[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const long j = j0 + tx * 4 + b;
            const int jb = sb[tx * 4 + b];
            if (i < A.n && j < A.m) v[b] = (ia >= 0 && jb >= 0) ? sB[ia * P + jb] : __builtin_nan("");
            else v[b] = kbuild_pad<SYM>(A, i, j);
        }
        kbuild_store_row<SYM>(A, i, j0, tx, v);
    }
}

// The bucketed gradient (see internal.h).  Per tile: the row / column indices go to LDS and two waves OR them into the masks of
// the outputs present among the tile's rows and columns; then, for every present pair (a, b) in a fixed order, each thread sums
// its masked 4 x 4 register elements and a fixed-order wave / block tree reduces them into the block's LDS record.  Rows sorted
// by output (build_XY) give one pair in nearly every tile: one reduction per tile.  FUSED runs over the lower tiles; the second
// sum d (diagonal elements, diagonal tiles only) lets S[b][a] receive the strict lower part once more: the symmetric completion.
template <bool FUSED>
__global__ __launch_bounds__(256) void k_grad_coreg(KernParams kp, const double* __restrict__ Xt1, long ld1, long n,
                                                    const double* __restrict__ Xt2, long ld2, long m,
                                                    const double* __restrict__ G, long ldg, const double* __restrict__ alpha,
                                                    int Dy, long ntiles, int ntc, double* __restrict__ partials,
                                                    const double* __restrict__ aa_scale, const double* __restrict__ Mul,
                                                    long ldm) {
    __shared__ double sacc[COREG_PMAX * COREG_PMAX];
    __shared__ int sa[KT], sb[KT];
    __shared__ unsigned smask[2];
    __shared__ double red[4][2];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4, lane = t & 63, wv = t >> 6;
    const int P = kp.ard;
    for (int k = t; k < P * P; k += 256) sacc[k] = 0.0;
    const double sc = (FUSED && aa_scale) ? aa_scale[0] : 1.0;
    bool poisoned = false;                                 // (thread 0) an index outside [0, P) was met

    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        long ti, tj;
        grad_tile<FUSED>(tile, ntc, ti, tj);
        const long i0 = ti * KT, j0 = tj * KT;
        __syncthreads();                                   // the previous tile's reads of sa / sb / smask are done
        if (wv < 2) {
            const long r = (wv == 0 ? i0 : j0) + lane;
            int v = -2;                                    // -2: padding (no element), -1: an invalid index
            if (wv == 0 && r < n) v = coreg_idx(Xt1[(long)kp.col * ld1 + r], P);
            if (wv == 1 && r < m) v = coreg_idx(Xt2[(long)kp.col * ld2 + r], P);
            unsigned bit = (v >= 0) ? (1u << v) : (v == -1 ? (1u << COREG_PMAX) : 0u);
            for (int off = 32; off > 0; off >>= 1) bit |= (unsigned)__shfl_xor((int)bit, off);
            if (wv == 0) sa[lane] = v;
            else sb[lane] = v;
            if (lane == 0) smask[wv] = bit;
        }
        double w[4][4];   // no doubling below the diagonal: sd completes symmetrically
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b)
                w[a][b] = grad_weight<FUSED, false>(i0 + ty * 4 + a, j0 + tx * 4 + b, n, m, G, ldg, alpha, Dy, sc, Mul, ldm);
        __syncthreads();
        const unsigned rm = smask[0], cm = smask[1];
        if (t == 0 && ((rm | cm) >> COREG_PMAX)) poisoned = true;
        int ra[4], cb[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) ra[a] = sa[ty * 4 + a];
#pragma unroll
        for (int b = 0; b < 4; ++b) cb[b] = sb[tx * 4 + b];
        const bool diag_tile = FUSED && ti == tj;
        for (unsigned rmm = rm & ((1u << COREG_PMAX) - 1); rmm; rmm &= rmm - 1) {
            const int pa = __ffs(rmm) - 1;
            for (unsigned cmm = cm & ((1u << COREG_PMAX) - 1); cmm; cmm &= cmm - 1) {
                const int pb = __ffs(cmm) - 1;
                double v = 0.0, dg = 0.0;
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if (ra[a] == pa && cb[b] == pb) {
                            v += w[a][b];
                            if (diag_tile && ty * 4 + a == tx * 4 + b) dg += w[a][b];
                        }
                for (int off = 32; off > 0; off >>= 1) {
                    v += __shfl_down(v, off);
                    dg += __shfl_down(dg, off);
                }
                if (lane == 0) {
                    red[wv][0] = v;
                    red[wv][1] = dg;
                }
                __syncthreads();
                if (t == 0) {
                    const double sv = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
                    const double sd = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
                    sacc[pa * P + pb] += sv;
                    if (FUSED) sacc[pb * P + pa] += sv - sd;
                }
                __syncthreads();
            }
        }
    }
    __syncthreads();
    if (t == 0 && poisoned) sacc[0] = __builtin_nan("");
    __syncthreads();
    double* out = partials + (long)blockIdx.x * P * P;
    for (int k = t; k < P * P; k += 256) out[k] = sacc[k];
}

int launch_grad_coreg(hipStream_t st, bool fused, KernParams kp, const double* Xt1, long ld1, long n, const double* Xt2, long ld2,
                      long m, const double* G, long ldg, const double* alpha, int Dy, double* partials, const double* aa_scale,
                      const double* Mul, long ldm) {
    const long ntr = (n + KT - 1) / KT, ntc = (m + KT - 1) / KT;
    const long ntiles = fused ? ntr * (ntr + 1) / 2 : ntr * ntc;
    const int nb = pick_grad_blocks(ntiles);
    if (fused)
        hipLaunchKernelGGL((k_grad_coreg<true>), dim3(nb), dim3(256), 0, st, kp, Xt1, ld1, n, Xt1, ld1, n, G, ldg, alpha, Dy,
                           ntiles, (int)ntr, partials, aa_scale, Mul, ldm);
    else
        hipLaunchKernelGGL((k_grad_coreg<false>), dim3(nb), dim3(256), 0, st, kp, Xt1, ld1, n, Xt2, ld2, m, G, ldg, nullptr, 0,
                           ntiles, (int)ntc, partials, nullptr, nullptr, 0);
    return nb;
}

// out[j] = kd[j] - sum_i M[i][j]^2: k_col_reduce's variance form with a per-point Kdiag (Coregionalize parts)
__global__ __launch_bounds__(256) void k_col_reduce_vec(const double* __restrict__ M, long ld, long rows, long cols,
                                                        const double* __restrict__ kd, double* __restrict__ out) {
    __shared__ double red[4][64];
    const int tx = threadIdx.x & 63, g = threadIdx.x >> 6;
    const long j = (long)blockIdx.x * 64 + tx;
    double s = 0.0;
    if (j < cols) {
        for (long i = g; i < rows; i += 4) {
            const double x = M[i * ld + j];
            s = fma(x, x, s);
        }
    }
    red[g][tx] = s;
    __syncthreads();
    if (g == 0 && j < cols) out[j] = kd[j] - ((red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx]));
}

void launch_col_reduce_vec(hipStream_t st, const double* M, long ld, long rows, long cols, const double* kd, double* out) {
    hipLaunchKernelGGL(k_col_reduce_vec, dim3((unsigned)((cols + 63) / 64)), dim3(256), 0, st, M, ld, rows, cols, kd, out);
}

// ------------------------------------------------------------------------------------------------
// Linear (kind 9, linear.py:13-114): K = sum_q var_q x_iq x_jq.  Inputs arrive scaled by sqrt(var_q) on the active dimensions
// (0 elsewhere), so K = sum_q x~_iq x~_jq with no further factor.  Its own kernels around the shared skeleton: the dot product is
// the accumulate step, the sum is the element.  The sum over q runs in the same order for (i, j) and (j, i) and
// fma(a, b, c) = fma(b, a, c): K(X, X) is bitwise symmetric.  The diagonal is what the sum gives (it depends on the point; there
// is no variance to put there).

// s[a][b] += sum_q xi[q][ty*4+a] * xj[q][tx*4+b]
__device__ __forceinline__ void accum_dot(const double* si, const double* sj, int qc, int ty, int tx, double (&s)[4][4]) {
    for (int q = 0; q < qc; ++q) {
        const d4 xi = *reinterpret_cast<const d4*>(si + q * KT + ty * 4);
        const d4 xj = ld_xj(sj, q, tx);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) s[a][b] = fma(xi[a], xj[b], s[a][b]);
    }
}

// Covariance assembly: the element is the sum itself.
template <bool SYM>
__global__ __launch_bounds__(256) void k_kbuild_lin(KbuildArgs A) {
    __shared__ __attribute__((aligned(16))) double si[KDC * KT];
    __shared__ __attribute__((aligned(16))) double sj[KDC * KTJ];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    long i0, j0;
    if (!kbuild_tile<SYM>(A, i0, j0)) return;
    double s[4][4];
    zero_tile(s);
    if (i0 < A.n && j0 < A.m)
        for (int q0 = 0; q0 < A.kp.D; q0 += KDC)
            accum_dot(si, sj, stage_chunk(A.kp.D, q0, A.Xt1, A.ld1, i0, A.Xt2, A.ld2, j0, si, sj, t), ty, tx, s);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const long i = i0 + ty * 4 + a;
        double v[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const long j = j0 + tx * 4 + b;
            if (i < A.n && j < A.m) v[b] = s[a][b];
            else v[b] = kbuild_pad<SYM>(A, i, j);
        }
        kbuild_store_row<SYM>(A, i, j0, tx, v);
    }
}

// Gradient pass of k_grad for the kind, one launch per group of 32 dimensions (q_off; one launch if !ard).  Record [GP_STRIDE]
// per block: [0] sum g K, ARD [2 + q] sum g x~_iq x~_jq (the host divides by variance / variance_q, linear.py:87-98).
// FUSED: g = 0.5 (sc alpha alpha^T - Dy W) over the lower triangle, off-diagonal weights doubled; else g = G (n x m).
// g is multiplied by Mul (product terms) and, if Hout is given (generic form), written there: the weights of gradients_X.
template <bool FUSED>
__global__ __launch_bounds__(256) void k_grad_lin(KernParams kp, const double* __restrict__ Xt1, long ld1, long n,
                                                  const double* __restrict__ Xt2, long ld2, long m,
                                                  const double* __restrict__ G, long ldg,
                                                  const double* __restrict__ alpha, int Dy, int q_off,
                                                  long ntiles, int ntc, double* __restrict__ partials,
                                                  double* __restrict__ Hout, long ldh, const double* __restrict__ aa_scale,
                                                  const double* __restrict__ Mul, long ldm) {
    __shared__ __attribute__((aligned(16))) double si[KDC * KT];
    __shared__ __attribute__((aligned(16))) double sj[KDC * KTJ];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    double a_var = 0.0;
    double a_q[KDC];
#pragma unroll
    for (int q = 0; q < KDC; ++q) a_q[q] = 0.0;
    const int qcnt = kp.ard ? ((kp.D - q_off < KDC) ? (kp.D - q_off) : KDC) : 0;
    const double sc = (FUSED && aa_scale) ? aa_scale[0] : 1.0;

    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        long ti, tj;
        grad_tile<FUSED>(tile, ntc, ti, tj);
        const long i0 = ti * KT, j0 = tj * KT;
        double s[4][4];
        zero_tile(s);
        int last_q0 = -1;
        for (int q0 = 0; q0 < kp.D; last_q0 = q0, q0 += KDC)
            accum_dot(si, sj, stage_chunk(kp.D, q0, Xt1, ld1, i0, Xt2, ld2, j0, si, sj, t), ty, tx, s);
        double gw[4][4];   // g
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const long i = i0 + ty * 4 + a;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const long j = j0 + tx * 4 + b;
                const double g = grad_weight<FUSED, true>(i, j, n, m, G, ldg, alpha, Dy, sc, Mul, ldm);
                if (!FUSED && Hout) store_h<false>(Hout, ldh, i, j, n, m, g, g);
                a_var = fma(g, s[a][b], a_var);
                gw[a][b] = g;
            }
        }
        if (qcnt > 0) {
            restage(last_q0, q_off, qcnt, Xt1, ld1, i0, Xt2, ld2, j0, si, sj, t);
#pragma unroll
            for (int q = 0; q < KDC; ++q) {
                if (q < qcnt) {
                    const d4 xi = *reinterpret_cast<const d4*>(si + q * KT + ty * 4);
                    const d4 xj = ld_xj(sj, q, tx);
                    double s1 = 0.0;
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        double r = 0.0;
#pragma unroll
                        for (int b = 0; b < 4; ++b) r = fma(gw[a][b], xj[b], r);
                        s1 = fma(xi[a], r, s1);
                    }
                    a_q[q] += s1;
                }
            }
        }
    }
    // deterministic block reduction -> partials[blockIdx][...]
    double* out = partials + (long)blockIdx.x * GP_STRIDE;
    const double sv = block_sum(t, a_var);
    if (t == 0) out[0] = sv;
#pragma unroll
    for (int q = 0; q < KDC; ++q) {
        if (q < qcnt) {
            const double sq = block_sum(t, a_q[q]);
            if (t == 0) out[2 + q] = sq;
        }
    }
}

static void launch_grad_lin(hipStream_t st, bool fused, KernParams kp, const double* Xt1, long ld1, long n, const double* Xt2,
                            long ld2, long m, const double* G, long ldg, const double* alpha, int Dy, long ntiles, int ntc,
                            double* partials, double* Hout, long ldh, const double* aa_scale, const double* Mul, long ldm) {
    const int nb = pick_grad_blocks(ntiles);
    const dim3 g((unsigned)nb), b(256);
    for_each_group(kp.D, kp.ard != 0, nb, partials, Hout, [&](int q_off, double* pa, double* h) {
        if (fused)
            hipLaunchKernelGGL((k_grad_lin<true>), g, b, 0, st, kp, Xt1, ld1, n, Xt2, ld2, m, G, ldg, alpha, Dy, q_off, ntiles, ntc, pa,
                               h, ldh, aa_scale, Mul, ldm);
        else
            hipLaunchKernelGGL((k_grad_lin<false>), g, b, 0, st, kp, Xt1, ld1, n, Xt2, ld2, m, G, ldg, alpha, Dy, q_off, ntiles, ntc, pa,
                               h, ldh, aa_scale, Mul, ldm);
    });
}

// ------------------------------------------------------------------------------------------------
// MLP (kind 10, mlp.py:48-147) and Poly (kind 11, poly.py:15-49): functions of the three numbers x.x', x.x and x'.x' of a pair.
// Inputs arrive scaled by sqrt(weight_variance_q) (MLP) / sqrt(scale) (Poly) on the active dimensions, 0 elsewhere, so with
// d_ij = sum_q x~_iq x~_jq, n_i = sum_q x~_iq^2 (both from the same staged slabs, kp.bias = b resp. c0):
//   MLP   s = d + b, p_i = n_i + b:  K = var (2/pi) asin(s / sqrt((p_i + 1)(p_j + 1)))
//   Poly  A = d + c0:                K = var A^order (kp.power; C pow for a negative A)
// Their own kernels around the shared skeleton: dot products (and MLP's norms) accumulate.  The sums over q run in the same
// order for (i, j) and (j, i), fma(a, b, c) = fma(b, a, c) and (p_i + 1)(p_j + 1) commutes: K(X, X) is bitwise symmetric.  n_i is
// the same fma chain as d_ii, so at i == j the element is the formula at s = p_i: var (2/pi) asin(p / sqrt((p + 1)^2)) = Kdiag.

// ni[a] += sum_q xi[q][ty*4+a]^2, nj[b] += sum_q xj[q][tx*4+b]^2
__device__ __forceinline__ void accum_norms(const double* si, const double* sj, int qc, int ty, int tx, double (&ni)[4],
                                            double (&nj)[4]) {
    for (int q = 0; q < qc; ++q) {
        const d4 xi = *reinterpret_cast<const d4*>(si + q * KT + ty * 4);
        const d4 xj = ld_xj(sj, q, tx);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            ni[a] = fma(xi[a], xi[a], ni[a]);
            nj[a] = fma(xj[a], xj[a], nj[a]);
        }
    }
}

#define TWO_OVER_PI 0.63661977236758134308
// the asin argument is below 1 in exact arithmetic (Cauchy-Schwarz on (x~, sqrt b)); the clamp only absorbs a last-bit excess
__device__ __forceinline__ double mlp_k(double var, double s, double qi, double qj) {
    const double t = s / sqrt(qi * qj);
    return var * TWO_OVER_PI * asin(fmin(fmax(t, -1.0), 1.0));
}

// Covariance assembly: the dot products, for MLP the squared norms of both sides as well.
template <bool SYM, int KIND>
__global__ __launch_bounds__(256) void k_kbuild_dot(KbuildArgs A) {
    __shared__ __attribute__((aligned(16))) double si[KDC * KT];
    __shared__ __attribute__((aligned(16))) double sj[KDC * KTJ];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    long i0, j0;
    if (!kbuild_tile<SYM>(A, i0, j0)) return;
    double s[4][4], ni[4], nj[4];
    zero_tile(s);
#pragma unroll
    for (int a = 0; a < 4; ++a) ni[a] = nj[a] = 0.0;
    if (i0 < A.n && j0 < A.m)
        for (int q0 = 0; q0 < A.kp.D; q0 += KDC) {
            const int qc = stage_chunk(A.kp.D, q0, A.Xt1, A.ld1, i0, A.Xt2, A.ld2, j0, si, sj, t);
            accum_dot(si, sj, qc, ty, tx, s);
            if (KIND == MI355GP_MLP) accum_norms(si, sj, qc, ty, tx, ni, nj);
        }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const long i = i0 + ty * 4 + a;
        double v[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const long j = j0 + tx * 4 + b;
            if (i < A.n && j < A.m) {
                const double sb = s[a][b] + A.kp.bias;
                if (KIND == MI355GP_MLP) v[b] = mlp_k(A.kp.variance, sb, ni[a] + A.kp.bias + 1.0, nj[b] + A.kp.bias + 1.0);
                else v[b] = A.kp.variance * pow(sb, A.kp.power);
            } else {
                v[b] = kbuild_pad<SYM>(A, i, j);
            }
        }
        kbuild_store_row<SYM>(A, i, j0, tx, v);
    }
}

// Gradient pass of k_grad for the two kinds, one launch per group of 32 dimensions (q_off; one launch unless MLP with ard).
// Record [GP_STRIDE] per block, g = the weight of the element (below):
//   MLP   c = var (2/pi) g / sqrt((p_i + 1)(p_j + 1) - s^2)                                                  (mlp.py:105)
//         [0] sum g K        [1] sum c (1 - s (1/(p_i+1) + 1/(p_j+1)) / 2)  = d/d bias_variance              (:122)
//         ARD  [2 + q] sum c (x~_iq x~_jq - s (x~_iq^2/(p_i+1) + x~_jq^2/(p_j+1)) / 2)  = w_q d/dw_q           (:107-120)
//         else [2]     sum c (d_ij - s (n_i/(p_i+1) + n_j/(p_j+1)) / 2)                 = w d/dw              (:121)
//   Poly  h = g var order A^(order-1):  [0] sum g K   [1] sum h = d/d bias   [2] sum h d_ij = scale d/d scale (poly.py:36-42)
// FUSED: g = 0.5 (sc alpha alpha^T - Dy W) over the lower triangle, off-diagonal weights doubled (every summand above is
// symmetric in (i, j) when both sides are the same points); else g = G (n x m).  g is multiplied by Mul (product terms).
// Generic form with Hout: c (MLP) is written there -- the weights of gradients_X (mlp.py:124-130, gradx_mlp in parts.h).
// Every sum runs in a fixed order: two evaluations give identical bits.
template <bool FUSED, int KIND>
__global__ __launch_bounds__(256) void k_grad_dot(KernParams kp, const double* __restrict__ Xt1, long ld1, long n,
                                                  const double* __restrict__ Xt2, long ld2, long m,
                                                  const double* __restrict__ G, long ldg,
                                                  const double* __restrict__ alpha, int Dy, int q_off,
                                                  long ntiles, int ntc, double* __restrict__ partials,
                                                  double* __restrict__ Hout, long ldh, const double* __restrict__ aa_scale,
                                                  const double* __restrict__ Mul, long ldm) {
    constexpr bool MLP = KIND == MI355GP_MLP;
    __shared__ __attribute__((aligned(16))) double si[KDC * KT];
    __shared__ __attribute__((aligned(16))) double sj[KDC * KTJ];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    double a_var = 0.0, a_b = 0.0, a_w = 0.0;
    double a_q[KDC];
#pragma unroll
    for (int q = 0; q < KDC; ++q) a_q[q] = 0.0;
    const int qcnt = (MLP && kp.ard) ? ((kp.D - q_off < KDC) ? (kp.D - q_off) : KDC) : 0;
    const double sc = (FUSED && aa_scale) ? aa_scale[0] : 1.0;
    const double coef = MLP ? kp.variance * TWO_OVER_PI : kp.variance * kp.power;

    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        long ti, tj;
        grad_tile<FUSED>(tile, ntc, ti, tj);
        const long i0 = ti * KT, j0 = tj * KT;
        double s[4][4], ni[4], nj[4];
        zero_tile(s);
#pragma unroll
        for (int a = 0; a < 4; ++a) ni[a] = nj[a] = 0.0;
        int last_q0 = -1;
        for (int q0 = 0; q0 < kp.D; last_q0 = q0, q0 += KDC) {
            const int qc = stage_chunk(kp.D, q0, Xt1, ld1, i0, Xt2, ld2, j0, si, sj, t);
            accum_dot(si, sj, qc, ty, tx, s);
            if (MLP) accum_norms(si, sj, qc, ty, tx, ni, nj);
        }
        // MLP: qi = p_i + 1, hi = 1 / (2 (p_i + 1)); padded rows have x~ = 0, so every quantity below stays finite there
        double qi[4], qj[4], hi[4], hj[4];
        if (MLP) {
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                qi[a] = ni[a] + kp.bias + 1.0;
                qj[a] = nj[a] + kp.bias + 1.0;
                hi[a] = 0.5 / qi[a];
                hj[a] = 0.5 / qj[a];
            }
        }
        double cw[4][4];            // MLP: c
        double rsum[4], csum[4];    // MLP with ard: row / column sums of c s over this thread's 4 x 4 elements
#pragma unroll
        for (int a = 0; a < 4; ++a) rsum[a] = csum[a] = 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const long i = i0 + ty * 4 + a;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const long j = j0 + tx * 4 + b;
                const double g = grad_weight<FUSED, true>(i, j, n, m, G, ldg, alpha, Dy, sc, Mul, ldm);
                const double sb = s[a][b] + kp.bias;
                if (MLP) {
                    const double prod = qi[a] * qj[b];
                    const double c = coef * g / sqrt(fma(-sb, sb, prod));
                    const double cs = c * sb;
                    a_var = fma(g, mlp_k(kp.variance, sb, qi[a], qj[b]), a_var);
                    a_b += fma(-cs, hi[a] + hj[b], c);
                    if (qcnt > 0) {
                        rsum[a] += cs;
                        csum[b] += cs;
                    } else {
                        a_w += fma(-cs, ni[a] * hi[a] + nj[b] * hj[b], c * s[a][b]);
                    }
                    cw[a][b] = c;
                    if (!FUSED && Hout) store_h<false>(Hout, ldh, i, j, n, m, c, c);
                } else {
                    const double pm1 = (i < n && j < m) ? pow(sb, kp.power - 1.0) : 0.0;
                    const double h = coef * g * pm1;
                    a_var = fma(g, kp.variance * pm1 * sb, a_var);
                    a_b += h;
                    a_w = fma(h, s[a][b], a_w);
                }
            }
        }
        if (MLP && qcnt > 0) {
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                rsum[a] *= hi[a];
                csum[a] *= hj[a];
            }
            restage(last_q0, q_off, qcnt, Xt1, ld1, i0, Xt2, ld2, j0, si, sj, t);
#pragma unroll
            for (int q = 0; q < KDC; ++q) {
                if (q < qcnt) {
                    const d4 xi = *reinterpret_cast<const d4*>(si + q * KT + ty * 4);
                    const d4 xj = ld_xj(sj, q, tx);
                    double s1 = 0.0, s2 = 0.0;
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        double r = 0.0;
#pragma unroll
                        for (int b = 0; b < 4; ++b) r = fma(cw[a][b], xj[b], r);
                        s1 = fma(xi[a], r, s1);
                        s2 = fma(rsum[a], xi[a] * xi[a], s2);
                        s2 = fma(csum[a], xj[a] * xj[a], s2);
                    }
                    a_q[q] += s1 - s2;
                }
            }
        }
    }
    // deterministic block reduction -> partials[blockIdx][...]
    double* out = partials + (long)blockIdx.x * GP_STRIDE;
    const double sv = block_sum(t, a_var);
    if (t == 0) out[0] = sv;
    const double sb = block_sum(t, a_b);
    if (t == 0) out[1] = sb;
    if (qcnt == 0) {
        const double sw = block_sum(t, a_w);
        if (t == 0) out[2] = sw;
    }
#pragma unroll
    for (int q = 0; q < KDC; ++q) {
        if (q < qcnt) {
            const double sq = block_sum(t, a_q[q]);
            if (t == 0) out[2 + q] = sq;
        }
    }
}

static void launch_grad_dot(hipStream_t st, bool fused, KernParams kp, const double* Xt1, long ld1, long n, const double* Xt2,
                            long ld2, long m, const double* G, long ldg, const double* alpha, int Dy, long ntiles, int ntc,
                            double* partials, double* Hout, long ldh, const double* aa_scale, const double* Mul, long ldm) {
    const int nb = pick_grad_blocks(ntiles);
    const dim3 g((unsigned)nb), b(256);
    const bool mlp = kp.kind == MI355GP_MLP;
    for_each_group(kp.D, mlp && kp.ard, nb, partials, Hout, [&](int q_off, double* pa, double* h) {
#define GRAD_DOT(F, K)                                                                                                           \
    hipLaunchKernelGGL((k_grad_dot<F, K>), g, b, 0, st, kp, Xt1, ld1, n, Xt2, ld2, m, G, ldg, alpha, Dy, q_off, ntiles, ntc, pa, \
                       h, ldh, aa_scale, Mul, ldm)
        if (mlp) {
            if (fused) GRAD_DOT(true, MI355GP_MLP);
            else GRAD_DOT(false, MI355GP_MLP);
        } else {
            if (fused) GRAD_DOT(true, MI355GP_POLY);
            else GRAD_DOT(false, MI355GP_POLY);
        }
#undef GRAD_DOT
    });
}

// ------------------------------------------------------------------------------------------------
// The launch functions of the assembly and gradient kernels: each prepares its geometry, one dispatch picks the kind's kernel.
template <bool SYM>
static void launch_kbuild(hipStream_t st, long nblocks, const KbuildArgs& A) {
    const dim3 g((unsigned)nblocks), b(256);
    switch (A.kp.kind) {
    case MI355GP_RATQUAD: hipLaunchKernelGGL((k_kbuild_ext<SYM, MI355GP_RATQUAD>), g, b, 0, st, A); break;
    case MI355GP_STDPERIODIC: hipLaunchKernelGGL((k_kbuild_ext<SYM, MI355GP_STDPERIODIC>), g, b, 0, st, A); break;
    case MI355GP_COREGIONALIZE: hipLaunchKernelGGL((k_kbuild_coreg<SYM>), g, b, 0, st, A); break;
    case MI355GP_LINEAR: hipLaunchKernelGGL((k_kbuild_lin<SYM>), g, b, 0, st, A); break;
    case MI355GP_MLP: hipLaunchKernelGGL((k_kbuild_dot<SYM, MI355GP_MLP>), g, b, 0, st, A); break;
    case MI355GP_POLY: hipLaunchKernelGGL((k_kbuild_dot<SYM, MI355GP_POLY>), g, b, 0, st, A); break;
    case MI355GP_COSINE: hipLaunchKernelGGL((k_kbuild_ext<SYM, MI355GP_COSINE>), g, b, 0, st, A); break;
    case MI355GP_SINC: hipLaunchKernelGGL((k_kbuild_ext<SYM, MI355GP_SINC>), g, b, 0, st, A); break;
    case MI355GP_EXPQUADCOSINE: hipLaunchKernelGGL((k_kbuild_ext<SYM, MI355GP_EXPQUADCOSINE>), g, b, 0, st, A); break;
    default:
        hipLaunchKernelGGL((k_kbuild<SYM>), g, b, 0, st, A.kp, A.Xt1, A.ld1, A.n, A.Xt2, A.ld2, A.m, A.out, A.ldo, A.nrows_out, A.noise,
                           A.noise_len, A.jit, A.lower_only, A.add_diag, A.ntc, A.accumulate, A.diag_same, A.mul);
        break;
    }
}

void launch_kbuild_sym(hipStream_t st, KernParams kp, const double* Xt, long ldx, long n, long npad, double* A,
                       const double* noise, long noise_len, double jit, int lower_only, int add_diag, int accumulate,
                       const double* mul) {
    const int nt = (int)(npad / KT);
    launch_kbuild<true>(st, (long)nt * nt, KbuildArgs{kp, Xt, ldx, n, Xt, ldx, n, A, npad, npad, noise, noise_len, jit, lower_only,
                                                      add_diag, nt, accumulate, 0, mul});
}

void launch_kbuild_cross(hipStream_t st, KernParams kp, const double* Xt1, long ld1, long n, const double* Xt2,
                         long ld2, long m, double* Kout, long ldk, int accumulate, int diag_same, const double* mul) {
    const int ntr = (int)((n + KT - 1) / KT), ntc = (int)((m + KT - 1) / KT);
    launch_kbuild<false>(st, (long)ntr * ntc, KbuildArgs{kp, Xt1, ld1, n, Xt2, ld2, m, Kout, ldk, n, nullptr, 0, 0.0, 0, 0, ntc,
                                                         accumulate, diag_same, mul});
}

// fused: over the lower tiles of W (n x n); else over the ntiles = ntr * ntc tiles of G.  The sparse path's rank term (rk) is
// the stationary kernel's alone: that path has no other kind.
static void launch_grad(hipStream_t st, bool fused, KernParams kp, const double* Xt1, long ld1, long n, const double* Xt2, long ld2,
                        long m, int diag_same, const double* G, long ldg, const double* alpha, int Dy, long ntiles, int ntc,
                        double* partials, double* Hout, long ldh, const double* aa_scale, const double* Mul, long ldm,
                        RankTerm rk) {
    if (kp.kind == MI355GP_COREGIONALIZE) return;          // (launch_grad_coreg: records of its own shape)
    if (kp.kind >= MI355GP_RATQUAD) {
        if (rk.Y) return;
        const bool dot = kp.kind == MI355GP_MLP || kp.kind == MI355GP_POLY;
        auto family = dot ? launch_grad_dot : kp.kind == MI355GP_LINEAR ? launch_grad_lin : launch_grad_ext;
        family(st, fused, kp, Xt1, ld1, n, Xt2, ld2, m, G, ldg, alpha, Dy, ntiles, ntc, partials, Hout, ldh, aa_scale, Mul, ldm);
        return;
    }
    const dim3 g((unsigned)pick_grad_blocks(ntiles)), b(256);
    static const int force_old = !diag_env_int(DIAG_ENV("GRAD_TILEGEMM"), 1);   // MI355GP_GRAD_TILEGEMM=0: k_grad everywhere (A/B)
    const bool tilegemm = grad_tilegemm_applies(GradLaunchCase{fused, kp.kind, kp.ard, Mul != nullptr, Hout != nullptr,
                                                               rk.Y != nullptr, (uintptr_t)G, ldg, force_old});
    for_each_group(kp.D, kp.ard != 0, (int)g.x, partials, Hout, [&](int q_off, double* pa, double* h) {
        if (tilegemm) {
#define GRAD_TG(K) \
    hipLaunchKernelGGL((k_grad_tilegemm<K>), g, b, 0, st, kp, Xt1, ld1, n, G, ldg, alpha, Dy, q_off, ntiles, pa, aa_scale)
            if (kp.kind == MI355GP_RBF) GRAD_TG(MI355GP_RBF);
            else if (kp.kind == MI355GP_MATERN52) GRAD_TG(MI355GP_MATERN52);
            else GRAD_TG(MI355GP_MATERN32);
#undef GRAD_TG
            return;
        }
#define GRAD(F, A)                                                                                                              \
    hipLaunchKernelGGL((k_grad<F, A>), g, b, 0, st, kp, Xt1, ld1, n, Xt2, ld2, m, G, ldg, alpha, Dy, q_off, ntiles, ntc, pa, h, ldh, \
                       diag_same, aa_scale, Mul, ldm, rk)
        if (fused) {
            if (kp.ard) GRAD(true, true);
            else GRAD(true, false);
        } else {
            if (kp.ard) GRAD(false, true);
            else GRAD(false, false);
        }
#undef GRAD
    });
}

void launch_grad_fused(hipStream_t st, KernParams kp, const double* Xt, long ldx, long n, const double* W,
                       long ldw, const double* alpha, int Dy, double* partials, const double* aa_scale,
                       const double* Mul, long ldm) {
    const long nt = (n + KT - 1) / KT;
    launch_grad(st, true, kp, Xt, ldx, n, Xt, ldx, n, 0, W, ldw, alpha, Dy, nt * (nt + 1) / 2, (int)nt, partials, nullptr, 0,
                aa_scale, Mul, ldm, RankTerm{nullptr, nullptr, 0, 0.0, 1.0, nullptr});
}

void launch_grad_generic(hipStream_t st, KernParams kp, const double* Xt1, long ld1, long n, const double* Xt2,
                         long ld2, long m, int symmetric, const double* G, long ldg, double* partials,
                         double* Hout, long ldh, RankTerm rk) {
    const long ntr = (n + KT - 1) / KT, ntc = (m + KT - 1) / KT;
    launch_grad(st, false, kp, Xt1, ld1, n, Xt2, ld2, m, symmetric, G, ldg, nullptr, 0, ntr * ntc, (int)ntc, partials, Hout, ldh,
                nullptr, nullptr, 0, rk);
}

// ------------------------------------------------------------------------------------------------
// Laplace approximation (GPy/inference/latent_function_inference/laplace.py): the three passes over the resident K = kern.K(X)
// that one mode search and its gradients need.  They share nothing with the assembly kernels above but the tile size.
//
// B = I + diag(sw) K diag(sw) (laplace.py:333-334), sw = sqrt(W), lower 64-tiles into A (npad x npad); identity in the
// padding; `jit` (the jitchol ladder term) on the diagonal.  One read and one 32-byte store per four elements.
__global__ __launch_bounds__(256) void k_laplace_B(const double* __restrict__ K, long ld, long n, const double* __restrict__ sw,
                                                   double jit, int nt, double* __restrict__ A) {
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const long ti = blockIdx.x / nt, tj = blockIdx.x % nt;
    if (tj > ti) return;
    const long j0 = tj * KT + tx * 4;
    double wj[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) wj[b] = (j0 + b < n) ? sw[j0 + b] : 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const long i = ti * KT + ty * 4 + a;
        const double wi = (i < n) ? sw[i] : 0.0;
        const d4 k = *reinterpret_cast<const d4*>(K + i * ld + j0);
        d4 o;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const long j = j0 + b;
            double v = (i < n && j < n) ? wi * k[b] * wj[b] : 0.0;
            if (i == j) v += (i < n) ? 1.0 + jit : 1.0;
            o[b] = v;
        }
        *reinterpret_cast<d4*>(A + i * ld + j0) = o;
    }
}
void launch_laplace_B(hipStream_t st, const double* K, long npad, long n, const double* sw, double jit, double* A) {
    const int nt = (int)(npad / KT);
    hipLaunchKernelGGL(k_laplace_B, dim3((unsigned)((long)nt * nt)), dim3(256), 0, st, K, npad, n, sw, jit, nt, A);
}

// y = K v for NV right-hand sides from the LOWER 64-tiles of the symmetric resident K: every tile is read once (4 N^2 bytes) and
// serves both its rows (y_i += K_ij v_j, j <= i) and, transposed, its columns (y_j += K_ij v_i, i > j).  Block = (row chunk c
// of 64 rows, segment s of SYMV_SEG tiles of that chunk's tile row): the row sums of the segment go to rowpart[s][i], the column
// sums of every tile to colpart[c][j]; k_symv_finish adds them in a fixed order: bit reproducible.  The next tile's four
// 32-byte loads per lane are issued before the current tile's arithmetic (eight loads in flight per lane).
#define SYMV_SEG 8
template <int NV>
__global__ __launch_bounds__(256) void k_symv_lower(const double* __restrict__ K, long ld, long n, const double* __restrict__ v0,
                                                    const double* __restrict__ v1, double* __restrict__ rowpart,
                                                    double* __restrict__ colpart) {
    __shared__ double red[NV][16][KT + 1];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const long c = blockIdx.x, s = blockIdx.y;
    const long tj0 = s * SYMV_SEG;
    if (tj0 > c) return;
    const long tj1 = (tj0 + SYMV_SEG - 1 < c) ? tj0 + SYMV_SEG - 1 : c;      // inclusive
    const long i0 = c * KT + ty * 4;
    const double* vv[2] = {v0, v1};
    double vi[NV][4], racc[NV][4];
#pragma unroll
    for (int r = 0; r < NV; ++r)
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            vi[r][a] = (i0 + a < n) ? vv[r][i0 + a] : 0.0;
            racc[r][a] = 0.0;
        }
    d4 cur[4], nxt[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) cur[a] = *reinterpret_cast<const d4*>(K + (i0 + a) * ld + tj0 * KT + tx * 4);
    for (long tj = tj0; tj <= tj1; ++tj) {
        if (tj < tj1) {
#pragma unroll
            for (int a = 0; a < 4; ++a) nxt[a] = *reinterpret_cast<const d4*>(K + (i0 + a) * ld + (tj + 1) * KT + tx * 4);
        }
        const long j0 = tj * KT + tx * 4;
        const bool diag = (tj == c);
        double vj[NV][4], cs[NV][4];
#pragma unroll
        for (int r = 0; r < NV; ++r)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                vj[r][b] = (j0 + b < n) ? vv[r][j0 + b] : 0.0;
                cs[r][b] = 0.0;
            }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const double k = cur[a][b];
                const bool lower = !diag || (j0 + b <= i0 + a), strict = !diag || (j0 + b < i0 + a);
#pragma unroll
                for (int r = 0; r < NV; ++r) {
                    if (lower) racc[r][a] = fma(k, vj[r][b], racc[r][a]);
                    if (strict) cs[r][b] = fma(k, vi[r][a], cs[r][b]);
                }
            }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < NV; ++r)
#pragma unroll
            for (int b = 0; b < 4; ++b) red[r][ty][tx * 4 + b] = cs[r][b];
        __syncthreads();
        if (t < KT * NV) {
            const int r = t / KT, col = t % KT;
            double sum = 0.0;
#pragma unroll
            for (int g = 0; g < 16; ++g) sum += red[r][g][col];
            colpart[((long)r * gridDim.x + c) * ld + tj * KT + col] = sum;
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) cur[a] = nxt[a];
    }
    // row sums of the segment: the 16 column groups of a row in a fixed order
    __syncthreads();
#pragma unroll
    for (int r = 0; r < NV; ++r)
#pragma unroll
        for (int a = 0; a < 4; ++a) red[r][tx][ty * 4 + a] = racc[r][a];
    __syncthreads();
    if (t < KT * NV) {
        const int r = t / KT, row = t % KT;
        double sum = 0.0;
#pragma unroll
        for (int g = 0; g < 16; ++g) sum += red[r][g][row];
        rowpart[((long)r * gridDim.y + s) * ld + c * KT + row] = sum;
    }
}
// y_j = sum over the segments of j's chunk of rowpart + sum over the chunks c >= j / 64 of colpart, both in ascending order
__global__ void k_symv_finish(const double* __restrict__ rowpart, const double* __restrict__ colpart, long ld, long n, int nchunks,
                              int nsegmax, double* __restrict__ y0, double* __restrict__ y1) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int r = blockIdx.y;
    const long cj = j / KT;
    double sum = 0.0;
    for (long s = 0; s * SYMV_SEG <= cj; ++s) sum += rowpart[((long)r * nsegmax + s) * ld + j];
    for (long c = cj; c < nchunks; ++c) sum += colpart[((long)r * nchunks + c) * ld + j];
    (r == 0 ? y0 : y1)[j] = sum;
}
size_t symv_part_doubles(long npad) {
    const long nchunks = npad / KT, nseg = (nchunks + SYMV_SEG - 1) / SYMV_SEG;
    return (size_t)2 * (size_t)(nchunks + nseg) * (size_t)npad;
}
void launch_symv_lower(hipStream_t st, const double* K, long npad, long n, const double* v0, const double* v1, double* y0,
                       double* y1, double* part) {
    const int nchunks = (int)((n + KT - 1) / KT), nseg = (nchunks + SYMV_SEG - 1) / SYMV_SEG, nv = v1 ? 2 : 1;
    double* rowpart = part;
    double* colpart = part + (size_t)2 * nseg * npad;
    if (nv == 2)
        hipLaunchKernelGGL((k_symv_lower<2>), dim3((unsigned)nchunks, (unsigned)nseg), dim3(256), 0, st, K, npad, n, v0, v1, rowpart,
                           colpart);
    else
        hipLaunchKernelGGL((k_symv_lower<1>), dim3((unsigned)nchunks, (unsigned)nseg), dim3(256), 0, st, K, npad, n, v0, v0, rowpart,
                           colpart);
    hipLaunchKernelGGL(k_symv_finish, dim3((unsigned)((n + 255) / 256), (unsigned)nv), dim3(256), 0, st, rowpart, colpart, npad, n,
                       nchunks, nseg, y0, y1);
}

// The symmetrised dL_dK of the Laplace approximation (laplace.py:260-272) from Binv = B^-1 (lower tiles, lauum) into G, BOTH
// triangles (launch_grad_generic reads every element):
//   G_ij = 0.5 (a_i a_j - sw_i Binv_ij sw_j) + 0.5 (a_i u_j + u_i a_j),   a = Ki_f,  u = dL_dfhat - K_Wi_i K dL_dfhat
// One block per lower 64-tile: the tile is read once, written row-wise, and its mirror is written row-wise from LDS.
__global__ __launch_bounds__(256) void k_laplace_dLdK(const double* __restrict__ Binv, long ld, long n,
                                                      const double* __restrict__ sw, const double* __restrict__ a,
                                                      const double* __restrict__ u, int nt, double* __restrict__ G) {
    __shared__ double tile[KT][KT + 1];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const long ti = blockIdx.x / nt, tj = blockIdx.x % nt;
    if (tj > ti) return;
    const long i0 = ti * KT, j0 = tj * KT;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long i = i0 + ty * 4 + r;
        const d4 bi = *reinterpret_cast<const d4*>(Binv + i * ld + j0 + tx * 4);
        const double ai = (i < n) ? a[i] : 0.0, ui = (i < n) ? u[i] : 0.0, wi = (i < n) ? sw[i] : 0.0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const long j = j0 + tx * 4 + b;
            double v = 0.0;
            if (i < n && j < n) {
                const double aj = a[j], uj = u[j];
                v = 0.5 * (ai * aj - wi * bi[b] * sw[j]) + 0.5 * (ai * uj + ui * aj);
            }
            tile[ty * 4 + r][tx * 4 + b] = v;
        }
    }
    __syncthreads();
    const bool diag = (ti == tj);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int li = ty * 4 + r;
        d4 o, m;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int lj = tx * 4 + b;
            o[b] = (diag && lj > li) ? tile[lj][li] : tile[li][lj];      // diagonal tile: the lower triangle on both sides
            m[b] = tile[lj][li];
        }
        *reinterpret_cast<d4*>(G + (i0 + li) * ld + j0 + tx * 4) = o;
        if (!diag) *reinterpret_cast<d4*>(G + (j0 + li) * ld + i0 + tx * 4) = m;
    }
}
void launch_laplace_dLdK(hipStream_t st, const double* Binv, long npad, long n, const double* sw, const double* a,
                         const double* u, double* G) {
    const int nt = (int)(npad / KT);
    hipLaunchKernelGGL(k_laplace_dLdK, dim3((unsigned)((long)nt * nt)), dim3(256), 0, st, Binv, npad, n, sw, a, u, nt, G);
}

// ------------------------------------------------------------------------------------------------
// Variational Gaussian approximation (GPy/inference/latent_function_inference/var_gauss.py): the passes of one backward over
// Ai = (I + diag(beta) K diag(beta))^-1, P1 = Ai Ai, P2 = Ai diag(beta^-2) Ai and the resident K.  Written like k_laplace_dLdK:
// one block per lower 64-tile, 32-byte loads, the mirror written from LDS.
//
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

// A symmetric matrix held in its lower triangle (lower 64-tiles, and the lower triangle of the diagonal tiles) -> both
// triangles, in place: what the full-tile Gram products of the backward read.  A block reads its own tile only and writes
// the mirrored one (or, on the diagonal, its own upper triangle), so no block reads what another writes.
__global__ __launch_bounds__(256) void k_vg_mirror(double* __restrict__ A, long ld, int nt) {
    __shared__ double tile[KT][KT + 1];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const long ti = blockIdx.x / nt, tj = blockIdx.x % nt;
    if (tj > ti) return;
    const long i0 = ti * KT, j0 = tj * KT;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const d4 x = *reinterpret_cast<const d4*>(A + (i0 + ty * 4 + r) * ld + j0 + tx * 4);
#pragma unroll
        for (int b = 0; b < 4; ++b) tile[ty * 4 + r][tx * 4 + b] = x[b];
    }
    __syncthreads();
    const bool diag = (ti == tj);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int li = ty * 4 + r;
        d4 o;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int lj = tx * 4 + b;
            o[b] = (diag && lj <= li) ? tile[li][lj] : tile[lj][li];
        }
        if (diag) *reinterpret_cast<d4*>(A + (i0 + li) * ld + j0 + tx * 4) = o;
        else *reinterpret_cast<d4*>(A + (j0 + li) * ld + i0 + tx * 4) = o;
    }
}
void launch_vg_mirror(hipStream_t st, double* A, long npad) {
    const int nt = (int)(npad / KT);
    hipLaunchKernelGGL(k_vg_mirror, dim3((unsigned)((long)nt * nt)), dim3(256), 0, st, A, npad, nt);
}

// First pass, while Ai is intact.  H holds P1 (lower tiles read) and receives, in place, the part of the symmetrised dL_dK
// that needs Ai and P1:
//   H_ij = 0.5 (alpha_i g_j + g_i alpha_j) - 0.5 (alpha_i alpha_j + beta_i beta_j (Ai_ij - P1_ij)),   g = dF_dm
// and every tile leaves the partial sums of the two beta gradients (var_gauss.py:51,57), f1 = Sigma_ij^2 weighted by
// v = dF_dv and f2 = K_ij (Ai - P1)_ij weighted by beta, over its rows for its 64 columns (cp[q][ti][j]) and, transposed,
// over its columns for its 64 rows (rp[q][tj][i]; the diagonal tile: lower / strictly lower, as k_symv_lower):
//   Sigma_ij = -Ai_ij / (beta_i beta_j) off the diagonal, Sigma_ii = var_i (the forward's cancellation-free diag Sigma).
// k_vg_finish_vec adds the partials in a fixed order: no atomics, two calls give the same bytes.
__global__ __launch_bounds__(256) void k_vg_assemble(const double* __restrict__ Ai, const double* __restrict__ K, long ld, long n,
                                                     const double* __restrict__ beta, const double* __restrict__ alpha,
                                                     const double* __restrict__ g, const double* __restrict__ v,
                                                     const double* __restrict__ var, int nt, int scaled, double* __restrict__ H,
                                                     double* __restrict__ cp, double* __restrict__ rp) {
    __shared__ double red[2][16][KT + 1];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const long ti = blockIdx.x / nt, tj = blockIdx.x % nt;
    if (tj > ti) return;
    const long i0 = ti * KT + ty * 4, j0 = tj * KT + tx * 4;
    const bool diag = (ti == tj);
    double bj[4], aj[4], gj[4], vj[4], cs1[4], cs2[4], rs1[4], rs2[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const bool in = j0 + b < n;
        bj[b] = in ? beta[j0 + b] : 0.0;
        aj[b] = in ? alpha[j0 + b] : 0.0;
        gj[b] = in ? g[j0 + b] : 0.0;
        vj[b] = in ? v[j0 + b] : 0.0;
        cs1[b] = cs2[b] = 0.0;
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const long i = i0 + a;
        const bool in_i = i < n;
        const double bi = in_i ? beta[i] : 0.0, ai = in_i ? alpha[i] : 0.0, gi = in_i ? g[i] : 0.0, vi = in_i ? v[i] : 0.0;
        const double si = in_i ? var[i] : 0.0;
        const d4 x = *reinterpret_cast<const d4*>(Ai + i * ld + j0);
        const d4 p = *reinterpret_cast<const d4*>(H + i * ld + j0);
        const d4 k = *reinterpret_cast<const d4*>(K + i * ld + j0);
        d4 o;
        double r1 = 0.0, r2 = 0.0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const long j = j0 + b;
            double h = 0.0;
            if (in_i && j < n) {
                const double d = x[b] - p[b], bb = bi * bj[b];
                h = 0.5 * (ai * gj[b] + gi * aj[b]) - 0.5 * (ai * aj[b] + bb * d);
                if (scaled) h /= bb;                                 // the exact form accumulates its Gram products onto H / (beta_i beta_j)
                const double s = (i == j) ? si : x[b] / bb;
                const double f1 = s * s, f2 = k[b] * d;
                if (!diag || j <= i) {
                    cs1[b] = fma(f1, vi, cs1[b]);
                    cs2[b] = fma(f2, bi, cs2[b]);
                }
                if (!diag || j < i) {
                    r1 = fma(f1, vj[b], r1);
                    r2 = fma(f2, bj[b], r2);
                }
            }
            o[b] = h;
        }
        *reinterpret_cast<d4*>(H + i * ld + j0) = o;
        rs1[a] = r1;
        rs2[a] = r2;
    }
    // column sums: the 16 row groups of a column in a fixed order
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        red[0][ty][tx * 4 + b] = cs1[b];
        red[1][ty][tx * 4 + b] = cs2[b];
    }
    __syncthreads();
    if (t < 2 * KT) {
        const int q = t / KT, col = t % KT;
        double sum = 0.0;
#pragma unroll
        for (int r = 0; r < 16; ++r) sum += red[q][r][col];
        cp[((long)q * nt + ti) * ld + tj * KT + col] = sum;
    }
    __syncthreads();
    // row sums: the 16 column groups of a row in a fixed order
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        red[0][tx][ty * 4 + a] = rs1[a];
        red[1][tx][ty * 4 + a] = rs2[a];
    }
    __syncthreads();
    if (t < 2 * KT) {
        const int q = t / KT, row = t % KT;
        double sum = 0.0;
#pragma unroll
        for (int r = 0; r < 16; ++r) sum += red[q][r][row];
        rp[((long)q * nt + tj) * ld + ti * KT + row] = sum;
    }
}
// beta.gradient_j = -2 beta_j S1_j - S2_j with S_j = the column partials of the tiles below j's chunk + the row partials of the
// tiles left of it, both ascending (var_gauss.py:51,57,60);  alpha.gradient_j = (K dF_dm)_j - m_j (:48,59)
__global__ void k_vg_finish_vec(const double* __restrict__ cp, const double* __restrict__ rp, long ld, long n, int nt,
                                const double* __restrict__ beta, const double* __restrict__ Kg, const double* __restrict__ m,
                                double* __restrict__ dalpha, double* __restrict__ dbeta) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const long cj = j / KT;
    double s[2];
    for (int q = 0; q < 2; ++q) {
        double sum = 0.0;
        for (long ti = cj; ti < nt; ++ti) sum += cp[((long)q * nt + ti) * ld + j];
        for (long tj = 0; tj <= cj; ++tj) sum += rp[((long)q * nt + tj) * ld + j];
        s[q] = sum;
    }
    dbeta[j] = -2.0 * beta[j] * s[0] - s[1];
    dalpha[j] = Kg[j] - m[j];
}
// Second pass: G = H + 0.5 (v_i + v_j) beta_i beta_j P2_ij from the lower tiles of H and P2, into BOTH triangles of H's buffer
// (launch_grad_generic reads every element); the upper triangle is the copy of the lower one, so G is bitwise symmetric
// exact != 0: G's buffer holds G_ij / (beta_i beta_j) in its lower tiles (launch_vg_assemble with scaled, then the Gram products of
// the exact form accumulated onto it) and is multiplied back; P2 is not read
__global__ __launch_bounds__(256) void k_vg_dLdK(const double* __restrict__ P2, long ld, long n, const double* __restrict__ beta,
                                                 const double* __restrict__ v, int nt, int exact, double* __restrict__ G) {
    __shared__ double tile[KT][KT + 1];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const long ti = blockIdx.x / nt, tj = blockIdx.x % nt;
    if (tj > ti) return;
    const long i0 = ti * KT, j0 = tj * KT;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long i = i0 + ty * 4 + r;
        const d4 h = *reinterpret_cast<const d4*>(G + i * ld + j0 + tx * 4);
        d4 p = {0.0, 0.0, 0.0, 0.0};
        if (!exact) p = *reinterpret_cast<const d4*>(P2 + i * ld + j0 + tx * 4);
        const double bi = (i < n) ? beta[i] : 0.0, vi = (i < n) ? v[i] : 0.0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const long j = j0 + tx * 4 + b;
            double val = 0.0;
            if (i < n && j < n) val = exact ? h[b] * (bi * beta[j]) : h[b] + 0.5 * (vi + v[j]) * (bi * beta[j]) * p[b];
            tile[ty * 4 + r][tx * 4 + b] = val;
        }
    }
    __syncthreads();
    const bool diag = (ti == tj);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int li = ty * 4 + r;
        d4 o, m;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int lj = tx * 4 + b;
            o[b] = (diag && lj > li) ? tile[lj][li] : tile[li][lj];      // diagonal tile: the lower triangle on both sides
            m[b] = tile[lj][li];
        }
        *reinterpret_cast<d4*>(G + (i0 + li) * ld + j0 + tx * 4) = o;
        if (!diag) *reinterpret_cast<d4*>(G + (j0 + li) * ld + i0 + tx * 4) = m;
    }
}
size_t vg_part_doubles(long npad) { return (size_t)4 * (size_t)(npad / KT) * (size_t)npad; }
void launch_vg_assemble(hipStream_t st, const double* Ai, const double* K, long npad, long n, const double* beta,
                        const double* alpha, const double* g, const double* v, const double* var, int scaled, double* H, double* part) {
    const int nt = (int)(npad / KT);
    double* cp = part;
    double* rp = part + (size_t)2 * nt * npad;
    hipLaunchKernelGGL(k_vg_assemble, dim3((unsigned)((long)nt * nt)), dim3(256), 0, st, Ai, K, npad, n, beta, alpha, g, v, var, nt,
                       scaled, H, cp, rp);
}
void launch_vg_finish_vec(hipStream_t st, const double* part, long npad, long n, const double* beta, const double* Kg,
                          const double* m, double* dalpha, double* dbeta) {
    const int nt = (int)(npad / KT);
    hipLaunchKernelGGL(k_vg_finish_vec, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part, part + (size_t)2 * nt * npad,
                       npad, n, nt, beta, Kg, m, dalpha, dbeta);
}
void launch_vg_dLdK(hipStream_t st, const double* P2, long npad, long n, const double* beta, const double* v, int exact, double* G) {
    const int nt = (int)(npad / KT);
    hipLaunchKernelGGL(k_vg_dLdK, dim3((unsigned)((long)nt * nt)), dim3(256), 0, st, P2, npad, n, beta, v, nt, exact, G);
}
// Out[i][j] = M[i][j] sqrt(max(sign v_i, 0)) / |beta_i| for i < rows, 0 for rows <= i < allrows (cols wide, ld shared): the factor R
// of Ai diag(max(sign v, 0) / beta^2) Ai = R^T R, one per sign of dF_dv
__global__ void k_vg_rowscale_v(const double* __restrict__ M, long ld, long rows, long cols, const double* __restrict__ v,
                                const double* __restrict__ beta, double sign, double* __restrict__ Out) {
    const long j = (long)blockIdx.y * blockDim.x + threadIdx.x, i = blockIdx.x;
    if (j >= cols) return;
    double s = 0.0;
    if (i < rows) {
        const double w = sign * v[i];
        s = w > 0.0 ? sqrt(w) / fabs(beta[i]) : 0.0;
    }
    Out[i * ld + j] = s != 0.0 ? M[i * ld + j] * s : 0.0;
}
void launch_vg_rowscale_v(hipStream_t st, const double* M, long ld, long rows, long allrows, long cols, const double* v,
                          const double* beta, double sign, double* Out) {
    hipLaunchKernelGGL(k_vg_rowscale_v, dim3((unsigned)allrows, (unsigned)((cols + 255) / 256)), dim3(256), 0, st, M, ld, rows, cols, v,
                       beta, sign, Out);
}
