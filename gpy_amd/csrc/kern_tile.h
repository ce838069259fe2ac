// kern_tile.h -- what a covariance tile kernel is built from: the tile geometry, the stationary covariance functions, the
// LDS staging of the input slabs, the K-build skeleton (KbuildArgs, kbuild_tile, kbuild_pad, kbuild_store_row) and the shared
// pieces of the gradient reductions (grad_tile, restage, grad_weight, store_h, block_sum).  Included by the covariance
// translation units alone: kern.hip (stationary kinds, dispatch), kern_families.hip (every other kind) and kern_sparse.hip
// (the streaming sparse path).  The launchers that kern.hip's dispatch reaches in kern_families.hip are declared at the end.
#pragma once
#include <cstdint>

#include "../../include/mi355gp.h"
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
// Every kind has a kernel of its own (k_kbuild in kern.hip for the stationary and static kinds, the others in
// kern_families.hip) that holds only what is the kind's: what it stages, what it accumulates over the staged slabs, how an
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

// ------------------------------------------------------------------------------------------------
// Gradient reduction.  For every (i, j): g = weight * dL_dK[i][j];
//   acc_var += g*K ; acc_iso += g*(dK/dr*r) ; acc_q += g*(dK/dr / r)*(x~_iq - x~_jq)^2   (x~ = x / l)
// FUSED: dL_dK = 0.5*(alpha_i . alpha_j - Dy*W_ij) from the lower triangle of W (off-diagonal weight 2).
// else : dL_dK read from G (n x m).
// Per-block partials [2 + 32]: [0] var, [1] iso, [2+q] lengthscale dims q_off..q_off+31.
// As for the assembly, every kind has a kernel of its own (k_grad in kern.hip, the others in kern_families.hip) around shared inlined
// pieces: grad_tile, stage_chunk / restage, grad_weight, store_h, block_sum, and -- what every gradient kernel used to write
// out for itself -- grad_qcnt, grad_aa_scale, for_each_dim and grad_put / grad_put_dims.

// What a gradient kernel is launched with, the counterpart of KbuildArgs.  The kernels of kern_families.hip take it as their
// one parameter; k_grad and k_grad_tilegemm (kern.hip) keep parameter lists of their own, as k_kbuild does.
struct GradArgs {
    KernParams kp;
    const double* Xt1;                 // row side: dimension-major inputs [D][ld1], n points
    long ld1, n;
    const double* Xt2;                 // column side, m points (the row side again in the fused form)
    long ld2, m;
    const double* G;                   // fused: W = Ky^-1, lower triangle read; else dL_dK (n x m)
    long ldg;
    const double* alpha;               // fused only: n x Dy
    int Dy;
    long ntiles;
    int ntc;
    double* partials;                  // the records of this launch's group, one per block
    double* Hout;                      // (generic form, may alias G) the weights of the gradients_X reductions, or null
    long ldh;
    const double* aa_scale;            // (fused, optional, device) factor on the alpha alpha^T term: Student-t process
    const double* Mul;                 // (optional) the other factors' covariances of a product kernel
    long ldm;
    int q_off;                         // first dimension of this launch's group: what for_each_group sets per launch, and
                                       // with it the group's `partials` and whether this launch is the one that stores Hout
};

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

// both for a kernel that holds its arguments as GradArgs
__device__ __forceinline__ int stage_chunk(const GradArgs& A, int q0, long i0, long j0, double* si, double* sj, int t) {
    return stage_chunk(A.kp.D, q0, A.Xt1, A.ld1, i0, A.Xt2, A.ld2, j0, si, sj, t);
}
__device__ __forceinline__ void restage(const GradArgs& A, int last_q0, int qcnt, long i0, long j0, double* si, double* sj, int t) {
    restage(last_q0, A.q_off, qcnt, A.Xt1, A.ld1, i0, A.Xt2, A.ld2, j0, si, sj, t);
}

// The dimensions a launch reduces: those of the group from q_off (at most 32) for a kind that reduces per dimension, none otherwise
__device__ __forceinline__ int grad_qcnt(bool perdim, int D, int q_off) {
    return perdim ? ((D - q_off < KDC) ? (D - q_off) : KDC) : 0;
}

// sc of grad_weight: the factor on alpha alpha^T
template <bool FUSED>
__device__ __forceinline__ double grad_aa_scale(const double* __restrict__ aa_scale) {
    return (FUSED && aa_scale) ? aa_scale[0] : 1.0;
}

// The weight dL_dK of element (i, j), 0 outside n x m.
//   FUSED: 0.5 (sc * alpha_i . alpha_j - Dy * W_ij) from the lower triangle of W = Ky^-1 (G), j <= i only; sc = 1 for the Gaussian
//          process, (nu+N)/(nu+beta-2) for the Student-t process (exact_studentt_inference.py:46).  With TWICE an element below
//          the diagonal counts for its mirror image as well.
//   else : G[i][j].
//   Mul  : factor of a product kernel -- dL_dK times the other factors' covariances (prod.py:86-99).  !TWICE (Coregionalize, which
//          completes symmetrically on its own) takes it on the elements j <= i of the fused form alone.
template <bool FUSED, bool TWICE>
__device__ __forceinline__ double grad_weight(const GradArgs& A, long i, long j, double sc) {
    double g = 0.0;
    if (i < A.n && j < A.m) {
        if (FUSED) {
            if (j <= i) {
                double aa = 0.0;
                for (int d = 0; d < A.Dy; ++d) aa = fma(A.alpha[i * A.Dy + d], A.alpha[j * A.Dy + d], aa);
                g = 0.5 * (sc * aa - (double)A.Dy * A.G[i * A.ldg + j]);
                if (TWICE) {
                    if (j < i) g *= 2.0;
                } else if (A.Mul) {
                    g *= A.Mul[i * A.ldm + j];
                }
            }
        } else {
            g = A.G[i * A.ldg + j];
        }
        if (TWICE && A.Mul) g *= A.Mul[i * A.ldm + j];
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

// The walk of a per-dimension reduction over the (re)staged slabs: body(q, xi, xj) for every q < qcnt with the thread's four row
// values and four column values of dimension q.  Unrolled over the 32 dimensions of a chunk, so that an accumulator array
// indexed by q stays in registers.
template <class Body>
__device__ __forceinline__ void for_each_dim(const double* si, const double* sj, int qcnt, int ty, int tx, Body body) {
#pragma unroll
    for (int q = 0; q < KDC; ++q)
        if (q < qcnt) body(q, *reinterpret_cast<const d4*>(si + q * KT + ty * 4), ld_xj(sj, q, tx));
}

// The epilogue: the block's sum of one accumulator goes to rec[slot]; of a per-dimension array, to rec[2 + q] for q < qcnt
__device__ __forceinline__ void grad_put(double* __restrict__ rec, int slot, int t, double v) {
    const double s = block_sum(t, v);
    if (t == 0) rec[slot] = s;
}
__device__ __forceinline__ void grad_put_dims(double* __restrict__ rec, int qcnt, int t, const double (&a)[KDC]) {
#pragma unroll
    for (int q = 0; q < KDC; ++q)
        if (q < qcnt) grad_put(rec, 2 + q, t, a[q]);
}
// two arrays to two records, dimension by dimension (neither array stays live through the other's 32 block sums)
__device__ __forceinline__ void grad_put_dims(double* __restrict__ recA, double* __restrict__ recB, int qcnt, int t,
                                              const double (&a)[KDC], const double (&b)[KDC]) {
#pragma unroll
    for (int q = 0; q < KDC; ++q)
        if (q < qcnt) {
            grad_put(recA, 2 + q, t, a[q]);
            grad_put(recB, 2 + q, t, b[q]);
        }
}

inline int pick_grad_blocks(long ntiles) { return (int)((ntiles < 2048) ? ntiles : 2048); }

// One launch per group of 32 dimensions for a kind that reduces per dimension (ARD), one launch otherwise: launch(g) with g = A
// but for q_off and what follows from it -- the records of group gidx at partials + gidx * nb * GP_STRIDE, and Hout, which may
// alias G (in place) that every launch reads: only the LAST group's launch gets it.
template <class Launch>
inline void for_each_group(bool perdim, int nb, const GradArgs& A, Launch launch) {
    if (!perdim) {
        launch(A);
        return;
    }
    for (int q_off = 0, gidx = 0; q_off < A.kp.D; q_off += KDC, ++gidx) {
        GradArgs g = A;
        g.q_off = q_off;
        g.partials = A.partials + (long)gidx * nb * GP_STRIDE;
        g.Hout = (q_off + KDC >= A.kp.D) ? A.Hout : nullptr;
        launch(g);
    }
}

// nb blocks of one kind's gradient kernel: its FUSED instantiation or the generic one
inline void launch_grad_kernel(hipStream_t st, bool fused, int nb, const GradArgs& A, void (*k_fused)(GradArgs),
                               void (*k_generic)(GradArgs)) {
    hipLaunchKernelGGL(fused ? k_fused : k_generic, dim3((unsigned)nb), dim3(256), 0, st, A);
}

// ------------------------------------------------------------------------------------------------
// kern_families.hip: per family, the K build of one kind (sym: the padded symmetric form) and its gradient pass (one launch
// per group of dimensions; A.q_off is theirs to set).  kern.hip's launch_kbuild / launch_grad pick the family.
void launch_kbuild_ext(hipStream_t st, bool sym, long nblocks, const KbuildArgs& A);
void launch_kbuild_coreg(hipStream_t st, bool sym, long nblocks, const KbuildArgs& A);
void launch_kbuild_lin(hipStream_t st, bool sym, long nblocks, const KbuildArgs& A);
void launch_kbuild_dot(hipStream_t st, bool sym, long nblocks, const KbuildArgs& A);
void launch_grad_ext(hipStream_t st, bool fused, const GradArgs& A);
void launch_grad_lin(hipStream_t st, bool fused, const GradArgs& A);
void launch_grad_dot(hipStream_t st, bool fused, const GradArgs& A);
