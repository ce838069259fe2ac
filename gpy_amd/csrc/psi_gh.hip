// psi_gh.hip -- psi-statistics by Gauss-Hermite quadrature for one stationary part of kind ExpQuad, Matern52, Matern32 or
// Exponential / OU (the r-functions cov_k / cov_all of kern_tile.h), and their gradients.  Restates (does not port)
// GPy/kern/src/psi_comp/gaussherm.py:17-101.  With nodes t_i, weights w_i, X(i) = mu + t_i sqrt(S) -- the same node in every
// dimension: the reference's rule, which for D > 1 is not a tensor quadrature -- and K_i = K(X(i), Z):
//   psi0[n] = sum_i w_i Kdiag = variance sum_i w_i     psi1 = sum_i w_i K_i     psi2 = sum_i w_i K_i^T K_i
//   G_i = w_i (dL_dpsi1 + K_i D2), D2 = dL_dpsi2 + dL_dpsi2^T;  the kernel's update_gradients_full / gradients_X of G_i at
//   (X(i), Z), summed over i;  dmu = sum_i dX_i,  dS = sum_i dX_i t_i / (2 sqrt(S)).
// Everything works on scaled coordinates x~ = x / l_q (il_q = 0 on a dimension the part does not see); squared distances are
// sums of squared differences, never the expanded form.
//
// WHY NOT gemm_tile_128.  psi2 is a Gram matrix over the (row, node) pairs and T_i = K_i D2 is a tile product, but gemm_tile's
// operands are LOADED (LDS-DMA from row-major buffers); here the K_i tiles are GENERATED, H = 11 of them per row, and writing them
// out first would be the N x M x H array this file exists to avoid.  So both kernels produce K_i in LDS and feed
// v_mfma_f64_16x16x4_f64 from there.
//
// k_gh_stats -- grid (lower pairs (ti, tj) of GH_MT = 64 column tiles, row splits), 256 threads = 4 waves.  Per row block of
//   GH_RB = 16 rows and per node the workgroup generates the 16 x 64 tiles A = K_i[:, ti] and B = K_i[:, tj] (one tile on the
//   diagonal) into LDS, thread = one column x 4 rows (a wave's 64 lanes write 64 consecutive doubles of one row).  psi1 accumulates
//   w_i K_i over the nodes in the generating thread's registers (workgroups with tj == 0 store it).  psi2's contraction index is the
//   (row, node) pair: 16 rows = four MFMA k-steps, wave w owns rows 16 w .. of the 64 x 64 result and all four column tiles,
//   acc[j] += (w_i A)^T B with the weight applied to the A fragment on its way out of LDS.  LDS layout: tile[row][GH_LDK = 80]; an
//   MFMA fragment read takes, for k = lane >> 4, 16 consecutive doubles of row k: with rows 80 doubles = 160 dwords apart, rows k
//   and k + 1 lie 32 dwords (mod 64) apart, so the two rows a half-wave of a 64-bit read touches fall on complementary halves of
//   the banks and the 16 doubles of one row on distinct ones: no conflict under a 32- or a 64-bank model.  Registers: 16 accumulator
//   + 4 psi1 doubles = 40 VGPRs of state; the compiler reports 122 VGPRs, 4 waves / SIMD, no scratch, no spill.
//   LDS: 2 x 16 x 80 + 2 x 16 x D doubles (36 KB at D = 64).
//   Row splits land in part[split][mp][mp]; launch_psi2_combine sums them in split order reading the lower triangle for both
//   positions: psi2 is bitwise symmetric and reproducible.  Cost of the simple ownership: the tiles of K_i are generated once per
//   tile PAIR, (nt + 1) / 2 times more often than necessary (nt = M / 64); at M = 256 that is 2.5x on the exp-bound part.
//
// k_gh_grad -- grid (row blocks of GH_RB = 16 rows), 256 threads.  The block keeps three 16 x mp operands, [column][16] so that an
//   MFMA A fragment (16 rows of one column per k) is 64 consecutive doubles: K_i (kb), dK/dr / r and then W (db), and dL_dpsi1 (gl,
//   formed once per block from the matrix or the rank form beta R v^T).  They live in LDS while 48 (mp + D) doubles fit in 144 KB
//   (mp <= 320 at D = 64), else in a per-workgroup slice of a global scratch (16 x mp x 3: not an N x M x H array) -- the template
//   parameter picks the address space.  Per node: (1) generate K_i and dK/dr / r, thread = row (t & 15) x columns (t >> 4) + 16 j: a
//   wave writes 64 consecutive doubles.  (2) T = K_i D2 on the MFMA: wave w owns columns 16 w .. of each 64-column tile, A from kb, B
//   = one double of D2 per lane straight from global memory: with a 16-row block every element of D2 feeds exactly one MFMA per node,
//   so a pass through LDS would add a round trip and no reuse (D2 is M x M and L2-resident).  The epilogue forms
//   G = w_i (gl + T), adds G K to the variance sum and overwrites db with W = G dK/dr / r.  (3) Row pass, thread = (row, q = t >> 4
//   + 16 j): sum_m W d and sum_m W d^2 with d = x~_q - z~_mq accumulate over the nodes in that thread's registers (dmu, t_i-weighted
//   dS, lengthscale sums L_q): no cross-thread sum until the block ends.  (4) Column pass, thread = column: sum_n W d per q goes to
//   the block's own Zpart[b][q][m] by the same thread at every node (read-add-write, no atomics).  Registers: 4 accumulator + 16 W +
//   12 sums = 64 VGPRs of state; the compiler reports 152 - 159 VGPRs over the eight instantiations, no scratch memory, no spill.  The nodes and
//   weights are read from a 2 H-double device buffer at a uniform address (scalar loads).  Both kernels are instantiated per kind (cov_k / cov_all fold to one r-function: with the
//   kind at run time the constants of four inlined exponentials did not fit the scalar registers) and the gradient kernel does its
//   index arithmetic in 32 bits: the resource remark shows 0 spilled SGPRs and VGPRs for every instantiation.
//   Cross-block sums (Zpart, recpart) are launch_sum_splits passes in block order.
#include <cmath>
#include <vector>

#include "../../include/mi355gp_psi_gh.h"
#include "internal.h"
#include "kern_tile.h"
#include "parts.h"
#include "psi_gh.h"

#define GH_LDK 80              // doubles between rows of a statistics tile in LDS (see above)
#define GH_LDS_MAX 147456      // bytes of LDS the gradient kernel may take for its row-block operands

__global__ void k_gh_zt(const double* __restrict__ Z, const double* __restrict__ il, long m, long mp, int D, double* __restrict__ Zt) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= mp * D) return;
    const long q = i / mp, c = i - q * mp;
    Zt[i] = c < m ? il[q] * Z[c * D + q] : 0.0;
}

// ra[r][q] = il_q mu, rb[r][q] = il_q sqrt(S) of rows n0 .. n0 + 15 (0 past nend); LAYOUT_QR: [q][16] instead of [r][D]
template <bool LAYOUT_QR>
__device__ __forceinline__ void gh_stage_rows(const GhKern& A, const double* __restrict__ mu, const double* __restrict__ S, long n0,
                                              long nend, double* ra, double* rb, int t) {
    const int D = A.D;
    for (int idx = t; idx < GH_RB * D; idx += 256) {
        const int r = LAYOUT_QR ? (idx & 15) : idx / D, q = LAYOUT_QR ? (idx >> 4) : idx - r * D;
        const long n = n0 + r;
        const bool ok = n < nend;
        const double ilq = A.il[q];
        ra[idx] = ok ? ilq * mu[n * D + q] : 0.0;
        rb[idx] = ok ? ilq * sqrt(S[n * D + q]) : 0.0;
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void k_gh_stats(GhKern A, const double* __restrict__ mu, const double* __restrict__ S,
                                                  long rows, long rps, double* __restrict__ psi1, long ld1,
                                                  double* __restrict__ part) {
    extern __shared__ __align__(16) double sm[];
    double *sA = sm, *sB = sA + GH_RB * GH_LDK, *ra = sB + GH_RB * GH_LDK, *rb = ra + GH_RB * A.D;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, c = t & 63, D = A.D;
    int ti, tj = 0;
    if (part) psi_tile(blockIdx.x, &ti, &tj);
    else ti = (int)blockIdx.x;                                 // psi1 alone: one workgroup per column tile
    const bool two = part && ti != tj;                         // (psi1 alone: one tile)
    const long mA = (long)ti * GH_MT + c, mB = (long)tj * GH_MT + c, mp = A.mp;
    const long r0 = (long)blockIdx.y * rps, r1 = (r0 + rps < rows) ? (r0 + rps) : rows;
    const double* Bt = two ? sB : sA;
    d4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = (d4){0.0, 0.0, 0.0, 0.0};
    for (long nb = r0; nb < r1; nb += GH_RB) {
        __syncthreads();
        gh_stage_rows<false>(A, mu, S, nb, r1, ra, rb, t);
        __syncthreads();
        double p1[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
        for (int i = 0; i < A.H; ++i) {
            const double tn = A.tw[i], wi = A.tw[A.H + i];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = w + 4 * j;
                double s2a = 0.0, s2b = 0.0;
#pragma unroll 1
                for (int q = 0; q < D; ++q) {
                    const double x = fma(tn, rb[row * D + q], ra[row * D + q]);
                    const double da = x - A.Zt[q * mp + mA];
                    s2a = fma(da, da, s2a);
                    if (two) {
                        const double db = x - A.Zt[q * mp + mB];
                        s2b = fma(db, db, s2b);
                    }
                }
                const bool ok = nb + row < r1;
                const double ka = (ok && mA < A.m) ? cov_k(KIND, A.var, s2a) : 0.0;
                sA[row * GH_LDK + c] = ka;
                if (two) sB[row * GH_LDK + c] = (ok && mB < A.m) ? cov_k(KIND, A.var, s2b) : 0.0;
                p1[j] = fma(wi, ka, p1[j]);
            }
            __syncthreads();
            if (part) {
#pragma unroll
                for (int s = 0; s < GH_RB / 4; ++s) {
                    const int k = 4 * s + (lane >> 4);
                    const double a = wi * sA[k * GH_LDK + 16 * w + (lane & 15)];
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[j] = mfma_f64(a, Bt[k * GH_LDK + 16 * j + (lane & 15)], acc[j]);
                }
            }
            __syncthreads();
        }
        if (psi1 && tj == 0 && mA < A.m) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long n = nb + w + 4 * j;
                if (n < r1) psi1[n * ld1 + mA] = p1[j];
            }
        }
    }
    if (!part) return;
    double* out = part + (long)blockIdx.y * mp * mp;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long mi = (long)ti * GH_MT + 16 * w + (lane >> 4) + 4 * r, oj = (long)tj * GH_MT + 16 * j + (lane & 15);
            out[mi * mp + oj] = acc[j][r];                     // (mi, oj < mp: the padding holds zeros)
        }
}

template <int KIND, bool INLDS>
__global__ __launch_bounds__(256) void k_gh_grad(GhKern A, const double* __restrict__ mu, const double* __restrict__ S,
                                                 int rows, const double* __restrict__ G, PsiRank rk,
                                                 const double* __restrict__ D2, int ldd,
                                                 double* __restrict__ scratch, double* __restrict__ dmu, double* __restrict__ dS,
                                                 double* __restrict__ Zpart, double* __restrict__ recpart) {
    extern __shared__ __align__(16) double sm[];
    __shared__ double red[256];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, D = A.D, nl = t & 15, slot = t >> 4;
    // 32-bit sizes (rows <= PSI_CHUNK, m <= PSI_MMAX): 64-bit arithmetic only where an offset into global memory is formed
    const int mp = (int)A.mp, m = (int)A.m, cnt = GH_RB * mp, nb0 = (int)blockIdx.x * GH_RB;
    double* big = INLDS ? sm : scratch + (long)blockIdx.x * 3 * cnt;
    double *kb = big, *db = kb + cnt, *gl = db + cnt;
    double* small = INLDS ? sm + 3 * cnt : sm;
    double *ra = small, *rb = ra + GH_RB * D, *xs = rb + GH_RB * D;      // all [q][16]
    gh_stage_rows<true>(A, mu, S, nb0, rows, ra, rb, t);
    for (int idx = t; idx < cnt; idx += 256) {                 // dL_dpsi1 of the block, once
        const int n = nb0 + (idx & 15), mc = idx >> 4;
        double v = 0.0;
        if (n < rows && mc < m) {
            if (G) v = G[(long)n * m + mc];
            else if (rk.R) {
                for (int d = 0; d < rk.Dy; ++d) v = fma(rk.R[(long)n * rk.Dy + d], rk.v[(long)mc * rk.Dy + d], v);
                v *= rk.beta;
            }
        }
        gl[idx] = v;
    }
    double gk = 0.0, rmu[4], rsv[4], lq[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) rmu[j] = rsv[j] = lq[j] = 0.0;
    __syncthreads();
#pragma unroll 1
    for (int i = 0; i < A.H; ++i) {
        const double tn = A.tw[i], wi = A.tw[A.H + i];
        for (int idx = t; idx < GH_RB * D; idx += 256) xs[idx] = fma(tn, rb[idx], ra[idx]);
        __syncthreads();
        // (1) K_i and dK/dr / r of the block
        for (int idx = t; idx < cnt; idx += 256) {             // idx & 15 == nl
            const int mc = idx >> 4;
            double s2 = 0.0;
#pragma unroll 1
            for (int q = 0; q < D; ++q) {
                const double d = xs[q * 16 + nl] - A.Zt[(long)q * mp + mc];
                s2 = fma(d, d, s2);
            }
            const bool ok = nb0 + nl < rows && mc < m;
            const CovVal cv = cov_all(KIND, A.var, s2);
            kb[idx] = ok ? cv.k : 0.0;
            db[idx] = ok ? cv.dk_or : 0.0;
        }
        __syncthreads();
        // (2) T = K_i D2 per 64-column tile, G = w_i (dL_dpsi1 + T), W = G dK/dr / r
        for (int c0 = 0; c0 < mp; c0 += GH_MT) {
            const int col = c0 + 16 * w + (lane & 15);
            d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
            if (D2)
#pragma unroll 1
                for (int o0 = 0; o0 < mp; o0 += 4) {
                    const int k = o0 + (lane >> 4);
                    acc = mfma_f64(kb[k * 16 + (lane & 15)], D2[(long)k * ldd + col], acc);
                }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int e = col * 16 + (lane >> 4) + 4 * r;
                const double g = wi * (gl[e] + acc[r]);
                gk = fma(g, kb[e], gk);
                db[e] = g * db[e];
            }
        }
        __syncthreads();
        // (3) rows: this thread's (row, q) sums over all columns
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int q = slot + 16 * j;
            if (q < D) {
                const double x = xs[q * 16 + nl];
                double s1 = 0.0, s2 = 0.0;
#pragma unroll 1
                for (int mc = 0; mc < m; ++mc) {
                    const double d = x - A.Zt[(long)q * mp + mc], wd = db[mc * 16 + nl] * d;
                    s1 += wd;
                    s2 = fma(wd, d, s2);
                }
                rmu[j] += s1;
                rsv[j] = fma(tn, s1, rsv[j]);
                lq[j] += s2;
            }
        }
        // (4) columns: sum over the block's rows, added to the block's own Zpart by the same thread at every node
        for (int mc = t; mc < m; mc += 256) {
            double wv[GH_RB];
#pragma unroll
            for (int n = 0; n < GH_RB; ++n) wv[n] = db[mc * 16 + n];
#pragma unroll 1
            for (int q = 0; q < D; ++q) {
                const double z = A.Zt[(long)q * mp + mc];
                double s = 0.0;
#pragma unroll
                for (int n = 0; n < GH_RB; ++n) s = fma(wv[n], xs[q * 16 + n] - z, s);
                double* zp = Zpart + ((long)blockIdx.x * D + q) * mp + mc;
                *zp = i == 0 ? s : *zp + s;
            }
        }
        __syncthreads();
    }
    // the block's results: dmu, dS (final), the record {sum G K, L_q}
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int q = slot + 16 * j;
        if (q < D) {
            const int n = nb0 + nl;
            const double ilq = A.il[q];
            if (n < rows) {
                dmu[(long)n * D + q] = ilq * rmu[j];
                dS[(long)n * D + q] = ilq * rsv[j] / (2.0 * sqrt(S[(long)n * D + q]));
            }
            double l = lq[j];                                  // over the 16 rows: lanes t & 15 of one wave, fixed tree
#pragma unroll
            for (int s = 1; s < 16; s <<= 1) l += __shfl_xor(l, s);
            if (nl == 0) recpart[(long)blockIdx.x * (1 + D) + 1 + q] = l;
        }
    }
    red[t] = gk;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    if (t == 0) recpart[(long)blockIdx.x * (1 + D)] = red[0];
}

// ---- launchers ---------------------------------------------------------------------------------------------------------
// one instantiation per kind: cov_k / cov_all fold to the kind's own r-function (one exp, and its constants, per kernel)
#define GH_KIND_SWITCH(kind, CALL)                      \
    switch (kind) {                                     \
        case MI355GP_RBF: { CALL(MI355GP_RBF); } break;            \
        case MI355GP_MATERN52: { CALL(MI355GP_MATERN52); } break;  \
        case MI355GP_MATERN32: { CALL(MI355GP_MATERN32); } break;  \
        default: { CALL(MI355GP_EXPONENTIAL); } break;             \
    }
void launch_gh_zt(hipStream_t st, const double* Z, const double* il, long m, long mp, int D, double* Zt) {
    const long cnt = mp * D;
    hipLaunchKernelGGL(k_gh_zt, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, Z, il, m, mp, D, Zt);
}

static int gh_nsplit(long rows, long mp) {
    const long nt = mp / GH_MT, ntl = nt * (nt + 1) / 2;
    long s = (1024 + ntl - 1) / ntl;                           // about four workgroups per CU
    const long smax = (rows + 63) / 64;
    if (s > smax) s = smax;
    if (s > PSI_SPLIT_MAX) s = PSI_SPLIT_MAX;
    return s < 1 ? 1 : (int)s;
}

int launch_gh_stats(hipStream_t st, const GhKern& k, const double* mu, const double* S, long rows, double* psi1,
                    long ld1, double* part) {
    const long nt = k.mp / GH_MT;
    const int ns = gh_nsplit(rows, k.mp);
    const long rps = round_up((rows + ns - 1) / ns, GH_RB);
    const size_t lds = sizeof(double) * (2 * GH_RB * GH_LDK + 2 * GH_RB * (size_t)k.D);
    const dim3 grid((unsigned)(part ? nt * (nt + 1) / 2 : nt), (unsigned)ns);
#define GH_CALL(KIND) hipLaunchKernelGGL((k_gh_stats<KIND>), grid, dim3(256), lds, st, k, mu, S, rows, rps, psi1, ld1, part)
    GH_KIND_SWITCH(k.kind, GH_CALL)
#undef GH_CALL
    return ns;
}

static size_t gh_grad_lds(long mp, int D, bool inlds) {
    return sizeof(double) * ((inlds ? 3 * GH_RB * (size_t)mp : 0) + 3 * GH_RB * (size_t)D);
}
static bool gh_grad_inlds(long mp, int D) { return gh_grad_lds(mp, D, true) <= GH_LDS_MAX; }
size_t gh_grad_scratch(long rows, long mp, int D) {
    return gh_grad_inlds(mp, D) ? 0 : (size_t)((rows + GH_RB - 1) / GH_RB) * 3 * GH_RB * (size_t)mp;
}

int launch_gh_grad(hipStream_t st, const GhKern& k, const double* mu, const double* S, long rows, const double* G,
                   PsiRank rk, const double* D2, long ldd, double* scratch, double* dmu, double* dS,
                   double* Zpart, double* recpart) {
    const int nb = (int)((rows + GH_RB - 1) / GH_RB);
    const bool inlds = gh_grad_inlds(k.mp, k.D);
    const size_t lds = gh_grad_lds(k.mp, k.D, inlds);
#define GH_CALL(KIND)                                                                                                          \
    if (inlds) {                                                                                                               \
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_gh_grad<KIND, true>), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                  GH_LDS_MAX);                                                                                 \
        hipLaunchKernelGGL((k_gh_grad<KIND, true>), dim3((unsigned)nb), dim3(256), lds, st, k, mu, S, (int)rows, G, rk, D2, (int)ldd, \
                           scratch, dmu, dS, Zpart, recpart);                                                         \
    } else {                                                                                                                   \
        hipLaunchKernelGGL((k_gh_grad<KIND, false>), dim3((unsigned)nb), dim3(256), lds, st, k, mu, S, (int)rows, G, rk, D2, (int)ldd, \
                           scratch, dmu, dS, Zpart, recpart);                                                         \
    }
    GH_KIND_SWITCH(k.kind, GH_CALL)
#undef GH_CALL
    return nb;
}

// ---- the stateless entry points ----------------------------------------------------------------------------------------
int gh_quad(const char* where, const double* nodes, const double* weights, int H, GhQuad* q) {
    if (!(nodes && weights)) PART_FAIL("%s: nodes or weights are NULL", where);
    if (H < 1 || H > GH_HMAX) PART_FAIL("%s: %d quadrature nodes; between 1 and %d are taken", where, H, GH_HMAX);
    q->H = H;
    q->wsum = 0.0;
    for (int i = 0; i < H; ++i) {
        if (!std::isfinite(nodes[i]) || !std::isfinite(weights[i])) PART_FAIL("%s: node or weight %d is not finite", where, i);
        q->tw[i] = nodes[i];
        q->tw[H + i] = weights[i];
        q->wsum += weights[i];
    }
    return 0;
}

namespace {
// what both entry points validate and upload
struct GhInputs {
    PartSpec spec;
    GhKern k;
    GhQuad q;
    long N = 0;
    DevBuf dIl, dZ, dZt, dMu, dS, dTw;
    int load(const char* where, int kind, int ard, const double* theta, const double* Z, int64_t M, const double* mu,
             const double* S, int64_t N_, int D, const double* nodes, const double* weights, int H) {
        if (!(theta && Z && mu && S && M > 0 && N_ > 0 && D > 0)) PART_FAIL("%s: bad arguments", where);
        if (M > PSI_MMAX) PART_FAIL("%s: %lld inducing points; the psi-statistics kernels take at most %d", where, (long long)M, PSI_MMAX);
        if (D > PSI_QMAX) PART_FAIL("%s: %d input dimensions; the psi-statistics kernels take at most %d", where, D, PSI_QMAX);
        if (int rc = gh_quad(where, nodes, weights, H, &q)) return rc;
        const mi355gp_part part{kind, ard ? 1 : 0, 0, nullptr, theta, 0};
        if (int rc = parse_part(part, D, KS_STATIONARY, where, &spec)) return rc;
        for (int64_t i = 0; i < N_ * D; ++i)
            if (!(S[i] > 0.0) || !std::isfinite(S[i]) || !std::isfinite(mu[i]))
                PART_FAIL("%s: input variance S[%lld][%lld] = %g (mean %g): every entry must be positive and finite", where,
                          (long long)(i / D), (long long)(i % D), S[i], mu[i]);
        for (int64_t i = 0; i < M * D; ++i)
            if (!std::isfinite(Z[i])) PART_FAIL("%s: Z[%lld][%lld] is not finite", where, (long long)(i / D), (long long)(i % D));
        N = N_;
        const long mp = round_up(M, GH_MT);
        HIP_CHECK(dIl.alloc(D));
        HIP_CHECK(dZ.alloc(M * D));
        HIP_CHECK(dZt.alloc(mp * D));
        HIP_CHECK(dMu.alloc(N * D));
        HIP_CHECK(dS.alloc(N * D));
        HIP_CHECK(dTw.alloc(2 * H));
        HIP_CHECK(hipMemcpy(dTw, q.tw, sizeof(double) * 2 * H, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dIl, spec.inv_ls.data(), sizeof(double) * D, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dZ, Z, sizeof(double) * M * D, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dMu, mu, sizeof(double) * N * D, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dS, S, sizeof(double) * N * D, hipMemcpyHostToDevice));
        k = GhKern{kind, D, spec.kp.variance, dIl, dZt, (long)M, mp, dTw, H};
        launch_gh_zt(0, dZ, dIl, (long)M, mp, D, dZt);
        return 0;
    }
};
}  // namespace

extern "C" {

int mi355gp_gh_psi(int device, int kind, int ard, const double* theta, const double* Z, int64_t M, const double* mu,
                   const double* S, int64_t N, int D, const double* nodes, const double* weights, int H, double* psi0_out,
                   double* psi1_out, double* psi2_out) {
    HIP_CHECK(hipSetDevice(device));
    GhInputs in;
    if (int rc = in.load("mi355gp_gh_psi", kind, ard, theta, Z, M, mu, S, N, D, nodes, weights, H)) return rc;
    hipStream_t st = 0;
    const long chunk = N < PSI_CHUNK ? N : PSI_CHUNK, mp = in.k.mp;
    DevBuf d1, part, d2;
    if (psi1_out) HIP_CHECK(d1.alloc(chunk * M));
    if (psi2_out) {
        HIP_CHECK(part.alloc((size_t)PSI_SPLIT_MAX * mp * mp));
        HIP_CHECK(d2.alloc(M * M));
    }
    int nch = 0;
    for (long r0 = 0; r0 < N && (psi1_out || psi2_out); r0 += PSI_CHUNK, ++nch) {      // chunks in row order
        const long rc = (N - r0 < PSI_CHUNK) ? (N - r0) : PSI_CHUNK;
        const int ns = launch_gh_stats(st, in.k, in.dMu + r0 * D, in.dS + r0 * D, rc, psi1_out ? (double*)d1 : nullptr,
                                       (long)M, psi2_out ? (double*)part : nullptr);
        if (psi1_out) HIP_CHECK(hipMemcpy(psi1_out + r0 * M, d1, sizeof(double) * rc * M, hipMemcpyDeviceToHost));
        if (psi2_out) launch_psi2_combine(st, part, mp, (long)M, ns, nch > 0, d2, (long)M);
    }
    if (psi2_out) HIP_CHECK(hipMemcpy(psi2_out, d2, sizeof(double) * M * M, hipMemcpyDeviceToHost));
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipGetLastError());
    if (psi0_out)
        for (int64_t n = 0; n < N; ++n) psi0_out[n] = in.k.var * in.q.wsum;
    return 0;
}

int mi355gp_gh_psi_grad(int device, int kind, int ard, const double* theta, const double* Z, int64_t M, const double* mu,
                        const double* S, int64_t N, int D, const double* nodes, const double* weights, int H,
                        const double* dL_dpsi0, const double* dL_dpsi1, const double* rank_R, const double* rank_v, int Dy,
                        double beta, const double* dL_dpsi2, double* dtheta_out, double* dZ_out, double* dmu_out,
                        double* dS_out) {
    const char* where = "mi355gp_gh_psi_grad";
    if (rank_R || rank_v) {
        if (!(rank_R && rank_v && Dy > 0)) PART_FAIL("%s: the rank form of dL_dpsi1 needs rank_R, rank_v and Dy > 0", where);
        if (dL_dpsi1) PART_FAIL("%s: dL_dpsi1 is given both as a matrix and in rank form", where);
    }
    HIP_CHECK(hipSetDevice(device));
    GhInputs in;
    if (int rc = in.load(where, kind, ard, theta, Z, M, mu, S, N, D, nodes, weights, H)) return rc;
    hipStream_t st = 0;
    const long chunk = N < PSI_CHUNK ? N : PSI_CHUNK, mp = in.k.mp, nbmax = (chunk + GH_RB - 1) / GH_RB;
    DevBuf dG, dR, dV, dD2, scratch, dMuO, dSO, Zpart, Zs, recpart, rec;
    HIP_CHECK(scratch.alloc(gh_grad_scratch(chunk, mp, D)));
    HIP_CHECK(dMuO.alloc(chunk * D));
    HIP_CHECK(dSO.alloc(chunk * D));
    HIP_CHECK(Zpart.alloc((size_t)nbmax * D * mp));
    HIP_CHECK(hipMemset(Zpart, 0, sizeof(double) * nbmax * D * mp));       // the kernel writes columns < M only
    HIP_CHECK(Zs.alloc((size_t)D * mp));
    HIP_CHECK(recpart.alloc((size_t)nbmax * (1 + D)));
    HIP_CHECK(rec.alloc(1 + D));
    if (dL_dpsi1) HIP_CHECK(dG.alloc(chunk * M));
    if (rank_R) {
        HIP_CHECK(dR.alloc(N * Dy));
        HIP_CHECK(dV.alloc(M * Dy));
        HIP_CHECK(hipMemcpy(dR, rank_R, sizeof(double) * N * Dy, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dV, rank_v, sizeof(double) * M * Dy, hipMemcpyHostToDevice));
    }
    if (dL_dpsi2) {                                            // D2 = dL_dpsi2 + dL_dpsi2^T (gaussherm.py:84), zero padded
        std::vector<double> d2((size_t)mp * mp, 0.0);
        for (long i = 0; i < M; ++i)
            for (long j = 0; j < M; ++j) d2[(size_t)i * mp + j] = dL_dpsi2[i * M + j] + dL_dpsi2[j * M + i];
        HIP_CHECK(dD2.alloc((size_t)mp * mp));
        HIP_CHECK(hipMemcpy(dD2, d2.data(), sizeof(double) * mp * mp, hipMemcpyHostToDevice));
    }
    int nch = 0;
    for (long r0 = 0; r0 < N; r0 += PSI_CHUNK, ++nch) {
        const long rc = (N - r0 < PSI_CHUNK) ? (N - r0) : PSI_CHUNK;
        if (dL_dpsi1) HIP_CHECK(hipMemcpy(dG, dL_dpsi1 + r0 * M, sizeof(double) * rc * M, hipMemcpyHostToDevice));
        const PsiRank rk{rank_R ? (const double*)dR + r0 * Dy : nullptr, dV, Dy, beta};
        const int nb = launch_gh_grad(st, in.k, in.dMu + r0 * D, in.dS + r0 * D, rc, dL_dpsi1 ? (const double*)dG : nullptr,
                                      rk, dL_dpsi2 ? (const double*)dD2 : nullptr, mp, scratch, dMuO, dSO, Zpart,
                                      recpart);
        launch_sum_splits(st, Zpart, D * mp, nb, nch > 0, Zs);
        launch_sum_splits(st, recpart, 1 + D, nb, nch > 0, rec);
        if (dmu_out) HIP_CHECK(hipMemcpy(dmu_out + r0 * D, dMuO, sizeof(double) * rc * D, hipMemcpyDeviceToHost));
        if (dS_out) HIP_CHECK(hipMemcpy(dS_out + r0 * D, dSO, sizeof(double) * rc * D, hipMemcpyDeviceToHost));
    }
    std::vector<double> zs((size_t)D * mp), hrec((size_t)(1 + D));
    HIP_CHECK(hipMemcpy(zs.data(), Zs, sizeof(double) * zs.size(), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(hrec.data(), rec, sizeof(double) * hrec.size(), hipMemcpyDeviceToHost));
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipGetLastError());
    if (dZ_out)
        for (long j = 0; j < M; ++j)
            for (int q = 0; q < D; ++q) dZ_out[j * D + q] = -in.spec.inv_ls[(size_t)q] * zs[(size_t)q * mp + j];
    if (dtheta_out) {
        std::vector<double> recs((size_t)((D + 31) / 32) * GP_STRIDE, 0.0);
        double v0 = hrec[0];
        if (dL_dpsi0) {                                        // psi0 = variance sum_i w_i
            double s0 = 0.0;
            for (int64_t i = 0; i < N; ++i) s0 += dL_dpsi0[i];
            v0 += s0 * in.q.wsum * in.k.var;
        }
        recs[0] = v0;
        for (int q = 0; q < D; ++q) {                          // part_dtheta: dl = -rec / l
            recs[(size_t)(q / 32) * GP_STRIDE + 2 + (q % 32)] = hrec[(size_t)(1 + q)];
            recs[1] += hrec[(size_t)(1 + q)];
        }
        part_dtheta(in.spec, recs.data(), nullptr, dtheta_out);
    }
    return 0;
}

}  // extern "C"
