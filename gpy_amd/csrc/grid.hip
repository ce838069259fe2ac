// grid.hip -- optional multi-GPU mode: the exact-GP evaluation on a Pr x Pc process grid with the N x N matrices
// 2D block-cyclic distributed (tile edge nb), panels exchanged with RCCL broadcasts over xGMI and the
// O(N) results combined with all-reduces (north_star config 4).  GPy has no counterpart: its only
// parallel code is the mpi4py data-parallel sparse GP (GPy/inference/latent_function_inference/var_dtc_parallel.py).
//
// One pass, right-looking in all three factors, so every exchange is a panel broadcast and every update a rank-nb
// outer product on the local tiles (the same MFMA tile GEMM as the single-GPU path):
//   step k:  owner(k,k): L_kk = chol(A_kk), D = L_kk^-1          -> bcast D down process column k%Pc and along row k%Pr
//            column k%Pc: L_ik = A_ik D^T (i > k)                 -> bcast along process rows       (row panel RP)
//            RP tiles with i%Pc == my column                      -> bcast down process columns     (col panel CP)
//            A_ij -= L_ik L_jk^T                (i >= j > k)        [potrf trailing update]
//            row k%Pr: X_kj = D B_kj (j < k), X_kk = D            -> bcast down process columns     (XR)
//            XR tiles with j%Pr == my row                         -> bcast along process rows       (XRr)
//            B_ij -= L_ik X_kj                  (i > k >= j)        [right-looking triangular inverse, B -> X = L^-1]
//            W_ij += X_ki^T X_kj                (k >= i >= j)       [Ky^-1 = X^T X accumulated as X rows complete]
// Afterwards alpha = X^T (X R), diag W and the gradient reduction run on the local tiles and are summed across ranks.
//
// Two transports behind one driver: RCCL (one rank per process, one GPU each; librccl.so is dlopen'ed so the
// single-GPU library has no RCCL dependency) and LOOPBACK (all Pr*Pc logical ranks inside one process on one
// device, broadcasts are device copies) used to test the algorithm on a 1-GPU box.  Both live in grid_comm.hip; this file
// holds the tile kernels, the context's lifecycle and the evaluation, built from named phases (grid_run at the end of them).
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/mi355gp_debug.h"
#include "gemm_tile.h"
#include "grid_ctx.h"
#include "parts.h"

#define LOG_2_PI 1.8378770664093454836

// ---------------------------------------------------------------------------------------------------
// device kernels specific to the distributed layout

// C (op)= A * B on the 128x128 tiles of a local region; operands may be "tile-major" panels ([tile][nb][nb], ld = nb).
//   mode 0: C = acc, 1: C += acc, 2: C -= acc.   pred: keep only tiles whose global nb-tile indices satisfy I >= J.
struct GridPred {
    int on, Pr, pr, Pc, pc, roff, coff;   // I = (roff + ti/q)*Pr + pr ;  J = (coff + tj/q)*Pc + pc
};
template <bool AK, bool BK>
__global__ __launch_bounds__(256, 2) void k_grid_gemm(double* __restrict__ C, long ldc, int c_tm,
                                                      const double* __restrict__ A, long lda, int a_tm,
                                                      const double* __restrict__ B, long ldb, int b_tm, int K,
                                                      int ntc, int q, long nb, int mode, GridPred pd) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int ti = blockIdx.x / ntc, tj = blockIdx.x % ntc;
    if (pd.on) {
        const int I = (pd.roff + ti / q) * pd.Pr + pd.pr, J = (pd.coff + tj / q) * pd.Pc + pd.pc;
        if (J > I) return;
    }
    const double* Ap;
    const double* Bp;
    if (AK) Ap = A + (long)ti * NB * lda;
    else Ap = a_tm ? A + (long)(ti / q) * nb * nb + (long)(ti % q) * NB : A + (long)ti * NB;
    if (BK) Bp = B + (long)tj * NB * ldb;
    else Bp = b_tm ? B + (long)(tj / q) * nb * nb + (long)(tj % q) * NB : B + (long)tj * NB;
    double* Cp = c_tm ? C + (long)(tj / q) * nb * nb + (long)ti * NB * nb + (long)(tj % q) * NB
                      : C + (long)ti * NB * ldc + (long)tj * NB;
    d4 acc[4][4];
    gt_zero<4>(acc);
    gemm_tile_128<AK, BK, 4>(Ap, lda, Bp, ldb, K, acc, smem);
    if (mode == 0) gt_store<0, 4>(Cp, ldc, acc);
    else if (mode == 1) gt_store<3, 4>(Cp, ldc, acc, 1.0, 1.0);
    else gt_store<2, 4>(Cp, ldc, acc);
}

struct GOp {
    const double* p;
    long ld;
    int tm;
};
template <bool AK, bool BK>
static void grid_gemm_t(hipStream_t st, double* C, long ldc, int c_tm, GOp a, GOp b, long M, long N, long K, long nb,
                        int mode, GridPred pd) {
    if (M <= 0 || N <= 0) return;
    static bool opted = false;
    if (!opted) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_grid_gemm<AK, BK>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, GT_LDS_BYTES);
        opted = true;
    }
    const int ntr = (int)(M / NB), ntc = (int)(N / NB);
    hipLaunchKernelGGL((k_grid_gemm<AK, BK>), dim3((unsigned)(ntr * ntc)), dim3(256), GT_LDS_BYTES, st, C, ldc, c_tm,
                       a.p, a.ld, a.tm, b.p, b.ld, b.tm, (int)K, ntc, (int)(nb / NB), nb, mode, pd);
}

// The aggregated updates: C (op)= sum over the panels k in [ks, k1) of A_k * B_k on the 128x128 tiles of a local region,
// ONE pass over C for the whole panel list (the tile pipeline rolls across panels: gemm_tile_128_v3_multi).
//   MODE 0: C = acc,  1: C += acc,  2: C -= acc   (1 / 2 read C before the k-loop: its latency hides behind the prologue)
//   Atab[k] / Btab[k]: base of panel k such that LOCAL nb-tile l of the operand starts at base + l * nb * nb
//       AK / BK = true : the panel is a tall [rows][nb] matrix (k contiguous): L_ik row panels / L_jk column panels
//       AK / BK = false: the panel is a sequence of [nb(k)][nb] tiles (m/n contiguous): X_ki / X_kj row panels
//   ti0 / tj0: first local 128-tile row / column of the region.   pd: keep tiles with I >= J (global nb-tile indices).
//   kpred: the first panel that touches tile (I, J):  0: k0;  1: max(k0, J) (B -= L X: X_kj = 0 for j > k);
//          2: max(k0, I, J) (W += X^T X).  A tile with no panel left keeps its C (MODE 0: stores zeros).
// Live-tile enumeration of a region under the lower predicate: pre[i] = number of live nb-tile pairs in the region's
// rows before row i (host-computed per launch, passed BY VALUE in the kernel arguments: <= 4 KB).  Consecutive
// workgroups then are consecutive LIVE tiles: a plain rows x columns grid whose dead half exits at once runs the same
// tiles 30 % slower (N=16384 X^T X: 48 vs 69 TF/s, mi355gp_dbg_grid_multi) -- workgroups go to the 8 XCDs round-robin
// by index, dead ones included, and the XCDs drift out of balance.
#define GRID_ROWTAB_MAX 960
struct GridRowTab {
    int n;                                    // rows in the table; 0 = plain rows x columns enumeration
    int pre[GRID_ROWTAB_MAX + 1];
};
template <bool AK, bool BK, int MODE>
__global__ __launch_bounds__(256, 2) void k_grid_gemm_multi(double* __restrict__ C, long ldc,
                                                            const double* const* __restrict__ Atab,
                                                            const double* const* __restrict__ Btab, int k0, int k1,
                                                            int ti0, int tj0, int ntc, int q, long nb, int kpred,
                                                            GridPred pd, long ldo, int tm, GridRowTab rt) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    int ti, tj;
    if (tm == 2) {                                           // experiment: triangular enumeration of a square region at (0, 0)
        const int bid = blockIdx.x;
        ti = (int)((sqrtf(8.0f * (float)bid + 1.0f) - 1.0f) * 0.5f);
        while ((long)ti * (ti + 1) / 2 > bid) --ti;
        while ((long)(ti + 1) * (ti + 2) / 2 <= bid) ++ti;
        tj = bid - (int)((long)ti * (ti + 1) / 2);
    } else if (rt.n > 0) {                                   // live nb-tile pairs in row order, q x q tiles per pair
        const int qq = q * q, p = (int)(blockIdx.x / qq), sub = (int)(blockIdx.x % qq);
        int lo = 0, hi = rt.n - 1;                           // last row with pre[row] <= p
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (rt.pre[mid] <= p) lo = mid;
            else hi = mid - 1;
        }
        ti = ti0 + lo * q + sub / q;
        tj = tj0 + (p - rt.pre[lo]) * q + sub % q;
    } else {
        ti = ti0 + blockIdx.x / ntc;
        tj = tj0 + blockIdx.x % ntc;
    }
    const int I = (ti / q) * pd.Pr + pd.pr, J = (tj / q) * pd.Pc + pd.pc;
    if (pd.on && J > I) return;
    int ks = k0;
    if (kpred >= 1 && J > ks) ks = J;
    if (kpred >= 2 && I > ks) ks = I;
    double* Ct = C + (long)ti * NB * ldc + (long)tj * NB;
    d4 acc[4][4];
    if (ks >= k1) {
        if (MODE == 0) {
            gt_zero<4>(acc);
            gt_store<0, 4>(Ct, ldc, acc);
        }
        return;
    }
    if (MODE == 0) gt_zero<4>(acc);
    else gt_load_buf<4>(Ct, ldc, acc);
    // ldo / tm: operand row stride and tile-major flag (the panel stores: ldo = nb, tm = 1; the microbenchmark also reads a
    // plain row-major matrix: ldo = its leading dimension, tm = 0)
    const long aoff = AK ? (long)ti * NB * ldo : (tm == 1 ? (long)(ti / q) * nb * nb + (long)(ti % q) * NB : (long)ti * NB);
    const long boff = BK ? (long)tj * NB * ldo : (tm == 1 ? (long)(tj / q) * nb * nb + (long)(tj % q) * NB : (long)tj * NB);
    gemm_tile_128_v3_multi<AK, BK, MODE == 2>(Atab, aoff, ldo, Btab, boff, ldo, ks, k1, (int)(nb / 16), acc, smem);
    gt_store<0, 4>(Ct, ldc, acc);
}

// region [ti0, ti1) x [tj0, tj1) in local nb-tiles
template <bool AK, bool BK, int MODE>
static void grid_gemm_multi(hipStream_t st, double* C, long ldc, const double* const* Atab, const double* const* Btab,
                            int k0, int k1, int ti0, int ti1, int tj0, int tj1, long nb, int kpred, GridPred pd,
                            long ldo = 0, int tm = 1) {
    if (ti1 <= ti0 || tj1 <= tj0 || k1 <= k0) return;
    static bool opted = false;
    if (!opted) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_grid_gemm_multi<AK, BK, MODE>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, GT_LDS_BYTES);
        opted = true;
    }
    const int q = (int)(nb / NB), ntr = (ti1 - ti0) * q, ntc = (tj1 - tj0) * q;
    long nblk = (tm == 2) ? (long)ntr * (ntr + 1) / 2 : (long)ntr * ntc;
    GridRowTab rt;
    rt.n = 0;
    if (pd.on && tm != 2 && ti1 - ti0 <= GRID_ROWTAB_MAX) {
        // live columns of local row li: lj with lj * Pc + pc <= li * Pr + pr, clipped to [tj0, tj1) (a prefix of the range)
        long tot = 0;
        int first = -1, last = -1;
        for (int li = ti0; li < ti1; ++li) {
            const long I = (long)li * pd.Pr + pd.pr;
            long m = (I >= pd.pc) ? (I - pd.pc) / pd.Pc + 1 : 0;             // local columns with J <= I
            long c = m - tj0;
            if (c < 0) c = 0;
            if (c > tj1 - tj0) c = tj1 - tj0;
            if (c > 0) {
                if (first < 0) first = li;
                last = li;
            }
            if (first >= 0) rt.pre[li - first] = (int)tot;
            tot += c;
        }
        if (tot == 0) return;
        rt.n = last - first + 1;
        rt.pre[rt.n] = (int)tot;
        ti0 = first;
        nblk = tot * q * q;
    }
    hipLaunchKernelGGL((k_grid_gemm_multi<AK, BK, MODE>), dim3((unsigned)nblk), dim3(256), GT_LDS_BYTES, st, C, ldc,
                       Atab, Btab, k0, k1, ti0 * q, tj0 * q, ntc, q, nb, kpred, pd, ldo ? ldo : nb, tm, rt);
}

// local diagonal fix-up after the cross-covariance build: entries with equal global index get noise + jitter
// (real points) or 1 (padding); one thread per element of every diagonal nb-tile this rank owns.
__global__ void k_grid_fix_diag(double* __restrict__ A, long ld, long nb, long n, int ndiag,
                                const int* __restrict__ dl_r, const int* __restrict__ dl_c,
                                const int* __restrict__ dg, const double* __restrict__ noise, long noise_len,
                                double jit) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)ndiag * nb) return;
    const int d = (int)(idx / nb);
    const long e = idx % nb, g = (long)dg[d] * nb + e;
    double* p = A + ((long)dl_r[d] * nb + e) * ld + (long)dl_c[d] * nb + e;
    if (g < n) *p += noise[noise_len > 1 ? g : 0] + jit;
    else *p = 1.0;
}

// G = w * 0.5 * (alpha_i . alpha_j - Dy * W_ij), w = 2 (global i > j), 1 (i == j), 0 (i < j): the lower-triangle
// weighting of the symmetric dL_dK (exact_gaussian_inference.py:70) on a block-cyclic local tile set.
__global__ void k_grid_dldk(const double* __restrict__ W, double* __restrict__ G, long ld, long rows, long cols,
                            const long* __restrict__ gr, const long* __restrict__ gc,
                            const double* __restrict__ alpha, int Dy, long n) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long i = blockIdx.y;
    if (j >= cols || i >= rows) return;
    const long gi = gr[i], gj = gc[j];
    double g = 0.0;
    if (gi < n && gj < n && gj <= gi) {
        double aa = 0.0;
        for (int d = 0; d < Dy; ++d) aa = fma(alpha[gi * Dy + d], alpha[gj * Dy + d], aa);
        g = 0.5 * (aa - (double)Dy * W[i * ld + j]);
        if (gj < gi) g *= 2.0;
    }
    G[i * ld + j] = g;
}

// y[i][d] = sum_j M[i][j] * v[g(j)][d]   (one wave per local row; v indexed by global column index, 0 beyond n)
__global__ __launch_bounds__(256) void k_grid_row_reduce(const double* __restrict__ M, long ld, long rows, long cols,
                                                         const long* __restrict__ gc, const double* __restrict__ v,
                                                         int Dy, int d, long n, double* __restrict__ y) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= rows) return;
    double s = 0.0;
    for (long j = lane; j < cols; j += 64) {
        const long g = gc[j];
        if (g < n) s = fma(M[i * ld + j], v[g * Dy + d], s);
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
    if (lane == 0) y[i] = s;
}

// out[j] = sum_i M[i][j] * (v ? v[g(i)][d] : M[i][j]) in two fixed-order stages: partials per chunk of CR_ROWS rows (64
// columns x CR_ROWS rows per block), then the sum over chunks.  M = X = L^-1 is lower block triangular in GLOBAL nb-tiles:
// a chunk whose tile row lies above the column's tile contributes exact zeros and is not read.
#define CR_ROWS 128
__global__ __launch_bounds__(256) void k_grid_col_reduce_part(const double* __restrict__ M, long ld, long rows, long cols,
                                                              const long* __restrict__ gr, const double* __restrict__ v,
                                                              int Dy, int d, long n, double* __restrict__ part, long nb,
                                                              int Pr, int pr, int Pc, int pc) {
    __shared__ double red[4][64];
    const int tx = threadIdx.x & 63, g = threadIdx.x >> 6;
    const long j = (long)blockIdx.x * 64 + tx, i0 = (long)blockIdx.y * CR_ROWS;
    const long I = (i0 / nb) * Pr + pr, J = (((long)blockIdx.x * 64) / nb) * Pc + pc;
    double s = 0.0;
    if (j < cols && I >= J) {
        const long i1 = (i0 + CR_ROWS < rows) ? i0 + CR_ROWS : rows;
        for (long i = i0 + g; i < i1; i += 4) {
            const double x = M[i * ld + j];
            if (v) {
                const long gi = gr[i];
                if (gi < n) s = fma(x, v[gi * Dy + d], s);
            } else {
                s = fma(x, x, s);
            }
        }
    }
    red[g][tx] = s;
    __syncthreads();
    if (g == 0 && j < cols) part[(long)blockIdx.y * cols + j] = (red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx]);
}
__global__ void k_grid_col_combine(const double* __restrict__ part, long nchunks, long cols, double* __restrict__ out) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cols) return;
    double s = 0.0;
    for (long c = 0; c < nchunks; ++c) s += part[c * cols + j];
    out[j] = s;
}

// gvec[g(l)*stride + d] = loc[l]  for g(l) < n
__global__ void k_grid_scatter(const double* __restrict__ loc, long cnt, const long* __restrict__ gidx, long n,
                               int stride, int d, double* __restrict__ gvec) {
    const long l = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= cnt) return;
    const long g = gidx[l];
    if (g < n) gvec[g * stride + d] = loc[l];
}

// nt tiles of nb x nb, contiguous at src, into the row block dst (row stride ldd): tile t at columns t * nb ..  (one launch
// instead of one 2-D copy per tile: 7,000 of them per evaluation at N = 32768 on a 2 x 4 grid)
__global__ __launch_bounds__(256) void k_tiles_to_rowblock(double* __restrict__ dst, long ldd, const double* __restrict__ src, int nb) {
    const double* s = src + (long)blockIdx.y * nb * nb;
    double* d = dst + (long)blockIdx.y * nb;
    const int half = nb >> 1;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < (long)nb * half; e += (long)gridDim.x * blockDim.x) {
        const long i = e / half, j = 2 * (e - i * half);
        *reinterpret_cast<d2*>(d + i * ldd + j) = *reinterpret_cast<const d2*>(s + i * nb + j);
    }
}

// after a tile factorisation: scal[0] += sum(logsum[0..q)) ; info_g = first failure in global numbering
__global__ void k_grid_tile_stats(const double* __restrict__ logsum, int q, const int* __restrict__ info_tile,
                                  long col0, double* __restrict__ scal, int* __restrict__ info_g) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (int i = 0; i < q; ++i) s += logsum[i];
    scal[0] += s;
    if (info_tile[0] >= PS_ABORT_INFO) {
        scal[2] += 1.0;                                  // a persistent tile factorisation did not run: every rank redoes the evaluation
    } else if (info_tile[0] != 0) {
        scal[1] += 1.0;                                  // summed over ranks: "some tile failed" is known everywhere
        if (info_g[0] == 0) info_g[0] = (int)(col0 + info_tile[0]);
    }
}

// The diagonal of D = L_kk^-1 is the reciprocal of the diagonal of L_kk AS STORED, correctly rounded (what dtrtri returns).  The
// tile factorisation forms L_ii = a y and 1 / L_ii = y from one refined rsq(a), each rounded on its own: D_ii L_ii - 1 is up to a
// few u, and at N = 1 that is all of X L - I (2.3 n u |X||L| against the 0.02 of a division).
__global__ void k_grid_inv_diag(double* __restrict__ Dv, const double* __restrict__ Lt, long nb) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nb) Dv[i * nb + i] = 1.0 / Lt[i * nb + i];
}

// ---------------------------------------------------------------------------------------------------
// process defaults of the schedule options: environment, else built-in
static void grid_default_option(mi355gp_grid* g, int o) {
    if (o == MI355GP_GRID_OPT_LOOKAHEAD) {
        const char* e = PRODUCT_ENV("GRID_LOOKAHEAD");
        g->lookahead = (e && *e) ? (atoi(e) ? 1 : 0) : 1;
    } else if (o == MI355GP_GRID_OPT_G) {
        const char* e = DIAG_ENV("GRID_G");
        g->G = (e && *e && atoi(e) >= 1) ? atoi(e) : 1;
    } else if (o == MI355GP_GRID_OPT_GW) {
        const char* e = DIAG_ENV("GRID_GW");
        g->GW = (e && *e && atoi(e) >= 0) ? atoi(e) : 4;
    } else if (o == MI355GP_GRID_OPT_CHECK_SEQ) {
        const char* e = PRODUCT_ENV("GRID_CHECK_SEQ");
        g->check_seq = (e && *e && atoi(e)) ? 1 : 0;
    }
}

static int cnt_le(long k, int p, int P) { return (k >= p) ? (int)((k - p) / P + 1) : 0; }   // tiles t <= k with t % P == p
static int cnt_lt(long k, int p, int P) { return (k > 0) ? cnt_le(k - 1, p, P) : 0; }

// the identity of a rank: what a fresh GridRank keeps of the one it replaces
static GridRank make_rank(int rank, int Pc, hipStream_t st, hipStream_t sc, hipStream_t sw) {
    GridRank r;
    r.rank = rank;
    r.pr = rank / Pc;
    r.pc = rank % Pc;
    r.st = st;
    r.sc = sc;
    r.sw = sw;
    return r;
}
// releases everything the rank holds on the device
static void free_rank(GridRank& r, int Pc) {
    factor_ws_free(&r.ws);
    r = make_rank(r.rank, Pc, r.st, r.sc, r.sw);
}

// the tiles t in (lo, hi] ... [lo, hi) with t % Pa == a and t % Pb == b, as first / step / count (step = lcm(Pa, Pb))
static void tile_progression(long lo, long hi, int a, int Pa, int b, int Pb, long* first, long* step, int* count) {
    long L = Pa;
    while (L % Pb != 0) L += Pa;
    *step = L;
    *first = -1;
    *count = 0;
    for (long t = lo; t < hi && t < lo + L; ++t)
        if (t % Pa == a && t % Pb == b) { *first = t; break; }
    if (*first >= 0) *count = (int)((hi - 1 - *first) / L + 1);
}
// (Re)allocates the four panel stores of a rank and their pointer tables for the current group size G (see GridRank).
static int alloc_panel_stores(mi355gp_grid* g, GridRank& r) {
    const long nb = g->nb, T = g->T;
    const size_t tile = (size_t)nb * nb;
    DevBuf* store[4] = {&r.RPs, &r.CPs, &r.XRs, &r.XRrs};
    DevArr<const double*>* table[4] = {&r.dRP, &r.dCP, &r.dXR, &r.dXRr};
    for (DevBuf* s : store) *s = DevBuf();                   // the stores sized for another G go first
    for (DevArr<const double*>* t : table) *t = DevArr<const double*>();
    const long G = g->G < 1 ? 1 : g->G;
    long slots = 2 * G;
    if (slots > T) slots = T;
    r.ring_slots = slots;
    std::vector<long> oXR((size_t)T + 1, 0), oXRr((size_t)T + 1, 0);
    for (long k = 0; k < T; ++k) {
        oXR[k + 1] = oXR[k] + cnt_le(k, r.pc, g->Pc);
        oXRr[k + 1] = oXRr[k] + cnt_le(k, r.pr, g->Pr);
    }
    const size_t bytes[4] = {sizeof(double) * tile * (size_t)(slots * r.TLr + 1), sizeof(double) * tile * (size_t)(slots * r.TLc + 1),
                             sizeof(double) * tile * (size_t)(oXR[T] + 1), sizeof(double) * tile * (size_t)(oXRr[T] + 1)};
    for (int i = 0; i < 4; ++i)
        if (store[i]->alloc(bytes[i] / sizeof(double)) != hipSuccess) {
            (void)hipGetLastError();
            mi355gp_set_error("grid mode: out of device memory for the panel stores of rank %d (N=%ld on %dx%d, nb=%ld: L-panel ring "
                              "%.2f + %.2f GB for G=%ld, X panels %.2f + %.2f GB, next to 3 x %.2f GB of local matrices); use more "
                              "GPUs or a smaller G",
                              r.rank, g->n, g->Pr, g->Pc, nb, bytes[0] / 1e9, bytes[1] / 1e9, G, bytes[2] / 1e9, bytes[3] / 1e9,
                              sizeof(double) * (double)r.LR * (double)r.LC / 1e9);
            return -4;
        }
    r.hRP.resize((size_t)T); r.hCP.resize((size_t)T); r.hXR.resize((size_t)T); r.hXRr.resize((size_t)T);
    for (long k = 0; k < T; ++k) {
        r.hRP[k] = r.RPs + (k % slots) * (long)r.TLr * (long)tile;       // full-height slot: local tile l at base + l * tile
        r.hCP[k] = r.CPs + (k % slots) * (long)r.TLc * (long)tile;
        r.hXR[k] = r.XRs + oXR[k] * (long)tile;
        r.hXRr[k] = r.XRrs + oXRr[k] * (long)tile;
    }
    const std::vector<double*>* host[4] = {&r.hRP, &r.hCP, &r.hXR, &r.hXRr};
    for (DevArr<const double*>* t : table) HIP_CHECK(t->alloc((size_t)T));
    for (int i = 0; i < 4; ++i)
        HIP_CHECK(hipMemcpy((void*)table[i]->p, host[i]->data(), sizeof(double*) * (size_t)T, hipMemcpyHostToDevice));
    return 0;
}

// Streams, events, ranks and communicators of a new context.  On a failing return the context is partly built:
// mi355gp_grid_create hands it to mi355gp_grid_destroy, which releases whatever is there.
static int grid_init(mi355gp_grid* g, const void* id128) {
    const int world = g->world, Pc = g->Pc;
    {
        const char* envf = DIAG_ENV("GRID_FORCE_GENERIC");
        if (g->loopback && world == 1 && !(envf && atoi(envf))) return mi355gp_create(g->device, &g->single);
    }
    HIP_CHECK(hipStreamCreateWithFlags(&g->st, hipStreamNonBlocking));
    {
        int least = 0, greatest = 0;
        HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIP_CHECK(hipStreamCreateWithPriority(&g->sc, hipStreamNonBlocking, greatest));
        HIP_CHECK(hipStreamCreateWithPriority(&g->sw, hipStreamNonBlocking, least));
        HIP_CHECK(hipEventCreateWithFlags(&g->ev_w, hipEventDisableTiming));
        for (int o = 0; o < MI355GP_GRID_OPT_NUM; ++o) grid_default_option(g, o);
        g->dbg_crit = diag_env_int(DIAG_ENV("GRID_DBG_CRIT"), 0);
    }
    for (auto& e : g->ev) HIP_CHECK(hipEventCreate(&e));
    if (g->loopback) {
        for (int r = 0; r < world; ++r) g->ranks.push_back(make_rank(r, Pc, g->st, g->sc, g->sw));
        return 0;
    }
    if (int rc = grid_comm_load()) return rc;
    g->ranks.push_back(make_rank(g->my_rank, Pc, g->st, g->sc, g->sw));
    return grid_comm_connect(g, g->ranks[0], id128);
}

extern "C" {

int mi355gp_grid_create(int device, int rank, int world, int Pr, int Pc, int nb, const void* id128,
                        mi355gp_grid** out) {
    ARG_CHECK(out && Pr >= 1 && Pc >= 1 && nb >= NB && nb % NB == 0, "mi355gp_grid_create: Pr, Pc >= 1, nb % 128 == 0");
    ARG_CHECK(world == Pr * Pc, "mi355gp_grid_create: world must equal Pr*Pc");
    ARG_CHECK(rank >= 0 && rank < world, "mi355gp_grid_create: bad rank");
    int ndev = 0;
    mi355gp_device_count(&ndev);
    if (device < 0 || device >= ndev) {
        mi355gp_set_error("mi355gp_grid_create: device %d not available (%d HIP devices visible)", device, ndev);
        return -2;
    }
    HIP_CHECK(hipSetDevice(device));
    mi355gp_grid* g = new mi355gp_grid();
    g->device = device;
    g->world = world;
    g->Pr = Pr;
    g->Pc = Pc;
    g->nb = nb;
    g->my_rank = rank;
    g->loopback = (id128 == nullptr);
    if (int rc = grid_init(g, id128)) {
        mi355gp_grid_destroy(g);
        return rc;
    }
    *out = g;
    return 0;
}

int mi355gp_grid_destroy(mi355gp_grid* g) {
    if (!g) return 0;
    if (g->single) {
        mi355gp_destroy(g->single);
        delete g;
        return 0;
    }
    // (also the exit of a mi355gp_grid_create that failed half way: every handle below may still be null, the lists empty)
    (void)hipSetDevice(g->device);
    if (g->st) (void)hipStreamSynchronize(g->st);
    for (GridRank& r : g->ranks) free_rank(r, g->Pc);
    grid_comm_disconnect(g);
    for (auto& e : g->ev)
        if (e) (void)hipEventDestroy(e);
    for (auto& e : g->ev_cr) (void)hipEventDestroy(e);
    for (auto& e : g->ev_p1) (void)hipEventDestroy(e);
    if (g->sc) {
        (void)hipStreamSynchronize(g->sc);
        (void)hipStreamDestroy(g->sc);
    }
    if (g->sw) {
        (void)hipStreamSynchronize(g->sw);
        (void)hipStreamDestroy(g->sw);
    }
    if (g->ev_w) (void)hipEventDestroy(g->ev_w);
    if (g->st) (void)hipStreamDestroy(g->st);
    delete g;
    return 0;
}

// Every rank passes the full (replicated) X and R: N*D*8 bytes is small next to the N^2/P matrix share.
int mi355gp_grid_set_data(mi355gp_grid* g, const double* X, int64_t N, int D, const double* R, int Dy) {
    ARG_CHECK(g && X && R && N > 0 && D > 0 && Dy > 0, "mi355gp_grid_set_data: bad arguments");
    if (g->single) {
        g->n = N;
        return mi355gp_set_data(g->single, X, N, D, R, Dy);
    }
    HIP_CHECK(hipSetDevice(g->device));
    HIP_CHECK(hipStreamSynchronize(g->st));
    HIP_CHECK(hipStreamSynchronize(g->sc));
    HIP_CHECK(hipStreamSynchronize(g->sw));
    const long nb = g->nb;
    g->n = N;
    g->T = (N + nb - 1) / nb;
    while ((long)g->ev_cr.size() < g->T + 1) {
        hipEvent_t e1, e2;
        HIP_CHECK(hipEventCreateWithFlags(&e1, hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&e2, hipEventDisableTiming));
        g->ev_cr.push_back(e1);
        g->ev_p1.push_back(e2);
    }
    g->npad = g->T * nb;
    g->D = D;
    g->Dy = Dy;
    g->have_result = false;
    const long T = g->T, TLrM = (T + g->Pr - 1) / g->Pr, TLcM = (T + g->Pc - 1) / g->Pc;
    const int groups = (D + 31) / 32;
    for (GridRank& r : g->ranks) {
        free_rank(r, g->Pc);                     // a fresh rank that keeps its identity
        const int pr = r.pr, pc = r.pc;
        r.TLr = cnt_le(T - 1, pr, g->Pr);
        r.TLc = cnt_le(T - 1, pc, g->Pc);
        r.LR = TLrM * nb;
        r.LC = TLcM * nb;
        const size_t mat = (size_t)r.LR * r.LC;
        HIP_CHECK(r.A.alloc(mat));
        HIP_CHECK(r.X.alloc(mat));
        HIP_CHECK(r.W.alloc(mat));
        if (int rc = alloc_panel_stores(g, r)) return rc;
        HIP_CHECK(r.cpart.alloc((size_t)(r.LR / CR_ROWS + 1) * r.LC));
        HIP_CHECK(r.Dt.alloc((size_t)nb * nb));
        HIP_CHECK(r.Dv.alloc((size_t)nb * nb));
        HIP_CHECK(r.Ds.alloc((size_t)nb * nb));
        if (!g->loopback) HIP_CHECK(r.bstage.alloc((size_t)nb * nb * (size_t)(TLrM > TLcM ? TLrM : TLcM)));
        // local point sets (host-side gather, uploaded once)
        std::vector<long> gR((size_t)r.LR), gC((size_t)r.LC);
        std::vector<double> XsR((size_t)r.LR * D, 0.0), XsC((size_t)r.LC * D, 0.0);
        r.nvr = r.nvc = 0;
        for (long l = 0; l < r.LR; ++l) {
            const long lt = l / nb;
            const long gi = (lt < r.TLr) ? (lt * g->Pr + pr) * nb + l % nb : g->npad + l;   // unused rows: beyond n
            gR[l] = gi;
            if (gi < N) { memcpy(&XsR[(size_t)l * D], X + gi * D, sizeof(double) * D); r.nvr = l + 1; }
        }
        for (long l = 0; l < r.LC; ++l) {
            const long lt = l / nb;
            const long gj = (lt < r.TLc) ? (lt * g->Pc + pc) * nb + l % nb : g->npad + l;
            gC[l] = gj;
            if (gj < N) { memcpy(&XsC[(size_t)l * D], X + gj * D, sizeof(double) * D); r.nvc = l + 1; }
        }
        HIP_CHECK(r.gR.alloc((size_t)r.LR));
        HIP_CHECK(r.gC.alloc((size_t)r.LC));
        HIP_CHECK(r.XsR.alloc((size_t)r.LR * D));
        HIP_CHECK(r.XsC.alloc((size_t)r.LC * D));
        HIP_CHECK(r.XtR.alloc((size_t)r.LR * D));
        HIP_CHECK(r.XtC.alloc((size_t)r.LC * D));
        HIP_CHECK(hipMemcpy(r.gR, gR.data(), sizeof(long) * r.LR, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(r.gC, gC.data(), sizeof(long) * r.LC, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(r.XsR, XsR.data(), sizeof(double) * r.LR * D, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(r.XsC, XsC.data(), sizeof(double) * r.LC * D, hipMemcpyHostToDevice));
        // diagonal tiles owned by this rank
        std::vector<int> dlr, dlc, dg;
        for (long t = 0; t < T; ++t)
            if (t % g->Pr == pr && t % g->Pc == pc) {
                dlr.push_back((int)(t / g->Pr));
                dlc.push_back((int)(t / g->Pc));
                dg.push_back((int)t);
            }
        r.ndiag = (int)dg.size();
        HIP_CHECK(r.dl_r.alloc((size_t)r.ndiag + 1));
        HIP_CHECK(r.dl_c.alloc((size_t)r.ndiag + 1));
        HIP_CHECK(r.dg.alloc((size_t)r.ndiag + 1));
        if (r.ndiag) {
            HIP_CHECK(hipMemcpy(r.dl_r, dlr.data(), sizeof(int) * r.ndiag, hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(r.dl_c, dlc.data(), sizeof(int) * r.ndiag, hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(r.dg, dg.data(), sizeof(int) * r.ndiag, hipMemcpyHostToDevice));
        }
        const long vmax = (r.LR > r.LC ? r.LR : r.LC);
        HIP_CHECK(r.vloc.alloc((size_t)vmax));
        HIP_CHECK(r.gvec2.alloc((size_t)N));
        HIP_CHECK(r.alpha.alloc((size_t)N * Dy));
        HIP_CHECK(r.ybuf.alloc((size_t)N * Dy));
        HIP_CHECK(r.Rg.alloc((size_t)N * Dy));
        HIP_CHECK(hipMemcpy(r.Rg, R, sizeof(double) * N * Dy, hipMemcpyHostToDevice));
        HIP_CHECK(r.scal.alloc(8));
        HIP_CHECK(r.gradPart.alloc((size_t)groups * 2048 * GP_STRIDE));
        HIP_CHECK(r.gradOut.alloc((size_t)groups * GP_STRIDE));
        HIP_CHECK(r.invls.alloc((size_t)D));
        HIP_CHECK(r.noise.alloc((size_t)N));
        HIP_CHECK(r.info_g.alloc(4));
        if (factor_ws_alloc(&r.ws, nb) != 0) return -3;
        r.ws.lookahead = 0;      // the nb x nb diagonal tile is factored in order on the rank's stream
    }
    return 0;
}

}  // extern "C"

// ---- one evaluation on all local ranks, phase by phase (grid_run at the end puts them in order) ----------------------------
// the stream of a rank's critical path: sc under look-ahead, else everything runs in order on st
static hipStream_t crit_stream(const mi355gp_grid* g, const GridRank& r) { return g->lookahead ? r.sc : r.st; }

// prepare: the L-panel ring is sized for the group size in effect when the data was set -- follow a later change of G; empty
// the collective logs
static int grid_prepare(mi355gp_grid* g) {
    long want = 2 * (g->G < 1 ? 1 : g->G);
    if (want > g->T) want = g->T;
    for (GridRank& r : g->ranks)
        if (r.ring_slots != want) {
            HIP_CHECK(hipDeviceSynchronize());
            if (int rc = alloc_panel_stores(g, r)) return rc;
        }
    grid_coll_reset(g);
    return 0;
}

// build K: the covariance tiles K(X_rows, X_cols) of every rank + the diagonal fix-up
static int grid_build_K(mi355gp_grid* g, const PartSpec& pt, const double* noise, int64_t noise_len, double jit) {
    const KernParams& kp = pt.kp;
    const long nb = g->nb;
    const int D = g->D;
    for (GridRank& r : g->ranks) {
        hipStream_t st = r.st;
        HIP_CHECK(hipMemcpyAsync(r.invls, pt.inv_ls.data(), sizeof(double) * D, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(r.noise, noise, sizeof(double) * noise_len, hipMemcpyHostToDevice, st));
        launch_scale_inputs(st, r.XsR, r.LR, D, r.invls, kp.ard, r.XtR, r.LR);
        launch_scale_inputs(st, r.XsC, r.LC, D, r.invls, kp.ard, r.XtC, r.LC);
        HIP_CHECK(hipMemsetAsync(r.A, 0, sizeof(double) * r.LR * r.LC, st));
        HIP_CHECK(hipMemsetAsync(r.X, 0, sizeof(double) * r.LR * r.LC, st));
        HIP_CHECK(hipMemsetAsync(r.W, 0, sizeof(double) * r.LR * r.LC, st));
        HIP_CHECK(hipMemsetAsync(r.scal, 0, sizeof(double) * 8, st));
        HIP_CHECK(hipMemsetAsync(r.info_g, 0, sizeof(int) * 4, st));
        if (r.nvr > 0 && r.nvc > 0) launch_kbuild_cross(st, kp, r.XtR, r.LR, r.nvr, r.XtC, r.LC, r.nvc, r.A, r.LC);
        if (r.ndiag > 0) {
            const long cnt = (long)r.ndiag * nb;
            hipLaunchKernelGGL(k_grid_fix_diag, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, r.A.p, r.LC, nb, g->n,
                               r.ndiag, r.dl_r.p, r.dl_c.p, r.dg.p, r.noise.p, (long)noise_len, jit);
        }
    }
    return 0;
}

// step k, the diagonal tile: (a) L_kk and D = L_kk^-1 on its owner, the factor back into A
static int grid_step_diag(mi355gp_grid* g, long k) {
    const long nb = g->nb, lkr = k / g->Pr, lkc = k / g->Pc;
    const int opr = (int)(k % g->Pr), opc = (int)(k % g->Pc), q = (int)(nb / NB);
    const size_t tile = (size_t)nb * nb;
    for (GridRank& r : g->ranks) {
        if (r.pr != opr || r.pc != opc) continue;
        hipStream_t s = crit_stream(g, r);
        double* At = r.A + lkr * nb * r.LC + lkc * nb;
        HIP_CHECK(hipMemcpy2DAsync(r.Dt, sizeof(double) * nb, At, sizeof(double) * r.LC, sizeof(double) * nb, nb,
                                   hipMemcpyDeviceToDevice, s));
        potrf_device(s, r.Dt, nb, &r.ws);
        hipLaunchKernelGGL(k_grid_tile_stats, dim3(1), dim3(64), 0, s, r.ws.logsum, q, r.ws.info, k * nb, r.scal.p,
                           r.info_g.p);
        HIP_CHECK(hipMemsetAsync(r.Dv, 0, sizeof(double) * tile, s));
        trtri_device(s, r.Dt, r.Dv, r.Ds, nb, &r.ws);
        hipLaunchKernelGGL(k_grid_inv_diag, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s, r.Dv.p, r.Dt.p, nb);
        HIP_CHECK(hipMemcpy2DAsync(At, sizeof(double) * r.LC, r.Dt, sizeof(double) * nb, sizeof(double) * nb, nb,
                                   hipMemcpyDeviceToDevice, s));
    }
    return 0;
}

// step k, the L panels: (b) D to its readers, (c) the panel solve, (d) the row panel along the process rows, (e) the column
// panel down the process columns.  nobc (diagnostics, dbg_crit >= 2): the broadcasts are skipped
static int grid_step_L_panels(mi355gp_grid* g, long k) {
    const long nb = g->nb, T = g->T, lkc = k / g->Pc;
    const int Pr = g->Pr, Pc = g->Pc, opr = (int)(k % Pr), opc = (int)(k % Pc);
    const size_t tile = (size_t)nb * nb;
    const bool nobc = g->dbg_crit >= 2;
    const GridPred nopred{0, 1, 0, 1, 0, 0, 0};
    // (b) D to the panel owners (process column opc) and to the owners of row k of X (process row opr)
    if (!nobc) {
        if (int rc = grid_bcast(g, GROUP_COL, opc, opr, tile, [](GridRank& r, bool) -> double* { return r.Dv; })) return rc;
        if (int rc = grid_bcast(g, GROUP_ROW, opr, opc, tile, [](GridRank& r, bool) -> double* { return r.Dv; })) return rc;
    }
    // (c) panel solve L_ik = A_ik D^T on process column opc
    for (GridRank& r : g->ranks) {
        if (r.pc != opc) continue;
        hipStream_t s = crit_stream(g, r);
        const int lr0 = cnt_le(k, r.pr, Pr);
        const long rows = (long)(r.TLr - lr0) * nb;
        if (rows <= 0) continue;
        double* Acol = r.A + (long)lr0 * nb * r.LC + lkc * nb;
        grid_gemm_t<true, true>(s, r.hRP[k] + (long)lr0 * tile, nb, 0, GOp{Acol, r.LC, 0}, GOp{r.Dv, nb, 0}, rows, nb,
                                nb, nb, 0, nopred);
        HIP_CHECK(hipMemcpy2DAsync(Acol, sizeof(double) * r.LC, r.hRP[k] + (long)lr0 * tile, sizeof(double) * nb,
                                   sizeof(double) * nb, rows, hipMemcpyDeviceToDevice, s));
    }
    // (d) row panel along every process row
    for (int pr = 0; pr < Pr && !nobc; ++pr) {
        const int lr0 = cnt_le(k, pr, Pr), TLr = cnt_le(T - 1, pr, Pr);
        const size_t cnt = (size_t)(TLr - lr0) * tile;
        if (int rc = grid_bcast(g, GROUP_ROW, pr, opc, cnt,
                                [&](GridRank& r, bool) { return r.hRP[k] + (long)lr0 * tile; }))
            return rc;
    }
    // (e) column panel: L_jk for the local columns j > k comes from process row j % Pr -- one broadcast per (process column,
    //     root) pair: at most Pr per column (grid_bcast_tile_runs)
    if (!nobc) {
        std::vector<TileRun> runs;
        for (int pc = 0; pc < Pc; ++pc)
            for (int root = 0; root < Pr; ++root) {
                long first, step;
                int cnt;
                tile_progression(k + 1, T, pc, Pc, root, Pr, &first, &step, &cnt);
                if (cnt > 0) runs.push_back(TileRun{GROUP_COL, pc, root, cnt, first / Pr, step / Pr, first / Pc, step / Pc});
            }
        if (int rc = grid_bcast_tile_runs(g, runs, tile, [&](GridRank& r) { return r.hRP[k]; }, [&](GridRank& r) { return r.hCP[k]; }))
            return rc;
    }
    return 0;
}

// step k, row k of X: (g) X_kj = D * B_kj (j < k), X_kk = D on process row opr and the row block back into X, (h) the X row
// panel down the process columns, (i) along the process rows
static int grid_step_X_row(mi355gp_grid* g, long k) {
    const long nb = g->nb, lkr = k / g->Pr;
    const int Pr = g->Pr, Pc = g->Pc, opr = (int)(k % Pr), opc = (int)(k % Pc);
    const size_t tile = (size_t)nb * nb;
    const bool nobc = g->dbg_crit >= 2;
    const GridPred nopred{0, 1, 0, 1, 0, 0, 0};
    // (g) row k of X on process row opr
    for (GridRank& r : g->ranks) {
        if (r.pr != opr) continue;
        hipStream_t s = crit_stream(g, r);
        const int lcB = cnt_lt(k, r.pc, Pc);                      // local columns with J < k
        const double* Brow = r.X + lkr * nb * r.LC;
        grid_gemm_t<true, false>(s, r.hXR[k], nb, 1, GOp{r.Dv, nb, 0}, GOp{Brow, r.LC, 0}, nb, (long)lcB * nb, nb, nb,
                                 0, nopred);
        if (r.pc == opc) HIP_CHECK(hipMemcpyAsync(r.hXR[k] + (long)lcB * tile, r.Dv, sizeof(double) * tile,
                                                  hipMemcpyDeviceToDevice, s));
        const int lc0 = cnt_le(k, r.pc, Pc);
        if (lc0 > 0)                                                // final X row block back into the local matrix
            hipLaunchKernelGGL(k_tiles_to_rowblock, dim3(64, (unsigned)lc0), dim3(256), 0, s, r.X + lkr * nb * r.LC, (long)r.LC,
                               (const double*)r.hXR[k], (int)nb);
    }
    // (h) X row panel down every process column
    for (int pc = 0; pc < Pc && !nobc; ++pc) {
        const size_t cnt = (size_t)cnt_le(k, pc, Pc) * tile;
        if (int rc = grid_bcast(g, GROUP_COL, pc, opr, cnt, [&](GridRank& r, bool) { return r.hXR[k]; })) return rc;
    }
    // (i) X_ki for the local rows i <= k comes from process column i % Pc -- at most Pc broadcasts per process row
    if (!nobc) {
        std::vector<TileRun> runs;
        for (int pr = 0; pr < Pr; ++pr)
            for (int root = 0; root < Pc; ++root) {
                long first, step;
                int cnt;
                tile_progression(0, k + 1, pr, Pr, root, Pc, &first, &step, &cnt);
                if (cnt > 0) runs.push_back(TileRun{GROUP_ROW, pr, root, cnt, first / Pc, step / Pc, first / Pr, step / Pr});
            }
        if (int rc = grid_bcast_tile_runs(g, runs, tile, [&](GridRank& r) { return r.hXR[k]; }, [&](GridRank& r) { return r.hXRr[k]; }))
            return rc;
    }
    return 0;
}

// crit(k), the critical path of step k: diagonal tile k, D = L_kk^-1, the panel solves, row k of X and ALL panel broadcasts
static int grid_crit(mi355gp_grid* g, long k) {
    if (int rc = grid_step_diag(g, k)) return rc;
    if (g->dbg_crit >= 3) return 0;
    if (int rc = grid_step_L_panels(g, k)) return rc;
    return grid_step_X_row(g, k);
}

// updates of A and B by the panels [k0, k1) on local tile columns J in [ca, cb) (A, rows I >= ca) and tile rows I in
// [ca, cb) (B, columns J < k1; panel k reaches the columns J <= k), on the critical-path stream or on st
static void grid_update_AB(mi355gp_grid* g, bool on_crit, long k0, long k1, long ca, long cb) {
    if (g->dbg_crit) return;
    const int Pr = g->Pr, Pc = g->Pc;
    for (GridRank& r : g->ranks) {
        hipStream_t s = on_crit ? crit_stream(g, r) : r.st;
        const GridPred lower{1, Pr, r.pr, Pc, r.pc, 0, 0}, all{0, Pr, r.pr, Pc, r.pc, 0, 0};
        grid_gemm_multi<true, true, 2>(s, r.A, r.LC, r.dRP, r.dCP, (int)k0, (int)k1, cnt_lt(ca, r.pr, Pr), r.TLr,
                                       cnt_lt(ca, r.pc, Pc), cnt_lt(cb, r.pc, Pc), g->nb, 0, lower);
        grid_gemm_multi<true, false, 2>(s, r.X, r.LC, r.dRP, r.dXR, (int)k0, (int)k1, cnt_lt(ca, r.pr, Pr),
                                        cnt_lt(cb, r.pr, Pr), 0, cnt_lt(k1, r.pc, Pc), g->nb, 1, all);
    }
}

// W_ij += sum over the steps k in [k0, k1) of X_ki^T X_kj, k >= i >= j, on the low-priority stream: fills whatever the other
// two leave idle
static void grid_update_W(mi355gp_grid* g, long k0, long k1) {
    const int Pr = g->Pr, Pc = g->Pc;
    for (GridRank& r : g->ranks) {
        const GridPred lower{1, Pr, r.pr, Pc, r.pc, 0, 0};
        grid_gemm_multi<false, false, 1>(g->lookahead ? r.sw : r.st, r.W, r.LC, r.dXRr, r.dXR, (int)k0, (int)k1, 0,
                                         cnt_lt(k1, r.pr, Pr), 0, cnt_lt(k1, r.pc, Pc), g->nb, 2, lower);
    }
}

// ---- factor and invert: the one-pass factorisation / inversion, two-level blocked ------------------------------------------
// Steps are taken in GROUPS of G (MI355GP_GRID_G).  Every step k runs its critical path crit(k) -- diagonal tile k,
// D = L_kk^-1, the panel solves, row k of X and ALL panel broadcasts -- and then brings only the REST OF ITS GROUP up to
// date with K = nb updates (near(k): tile columns k+1 .. ge-1 of A, tile rows k+1 .. ge-1 of B; ge = first step of the
// next group).  Everything beyond the group receives the group's G panels in ONE pass over C with K = G * nb
// (k_grid_gemm_multi): first the next group's columns / rows (part1(g), on the critical path), then the bulk.  W = X^T X is
// not read by anything before the end: its updates are aggregated over GW steps (MI355GP_GRID_GW; 0 = one deep-K pass
// after the last step, the distributed lauum).  The three read-modify-write passes per step of the one-level form
// become one pass per G (A, B) and per GW (W) steps: the C traffic of the updates drops accordingly and the tile
// pipeline runs K = G * nb deep (k_grid_gemm at K = 512: 0.61 of the fp64 peak; lauum-deep: 0.87).
// Two streams per rank, one group of look-ahead:
//   sc (high priority): crit(k), near(k) for the steps of group g, then part1(g) [after bulk(g-1): both write the
//                       columns / rows of group g+1], then group g+1
//   st                : bulk(g) [after crit of the group's last step]
//   sw (low priority) : the W updates [after crit of the last step they read]; st joins it after the loop
// bulk(g) touches columns / rows >= the start of group g+2 only, the critical path of group g+1 stays inside group
// g+1's columns / rows: they run concurrently.  The X panels keep one buffer per step for the whole evaluation (the
// deferred W = X^T X reads them late); the L panels live in a RING of 2 G full-height slots (alloc_panel_stores): slot
// reuse is safe because sc waits for ev_p1[gi-1] -- i.e. for bulk(g-1) on st -- before part1(g), so every reader of group
// g's panels has been enqueued behind the event that group g+2's crit (the next writer of those slots) waits for.
// Every rank enqueues the same sequence of collectives on sc, so their order is consistent across the grid.
static int grid_factor_invert(mi355gp_grid* g) {
    const bool la = g->lookahead != 0;
    hipStream_t scs = la ? g->sc : g->st;
    const long T = g->T, G = g->G < 1 ? 1 : g->G, GW = g->GW;
    if (la) {
        HIP_CHECK(hipEventRecord(g->ev[5], g->st));          // the covariance tiles precede everything on sc / sw
        HIP_CHECK(hipStreamWaitEvent(g->sc, g->ev[5], 0));
        HIP_CHECK(hipStreamWaitEvent(g->sw, g->ev[5], 0));
    }
    long kw0 = 0;                                            // first step whose X panels W has not received yet
    const long ngroups = (T + G - 1) / G;
    for (long gi = 0; gi < ngroups; ++gi) {
        const long kb = gi * G, ge = (kb + G < T) ? kb + G : T, ge2 = (ge + G < T) ? ge + G : T;
        for (long k = kb; k < ge; ++k) {
            if (int rc = grid_crit(g, k)) return rc;
            if (k + 1 < ge) grid_update_AB(g, true, k, k + 1, k + 1, ge);          // near(k)
        }
        if (la) HIP_CHECK(hipEventRecord(g->ev_cr[gi], scs));
        if (ge < T) {                                                              // part1(g): the next group's columns / rows
            if (la && gi > 0) HIP_CHECK(hipStreamWaitEvent(g->sc, g->ev_p1[gi - 1], 0));
            grid_update_AB(g, true, kb, ge, ge, ge2);
        }
        if (la) HIP_CHECK(hipStreamWaitEvent(g->st, g->ev_cr[gi], 0));
        if (ge2 < T) grid_update_AB(g, false, kb, ge, ge2, T);                     // bulk(g)
        if (la) HIP_CHECK(hipEventRecord(g->ev_p1[gi], g->st));
        const bool flush = !g->dbg_crit && ((ge == T) || (GW > 0 && ge - kw0 >= GW));
        if (flush) {                                                               // W over the finished steps
            if (la) HIP_CHECK(hipStreamWaitEvent(g->sw, g->ev_cr[gi], 0));
            grid_update_W(g, kw0, ge);
            kw0 = ge;
        }
    }
    if (la) {
        HIP_CHECK(hipEventRecord(g->ev_w, g->sw));
        HIP_CHECK(hipStreamWaitEvent(g->st, g->ev_w, 0));
    }
    return 0;
}

// vloc[j] = sum_i X_ij * (v ? v[g(i)][d] : X_ij)
static void grid_col_reduce(mi355gp_grid* g, GridRank& r, const double* v, int d) {
    const long nch = (r.LR + CR_ROWS - 1) / CR_ROWS;
    hipLaunchKernelGGL(k_grid_col_reduce_part, dim3((unsigned)((r.LC + 63) / 64), (unsigned)nch), dim3(256), 0, r.st, r.X.p,
                       r.LC, r.LR, r.LC, r.gR.p, v, v ? g->Dy : 1, d, g->n, r.cpart.p, g->nb, g->Pr, r.pr, g->Pc, r.pc);
    hipLaunchKernelGGL(k_grid_col_combine, dim3((unsigned)((r.LC + 255) / 256)), dim3(256), 0, r.st, r.cpart.p, nch, r.LC,
                       r.vloc.p);
}

// solve: y = X R, alpha = X^T y, diag W, and the sums over ranks (logdet and the failure counts travel in scal)
static int grid_solve(mi355gp_grid* g) {
    const long n = g->n;
    const int Dy = g->Dy;
    for (GridRank& r : g->ranks) {                       // y = X R (partial over the local columns)
        HIP_CHECK(hipMemsetAsync(r.ybuf, 0, sizeof(double) * n * Dy, r.st));
        for (int d = 0; d < Dy; ++d) {
            hipLaunchKernelGGL(k_grid_row_reduce, dim3((unsigned)((r.LR + 3) / 4)), dim3(256), 0, r.st, r.X.p, r.LC, r.LR,
                               r.LC, r.gC.p, r.Rg.p, Dy, d, n, r.vloc.p);
            hipLaunchKernelGGL(k_grid_scatter, dim3((unsigned)((r.LR + 255) / 256)), dim3(256), 0, r.st, r.vloc.p, r.LR,
                               r.gR.p, n, Dy, d, r.ybuf.p);
        }
    }
    // NB: a rank's partial y covers only its local columns, and ranks of one process row write the same global
    // rows: the scatter above must not overwrite -- every rank owns a private ybuf, and the all-reduce sums them.
    if (int rc = grid_allreduce(g, (size_t)n * Dy, [](GridRank& r) -> double* { return r.ybuf; })) return rc;
    for (GridRank& r : g->ranks) {                       // alpha = X^T y (partial over the local rows), diag W
        HIP_CHECK(hipMemsetAsync(r.alpha, 0, sizeof(double) * n * Dy, r.st));
        HIP_CHECK(hipMemsetAsync(r.gvec2, 0, sizeof(double) * n, r.st));
        for (int d = 0; d < Dy; ++d) {
            grid_col_reduce(g, r, r.ybuf, d);
            hipLaunchKernelGGL(k_grid_scatter, dim3((unsigned)((r.LC + 255) / 256)), dim3(256), 0, r.st, r.vloc.p, r.LC,
                               r.gC.p, n, Dy, d, r.alpha.p);
        }
        grid_col_reduce(g, r, nullptr, 0);
        hipLaunchKernelGGL(k_grid_scatter, dim3((unsigned)((r.LC + 255) / 256)), dim3(256), 0, r.st, r.vloc.p, r.LC, r.gC.p,
                           n, 1, 0, r.gvec2.p);
    }
    if (int rc = grid_allreduce(g, (size_t)n * Dy, [](GridRank& r) -> double* { return r.alpha; })) return rc;
    if (int rc = grid_allreduce(g, (size_t)n, [](GridRank& r) -> double* { return r.gvec2; })) return rc;
    return grid_allreduce(g, 8, [](GridRank& r) -> double* { return r.scal; });
}

// gradient: the reduction over the local dL_dK tiles, summed over ranks
static int grid_gradient(mi355gp_grid* g, const KernParams& kp) {
    const int groups = (g->D + 31) / 32;
    for (GridRank& r : g->ranks) {
        HIP_CHECK(hipMemsetAsync(r.gradOut, 0, sizeof(double) * groups * GP_STRIDE, r.st));
        if (r.nvr <= 0 || r.nvc <= 0) continue;
        // W is consumed in place: dL/dK overwrites it once diag W has been taken
        hipLaunchKernelGGL(k_grid_dldk, dim3((unsigned)((r.nvc + 255) / 256), (unsigned)r.nvr), dim3(256), 0, r.st, r.W.p,
                           r.W.p, r.LC, r.nvr, r.nvc, r.gR.p, r.gC.p, r.alpha.p, g->Dy, g->n);
        const int nbk = grad_generic_num_blocks(r.nvr, r.nvc);
        launch_grad_generic(r.st, kp, r.XtR, r.LR, r.nvr, r.XtC, r.LC, r.nvc, 0, r.W, r.LC, r.gradPart);
        for (int gi = 0; gi < (kp.ard ? groups : 1); ++gi)
            launch_reduce_partials(r.st, r.gradPart + (long)gi * nbk * GP_STRIDE, nbk, GP_STRIDE,
                                   r.gradOut + (long)gi * GP_STRIDE);
    }
    return grid_allreduce(g, (size_t)groups * GP_STRIDE, [](GridRank& r) -> double* { return r.gradOut; });
}

// what the host reads back from an evaluation (the results are replicated on every rank: rank 0's copy)
struct GridHost {
    std::vector<double> alpha, dW, R, sums;
    double scal[8];
    int info = 0;
    bool redo = false;               // a persistent tile factorisation did not run: the evaluation has to be redone
};

// collect: copy to the host, agree on info across ranks, check the collective sequences, decide on a redo
static int grid_collect(mi355gp_grid* g, GridHost& h) {
    const long n = g->n;
    const int Dy = g->Dy, groups = (g->D + 31) / 32;
    GridRank& r0 = g->ranks[0];
    h.alpha.resize((size_t)n * Dy);
    h.dW.resize((size_t)n);
    h.R.resize((size_t)n * Dy);
    h.sums.resize((size_t)groups * GP_STRIDE);
    HIP_CHECK(hipMemcpyAsync(h.alpha.data(), r0.alpha, sizeof(double) * n * Dy, hipMemcpyDeviceToHost, g->st));
    HIP_CHECK(hipMemcpyAsync(h.dW.data(), r0.gvec2, sizeof(double) * n, hipMemcpyDeviceToHost, g->st));
    HIP_CHECK(hipMemcpyAsync(h.R.data(), r0.Rg, sizeof(double) * n * Dy, hipMemcpyDeviceToHost, g->st));
    HIP_CHECK(hipMemcpyAsync(h.sums.data(), r0.gradOut, sizeof(double) * groups * GP_STRIDE, hipMemcpyDeviceToHost, g->st));
    HIP_CHECK(hipMemcpyAsync(h.scal, r0.scal, sizeof(double) * 8, hipMemcpyDeviceToHost, g->st));
    HIP_CHECK(hipStreamSynchronize(g->st));
    // Every rank must take the same branch of the caller's jitter ladder: "some tile failed" travels in the all-reduced
    // scal[1]; the failing column itself is only known to the ranks hosting that tile (others report N).
    for (GridRank& r : g->ranks) {
        int ir = 0;
        HIP_CHECK(hipMemcpy(&ir, r.info_g, sizeof(int), hipMemcpyDeviceToHost));
        if (ir > 0 && (h.info == 0 || ir < h.info)) h.info = ir;
    }
    if (h.scal[1] > 0.0 && h.info == 0) h.info = (int)n;
    HIP_CHECK(hipGetLastError());
    if (g->check_seq)
        if (int rc = grid_check_sequences(g)) return rc;
    if (h.scal[2] > 0.0) {
        // A persistent factorisation of a diagonal tile was called off (co-residency gate) or aborted on some rank: the count
        // travels in the all-reduced scal[2], so EVERY rank takes this branch and the collectives of the redone evaluation
        // line up.  The tile factorisations stay on the launch-per-step schedule from here on.
        for (GridRank& r : g->ranks) {
            r.ws.persist_aborts += 1;
            r.ws.persist = 0;
        }
        h.redo = true;
    }
    return 0;
}

// the caller's outputs of one evaluation
struct GridOut {
    double *scalars, *alpha, *dtheta, *diag, *stage_ms;
};

static int grid_stage_times(mi355gp_grid* g, double* stage_ms) {
    for (int i = 0; i < MI355GP_NUM_T; ++i) stage_ms[i] = 0.0;
    float ms;
    const int map[4] = {MI355GP_T_KBUILD, MI355GP_T_POTRF, MI355GP_T_SOLVE, MI355GP_T_GRAD};
    for (int i = 0; i < 4; ++i) {
        HIP_CHECK(hipEventElapsedTime(&ms, g->ev[i], g->ev[i + 1]));
        stage_ms[map[i]] = ms;
    }
    HIP_CHECK(hipEventElapsedTime(&ms, g->ev[0], g->ev[4]));
    stage_ms[MI355GP_T_TOTAL] = ms;
    return 0;
}

// the scalars and vectors of the result from what grid_collect read back; returns the LAPACK-style info of a failed factorisation
static int grid_assemble(mi355gp_grid* g, const PartSpec& pt, const GridHost& h, const GridOut& out) {
    const long n = g->n;
    const int Dy = g->Dy;
    int info = h.info;
    // a failed factorisation poisons logdet/alpha with NaN on every rank: detect it everywhere, not only on the owner
    double datafit = 0.0, alpha2 = 0.0, trw = 0.0;
    for (long i = 0; i < n * Dy; ++i) {
        datafit += h.alpha[i] * h.R[i];
        alpha2 += h.alpha[i] * h.alpha[i];
    }
    for (long i = 0; i < n; ++i) trw += h.dW[i];
    const double logdet = 2.0 * h.scal[0];
    if (info == 0 && !(std::isfinite(logdet) && std::isfinite(datafit))) info = (int)n;
    if (info > 0) {
        g->have_result = false;
        return info > n ? (int)n : info;
    }
    g->have_result = true;
    for (int i = 0; i < MI355GP_NUM_OUT; ++i) out.scalars[i] = 0.0;
    out.scalars[MI355GP_OUT_LML] = 0.5 * (-(double)n * Dy * LOG_2_PI - Dy * logdet - datafit);
    out.scalars[MI355GP_OUT_LOGDET] = logdet;
    out.scalars[MI355GP_OUT_DATAFIT] = datafit;
    out.scalars[MI355GP_OUT_DNOISE] = 0.5 * (alpha2 - Dy * trw);
    out.scalars[MI355GP_OUT_TRKINV] = trw;
    if (out.alpha) memcpy(out.alpha, h.alpha.data(), sizeof(double) * n * Dy);
    if (out.diag)
        for (long i = 0; i < n; ++i) {
            double a2 = 0.0;
            for (int d = 0; d < Dy; ++d) a2 += h.alpha[i * Dy + d] * h.alpha[i * Dy + d];
            out.diag[i] = 0.5 * (a2 - Dy * h.dW[i]);
        }
    if (out.dtheta) part_dtheta(pt, h.sums.data(), nullptr, out.dtheta);
    return 0;
}

// The driver.  ev[0..4] bracket the four timed stages on st; a pass that met a called-off persistent tile factorisation is
// redone once on the launch-per-step schedule.
static int grid_run(mi355gp_grid* g, const PartSpec& pt, const double* noise, int64_t noise_len, double jit, const GridOut& out) {
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (int rc = grid_prepare(g)) return rc;
        HIP_CHECK(hipEventRecord(g->ev[0], g->st));
        if (int rc = grid_build_K(g, pt, noise, noise_len, jit)) return rc;
        HIP_CHECK(hipEventRecord(g->ev[1], g->st));
        if (int rc = grid_factor_invert(g)) return rc;
        HIP_CHECK(hipEventRecord(g->ev[2], g->st));
        if (int rc = grid_solve(g)) return rc;
        HIP_CHECK(hipEventRecord(g->ev[3], g->st));
        if (int rc = grid_gradient(g, pt.kp)) return rc;
        HIP_CHECK(hipEventRecord(g->ev[4], g->st));
        GridHost h;
        if (int rc = grid_collect(g, h)) return rc;
        if (h.redo) continue;
        if (out.stage_ms)
            if (int rc = grid_stage_times(g, out.stage_ms)) return rc;
        return grid_assemble(g, pt, h, out);
    }
    mi355gp_set_error("mi355gp_grid_exact_inference: a tile factorisation aborted twice");
    return -6;
}

extern "C" {

int mi355gp_grid_exact_inference(mi355gp_grid* g, int kind, int ard, const double* theta, const double* noise,
                                 int64_t noise_len, double jitter, double extra_jitter, double* out_scalars,
                                 double* alpha_out, double* dtheta_out, double* diag_dLdK_out, double* stage_ms) {
    ARG_CHECK(g && g->n > 0, "mi355gp_grid_exact_inference: set_data first");
    ARG_CHECK(out_scalars && theta && noise, "mi355gp_grid_exact_inference: NULL argument");
    if (int rc = check_kind(kind, KS_STATIONARY, "grid path")) return rc;     // (not the exact-only kinds 6 / 7 / 8)
    if (g->single) {
        double ms[MI355GP_NUM_T];
        const int rc = mi355gp_exact_inference(g->single, kind, ard, theta, noise, noise_len, jitter, extra_jitter, out_scalars,
                                               alpha_out, dtheta_out, diag_dLdK_out, stage_ms ? ms : nullptr);
        if (stage_ms) {       // the grid's stage layout: the whole factorisation + inversion under POTRF
            for (int i = 0; i < MI355GP_NUM_T; ++i) stage_ms[i] = 0.0;
            stage_ms[MI355GP_T_KBUILD] = ms[MI355GP_T_KBUILD];
            stage_ms[MI355GP_T_POTRF] = ms[MI355GP_T_POTRF] + ms[MI355GP_T_TRTRI] + ms[MI355GP_T_LAUUM];
            stage_ms[MI355GP_T_SOLVE] = ms[MI355GP_T_SOLVE];
            stage_ms[MI355GP_T_GRAD] = ms[MI355GP_T_GRAD];
            stage_ms[MI355GP_T_TOTAL] = ms[MI355GP_T_TOTAL];
        }
        g->have_result = (rc == 0);
        return rc;
    }
    ARG_CHECK(noise_len == 1 || noise_len == g->n, "noise must have 1 or N entries");
    PartSpec pt;
    if (int rc = parse_part(mi355gp_part{kind, ard, 0, nullptr, theta, 0}, g->D, KS_STATIONARY, "grid path", &pt)) return rc;
    HIP_CHECK(hipSetDevice(g->device));
    return grid_run(g, pt, noise, noise_len, jitter + extra_jitter,
                    GridOut{out_scalars, alpha_out, dtheta_out, diag_dLdK_out, stage_ms});
}

int mi355gp_grid_set_option(mi355gp_grid* g, int option, int value) {
    ARG_CHECK(g && option >= 0 && option < MI355GP_GRID_OPT_NUM, "mi355gp_grid_set_option: unknown option");
    ARG_CHECK(value >= -1, "mi355gp_grid_set_option: value must be >= 0 (or -1 for the default)");
    if (g->single) return 0;                              // the degenerate 1 x 1 grid runs the single-GPU pipeline
    if (value < 0) {
        grid_default_option(g, option);
        return 0;
    }
    if (option == MI355GP_GRID_OPT_LOOKAHEAD) g->lookahead = value ? 1 : 0;
    else if (option == MI355GP_GRID_OPT_G) {
        ARG_CHECK(value >= 1, "mi355gp_grid_set_option: G >= 1");
        g->G = value;
    } else if (option == MI355GP_GRID_OPT_CHECK_SEQ) g->check_seq = value ? 1 : 0;
    else g->GW = value;
    return 0;
}

int mi355gp_grid_get_option(mi355gp_grid* g, int option, int* value) {
    ARG_CHECK(g && value && option >= 0 && option < MI355GP_GRID_OPT_NUM, "mi355gp_grid_get_option: unknown option");
    *value = option == MI355GP_GRID_OPT_LOOKAHEAD ? g->lookahead : option == MI355GP_GRID_OPT_G ? g->G
             : option == MI355GP_GRID_OPT_CHECK_SEQ ? g->check_seq : g->GW;
    return 0;
}

// Host copy of the tiles owned by this process's ranks, placed at their global position in an N x N row-major array
// (entries owned by other processes are left untouched: callers zero `out` first and sum over ranks).
// which: MI355GP_FETCH_L (lower tiles of L), MI355GP_FETCH_KINV is not available after the gradient pass consumed W;
// 100 = X = L^-1 (lower).
int mi355gp_grid_fetch(mi355gp_grid* g, int which, double* out) {
    ARG_CHECK(g && out && g->n > 0 && g->have_result, "mi355gp_grid_fetch: run an inference call first");
    ARG_CHECK(which == MI355GP_FETCH_L || which == 100, "mi355gp_grid_fetch: L (0) or L^-1 (100)");
    if (g->single) return mi355gp_fetch(g->single, which, out, 0);
    HIP_CHECK(hipSetDevice(g->device));
    const long nb = g->nb, n = g->n;
    std::vector<double> tilebuf((size_t)nb * nb);
    for (GridRank& r : g->ranks) {
        const double* M = (which == MI355GP_FETCH_L) ? r.A : r.X;
        for (int li = 0; li < r.TLr; ++li)
            for (int lj = 0; lj < r.TLc; ++lj) {
                const long I = (long)li * g->Pr + r.pr, J = (long)lj * g->Pc + r.pc;
                if (J > I) continue;
                HIP_CHECK(hipMemcpy2D(tilebuf.data(), sizeof(double) * nb, M + (long)li * nb * r.LC + (long)lj * nb,
                                      sizeof(double) * r.LC, sizeof(double) * nb, nb, hipMemcpyDeviceToHost));
                for (long a = 0; a < nb; ++a) {
                    const long gi = I * nb + a;
                    if (gi >= n) break;
                    for (long b = 0; b < nb; ++b) {
                        const long gj = J * nb + b;
                        if (gj >= n || gj > gi) break;
                        out[gi * n + gj] = tilebuf[(size_t)a * nb + b];
                    }
                }
            }
    }
    return 0;
}

// Microbenchmark of the deep-K W = X^T X pass on ONE device (1 x 1 layout, T tiles of nb): out_ms[v] for
//   v = 0: k_lauum on the row-major matrix (the single-GPU path's kernel)
//   v = 1: k_grid_gemm_multi on the tile-major panel stores (two copies: XRr and XR), as the grid mode runs it
//   v = 2: the same with ONE panel store for both operands
//   v = 3: k_grid_gemm_multi reading the row-major matrix (panel k = rows k*nb ..)
int mi355gp_dbg_grid_multi(int device, int T, int nb, int reps, double* out_ms) {
    ARG_CHECK(T >= 1 && nb >= NB && nb % NB == 0 && reps >= 1 && out_ms, "mi355gp_dbg_grid_multi: bad arguments");
    HIP_CHECK(hipSetDevice(device));
    const long N = (long)T * nb;
    const size_t tile = (size_t)nb * nb;
    double *X = nullptr, *W = nullptr, *P1 = nullptr, *P2 = nullptr;
    const double **t1 = nullptr, **t2 = nullptr, **t3 = nullptr;
    HIP_CHECK(hipMalloc(&X, sizeof(double) * N * N));
    HIP_CHECK(hipMalloc(&W, sizeof(double) * N * N));
    const long ntl = (long)T * (T + 1) / 2;
    HIP_CHECK(hipMalloc(&P1, sizeof(double) * tile * ntl));
    HIP_CHECK(hipMalloc(&P2, sizeof(double) * tile * ntl));
    {
        std::vector<double> h((size_t)N * 64);
        for (size_t i = 0; i < h.size(); ++i) h[i] = 1e-3 * (double)((i * 2654435761u) % 1024) - 0.5;
        for (long r = 0; r < N; r += 64) HIP_CHECK(hipMemcpy(X + r * N, h.data(), sizeof(double) * N * 64, hipMemcpyHostToDevice));
    }
    std::vector<const double*> h1((size_t)T), h2((size_t)T), h3((size_t)T);
    long off = 0;
    for (long k = 0; k < T; ++k) {
        h1[k] = P1 + off * tile;
        h2[k] = P2 + off * tile;
        h3[k] = X + k * nb * N;
        for (long j = 0; j <= k; ++j) {
            HIP_CHECK(hipMemcpy2D(P1 + (off + j) * tile, sizeof(double) * nb, X + k * nb * N + j * nb, sizeof(double) * N,
                                  sizeof(double) * nb, nb, hipMemcpyDeviceToDevice));
        }
        off += k + 1;
    }
    HIP_CHECK(hipMemcpy(P2, P1, sizeof(double) * tile * ntl, hipMemcpyDeviceToDevice));
    const size_t tb = sizeof(double*) * (size_t)T;
    HIP_CHECK(hipMalloc((void**)&t1, tb));
    HIP_CHECK(hipMalloc((void**)&t2, tb));
    HIP_CHECK(hipMalloc((void**)&t3, tb));
    HIP_CHECK(hipMemcpy((void*)t1, h1.data(), tb, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy((void*)t2, h2.data(), tb, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy((void*)t3, h3.data(), tb, hipMemcpyHostToDevice));
    hipStream_t st;
    HIP_CHECK(hipStreamCreate(&st));
    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
    const GridPred lower{1, 1, 0, 1, 0, 0, 0};
    for (int v = 0; v < 5; ++v) {
        for (int rep = -1; rep < reps; ++rep) {
            if (rep == 0) HIP_CHECK(hipEventRecord(e0, st));
            if (v == 0) launch_lauum(st, X, W, N, (int)(N / NB));
            else if (v == 1) grid_gemm_multi<false, false, 0>(st, W, N, t1, t2, 0, T, 0, T, 0, T, nb, 2, lower);
            else if (v == 2) grid_gemm_multi<false, false, 0>(st, W, N, t1, t1, 0, T, 0, T, 0, T, nb, 2, lower);
            else if (v == 3) grid_gemm_multi<false, false, 0>(st, W, N, t3, t3, 0, T, 0, T, 0, T, nb, 2, lower, N, 0);
            else grid_gemm_multi<false, false, 0>(st, W, N, t3, t3, 0, T, 0, T, 0, T, nb, 2, lower, N, 2);
        }
        HIP_CHECK(hipEventRecord(e1, st));
        HIP_CHECK(hipStreamSynchronize(st));
        float ms = 0.f;
        HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
        out_ms[v] = ms / reps;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipStreamDestroy(st);
    for (void* p : {(void*)X, (void*)W, (void*)P1, (void*)P2, (void*)t1, (void*)t2, (void*)t3}) (void)hipFree(p);
    return 0;
}

}  // extern "C"
