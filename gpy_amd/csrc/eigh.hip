// eigh.hip -- fp64 eigendecomposition of a symmetric positive semi-definite matrix on the device (C-ABI mi355gp_eigh,
// include/mi355gp_eigh.h; eigh_device for callers inside the library, eigh.h).  DESIGN.md 6v.
//
// Blocked one-sided Jacobi (Hestenes): G = A and V = I are kept COLUMN-major (a column is contiguous), L x L with L = n rounded
// up to the block width EB = 32, the padding zero.  Only columns are ever combined, G <- G J and V <- V J with orthogonal J, so
// G = A V holds throughout and V stays orthogonal whatever J was.  The columns of G end up mutually orthogonal; G^T G = V^T A^2 V
// is then diagonal, the v_j are eigenvectors of A^2 and, A being positive semi-definite, of A, with lambda_j = v_j^T g_j.
//
// One sweep is T - 1 rounds of a round-robin tournament on the T = nb (+ 1 bye when nb is odd) column blocks; the T / 2 block
// pairs of a round touch disjoint columns and run in the same three launches:
//   k_eigh_gram   the 64 x 64 Gram W = [G_p G_q]^T [G_p G_q] of every pair on v_mfma_f64_16x16x4, the rows cut into chunks that
//                 different workgroups take (a partial W each; k ascending inside a chunk);
//   k_eigh_sub    one workgroup per pair: adds the partial Grams in chunk order, diagonalises W by cyclic two-sided Jacobi
//                 entirely in LDS (32 disjoint rotations per step, 63 steps per inner sweep, at most EIGH_INNER inner sweeps) and
//                 leaves the accumulated rotation J, brought back to orthogonality by one Newton-Schulz step, its columns
//                 permuted so that the pair's columns come out in descending order of norm;
//   k_eigh_apply  [G_p G_q] J and [V_p V_q] J on the matrix pipe, J held in registers as the MFMA's A operand, 16 rows of the
//                 panel at a time read, multiplied and written back in place (a wave owns its rows: nothing else reads them).
// A pair whose partner is the bye runs the same code on [G_p 0]: its 32 columns are orthogonalised among themselves, which is
// also all there is to do when n <= 32.
//
// Degenerate columns.  A rotation is skipped when |w_ij| <= eps sqrt(w_ii w_jj) (exact zeros skip: the zero columns of the
// padding are never mixed into anything) and when either column's squared norm is at most eps^2 times the largest squared
// column norm of G at the start of the sweep: such a column is rounding noise of A's null space, where any orthonormal basis
// serves.  (The factor is eps and not n eps: a column g_j = A v_j left alone at norm tau lambda_max IS a residual of tau, and
// with n eps the residual measured n eps, the whole allowance of a backward-stable method, on rank-deficient RBF matrices; with
// eps it measured below LAPACK's and the sweep counts stayed the same, because termination does not hang on this rule.)
// Convergence: a pair raises the sweep's flag when it rotated at |w_ij| > L eps m (sqrt(w_ii) + sqrt(w_jj)), m the largest column
// norm (an upper estimate of lambda_max): with M = V^T A V and G^T G = M^2, w_ij is (m_i + m_j) M_ij to first order, so the flag
// asks whether an off-diagonal entry of V^T A V -- a residual -- still stands above L eps ||A||, the rounding of the L-term sums
// behind it.  A test relative to sqrt(w_ii w_jj) alone asks more than a norm-wise backward-stable method can give on a graded
// spectrum: a column of norm 1e-6 carries eps ||A|| of absolute noise, 1e-7 of its own length.  The rotations below the
// flag's level are still applied.  The host reads the flag once per sweep and stops at the first sweep that left it down, or at
// MI355GP_EIGH_MAX_SWEEPS (reported, never spun on).  No kernel loops on data without a fixed bound.
//
// Reproducibility: every sum has a fixed order (k ascending per chunk, chunks ascending, lane trees by xor-shuffle), the flags
// are integers, there are no floating-point atomics.
#include <cfloat>
#include <vector>

#include "../../include/mi355gp_eigh.h"
#include "eigh.h"

#define EB MI355GP_EIGH_B
#define EW (2 * EB)           // columns of a pair = order of a subproblem
#define EWW (EW * EW)
#define ELD (EW + 1)          // LDS row stride of W and J: odd, so a column walk hits 64 different banks
#define EG_KS 32              // rows per LDS slab of the Gram kernel
#define EG_LD (EG_KS + 1)
#define EA_ROWS 256           // rows of the panel per workgroup of the apply kernel
#define EIGH_NFLAGS 32        // one flag per sweep (MI355GP_EIGH_MAX_SWEEPS = 30 of them)
#define EIGH_INNER 12         // inner sweeps of a subproblem at most
#define ES_LDS_BYTES ((2 * EW * ELD + 2 * EB) * 8 + (2 * EB + 4) * 4)

// Round r (0 .. T-2) of the circle tournament on T players (T even), table k (0 .. T/2-1): player T-1 keeps its seat, the others
// move round; lo < hi are the two players.
__device__ __forceinline__ void eigh_pairing(int T, int r, int k, int* lo, int* hi) {
    const int m = T - 1;
    const int a = (k == 0) ? r : (r + k) % m, b = (k == 0) ? m : (r + m - k) % m;
    *lo = a < b ? a : b;
    *hi = a < b ? b : a;
}

// global column of column c (0 .. 63) of the pair (p, q)
__device__ __forceinline__ long eigh_col(int p, int q, int c) { return c < EB ? (long)p * EB + c : (long)q * EB + (c - EB); }

// G (column-major L x L) = A padded with zeros, V = I on the n leading columns; the sweep flags are lowered
__global__ __launch_bounds__(256) void k_eigh_init(const double* __restrict__ A, long lda, long n, long L, double* __restrict__ G,
                                                   double* __restrict__ V, int* __restrict__ flags) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx < EIGH_NFLAGS) flags[idx] = 0;
    if (idx >= L * L) return;
    const long j = idx / L, i = idx - j * L;
    const bool in = i < n && j < n;
    G[idx] = in ? (i >= j ? A[i * lda + j] : A[j * lda + i]) : 0.0;
    V[idx] = (in && i == j) ? 1.0 : 0.0;
}

// out[j] = sum_i X[i][j] Y[i][j], one wave per column: a lane adds its rows in ascending order, the 64 lane sums go down an
// xor-shuffle tree.  The squared column norms (X = Y = G) and, at the end, lambda_j = v_j^T g_j.
__global__ __launch_bounds__(256) void k_eigh_coldot(const double* __restrict__ X, const double* __restrict__ Y, long L,
                                                     double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long j = (long)blockIdx.x * 4 + (threadIdx.x >> 6);              // L is a multiple of 32: j < L
    const double *x = X + j * L, *y = Y + j * L;
    double s = 0.0;
    for (long i = lane; i < L; i += 64) s += x[i] * y[i];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) out[j] = s;
}

// tiny2[0] = eps^2 max_j norm2[j], tiny2[1] = max_j norm2[j]: squared column norms at or below it count as converged in this sweep (one workgroup)
__global__ __launch_bounds__(256) void k_eigh_tiny(const double* __restrict__ norm2, long L, double* __restrict__ tiny2) {
    __shared__ double red[256];
    double m = 0.0;
    for (long j = threadIdx.x; j < L; j += 256) m = fmax(m, norm2[j]);
    red[threadIdx.x] = m;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        tiny2[0] = DBL_EPSILON * DBL_EPSILON * red[0];
        tiny2[1] = red[0];
    }
}

// Partial Gram of pair blockIdx.x over the rows of chunk blockIdx.y.  The 64 columns of the pair are staged 32 rows at a time into
// LDS (each thread 8 consecutive rows of one column); wave w owns rows 16 w .. 16 w + 15 of W and all four column tiles.  Both MFMA
// operands are columns of the panel: A[row = a][k] = P[k][a], B[k][col = c] = P[k][c].
__global__ __launch_bounds__(256) void k_eigh_gram(const double* __restrict__ G, long L, int nb, int T, int round, int chr, int nch,
                                                   double* __restrict__ part) {
    __shared__ double s[EW * EG_LD];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    int p, q;
    eigh_pairing(T, round, blockIdx.x, &p, &q);
    const int col = t >> 2, kq = (t & 3) * 8;
    const bool live = col < EB || q < nb;                                  // the bye's columns read as zero
    const double* src = G + (live ? eigh_col(p, q, col) : 0) * L;
    d4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = (d4){0.0, 0.0, 0.0, 0.0};
    const long kb = (long)blockIdx.y * chr, ke = kb + chr < L ? kb + chr : L;    // chr and L are multiples of EG_KS
    for (long k0 = kb; k0 < ke; k0 += EG_KS) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 8; ++i) s[col * EG_LD + kq + i] = live ? src[k0 + kq + i] : 0.0;
        __syncthreads();
#pragma unroll
        for (int ss = 0; ss < EG_KS / 4; ++ss) {
            const int ks = (lane >> 4) + 4 * ss;
            const double a = s[(16 * w + (lane & 15)) * EG_LD + ks];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = mfma_f64(a, s[(16 * j + (lane & 15)) * EG_LD + ks], acc[j]);
        }
    }
    double* out = part + ((long)blockIdx.x * nch + blockIdx.y) * EWW;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) out[(16 * w + (lane >> 4) + 4 * r) * EW + 16 * j + (lane & 15)] = acc[j][r];
}

// The subproblem of pair blockIdx.x: W (sum of the partial Grams, chunks ascending) is diagonalised in LDS, J = the product of the
// rotations.  One step rotates the 32 disjoint index pairs of one round of the circle tournament on 64 indices: 32 threads
// compute (cs, sn), then every thread updates its share of the columns of W and J, then of the rows of W.  With
// R = [[cs, sn], [-sn, cs]] on (i, j): W <- R^T W R, J <- J R, t = tan from zeta = (w_jj - w_ii) / (2 w_ij), the smaller root.
// pair_rot: some rotation was applied or a column moved (otherwise J = I and the apply kernel has nothing to do).
__global__ __launch_bounds__(256) void k_eigh_sub(const double* __restrict__ part, int nch, const double* __restrict__ tiny2p,
                                                  double tol_conv, double* __restrict__ Jout, int* __restrict__ pair_rot,
                                                  int* __restrict__ sweep_flag) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    double *W = smem, *J = W + EW * ELD, *rc = J + EW * ELD, *rs = rc + EB;
    int *ri = (int*)(rs + EB), *rj = ri + EB, *fl = rj + EB;              // fl: 0 inner sweep rotated, 1 anything rotated, 2 the sweep's flag
    const int t = threadIdx.x;
    const double* src = part + (long)blockIdx.x * nch * EWW;
    for (int e = t; e < EWW; e += 256) {
        double sum = 0.0;
        for (int ch = 0; ch < nch; ++ch) sum += src[(long)ch * EWW + e];
        W[(e >> 6) * ELD + (e & 63)] = sum;
        J[(e >> 6) * ELD + (e & 63)] = (e >> 6) == (e & 63) ? 1.0 : 0.0;
    }
    if (t < 3) fl[t] = 0;
    const double tiny2 = tiny2p[0], conv_lim = tol_conv * sqrt(tiny2p[1]), tol_in = EW * DBL_EPSILON;
    __syncthreads();
    for (int isw = 0; isw < EIGH_INNER; ++isw) {
        for (int step = 0; step < EW - 1; ++step) {
            if (t < EB) {
                int i, j;
                eigh_pairing(EW, step, t, &i, &j);
                const double aa = W[i * ELD + i], bb = W[j * ELD + j], cc = W[i * ELD + j];
                double cs = 1.0, sn = 0.0;
                if (aa > tiny2 && bb > tiny2) {
                    const double lim = sqrt(aa * bb);
                    if (!(fabs(cc) <= DBL_EPSILON * lim)) {
                        const double zeta = (bb - aa) / (2.0 * cc);
                        const double tt = fabs(zeta) > 1e150 ? 0.5 / zeta : copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                        cs = 1.0 / sqrt(1.0 + tt * tt);
                        sn = cs * tt;
                        fl[1] = 1;
                        if (fabs(cc) > tol_in * lim) fl[0] = 1;
                        if (fabs(cc) > conv_lim * (sqrt(aa) + sqrt(bb))) fl[2] = 1;
                    }
                }
                ri[t] = i;
                rj[t] = j;
                rc[t] = cs;
                rs[t] = sn;
            }
            __syncthreads();
            for (int idx = t; idx < EB * EW; idx += 256) {                 // columns i, j of W and J; (idx >> 6) is one per wave
                const int pr = idx >> 6, r = idx & 63;
                const double sn = rs[pr];
                if (sn != 0.0) {
                    const double cs = rc[pr];
                    const int i = ri[pr], j = rj[pr];
                    double x = W[r * ELD + i], y = W[r * ELD + j];
                    W[r * ELD + i] = cs * x - sn * y;
                    W[r * ELD + j] = sn * x + cs * y;
                    x = J[r * ELD + i], y = J[r * ELD + j];
                    J[r * ELD + i] = cs * x - sn * y;
                    J[r * ELD + j] = sn * x + cs * y;
                }
            }
            __syncthreads();
            for (int idx = t; idx < EB * EW; idx += 256) {                 // rows i, j of W; w_ij = w_ji = 0 exactly
                const int pr = idx >> 6, c = idx & 63;
                const double sn = rs[pr];
                if (sn != 0.0) {
                    const double cs = rc[pr];
                    const int i = ri[pr], j = rj[pr];
                    const double x = W[i * ELD + c], y = W[j * ELD + c];
                    W[i * ELD + c] = c == j ? 0.0 : cs * x - sn * y;
                    W[j * ELD + c] = c == i ? 0.0 : sn * x + cs * y;
                }
            }
            __syncthreads();
        }
        const int again = fl[0];
        __syncthreads();
        if (t == 0) fl[0] = 0;
        __syncthreads();
        if (!again) break;                                                 // the same for every thread
    }
    // The pair's columns leave in descending order of their new squared norms (the diagonal of W), ties in place: block Jacobi
    // on G = A needs the large columns to travel to one end.  Without the order the residual of a smooth RBF matrix fell 2.5-fold
    // a sweep, with it 15-fold and then quadratically.  The zero columns of the padding and of the bye have the highest indices
    // of a pair and squared norm 0, no column has less: they keep their places.  rc..rs holds the norms, ri..rj the new places.
    if (t < EW) rc[t] = fmax(W[t * ELD + t], 0.0);
    __syncthreads();
    if (t < EW) {
        const double d = rc[t];
        int cnt = 0;
        for (int k = 0; k < EW; ++k) cnt += (rc[k] > d || (rc[k] == d && k < t)) ? 1 : 0;
        ri[t] = cnt;                                                       // < EW whatever W holds
        if (cnt != t) fl[1] = 1;
    }
    // One Newton-Schulz step, J <- J (3 I - J^T J) / 2, takes the rounding of the several hundred rotations behind every column
    // of J (measured: |J^T J - I| near 100 eps) down to that of one product.  Without it that error, compounded over every round
    // of every sweep, is what V's orthogonality and the residual end up with.  W's buffer takes S = J^T J.
    for (int e = t; e < EWW; e += 256) {
        const int a = e >> 6, c = e & 63;
        double sum = 0.0;
        for (int r = 0; r < EW; ++r) sum += J[r * ELD + a] * J[r * ELD + c];
        W[a * ELD + c] = sum;
    }
    __syncthreads();
    double* out = Jout + (long)blockIdx.x * EWW;
    for (int e = t; e < EWW; e += 256) {
        const int r = e >> 6, c = e & 63;
        double sum = 0.0;
        for (int k = 0; k < EW; ++k) sum += J[r * ELD + k] * ((k == c ? 1.5 : 0.0) - 0.5 * W[k * ELD + c]);
        out[r * EW + ri[c]] = sum;
    }
    if (t == 0) {
        pair_rot[blockIdx.x] = fl[1];
        if (fl[2]) *sweep_flag = 1;                                        // every writer writes 1
    }
}

// X <- X J on the 64 columns of pair blockIdx.x, rows blockIdx.y * EA_ROWS .. + EA_ROWS - 1, for X = G then X = V.  Computed
// transposed so that loads and stores walk down columns: D[row = c][col = r] = sum_k J[k][c] X[r][k]; the MFMA's A operand is J^T
// (64 doubles per lane, loaded once), its B operand 16 rows of the panel.  A wave reads its 16 rows of all 64 columns before it
// writes any of them, and no other wave touches those rows.
__global__ __launch_bounds__(256) void k_eigh_apply(double* __restrict__ G, double* __restrict__ V, long L, int nb, int T, int round,
                                                    const double* __restrict__ Jw, const int* __restrict__ pair_rot) {
    if (!pair_rot[blockIdx.x]) return;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int p, q;
    eigh_pairing(T, round, blockIdx.x, &p, &q);
    const bool hasq = q < nb;
    const double* Jp = Jw + (long)blockIdx.x * EWW;
    double ja[4][16];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int s = 0; s < 16; ++s) ja[j][s] = Jp[(4 * s + (lane >> 4)) * EW + 16 * j + (lane & 15)];
    for (int m = 0; m < 2; ++m) {
        double* X = m ? V : G;
        for (int it = 0; it < EA_ROWS / 64; ++it) {
            const long r0 = (long)blockIdx.y * EA_ROWS + 16 * (w + 4 * it);    // L is a multiple of 32: a tile of 16 rows is whole
            if (r0 >= L) break;
            double x[16];
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const int k = 4 * s + (lane >> 4);
                x[s] = (k < EB || hasq) ? X[eigh_col(p, q, k) * L + r0 + (lane & 15)] : 0.0;
            }
            d4 acc[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int s = 0; s < 16; ++s)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = mfma_f64(ja[j][s], x[s], acc[j]);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int c = 16 * j + (lane >> 4) + 4 * r;
                    if (c < EB || hasq) X[eigh_col(p, q, c) * L + r0 + (lane & 15)] = acc[j][r];
                }
        }
    }
}

// rank[j] = the place of lambda_j in ascending order (ties by column), w[rank[j]] = lambda_j
__global__ __launch_bounds__(256) void k_eigh_rank(const double* __restrict__ lam, long n, int* __restrict__ rank, double* __restrict__ w) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const double lj = lam[j];
    int cnt = 0;
    for (long i = 0; i < n; ++i) {
        const double li = lam[i];
        cnt += (li < lj || (li == lj && i < j)) ? 1 : 0;
    }
    rank[j] = cnt;                                                         // < n whatever lam holds
    w[cnt] = lj;
}

// Vout[i][rank[j]] = V[i][j]: the column-major work matrix to the row-major result, a 32 x 32 tile through LDS
__global__ __launch_bounds__(256) void k_eigh_emit(const double* __restrict__ V, long L, long n, const int* __restrict__ rank,
                                                   double* __restrict__ Vout, long ldv) {
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const long j0 = (long)blockIdx.x * 32, i0 = (long)blockIdx.y * 32;
#pragma unroll
    for (int k = 0; k < 4; ++k) tile[ty + 8 * k][tx] = V[(j0 + ty + 8 * k) * L + i0 + tx];     // j0 + 31 < L, i0 + 31 < L
    __syncthreads();
    const long j = j0 + tx;
    if (j >= n) return;
    const long rj = rank[j];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long i = i0 + ty + 8 * k;
        if (i < n) Vout[i * ldv + rj] = tile[tx][ty + 8 * k];
    }
}

int eigh_ws_alloc(EighWs* ws, long n) {
    ARG_CHECK(n >= 1 && n <= MI355GP_EIGH_MAX_N, "eigh: n must be 1 .. 16384");
    const long L = round_up(n, EB);
    ws->n = n;
    ws->L = L;
    ws->nb = (int)(L / EB);
    ws->T = ws->nb + (ws->nb & 1);
    const long chr = round_up((L + 15) / 16, EG_KS);                       // at most 16 chunks of at least 256 rows
    ws->chr = (int)(chr < 256 ? 256 : chr);
    ws->nch = (int)((L + ws->chr - 1) / ws->chr);
    const long npairs = ws->T / 2;
    HIP_CHECK(ws->G.alloc((size_t)L * L));
    HIP_CHECK(ws->V.alloc((size_t)L * L));
    HIP_CHECK(ws->part.alloc((size_t)npairs * ws->nch * EWW));
    HIP_CHECK(ws->J.alloc((size_t)npairs * EWW));
    HIP_CHECK(ws->norm2.alloc(L));
    HIP_CHECK(ws->lam.alloc(L));
    HIP_CHECK(ws->tiny2.alloc(2));
    HIP_CHECK(ws->pair_rot.alloc(npairs));
    HIP_CHECK(ws->flags.alloc(EIGH_NFLAGS));
    HIP_CHECK(ws->rank.alloc(L));
    return 0;
}

int eigh_device(hipStream_t st, const double* A, long lda, long n, double* w, double* V, long ldv, EighWs* ws, int* sweeps) {
    ARG_CHECK(ws && ws->n == n && A && w && V && lda >= n && ldv >= n, "eigh_device: bad arguments or a workspace of another n");
    // k_eigh_sub takes 65.8 KiB of dynamic LDS; the opt-in belongs to the current device, so it is made on every call
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_eigh_sub), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  ES_LDS_BYTES));
    const long L = ws->L;
    const int npairs = ws->T / 2, nrc = (int)((L + EA_ROWS - 1) / EA_ROWS);
    const double tol_conv = (double)(L + EW) * DBL_EPSILON;
    hipLaunchKernelGGL(k_eigh_init, dim3((unsigned)((L * L + 255) / 256)), dim3(256), 0, st, A, lda, n, L, (double*)ws->G,
                       (double*)ws->V, (int*)ws->flags);
    int done = 0, converged = 0;
    while (done < MI355GP_EIGH_MAX_SWEEPS && !converged) {
        hipLaunchKernelGGL(k_eigh_coldot, dim3((unsigned)(L / 4)), dim3(256), 0, st, (const double*)ws->G, (const double*)ws->G, L,
                           (double*)ws->norm2);
        hipLaunchKernelGGL(k_eigh_tiny, dim3(1), dim3(256), 0, st, (const double*)ws->norm2, L, (double*)ws->tiny2);
        for (int r = 0; r < ws->T - 1; ++r) {
            hipLaunchKernelGGL(k_eigh_gram, dim3(npairs, ws->nch), dim3(256), 0, st, (const double*)ws->G, L, ws->nb, ws->T, r, ws->chr,
                               ws->nch, (double*)ws->part);
            hipLaunchKernelGGL(k_eigh_sub, dim3(npairs), dim3(256), ES_LDS_BYTES, st, (const double*)ws->part, ws->nch,
                               (const double*)ws->tiny2, tol_conv, (double*)ws->J, (int*)ws->pair_rot, (int*)ws->flags + done);
            hipLaunchKernelGGL(k_eigh_apply, dim3(npairs, nrc), dim3(256), 0, st, (double*)ws->G, (double*)ws->V, L, ws->nb, ws->T, r,
                               (const double*)ws->J, (const int*)ws->pair_rot);
        }
        HIP_CHECK(hipGetLastError());
        int flag = 0;
        HIP_CHECK(hipMemcpyAsync(&flag, (int*)ws->flags + done, sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        ++done;
        converged = !flag;
    }
    hipLaunchKernelGGL(k_eigh_coldot, dim3((unsigned)(L / 4)), dim3(256), 0, st, (const double*)ws->V, (const double*)ws->G, L,
                       (double*)ws->lam);
    hipLaunchKernelGGL(k_eigh_rank, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const double*)ws->lam, n, (int*)ws->rank, w);
    hipLaunchKernelGGL(k_eigh_emit, dim3((unsigned)(L / 32), (unsigned)(L / 32)), dim3(256), 0, st, (const double*)ws->V, L, n,
                       (const int*)ws->rank, V, ldv);
    HIP_CHECK(hipGetLastError());
    if (sweeps) *sweeps = done;
    return converged ? 0 : 1;
}

extern "C" int mi355gp_eigh(int device, const double* A, int64_t n, double* w, double* V, int* sweeps, double* ms) {
    ARG_CHECK(A && w && V && n >= 1 && n <= MI355GP_EIGH_MAX_N, "mi355gp_eigh: A, w, V and n in 1 .. 16384");
    HIP_CHECK(hipSetDevice(device));
    DevBuf dA, dw, dV;                                                     // released on every return path
    EighWs ws;
    if (int rc = eigh_ws_alloc(&ws, n)) return rc;
    HIP_CHECK(dA.alloc((size_t)n * n));
    HIP_CHECK(dw.alloc(n));
    HIP_CHECK(dV.alloc((size_t)n * n));
    struct Events {
        hipEvent_t e[2] = {nullptr, nullptr};
        ~Events() {
            for (hipEvent_t ev : e)
                if (ev) (void)hipEventDestroy(ev);
        }
    } ev;
    HIP_CHECK(hipEventCreate(&ev.e[0]));
    HIP_CHECK(hipEventCreate(&ev.e[1]));
    HIP_CHECK(hipMemcpy(dA, A, sizeof(double) * n * n, hipMemcpyHostToDevice));
    HIP_CHECK(hipEventRecord(ev.e[0], 0));
    const int info = eigh_device(0, dA, n, n, dw, dV, n, &ws, sweeps);
    if (info < 0) return info;
    HIP_CHECK(hipEventRecord(ev.e[1], 0));
    HIP_CHECK(hipMemcpy(w, dw, sizeof(double) * n, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(V, dV, sizeof(double) * n * n, hipMemcpyDeviceToHost));
    if (ms) {
        float t;
        HIP_CHECK(hipEventElapsedTime(&t, ev.e[0], ev.e[1]));
        *ms = t;
    }
    return info;
}
