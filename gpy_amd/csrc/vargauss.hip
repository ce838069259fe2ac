// vargauss.hip -- the variational Gaussian approximation (C-ABI mi355gp_vargauss_*, include/mi355gp_vargauss.h) inside the
// Laplace session of an exact context: everything N x N of GPy/inference/latent_function_inference/var_gauss.py:34-65 stays in
// HBM; the likelihood's variational expectations are O(N) host work between forward and backward.
//
// beta takes the place of W^1/2 in the session (LV_SW, signed): A = I + diag(beta) K diag(beta) is the B of laplace.hip, so the
// factorisation, diag Sigma, prediction and the woodbury_inv = beta Ai beta are the session's own.  Buffers of one evaluation
// (the session's five N x N: K, A, B, C, Mbuf; DESIGN.md "VarGauss"):
//   forward   A: diag(beta) K, scratch        B: X = L_A^-1         C: Ai = X^T X (lower tiles)
//   backward  C: Ai mirrored to both triangles -> A: P1 = Ai Ai -> A: the Ai / P1 part of dL_dK in place + the beta partials
//             -> C: diag(beta^-1) Ai in place -> Mbuf: P2 = Ai diag(beta^-2) Ai -> A: dL_dK, both triangles
// (mi355gp_vargauss_backward_exact: C keeps Ai; Mbuf: one row-scaled copy of Ai per sign of dF_dv, its Gram accumulated onto A)
// X survives, so prediction gives the same bytes before and after backward; Ai comes back by one lauum on fetch.
// Both Gram products run on full tiles (launch_gemm_tn_sq): 2 x 2 N^3 flops, of which only the lower tiles are read.
#include <cmath>
#include <cstring>

#include "../../include/mi355gp_vargauss.h"
#include "lap_session.h"

#define VG_VGRID(n) dim3((unsigned)(((n) + 255) / 256)), dim3(256)

#define KT 64      // edge of the tiles of the resident K and of every N x N buffer of the session (the covariance tile, kern_tile.h)

// ------------------------------------------------------------------------------------------------
// Variational Gaussian approximation (GPy/inference/latent_function_inference/var_gauss.py): the passes of one backward over
// Ai = (I + diag(beta) K diag(beta))^-1, P1 = Ai Ai, P2 = Ai diag(beta^-2) Ai and the resident K.  Written like k_laplace_dLdK:
// one block per lower 64-tile, 32-byte loads, the mirror written from LDS.
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

static int vg_check_beta(const double* beta, long n) {
    for (long i = 0; i < n; ++i)
        if (!std::isfinite(beta[i]) || beta[i] == 0.0) {
            mi355gp_set_error("mi355gp_vargauss_forward: beta[%ld] = %g is not a finite non-zero number (the gradients divide by beta)",
                              i, beta[i]);
            return -1;
        }
    return 0;
}

// Both backward calls.  exact: the dF_dv term of dL_dK is T diag(dF_dv) T^T = beta beta^T o Ai diag(dF_dv / beta^2) Ai, the derivative
// of the bound (d var_i / dK = T[:, i] T[:, i]^T); otherwise the reference's (T o dF_dv) T^T (var_gauss.py:65, rows scaled), symmetrised.
// The exact product is not a Gram matrix when dF_dv changes sign, so it is taken as one Gram per sign of dF_dv, R = diag(sqrt(max(+-dF_dv,
// 0)) / |beta|) Ai built in Mbuf and R^T R accumulated with its sign onto A = H / (beta beta^T); Ai in C stays whole.
static int vg_backward(mi355gp_ctx* c, const double* dF_dm, const double* dF_dv, double* dalpha_out, double* dbeta_out,
                       double* dtheta_out, bool exact, const char* where) {
    if (!(c && c->n > 0 && c->lap && c->lap_stage >= 3 && c->lap->vg && !c->lap->vg_bwd)) {
        mi355gp_set_error("%s: call mi355gp_vargauss_forward first (one backward per forward)", where);
        return -1;
    }
    if (!(dF_dm && dF_dv && dalpha_out && dbeta_out && dtheta_out)) {
        mi355gp_set_error("%s: NULL argument", where);
        return -1;
    }
    const long n = c->n, np = c->npad;
    if (int rc = lap_check_vec(dF_dm, n, where, "dF_dm")) return rc;
    if (int rc = lap_check_vec(dF_dv, n, where, "dF_dv")) return rc;
    HIP_CHECK(hipSetDevice(c->device));
    EngineShared gate(c->device);
    LaplaceSession* L = c->lap;
    hipStream_t st = c->st;
    if (!c->Mbuf) HIP_CHECK(hipMalloc(&c->Mbuf, sizeof(double) * np * np));
    const int nt = (int)(np / NB);
    L->vg_ai = exact;                                           // reference form: C is mirrored, then scaled, no longer Ai
    L->vg_bwd = true;
    HIP_CHECK(hipMemcpyAsync(lvec(c, LV_S), dF_dm, sizeof(double) * n, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(lvec(c, LV_U), dF_dv, sizeof(double) * n, hipMemcpyHostToDevice, st));
    launch_symv_lower(st, L->K, np, n, lvec(c, LV_S), nullptr, lvec(c, LV_T0), nullptr, L->part);       // K dF_dm
    launch_vg_mirror(st, c->C, np);
    launch_gemm_tn_sq(st, c->C, np, np, c->A, np, nt, 1.0, 0.0);                                         // P1 = Ai Ai
    launch_vg_assemble(st, c->C, L->K, np, n, lvec(c, LV_SW), lvec(c, LV_A), lvec(c, LV_S), lvec(c, LV_U), lvec(c, LV_DIAG), exact ? 1 : 0,
                       c->A, L->vgPart);
    launch_vg_finish_vec(st, L->vgPart, np, n, lvec(c, LV_SW), lvec(c, LV_T0), lvec(c, LV_KA), lvec(c, LV_T1), lvec(c, LV_T2));
    if (!exact) {
        launch_rowscale(st, c->C, np, n, np, lvec(c, LV_SW), 1, c->C);                                   // diag(beta^-1) Ai
        launch_gemm_tn_sq(st, c->C, np, np, c->Mbuf, np, nt, 1.0, 0.0);                                  // P2 = Ai diag(beta^-2) Ai
        launch_vg_dLdK(st, c->Mbuf, np, n, lvec(c, LV_SW), lvec(c, LV_U), 0, c->A);
    } else {
        bool pos = false, neg = false;
        for (long i = 0; i < n; ++i) {
            pos = pos || dF_dv[i] > 0.0;
            neg = neg || dF_dv[i] < 0.0;
        }
        for (int sgn = 0; sgn < 2; ++sgn) {
            if (!(sgn == 0 ? neg : pos)) continue;
            const double sign = sgn == 0 ? -1.0 : 1.0;
            launch_vg_rowscale_v(st, c->C, np, n, np, np, lvec(c, LV_U), lvec(c, LV_SW), sign, c->Mbuf);
            launch_gemm_tn_sq(st, c->Mbuf, np, np, c->A, np, nt, sign, 1.0);
        }
        launch_vg_dLdK(st, nullptr, np, n, lvec(c, LV_SW), lvec(c, LV_U), 1, c->A);
    }
    c->lap_stage = 4;
    L->host.resize((size_t)2 * np + 8);
    HIP_CHECK(hipMemcpyAsync(L->host.data(), lvec(c, LV_T1), sizeof(double) * n, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(L->host.data() + np, lvec(c, LV_T2), sizeof(double) * n, hipMemcpyDeviceToHost, st));
    if (int rc = lap_reduce_dtheta(c, dtheta_out)) return rc;
    memcpy(dalpha_out, L->host.data(), sizeof(double) * n);
    memcpy(dbeta_out, L->host.data() + np, sizeof(double) * n);
    return 0;
}

extern "C" {

int mi355gp_vargauss_forward(mi355gp_ctx* c, const double* alpha, const double* beta, double extra_jitter, double* m_out,
                             double* var_out, double* scal_out) {
    ARG_CHECK(c && c->n > 0 && c->lap && c->lap_stage >= 1, "mi355gp_vargauss_forward: call mi355gp_laplace_begin first");
    ARG_CHECK(alpha && beta && m_out && var_out && scal_out, "mi355gp_vargauss_forward: NULL argument");
    const long n = c->n, np = c->npad;
    if (int rc = lap_check_vec(alpha, n, "mi355gp_vargauss_forward", "alpha")) return rc;
    if (int rc = vg_check_beta(beta, n)) return rc;
    HIP_CHECK(hipSetDevice(c->device));
    EngineShared gate(c->device);
    LaplaceSession* L = c->lap;
    hipStream_t st = c->st;
    c->lap_stage = 1;
    L->vg = L->vg_ai = L->vg_bwd = false;
    if (!L->vgPart) HIP_CHECK(hipMalloc(&L->vgPart, sizeof(double) * vg_part_doubles(np)));
    HIP_CHECK(hipMemcpyAsync(lvec(c, LV_A), alpha, sizeof(double) * n, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(lvec(c, LV_SW), beta, sizeof(double) * n, hipMemcpyHostToDevice, st));
    L->host.resize((size_t)2 * np + 8);
    const int nt = (int)(np / NB);
    int info = 0;
    for (int attempt = 0;; ++attempt) {
        lap_enqueue_factor_sw(c, extra_jitter);
        // diag Sigma = Kdiag - colsumsq(X (beta K)), the diag(Ki_W_i) of mi355gp_laplace_finish for W = beta^2; then C = Ai = X^T X
        launch_rowscale(st, L->K, np, n, np, lvec(c, LV_SW), 0, c->A);
        launch_trmm_lower(st, c->B, np, c->A, np, c->C, np, nt, nt);
        launch_col_reduce_vec(st, c->C, np, n, n, lvec(c, LV_KD), lvec(c, LV_DIAG));
        lauum_device(st, c->B, c->C, np, &L->ws);
        // m = K alpha; [0] = m^T alpha, [2] = tr Ai, [3] = log det A, [6] = info, each summed in a fixed order
        launch_symv_lower(st, L->K, np, n, lvec(c, LV_A), nullptr, lvec(c, LV_KA), nullptr, L->part);
        launch_scalars(st, lvec(c, LV_A), lvec(c, LV_KA), c->C, np, n, 1, L->ws.logsum, L->ws.nblk, lscal(c), nullptr, L->ws.info);
        HIP_CHECK(hipMemcpyAsync(L->host.data(), lvec(c, LV_KA), sizeof(double) * n, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(L->host.data() + np, lvec(c, LV_DIAG), sizeof(double) * n, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(L->host.data() + 2 * np, lscal(c), sizeof(double) * 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        HIP_CHECK(hipGetLastError());
        const int rc = lap_factor_outcome(c, (int)L->host[(size_t)2 * np + 6], attempt, &info);
        if (rc < 0) return rc;
        if (rc == 0) break;
    }
    if (info > 0) return info;
    memcpy(m_out, L->host.data(), sizeof(double) * n);
    memcpy(var_out, L->host.data() + np, sizeof(double) * n);
    scal_out[0] = L->host[(size_t)2 * np + 3];
    scal_out[1] = L->host[(size_t)2 * np + 2];
    scal_out[2] = L->host[(size_t)2 * np + 0];
    L->vg = L->vg_ai = true;
    c->lap_stage = 3;
    return 0;
}

int mi355gp_vargauss_backward(mi355gp_ctx* c, const double* dF_dm, const double* dF_dv, double* dalpha_out, double* dbeta_out,
                              double* dtheta_out) {
    return vg_backward(c, dF_dm, dF_dv, dalpha_out, dbeta_out, dtheta_out, /*exact=*/false, "mi355gp_vargauss_backward");
}

int mi355gp_vargauss_backward_exact(mi355gp_ctx* c, const double* dF_dm, const double* dF_dv, double* dalpha_out, double* dbeta_out,
                                    double* dtheta_out) {
    return vg_backward(c, dF_dm, dF_dv, dalpha_out, dbeta_out, dtheta_out, /*exact=*/true, "mi355gp_vargauss_backward_exact");
}

}  // extern "C"
