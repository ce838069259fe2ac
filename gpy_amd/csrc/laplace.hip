// laplace.hip -- the Laplace approximation for a non-Gaussian likelihood on an exact context (C-ABI mi355gp_laplace_*,
// include/mi355gp.h): everything N x N of GPy/inference/latent_function_inference/laplace.py:122-353 stays in HBM.  The
// likelihood's derivatives (W, b, dL_dfhat) are O(N) host work and arrive as vectors; nothing N x N crosses PCIe.
//
// Buffers of one session: K = kern.K(X) in a FOURTH npad x npad buffer (allocated by the first mi355gp_laplace_begin of a
// context), the context's A (B = I + W^1/2 K W^1/2, then its Cholesky factor, after the mode the dL_dK), B (X = L_B^-1) and
// C (scratch of the inverse, then B^-1).  The session factors through a FactorWs of its own, so the schedule calibration and
// the captured graph of the context's Gaussian path never see it.
#include <cmath>
#include <cstring>
#include <vector>

#include "lap_session.h"

void laplace_session_free(LaplaceSession* s) {
    if (!s) return;
    double** ptrs[] = {&s->K, &s->vec, &s->part, &s->coregPart, &s->vgPart};
    for (auto p : ptrs)
        if (*p) (void)hipFree(*p);
    if (s->ws_ok) factor_ws_free(&s->ws);
    delete s;
}

#define KT 64      // edge of the tiles of the resident K and of every N x N buffer of the session (the covariance tile, kern_tile.h)

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

// elementwise helpers on N-vectors (grid: ceil(n / 256) blocks of 256)
__global__ void k_lap_sqrt(const double* __restrict__ w, long n, double* __restrict__ sw) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) sw[i] = sqrt(w[i]);
}
// out = x - sw * t       (a = b - W^1/2 B^-1 (W^1/2 K b), laplace.py:195-198; u likewise from dL_dfhat)
__global__ void k_lap_sub_scaled(const double* __restrict__ x, const double* __restrict__ sw, const double* __restrict__ t, long n,
                                 double* __restrict__ out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = x[i] - sw[i] * t[i];
}
__global__ void k_lap_mul(const double* __restrict__ x, const double* __restrict__ y, long n, double* __restrict__ out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = x[i] * y[i];
}
__global__ void k_lap_diag(const double* __restrict__ K, long ld, long n, double* __restrict__ kd) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) kd[i] = K[i * ld + i];
}
// M[i][j] *= G[i][j] over n x n (ld shared): dL_dK times the other factors of a product term (prod.py:86-99)
__global__ void k_lap_mm_mul(double* __restrict__ M, const double* __restrict__ G, long ld, long n) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j < n) M[i * ld + j] *= G[i * ld + j];
}
// out[i][j] = sw_max A_(max, min) sw_min: K_Wi_i = W^1/2 B^-1 W^1/2 (laplace.py:338) from the lower tiles of B^-1.  The two
// products are taken in the order of the lower triangle on both sides of the diagonal (the order k_laplace_dLdK uses), so that
// (i, j) and (j, i) are the same number: (sw_i A) sw_j and (sw_j A) sw_i differ in the last bit
__global__ void k_lap_extract_kwi(const double* __restrict__ A, long ld, long n, const double* __restrict__ sw,
                                  double* __restrict__ out) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= n) return;
    const long hi = i > j ? i : j, lo = i > j ? j : i;
    out[i * n + j] = sw[hi] * A[hi * ld + lo] * sw[lo];
}
__global__ void k_lap_extract_full(const double* __restrict__ A, long ld, long n, double* __restrict__ out) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j < n) out[i * n + j] = A[i * ld + j];
}
#define VGRID(n) dim3((unsigned)(((n) + 255) / 256)), dim3(256)
#define MGRID(n) dim3((unsigned)(((n) + 255) / 256), (unsigned)(n)), dim3(256)

int lap_check_W(const double* W, long n, const char* where) {
    for (long i = 0; i < n; ++i) {
        if (std::isnan(W[i])) {
            mi355gp_set_error("%s: One or more element(s) of W is NaN (element %ld)", where, i);
            return -1;
        }
        if (!(W[i] >= 0.0) || std::isinf(W[i])) {
            mi355gp_set_error("%s: W[%ld] = %g is not a finite non-negative number (W^1/2 is taken)", where, i, W[i]);
            return -1;
        }
    }
    return 0;
}
int lap_check_vec(const double* v, long n, const char* where, const char* name) {
    for (long i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) {
            mi355gp_set_error("%s: %s[%ld] = %g is not finite", where, name, i, v[i]);
            return -1;
        }
    return 0;
}

// W (device, LV_W) -> sw, B into A, L_B in place, X = L_B^-1 into the context's B buffer; all enqueued, nothing read back
void lap_enqueue_factor(mi355gp_ctx* c, double jit) {
    LaplaceSession* L = c->lap;
    L->vg = L->vg_ai = L->vg_bwd = false;                    // sw is W^1/2 again: nothing of a VarGauss evaluation is left
    hipLaunchKernelGGL(k_lap_sqrt, VGRID(c->n), 0, c->st, lvec(c, LV_W), c->n, lvec(c, LV_SW));
    lap_enqueue_factor_sw(c, jit);
}
void lap_enqueue_factor_sw(mi355gp_ctx* c, double jit) {
    LaplaceSession* L = c->lap;
    L->ep_sigma = false;                                     // A is overwritten: a resident EP Sigma is gone
    hipStream_t st = c->st;
    const long n = c->n, np = c->npad;
    launch_laplace_B(st, L->K, np, n, lvec(c, LV_SW), jit, c->A);
    L->ws.scratchX = c->B;                                   // free until trtri overwrites them
    L->ws.scratchT = c->C;
    potrf_device(st, c->A, np, &L->ws);
    trtri_device(st, c->A, c->B, c->C, np, &L->ws);
}
// t = B^-1 r = X^T (X r)
void lap_enqueue_Binv(mi355gp_ctx* c, const double* r, double* t) {
    launch_tri_matvec(c->st, c->B, c->npad, c->n, r, 1, c->dTmp, t, c->dTrmvPart);
}
// LV_U = u = (I - K_Wi_i K) LV_S = s - W^1/2 B^-1 (W^1/2 K s) for the W of the last finish (LV_SW, X in the context's B buffer)
static void lap_enqueue_u(mi355gp_ctx* c) {
    LaplaceSession* L = c->lap;
    hipStream_t st = c->st;
    const long n = c->n, np = c->npad;
    launch_symv_lower(st, L->K, np, n, lvec(c, LV_S), nullptr, lvec(c, LV_T0), nullptr, L->part);
    hipLaunchKernelGGL(k_lap_mul, VGRID(n), 0, st, lvec(c, LV_SW), lvec(c, LV_T0), n, lvec(c, LV_T1));
    lap_enqueue_Binv(c, lvec(c, LV_T1), lvec(c, LV_T2));
    hipLaunchKernelGGL(k_lap_sub_scaled, VGRID(n), 0, st, lvec(c, LV_S), lvec(c, LV_SW), lvec(c, LV_T2), n, lvec(c, LV_U));
}
// after the stream has drained: info of the factorisation (from the scalar block).  Returns 1 = redo (persistent launch called
// off), 0 = go on (*info_out: LAPACK info), < 0 error
int lap_factor_outcome(mi355gp_ctx* c, int info, int attempt, int* info_out) {
    bool clean = false;
    if (potrf_persist_aborted(info, &c->lap->ws, &clean)) {
        if (attempt == 0) return 1;                          // B is rebuilt from the resident K either way
        mi355gp_set_error("the persistent factorisation of the Laplace B matrix aborted twice (info %d)", info);
        return -6;
    }
    if (info > c->n) info = (int)c->n;
    *info_out = info;
    return 0;
}

// every part reduces the dL_dK in the context's A against its own dK/dtheta (the unfused reductions of mi355gp_update_gradients_full)
int lap_reduce_dtheta(mi355gp_ctx* c, double* dtheta_out) {
    LaplaceSession* L = c->lap;
    hipStream_t st = c->st;
    const long n = c->n, np = c->npad;
    const int groups = (c->D + 31) / 32;
    const size_t nparts = c->parts.size();
    HIP_CHECK(hipMemsetAsync(c->dGradOutAll, 0, sizeof(double) * nparts * groups * GP_STRIDE, st));
    HIP_CHECK(hipMemsetAsync(c->dPack + c->offExt, 0, sizeof(double) * nparts * groups * GP_STRIDE, st));
    const int nb = grad_generic_num_blocks(n, n);
    bool coreg = false;
    for (size_t p = 0; p < nparts; ++p) {
        const mi355gp_ctx::Part& pt = c->parts[p];
        // factor of a product: dL_dK times the covariances of the term's other factors (prod.py:86-99), materialised in Mbuf
        const bool prod = emit_other_factors(c->terms, pt.tix, p, c->Mbuf, [&](int g, double* dst, const double* mul, int, bool) {
            launch_kbuild_sym(st, c->parts[(size_t)g].kp, c->parts[(size_t)g].dXt, np, n, np, dst, nullptr, 0, 0.0, /*lower_only=*/0,
                              /*add_diag=*/0, /*accumulate=*/0, mul);
        });
        if (prod) hipLaunchKernelGGL(k_lap_mm_mul, MGRID(n), 0, st, c->Mbuf, c->A, np, n);
        const double* G = prod ? c->Mbuf : c->A;
        if (pt.coreg()) {
            coreg = true;
            const int P = pt.kp.ard;
            const int nbc = launch_grad_coreg(st, false, pt.kp, pt.dXt, np, n, pt.dXt, np, n, G, np, nullptr, 0, L->coregPart);
            launch_reduce_partials(st, L->coregPart, nbc, P * P, c->dPack + c->offCoreg + p * COREG_REC);
            continue;
        }
        launch_grad_generic(st, pt.kp, pt.dXt, np, n, pt.dXt, np, n, /*symmetric=*/1, G, np, c->dGradPart);
        for (int r = 0; r < (pt.ext() ? 2 : 1); ++r)
            for (int g = 0; g < (pt.kp.ard ? groups : 1); ++g)
                launch_reduce_partials(st, c->dGradPart + ((long)r * groups + g) * nb * GP_STRIDE, nb, GP_STRIDE,
                                       (r == 0 ? c->dGradOutAll : c->dPack + c->offExt) + ((long)p * groups + g) * GP_STRIDE);
    }
    const size_t ncopy = coreg ? c->packDoubles : c->offAlpha;
    HIP_CHECK(hipMemcpyAsync(c->hPack, c->dPack, sizeof(double) * ncopy, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    double* o = dtheta_out;
    for (size_t p = 0; p < nparts; ++p) {
        const double* rec = c->parts[p].coreg() ? c->hPack + c->offCoreg + p * COREG_REC
                                                : c->hPack + c->offGrad + p * (size_t)groups * GP_STRIDE;
        o += part_dtheta(c->parts[p], rec, c->hPack + c->offExt + p * (size_t)groups * GP_STRIDE, o);
    }
    return 0;
}

extern "C" {

int mi355gp_laplace_begin(mi355gp_ctx* c, int nparts, const mi355gp_part* parts) {
    ARG_CHECK(c && c->n > 0, "mi355gp_laplace_begin: set_data first");
    if (c->Dy != 1) {
        mi355gp_set_error("mi355gp_laplace_begin: the Laplace approximation takes one output column, this context holds Dy = %d", c->Dy);
        return -1;
    }
    HIP_CHECK(hipSetDevice(c->device));
    EngineShared gate(c->device);
    if (int rc = ctx_prepare_parts(c, nparts, parts)) return rc;
    const long n = c->n, np = c->npad;
    if (!c->lap) c->lap = new LaplaceSession();
    LaplaceSession* L = c->lap;
    if (!L->K) HIP_CHECK(hipMalloc(&L->K, sizeof(double) * np * np));
    if (!L->vec) HIP_CHECK(hipMalloc(&L->vec, sizeof(double) * ((size_t)LV_NUM * np + 8)));
    if (!L->part) HIP_CHECK(hipMalloc(&L->part, sizeof(double) * symv_part_doubles(np)));
    if (!L->ws_ok) {
        if (factor_ws_alloc(&L->ws, np) != 0) return -3;
        L->ws_ok = true;
    }
    for (const auto& p : c->parts)
        if (p.coreg() && !L->coregPart) HIP_CHECK(hipMalloc(&L->coregPart, sizeof(double) * 2048 * COREG_REC));
    hipStream_t st = c->st;
    c->have_kernel = true;
    c->have_factor = false;                                   // A / B / C belong to the session from here on
    c->lap_stage = 0;
    L->ep_sigma = false;
    L->vg = L->vg_ai = L->vg_bwd = false;
    ctx_scale_parts(c);
    // K = sum_t prod_f K_f, both triangles (the prediction-style products read it whole; the mat-vecs read its lower tiles)
    emit_expression(c->terms, L->K, c->Mbuf, false, [&](int p, double* dst, const double* mul, int acc, bool) {
        launch_kbuild_sym(st, c->parts[(size_t)p].kp, c->parts[(size_t)p].dXt, np, n, np, dst, nullptr, 0, 0.0, /*lower_only=*/0,
                          /*add_diag=*/0, acc, mul);
    });
    hipLaunchKernelGGL(k_lap_diag, VGRID(n), 0, st, L->K, np, n, lvec(c, LV_KD));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    c->lap_stage = 1;
    return 0;
}

int mi355gp_laplace_newton(mi355gp_ctx* c, const double* W, const double* b, double extra_jitter, double* a_out, double* Ka_out,
                           double* logdet_out) {
    ARG_CHECK(c && c->n > 0 && c->lap && c->lap_stage >= 1, "mi355gp_laplace_newton: call mi355gp_laplace_begin first");
    ARG_CHECK(W && b && a_out && Ka_out, "mi355gp_laplace_newton: NULL argument");
    const long n = c->n, np = c->npad;
    if (int rc = lap_check_W(W, n, "mi355gp_laplace_newton")) return rc;
    if (int rc = lap_check_vec(b, n, "mi355gp_laplace_newton", "b")) return rc;
    HIP_CHECK(hipSetDevice(c->device));
    EngineShared gate(c->device);
    LaplaceSession* L = c->lap;
    hipStream_t st = c->st;
    c->lap_stage = 1;
    HIP_CHECK(hipMemcpyAsync(lvec(c, LV_W), W, sizeof(double) * n, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(lvec(c, LV_B), b, sizeof(double) * n, hipMemcpyHostToDevice, st));
    L->host.resize((size_t)2 * np + 8);
    int info = 0;
    for (int attempt = 0;; ++attempt) {
        lap_enqueue_factor(c, extra_jitter);
        // a = b - W^1/2 B^-1 (W^1/2 K b), then K a   (laplace.py:193-198; f_trial = f + s K dKi_f is linear in the step, :202-208)
        launch_symv_lower(st, L->K, np, n, lvec(c, LV_B), nullptr, lvec(c, LV_T0), nullptr, L->part);
        hipLaunchKernelGGL(k_lap_mul, VGRID(n), 0, st, lvec(c, LV_SW), lvec(c, LV_T0), n, lvec(c, LV_T1));
        lap_enqueue_Binv(c, lvec(c, LV_T1), lvec(c, LV_T2));
        hipLaunchKernelGGL(k_lap_sub_scaled, VGRID(n), 0, st, lvec(c, LV_B), lvec(c, LV_SW), lvec(c, LV_T2), n, lvec(c, LV_A));
        launch_symv_lower(st, L->K, np, n, lvec(c, LV_A), nullptr, lvec(c, LV_KA), nullptr, L->part);
        launch_scalars(st, lvec(c, LV_A), lvec(c, LV_A), nullptr, 0, n, 1, L->ws.logsum, L->ws.nblk, lscal(c), nullptr, L->ws.info);
        HIP_CHECK(hipMemcpyAsync(L->host.data(), lvec(c, LV_A), sizeof(double) * n, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(L->host.data() + np, lvec(c, LV_KA), sizeof(double) * n, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(L->host.data() + 2 * np, lscal(c), sizeof(double) * 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        HIP_CHECK(hipGetLastError());
        const int rc = lap_factor_outcome(c, (int)L->host[(size_t)2 * np + 6], attempt, &info);
        if (rc < 0) return rc;
        if (rc == 0) break;
    }
    if (info > 0) return info;
    memcpy(a_out, L->host.data(), sizeof(double) * n);
    memcpy(Ka_out, L->host.data() + np, sizeof(double) * n);
    if (logdet_out) *logdet_out = L->host[(size_t)2 * np + 3];
    c->lap_stage = 2;
    return 0;
}

int mi355gp_laplace_finish(mi355gp_ctx* c, const double* W, double extra_jitter, double* diagKiWi_out, double* logdet_out) {
    ARG_CHECK(c && c->n > 0 && c->lap && c->lap_stage >= 1, "mi355gp_laplace_finish: call mi355gp_laplace_begin first");
    ARG_CHECK(W && diagKiWi_out && logdet_out, "mi355gp_laplace_finish: NULL argument");
    const long n = c->n, np = c->npad;
    if (int rc = lap_check_W(W, n, "mi355gp_laplace_finish")) return rc;
    HIP_CHECK(hipSetDevice(c->device));
    EngineShared gate(c->device);
    LaplaceSession* L = c->lap;
    hipStream_t st = c->st;
    c->lap_stage = 1;
    HIP_CHECK(hipMemcpyAsync(lvec(c, LV_W), W, sizeof(double) * n, hipMemcpyHostToDevice, st));
    L->host.resize((size_t)2 * np + 8);
    const int nt = (int)(np / NB);
    int info = 0;
    for (int attempt = 0;; ++attempt) {
        lap_enqueue_factor(c, extra_jitter);
        // diag(Ki_W_i) = Kdiag - colsumsq(X (W^1/2 K))  (laplace.py:347-348): the scaled K goes through A (L_B is not needed
        // once X exists), the product through C; then C = B^-1 = X^T X
        launch_rowscale_sqrt(st, L->K, np, n, np, lvec(c, LV_W), c->A);
        launch_trmm_lower(st, c->B, np, c->A, np, c->C, np, nt, nt);
        launch_col_reduce_vec(st, c->C, np, n, n, lvec(c, LV_KD), lvec(c, LV_DIAG));
        lauum_device(st, c->B, c->C, np, &L->ws);
        launch_scalars(st, lvec(c, LV_DIAG), lvec(c, LV_DIAG), nullptr, 0, n, 1, L->ws.logsum, L->ws.nblk, lscal(c), nullptr,
                       L->ws.info);
        HIP_CHECK(hipMemcpyAsync(L->host.data(), lvec(c, LV_DIAG), sizeof(double) * n, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(L->host.data() + 2 * np, lscal(c), sizeof(double) * 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        HIP_CHECK(hipGetLastError());
        const int rc = lap_factor_outcome(c, (int)L->host[(size_t)2 * np + 6], attempt, &info);
        if (rc < 0) return rc;
        if (rc == 0) break;
    }
    if (info > 0) return info;
    memcpy(diagKiWi_out, L->host.data(), sizeof(double) * n);
    *logdet_out = L->host[(size_t)2 * np + 3];
    c->lap_stage = 3;
    return 0;
}

int mi355gp_laplace_gradients(mi355gp_ctx* c, const double* Ki_f, const double* dL_dfhat, double* dtheta_out) {
    ARG_CHECK(c && c->n > 0 && c->lap && c->lap_stage >= 3, "mi355gp_laplace_gradients: call mi355gp_laplace_finish first");
    ARG_CHECK(Ki_f && dL_dfhat && dtheta_out, "mi355gp_laplace_gradients: NULL argument");
    ARG_CHECK(!c->lap->vg, "mi355gp_laplace_gradients: the session holds a VarGauss evaluation, call mi355gp_laplace_finish first");
    const long n = c->n, np = c->npad;
    if (int rc = lap_check_vec(Ki_f, n, "mi355gp_laplace_gradients", "Ki_f")) return rc;
    if (int rc = lap_check_vec(dL_dfhat, n, "mi355gp_laplace_gradients", "dL_dfhat")) return rc;
    HIP_CHECK(hipSetDevice(c->device));
    EngineShared gate(c->device);
    hipStream_t st = c->st;
    HIP_CHECK(hipMemcpyAsync(lvec(c, LV_A), Ki_f, sizeof(double) * n, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(lvec(c, LV_S), dL_dfhat, sizeof(double) * n, hipMemcpyHostToDevice, st));
    // u = (I - K_Wi_i K) dL_dfhat, K_Wi_i = W^1/2 B^-1 W^1/2: the implicit part a dL_dfhat^T (I - K K_Wi_i) is a u^T (laplace.py:257-270)
    lap_enqueue_u(c);
    // dL_dK, symmetrised, into A (what finish left there is spent); C keeps B^-1 for MI355GP_FETCH_KINV and prediction keeps X
    launch_laplace_dLdK(st, c->C, np, n, lvec(c, LV_SW), lvec(c, LV_A), lvec(c, LV_U), c->A);
    c->lap_stage = 4;
    return lap_reduce_dtheta(c, dtheta_out);
}

int mi355gp_laplace_implicit(mi355gp_ctx* c, const double* dL_dfhat, double* s_out) {
    ARG_CHECK(c && c->n > 0 && c->lap && c->lap_stage >= 3, "mi355gp_laplace_implicit: call mi355gp_laplace_finish first");
    ARG_CHECK(dL_dfhat && s_out, "mi355gp_laplace_implicit: NULL argument");
    ARG_CHECK(!c->lap->vg, "mi355gp_laplace_implicit: the session holds a VarGauss evaluation, call mi355gp_laplace_finish first");
    const long n = c->n, np = c->npad;
    if (int rc = lap_check_vec(dL_dfhat, n, "mi355gp_laplace_implicit", "dL_dfhat")) return rc;
    HIP_CHECK(hipSetDevice(c->device));
    EngineShared gate(c->device);
    LaplaceSession* L = c->lap;
    hipStream_t st = c->st;
    HIP_CHECK(hipMemcpyAsync(lvec(c, LV_S), dL_dfhat, sizeof(double) * n, hipMemcpyHostToDevice, st));
    // s = K u with the u of mi355gp_laplace_gradients: dL_dfhat^T (I - K K_Wi_i) K g = s^T g for every g, because K and K_Wi_i
    // are symmetric (laplace.py:293-295).  Only vectors are written: K, X, B^-1 and a resident dL_dK stay as they are
    lap_enqueue_u(c);
    launch_symv_lower(st, L->K, np, n, lvec(c, LV_U), nullptr, lvec(c, LV_T0), nullptr, L->part);
    HIP_CHECK(hipMemcpyAsync(s_out, lvec(c, LV_T0), sizeof(double) * n, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    return 0;
}

int mi355gp_laplace_predict(mi355gp_ctx* c, int nparts, const mi355gp_part* parts, const double* Xnew, int64_t M, const double* wv,
                            double* mu_out, double* var_out, int full_cov) {
    ARG_CHECK(c && c->n > 0 && c->lap && c->lap_stage >= 3, "mi355gp_laplace_predict: call mi355gp_laplace_finish first");
    ARG_CHECK(Xnew && M > 0 && wv && mu_out, "mi355gp_laplace_predict: bad arguments");
    const long n = c->n, np = c->npad, mp = round_up(M, NB);
    if (int rc = lap_check_vec(wv, n, "mi355gp_laplace_predict", "woodbury_vector")) return rc;
    HIP_CHECK(hipSetDevice(c->device));
    EngineShared gate(c->device);
    if (int rc = ctx_prepare_parts(c, nparts, parts)) return rc;
    if (int rc = ctx_coreg_check_points(c, Xnew, M, "prediction")) return rc;
    hipStream_t st = c->st;
    ctx_scale_parts(c);
    PointSet xs;
    DevBuf dKx, dTmp, dMu, dVar, dKd, dWv, dScr1, dScr2;
    if (int rc = xs.load(st, Xnew, M, c->D)) return rc;
    HIP_CHECK(dKx.alloc(np * mp));
    HIP_CHECK(dTmp.alloc(np * mp));
    HIP_CHECK(dMu.alloc(M));
    HIP_CHECK(dWv.alloc(n));
    HIP_CHECK(dVar.alloc((full_cov ? mp * mp : M)));
    HIP_CHECK(hipMemcpyAsync(dWv, wv, sizeof(double) * n, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemsetAsync(dKx, 0, sizeof(double) * np * mp, st));
    if (full_cov && var_out) HIP_CHECK(hipMemsetAsync(dVar, 0, sizeof(double) * mp * mp, st));
    const double kdiag = expression_kdiag(c->parts, c->terms);
    const bool kd_points = ctx_has_point_diag(c) && !full_cov && var_out;
    std::vector<double> kd;
    if (kd_points) {
        kd = ctx_kdiag_points(c, Xnew, M);
        HIP_CHECK(dKd.alloc(M));
        HIP_CHECK(hipMemcpyAsync(dKd, kd.data(), sizeof(double) * M, hipMemcpyHostToDevice, st));
    }
    if (has_product(c->terms)) {
        HIP_CHECK(dScr1.alloc(np * mp));
        if (full_cov && var_out) HIP_CHECK(dScr2.alloc(mp * mp));
    }
    // Posterior._raw_predict for (woodbury_vector = Ki_fhat, woodbury_inv = K_Wi_i) (posterior.py:198-262, laplace.py:146):
    //   mu = K(X*, X) Ki_fhat;  var = K** - Kx^T W^1/2 B^-1 W^1/2 Kx = K** - |X (W^1/2 Kx)|^2
    emit_cross(st, c->parts, c->terms, ctx_training_points(c), xs, dKx, mp, dScr1, true, 0);
    if (full_cov && var_out) emit_cross(st, c->parts, c->terms, xs, xs, dVar, mp, dScr2, true, /*diag_same=*/1);
    launch_col_reduce(st, dKx, mp, n, M, dWv, 1, 0.0, 0, dMu);
    if (var_out) {
        if (c->lap->vg) launch_rowscale(st, dKx, mp, n, mp, lvec(c, LV_SW), 0, dKx);     // VarGauss: sw is the signed beta
        else launch_rowscale_sqrt(st, dKx, mp, n, mp, lvec(c, LV_W), dKx);
        launch_trmm_lower(st, c->B, np, dKx, mp, dTmp, mp, (int)(np / NB), (int)(mp / NB));
        if (!full_cov) {
            if (kd_points) launch_col_reduce_vec(st, dTmp, mp, n, M, dKd, dVar);
            else launch_col_reduce(st, dTmp, mp, n, M, nullptr, 1, kdiag, 1, dVar);
        } else {
            launch_gemm_tn_sq(st, dTmp, mp, np, dVar, mp, (int)(mp / NB), -1.0, 1.0);
        }
    }
    HIP_CHECK(hipMemcpyAsync(mu_out, dMu, sizeof(double) * M, hipMemcpyDeviceToHost, st));
    if (var_out) {
        if (!full_cov)
            HIP_CHECK(hipMemcpyAsync(var_out, dVar, sizeof(double) * M, hipMemcpyDeviceToHost, st));
        else
            HIP_CHECK(hipMemcpy2DAsync(var_out, sizeof(double) * M, dVar, sizeof(double) * mp, sizeof(double) * M, M,
                                       hipMemcpyDeviceToHost, st));
    }
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"

int laplace_fetch(mi355gp_ctx* c, int which, double* tmp) {
    const long n = c->n, np = c->npad;
    hipStream_t st = c->st;
    if (which == MI355GP_FETCH_K) {
        hipLaunchKernelGGL(k_lap_extract_full, MGRID(n), 0, st, c->lap->K, np, n, tmp);
    } else if (which == MI355GP_FETCH_KINV && c->lap_stage >= 3) {
        if (c->lap->vg && !c->lap->vg_ai) {                  // VarGauss's backward spent Ai: one lauum of the resident X brings it back
            lauum_device(st, c->B, c->C, np, &c->lap->ws);
            c->lap->vg_ai = true;
        }
        hipLaunchKernelGGL(k_lap_extract_kwi, MGRID(n), 0, st, c->C, np, n, lvec(c, LV_SW), tmp);
    } else if (which == MI355GP_FETCH_DLDK && c->lap_stage >= 4) {
        hipLaunchKernelGGL(k_lap_extract_full, MGRID(n), 0, st, c->A, np, n, tmp);
    } else {
        mi355gp_set_error("mi355gp_fetch: matrix %d is not available at this stage of the Laplace session (K after begin, the "
                          "woodbury_inv K_Wi_i after finish, dL_dK after gradients; there is no Cholesky factor of Ky)", which);
        return -4;
    }
    return 0;
}
