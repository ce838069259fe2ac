// sparse.hip -- the variational sparse GP (VarDTC) path on device: BASELINE config 5 / SURVEY.md a18.
// Replaces, for certain inputs and a homoscedastic Gaussian likelihood,
//   VarDTC.inference                 GPy/inference/latent_function_inference/var_dtc.py:66-215 (+ helpers :217-276)
//   SparseGP._update_gradients       GPy/core/sparse_gp.py:108-118  (kernel and inducing-input gradients)
//   Stationary.gradients_X           GPy/kern/src/stationary.py:245-252,330-358 (C kernel stationary_utils.c)
// in the streaming (two-pass) form the reference itself uses for its MPI variant
// (VarDTC_minibatch.gatherPsiStat, var_dtc_parallel.py:72-133):
//   pass 1 over row chunks of X:  Kfu chunk -> psi2 += Kuf Kfu (split-K MFMA Gram), psi1Y += Kuf Y
//   M x M algebra (M <= a few thousand): Lm, Lm^-1, A, LB, LB^-1, B^-1, dL_dKmm, dL_dpsi2, woodbury_inv
//   pass 2 over the same chunks:   T = Kfu dL_dpsi2 (MFMA), dL_dKnm = beta Y v^T + 2 T formed in place,
//                                  theta reductions + H = dL_dKnm * dK/dr / r, then H^T [X~ | 1] for dL/dZ
// Larger N streams through bounded chunk buffers (<= 262144 rows: 2 x 4.3 GB at M = 2048); up to that size the Kfu
// chunk of pass 1 is still resident in pass 2 and is not rebuilt.
#include <functional>
#include <memory>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/mi355gp.h"
#include "../../include/mi355gp_debug.h"
#include "../../include/mi355gp_sparse_diag.h"
#include "../../include/mi355gp_sparse_coreg.h"
#include "../../include/mi355gp_debug_sparse_coreg.h"
#include "../../include/mi355gp_psi_lin.h"
#include "../../include/mi355gp_psi_ss.h"
#include "../../include/mi355gp_sparse_missing.h"
#include "internal.h"
#include "parts.h"
#include "psi.h"
#include "psi_ss.h"
#include "psi_missing.h"
#include "sparse_ctx.h"

#define SPLITK_MAX 16
#define CHUNK_MAX 262144                    // rows per chunk: 2 x (chunk x Mp) doubles of HBM (8.6 GB at M = 2048)

// ---- elementwise M x M helpers (mp x mp row-major, ld = mp) --------------------------------------------------
// mirror the lower triangle onto the upper one; optionally sum `nsplit` partial matrices first
__global__ void k_sym_from_lower(const double* __restrict__ part, long mp, int nsplit, double* __restrict__ out) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= mp) return;
    const long a = (i >= j) ? i : j, b = (i >= j) ? j : i;
    double s = 0.0;
    for (int k = 0; k < nsplit; ++k) s += part[(long)k * mp * mp + a * mp + b];
    out[i * mp + j] = s;
}
// out = ca * A + cb * B + ci * I   (A or B may be NULL)
__global__ void k_mm_axpby(const double* __restrict__ A, double ca, const double* __restrict__ B, double cb, double ci,
                           long mp, double* __restrict__ out) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= mp) return;
    double v = (i == j) ? ci : 0.0;
    if (A) v += ca * A[i * mp + j];
    if (B) v += cb * B[i * mp + j];
    out[i * mp + j] = v;
}
// P = Dy * sym(Wlow) + w w^T   (Wlow: lower tiles of B^-1 from lauum; w: mp x Dy)
__global__ void k_form_P(const double* __restrict__ Wlow, const double* __restrict__ w, int Dy, long mp, long m,
                         double* __restrict__ P) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= mp) return;
    const long a = (i >= j) ? i : j, b = (i >= j) ? j : i;
    double v = (double)Dy * Wlow[a * mp + b];
    if (i < m && j < m)
        for (int d = 0; d < Dy; ++d) v = fma(w[i * Dy + d], w[j * Dy + d], v);
    P[i * mp + j] = v;
}
// out[0] = trace(A) ; out[1] = sum(A * P) ; out[2] = sum_i log(LB_ii) ; out[3] = sum(c^2)   over the leading m x m / m x Dy
// stage 1: one block per row i: rowpart[i] = {A_ii, sum_j A_ij P_ij, log LB_ii, sum_d c_id^2}
__global__ __launch_bounds__(256) void k_sparse_scalars_rows(const double* __restrict__ A, const double* __restrict__ P,
                                                             const double* __restrict__ LB,
                                                             const double* __restrict__ c, int Dy, long mp, long m,
                                                             double* __restrict__ rowpart) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    const long i = blockIdx.x;
    double s1 = 0.0;
    for (long j = t; j < m; j += 256) s1 = fma(A[i * mp + j], P[i * mp + j], s1);
    red[t] = s1;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (t < k) red[t] += red[t + k];
        __syncthreads();
    }
    if (t == 0) {
        double c2 = 0.0;
        for (int d = 0; d < Dy; ++d) c2 = fma(c[i * Dy + d], c[i * Dy + d], c2);
        rowpart[i * 4 + 0] = A[i * mp + i];
        rowpart[i * 4 + 1] = red[0];
        rowpart[i * 4 + 2] = log(LB[i * mp + i]);
        rowpart[i * 4 + 3] = c2;
    }
}
// stage 2 (fixed order): out[q] = sum_i rowpart[i][q]
__global__ __launch_bounds__(256) void k_sparse_scalars(const double* __restrict__ rowpart, long m,
                                                        double* __restrict__ out) {
    __shared__ double red[4][256];
    const int t = threadIdx.x;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (long i = t; i < m; i += 256)
        for (int q = 0; q < 4; ++q) s[q] += rowpart[i * 4 + q];
    for (int q = 0; q < 4; ++q) red[q][t] = s[q];
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (t < k)
            for (int q = 0; q < 4; ++q) red[q][t] += red[q][t + k];
        __syncthreads();
    }
    if (t < 4) out[t] = red[t][0];
}
// G[i][j] = beta_i * (sum_d R[i][d] v[j][d] + 2 G[i][j]) for i < rows, j < m; 0 in the padding   (dL_dKnm, var_dtc.py:219-233)
__global__ void k_form_dLdKnm(double* __restrict__ G, long ld, long rows, long rows_pad, long m,
                              const double* __restrict__ Y, const double* __restrict__ v, int Dy,
                              const double* __restrict__ beta) {
    const long j = (long)blockIdx.y * blockDim.x + threadIdx.x, i = blockIdx.x;   // rows on x: no 65535 limit
    if (j >= ld || i >= rows_pad) return;
    double g = 0.0;
    if (i < rows && j < m) {
        double yv = 0.0;
        for (int d = 0; d < Dy; ++d) yv = fma(Y[i * Dy + d], v[j * Dy + d], yv);
        g = beta[i] * fma(2.0, G[i * ld + j], yv);
    }
    G[i * ld + j] = g;
}
// out[j] = c0 - sum_i A[i][j] * B[i][j], c0 = cv[j] where a vector is given   (64 columns per block, 4 row groups, fixed-order
// combine)
__global__ __launch_bounds__(256) void k_col_dot(const double* __restrict__ A, const double* __restrict__ B, long ld,
                                                 long rows, long cols, double c0, const double* __restrict__ cv,
                                                 double* __restrict__ out) {
    __shared__ double red[4][64];
    const int tx = threadIdx.x & 63, g = threadIdx.x >> 6;
    const long j = (long)blockIdx.x * 64 + tx;
    double acc = 0.0;
    if (j < cols)
        for (long i = g; i < rows; i += 4) acc = fma(A[i * ld + j], B[i * ld + j], acc);
    red[g][tx] = acc;
    __syncthreads();
    if (g == 0 && j < cols) out[j] = (cv ? cv[j] : c0) - ((red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx]));
}
__global__ void k_vec_axpy(double* __restrict__ dst, const double* __restrict__ src, long cnt, double a) {
    const long l = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (l < cnt) dst[l] = fma(a, src[l], dst[l]);
}

// out[i][d] = w[i] * in[i][d]
__global__ void k_scale_rows(const double* __restrict__ in, const double* __restrict__ w, long cnt, int Dy,
                             double* __restrict__ out) {
    const long l = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (l < cnt) out[l] = w[l / Dy] * in[l];
}

__global__ void k_fill_const(double* __restrict__ out, long cnt, double v) {
    const long l = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (l < cnt) out[l] = v;
}

dim3 grid2d(long cols, long rows) { return dim3((unsigned)((cols + 255) / 256), (unsigned)rows); }
void launch_mm_sym(hipStream_t st, const double* low, long mp, double* out) {
    hipLaunchKernelGGL(k_sym_from_lower, grid2d(mp, mp), dim3(256), 0, st, low, mp, 1, out);
}
void launch_mm_axpby(hipStream_t st, const double* A, double ca, const double* B, double cb, double ci, long mp, double* out) {
    hipLaunchKernelGGL(k_mm_axpby, grid2d(mp, mp), dim3(256), 0, st, A, ca, B, cb, ci, mp, out);
}

// ---- communicators of the row-sharded mode ------------------------------------------------------------------------
// RCCL (one rank per process / GPU) or LOOPBACK: `world` contexts of ONE process on one device, driven by one host thread
// each, meet at a process-local rendezvous and are summed in rank order -- the transport that lets the world > 1 logic
// (global N, tr(YY^T), the two exchange steps, replicated M x M algebra) be parity-tested on a 1-GPU box.
#include <condition_variable>
#include <map>
#include <mutex>
struct LoopGroup {
    std::mutex mu;
    std::condition_variable cv;
    int world = 0, arrived = 0;
    long gen = 0;
    std::vector<double*> bufs;
};
static std::map<int, LoopGroup*> g_loop_groups;
static std::mutex g_loop_mu;

__global__ void k_vec_add(double* __restrict__ dst, const double* __restrict__ src, long cnt) {
    const long l = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (l < cnt) dst[l] += src[l];
}

static int loop_allreduce(LoopGroup* G, int rank, double* buf, size_t count, hipStream_t st) {
    HIP_CHECK(hipStreamSynchronize(st));                      // this rank's partial sums are complete
    std::unique_lock<std::mutex> lk(G->mu);
    G->bufs[(size_t)rank] = buf;
    const long gen = G->gen;
    if (++G->arrived == G->world) {                           // the last arrival reduces, in rank order, and redistributes
        const unsigned nblk = (unsigned)((count + 255) / 256);
        for (int r = 1; r < G->world; ++r)
            hipLaunchKernelGGL(k_vec_add, dim3(nblk), dim3(256), 0, st, G->bufs[0], G->bufs[(size_t)r], (long)count);
        for (int r = 1; r < G->world; ++r)
            HIP_CHECK(hipMemcpyAsync(G->bufs[(size_t)r], G->bufs[0], count * sizeof(double), hipMemcpyDeviceToDevice, st));
        HIP_CHECK(hipStreamSynchronize(st));
        G->arrived = 0;
        ++G->gen;
        G->cv.notify_all();
    } else {
        G->cv.wait(lk, [&] { return G->gen != gen; });
    }
    return 0;
}


static int sparse_allreduce(mi355gp_sparse* s, double* buf, size_t count) {
    if (s->comm) return rccl_allreduce_sum(s->comm, buf, count, s->st);
    if (s->loop) return loop_allreduce(s->loop, s->rank, buf, count, s->st);
    return 0;
}
bool sharded(const mi355gp_sparse* s) { return s->comm != nullptr || s->loop != nullptr; }

static void free_m(mi355gp_sparse* s) {
    svgp_release(s);
    pep_release(s);
    epdtc_release(s);
    s->parts.clear();
    double** ptrs[] = {&s->dZ, &s->zero1, &s->Lm, &s->Xm, &s->Tm, &s->psi2part, &s->psi2, &s->Amat,
                       &s->LB, &s->XB, &s->Bi, &s->P, &s->E, &s->T1, &s->Q2, &s->dLdKmm, &s->Winv, &s->psi1Y, &s->vecA,
                       &s->vecB, &s->cvec, &s->wvec, &s->vvec, &s->trmvPart, &s->colPart, &s->gradPart,
                       &s->gradChunk, &s->scal, &s->redbuf, &s->Kfu, &s->T};
    for (auto p : ptrs) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
    if (s->ws_ok) factor_ws_free(&s->ws);
    s->ws_ok = false;
    s->m = s->mp = 0;
    s->have_result = s->winv_ok = s->svgp_result = false;
}

int alloc_m(mi355gp_sparse* s, long M) {
    free_m(s);
    s->m = M;
    s->mp = round_up(M, NB);
    {
        // The Gram matrix has only ntl = (mp/128)(mp/128+1)/2 output tiles (136 at M = 2048) against 512 workgroup slots:
        // split K into S partial matrices, S chosen so that ntl*S fills whole rounds of the machine.
        const long nt = s->mp / NB, ntl = nt * (nt + 1) / 2;
        int best = 1;
        double beff = 0.0;
        for (int S = 1; S <= SPLITK_MAX; ++S) {
            const double wg = (double)ntl * S, eff = wg / (ceil(wg / 512.0) * 512.0);
            if (eff > beff + 1e-9 || (eff > beff - 0.02 && S < best)) { best = S; beff = eff; }
        }
        if (ntl >= 2048) best = 1;
        s->splitk = best;
        const long gran = 128L * best;                        // every split a multiple of 128 rows
        const long cmax = (CHUNK_MAX / gran) * gran;
        const long nchunks = (s->n + cmax - 1) / cmax;        // balanced chunks: no nearly-empty last chunk
        s->chunk = round_up((s->n + nchunks - 1) / nchunks, gran);
    }
    const long mp = s->mp, D = s->D, Dy = s->Dy;
    const size_t mm = sizeof(double) * mp * mp;
    const int groups = (int)((D + 31) / 32);
    HIP_CHECK(hipMalloc(&s->dZ, sizeof(double) * M * D));
    HIP_CHECK(hipMalloc(&s->zero1, sizeof(double) * 8));
    HIP_CHECK(hipMemset(s->zero1, 0, sizeof(double) * 8));
    double** mats[] = {&s->Lm, &s->Xm, &s->Tm, &s->psi2, &s->Amat, &s->LB, &s->XB, &s->Bi, &s->P, &s->E, &s->T1, &s->Q2,
                       &s->dLdKmm, &s->Winv};
    for (auto p : mats) HIP_CHECK(hipMalloc(p, mm));
    HIP_CHECK(hipMalloc(&s->psi2part, mm * SPLITK_MAX));
    HIP_CHECK(hipMalloc(&s->Kfu, sizeof(double) * s->chunk * mp));
    HIP_CHECK(hipMalloc(&s->T, sizeof(double) * s->chunk * mp));
    double** vecs[] = {&s->psi1Y, &s->vecA, &s->vecB, &s->cvec, &s->wvec, &s->vvec};
    for (auto p : vecs) HIP_CHECK(hipMalloc(p, sizeof(double) * mp * Dy));
    const long nchunks = (mp + trmv_chunk_rows(mp) - 1) / trmv_chunk_rows(mp);
    HIP_CHECK(hipMalloc(&s->trmvPart, sizeof(double) * nchunks * mp * Dy));
    const long nvmax = (D + 1 > Dy ? D + 1 : Dy);
    HIP_CHECK(hipMalloc(&s->colPart, sizeof(double) * 64 * mp * nvmax));
    HIP_CHECK(hipMalloc(&s->gradPart, sizeof(double) * groups * 2048 * GP_STRIDE));
    HIP_CHECK(hipMalloc(&s->gradChunk, sizeof(double) * groups * GP_STRIDE));
    HIP_CHECK(hipMalloc(&s->scal, sizeof(double) * 8));
    if (factor_ws_alloc(&s->ws, mp) != 0) return -3;
    s->ws_ok = true;
    return 0;
}

// Describes an expression to the kernels of kern_diag.hip: the terms, the constant diagonals, and per by-point part its D
// coefficients (Linear: variance_q itself, not the square of the input scaling), per Coregionalize part its index column, P and
// diag(B) behind those (MLP / Poly are not sparse-path kinds).  Part: PartSpec or anything derived from it, grouped by group_terms.
template <class Part>
static void describe_diag(const std::vector<Part>& parts, const Terms& terms, int D, DiagDesc* ds, std::vector<double>* coef) {
    const int np_ = (int)parts.size();
    ds->nparts = np_;
    ds->nterms = (int)terms.size();
    int k = 0;
    for (size_t t = 0; t < terms.size(); ++t) {
        ds->tstart[t] = k;
        for (int f : terms[t]) ds->tpart[k++] = f;
    }
    ds->tstart[terms.size()] = k;
    coef->assign(kdiag_coefs(np_, D), 0.0);
    ds->width = D;
    for (int i = 0; i < np_; ++i) {
        const Part& p = parts[(size_t)i];
        ds->tix[i] = p.tix;
        ds->by_point[i] = p.coreg() ? 2 : p.diag_by_point() ? 1 : 0;
        ds->var[i] = p.kp.variance;
        ds->ccol[i] = ds->cP[i] = 0;
        if (p.linear())
            for (size_t a = 0; a < p.dims.size(); ++a) (*coef)[(size_t)i * D + p.dims[a]] = p.theta[p.kp.ard ? a : 0];
        if (p.coreg()) {                                                     // diag(B) behind the nparts x D coefficients
            const int P = p.ard_in;
            ds->ccol[i] = p.kp.col;
            ds->cP[i] = P;
            if (P > ds->width) ds->width = P;
            for (int a = 0; a < P; ++a) (*coef)[(size_t)np_ * D + (size_t)i * KDIAG_MAX_OUT + a] = p.theta[(size_t)a * P + a];
        }
    }
}
// update_gradients_diag of every part in theta order from a record of weighted sums, times `scale`
template <class Part>
static void diag_dtheta(const std::vector<Part>& parts, int D, const std::vector<double>& sums, double scale, std::vector<double>* out) {
    out->clear();
    int width = D;                                                           // (DiagDesc::width, as describe_diag sets it)
    for (const Part& p : parts)
        if (p.coreg() && p.ard_in > width) width = p.ard_in;
    for (size_t i = 0; i < parts.size(); ++i) {
        const Part& p = parts[i];
        const double* r = sums.data() + 2 + i * (size_t)width;
        const size_t o = out->size();
        out->resize(o + p.theta.size(), 0.0);
        double* g = out->data() + o;
        if (!p.diag_by_point()) g[0] = scale * r[0];                         // the variance slot (stationary.py:175-184, static.py)
        else if (p.coreg())                                                  // the per-output sums land on dB[a][a] (coregionalize.py:145-151)
            for (int a = 0; a < p.ard_in; ++a) g[(size_t)a * p.ard_in + a] = scale * r[a];
        else if (p.kp.ard)                                                   // linear.py:100-105
            for (size_t a = 0; a < p.dims.size(); ++a) g[a] = scale * r[p.dims[a]];
        else
            for (size_t a = 0; a < p.dims.size(); ++a) g[0] += scale * r[p.dims[a]];
    }
}

// Decides whether Kdiag of the call's expression is a vector (a diag_by_point() part) and, if so, leaves its description in
// s->diag and the coefficients on the device
static int prepare_diag(mi355gp_sparse* s) {
    s->diag_pt = false;
    for (const SPart& p : s->parts) s->diag_pt = s->diag_pt || p.diag_by_point();
    if (!s->diag_pt) return 0;
    std::vector<double> coef;
    describe_diag(s->parts, s->terms, s->D, &s->diag, &coef);
    HIP_CHECK(s->diagCoef.need(coef.size()));
    // (pageable memory: the copy has left `coef` when the call returns)
    HIP_CHECK(hipMemcpyAsync(s->diagCoef, coef.data(), sizeof(double) * coef.size(), hipMemcpyHostToDevice, s->st));
    return 0;
}

// the kernels of kern_diag.hip for a described expression (coef: device); the record of weighted sums on its way to host_sums
static int run_kdiag(mi355gp_sparse* s, const DiagDesc& ds, const double* coef, const double* X, long rows, const double* w,
                     double* kd_out, std::vector<double>* host_sums) {
    const int S = kdiag_slots(ds.nparts, ds.width);
    if (w) {
        HIP_CHECK(s->diagPart.need((size_t)kdiag_blocks(rows) * S));
        HIP_CHECK(s->diagSums.need((size_t)S));
    }
    launch_kdiag(s->st, ds, X, rows, s->D, coef, w, kd_out, s->diagPart, s->diagSums);
    if (w && host_sums) {
        host_sums->assign((size_t)S, 0.0);
        HIP_CHECK(hipMemcpyAsync(host_sums->data(), s->diagSums, sizeof(double) * S, hipMemcpyDeviceToHost, s->st));
    }
    return 0;
}
int sparse_kdiag(mi355gp_sparse* s, const double* X, long rows, const double* w, double* kd_out, std::vector<double>* host_sums) {
    return run_kdiag(s, s->diag, s->diagCoef, X, rows, w, kd_out, host_sums);
}
int sparse_kdiag_data(mi355gp_sparse* s, const double* w, std::vector<double>* host_sums) {
    HIP_CHECK(s->dKd.need((size_t)s->n));
    return sparse_kdiag(s, s->dX, s->n, w, s->dKd, host_sums);
}
void sparse_diag_dtheta(const mi355gp_sparse* s, const std::vector<double>& sums, double scale, std::vector<double>* out) {
    diag_dtheta(s->parts, s->D, sums, scale, out);
}

// The index column of the context's rows against a Coregionalize part, on the host copy that set_data keeps while
// mi355gp_sparse_set_coregionalize is on; once per (column, P) and data set
static int coreg_check_data(mi355gp_sparse* s, const PartSpec& p) {
    const std::pair<int, int> key(p.kp.col, p.ard_in);
    for (const auto& k : s->coreg_ok)
        if (k == key) return 0;
    if (s->hX.size() != (size_t)s->n * (size_t)s->D)
        PART_FAIL("sparse path: Coregionalize (kind 8): mi355gp_sparse_set_coregionalize must be on before mi355gp_sparse_set_data "
                  "(the rows' output indices are checked on the host copy that set_data keeps while it is on)");
    if (int rc = coreg_check_index(s->hX.data() + p.kp.col, s->n, s->D, p.ard_in, "training")) return rc;
    s->coreg_ok.push_back(key);
    return 0;
}
// the same check of m row-major points (Z, new points) against every Coregionalize part of the call: every time
static int coreg_check_points(const mi355gp_sparse* s, const double* X, long m, const char* what) {
    for (const SPart& p : s->parts)
        if (p.coreg())
            if (int rc = coreg_check_index(X + p.kp.col, m, s->D, p.ard_in, what)) return rc;
    return 0;
}

// (re)builds the part list of a call; the device buffers of a part are kept while the number of parts is unchanged
int prepare_sparse_parts(mi355gp_sparse* s, int nparts, const mi355gp_part* parts, bool coreg) {
    ARG_CHECK(nparts >= 1 && nparts <= 16 && parts, "between 1 and 16 kernel parts");
    // Linear is taken where the context was told so (mi355gp_sparse_set_linear; off in a new context: a caller that has not
    // asked keeps the refusal by name); Coregionalize likewise (mi355gp_sparse_set_coregionalize), by the entry points that say so
    const KindSet accepted = KS_STATIONARY | KS_STATIC | (s->take_linear ? KS_LINEAR : 0u) | (s->take_coreg && coreg ? KS_COREG : 0u);
    for (int i = 0; i < nparts; ++i)                             // before any device work: the global sums of a per-point
        if (kind_in(parts[i].kind, accepted) && parts[i].kind == MI355GP_LINEAR && sharded(s))   // diagonal would need another all-reduce
            PART_FAIL("sparse path: a Linear (kind 9) part is not supported by a row-sharded context (its Kdiag depends on the "
                      "point: the sums over rows would need a collective of their own)");
    for (int i = 0; i < nparts; ++i) {
        if (parts[i].kind != MI355GP_COREGIONALIZE || !s->take_coreg) continue;
        if (!coreg)
            PART_FAIL("sparse path: a Coregionalize (kind 8) part is taken by mi355gp_vardtc_inference_sum and mi355gp_sparse_predict "
                      "alone; this entry point does not evaluate the kind (PEP / FITC, SVGP and EPDTC have no per-point noise model that "
                      "fits the outputs' own noise variances; uncertain inputs have no psi-statistics for it)");
        if (sharded(s))
            PART_FAIL("sparse path: a Coregionalize (kind 8) part is not supported by a row-sharded context (its Kdiag depends on "
                      "the point: the sums over rows would need a collective of their own)");
    }
    const long mp = s->mp, D = s->D;
    const int groups = (int)((D + 31) / 32);
    if ((int)s->parts.size() != nparts) {
        s->parts.clear();
        s->parts.resize((size_t)nparts);
        if (s->redbuf) (void)hipFree(s->redbuf);
        s->redbuf = nullptr;
        HIP_CHECK(hipMalloc(&s->redbuf, sizeof(double) * nparts * ((size_t)groups * GP_STRIDE + (size_t)mp * (D + 1))));
        for (SPart& p : s->parts) {
            HIP_CHECK(p.XtZ.alloc(D * mp));
            HIP_CHECK(p.XtC.alloc(D * s->chunk));
            HIP_CHECK(p.HX.alloc(mp * (D + 1)));
            HIP_CHECK(p.HZ.alloc(mp * (D + 1)));
            HIP_CHECK(p.gradNM.alloc(groups * GP_STRIDE));
            HIP_CHECK(p.gradMM.alloc(groups * GP_STRIDE));
        }
    }
    for (int i = 0; i < nparts; ++i) {
        SPart& p = s->parts[(size_t)i];
        if (int rc = parse_part(parts[i], (int)D, accepted, "sparse path", &p)) return rc;
        if (p.coreg()) {
            if (int rc = coreg_check_data(s, p)) return rc;             // before any launch reads an index of X
            if (!p.cgNM) HIP_CHECK(p.cgNM.alloc(COREG_REC));
            if (!p.cgMM) HIP_CHECK(p.cgMM.alloc(COREG_REC));
            HIP_CHECK(s->cgPart.need((size_t)2048 * COREG_REC));
            HIP_CHECK(s->cgChunk.need(COREG_REC));
        }
        if (int rc = p.upload(s->st)) return rc;
    }
    s->terms = group_terms(s->parts);
    for (const auto& t : s->terms)
        if (t.size() > 1)
            for (int f : t)
                ARG_CHECK(s->parts[(size_t)f].kp.kind != MI355GP_WHITE, "a White factor inside a product is not supported by the sparse path");
    return prepare_diag(s);
}

// product of the OTHER factors' variances of part p's summand (= dKdiag/dvariance_p; 1 for a plain summand)
double sparse_other_variances(const mi355gp_sparse* s, size_t p) {
    double v = 1.0;
    for (int f : s->terms[(size_t)s->parts[p].tix])
        if ((size_t)f != p) v *= s->parts[(size_t)f].kp.variance;
    return v;
}
// cross-covariances leave out summands that are a White part alone (White contributes nothing off the diagonal, static.py:77-81)
bool skip_white(const mi355gp_sparse* s, const std::vector<int>& t) {
    return t.size() == 1 && s->parts[(size_t)t[0]].kp.kind == MI355GP_WHITE;
}

// scaled, dimension-major copies of `rows` points (row-major src) for every part
void scale_for_parts(mi355gp_sparse* s, const double* src, long rows, long ldt, bool inducing) {
    for (SPart& p : s->parts) launch_scale_inputs(s->st, src, rows, s->D, p.dIl, 1, inducing ? p.XtZ : p.XtC, ldt);
}
// the inducing inputs as one side of a cross-covariance (emit_cross)
Resident<SPart> inducing_points(const mi355gp_sparse* s) { return {&SPart::XtZ, s->mp, s->m}; }

// Kfu chunk = sum over summands of (the product of) K_p(X_chunk, Z)  (add.py:58-72, prod.py:58-65; White contributes nothing
// off the diagonal, static.py:77-81).  Products are multiplied up in `scratch` (chunk x mp, e.g. the T buffer).
void build_cross_chunk(mi355gp_sparse* s, long rc, double* out, double* scratch) {
    const bool any = emit_cross(s->st, s->parts, s->terms, Resident<SPart>{&SPart::XtC, s->chunk, rc}, inducing_points(s), out, s->mp,
                                scratch, false, 0, [&](const std::vector<int>& t) { return skip_white(s, t); });
    if (!any) (void)hipMemsetAsync(out, 0, sizeof(double) * rc * s->mp, s->st);       // only White parts: K(X, Z) = 0
}
// K(Z) (lower tiles; diag != NULL: + diag on the diagonal) of the expression into out (mp x mp), scratch mp x mp
void build_kmm(mi355gp_sparse* s, double* out, double* scratch, double jitter, int lower_only, hipStream_t st) {
    if (!st) st = s->st;
    emit_expression(s->terms, out, scratch, false, [&](int p, double* dst, const double* mul, int acc, bool first) {
        const SPart& pt = s->parts[(size_t)p];
        launch_kbuild_sym(st, pt.kp, pt.XtZ, s->mp, s->m, s->mp, dst, s->zero1, 1, jitter, lower_only,
                          /*add_diag=*/(first && dst == out) ? 1 : 0, acc, mul);
    });
}
// W[i][j] = beta_i (sum_d R[i][d] v[j][d] + 2 T[i][j]) * W[i][j] for i < rows, j < m; 0 in the padding: dL_dKnm times the other
// factors' covariance (prod.py:86-99), the weights one factor of a product sees
__global__ void k_form_dLdKnm_times(const double* __restrict__ T, double* __restrict__ W, long ld, long rows, long rows_pad,
                                    long m, const double* __restrict__ Y, const double* __restrict__ v, int Dy,
                                    const double* __restrict__ beta) {
    const long j = (long)blockIdx.y * blockDim.x + threadIdx.x, i = blockIdx.x;
    if (j >= ld || i >= rows_pad) return;
    double g = 0.0;
    if (i < rows && j < m) {
        double yv = 0.0;
        for (int d = 0; d < Dy; ++d) yv = fma(Y[i * Dy + d], v[j * Dy + d], yv);
        g = beta[i] * fma(2.0, T[i * ld + j], yv) * W[i * ld + j];
    }
    W[i * ld + j] = g;
}
// A[i][j] *= B[i][j]  (mp x mp)
__global__ void k_mm_mul(double* __restrict__ A, const double* __restrict__ B, long mp) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j < mp) A[i * mp + j] *= B[i * mp + j];
}

extern "C" {

int mi355gp_sparse_create(int device, mi355gp_sparse** out) {
    int n = 0;
    mi355gp_device_count(&n);
    if (device < 0 || device >= n) {
        mi355gp_set_error("mi355gp_sparse_create: device %d not available (%d HIP devices visible)", device, n);
        return -2;
    }
    HIP_CHECK(hipSetDevice(device));
    mi355gp_sparse* s = new mi355gp_sparse();
    s->device = device;
    if (factor_engine(device, &s->st, nullptr, nullptr) != 0) return -2;    // the device's shared main stream
    {
        const char* e = DIAG_ENV("SPARSE_FUSE_COLS");
        if (e && *e) s->fuse_cols = atoi(e) ? 1 : 0;
    }
    for (auto& e : s->ev) HIP_CHECK(hipEventCreate(&e));
    {
        const char* e = DIAG_ENV("SPARSE_KMM_OVERLAP");
        if (e && *e) s->kmm_overlap = atoi(e) ? 1 : 0;
        HIP_CHECK(hipStreamCreateWithFlags(&s->st_kmm, hipStreamNonBlocking));
        HIP_CHECK(hipEventCreateWithFlags(&s->ev_z, hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&s->ev_kmm, hipEventDisableTiming));
    }
    *out = s;
    return 0;
}

int mi355gp_sparse_get_profile(mi355gp_sparse* s, double* out6) {
    ARG_CHECK(s && out6, "mi355gp_sparse_get_profile: NULL argument");
    HIP_CHECK(hipSetDevice(s->device));
    HIP_CHECK(hipStreamSynchronize(s->st));
    double ms[PF_NUM], fl[PF_NUM];
    int nl[PF_NUM];
    if (s->mfma_prof.collect(ms, fl, nl) != 0) {
        mi355gp_set_error("mi355gp_sparse_get_profile: event timing failed");
        return -5;
    }
    for (int f = 0; f < 2; ++f) {
        out6[3 * f] = ms[f];
        out6[3 * f + 1] = fl[f];
        out6[3 * f + 2] = (double)nl[f];
    }
    return 0;
}

int mi355gp_sparse_destroy(mi355gp_sparse* s) {
    if (!s) return 0;
    (void)hipSetDevice(s->device);
    (void)hipStreamSynchronize(s->st);
    free_m(s);
    missing_release(s);
    double** ptrs[] = {&s->dX, &s->dY, &s->dV, &s->dBeta, &s->dRowS, &s->dRowT, &s->dRowR, &s->dSvar, &s->dGam};
    for (auto p : ptrs)
        if (*p) (void)hipFree(*p);
    if (s->comm) rccl_comm_destroy(s->comm);
    for (auto& e : s->ev)
        if (e) (void)hipEventDestroy(e);
    if (s->st_kmm) {
        (void)hipStreamSynchronize(s->st_kmm);
        (void)hipStreamDestroy(s->st_kmm);
    }
    if (s->ev_z) (void)hipEventDestroy(s->ev_z);
    if (s->ev_kmm) (void)hipEventDestroy(s->ev_kmm);
    s->mfma_prof.destroy();
    if (s->st) (void)hipStreamSynchronize(s->st);
    delete s;
    return 0;
}

int mi355gp_sparse_set_data(mi355gp_sparse* s, const double* X, int64_t N, int D, const double* Y, int Dy) {
    ARG_CHECK(s && X && Y && N > 0 && D > 0 && Dy > 0, "mi355gp_sparse_set_data: bad arguments");
    HIP_CHECK(hipSetDevice(s->device));
    EngineShared gate(s->device);
    HIP_CHECK(hipStreamSynchronize(s->st));
    free_m(s);
    missing_release(s);                                         // (the output groups of mi355gp_sparse_set_output_groups)
    double** ptrs[] = {&s->dX, &s->dY, &s->dV, &s->dBeta, &s->dRowS, &s->dRowT, &s->dRowR, &s->dSvar, &s->dGam};
    for (auto p : ptrs) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
    s->n = N;
    s->D = D;
    s->Dy = Dy;
    HIP_CHECK(hipMalloc(&s->dX, sizeof(double) * N * D));
    HIP_CHECK(hipMalloc(&s->dY, sizeof(double) * N * Dy));
    HIP_CHECK(hipMalloc(&s->dV, sizeof(double) * N * Dy));
    HIP_CHECK(hipMalloc(&s->dBeta, sizeof(double) * N));
    HIP_CHECK(hipMalloc(&s->dRowS, sizeof(double) * N * Dy));
    HIP_CHECK(hipMalloc(&s->dRowT, sizeof(double) * N));
    HIP_CHECK(hipMalloc(&s->dRowR, sizeof(double) * N));
    HIP_CHECK(hipMemcpy(s->dX, X, sizeof(double) * N * D, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(s->dY, Y, sizeof(double) * N * Dy, hipMemcpyHostToDevice));
    s->coreg_ok.clear();                                        // (Coregionalize: the rows' indices are checked against this copy)
    if (s->take_coreg) s->hX.assign(X, X + N * D);
    else std::vector<double>().swap(s->hX);
    double t = 0.0;
    s->rowYY.assign((size_t)N, 0.0);
    for (int64_t i = 0; i < N; ++i) {
        double r = 0.0;
        for (int d = 0; d < Dy; ++d) r += Y[i * Dy + d] * Y[i * Dy + d];
        s->rowYY[(size_t)i] = r;
        t += r;                                                 // get_trYYT (var_dtc.py:48-54)
    }
    s->trYYT = t;
    s->trYYT_local = t;                                        // this shard's share (the per-shard sums of the log likelihood)
    s->n_global = N;
    if (sharded(s)) {                                          // global N and tr(Y Y^T) over the shards
        double h[2] = {(double)N, t}, *d = nullptr;
        HIP_CHECK(hipMalloc(&d, sizeof(h)));
        HIP_CHECK(hipMemcpy(d, h, sizeof(h), hipMemcpyHostToDevice));
        if (int rc = sparse_allreduce(s, d, 2)) return rc;
        HIP_CHECK(hipStreamSynchronize(s->st));
        HIP_CHECK(hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost));
        (void)hipFree(d);
        s->n_global = (long)(h[0] + 0.5);
        s->trYYT = h[1];
    }
    return 0;
}

// Input variances S (N x D, the shape of set_data's X, which is then read as the mean of q(x_n) = N(mu_n, diag S_n)); every
// entry must be positive and finite, checked here on the host before anything is launched.  set_data discards them.
int mi355gp_sparse_set_input_variance(mi355gp_sparse* s, const double* S, int64_t N, int D) {
    ARG_CHECK(s && s->n > 0, "mi355gp_sparse_set_input_variance: set_data first");
    ARG_CHECK(S && N == s->n && D == s->D, "mi355gp_sparse_set_input_variance: S must be N x D, the shape of X");
    ARG_CHECK(!sharded(s), "mi355gp_sparse_set_input_variance: uncertain inputs are not supported by a row-sharded context");
    for (int64_t i = 0; i < N * D; ++i)
        if (!(S[i] > 0.0) || !std::isfinite(S[i]))
            PART_FAIL("mi355gp_sparse_set_input_variance: input variance S[%lld][%lld] = %g: every entry must be positive and finite",
                      (long long)(i / D), (long long)(i % D), S[i]);
    HIP_CHECK(hipSetDevice(s->device));
    EngineShared gate(s->device);
    HIP_CHECK(hipStreamSynchronize(s->st));
    if (!s->dSvar) HIP_CHECK(hipMalloc(&s->dSvar, sizeof(double) * N * D));
    HIP_CHECK(hipMemcpy(s->dSvar, S, sizeof(double) * N * D, hipMemcpyHostToDevice));
    s->have_result = s->winv_ok = s->svgp_result = false;
    return 0;
}

// Replaces the inputs of set_data -- X (N x D), and with S != NULL the input variances -- and nothing else: Y and everything
// sized by Y stay resident (a Bayesian GPLVM step changes every mean and variance of q(X) and not Y, the wide matrix).  S is
// validated as mi355gp_sparse_set_input_variance validates it; the last result is forgotten as after set_data.
int mi355gp_sparse_set_inputs(mi355gp_sparse* s, const double* X, const double* S, int64_t N, int D) {
    ARG_CHECK(s && s->n > 0, "mi355gp_sparse_set_inputs: set_data first");
    ARG_CHECK(X && N == s->n && D == s->D, "mi355gp_sparse_set_inputs: X (and S) must be N x D, the shape of set_data's X");
    ARG_CHECK(!sharded(s), "mi355gp_sparse_set_inputs: replacing the inputs of a row-sharded context is not supported");
    for (int64_t i = 0; i < N * D; ++i) {
        if (!std::isfinite(X[i]))
            PART_FAIL("mi355gp_sparse_set_inputs: input X[%lld][%lld] = %g is not finite", (long long)(i / D), (long long)(i % D), X[i]);
        if (S && (!(S[i] > 0.0) || !std::isfinite(S[i])))
            PART_FAIL("mi355gp_sparse_set_inputs: input variance S[%lld][%lld] = %g: every entry must be positive and finite",
                      (long long)(i / D), (long long)(i % D), S[i]);
    }
    HIP_CHECK(hipSetDevice(s->device));
    EngineShared gate(s->device);
    HIP_CHECK(hipStreamSynchronize(s->st));
    if (S && !s->dSvar) HIP_CHECK(hipMalloc(&s->dSvar, sizeof(double) * N * D));
    HIP_CHECK(hipMemcpy(s->dX, X, sizeof(double) * N * D, hipMemcpyHostToDevice));
    if (S) HIP_CHECK(hipMemcpy(s->dSvar, S, sizeof(double) * N * D, hipMemcpyHostToDevice));
    s->coreg_ok.clear();                                        // (as set_data: no stale rows for a later index check)
    if (s->take_coreg) s->hX.assign(X, X + N * D);
    else std::vector<double>().swap(s->hX);
    s->have_result = s->winv_ok = s->svgp_result = false;
    return 0;
}

// Slab probabilities gamma (N x D) next to the resident means (set_data's X) and variances: q(x_nq) is then the spike-and-slab
// gamma_nq N(mu_nq, S_nq) + (1 - gamma_nq) delta_0 of mi355gp_vardtc_inference_ss.  gamma == NULL takes the context back to
// Gaussian inputs.  Every entry must be finite and strictly inside (0, 1); set_data discards them.
static int check_binary_prob(const char* where, const double* gamma, int64_t N, int D) {
    for (int64_t i = 0; i < N * D; ++i)
        if (!(gamma[i] > 0.0 && gamma[i] < 1.0))
            PART_FAIL("%s: slab probability gamma[%lld][%lld] = %g: every entry must be finite and strictly inside (0, 1)", where,
                      (long long)(i / D), (long long)(i % D), gamma[i]);
    return 0;
}
int mi355gp_sparse_set_binary_prob(mi355gp_sparse* s, const double* gamma, int64_t N, int D) {
    ARG_CHECK(s && s->n > 0, "mi355gp_sparse_set_binary_prob: set_data first");
    ARG_CHECK(!sharded(s), "mi355gp_sparse_set_binary_prob: spike-and-slab inputs are not supported by a row-sharded context");
    HIP_CHECK(hipSetDevice(s->device));
    if (!gamma) {
        EngineShared gate(s->device);
        HIP_CHECK(hipStreamSynchronize(s->st));
        if (s->dGam) (void)hipFree(s->dGam);
        s->dGam = nullptr;
        s->have_result = s->winv_ok = s->svgp_result = false;
        return 0;
    }
    ARG_CHECK(N == s->n && D == s->D, "mi355gp_sparse_set_binary_prob: gamma must be N x D, the shape of X");
    ARG_CHECK(s->dSvar, "mi355gp_sparse_set_binary_prob: no input variances; call mi355gp_sparse_set_input_variance first");
    if (int rc = check_binary_prob("mi355gp_sparse_set_binary_prob", gamma, N, D)) return rc;
    EngineShared gate(s->device);
    HIP_CHECK(hipStreamSynchronize(s->st));
    if (!s->dGam) HIP_CHECK(hipMalloc(&s->dGam, sizeof(double) * N * D));
    HIP_CHECK(hipMemcpy(s->dGam, gamma, sizeof(double) * N * D, hipMemcpyHostToDevice));
    s->have_result = s->winv_ok = s->svgp_result = false;
    return 0;
}

// The three-array form of mi355gp_sparse_set_inputs, the upload of one SSGPLVM step: means, variances and slab probabilities
// (all N x D, all required); Y stays resident.
int mi355gp_sparse_set_inputs_ss(mi355gp_sparse* s, const double* X, const double* S, const double* gamma, int64_t N, int D) {
    ARG_CHECK(s && s->n > 0, "mi355gp_sparse_set_inputs_ss: set_data first");
    ARG_CHECK(X && S && gamma && N == s->n && D == s->D,
              "mi355gp_sparse_set_inputs_ss: X, S and gamma must be N x D, the shape of set_data's X");
    ARG_CHECK(!sharded(s), "mi355gp_sparse_set_inputs_ss: replacing the inputs of a row-sharded context is not supported");
    if (int rc = check_binary_prob("mi355gp_sparse_set_inputs_ss", gamma, N, D)) return rc;
    if (int rc = mi355gp_sparse_set_inputs(s, X, S, N, D)) return rc;
    EngineShared gate(s->device);
    if (!s->dGam) HIP_CHECK(hipMalloc(&s->dGam, sizeof(double) * N * D));
    HIP_CHECK(hipMemcpy(s->dGam, gamma, sizeof(double) * N * D, hipMemcpyHostToDevice));
    return 0;
}

// Row-sharded mode: call once, before set_data, on every rank (id128 from mi355gp_grid_unique_id on rank 0).
// Each rank then passes ITS rows to mi355gp_sparse_set_data; Z and theta are replicated; results are identical on all ranks.
int mi355gp_sparse_attach_comm(mi355gp_sparse* s, int rank, int world, const void* id128) {
    ARG_CHECK(s && id128 && world >= 1 && rank >= 0 && rank < world, "mi355gp_sparse_attach_comm: bad arguments");
    HIP_CHECK(hipSetDevice(s->device));
    EngineShared gate(s->device);
    if (s->comm) rccl_comm_destroy(s->comm);
    s->comm = nullptr;
    s->loop = nullptr;
    if (int rc = rccl_comm_create(rank, world, id128, &s->comm)) return rc;
    s->rank = rank;
    s->world = world;
    return 0;
}

// The same mode over the LOOPBACK transport: `world` contexts of this process (one host thread each, any devices... the
// 1-GPU box: all on one) that name the same group_key meet at a process-local rendezvous for every exchange step.
int mi355gp_sparse_attach_loopback(mi355gp_sparse* s, int rank, int world, int group_key) {
    ARG_CHECK(s && world >= 1 && rank >= 0 && rank < world, "mi355gp_sparse_attach_loopback: bad arguments");
    std::lock_guard<std::mutex> lk(g_loop_mu);
    LoopGroup*& G = g_loop_groups[group_key];
    if (!G) {
        G = new LoopGroup();
        G->world = world;
        G->bufs.assign((size_t)world, nullptr);
    }
    ARG_CHECK(G->world == world, "mi355gp_sparse_attach_loopback: the group exists with a different world size");
    if (s->comm) rccl_comm_destroy(s->comm);
    s->comm = nullptr;
    s->loop = G;
    s->rank = rank;
    s->world = world;
    return 0;
}

// Cholesky of an M x M matrix of the sparse path with the persistent launch's "did not run" outcomes handled in place: when the
// single-launch schedule was taken, the host reads info[0] right away (one stream sync, twice per evaluation: ~0.1 % of
// configuration 5) and, if the launch was called off at its co-residency gate or aborted, redoes the factorisation with the
// launch-per-step schedule -- on the untouched matrix, or after rebuild() if it was partly overwritten.  Doing it HERE (and not
// by repeating the evaluation) keeps a row-sharded run in step: the redo involves no collective.  info_host receives the
// LAPACK-style info (0 or the first non-positive pivot), never an abort code.
static int factor_launch(hipStream_t st, double* A, double* X, double* T, double* W, long mp, FactorWs* ws) {
    // A -> L (in place), X = L^-1 (T: scratch of the launch-per-step inverse), W = X^T X if W != NULL.  X is used as a FULL
    // matrix by the GEMMs of the M x M phase: its strictly upper tiles are zeroed here (no schedule writes them).
    HIP_CHECK(hipMemsetAsync(X, 0, sizeof(double) * mp * mp, st));
    potrf_device(st, A, mp, ws);
    trtri_device(st, A, X, T, mp, ws);
    if (W) lauum_device(st, X, W, mp, ws);
    return 0;
}
// the host side of the same: reads info[0] (one stream sync when the persistent schedule was taken) and redoes the factorisation
// on the launch-per-step schedule if the launch was called off (matrix untouched) or aborted (rebuild() first)
static int factor_check(hipStream_t st, double* A, double* X, double* T, double* W, long mp, FactorWs* ws, int* info_host,
                        const std::function<void()>& rebuild) {
    if (!ws->persist_used) {
        HIP_CHECK(hipMemcpyAsync(info_host, ws->info, sizeof(int), hipMemcpyDeviceToHost, st));
        return 0;
    }
    int info = 0;
    HIP_CHECK(hipMemcpyAsync(&info, ws->info, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    bool clean = false;
    if (potrf_persist_aborted(info, ws, &clean)) {
        if (!clean) rebuild();
        HIP_CHECK(hipMemsetAsync(X, 0, sizeof(double) * mp * mp, st));
        potrf_device(st, A, mp, ws);                           // persist_skip > 0: the launch-per-step schedule
        trtri_device(st, A, X, T, mp, ws);
        if (W) lauum_device(st, X, W, mp, ws);
        HIP_CHECK(hipMemcpyAsync(&info, ws->info, sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (info >= PS_ABORT_INFO) {
            mi355gp_set_error("sparse path: the M x M factorisation aborted twice (info %d)", info);
            return -6;
        }
    }
    *info_host = info;
    return 0;
}
int potrf_checked(hipStream_t st, double* A, double* X, double* T, double* W, long mp, FactorWs* ws, int* info_host,
                  const std::function<void()>& rebuild) {
    if (int rc = factor_launch(st, A, X, T, W, mp, ws)) return rc;
    return factor_check(st, A, X, T, W, mp, ws, info_host, rebuild);
}

// The M x M phase of an evaluation, shared by the certain- and the uncertain-input entry points: from psi2 (s->psi2), psi1^T V
// (s->psi1Y) and Lm / Xm to A, LB, B^-1, the Woodbury vectors, dL_dKmm, Q2 = dL_dpsi2_beta and the four scalars; records ev[2].
static int sparse_mm_block(mi355gp_sparse* s, bool het, double beta, int inject) {
    hipStream_t st = s->st;
    const long m = s->m, mp = s->mp;
    const int Dy = s->Dy;
    const bool het_multi = het && Dy > 1;
    // ---- M x M algebra ----------------------------------------------------------------------------------------
    // A = Lm^-1 psi2_beta Lm^-T (var_dtc.py:129-134), B = I + A (:137), LB = chol(B) (:138), XB = LB^-1
    // (Xm = Lm^-1 is lower triangular: the four products below walk only its non-zero k range, half the flops of full GEMMs)
    const int ntm = (int)(mp / NB);
    launch_trmm64(st, 0, s->Xm, mp, s->psi2, mp, s->T1, mp, ntm, ntm, 1.0);
    launch_trmm64(st, 2, s->Xm, mp, s->T1, mp, s->Amat, mp, ntm, ntm, het ? 1.0 : beta);
    auto build_B = [&]() { launch_mm_axpby(st, s->Amat, 1.0, nullptr, 0.0, 1.0, mp, s->LB); };
    build_B();
    if (inject == 11 || inject == 12) s->ws.persist_test = inject - 10, s->ws.persist_skip = 0;
    // LB = chol(B), XB = LB^-1 and B^-1 = XB^T XB (lower tiles; :150) in one go
    if (int rc = potrf_checked(st, s->LB, s->XB, s->Tm, s->Bi, mp, &s->ws, &s->h_info[1], build_B)) return rc;
    // c = LB^-1 Lm^-1 psi1 V (:141-143), w = LB^-T c (:144), v = Lm^-T w = woodbury_vector (:145)
    launch_trmv_lower(st, s->Xm, mp, mp, s->psi1Y, Dy, s->vecA);
    launch_trmv_lower(st, s->XB, mp, mp, s->vecA, Dy, s->cvec);
    launch_trmv_lower_T(st, s->XB, mp, mp, s->cvec, Dy, s->wvec, s->trmvPart);
    launch_trmv_lower_T(st, s->Xm, mp, mp, s->wvec, Dy, s->vvec, s->trmvPart);
    // B^-1 = XB^T XB (lower tiles: computed with the factorisation above), P = Dy B^-1 + w w^T = DBi_plus_BiPBi (:150-152)
    hipLaunchKernelGGL(k_form_P, grid2d(mp, mp), dim3(256), 0, st, s->Bi, s->wvec, Dy, mp, m, s->P);
    // dL_dKmm = Lm^-T (-0.5 P - 0.5 Dy B + Dy I) Lm^-1 (:153-158);  -0.5 Dy (I + A) + Dy I = -0.5 Dy A + 0.5 Dy I
    launch_mm_axpby(st, s->P, -0.5, s->Amat, -0.5 * Dy, 0.5 * Dy, mp, s->E);
    launch_trmm64(st, 1, s->Xm, mp, s->E, mp, s->T1, mp, ntm, ntm, 1.0);                 // Xm^T E
    launch_trmm64(st, 3, s->Xm, mp, s->T1, mp, s->dLdKmm, mp, ntm, ntm, 1.0);            // (Xm^T E) Xm
    // Q2 = dL_dpsi2_beta = 0.5 Lm^-T (Dy I - P) Lm^-1 (:220); the precision enters per row in pass 2 (:224-226,231)
    launch_mm_axpby(st, s->P, -0.5, nullptr, 0.0, 0.5 * Dy, mp, s->E);
    launch_trmm64(st, 1, s->Xm, mp, s->E, mp, s->T1, mp, ntm, ntm, 1.0);
    launch_trmm64(st, 3, s->Xm, mp, s->T1, mp, s->Q2, mp, ntm, ntm, 1.0);
    if (het_multi) {
        // several output columns with per-point noise: dL_dR (var_dtc.py:240-256) needs r_n = |LB^-1 Lm^-1 k_n|^2 on its own
        // (for Dy = 1 it folds into t_n and s_n); r_n = k_n^T Gr k_n with Gr = Lm^-T B^-1 Lm^-1, built in the Winv buffer
        launch_mm_sym(st, s->Bi, mp, s->E);
        launch_trmm64(st, 1, s->Xm, mp, s->E, mp, s->T1, mp, ntm, ntm, 1.0);
        launch_trmm64(st, 3, s->Xm, mp, s->T1, mp, s->Winv, mp, ntm, ntm, 1.0);
    }
    hipLaunchKernelGGL(k_sparse_scalars_rows, dim3((unsigned)m), dim3(256), 0, st, s->Amat, s->P, s->LB, s->cvec, Dy, mp, m,
                       s->colPart);
    hipLaunchKernelGGL(k_sparse_scalars, dim3(1), dim3(256), 0, st, s->colPart, m, s->scal);
    HIP_CHECK(hipEventRecord(s->ev[2], st));
    return 0;
}

// update_gradients_full(dL_dKmm, Z) and gradients_X(dL_dKmm, Z) of every part into its gradMM records and HZ
void sparse_kmm_gradients(mi355gp_sparse* s) {
    hipStream_t st = s->st;
    const long m = s->m, mp = s->mp;
    const int D = s->D, groups = (D + 31) / 32;
    // the M x M part: update_gradients_full(dL_dKmm, Z) and gradients_X(dL_dKmm, Z) (sparse_gp.py:114-117), per part; a factor
    // of a product sees dL_dKmm times the other factors' K(Z) (prod.py:86-99), materialised in T1
    for (size_t pi = 0; pi < s->parts.size(); ++pi) {
        SPart& p = s->parts[pi];
        const int nbk = grad_generic_num_blocks(m, m);
        const bool prod = emit_other_factors(s->terms, p.tix, pi, s->T1, [&](int f, double* dst, const double* mul, int, bool) {
            const SPart& pf = s->parts[(size_t)f];
            launch_kbuild_cross(st, pf.kp, pf.XtZ, mp, m, pf.XtZ, mp, m, dst, mp, 0, /*diag_same=*/1, mul);
        });
        if (prod) hipLaunchKernelGGL(k_mm_mul, grid2d(mp, mp), dim3(256), 0, st, s->T1, s->dLdKmm, mp);
        if (p.coreg()) {
            // the bucketed pass over the whole M x M matrix (dL_dKmm is symmetric; every element once): S[a][b] = the sum over
            // rows of output a and columns of output b, blocks combined in block order; gradients_X is zero (coregionalize.py:153)
            const int P2 = p.ard_in * p.ard_in;
            const int nb = launch_grad_coreg(st, false, p.kp, p.XtZ, mp, m, p.XtZ, mp, m, prod ? s->T1 : s->dLdKmm, mp, nullptr, 0, s->cgPart);
            launch_reduce_partials(st, s->cgPart, nb, P2, p.cgMM);
            continue;
        }
        launch_grad_generic(st, p.kp, p.XtZ, mp, m, p.XtZ, mp, m, 1, prod ? s->T1 : s->dLdKmm, mp, s->gradPart,
                            p.stationary() ? s->T1 : nullptr, mp);
        for (int g = 0; g < (p.kp.ard ? groups : 1); ++g)
            launch_reduce_partials(st, s->gradPart + (long)g * nbk * GP_STRIDE, nbk, GP_STRIDE, p.gradMM + (long)g * GP_STRIDE);
        if (p.stationary()) {
            const int ns = launch_colreduce_multi(st, s->T1, mp, m, mp, p.XtZ, 1, mp, D, 1, s->colPart);
            launch_sum_splits(st, s->colPart, mp * (D + 1), ns, 0, p.HZ);
        } else if (p.linear()) {                         // HZ = G^T z~ of the weights themselves (linear.py:108-114)
            const int ns = launch_colreduce_multi(st, prod ? s->T1 : s->dLdKmm, mp, m, mp, p.XtZ, 1, mp, D, 0, s->colPart);
            launch_sum_splits(st, s->colPart, mp * D, ns, 0, p.HZ);
        }
    }
}

// ---- the phases an inference family is built from ---------------------------------------------------------
// Opens a call (the caller holds the EngineShared gate): the buffers for M inducing points and the part list; the previous
// result is forgotten
int sparse_open(mi355gp_sparse* s, int nparts, const mi355gp_part* parts, int64_t M, bool coreg) {
    HIP_CHECK(hipSetDevice(s->device));
    if (M != s->m)
        if (int rc = alloc_m(s, M)) return rc;
    s->have_result = s->winv_ok = s->svgp_result = s->pep_result = false;
    s->kmm_jitter = 1e-8;
    s->h_info[0] = s->h_info[1] = 0;
    return prepare_sparse_parts(s, nparts, parts, coreg);
}

// Starts the stream work of a call: the precision vector (nbeta = 1: beta[0] for every row, filled on the device; nbeta = n:
// per point; 0: the family has none), Z, ev[0], V = beta R (var_dtc.py:88) and Z scaled for every part
int sparse_start(mi355gp_sparse* s, const double* Z, const double* beta, long nbeta) {
    hipStream_t st = s->st;
    const long n = s->n, cnt = n * s->Dy;
    if (nbeta > 1) HIP_CHECK(hipMemcpyAsync(s->dBeta, beta, sizeof(double) * n, hipMemcpyHostToDevice, st));
    else if (nbeta == 1) hipLaunchKernelGGL(k_fill_const, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, s->dBeta, n, beta[0]);
    HIP_CHECK(hipMemcpyAsync(s->dZ, Z, sizeof(double) * s->m * s->D, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipEventRecord(s->ev[0], st));
    if (nbeta) hipLaunchKernelGGL(k_scale_rows, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, s->dY, s->dBeta, cnt, s->Dy, s->dV);
    scale_for_parts(s, s->dZ, s->m, s->mp, true);
    return 0;
}

// Ends the stream work of a call: waits for it; stage_ms (optional): [i] = ev[i] .. ev[i + 1] for i < nstage, [nstage] = the
// total.  Returns the LAPACK-style info of the call's two M x M factorisations: 0, or 1 .. M when one is not positive
// definite (the caller adds jitter), or a negative error.
int sparse_finish(mi355gp_sparse* s, int nstage, double* stage_ms) {
    HIP_CHECK(hipStreamSynchronize(s->st));
    HIP_CHECK(hipGetLastError());
    if (stage_ms) {
        float ms;
        for (int i = 0; i < nstage; ++i) {
            HIP_CHECK(hipEventElapsedTime(&ms, s->ev[i], s->ev[i + 1]));
            stage_ms[i] = ms;
        }
        HIP_CHECK(hipEventElapsedTime(&ms, s->ev[0], s->ev[nstage]));
        stage_ms[nstage] = ms;
    }
    for (int info : s->h_info)
        if (info > 0) return info > s->m ? (int)s->m : info;
    return 0;
}

// Kfu of rows [r0, r0 + rc) of X into s->Kfu (products are multiplied up in s->T).  The cross-covariance kernels write rows
// < rc, columns < m only: rows [z0, z1) of the buffer are zeroed first (z0 >= z1: nothing is).  V != NULL: where one pass can do
// both (one plain stationary part), the column partials of Kfu^T V go to s->colPart as well and their number of splits is
// returned; otherwise 0, or a negative error.
int sparse_cross_rows(mi355gp_sparse* s, long r0, long rc, long z0, long z1, const double* V) {
    const long mp = s->mp, chunk = s->chunk;
    scale_for_parts(s, s->dX + r0 * s->D, rc, chunk, false);
    if (z0 < z1) HIP_CHECK(hipMemsetAsync(s->Kfu + z0 * mp, 0, sizeof(double) * (z1 - z0) * mp, s->st));
    if (V && s->parts.size() == 1 && s->parts[0].stationary() && s->fuse_cols) {
        const SPart& pt = s->parts[0];
        const int ns = launch_kbuild_cols(s->st, pt.kp, pt.XtC, chunk, rc, pt.XtZ, mp, s->m, mp, s->Kfu, mp, V, s->Dy, s->colPart);
        if (ns > 0) return ns;
    }
    build_cross_chunk(s, rc, s->Kfu, s->T);
    return 0;
}

// zeroes what sparse_rows_gradients accumulates over the chunks of a call
int sparse_rows_gradients_reset(mi355gp_sparse* s) {
    for (SPart& p : s->parts) {
        HIP_CHECK(hipMemsetAsync(p.gradNM, 0, sizeof(double) * rec_doubles(s), s->st));
        HIP_CHECK(hipMemsetAsync(p.HX, 0, sizeof(double) * hsum_doubles(s), s->st));
        if (p.coreg()) HIP_CHECK(hipMemsetAsync(p.cgNM, 0, sizeof(double) * COREG_REC, s->st));
    }
    return 0;
}

// The other factor of part pi where its term is exactly one stationary factor times one Coregionalize factor and the pass fused
// over the two (k_grad_cols_icm) applies (grad_cols_icm_applies, the launcher's own list of conditions) and fuse_cols is on.
// -1 otherwise
static int icm_partner(const mi355gp_sparse* s, size_t pi) {
    const std::vector<int>& t = s->terms[(size_t)s->parts[pi].tix];
    if (!s->fuse_cols || t.size() != 2) return -1;
    const SPart &a = s->parts[(size_t)t[0]], &b = s->parts[(size_t)t[1]];
    if (!((a.stationary() && b.coreg()) || (a.coreg() && b.stationary()))) return -1;
    if (!grad_cols_icm_applies(s->D, (a.coreg() ? a : b).ard_in, s->mp)) return -1;      // (what the launcher itself asks)
    return (size_t)t[0] == pi ? t[1] : t[0];
}

// The row-gradient step of one chunk of rc rows (scaled into the parts' XtC): from W, the chunk's rows of dL_dKnm without the
// rank term rk, every part's theta record (added to gradNM) and H^T [X~ | 1] (added to HX), H = dL_dKnm * (dK/dr) / r.
// dL_dKnm is formed inside the gradient pass (no separate read-modify-write of the chunk).  D <= 16: the same pass also
// accumulates H^T [X~ | 1] (H stays on chip); otherwise H is written to `scratch` (rc x mp) and reduced by a second pass -- W
// itself must survive for the parts that follow.  A factor of a product sees dL_dKnm TIMES the other factors' covariance
// (prod.py:86-99): those are multiplied up in `scratch`, and form_times(), the call site's own launch, forms dL_dKnm on top.
void sparse_rows_gradients(mi355gp_sparse* s, long rc, const double* W, double* scratch, const RankTerm& rk,
                           const std::function<void()>& form_times) {
    hipStream_t st = s->st;
    const long m = s->m, mp = s->mp, chunk = s->chunk;
    const int D = s->D, groups = (D + 31) / 32;
    const long gsz = (long)rec_doubles(s);
    for (size_t pi = 0; pi < s->parts.size(); ++pi) {
        SPart& p = s->parts[pi];
        if (p.kp.kind == MI355GP_WHITE) continue;        // White: K(X, Z) = 0, no contribution (static.py:89-93)
        int nbk = 0, ns = 0;
        // a term that is exactly stationary x Coregionalize (ICM; one such term per summand of an LCM), D <= 16: both factors'
        // gradients from ONE pass over the weights (k_grad_cols_icm), made when the stationary factor comes up; fuse_cols off
        // (or a pass that does not apply) leaves both to the product route below
        const int partner = icm_partner(s, pi);
        if (partner >= 0) {
            if (p.coreg()) continue;                     // (done with its stationary partner)
            // (icm_partner has asked grad_cols_icm_applies, the launcher's own conditions: the launch is made, ns >= 1)
            SPart& c = s->parts[(size_t)partner];
            ns = launch_grad_cols_icm(st, p.kp, c.kp, p.XtC, chunk, rc, p.XtZ, mp, m, mp, c.XtC, chunk, c.XtZ, mp, W, mp, rk, s->gradPart,
                                      s->colPart, s->cgPart, &nbk);
            for (int g = 0; g < (p.kp.ard ? groups : 1); ++g)
                launch_reduce_partials(st, s->gradPart + (long)g * nbk * GP_STRIDE, nbk, GP_STRIDE, s->gradChunk + (long)g * GP_STRIDE);
            hipLaunchKernelGGL(k_vec_axpy, dim3((unsigned)((gsz + 255) / 256)), dim3(256), 0, st, p.gradNM, s->gradChunk, gsz, 1.0);
            launch_sum_splits(st, s->colPart, mp * (D + 1), ns, 1, p.HX);
            const int P2 = c.ard_in * c.ard_in;
            launch_reduce_partials(st, s->cgPart, nbk, P2, s->cgChunk);
            hipLaunchKernelGGL(k_vec_axpy, dim3(1), dim3(256), 0, st, (double*)c.cgNM, (const double*)s->cgChunk, (long)P2, 1.0);
            continue;
        }
        const bool prod = emit_other_factors(s->terms, p.tix, pi, scratch, [&](int f, double* dst, const double* mul, int, bool) {
            const SPart& pf = s->parts[(size_t)f];
            launch_kbuild_cross(st, pf.kp, pf.XtC, chunk, rc, pf.XtZ, mp, m, dst, mp, 0, 0, mul);
        });
        if (p.coreg()) {
            // the bucketed pass (k_grad_coreg) over the weights in memory -- dL_dKnm times the other factors' covariance, or
            // dL_dKnm itself formed from the rank term -- every element once; the chunk's S is the blocks' records summed in
            // block order, and the chunks are added in chunk order.  No H: gradients_X is zero (coregionalize.py:153-154)
            const double* g = W;
            if (prod) {
                form_times();
                g = scratch;
            } else if (rk.Y) {
                launch_form_rank_weights(st, W, mp, rc, m, rk, scratch);
                g = scratch;
            }
            const int P2 = p.ard_in * p.ard_in;
            const int nb = launch_grad_coreg(st, false, p.kp, p.XtC, chunk, rc, p.XtZ, mp, m, g, mp, nullptr, 0, s->cgPart);
            launch_reduce_partials(st, s->cgPart, nb, P2, s->cgChunk);
            hipLaunchKernelGGL(k_vec_axpy, dim3(1), dim3(256), 0, st, (double*)p.cgNM, (const double*)s->cgChunk, (long)P2, 1.0);
            continue;
        }
        if (p.linear()) {
            // HX = g^T x~ is all there is (k_grad_cols_lin); the theta record follows on the host (sparse_assemble_gradients).
            // A factor of a product, D > 16: the weights in memory (launch_grad returns without a launch for a kind past the
            // stationary ones when a rank term is given), then the column reduction of the stationary fallback
            if (prod) form_times();
            else if (s->fuse_cols) ns = launch_grad_cols_lin(st, p.XtC, chunk, rc, D, m, mp, W, mp, rk, s->colPart);
            const double* g = nullptr;                   // the weights in memory, where a pass needed them there
            if (ns == 0) {
                g = prod ? scratch : W;
                if (!prod && rk.Y) {
                    launch_form_rank_weights(st, W, mp, rc, m, rk, scratch);
                    g = scratch;
                }
                ns = launch_colreduce_multi(st, g, mp, rc, mp, p.XtC, 1, chunk, D, 0, s->colPart);
            }
            launch_sum_splits(st, s->colPart, mp * D, ns, 1, p.HX);
            if (s->lin_dmu) {
                // uncertain inputs: the gradient in the rows' means while the chunk's weights are hot (k_grad_rows_lin: one
                // more read of them, formed on the fly as above; where they are in memory already, the plain kernel)
                double* o = s->lin_dmu + s->lin_row0 * D;
                // (g == NULL means the fused column pass ran, which it does for D <= 16 only: the fused row kernel applies)
                if (g) launch_rows_lin_plain(st, p.XtC, chunk, rc, D, p.XtZ, mp, m, g, mp, p.dIl, s->lin_c0, o);
                else launch_grad_rows_lin(st, p.XtC, chunk, rc, D, p.XtZ, mp, m, W, mp, rk, p.dIl, s->lin_c0, o);
            }
            continue;
        }
        if (prod) {
            form_times();
            nbk = grad_generic_num_blocks(rc, m);
            launch_grad_generic(st, p.kp, p.XtC, chunk, rc, p.XtZ, mp, m, 0, scratch, mp, s->gradPart,
                                p.stationary() ? scratch : nullptr, mp);            // H over the weights, in place
            if (p.stationary()) ns = launch_colreduce_multi(st, scratch, mp, rc, mp, p.XtC, 1, chunk, D, 1, s->colPart);
        } else {
            if (p.stationary() && s->fuse_cols)
                ns = launch_grad_cols(st, p.kp, p.XtC, chunk, rc, p.XtZ, mp, m, mp, W, mp, rk, s->gradPart, s->colPart, &nbk);
            if (ns == 0) {
                nbk = grad_generic_num_blocks(rc, m);
                launch_grad_generic(st, p.kp, p.XtC, chunk, rc, p.XtZ, mp, m, 0, W, mp, s->gradPart,
                                    p.stationary() ? scratch : nullptr, mp, rk);
                if (p.stationary()) ns = launch_colreduce_multi(st, scratch, mp, rc, mp, p.XtC, 1, chunk, D, 1, s->colPart);
            }
        }
        for (int g = 0; g < (p.kp.ard ? groups : 1); ++g)
            launch_reduce_partials(st, s->gradPart + (long)g * nbk * GP_STRIDE, nbk, GP_STRIDE, s->gradChunk + (long)g * GP_STRIDE);
        // (every entry of the record: one block of 256 threads ends at dimension 239)
        hipLaunchKernelGGL(k_vec_axpy, dim3((unsigned)((gsz + 255) / 256)), dim3(256), 0, st, p.gradNM, s->gradChunk, gsz, 1.0);
        if (p.stationary()) launch_sum_splits(st, s->colPart, mp * (D + 1), ns, 1, p.HX);
    }
}

// The kernel-side gradients of a call, first half: the parts' reduction records and H^T [X~ | 1] sums on their way to the
// host (valid after the call's stream synchronisation); with_nm = false: the Kmm side only (gradMM, HZ)
int sparse_fetch_gradients(mi355gp_sparse* s, bool with_nm, KernGrads* h) {
    const size_t np_ = s->parts.size(), gsz = rec_doubles(s), hsz = hsum_doubles(s), zsz = (size_t)s->D * s->mp;
    h->with_nm = with_nm;
    h->gnm.assign(np_ * gsz, 0.0);
    h->gmm.assign(np_ * gsz, 0.0);
    h->HX.assign(np_ * hsz, 0.0);
    h->HZ.assign(np_ * hsz, 0.0);
    h->Zs.assign(np_ * zsz, 0.0);
    h->cnm.clear();
    h->cmm.clear();
    for (const SPart& p : s->parts)
        if (p.coreg() && h->cmm.empty()) {
            h->cnm.assign(np_ * COREG_REC, 0.0);
            h->cmm.assign(np_ * COREG_REC, 0.0);
        }
    for (size_t i = 0; i < np_; ++i) {
        SPart& p = s->parts[i];
        if (p.coreg()) {                                  // S of the two sides; no record of the stationary shape, no H sums
            const size_t P2 = (size_t)p.ard_in * p.ard_in;
            if (with_nm) HIP_CHECK(hipMemcpyAsync(h->cnm.data() + i * COREG_REC, p.cgNM, sizeof(double) * P2, hipMemcpyDeviceToHost, s->st));
            HIP_CHECK(hipMemcpyAsync(h->cmm.data() + i * COREG_REC, p.cgMM, sizeof(double) * P2, hipMemcpyDeviceToHost, s->st));
            continue;
        }
        if (with_nm) HIP_CHECK(hipMemcpyAsync(h->gnm.data() + i * gsz, p.gradNM, sizeof(double) * gsz, hipMemcpyDeviceToHost, s->st));
        HIP_CHECK(hipMemcpyAsync(h->gmm.data() + i * gsz, p.gradMM, sizeof(double) * gsz, hipMemcpyDeviceToHost, s->st));
        if (!p.stationary() && !p.linear()) continue;
        if (with_nm) HIP_CHECK(hipMemcpyAsync(h->HX.data() + i * hsz, p.HX, sizeof(double) * hsz, hipMemcpyDeviceToHost, s->st));
        HIP_CHECK(hipMemcpyAsync(h->HZ.data() + i * hsz, p.HZ, sizeof(double) * hsz, hipMemcpyDeviceToHost, s->st));
        HIP_CHECK(hipMemcpyAsync(h->Zs.data() + i * zsz, p.XtZ, sizeof(double) * zsz, hipMemcpyDeviceToHost, s->st));
    }
    return 0;
}

// ... second half, on the host.  dtheta_out (optional): the parts' parameter gradients, concatenated: per part the Knm and the
// Kmm record summed, part_dtheta, then update_gradients_diag: kdiag_coef = sum_n dL_dKdiag_n to the variance (stationary.py:
// 175-184, static.py:95-96; a factor of a product: times the other factors' variances, prod.py:67-71).  dZ_out (optional,
// M x D) = gradients_X(dL_dKnm^T, Z, X) + gradients_X(dL_dKmm, Z), summed over the parts (add.py:84-88):
//   sum_n H[n,m] (z~_mq - x~_nq) / l_q  +  2 sum_j Hmm[j,m] (z~_mq - z~_jq) / l_q
void sparse_assemble_gradients(const mi355gp_sparse* s, const KernGrads& h, double kdiag_coef, double* dtheta_out, double* dZ_out) {
    const size_t np_ = s->parts.size(), gsz = rec_doubles(s), hsz = hsum_doubles(s);
    const long m = s->m, mp = s->mp;
    const int D = s->D;
    if (dtheta_out) {
        double* o = dtheta_out;
        std::vector<double> ab(gsz);
        for (size_t i = 0; i < np_; ++i) {
            const double* a = h.gnm.data() + i * gsz;
            const double* b = h.gmm.data() + i * gsz;
            for (size_t k = 0; k < gsz; ++k) ab[k] = h.with_nm ? a[k] + b[k] : b[k];
            const SPart& p = s->parts[i];
            if (p.coreg()) {                             // S = S_nm + S_mm in B's order, the per-output diagonal sums on dB[a][a]
                const int P2 = p.ard_in * p.ard_in;
                const double* cn = h.cnm.data() + i * COREG_REC;
                const double* cm = h.cmm.data() + i * COREG_REC;
                for (int c = 0; c < P2; ++c) {
                    o[c] = h.with_nm ? cn[c] + cm[c] : cm[c];
                    if (!h.ddiag.empty()) o[c] += h.ddiag[(size_t)(o - dtheta_out) + c];
                }
                o += P2;
                continue;
            }
            if (p.linear() && h.with_nm) {               // the Knm record: sum_j z~_jq HX[j][q] per dimension (k_grad_cols_lin)
                const double* hx = h.HX.data() + i * hsz;
                const double* zs = h.Zs.data() + i * (size_t)D * mp;
                for (int q = 0; q < D; ++q) {
                    if (p.inv_ls[(size_t)q] == 0.0) continue;
                    double sq = 0.0;
                    for (long j = 0; j < m; ++j) sq = fma(zs[(size_t)q * mp + j], hx[j * D + q], sq);
                    ab[p.kp.ard ? (size_t)(q / 32) * GP_STRIDE + 2 + (q % 32) : 0] += sq;
                }
            }
            const int k = part_dtheta(p, ab.data(), nullptr, o);
            if (h.ddiag.empty()) o[0] = kdiag_coef * sparse_other_variances(s, i) + o[0];
            else
                for (int c = 0; c < k; ++c) o[c] += h.ddiag[(size_t)(o - dtheta_out) + c];
            o += k;
        }
    }
    if (dZ_out) {
        for (long j = 0; j < m * D; ++j) dZ_out[j] = 0.0;
        for (size_t i = 0; i < np_; ++i) {
            const SPart& p = s->parts[i];
            if (!p.stationary() && !p.linear()) continue;
            const double* hx = h.HX.data() + i * hsz;
            const double* hz = h.HZ.data() + i * hsz;
            const double* zs = h.Zs.data() + i * (size_t)D * mp;
            if (p.linear()) {                            // sqrt(variance_q) (HX + 2 HZ) (linear.py:108-114; dL_dKmm is symmetric);
                for (long j = 0; j < m; ++j)             // an inactive dimension has il = 0 and stays exactly zero
                    for (int q = 0; q < D; ++q) {
                        const double il = p.inv_ls[(size_t)q];
                        if (il == 0.0) continue;
                        dZ_out[j * D + q] += ((h.with_nm ? hx[j * D + q] : 0.0) + 2.0 * hz[j * D + q]) * il;
                    }
                continue;
            }
            for (long j = 0; j < m; ++j)
                for (int q = 0; q < D; ++q) {
                    const double il = p.inv_ls[(size_t)q];
                    if (il == 0.0) continue;
                    const double z = zs[(size_t)q * mp + j];
                    const double a = h.with_nm ? z * hx[j * (D + 1) + D] - hx[j * (D + 1) + q] : 0.0;
                    const double b = z * hz[j * (D + 1) + D] - hz[j * (D + 1) + q];
                    dZ_out[j * D + q] += (a + 2.0 * b) * il;
                }
        }
    }
}

// Prediction at Mn new points, first half: Kx = K(Z, X*) (mp x mnp, zero in the padding), with want_cov Kss = K(X*, X*), and
// the mean Kx^T wv (wv: mp x ncol) into q->Mu.  Every factor is evaluated with ITS scaling of the new inputs; products are
// multiplied up in Tmp / a second M* x M* scratch.
int sparse_newpoints(mi355gp_sparse* s, const double* Xnew, int64_t Mn, bool want_cov, const double* wv, int ncol,
                     const char* where, NewPoints* q) {
    hipStream_t st = s->st;
    const long m = s->m, mp = s->mp, mnp = round_up(Mn, NB);
    q->Mn = Mn;
    q->mnp = mnp;
    q->kdiag = s->diag_pt ? 0.0 : expression_kdiag(s->parts, s->terms);
    if (int rc = q->xs.load(st, Xnew, Mn, s->D)) return rc;
    if (s->diag_pt) {                                             // Kdiag(X*) by point, from the raw rows just uploaded
        HIP_CHECK(q->kdv.alloc(Mn));
        if (int rc = sparse_kdiag(s, q->xs.raw, Mn, nullptr, q->kdv, nullptr)) return rc;
    }
    HIP_CHECK(q->Kx.alloc(mp * mnp));
    HIP_CHECK(q->Tmp.alloc(mp * mnp));
    HIP_CHECK(q->Mu.alloc(Mn * ncol));
    HIP_CHECK(hipMemsetAsync(q->Kx, 0, sizeof(double) * mp * mnp, st));
    emit_cross(st, s->parts, s->terms, inducing_points(s), q->xs, q->Kx, mnp, q->Tmp, false, 0,
               [&](const std::vector<int>& t) { return skip_white(s, t); });
    if (want_cov) {
        HIP_CHECK(q->Kss.alloc(mnp * mnp));
        HIP_CHECK(hipMemsetAsync(q->Kss, 0, sizeof(double) * mnp * mnp, st));
        if (has_product(s->terms) && q->scr.alloc(mnp * mnp) != hipSuccess) {
            mi355gp_set_error("%s: out of memory for the product scratch", where);
            return -3;
        }
        emit_cross(st, s->parts, s->terms, q->xs, q->xs, q->Kss, mnp, q->scr, false, /*diag_same=*/1);
    }
    launch_col_reduce(st, q->Kx, mnp, m, Mn, wv, ncol, 0.0, 0, q->Mu);
    return 0;
}
// ... second half, once per Woodbury inverse: Kdiag - sum(Kx * (Winv Kx), 0) (Mn doubles), or with full_cov
// K(X*, X*) - Kx^T Winv Kx (ld mnp).  The result is in q->var: q->Var, or Kss itself when it need not be kept for another inverse.
int sparse_newpoints_var(mi355gp_sparse* s, NewPoints* q, const double* Winv, bool full_cov, bool keep_kss) {
    hipStream_t st = s->st;
    const long m = s->m, mp = s->mp, mnp = q->mnp, Mn = q->Mn;
    q->var = q->Kss;
    if (!full_cov || keep_kss) {
        if (!q->Var) HIP_CHECK(q->Var.alloc(full_cov ? mnp * mnp : Mn));
        q->var = q->Var;
    }
    launch_gemm(st, 0, 1, mp, mnp, mp, Winv, mp, q->Kx, mnp, q->Tmp, mnp, 1.0, 0.0);                   // Winv Kx
    if (!full_cov) {
        hipLaunchKernelGGL(k_col_dot, dim3((unsigned)((Mn + 63) / 64)), dim3(256), 0, st, (const double*)q->Kx, (const double*)q->Tmp,
                           mnp, m, Mn, q->kdiag, (const double*)q->kdv, q->var);
        return 0;
    }
    if (keep_kss) HIP_CHECK(hipMemcpyAsync(q->var, q->Kss, sizeof(double) * mnp * mnp, hipMemcpyDeviceToDevice, st));
    launch_gemm(st, 1, 1, mnp, mnp, mp, q->Kx, mnp, q->Tmp, mnp, q->var, mnp, -1.0, 1.0);               // K** - Kx^T Winv Kx
    return 0;
}

// ---- VarDTC -------------------------------------------------------------------------------------------------------------
// _compute_log_marginal_likelihood (var_dtc.py:264-276) and, for one noise variance (beta > 0), _compute_dL_dR (:258-261) into
// out_scalars: [0] log marginal likelihood, [1] dL/d(noise variance) (0 for per-point noise), [2] trace(A), [3] data_fit,
// [4] sum(log diag LB), [5] beta.  scal: the four sums of sparse_mm_block; kdiag: psi0_n, the same for every row; sums: {sum
// beta_n, sum log beta_n, sum beta_n |R_n|^2} over ALL shards (read for per-point noise, beta == 0, only)
// psi0 (NULL: Kdiag is the one number kdiag): {sum beta_n kd_n, sum beta_n^2 kd_n} of a per-point diagonal, which take the place
// of sum(beta) kdiag and N beta^2 kdiag
static void vardtc_scalars(const mi355gp_sparse* s, const double* scal, double kdiag, double beta, const double* sums,
                           double* out_scalars, const double* psi0 = nullptr) {
    const int Dy = s->Dy;
    const double trA = scal[0], sumAP = scal[1], logLB = scal[2], data_fit = scal[3];
    const double ng = (double)s->n_global, nd = ng * Dy;
    double lik_1, lik_2;
    if (beta == 0.0) {
        lik_1 = -0.5 * nd * log(2.0 * M_PI) + 0.5 * Dy * sums[1] - 0.5 * sums[2];
        lik_2 = -0.5 * Dy * ((psi0 ? psi0[0] : sums[0] * kdiag) - trA);
    } else {
        lik_1 = -0.5 * nd * (log(2.0 * M_PI) - log(beta)) - 0.5 * beta * s->trYYT;
        lik_2 = -0.5 * Dy * ((psi0 ? psi0[0] : beta * ng * kdiag) - trA);
    }
    const double lik_3 = -(double)Dy * logLB;
    for (int i = 0; i < MI355GP_NUM_OUT; ++i) out_scalars[i] = 0.0;
    out_scalars[0] = lik_1 + lik_2 + lik_3 + 0.5 * data_fit;
    out_scalars[2] = trA;
    out_scalars[3] = data_fit;
    out_scalars[4] = logLB;
    out_scalars[5] = beta;
    if (beta != 0.0) {
        double dL_dR = -0.5 * nd * beta + 0.5 * s->trYYT * beta * beta;
        dL_dR += 0.5 * Dy * ((psi0 ? psi0[1] : ng * kdiag * beta * beta) - trA * beta);
        dL_dR += beta * (0.5 * sumAP - data_fit);
        out_scalars[1] = dL_dR;
    }
}

// Kmm + kmm_jitter I (VarDTC: 1e-8 + extra_jitter, var_dtc.py:93-94) = sum of the parts' K(Z) (White on the diagonal),
// Lm = chol (jitchol, :95), Xm = Lm^-1, and pass 1 over the row chunks: psi2 = sum_n beta_n k_n k_n^T (heteroscedastic) or
// Kuf Kfu (then A carries beta), psi1V = Kuf V; records ev[1].
// Kmm's three steps need only Z: when the factorisation is the single persistent launch (a latency-bound chain on an otherwise
// idle GPU), they go to a side stream and pass 1 is enqueued underneath; the launch is first in line, so its workgroups are
// resident before pass 1 fills the remaining CUs.  info is read (and a called-off launch redone) after pass 1 is queued.
static int vardtc_pass1(mi355gp_sparse* s, bool het, double kmm_jitter) {
    hipStream_t st = s->st;
    const long n = s->n, m = s->m, mp = s->mp, chunk = s->chunk;
    const int Dy = s->Dy;
    const bool overlap_kmm = s->kmm_overlap && s->st_kmm && potrf_persist_eligible(mp, &s->ws);
    hipStream_t sk = overlap_kmm ? s->st_kmm : st;
    auto rebuild_kmm = [&]() { build_kmm(s, s->Lm, s->T1, kmm_jitter, /*lower_only=*/1, sk); };
    if (overlap_kmm) {
        HIP_CHECK(hipEventRecord(s->ev_z, st));
        HIP_CHECK(hipStreamWaitEvent(sk, s->ev_z, 0));
    }
    rebuild_kmm();
    s->ws.ev_persist_pre = overlap_kmm ? s->ev_z : nullptr;     // (ev_z has served its purpose: reused as "progress words zeroed")
    const int rcl = factor_launch(sk, s->Lm, s->Xm, s->Tm, nullptr, mp, &s->ws);
    s->ws.ev_persist_pre = nullptr;
    if (rcl) return rcl;
    if (!overlap_kmm) {
        if (int rc = factor_check(sk, s->Lm, s->Xm, s->Tm, nullptr, mp, &s->ws, &s->h_info[0], rebuild_kmm)) return rc;
    } else if (s->ws.persist_used) {
        // pass 1 must not take the CUs' LDS before the 155 KB workgroups of the persistent launch are in place
        HIP_CHECK(hipStreamWaitEvent(st, s->ev_z, 0));
        launch_wait_persist_resident(st, &s->ws);
    }
    HIP_CHECK(hipMemsetAsync(s->psi1Y, 0, sizeof(double) * mp * Dy, st));
    int nch = 0;
    for (long r0 = 0; r0 < n; r0 += chunk, ++nch) {
        const long rc = (n - r0 < chunk) ? (n - r0) : chunk;
        // zero only what the cross-covariance kernel leaves out: the padding columns (m < mp) of a buffer not yet zeroed or
        // holding the rows of a longer chunk, else the rows past a short chunk
        long z0 = 0, z1 = 0;
        if (m < mp) {
            if (rc < chunk || nch == 0) z1 = chunk;
        } else if (rc < chunk) {
            z0 = rc, z1 = chunk;
        }
        // one plain stationary part: K(X_chunk, Z) and the column sums of psi1^T V in ONE pass over the chunk; otherwise the
        // expression is accumulated part by part and reduced by a second pass
        const int ns_fused = sparse_cross_rows(s, r0, rc, z0, z1, s->dV + r0 * Dy);
        if (ns_fused < 0) return ns_fused;
        const double* G = s->Kfu;
        if (het) {                                            // rows scaled by sqrt(beta_n) (var_dtc.py:126-129) into T
            HIP_CHECK(hipMemsetAsync(s->T + rc * mp, 0, sizeof(double) * (round_up(rc, 16L * s->splitk) - rc) * mp, st));
            launch_rowscale_sqrt(st, s->Kfu, mp, rc, mp, s->dBeta + r0, s->T);
            G = s->T;
        }
        s->mfma_prof.begin(st, 1, (double)rc * (double)m * (double)m);            // algorithmic: the lower half of psi2
        launch_gram_splitk(st, G, mp, round_up(rc, 16L * s->splitk), mp, s->splitk, nch > 0, s->psi2part);   // rows >= rc are zero
        s->mfma_prof.end(st);
        const int ns = ns_fused > 0 ? ns_fused : launch_colreduce_multi(st, s->Kfu, mp, rc, mp, s->dV + r0 * Dy, Dy, 1, Dy, 0, s->colPart);
        launch_sum_splits(st, s->colPart, mp * Dy, ns, 1, s->psi1Y);               // psi1V += Kuf V_chunk
    }
    if (overlap_kmm) {                                          // Kmm's factorisation: long finished; join the main stream
        if (int rc = factor_check(sk, s->Lm, s->Xm, s->Tm, nullptr, mp, &s->ws, &s->h_info[0], rebuild_kmm)) return rc;
        HIP_CHECK(hipEventRecord(s->ev_kmm, sk));
        HIP_CHECK(hipStreamWaitEvent(st, s->ev_kmm, 0));
    }
    hipLaunchKernelGGL(k_sym_from_lower, grid2d(mp, mp), dim3(256), 0, st, s->psi2part, mp, s->splitk, s->psi2);
    if (sharded(s)) {                                           // the one exchange step of pass 1
        if (int rc = sparse_allreduce(s, s->psi2, (size_t)mp * mp)) return rc;
        if (int rc = sparse_allreduce(s, s->psi1Y, (size_t)mp * Dy)) return rc;
    }
    HIP_CHECK(hipEventRecord(s->ev[1], st));
    return 0;
}

// pass 2 over the same chunks: dL_dKnm = beta_n (R v^T + 2 Kfu Q2) (var_dtc.py:219,224-226,233), its theta reductions and
// H^T [X~ | 1] per part; want_rows: the per-row sums of dL_dm and of the per-point noise gradient as well
static int vardtc_pass2(mi355gp_sparse* s, bool het, bool want_rows) {
    hipStream_t st = s->st;
    const long n = s->n, m = s->m, mp = s->mp, chunk = s->chunk;
    const int Dy = s->Dy;
    const bool het_multi = het && Dy > 1, one_chunk = (n <= chunk);
    if (int rc = sparse_rows_gradients_reset(s)) return rc;
    for (long r0 = 0; r0 < n; r0 += chunk) {
        const long rc = (n - r0 < chunk) ? (n - r0) : chunk;
        const long rcp = round_up(rc, NB);
        if (!one_chunk)                                      // a single chunk is still resident from pass 1
            if (int rc2 = sparse_cross_rows(s, r0, rc, rc, chunk, nullptr)) return rc2;
        if (het_multi) {                                     // r_n = sum_j (Kfu Gr)_nj Kfu_nj, before T is needed for anything else
            launch_gemm(st, 0, 1, rcp, mp, mp, s->Kfu, mp, s->Winv, mp, s->T, mp, 1.0, 0.0);
            launch_rowdots(st, s->Kfu, s->T, mp, rc, m, s->vvec, Dy, s->dRowS + r0 * Dy, s->dRowR + r0);
        }
        s->mfma_prof.begin(st, 0, 2.0 * (double)rc * (double)m * (double)m);
        launch_gemm(st, 0, 1, rcp, mp, mp, s->Kfu, mp, s->Q2, mp, s->T, mp, 1.0, 0.0);
        s->mfma_prof.end(st);
        // per-row reductions for dL_dm = V - Kfu v (:148) and the per-point noise gradient (t_n = sum_j T_nj Kfu_nj)
        if (want_rows) launch_rowdots(st, s->Kfu, s->T, mp, rc, m, s->vvec, Dy, s->dRowS + r0 * Dy, het ? s->dRowT + r0 : nullptr);
        // the weights are T, the scratch the Kfu buffer: not needed any more for this chunk (the gradient kernels recompute
        // the covariance from the inputs)
        const RankTerm rk{s->dY + r0 * Dy, s->vvec, Dy, 1.0, 2.0, s->dBeta + r0};
        s->lin_row0 = r0;                                    // (read with lin_dmu only: a Linear part under uncertain inputs)
        sparse_rows_gradients(s, rc, s->T, s->Kfu, rk, [&]() {
            hipLaunchKernelGGL(k_form_dLdKnm_times, dim3((unsigned)rcp, (unsigned)((mp + 255) / 256)), dim3(256), 0, st, s->T, s->Kfu,
                               mp, rc, rcp, m, s->dY + r0 * Dy, s->vvec, Dy, s->dBeta + r0);
        });
    }
    if (sharded(s)) {                                           // the one exchange step of pass 2 (one buffer, one all-reduce)
        const size_t gsz = rec_doubles(s), hsz = hsum_doubles(s);
        double* rb = s->redbuf;
        for (SPart& p : s->parts) {
            HIP_CHECK(hipMemcpyAsync(rb, p.gradNM, sizeof(double) * gsz, hipMemcpyDeviceToDevice, st));
            HIP_CHECK(hipMemcpyAsync(rb + gsz, p.HX, sizeof(double) * hsz, hipMemcpyDeviceToDevice, st));
            rb += gsz + hsz;
        }
        if (int rc = sparse_allreduce(s, s->redbuf, s->parts.size() * (gsz + hsz))) return rc;
        rb = s->redbuf;
        for (SPart& p : s->parts) {
            HIP_CHECK(hipMemcpyAsync(p.gradNM, rb, sizeof(double) * gsz, hipMemcpyDeviceToDevice, st));
            HIP_CHECK(hipMemcpyAsync(p.HX, rb + gsz, sizeof(double) * hsz, hipMemcpyDeviceToDevice, st));
            rb += gsz + hsz;
        }
    }
    return 0;
}

// dL_dR per point and output column for per-point noise (var_dtc.py:240-256 AS WRITTEN there), with s_nd = k_n^T v_d,
// t_n = sum_j T_nj Kfu_nj, q_n = |Lm^-1 k_n|^2, r_n = |LB^-1 Lm^-1 k_n|^2 and the identity Dy q_n = 2 t_n + Dy r_n + sum_d s_nd^2:
//   dL_dR_nd = -b/2 + (b R_nd)^2/2 + Dy b^2 psi0/2 - b^2 t_n - (Dy - 1) b^2 r_n/2 - b^2 sum_d' s_nd'^2/2
//              - b^2 s_nd R_nd + b^2 s_nd^2/2                       (Dy = 1: the r_n and s^2 terms cancel; rowR is then empty)
// kdv (NULL: psi0 is kdiag for every row): psi0_n of a per-point diagonal
static void vardtc_dnoise_rows(long n, int Dy, double kdiag, const double* kdv, const double* hbeta, const double* Rh,
                               const std::vector<double>& rowS, const std::vector<double>& rowT, const std::vector<double>& rowR,
                               double* out) {
    for (long i = 0; i < n; ++i) {
        const double b = hbeta[i], b2 = b * b;
        double ss = 0.0;
        for (int d = 0; d < Dy; ++d) ss += rowS[(size_t)i * Dy + d] * rowS[(size_t)i * Dy + d];
        if (kdv) kdiag = kdv[i];
        const double common = -0.5 * b + 0.5 * Dy * b2 * kdiag - b2 * rowT[(size_t)i] - 0.5 * b2 * ss -
                              (rowR.empty() ? 0.0 : 0.5 * (Dy - 1) * b2 * rowR[(size_t)i]);
        for (int d = 0; d < Dy; ++d) {
            const double R = Rh[(size_t)i * Dy + d], sv = rowS[(size_t)i * Dy + d];
            out[i * Dy + d] = common + 0.5 * b2 * R * R - b2 * sv * R + 0.5 * b2 * sv * sv;
        }
    }
}

// One SparseGP.parameters_changed for a SUM of kernels, scalar or per-point noise and R = Y - mean (see mi355gp.h), as
// VarDTC.inference reads: pass 1 (the psi statistics of certain inputs), the M x M algebra, pass 2 (dL_dKnm and what the
// kernels make of it), the Kmm gradients, the scalars.  out_scalars: see vardtc_scalars.
int mi355gp_vardtc_inference_sum(mi355gp_sparse* s, int nparts, const mi355gp_part* parts, const double* Z, int64_t M,
                                 const double* noise, int64_t noise_len, double extra_jitter, double* out_scalars,
                                 double* dtheta_out, double* dZ_out, double* wv_out, double* dnoise_rows_out,
                                 double* dLdm_out, double* stage_ms) {
    ARG_CHECK(s && s->n > 0, "mi355gp_vardtc_inference: set_data first");
    ARG_CHECK(parts && Z && M > 0 && out_scalars && noise, "mi355gp_vardtc_inference: bad arguments");
    ARG_CHECK(noise_len == 1 || noise_len == s->n, "noise must have 1 or N entries");
    const bool het = noise_len > 1;
    ARG_CHECK(!het || dnoise_rows_out, "per-point noise: dnoise_rows_out (N x Dy) is required");
    EngineShared gate(s->device);
    if (int rc = sparse_open(s, nparts, parts, M, /*coreg=*/true)) return rc;
    if (int rc = coreg_check_points(s, Z, M, "inducing")) return rc;       // (X's: prepare_sparse_parts; no kernel has run yet)
    const long n = s->n;
    // per-point precision beta_n = 1 / max(noise_n, 1e-8) (var_dtc.py:78-80)
    // (scalar noise: the three sums are closed forms -- unused by the homoscedastic formulas -- and the precision vector is filled on
    //  the device: the N-element host loop with its logarithms and the 1.6 MB upload cost ~1 ms per evaluation at N = 200000)
    std::vector<double> hbeta(het ? (size_t)n : (size_t)1);
    double glob[3] = {0.0, 0.0, 0.0};                            // sum beta_n, sum log beta_n, sum beta_n |R_n|^2
    if (het) {
        for (long i = 0; i < n; ++i) {
            const double b = 1.0 / fmax(noise[i], 1e-8);
            hbeta[(size_t)i] = b;
            glob[0] += b;
            glob[1] += log(b);
            glob[2] += b * s->rowYY[(size_t)i];
        }
    } else {
        hbeta[0] = 1.0 / fmax(noise[0], 1e-8);
        glob[0] = hbeta[0] * (double)n;
        glob[1] = log(hbeta[0]) * (double)n;
        glob[2] = hbeta[0] * s->trYYT_local;
    }
    return vardtc_evaluate(s, Z, hbeta, glob, 1e-8 + extra_jitter, out_scalars, dtheta_out, dZ_out, wv_out, dnoise_rows_out, dLdm_out,
                           stage_ms);
}

}  // extern "C"

// The evaluation itself, for a call that sparse_open has opened: hbeta = the precisions (one for every row, or n), glob =
// {sum beta_n, sum log beta_n, sum beta_n |R_n|^2} of this shard, kmm_jitter = the whole term on Kmm's diagonal.  The targets
// are the context's (dY, rowYY, trYYT).  EPDTC (epdtc.hip) evaluates its converged sites through it.
int vardtc_evaluate(mi355gp_sparse* s, const double* Z, const std::vector<double>& hbeta, double (&glob)[3], double kmm_jitter,
                    double* out_scalars, double* dtheta_out, double* dZ_out, double* wv_out, double* dnoise_rows_out,
                    double* dLdm_out, double* stage_ms) {
    hipStream_t st = s->st;
    const long n = s->n, m = s->m;
    const int Dy = s->Dy;
    const bool het = hbeta.size() > 1;
    const double beta = het ? 0.0 : hbeta[0];
    s->beta_scalar = beta;
    s->mfma_prof.on = true;
    s->mfma_prof.mask = 0x3u;
    s->mfma_prof.reset();
    if (int rc = sparse_start(s, Z, hbeta.data(), (long)hbeta.size())) return rc;
    // a per-point diagonal: psi0_n = Kdiag(x_n) and its sums against w_n = beta_n -- sum beta kd, sum beta^2 kd and the
    // update_gradients_diag sums (dL_dKdiag_n = -Dy beta_n / 2, sparse_gp.py:110)
    std::vector<double> dsums, kdh;
    if (s->diag_pt)
        if (int rc = sparse_kdiag_data(s, s->dBeta, &dsums)) return rc;
    int inject = 0;                                            // fault injection for the tests: 1 / 2 hit Kmm's launch, 11 / 12 B's
    {
        const char* et = DIAG_ENV("SPARSE_PERSIST_TEST");
        if (et && *et) inject = atoi(et);
    }
    if (inject == 1 || inject == 2) s->ws.persist_test = inject, s->ws.persist_skip = 0;
    const bool want_rows = het || dLdm_out != nullptr;
    if (int rc = vardtc_pass1(s, het, kmm_jitter)) return rc;
    if (int rc = sparse_mm_block(s, het, beta, inject)) return rc;
    if (int rc = vardtc_pass2(s, het, want_rows)) return rc;
    sparse_kmm_gradients(s);
    HIP_CHECK(hipEventRecord(s->ev[3], st));
    // ---- small results to the host -------------------------------------------------------------------------------------
    KernGrads kg;
    std::vector<double> rowS, rowT, rowR, Rh;
    double scal[8];
    if (int rc = sparse_fetch_gradients(s, true, &kg)) return rc;
    HIP_CHECK(hipMemcpyAsync(scal, s->scal, sizeof(double) * 4, hipMemcpyDeviceToHost, st));
    if (wv_out) HIP_CHECK(hipMemcpyAsync(wv_out, s->vvec, sizeof(double) * m * Dy, hipMemcpyDeviceToHost, st));
    if (want_rows) {
        rowS.resize((size_t)n * Dy);
        HIP_CHECK(hipMemcpyAsync(rowS.data(), s->dRowS, sizeof(double) * n * Dy, hipMemcpyDeviceToHost, st));
        if (het) {
            rowT.resize((size_t)n);
            HIP_CHECK(hipMemcpyAsync(rowT.data(), s->dRowT, sizeof(double) * n, hipMemcpyDeviceToHost, st));
            if (Dy > 1) {
                rowR.resize((size_t)n);
                HIP_CHECK(hipMemcpyAsync(rowR.data(), s->dRowR, sizeof(double) * n, hipMemcpyDeviceToHost, st));
            }
            if (s->diag_pt) {
                kdh.resize((size_t)n);
                HIP_CHECK(hipMemcpyAsync(kdh.data(), s->dKd, sizeof(double) * n, hipMemcpyDeviceToHost, st));
            }
        }
    }
    if (int rc = sparse_finish(s, 3, stage_ms)) return rc;      // (info > 0: Kmm or B not positive definite, the caller adds jitter)
    if (sharded(s)) {                                           // sums over ALL shards of the per-point quantities
        HIP_CHECK(hipMemcpy(s->scal + 4, glob, sizeof(glob), hipMemcpyHostToDevice));
        if (int rc = sparse_allreduce(s, s->scal + 4, 3)) return rc;
        HIP_CHECK(hipStreamSynchronize(st));
        HIP_CHECK(hipMemcpy(glob, s->scal + 4, sizeof(glob), hipMemcpyDeviceToHost));
    }
    // psi0_n = Kdiag of the expression: one number, or by point (then the two sums of the record stand in for it)
    const double kdiag = s->diag_pt ? 0.0 : expression_kdiag(s->parts, s->terms);
    vardtc_scalars(s, scal, kdiag, beta, glob, out_scalars, s->diag_pt ? dsums.data() : nullptr);
    if (want_rows) {
        Rh.resize((size_t)n * Dy);
        HIP_CHECK(hipMemcpy(Rh.data(), s->dY, sizeof(double) * n * Dy, hipMemcpyDeviceToHost));
    }
    if (het) vardtc_dnoise_rows(n, Dy, kdiag, s->diag_pt ? kdh.data() : nullptr, hbeta.data(), Rh.data(), rowS, rowT, rowR, dnoise_rows_out);
    if (dLdm_out)                                                // dL_dm = V - Kfu v (var_dtc.py:148)
        for (long i = 0; i < n; ++i)
            for (int d = 0; d < Dy; ++d) dLdm_out[i * Dy + d] = hbeta[het ? (size_t)i : (size_t)0] * Rh[(size_t)i * Dy + d] - rowS[(size_t)i * Dy + d];
    // update_gradients_diag(dL_dKdiag = -0.5 Dy beta_n) (sparse_gp.py:110)
    if (s->diag_pt) sparse_diag_dtheta(s, dsums, -0.5 * Dy, &kg.ddiag);
    sparse_assemble_gradients(s, kg, -0.5 * Dy * glob[0], dtheta_out, dZ_out);
    s->have_result = true;
    s->uncertain_result = false;
    return 0;
}

extern "C" {

int mi355gp_vardtc_inference(mi355gp_sparse* s, int kind, int ard, const double* theta, const double* Z, int64_t M,
                             double noise_var, double extra_jitter, double* out_scalars, double* dtheta_out,
                             double* dZ_out, double* wv_out, double* stage_ms) {
    if (int rc = check_kind(kind, KS_STATIONARY, "mi355gp_vardtc_inference")) return rc;
    ARG_CHECK(theta, "mi355gp_vardtc_inference: theta is NULL");
    const mi355gp_part part{kind, ard, 0, nullptr, theta, 0};
    return mi355gp_vardtc_inference_sum(s, 1, &part, Z, M, &noise_var, 1, extra_jitter, out_scalars, dtheta_out, dZ_out, wv_out,
                                        nullptr, nullptr, stage_ms);
}

// ---- VarDTC with uncertain inputs -----------------------------------------------------------------------------------------
// out = scale * (A + A^T) / 2 over the leading m x m of mp x mp matrices, 0 in the padding (rbf_psi_comp.py:109)
__global__ void k_sym_scaled(const double* __restrict__ A, long mp, long m, double scale, double* __restrict__ out) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= mp) return;
    out[i * mp + j] = (i < m && j < m) ? 0.5 * scale * (A[i * mp + j] + A[j * mp + i]) : 0.0;
}

// The psi kernels' operands and partial sums for one call: a_q = 1 / l_q^2 (0 on a dimension the RBF part does not see), Z zero
// padded to mpad x Qp, the per-chunk row records and the sums the two passes leave behind
struct PsiWork {
    bool ss = false;                        // spike-and-slab inputs (s->dGam): the kernels and layouts of psi_ss.hip
    int Qp = 0, RL = 0, ZL = 0;             // doubles of one row record and of one inducing point's Z sums
    long mpad = 0, ld2 = 0, mt = 0, chunk = 0;
    double var = 0.0;                       // the RBF part's variance
    std::vector<double> ha, hzp, sums;      // a_q; padded Z; [0] the variance record, [1 + q] the lengthscale sums of psi1 and psi2
    DevBuf dA, dZp, dEp, rd1, rd2, lg1, lg2, Ppart, P1s, P2s, Zpart, Zs1, Zs2, dMuO, dSO, dGO, rowrec, rec, zz;
    // Bias parts (b > 0, mi355gp_sparse_set_psi_lin_bias): the column sums c of the RBF part's psi1 (mp), of V (Dy),
    // t = 2 rowsum(dL_dpsi2) (m), b t (m) and the RBF part's own psi2 (mp x mp: s->psi2 then holds the expression's) -- the
    // context's buffers (biasC ...), kept between calls
    double b = 0.0;
    double *csum = nullptr, *vsum = nullptr, *tvec = nullptr, *addv = nullptr, *psi2rbf = nullptr;
};

static int psi_work_setup(mi355gp_sparse* s, const SPart& rbf, const double* Z, PsiWork* w) {
    const long n = s->n, m = s->m;
    const int D = s->D, Qp = psi_qp(D);
    w->Qp = Qp;
    w->RL = w->ss ? PSS_RL(Qp) : 1 + 2 * Qp;
    w->ZL = w->ss ? PSS_NZ * Qp : Qp;
    w->var = rbf.kp.variance;
    w->mpad = round_up(m, PSI_KT);
    w->ld2 = round_up(m, PSI_T2);
    w->mt = (m + 15) / 16;
    w->chunk = n < PSI_CHUNK ? n : PSI_CHUNK;
    const long chunk = w->chunk, mpad = w->mpad, nzb = (chunk + PSI_GROWS - 1) / PSI_GROWS;
    std::vector<double>& hzp = w->hzp;
    hzp.assign((size_t)mpad * Qp, 0.0);
    w->ha.assign((size_t)Qp, 0.0);
    w->sums.assign((size_t)(1 + Qp), 0.0);
    for (int q = 0; q < D; ++q) w->ha[(size_t)q] = rbf.inv_ls[(size_t)q] * rbf.inv_ls[(size_t)q];
    for (long i = 0; i < m; ++i)
        for (int q = 0; q < D; ++q) hzp[(size_t)i * Qp + q] = Z[i * D + q];
    HIP_CHECK(w->dA.alloc(Qp));
    HIP_CHECK(w->dZp.alloc(hzp.size()));
    HIP_CHECK(w->rd1.alloc((w->ss ? 4 : 2) * chunk * Qp));
    HIP_CHECK(w->rd2.alloc((w->ss ? 4 : 2) * chunk * Qp));
    if (!w->ss) {                                                 // (the spike-and-slab records carry their prefactors)
        HIP_CHECK(w->lg1.alloc(chunk));
        HIP_CHECK(w->lg2.alloc(chunk));
    }
    HIP_CHECK(w->Ppart.alloc((size_t)w->mt * chunk * w->RL));
    HIP_CHECK(w->P1s.alloc((size_t)chunk * w->RL));
    HIP_CHECK(w->P2s.alloc((size_t)chunk * w->RL));
    HIP_CHECK(w->Zpart.alloc((size_t)nzb * mpad * w->ZL));
    HIP_CHECK(w->Zs1.alloc((size_t)mpad * w->ZL));
    HIP_CHECK(w->Zs2.alloc((size_t)mpad * w->ZL));
    HIP_CHECK(w->dMuO.alloc(n * D));
    HIP_CHECK(w->dSO.alloc(n * D));
    HIP_CHECK(w->rowrec.alloc((size_t)chunk * (1 + Qp)));
    HIP_CHECK(w->rec.alloc(1 + Qp));
    if (!w->ss) HIP_CHECK(w->zz.alloc((size_t)m * 2 * Qp));      // (spike-and-slab: the z_m - z_o sums come from the gradient kernel)
    HIP_CHECK(hipMemcpyAsync(w->dA, w->ha.data(), sizeof(double) * Qp, hipMemcpyHostToDevice, s->st));
    HIP_CHECK(hipMemcpyAsync(w->dZp, hzp.data(), sizeof(double) * hzp.size(), hipMemcpyHostToDevice, s->st));
    HIP_CHECK(hipMemsetAsync(w->Zpart, 0, sizeof(double) * nzb * mpad * w->ZL, s->st));   // the kernels write rows < round_up(m, 16) only
    if (w->ss) {
        HIP_CHECK(w->dEp.alloc(hzp.size()));
        HIP_CHECK(w->dGO.alloc(n * D));
        launch_pss_e(s->st, w->dZp, w->dA, mpad, Qp, w->dEp);
    }
    return 0;
}

// Kmm, Lm, Xm as for certain inputs, on the main stream; pass 1 over chunks of PSI_CHUNK rows: psi1 chunk (in the Kfu buffer,
// ld mp) -> psi1^T V, psi2 += the chunk's sum (fixed order); records ev[1]
// With Bias parts (w.b > 0): psi1 = psi1_rbf + b, so psi1^T V gains b colsum(V) and psi2 gains b (c 1^T + 1 c^T) + N b^2 with
// c = colsum(psi1_rbf), summed per chunk in chunk order; the Kfu buffer keeps the RBF part's psi1 alone
static int uncertain_pass1(mi355gp_sparse* s, PsiWork& w, double extra_jitter, bool want_psi2 = true) {
    hipStream_t st = s->st;
    const long n = s->n, m = s->m, mp = s->mp;
    const int D = s->D, Dy = s->Dy;
    auto rebuild_kmm = [&]() { build_kmm(s, s->Lm, s->T1, 1e-8 + extra_jitter, /*lower_only=*/1, st); };
    rebuild_kmm();
    if (int rc = potrf_checked(st, s->Lm, s->Xm, s->Tm, nullptr, mp, &s->ws, &s->h_info[0], rebuild_kmm)) return rc;
    HIP_CHECK(hipMemsetAsync(s->psi1Y, 0, sizeof(double) * mp * Dy, st));
    HIP_CHECK(hipMemsetAsync(s->psi2, 0, sizeof(double) * mp * mp, st));
    int nch = 0;
    for (long r0 = 0; r0 < n; r0 += PSI_CHUNK, ++nch) {
        const long rc = (n - r0 < PSI_CHUNK) ? (n - r0) : PSI_CHUNK;
        if (w.ss) launch_pss_rows(st, s->dX + r0 * D, s->dSvar + r0 * D, s->dGam + r0 * D, w.dA, rc, D, w.Qp, w.rd1, w.rd2);
        else launch_psi_rows(st, s->dX + r0 * D, s->dSvar + r0 * D, w.dA, rc, D, w.Qp, w.rd1, w.rd2, w.lg1, w.lg2);
        HIP_CHECK(hipMemsetAsync(s->Kfu, 0, sizeof(double) * rc * mp, st));          // psi1 writes columns < m only
        if (w.ss) launch_pss_psi1(st, w.rd1, w.dZp, w.dEp, rc, m, w.mpad, w.Qp, w.var, s->Kfu, mp);
        else launch_psi1(st, w.rd1, w.lg1, w.dZp, rc, m, w.mpad, w.Qp, w.var, s->Kfu, mp);
        const int nsc = launch_colreduce_multi(st, s->Kfu, mp, rc, mp, s->dV + r0 * Dy, Dy, 1, Dy, 0, s->colPart);
        launch_sum_splits(st, s->colPart, mp * Dy, nsc, 1, s->psi1Y);                 // psi1^T V += psi1_chunk^T V_chunk
        if (w.b > 0.0) {                                                              // c += the chunk's column sums of psi1
            const int nso = launch_colreduce_multi(st, s->Kfu, mp, rc, mp, nullptr, 0, 0, 0, 1, s->colPart);
            launch_sum_splits(st, s->colPart, mp, nso, nch > 0, w.csum);
        }
        if (!want_psi2) continue;                                                     // (missing data: psi2 per group, by the caller)
        const int ns = w.ss ? launch_pss_psi2(st, w.rd2, nullptr, w.dZp, w.dEp, w.dA, rc, m, w.Qp, w.var * w.var, w.ld2, s->psi2part)
                            : launch_psi2(st, w.rd2, w.lg2, nullptr, w.dZp, w.dA, rc, m, w.Qp, w.var * w.var, w.ld2, s->psi2part);
        launch_psi2_combine(st, s->psi2part, w.ld2, m, ns, nch > 0, s->psi2, mp);
    }
    if (w.b > 0.0) {
        HIP_CHECK(hipMemcpyAsync(w.psi2rbf, s->psi2, sizeof(double) * mp * mp, hipMemcpyDeviceToDevice, st));
        launch_psi2_bias_add(st, s->psi2, mp, m, w.csum, w.b, (double)n * w.b * w.b);
        const int nsv = launch_colreduce_multi(st, s->dV, Dy, n, Dy, nullptr, 0, 0, 0, 1, s->colPart);   // colsum(V), Dy numbers
        launch_sum_splits(st, s->colPart, Dy, nsv, 0, w.vsum);
        launch_psi1y_bias_add(st, s->psi1Y, m, Dy, w.vsum, w.b);
    }
    HIP_CHECK(hipEventRecord(s->ev[1], st));
    return 0;
}

// pass 2, the chain rule through psi1 and psi2: the psi1 / psi2 gradient kernels with dL_dpsi1 = beta R v^T formed on the fly
// and dL_dpsi2 = beta Q2 symmetrised (in E; LS = dL_dpsi2 * psi2 carries the z_m - z_o terms); leaves dmu / dS per row, the Z
// sums (Zs1, Zs2, zz) and, on the host, w.sums
static int uncertain_pass2(mi355gp_sparse* s, PsiWork& w, double beta) {
    hipStream_t st = s->st;
    const long n = s->n, m = s->m, mp = s->mp;
    const int D = s->D, Dy = s->Dy, Qp = w.Qp;
    hipLaunchKernelGGL(k_sym_scaled, grid2d(mp, mp), dim3(256), 0, st, s->Q2, mp, m, beta, s->E);
    if (!w.ss) launch_psi2_zz(st, s->E, w.b > 0.0 ? (const double*)w.psi2rbf : (const double*)s->psi2, mp, w.dZp, m, Qp, w.zz);
    if (w.b > 0.0) {                                           // Bias parts: dL_dpsi1 of the RBF part gains b t^T, t = 2 rowsum(E)
        launch_mm_colsums(st, s->E, mp, m, 2.0, w.tvec);
        launch_mm_colsums(st, s->E, mp, m, 2.0 * w.b, w.addv);
    }
    const double* add = w.b > 0.0 ? w.addv : nullptr;
    std::vector<double> csum((size_t)(1 + Qp));
    int nch = 0;
    for (long r0 = 0; r0 < n; r0 += PSI_CHUNK, ++nch) {
        const long rc = (n - r0 < PSI_CHUNK) ? (n - r0) : PSI_CHUNK;
        const int nb = (int)((rc + PSI_GROWS - 1) / PSI_GROWS);
        const PsiRank rk{s->dY + r0 * Dy, s->vvec, Dy, beta};
        if (w.ss) {
            launch_pss_rows(st, s->dX + r0 * D, s->dSvar + r0 * D, s->dGam + r0 * D, w.dA, rc, D, Qp, w.rd1, w.rd2);
            launch_pss_psi1_grad(st, w.rd1, w.dZp, w.dEp, nullptr, 0, rk, rc, m, w.mpad, Qp, w.var, w.Ppart, w.Zpart);
        } else {
            launch_psi_rows(st, s->dX + r0 * D, s->dSvar + r0 * D, w.dA, rc, D, Qp, w.rd1, w.rd2, w.lg1, w.lg2);
            launch_psi1_grad(st, w.rd1, w.lg1, w.dZp, nullptr, 0, rk, rc, m, w.mpad, Qp, w.var, w.Ppart, w.Zpart, add);
        }
        launch_sum_splits(st, w.Ppart, rc * w.RL, (int)w.mt, 0, w.P1s);
        launch_sum_splits(st, w.Zpart, w.mpad * w.ZL, nb, nch > 0, w.Zs1);
        if (w.ss) launch_pss_psi2_grad(st, w.rd2, nullptr, w.dZp, w.dEp, w.dA, s->E, mp, rc, m, w.mpad, Qp, w.var * w.var, w.Ppart, w.Zpart);
        else launch_psi2_grad(st, w.rd2, w.lg2, nullptr, w.dZp, w.dA, s->E, mp, rc, m, w.mpad, Qp, w.var * w.var, w.Ppart, w.Zpart);
        launch_sum_splits(st, w.Ppart, rc * w.RL, (int)w.mt, 0, w.P2s);
        launch_sum_splits(st, w.Zpart, w.mpad * w.ZL, nb, nch > 0, w.Zs2);
        if (w.ss)
            launch_pss_rowfinish(st, w.P1s, w.P2s, s->dSvar + r0 * D, s->dGam + r0 * D, w.dA, rc, D, Qp, w.dMuO + r0 * D, w.dSO + r0 * D,
                                 w.dGO + r0 * D, w.rowrec);
        else launch_psi_rowfinish(st, w.P1s, w.P2s, s->dSvar + r0 * D, w.dA, rc, D, Qp, w.dMuO + r0 * D, w.dSO + r0 * D, w.rowrec);
        launch_reduce_partials(st, w.rowrec, (int)rc, 1 + Qp, w.rec);
        HIP_CHECK(hipMemcpyAsync(csum.data(), w.rec, sizeof(double) * (1 + Qp), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        for (int k = 0; k <= Qp; ++k) w.sums[(size_t)k] += csum[(size_t)k];           // chunks in row order
    }
    return 0;
}

// The expressions the uncertain-input entry points take, checked before any device work.  By default one RBF part and White
// parts; on a context that was asked to (mi355gp_sparse_set_psi_lin_bias) ONE input-dependent part, RBF or Linear, with Bias
// and White parts.  irbf_out: the index of that part.
static int uncertain_check_parts(const mi355gp_sparse* s, int nparts, const mi355gp_part* parts, int64_t M, int* irbf_out,
                                 const char* where = "mi355gp_vardtc_inference_uncertain", bool ss = false) {
    int irbf = -1;
    if (s->take_psi_lin && !ss) {                                  // (spike-and-slab inputs: one RBF part and White parts on every context)
        for (int i = 0; i < nparts; ++i) {
            if (parts[i].term != 0) PART_FAIL("%s: part %d is a factor of a product; products have no psi statistics here", where, i);
            if (parts[i].kind == MI355GP_WHITE || parts[i].kind == MI355GP_BIAS) continue;
            if (parts[i].kind != MI355GP_RBF && parts[i].kind != MI355GP_LINEAR)
                PART_FAIL("%s: part %d is a %s (kind %d) part; uncertain inputs take one RBF or Linear part with Bias and White parts "
                          "only", where, i, kind_name(parts[i].kind), parts[i].kind);
            if (irbf >= 0)
                PART_FAIL("%s: parts %d (%s) and %d (%s) are both input-dependent; uncertain inputs take ONE RBF or Linear part (psi2 "
                          "of two has cross terms that need E[k1 k2^T]), with Bias and White parts", where, irbf,
                          kind_name(parts[irbf].kind), i, kind_name(parts[i].kind));
            irbf = i;
        }
        if (irbf < 0) PART_FAIL("%s: no RBF or Linear part; uncertain inputs take one RBF or Linear part with Bias and White parts", where);
        if (s->D > PSI_QMAX) PART_FAIL("%s: the psi-statistics kernels take at most 64 input dimensions", where);
        if (M > PSI_MMAX) PART_FAIL("%s: the psi-statistics kernels take at most 65535 inducing points", where);
        *irbf_out = irbf;
        return 0;
    }
    for (int i = 0; i < nparts; ++i) {
        if (parts[i].term != 0) PART_FAIL("%s: part %d is a factor of a product; products have no psi statistics here", where, i);
        if (parts[i].kind == MI355GP_WHITE) continue;
        if (parts[i].kind != MI355GP_RBF)
            PART_FAIL("%s: part %d is a %s (kind %d) part; uncertain inputs take one RBF part and White parts only%s", where, i,
                      kind_name(parts[i].kind), parts[i].kind,
                      (!ss && (parts[i].kind == MI355GP_BIAS || parts[i].kind == MI355GP_LINEAR))
                          ? " (Bias and Linear: ask the context with mi355gp_sparse_set_psi_lin_bias)" : "");
        if (irbf >= 0) PART_FAIL("%s: parts %d and %d are both RBF; uncertain inputs take ONE RBF part (and White parts)", where, irbf, i);
        irbf = i;
    }
    if (irbf < 0) PART_FAIL("%s: no RBF part; uncertain inputs take one RBF part and White parts only", where);
    if (s->D > PSI_QMAX) PART_FAIL("%s: the psi-statistics kernels take at most 64 input dimensions", where);
    if (M > PSI_MMAX) PART_FAIL("%s: the psi-statistics kernels take at most 65535 inducing points", where);
    *irbf_out = irbf;
    return 0;
}

// b = the sum of the Bias parts' variances of the call's expression (0: none)
static double bias_sum(const mi355gp_sparse* s) {
    double b = 0.0;
    for (const SPart& p : s->parts)
        if (p.kp.kind == MI355GP_BIAS) b += p.kp.variance;
    return b;
}

struct LinDmuScope {           // sparse_rows_gradients writes row gradients only inside the call that asked for them
    mi355gp_sparse* s;
    ~LinDmuScope() { s->lin_dmu = nullptr; }
};

// The uncertain-input evaluation of an opened call whose input-dependent part is Linear (part ilin), with Bias (b) and White
// parts.  The statistics are the certain-input ones at X = mu plus terms of size M or D:
//   psi1 = K(mu, Z) of the expression,  psi2 = sum_n k_n k_n^T + Zv diag(s) Zv^T,  psi0_n = sum_q v_q (mu_nq^2 + S_nq) + b + w
// (Zv = Z diag(v), s_q = sum_n S_nq), so the two passes are vardtc_pass1 / vardtc_pass2 over the resident means; on top of them
// the rank-D term of psi2, the row gradient k_grad_rows_lin inside pass 2, and with E = beta sym(Q2), ze = diag(Z^T E Z):
//   dS_nq = v_q^2 ze_q + dpsi0 v_q,  dZ += v^2 s (2 E Z),  dv_q += 2 v_q s_q ze_q + dpsi0 (sum_n mu_nq^2 + s_q)
static int vardtc_uncertain_linear(mi355gp_sparse* s, int ilin, const double* Z, double beta, double extra_jitter,
                                   double* out_scalars, double* dtheta_out, double* dZ_out, double* wv_out, double* dmu_out,
                                   double* dS_out, double* stage_ms) {
    hipStream_t st = s->st;
    const long n = s->n, m = s->m, mp = s->mp;
    const int D = s->D, Dy = s->Dy;
    const double dpsi0 = -0.5 * Dy * beta;
    s->mfma_prof.on = true;
    s->mfma_prof.mask = 0x3u;
    s->mfma_prof.reset();
    const SPart& lin = s->parts[(size_t)ilin];
    HIP_CHECK(s->linDmu.need((size_t)n * D));
    HIP_CHECK(s->linEZ.need((size_t)m * D));
    double *dMuO = s->linDmu, *dEZ = s->linEZ;
    HIP_CHECK(s->diagPart.need((size_t)kdiag_blocks(n) * 2 * D));
    HIP_CHECK(s->diagSums.need((size_t)2 * D));
    if (int rc = sparse_start(s, Z, &beta, 1)) return rc;
    launch_kdiag_var_sums(st, s->dX, s->dSvar, n, D, s->diagPart, s->diagSums);       // s_q and sum_n mu_nq^2
    if (int rc = vardtc_pass1(s, false, 1e-8 + extra_jitter)) return rc;
    launch_psi2_rank_add(st, s->dZ, lin.dIl, s->diagSums, m, D, s->psi2, mp);
    if (int rc = sparse_mm_block(s, false, beta, 0)) return rc;
    hipLaunchKernelGGL(k_sym_scaled, grid2d(mp, mp), dim3(256), 0, st, s->Q2, mp, m, beta, s->E);
    launch_mm_times_z(st, s->E, mp, s->dZ, m, D, dEZ);
    {
        LinDmuScope scope{s};
        s->lin_dmu = dMuO;
        s->lin_c0 = 2.0 * dpsi0;
        if (int rc = vardtc_pass2(s, false, false)) return rc;
    }
    sparse_kmm_gradients(s);
    HIP_CHECK(hipEventRecord(s->ev[3], st));
    // ---- small results to the host -----------------------------------------------------------------------------------------
    KernGrads kg;
    std::vector<double> ez((size_t)m * D), cs((size_t)2 * D), hz((size_t)m * D);
    double scal[8];
    if (int rc = sparse_fetch_gradients(s, true, &kg)) return rc;
    HIP_CHECK(hipMemcpyAsync(ez.data(), dEZ, sizeof(double) * m * D, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(cs.data(), s->diagSums, sizeof(double) * 2 * D, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(hz.data(), s->dZ, sizeof(double) * m * D, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(scal, s->scal, sizeof(double) * 4, hipMemcpyDeviceToHost, st));
    if (wv_out) HIP_CHECK(hipMemcpyAsync(wv_out, s->vvec, sizeof(double) * m * Dy, hipMemcpyDeviceToHost, st));
    if (dmu_out) HIP_CHECK(hipMemcpyAsync(dmu_out, dMuO, sizeof(double) * n * D, hipMemcpyDeviceToHost, st));
    if (int rc = sparse_finish(s, 3, stage_ms)) return rc;
    std::vector<double> v((size_t)D), ze((size_t)D, 0.0);
    double psi0sum = 0.0;
    for (int q = 0; q < D; ++q) {
        v[(size_t)q] = lin.inv_ls[(size_t)q] * lin.inv_ls[(size_t)q];
        for (long j = 0; j < m; ++j) ze[(size_t)q] = fma(hz[(size_t)(j * D + q)], ez[(size_t)(j * D + q)], ze[(size_t)q]);
        psi0sum = fma(v[(size_t)q], cs[(size_t)(D + q)] + cs[(size_t)q], psi0sum);
    }
    for (const SPart& p : s->parts)
        if (!p.linear()) psi0sum += (double)n * p.kp.variance;           // Bias and White: their variance at every row
    const double psi0[2] = {beta * psi0sum, beta * beta * psi0sum};
    vardtc_scalars(s, scal, 0.0, beta, nullptr, out_scalars, psi0);
    // update_gradients_expectations through psi0 (every part) and the rank-D term of psi2 (the Linear part), in theta order
    for (const SPart& p : s->parts) {
        const size_t o = kg.ddiag.size();
        kg.ddiag.resize(o + p.theta.size(), 0.0);
        double* g = kg.ddiag.data() + o;
        if (!p.linear()) {
            g[0] = dpsi0 * (double)n;
            continue;
        }
        for (size_t a = 0; a < p.dims.size(); ++a) {
            const size_t q = (size_t)p.dims[a];
            g[p.kp.ard ? a : 0] += 2.0 * v[q] * cs[q] * ze[q] + dpsi0 * (cs[(size_t)D + q] + cs[q]);
        }
    }
    sparse_assemble_gradients(s, kg, 0.0, dtheta_out, dZ_out);
    if (dZ_out)
        for (long j = 0; j < m; ++j)
            for (int q = 0; q < D; ++q) dZ_out[j * D + q] += v[(size_t)q] * v[(size_t)q] * cs[(size_t)q] * 2.0 * ez[(size_t)(j * D + q)];
    if (dS_out)
        for (long i = 0; i < n; ++i)
            for (int q = 0; q < D; ++q) dS_out[i * D + q] = fma(v[(size_t)q] * v[(size_t)q], ze[(size_t)q], dpsi0 * v[(size_t)q]);
    s->have_result = true;
    s->uncertain_result = true;
    return 0;
}

// The uncertain-input evaluation of an opened call whose input-dependent part is the RBF part irbf: sparse_start, pass 1, the
// M x M block, pass 2, the results.  ss: the inputs are spike-and-slab (s->dGam; no Bias parts then) and dgamma_out (optional,
// N x D) takes the gradient with respect to the slab probabilities.
static int vardtc_uncertain_rbf(mi355gp_sparse* s, int irbf, bool ss, const double* Z, double beta, double extra_jitter,
                                double* out_scalars, double* dtheta_out, double* dZ_out, double* wv_out, double* dmu_out,
                                double* dS_out, double* dgamma_out, double* stage_ms) {
    hipStream_t st = s->st;
    const long n = s->n, m = s->m;
    const int D = s->D, Dy = s->Dy;
    s->mfma_prof.on = false;
    const SPart& rbf = s->parts[(size_t)irbf];
    PsiWork w;
    w.ss = ss;
    if (int rc = psi_work_setup(s, rbf, Z, &w)) return rc;
    w.b = ss ? 0.0 : bias_sum(s);
    if (w.b > 0.0) {                                             // (a part's variance is positive: parse_part refuses any other)
        HIP_CHECK(s->biasC.need((size_t)s->mp));
        HIP_CHECK(s->biasV.need((size_t)s->Dy));
        HIP_CHECK(s->biasT.need((size_t)s->m));
        HIP_CHECK(s->biasAdd.need((size_t)s->m));
        HIP_CHECK(s->biasPsi2.need((size_t)s->mp * s->mp));
        w.csum = s->biasC, w.vsum = s->biasV, w.tvec = s->biasT, w.addv = s->biasAdd, w.psi2rbf = s->biasPsi2;
    }
    if (int rc = sparse_start(s, Z, &beta, 1)) return rc;
    if (int rc = uncertain_pass1(s, w, extra_jitter)) return rc;
    if (int rc = sparse_mm_block(s, false, beta, 0)) return rc;
    if (int rc = uncertain_pass2(s, w, beta)) return rc;
    sparse_kmm_gradients(s);
    HIP_CHECK(hipEventRecord(s->ev[3], st));
    // ---- small results to the host -----------------------------------------------------------------------------------------
    const int Qp = w.Qp;
    KernGrads kg;
    std::vector<double> zs1((size_t)w.mpad * w.ZL), zs2((size_t)w.mpad * w.ZL), zzh((size_t)m * 2 * Qp);
    std::vector<double> hc, ht, hvs, hwv;                          // Bias parts: c, t, colsum(V), the Woodbury vector
    double scal[8];
    if (int rc = sparse_fetch_gradients(s, false, &kg)) return rc;
    if (w.b > 0.0) {
        hc.resize((size_t)m), ht.resize((size_t)m), hvs.resize((size_t)Dy), hwv.resize((size_t)m * Dy);
        HIP_CHECK(hipMemcpyAsync(hc.data(), w.csum, sizeof(double) * m, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(ht.data(), w.tvec, sizeof(double) * m, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(hvs.data(), w.vsum, sizeof(double) * Dy, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(hwv.data(), s->vvec, sizeof(double) * m * Dy, hipMemcpyDeviceToHost, st));
    }
    HIP_CHECK(hipMemcpyAsync(zs1.data(), w.Zs1, sizeof(double) * zs1.size(), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(zs2.data(), w.Zs2, sizeof(double) * zs2.size(), hipMemcpyDeviceToHost, st));
    if (!ss) HIP_CHECK(hipMemcpyAsync(zzh.data(), w.zz, sizeof(double) * zzh.size(), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(scal, s->scal, sizeof(double) * 4, hipMemcpyDeviceToHost, st));
    if (wv_out) HIP_CHECK(hipMemcpyAsync(wv_out, s->vvec, sizeof(double) * m * Dy, hipMemcpyDeviceToHost, st));
    if (dmu_out) HIP_CHECK(hipMemcpyAsync(dmu_out, w.dMuO, sizeof(double) * n * D, hipMemcpyDeviceToHost, st));
    if (dS_out) HIP_CHECK(hipMemcpyAsync(dS_out, w.dSO, sizeof(double) * n * D, hipMemcpyDeviceToHost, st));
    if (ss && dgamma_out) HIP_CHECK(hipMemcpyAsync(dgamma_out, w.dGO, sizeof(double) * n * D, hipMemcpyDeviceToHost, st));
    if (int rc = sparse_finish(s, 3, stage_ms)) return rc;
    // psi0_n = variance_rbf + sum variance_white, every row: psi0.sum() = N psi0
    vardtc_scalars(s, scal, expression_kdiag(s->parts, s->terms), beta, nullptr, out_scalars);
    // on top of the Kmm record of the RBF part: the psi1 / psi2 sums in the layout of the reduction records (part_dtheta:
    // dvariance = rec[0] / variance, dl = -rec / l); the z_m - z_o terms of psi2 add a_q sum LS dz^2 / 2 to dimension q
    double* ab = kg.gmm.data() + (size_t)irbf * rec_doubles(s);
    ab[0] += w.sums[0];
    std::vector<double> dZss;                                      // spike-and-slab: the psi1 / psi2 shares of dZ (psi_ss.hip)
    if (ss) {
        dZss.assign((size_t)m * D, 0.0);
        pss_finish_z(zs1.data(), zs2.data(), w.ha.data(), w.hzp.data(), m, D, Qp, dZss.data(), w.sums.data() + 1);
    }
    for (int q = 0; q < D; ++q) {
        double zq = 0.0;
        if (!ss)
            for (long j = 0; j < m; ++j) zq += zzh[(size_t)j * 2 * Qp + Qp + q];
        const double lq = ss ? w.sums[(size_t)(1 + q)] : w.sums[(size_t)(1 + q)] + 0.5 * w.ha[(size_t)q] * zq;
        ab[(size_t)(q / 32) * GP_STRIDE + 2 + (q % 32)] -= lq;
        ab[1] -= lq;
    }
    if (w.b > 0.0) {
        // every Bias part, on top of Kmm's record and of N dL_dpsi0 below: sum dL_dpsi1 + t . c + 2 N b sum(E)   (static.py:165-
        // 172 with add.py's cross terms; sum dL_dpsi1 = colsum(V) . colsum(v)); the record is divided by the variance later
        double s1 = 0.0, tc = 0.0, ts = 0.0;
        for (int d = 0; d < Dy; ++d) {
            double cv = 0.0;
            for (long j = 0; j < m; ++j) cv += hwv[(size_t)(j * Dy + d)];
            s1 = fma(hvs[(size_t)d], cv, s1);
        }
        for (long j = 0; j < m; ++j) {
            tc = fma(ht[(size_t)j], hc[(size_t)j], tc);
            ts += ht[(size_t)j];
        }
        const double extra = s1 + tc + (double)s->n * w.b * ts;        // (sum(E) = sum(t) / 2)
        for (size_t i = 0; i < s->parts.size(); ++i)
            if (s->parts[i].kp.kind == MI355GP_BIAS) kg.gmm[i * rec_doubles(s)] += extra * s->parts[i].kp.variance;
    }
    // dL_dpsi0 = -Dy beta / 2 per row, dpsi0 / dvariance = 1
    sparse_assemble_gradients(s, kg, -0.5 * Dy * beta * (double)n, dtheta_out, dZ_out);
    if (dZ_out && ss)
        for (long j = 0; j < m * D; ++j) dZ_out[j] += dZss[(size_t)j];
    if (dZ_out && !ss)  // + gradients_Z_expectations (the psi1 and psi2 parts; sparse_gp.py:100-107)
        for (long j = 0; j < m; ++j)
            for (int q = 0; q < D; ++q)
                dZ_out[j * D + q] += zs1[(size_t)j * Qp + q] + 2.0 * zs2[(size_t)j * Qp + q] - w.ha[(size_t)q] * zzh[(size_t)j * 2 * Qp + q];
    s->have_result = true;
    s->uncertain_result = true;
    return 0;
}

// One SparseGP.parameters_changed for UNCERTAIN inputs q(x_n) = N(X_n, diag S_n) (set_data + set_input_variance), a scalar
// noise variance and one RBF part alone or with White parts (var_dtc.py:93-120,133-163,217-233,258-276 with psi statistics
// in place of Kdiag / Knm / Knm^T Knm; rbf_psi_comp.py; static.py: White adds its variance to psi0 and to Kmm's diagonal):
// the phases of the certain-input call with the psi kernels in the two passes and dL_dpsi0 = -Dy beta / 2.
// out_scalars, dtheta_out (concatenated over the parts), dZ_out, wv_out, stage_ms as mi355gp_vardtc_inference_sum;
// dmu_out / dS_out (optional, N x D): the gradients with respect to the means and variances of the inputs.
int mi355gp_vardtc_inference_uncertain(mi355gp_sparse* s, int nparts, const mi355gp_part* parts, const double* Z, int64_t M,
                                       const double* noise, int64_t noise_len, double extra_jitter, double* out_scalars,
                                       double* dtheta_out, double* dZ_out, double* wv_out, double* dmu_out, double* dS_out,
                                       double* stage_ms) {
    ARG_CHECK(s && s->n > 0, "mi355gp_vardtc_inference_uncertain: set_data first");
    ARG_CHECK(parts && Z && M > 0 && out_scalars && noise && nparts >= 1, "mi355gp_vardtc_inference_uncertain: bad arguments");
    ARG_CHECK(!sharded(s), "mi355gp_vardtc_inference_uncertain: a row-sharded context is not supported with uncertain inputs");
    ARG_CHECK(s->dSvar, "mi355gp_vardtc_inference_uncertain: no input variances; call mi355gp_sparse_set_input_variance after set_data");
    ARG_CHECK(!s->dGam, "mi355gp_vardtc_inference_uncertain: the context holds slab probabilities (mi355gp_sparse_set_binary_prob), which "
                        "this entry would drop; call mi355gp_vardtc_inference_ss, or clear them with a NULL gamma");
    ARG_CHECK(!s->missing, "mi355gp_vardtc_inference_uncertain: the context holds output groups (mi355gp_sparse_set_output_groups), whose "
                           "mask this entry would ignore; call mi355gp_vardtc_inference_missing, or clear them with G = 0");
    if (noise_len != 1)
        PART_FAIL("mi355gp_vardtc_inference_uncertain: per-point noise (%lld variances) is not supported with uncertain inputs "
                  "(var_dtc.py:243); pass one noise variance", (long long)noise_len);
    int irbf = -1;
    if (int rc = uncertain_check_parts(s, nparts, parts, M, &irbf)) return rc;
    EngineShared gate(s->device);
    if (int rc = sparse_open(s, nparts, parts, M)) return rc;
    const double beta = 1.0 / fmax(noise[0], 1e-8);
    s->beta_scalar = beta;
    if (s->parts[(size_t)irbf].linear())
        return vardtc_uncertain_linear(s, irbf, Z, beta, extra_jitter, out_scalars, dtheta_out, dZ_out, wv_out, dmu_out, dS_out,
                                       stage_ms);
    return vardtc_uncertain_rbf(s, irbf, false, Z, beta, extra_jitter, out_scalars, dtheta_out, dZ_out, wv_out, dmu_out, dS_out, nullptr,
                                stage_ms);
}

// VarDTC with spike-and-slab inputs q(x_nq) = gamma_nq N(mu_nq, S_nq) + (1 - gamma_nq) delta_0 (set_data's X as the means,
// mi355gp_sparse_set_input_variance, mi355gp_sparse_set_binary_prob; GPy/models/ss_gplvm.py with ssrbf_psi_comp.py): the phases of
// mi355gp_vardtc_inference_uncertain with the kernels of psi_ss.hip in the psi slots.  One RBF part alone or summed with White
// parts, one noise variance.  dgamma_out (optional, N x D): the gradient with respect to gamma.  The result lies where VarDTC's
// does: mi355gp_sparse_predict, mi355gp_sparse_fetch and mi355gp_sparse_predict_uncertain (Gaussian new points) serve it.
int mi355gp_vardtc_inference_ss(mi355gp_sparse* s, int nparts, const mi355gp_part* parts, const double* Z, int64_t M,
                                const double* noise, int64_t noise_len, double extra_jitter, double* out_scalars, double* dtheta_out,
                                double* dZ_out, double* wv_out, double* dmu_out, double* dS_out, double* dgamma_out,
                                double* stage_ms) {
    const char* where = "mi355gp_vardtc_inference_ss";
    ARG_CHECK(s && s->n > 0, "mi355gp_vardtc_inference_ss: set_data first");
    ARG_CHECK(parts && Z && M > 0 && out_scalars && noise && nparts >= 1, "mi355gp_vardtc_inference_ss: bad arguments");
    ARG_CHECK(!sharded(s), "mi355gp_vardtc_inference_ss: a row-sharded context is not supported with spike-and-slab inputs");
    ARG_CHECK(s->dSvar && s->dGam, "mi355gp_vardtc_inference_ss: no slab probabilities; call mi355gp_sparse_set_input_variance and "
                                   "mi355gp_sparse_set_binary_prob (or mi355gp_sparse_set_inputs_ss) after set_data");
    ARG_CHECK(!s->missing, "mi355gp_vardtc_inference_ss: the context holds output groups (mi355gp_sparse_set_output_groups), whose mask "
                           "this entry would ignore; clear them with G = 0");
    if (noise_len != 1)
        PART_FAIL("%s: per-point noise (%lld variances) is not supported with spike-and-slab inputs; pass one noise variance", where,
                  (long long)noise_len);
    int irbf = -1;
    if (int rc = uncertain_check_parts(s, nparts, parts, M, &irbf, where, true)) return rc;
    EngineShared gate(s->device);
    if (int rc = sparse_open(s, nparts, parts, M)) return rc;
    const double beta = 1.0 / fmax(noise[0], 1e-8);
    s->beta_scalar = beta;
    return vardtc_uncertain_rbf(s, irbf, true, Z, beta, extra_jitter, out_scalars, dtheta_out, dZ_out, wv_out, dmu_out, dS_out, dgamma_out,
                                stage_ms);
}

// ---- VarDTC with uncertain inputs and MISSING entries of Y (include/mi355gp_sparse_missing.h) ----------------------------------
// The reference's loop (GPy/models/sparse_gp_minibatch.py:228-286): output columns with the same observed rows form a group g
// (row weights w_g, c_g columns, N_g rows); every group is a VarDTC problem of its own on the shared Kmm,
//   psi2_g = sum_n w_ng psi2n,  psi1^T V restricted to the group's columns (V = beta Y with Y = 0 where unobserved),
// and the gradients add up: dL_dKmm = sum_g, dL_dpsi1 = beta Y v^T over ALL Woodbury columns (the zeros of Y make it the right
// chain rule for every pattern at once), dL_dpsi2[n] = sum_g w_ng E_g with E_g = beta sym(Q2_g), dL_dpsi0[n] = -beta/2 times the
// number of outputs observed at n.  psi2_g and the psi2 row pass go through the group-batched kernels of psi_missing.hip, the
// M x M phase (sparse_mm_block) runs once per group in group order on the context's own buffers.
struct MissingState {
    int G = 0;
    long n = 0, mp = 0;
    std::vector<int> gof;                    // Dy: group of output d
    std::vector<std::vector<int>> cols;      // per group: its output columns, ascending
    std::vector<long> Ng;                    // per group: observed rows
    std::vector<double> yy, gscal;           // per group: sum y^2 over its observed entries; MI355GP_NUM_OUT scalars of the last call
    double obs_total = 0.0;                  // sum_g c_g N_g: observed entries of Y
    std::vector<long> coff;                  // per group: where its columns start in dCols
    DevBuf dWt, dCols;                       // the weights, group-major (G x n); the groups' column lists, concatenated (Dy ints)
    // per M (grown on demand, kept between evaluations so that an optimiser step allocates nothing): G x {psi2_g, E_g, Winv_g},
    // the wide Woodbury vector, a thin psi1^T V, the dL_dKmm and z_m - z_o sums, the partial buffer of one group batch
    GrowBuf psi2g, Eg, Winvg, vvAll, psi1Yg, dKacc, zzAcc, part;
    bool have = false;                       // the per-group results describe the context's latest evaluation
};

void missing_release(mi355gp_sparse* s) {
    delete s->missing;
    s->missing = nullptr;
}

// out = scale (A + A^T) / 2 over the leading m x m, 0 in the padding (k_sym_scaled)
static void missing_sym(hipStream_t st, const double* A, long mp, long m, double scale, double* out) {
    hipLaunchKernelGGL(k_sym_scaled, grid2d(mp, mp), dim3(256), 0, st, A, mp, m, scale, out);
}
// dst[j][cols[k]] = src[j][k] (scatter: src mp x c, dst mp x Dy) or src2[j][k] = dst[j][cols[k]] (gather), j < rows
__global__ void k_missing_cols(double* __restrict__ wide, int Dy, double* __restrict__ thin, int c, const int* __restrict__ cols,
                               long rows, int gather) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * c) return;
    const long j = i / c;
    const int k = (int)(i - j * c);
    if (gather) thin[i] = wide[j * Dy + cols[k]];
    else wide[j * Dy + cols[k]] = thin[i];
}

// restores what the per-group M x M phase borrows from the context, whatever way the call ends
struct MissingBorrow {
    mi355gp_sparse* s;
    int Dy;
    long n_global;
    double trYYT;
    double *psi2, *psi1Y;
    explicit MissingBorrow(mi355gp_sparse* s_) : s(s_), Dy(s_->Dy), n_global(s_->n_global), trYYT(s_->trYYT), psi2(s_->psi2), psi1Y(s_->psi1Y) {}
    ~MissingBorrow() { s->Dy = Dy, s->n_global = n_global, s->trYYT = trYYT, s->psi2 = psi2, s->psi1Y = psi1Y; }
};

int mi355gp_sparse_set_output_groups(mi355gp_sparse* s, int G, const int* group_of_output, const double* W) {
    const char* where = "mi355gp_sparse_set_output_groups";
    ARG_CHECK(s && s->n > 0, "mi355gp_sparse_set_output_groups: set_data first");
    HIP_CHECK(hipSetDevice(s->device));
    if (G == 0) {
        EngineShared gate(s->device);
        HIP_CHECK(hipStreamSynchronize(s->st));
        missing_release(s);
        s->have_result = s->winv_ok = false;
        return 0;
    }
    ARG_CHECK(G > 0 && group_of_output && W, "mi355gp_sparse_set_output_groups: bad arguments");
    ARG_CHECK(!sharded(s), "mi355gp_sparse_set_output_groups: a row-sharded context is not supported with missing data");
    ARG_CHECK(s->dSvar, "mi355gp_sparse_set_output_groups: no input variances (missing data is handled on the uncertain-input path); call "
                        "mi355gp_sparse_set_input_variance after set_data");
    ARG_CHECK(!s->dGam, "mi355gp_sparse_set_output_groups: the context holds slab probabilities; spike-and-slab inputs are not supported with missing data");
    ARG_CHECK(!s->take_psi_lin && !s->take_linear && !s->take_coreg,
              "mi355gp_sparse_set_output_groups: a context asked for psi_lin_bias, linear or coregionalize is not supported with missing data");
    const long n = s->n;
    const int Dy = s->Dy;
    if (G > Dy) PART_FAIL("%s: %d groups for %d outputs", where, G, Dy);
    MissingState* ms = new MissingState;
    std::unique_ptr<MissingState> hold(ms);
    ms->G = G, ms->n = n;
    ms->gof.assign(group_of_output, group_of_output + Dy);
    ms->cols.resize((size_t)G);
    for (int d = 0; d < Dy; ++d) {
        if (ms->gof[(size_t)d] < 0 || ms->gof[(size_t)d] >= G) PART_FAIL("%s: output %d is in group %d of %d", where, d, ms->gof[(size_t)d], G);
        ms->cols[(size_t)ms->gof[(size_t)d]].push_back(d);
    }
    for (int g = 0; g < G; ++g)
        if (ms->cols[(size_t)g].empty()) PART_FAIL("%s: group %d has no output", where, g);
    std::vector<double> wt((size_t)G * n), hy((size_t)n * Dy);
    ms->Ng.assign((size_t)G, 0);
    ms->yy.assign((size_t)G, 0.0);
    for (long i = 0; i < n; ++i)
        for (int g = 0; g < G; ++g) {
            const double w = W[i * G + g];
            if (w != 0.0 && w != 1.0) PART_FAIL("%s: W[%ld][%d] = %g; the row weights are 0 or 1", where, i, g, w);
            wt[(size_t)g * n + i] = w;
            ms->Ng[(size_t)g] += (w == 1.0);
        }
    for (int g = 0; g < G; ++g)
        if (ms->Ng[(size_t)g] == 0) PART_FAIL("%s: group %d (first output %d) has no observed row", where, g, ms->cols[(size_t)g][0]);
    EngineShared gate(s->device);
    HIP_CHECK(hipStreamSynchronize(s->st));
    HIP_CHECK(hipMemcpy(hy.data(), s->dY, sizeof(double) * n * Dy, hipMemcpyDeviceToHost));
    for (long i = 0; i < n; ++i)
        for (int d = 0; d < Dy; ++d) {
            const double y = hy[(size_t)(i * Dy + d)];
            const int g = ms->gof[(size_t)d];
            if (!std::isfinite(y)) PART_FAIL("%s: Y[%ld][%d] is not finite; store 0 where an entry is unobserved", where, i, d);
            if (wt[(size_t)g * n + i] == 0.0 && y != 0.0)
                PART_FAIL("%s: Y[%ld][%d] = %g is unobserved by its group %d; store 0 there", where, i, d, y, g);
            ms->yy[(size_t)g] += y * y;
        }
    ms->obs_total = 0.0;
    for (int g = 0; g < G; ++g) ms->obs_total += (double)ms->Ng[(size_t)g] * (double)ms->cols[(size_t)g].size();
    HIP_CHECK(ms->dWt.alloc(wt.size()));
    HIP_CHECK(hipMemcpy(ms->dWt, wt.data(), sizeof(double) * wt.size(), hipMemcpyHostToDevice));
    std::vector<int> call;
    for (int g = 0; g < G; ++g) {
        ms->coff.push_back((long)call.size());
        call.insert(call.end(), ms->cols[(size_t)g].begin(), ms->cols[(size_t)g].end());
    }
    HIP_CHECK(ms->dCols.alloc((size_t)(Dy + 1) / 2 + 1));                 // Dy ints
    HIP_CHECK(hipMemcpy(ms->dCols, call.data(), sizeof(int) * call.size(), hipMemcpyHostToDevice));
    missing_release(s);
    s->missing = hold.release();
    s->have_result = s->winv_ok = false;
    return 0;
}

// the M x M buffers of the groups for the context's current mp: G x {psi2_g, E_g, Winv_g}, the wide Woodbury vector, a thin
// psi1^T V, the dL_dKmm sum
static int missing_alloc_m(mi355gp_sparse* s) {
    MissingState* ms = s->missing;
    const size_t mm = (size_t)s->mp * s->mp;
    const long chunk = s->n < PSI_CHUNK ? s->n : PSI_CHUNK, ld2 = round_up(s->m, PSI_T2);
    HIP_CHECK(ms->psi2g.need(mm * ms->G));
    HIP_CHECK(ms->Eg.need(mm * ms->G));
    HIP_CHECK(ms->Winvg.need(mm * ms->G));
    HIP_CHECK(ms->vvAll.need((size_t)s->mp * s->Dy));
    HIP_CHECK(ms->psi1Yg.need((size_t)s->mp * s->Dy));
    HIP_CHECK(ms->dKacc.need(mm));
    HIP_CHECK(ms->zzAcc.need((size_t)s->m * 2 * psi_qp(s->D)));
    HIP_CHECK(ms->part.need((size_t)PSI_GB * psi2_nsplit(chunk, s->m) * ld2 * ld2));
    ms->mp = s->mp;
    return 0;
}

int mi355gp_vardtc_inference_missing(mi355gp_sparse* s, int nparts, const mi355gp_part* parts, const double* Z, int64_t M,
                                     const double* noise, int64_t noise_len, double extra_jitter, double* out_scalars,
                                     double* dtheta_out, double* dZ_out, double* wv_out, double* dmu_out, double* dS_out,
                                     double* stage_ms) {
    const char* where = "mi355gp_vardtc_inference_missing";
    ARG_CHECK(s && s->n > 0, "mi355gp_vardtc_inference_missing: set_data first");
    ARG_CHECK(parts && Z && M > 0 && out_scalars && noise && nparts >= 1, "mi355gp_vardtc_inference_missing: bad arguments");
    ARG_CHECK(!sharded(s), "mi355gp_vardtc_inference_missing: a row-sharded context is not supported with missing data");
    ARG_CHECK(s->missing, "mi355gp_vardtc_inference_missing: no output groups; call mi355gp_sparse_set_output_groups after set_data and "
                          "mi355gp_sparse_set_input_variance");
    ARG_CHECK(s->dSvar && !s->dGam, "mi355gp_vardtc_inference_missing: Gaussian input variances are required (and no slab probabilities)");
    ARG_CHECK(!s->take_psi_lin && !s->take_linear && !s->take_coreg,
              "mi355gp_vardtc_inference_missing: a context asked for psi_lin_bias, linear or coregionalize is not supported with missing data");
    if (noise_len != 1)
        PART_FAIL("%s: per-point noise (%lld variances) is not supported with missing data; pass one noise variance", where, (long long)noise_len);
    int irbf = -1;
    if (int rc = uncertain_check_parts(s, nparts, parts, M, &irbf, where, true)) return rc;
    EngineShared gate(s->device);
    if (int rc = sparse_open(s, nparts, parts, M)) return rc;
    MissingState* ms = s->missing;
    ms->have = false;
    if (int rc = missing_alloc_m(s)) return rc;
    const double beta = 1.0 / fmax(noise[0], 1e-8);
    s->beta_scalar = beta;
    hipStream_t st = s->st;
    const long n = s->n, m = s->m, mp = s->mp;
    const size_t mm = (size_t)mp * mp;
    const int D = s->D, Dy = s->Dy, G = ms->G;
    s->mfma_prof.on = false;
    const SPart& rbf = s->parts[(size_t)irbf];
    PsiWork w;
    if (int rc = psi_work_setup(s, rbf, Z, &w)) return rc;
    const int Qp = w.Qp;
    double* part = ms->part;
    if (int rc = sparse_start(s, Z, &beta, 1)) return rc;
    // ---- pass 1: Kmm, Lm, Lm^-1 and psi1^T V as for complete data; psi2_g for every group through the batched kernel ----------
    if (int rc = uncertain_pass1(s, w, extra_jitter, /*want_psi2=*/false)) return rc;
    HIP_CHECK(hipMemsetAsync(ms->psi2g, 0, sizeof(double) * mm * G, st));
    int nch = 0;
    for (long r0 = 0; r0 < n; r0 += PSI_CHUNK, ++nch) {
        const long rc = (n - r0 < PSI_CHUNK) ? (n - r0) : PSI_CHUNK;
        launch_psi_rows(st, s->dX + r0 * D, s->dSvar + r0 * D, w.dA, rc, D, Qp, w.rd1, w.rd2, w.lg1, w.lg2);
        for (int g0 = 0; g0 < G; g0 += PSI_GB) {
            const int gb = (G - g0 < PSI_GB) ? (G - g0) : PSI_GB;
            const int ns = launch_psi2_multi(st, w.rd2, w.lg2, ms->dWt + (long)g0 * n + r0, n, gb, w.dZp, w.dA, rc, m, Qp, w.var * w.var,
                                             w.ld2, part);
            for (int g = 0; g < gb; ++g)
                launch_psi2_combine(st, part + (size_t)g * ns * w.ld2 * w.ld2, w.ld2, m, ns, nch > 0, ms->psi2g + (size_t)(g0 + g) * mm, mp);
        }
    }
    HIP_CHECK(hipEventRecord(s->ev[1], st));
    // ---- the M x M phase, once per group in group order ---------------------------------------------------------------------
    std::vector<double> scal((size_t)G * 4);
    int info_b = 0;                                                       // the first group's B that is not positive definite
    {
        MissingBorrow borrow(s);
        for (int g = 0; g < G; ++g) {
            const std::vector<int>& cg = ms->cols[(size_t)g];
            const int c = (int)cg.size();
            const int* dcols = (const int*)ms->dCols.p + ms->coff[(size_t)g];
            hipLaunchKernelGGL(k_missing_cols, dim3((unsigned)((mp * c + 255) / 256)), dim3(256), 0, st, borrow.psi1Y, Dy, (double*)ms->psi1Yg, c,
                               dcols, mp, 1);
            s->Dy = c;
            s->psi1Y = ms->psi1Yg;
            s->psi2 = ms->psi2g + (size_t)g * mm;
            if (int rc = sparse_mm_block(s, false, beta, 0)) return rc;
            hipLaunchKernelGGL(k_missing_cols, dim3((unsigned)((mp * c + 255) / 256)), dim3(256), 0, st, (double*)ms->vvAll, Dy, s->vvec, c,
                               dcols, mp, 0);
            missing_sym(st, s->Q2, mp, m, beta, ms->Eg + (size_t)g * mm);
            launch_mm_axpby(st, s->dLdKmm, 1.0, g ? (const double*)ms->dKacc : nullptr, 1.0, 0.0, mp, ms->dKacc);
            // woodbury_inv_g = Lm^-T (I - B_g^-1) Lm^-1 (ensure_winv's steps, into the group's own matrix)
            launch_mm_sym(st, s->Bi, mp, s->E);
            launch_mm_axpby(st, s->E, -1.0, nullptr, 0.0, 1.0, mp, s->E);
            launch_gemm(st, 1, 1, mp, mp, mp, s->Xm, mp, s->E, mp, s->T1, mp, 1.0, 0.0);
            launch_gemm(st, 0, 1, mp, mp, mp, s->T1, mp, s->Xm, mp, ms->Winvg + (size_t)g * mm, mp, 1.0, 0.0);
            HIP_CHECK(hipMemcpyAsync(scal.data() + (size_t)g * 4, s->scal, sizeof(double) * 4, hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));                          // (h_info[1] is written again by the next group's factorisation)
            if (!info_b && s->h_info[1] > 0) info_b = s->h_info[1];
        }
    }
    s->h_info[1] = info_b;
    HIP_CHECK(hipMemcpyAsync(s->vvec, ms->vvAll, sizeof(double) * mp * Dy, hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipMemcpyAsync(s->dLdKmm, ms->dKacc, sizeof(double) * mm, hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipEventRecord(s->ev[2], st));
    // ---- pass 2: psi1 with dL_dpsi1 = beta Y v^T over all Woodbury columns; psi2 with the per-row sum_g w_ng E_g ---------------
    for (int g = 0; g < G; ++g) {
        launch_psi2_zz(st, ms->Eg + (size_t)g * mm, ms->psi2g + (size_t)g * mm, mp, w.dZp, m, Qp, w.zz);
        launch_sum_splits(st, w.zz, m * 2 * Qp, 1, g > 0, ms->zzAcc);
    }
    std::vector<double> csum((size_t)(1 + Qp));
    nch = 0;
    for (long r0 = 0; r0 < n; r0 += PSI_CHUNK, ++nch) {
        const long rc = (n - r0 < PSI_CHUNK) ? (n - r0) : PSI_CHUNK;
        const int nb = (int)((rc + PSI_GROWS - 1) / PSI_GROWS);
        const PsiRank rk{s->dY + r0 * Dy, s->vvec, Dy, beta};
        launch_psi_rows(st, s->dX + r0 * D, s->dSvar + r0 * D, w.dA, rc, D, Qp, w.rd1, w.rd2, w.lg1, w.lg2);
        launch_psi1_grad(st, w.rd1, w.lg1, w.dZp, nullptr, 0, rk, rc, m, w.mpad, Qp, w.var, w.Ppart, w.Zpart, nullptr);
        launch_sum_splits(st, w.Ppart, rc * w.RL, (int)w.mt, 0, w.P1s);
        launch_sum_splits(st, w.Zpart, w.mpad * w.ZL, nb, nch > 0, w.Zs1);
        for (int g0 = 0; g0 < G; g0 += PSI_GB) {
            const int gb = (G - g0 < PSI_GB) ? (G - g0) : PSI_GB;
            launch_psi2_grad_multi(st, w.rd2, w.lg2, ms->dWt + (long)g0 * n + r0, n, gb, w.dZp, w.dA, ms->Eg + (size_t)g0 * mm, (long)mm, mp,
                                   rc, m, w.mpad, Qp, w.var * w.var, w.Ppart, w.Zpart);
            launch_sum_splits(st, w.Ppart, rc * w.RL, (int)w.mt, g0 > 0, w.P2s);
            launch_sum_splits(st, w.Zpart, w.mpad * w.ZL, nb, nch > 0 || g0 > 0, w.Zs2);
        }
        launch_psi_rowfinish(st, w.P1s, w.P2s, s->dSvar + r0 * D, w.dA, rc, D, Qp, w.dMuO + r0 * D, w.dSO + r0 * D, w.rowrec);
        launch_reduce_partials(st, w.rowrec, (int)rc, 1 + Qp, w.rec);
        HIP_CHECK(hipMemcpyAsync(csum.data(), w.rec, sizeof(double) * (1 + Qp), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        for (int k = 0; k <= Qp; ++k) w.sums[(size_t)k] += csum[(size_t)k];           // chunks in row order
    }
    sparse_kmm_gradients(s);
    HIP_CHECK(hipEventRecord(s->ev[3], st));
    // ---- small results to the host -----------------------------------------------------------------------------------------
    KernGrads kg;
    std::vector<double> zs1((size_t)w.mpad * w.ZL), zs2((size_t)w.mpad * w.ZL), zzh((size_t)m * 2 * Qp);
    if (int rc = sparse_fetch_gradients(s, false, &kg)) return rc;
    HIP_CHECK(hipMemcpyAsync(zs1.data(), w.Zs1, sizeof(double) * zs1.size(), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(zs2.data(), w.Zs2, sizeof(double) * zs2.size(), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(zzh.data(), ms->zzAcc, sizeof(double) * zzh.size(), hipMemcpyDeviceToHost, st));
    if (wv_out) HIP_CHECK(hipMemcpyAsync(wv_out, s->vvec, sizeof(double) * m * Dy, hipMemcpyDeviceToHost, st));
    if (dmu_out) HIP_CHECK(hipMemcpyAsync(dmu_out, w.dMuO, sizeof(double) * n * D, hipMemcpyDeviceToHost, st));
    if (dS_out) HIP_CHECK(hipMemcpyAsync(dS_out, w.dSO, sizeof(double) * n * D, hipMemcpyDeviceToHost, st));
    if (int rc = sparse_finish(s, 3, stage_ms)) return rc;
    // the scalars: the existing formulas per group with (N_g, c_g, sum y^2 over the group's observed entries), added in group order
    ms->gscal.assign((size_t)G * MI355GP_NUM_OUT, 0.0);
    for (int i = 0; i < MI355GP_NUM_OUT; ++i) out_scalars[i] = 0.0;
    {
        MissingBorrow borrow(s);
        const double kd = expression_kdiag(s->parts, s->terms);
        for (int g = 0; g < G; ++g) {
            double* og = ms->gscal.data() + (size_t)g * MI355GP_NUM_OUT;
            s->Dy = (int)ms->cols[(size_t)g].size();
            s->n_global = ms->Ng[(size_t)g];
            s->trYYT = ms->yy[(size_t)g];
            vardtc_scalars(s, scal.data() + (size_t)g * 4, kd, beta, nullptr, og);
            for (int i = 0; i < 5; ++i) out_scalars[i] += og[i];
        }
    }
    out_scalars[5] = beta;
    double* ab = kg.gmm.data() + (size_t)irbf * rec_doubles(s);
    ab[0] += w.sums[0];
    for (int q = 0; q < D; ++q) {
        double zq = 0.0;
        for (long j = 0; j < m; ++j) zq += zzh[(size_t)j * 2 * Qp + Qp + q];
        const double lq = w.sums[(size_t)(1 + q)] + 0.5 * w.ha[(size_t)q] * zq;
        ab[(size_t)(q / 32) * GP_STRIDE + 2 + (q % 32)] -= lq;
        ab[1] -= lq;
    }
    // sum_n dL_dpsi0_n = -beta/2 times the observed entries of Y, dpsi0 / dvariance = 1
    sparse_assemble_gradients(s, kg, -0.5 * beta * ms->obs_total, dtheta_out, dZ_out);
    if (dZ_out)
        for (long j = 0; j < m; ++j)
            for (int q = 0; q < D; ++q)
                dZ_out[j * D + q] += zs1[(size_t)j * Qp + q] + 2.0 * zs2[(size_t)j * Qp + q] - w.ha[(size_t)q] * zzh[(size_t)j * 2 * Qp + q];
    // the context's current result: the last group's B^-1 is still in place; point woodbury_inv at group 0 (select to change)
    HIP_CHECK(hipMemcpyAsync(s->Winv, ms->Winvg, sizeof(double) * mm, hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipMemcpyAsync(s->psi2, ms->psi2g, sizeof(double) * mm, hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));
    s->winv_ok = true;
    s->have_result = true;
    s->uncertain_result = true;
    ms->have = true;
    return 0;
}

// Makes group g's woodbury_inv (and psi2) the context's current ones: mi355gp_sparse_predict, mi355gp_sparse_predict_uncertain and
// mi355gp_sparse_fetch then serve the outputs of that group (posterior.py:243-246, :268); the mean uses all Woodbury columns
int mi355gp_sparse_select_output_group(mi355gp_sparse* s, int g) {
    ARG_CHECK(s && s->missing && s->missing->have && s->have_result && s->missing->mp == s->mp,
              "mi355gp_sparse_select_output_group: run mi355gp_vardtc_inference_missing first");
    MissingState* ms = s->missing;
    if (g < 0 || g >= ms->G) PART_FAIL("mi355gp_sparse_select_output_group: group %d of %d", g, ms->G);
    HIP_CHECK(hipSetDevice(s->device));
    EngineShared gate(s->device);
    const size_t mm = (size_t)s->mp * s->mp;
    HIP_CHECK(hipMemcpyAsync(s->Winv, ms->Winvg + (size_t)g * mm, sizeof(double) * mm, hipMemcpyDeviceToDevice, s->st));
    HIP_CHECK(hipMemcpyAsync(s->psi2, ms->psi2g + (size_t)g * mm, sizeof(double) * mm, hipMemcpyDeviceToDevice, s->st));
    HIP_CHECK(hipStreamSynchronize(s->st));
    s->winv_ok = true;
    return 0;
}

// The per-group copies of out_scalars of the last mi355gp_vardtc_inference_missing call: G x 8, rows in group order
int mi355gp_sparse_fetch_group_scalars(mi355gp_sparse* s, double* out) {
    ARG_CHECK(s && out && s->missing && s->missing->have, "mi355gp_sparse_fetch_group_scalars: run mi355gp_vardtc_inference_missing first");
    memcpy(out, s->missing->gscal.data(), sizeof(double) * s->missing->gscal.size());
    return 0;
}

// ---- results of the last VarDTC call ------------------------------------------------------------------------------------
// woodbury_inv = Lm^-T (I - B^-1) Lm^-1 (var_dtc.py:206-210) into s->Winv, once per inference call
static int ensure_winv(mi355gp_sparse* s) {
    if (s->winv_ok) return 0;
    hipStream_t st = s->st;
    const long mp = s->mp;
    launch_mm_sym(st, s->Bi, mp, s->E);
    launch_mm_axpby(st, s->E, -1.0, nullptr, 0.0, 1.0, mp, s->E);
    launch_gemm(st, 1, 1, mp, mp, mp, s->Xm, mp, s->E, mp, s->T1, mp, 1.0, 0.0);
    launch_gemm(st, 0, 1, mp, mp, mp, s->T1, mp, s->Xm, mp, s->Winv, mp, 1.0, 0.0);
    s->winv_ok = true;
    return 0;
}

// M x M results of the last call: 0 = dL_dKmm, 1 = woodbury_inv = Lm^-T (I - B^-1) Lm^-1 (var_dtc.py:206-210),
// 2 = Lm (lower, strict upper zero), 3 = Kmm (with the 1e-8 jitter), 4 = psi2 (heteroscedastic: sum_n beta_n k_n k_n^T),
// 5 = dL_dpsi2_beta = Lm^-T (Dy I - P) Lm^-1 / 2 (var_dtc.py:220; dL_dpsi2 = beta times it for a scalar noise)
int mi355gp_sparse_fetch(mi355gp_sparse* s, int which, double* out) {
    ARG_CHECK(!s || !s->svgp_result, "mi355gp_sparse_fetch: the last call on this context was an SVGP call (this entry describes VarDTC's result; mi355gp_svgp_predict serves SVGP)");
    ARG_CHECK(s && out && s->have_result, "mi355gp_sparse_fetch: run mi355gp_vardtc_inference first");
    HIP_CHECK(hipSetDevice(s->device));
    EngineShared gate(s->device);
    hipStream_t st = s->st;
    const long m = s->m, mp = s->mp;
    const double* src = nullptr;
    if (which == 0) src = s->dLdKmm;
    else if (which == 1) {
        if (int rc = ensure_winv(s)) return rc;
        src = s->Winv;
    } else if (which == 2) {
        launch_extract(st, s->Lm, mp, mp, 0, nullptr, 0, s->E, 0);
        src = s->E;
    } else if (which == 3) {
        build_kmm(s, s->E, s->T1, s->kmm_jitter, /*lower_only=*/0);
        src = s->E;
    } else if ((which == 4 || which == 5) && s->pep_result) {
        mi355gp_set_error("mi355gp_sparse_fetch: matrix id %d (psi2 / dL_dpsi2) does not exist for a PEP / FITC result", which);
        return -1;
    } else if (which == 4) src = s->psi2;
    else if (which == 5) src = s->Q2;
    else {
        mi355gp_set_error("mi355gp_sparse_fetch: unknown matrix id %d", which);
        return -1;
    }
    HIP_CHECK(hipMemcpy2DAsync(out, sizeof(double) * m, src, sizeof(double) * mp, sizeof(double) * m, m,
                               hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}

// Rows [row0, row0 + nrows) of dL_dKnm = beta_n (R_n v^T + 2 k_n^T dL_dpsi2_beta) (var_dtc.py:219-233), nrows x M row-major:
// what SparseGP._update_gradients hands to a FOREIGN kernel's update_gradients_full / gradients_X (sparse_gp.py:108-118).
// The N x M matrix is never resident: the caller walks it in row blocks (nrows <= the context's chunk size).
int mi355gp_sparse_fetch_dLdKnm(mi355gp_sparse* s, int64_t row0, int64_t nrows, double* out) {
    ARG_CHECK(!s || !s->svgp_result, "mi355gp_sparse_fetch_dLdKnm: the last call on this context was an SVGP call (this entry describes VarDTC's result; mi355gp_svgp_predict serves SVGP)");
    ARG_CHECK(s && out && s->have_result, "mi355gp_sparse_fetch_dLdKnm: run mi355gp_vardtc_inference first");
    ARG_CHECK(row0 >= 0 && nrows > 0 && row0 + nrows <= s->n && nrows <= s->chunk, "mi355gp_sparse_fetch_dLdKnm: bad row range");
    ARG_CHECK(!s->uncertain_result, "mi355gp_sparse_fetch_dLdKnm: the last call had uncertain inputs (dL_dpsi1 / dL_dpsi2 take dL_dKnm's place)");
    HIP_CHECK(hipSetDevice(s->device));
    EngineShared gate(s->device);
    if (s->pep_result) return pep_fetch_dLdKnm(s, row0, nrows, out);      // (pep.py:81-84: PEP's rows, formed by pep.hip)
    hipStream_t st = s->st;
    const long m = s->m, mp = s->mp, rc = nrows, rcp = round_up(rc, NB);
    if (int rc2 = sparse_cross_rows(s, row0, rc, 0, rcp, nullptr)) return rc2;
    launch_gemm(st, 0, 1, rcp, mp, mp, s->Kfu, mp, s->Q2, mp, s->T, mp, 1.0, 0.0);
    hipLaunchKernelGGL(k_form_dLdKnm, dim3((unsigned)rcp, (unsigned)((mp + 255) / 256)), dim3(256), 0, st, s->T, mp, rc, rcp, m,
                       s->dY + row0 * s->Dy, s->vvec, s->Dy, s->dBeta + row0);
    HIP_CHECK(hipMemcpy2DAsync(out, sizeof(double) * m, s->T, sizeof(double) * mp, sizeof(double) * m, rc,
                               hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    return 0;
}

// Sparse posterior prediction on the device (Posterior._raw_predict, posterior.py:198-262, for the woodbury_inv /
// woodbury_vector representation VarDTC returns): mu = K(X*, Z) v; var = Kdiag - sum(Kx * (Winv Kx), 0) or the full
// K(X*, X*) - Kx^T Winv Kx.  The kernel (parts) must be the one of the last inference call.
int mi355gp_sparse_predict(mi355gp_sparse* s, int nparts, const mi355gp_part* parts, const double* Xnew, int64_t Mn,
                           double* mu_out, double* var_out, int full_cov) {
    ARG_CHECK(!s || !s->svgp_result, "mi355gp_sparse_predict: the last call on this context was an SVGP call (this entry describes VarDTC's result; mi355gp_svgp_predict serves SVGP)");
    ARG_CHECK(s && s->have_result, "mi355gp_sparse_predict: run mi355gp_vardtc_inference first");
    ARG_CHECK(Xnew && Mn > 0 && mu_out, "mi355gp_sparse_predict: bad arguments");
    HIP_CHECK(hipSetDevice(s->device));
    EngineShared gate(s->device);
    if (int rc = prepare_sparse_parts(s, nparts, parts, /*coreg=*/true)) return rc;
    if (int rc = coreg_check_points(s, Xnew, Mn, "new-point")) return rc;
    hipStream_t st = s->st;
    scale_for_parts(s, s->dZ, s->m, s->mp, true);
    if (int rc = ensure_winv(s)) return rc;
    NewPoints q;
    if (int rc = sparse_newpoints(s, Xnew, Mn, full_cov && var_out, s->vvec, s->Dy, "mi355gp_sparse_predict", &q)) return rc;
    if (var_out)
        if (int rc = sparse_newpoints_var(s, &q, s->Winv, full_cov != 0, /*keep_kss=*/false)) return rc;
    HIP_CHECK(hipMemcpyAsync(mu_out, q.Mu, sizeof(double) * Mn * s->Dy, hipMemcpyDeviceToHost, st));
    if (var_out) {
        if (!full_cov)
            HIP_CHECK(hipMemcpyAsync(var_out, q.var, sizeof(double) * Mn, hipMemcpyDeviceToHost, st));
        else
            HIP_CHECK(hipMemcpy2DAsync(var_out, sizeof(double) * Mn, q.var, sizeof(double) * q.mnp, sizeof(double) * Mn, Mn,
                                       hipMemcpyDeviceToHost, st));
    }
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    if (var_out && !full_cov)
        for (int64_t i = 0; i < Mn; ++i) var_out[i] = var_out[i] < 1e-15 ? 1e-15 : var_out[i];      // posterior.py:248
    return 0;
}

// Prediction at uncertain points for a Linear part (ilin) with Bias and White parts.  psi1* is the expression's K(mu*, Z) and the
// psi1 psi1^T half of psi2n contracts to (k lam_d)^2 - k W k^T, so with Zv = Z diag(v)
//   var[n][d] = Kdiag(mu*_n) - k_n W k_n^T + sum_q S*_nq [ v_q + (Zv^T lam_d)_q^2 - diag(Zv^T W Zv)_q ],  clipped at 1e-15:
// the certain-input prediction at the means plus a D-vector dot per row (k_lin_predvar); no psi2n is formed.
static int predict_uncertain_linear(mi355gp_sparse* s, int ilin, const double* mu_new, const double* S_new, int64_t Mn,
                                    double* mean_out, double* var_out) {
    hipStream_t st = s->st;
    const long m = s->m, mp = s->mp;
    const int D = s->D, Dy = s->Dy;
    const SPart& lin = s->parts[(size_t)ilin];
    HIP_CHECK(hipEventRecord(s->ev[4], st));
    NewPoints q;
    if (int rc = sparse_newpoints(s, mu_new, Mn, false, s->vvec, Dy, "mi355gp_sparse_predict_uncertain", &q)) return rc;
    HIP_CHECK(hipMemcpyAsync(mean_out, q.Mu, sizeof(double) * Mn * Dy, hipMemcpyDeviceToHost, st));
    DevBuf dWZ, dS, dG, dVar;
    if (var_out) {
        if (int rc = sparse_newpoints_var(s, &q, s->Winv, false, false)) return rc;
        std::vector<double> wz((size_t)m * D), hz((size_t)m * D), lam((size_t)m * Dy), g((size_t)Dy * D);
        HIP_CHECK(dWZ.alloc(m * D));
        launch_mm_times_z(st, s->Winv, mp, s->dZ, m, D, dWZ);
        HIP_CHECK(hipMemcpyAsync(wz.data(), dWZ, sizeof(double) * m * D, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(hz.data(), s->dZ, sizeof(double) * m * D, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(lam.data(), s->vvec, sizeof(double) * m * Dy, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        for (int c = 0; c < D; ++c) {
            const double v = lin.inv_ls[(size_t)c] * lin.inv_ls[(size_t)c];
            double zwz = 0.0;
            for (long j = 0; j < m; ++j) zwz = fma(hz[(size_t)(j * D + c)], wz[(size_t)(j * D + c)], zwz);
            for (int d = 0; d < Dy; ++d) {
                double zl = 0.0;
                for (long j = 0; j < m; ++j) zl = fma(hz[(size_t)(j * D + c)], lam[(size_t)(j * Dy + d)], zl);
                g[(size_t)(d * D + c)] = v + v * v * (zl * zl - zwz);
            }
        }
        HIP_CHECK(dS.alloc(Mn * D));
        HIP_CHECK(dG.alloc(Dy * D));
        HIP_CHECK(dVar.alloc(Mn * Dy));
        HIP_CHECK(hipMemcpyAsync(dS, S_new, sizeof(double) * Mn * D, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(dG, g.data(), sizeof(double) * Dy * D, hipMemcpyHostToDevice, st));
        launch_lin_predvar(st, q.var, dS, dG, Mn, D, Dy, dVar);
        HIP_CHECK(hipMemcpyAsync(var_out, dVar, sizeof(double) * Mn * Dy, hipMemcpyDeviceToHost, st));
    }
    HIP_CHECK(hipEventRecord(s->ev[5], st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    float ms = 0.0f;
    HIP_CHECK(hipEventElapsedTime(&ms, s->ev[4], s->ev[5]));
    s->predict_ms = ms;
    return 0;
}

// Prediction at UNCERTAIN new points q(x*) = N(mu_new, diag S_new) (Posterior._raw_predict with a VariationalPosterior,
// posterior.py:249-269, full_cov = False) for the kernel of the last VarDTC call, one RBF part alone or with White parts
// (White adds to psi0* only: its psi1 / psi2 are zero, static.py):
//   mean = psi1* lam,  var[n][d] = psi0* + sum_mo psi2n*[m][o] (lam[m][d] lam[o][d] - W[m][o]) - mean[n][d]^2, clipped at 1e-15
// with lam = woodbury_vector and W = woodbury_inv, both resident.  Rows go in chunks of PSI_CHUNK: psi1 and the thin product
// for the mean, k_psi2n_contract (psi.hip) for the two sums; every sum has a fixed order.
int mi355gp_sparse_predict_uncertain(mi355gp_sparse* s, int nparts, const mi355gp_part* parts, const double* mu_new,
                                     const double* S_new, int64_t Mn, double* mean_out, double* var_out) {
    const char* where = "mi355gp_sparse_predict_uncertain";
    ARG_CHECK(!s || !s->svgp_result, "mi355gp_sparse_predict_uncertain: the last call on this context was an SVGP call (this entry describes VarDTC's result)");
    ARG_CHECK(s && s->have_result, "mi355gp_sparse_predict_uncertain: no result yet; run a VarDTC inference call first");
    ARG_CHECK(!sharded(s), "mi355gp_sparse_predict_uncertain: a row-sharded context is not supported at uncertain points");
    ARG_CHECK(parts && nparts >= 1 && mu_new && S_new && Mn > 0 && mean_out, "mi355gp_sparse_predict_uncertain: bad arguments");
    int irbf = -1;
    if (int rc = uncertain_check_parts(s, nparts, parts, s->m, &irbf, where)) return rc;
    const int D = s->D, Dy = s->Dy, NC = Dy + 1;
    for (int64_t i = 0; i < Mn * D; ++i)
        if (!(S_new[i] > 0.0) || !std::isfinite(S_new[i]) || !std::isfinite(mu_new[i]))
            PART_FAIL("%s: input variance S[%lld][%lld] = %g (mean %g): every entry must be positive and finite", where,
                      (long long)(i / D), (long long)(i % D), S_new[i], mu_new[i]);
    HIP_CHECK(hipSetDevice(s->device));
    EngineShared gate(s->device);
    if (int rc = prepare_sparse_parts(s, nparts, parts)) return rc;
    hipStream_t st = s->st;
    scale_for_parts(s, s->dZ, s->m, s->mp, true);
    if (int rc = ensure_winv(s)) return rc;
    if (s->parts[(size_t)irbf].linear()) return predict_uncertain_linear(s, irbf, mu_new, S_new, Mn, mean_out, var_out);
    const long m = s->m, mp = s->mp, mpad = round_up(m, PSI_KT), chunk = Mn < PSI_CHUNK ? Mn : PSI_CHUNK;
    const int Qp = psi_qp(D);
    const SPart& rbf = s->parts[(size_t)irbf];
    // Bias parts (b > 0): psi1 = psi1_rbf + b and psi2n = psi2n_rbf + b (psi1_n 1^T + 1 psi1_n^T) + b^2, so with A_d = lam_d lam_d^T - W
    //   mean += b sum(lam_d),   C[n][d] += 2 b psi1_n . (A_d 1) + b^2 1^T A_d 1,   A_d 1 = lam_d sum(lam_d) - W 1
    // -- u = 2 b (A_d 1) (m x Dy) and the two Dy-vectors are formed once on the host from lam and the row sums of W
    const double bsum = bias_sum(s);
    DevBuf dW1, dU, dCst, dBsl;
    if (bsum > 0.0) {
        std::vector<double> lam((size_t)m * Dy), w1((size_t)m), u((size_t)m * Dy), cst((size_t)Dy), bsl((size_t)Dy);
        HIP_CHECK(dW1.alloc(m));
        launch_mm_colsums(st, s->Winv, mp, m, 1.0, dW1);
        HIP_CHECK(hipMemcpyAsync(w1.data(), dW1, sizeof(double) * m, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(lam.data(), s->vvec, sizeof(double) * m * Dy, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        double sw = 0.0;
        for (long j = 0; j < m; ++j) sw += w1[(size_t)j];
        for (int d = 0; d < Dy; ++d) {
            double sl = 0.0;
            for (long j = 0; j < m; ++j) sl += lam[(size_t)(j * Dy + d)];
            for (long j = 0; j < m; ++j) u[(size_t)(j * Dy + d)] = 2.0 * bsum * (lam[(size_t)(j * Dy + d)] * sl - w1[(size_t)j]);
            cst[(size_t)d] = bsum * bsum * (sl * sl - sw);
            bsl[(size_t)d] = bsum * sl;
        }
        HIP_CHECK(dU.alloc(m * Dy));
        HIP_CHECK(dCst.alloc(Dy));
        HIP_CHECK(dBsl.alloc(Dy));
        HIP_CHECK(hipMemcpy(dU, u.data(), sizeof(double) * m * Dy, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dCst, cst.data(), sizeof(double) * Dy, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dBsl, bsl.data(), sizeof(double) * Dy, hipMemcpyHostToDevice));
    }
    const double var = rbf.kp.variance, psi0 = expression_kdiag(s->parts, s->terms);
    std::vector<double> ha((size_t)Qp, 0.0), hz((size_t)m * D), hzp((size_t)mpad * Qp, 0.0);
    HIP_CHECK(hipMemcpyAsync(hz.data(), s->dZ, sizeof(double) * m * D, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    for (int q = 0; q < D; ++q) ha[(size_t)q] = rbf.inv_ls[(size_t)q] * rbf.inv_ls[(size_t)q];
    for (long i = 0; i < m; ++i)
        for (int q = 0; q < D; ++q) hzp[(size_t)i * Qp + q] = hz[(size_t)i * D + q];
    DevBuf dA, dZp, dMu, dS, rd1, rd2, lg1, lg2, psi1, part, C, mean, vout;
    HIP_CHECK(dA.alloc(Qp));
    HIP_CHECK(dZp.alloc(hzp.size()));
    HIP_CHECK(dMu.alloc(chunk * D));
    HIP_CHECK(dS.alloc(chunk * D));
    HIP_CHECK(rd1.alloc(2 * chunk * Qp));
    HIP_CHECK(rd2.alloc(2 * chunk * Qp));
    HIP_CHECK(lg1.alloc(chunk));
    HIP_CHECK(lg2.alloc(chunk));
    HIP_CHECK(psi1.alloc(chunk * m));
    HIP_CHECK(mean.alloc(chunk * Dy));
    if (var_out) {
        const long last = Mn - (Mn - 1) / PSI_CHUNK * PSI_CHUNK;       // rows of the last chunk: its split count may be larger
        const size_t full = (size_t)psi_contract_nsplit(chunk, m, Qp) * chunk, tail = (size_t)psi_contract_nsplit(last, m, Qp) * last;
        HIP_CHECK(part.alloc((full > tail ? full : tail) * NC));
        HIP_CHECK(C.alloc(chunk * NC));
        HIP_CHECK(vout.alloc(chunk * Dy));
    }
    HIP_CHECK(hipMemcpyAsync(dA, ha.data(), sizeof(double) * Qp, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(dZp, hzp.data(), sizeof(double) * hzp.size(), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipEventRecord(s->ev[4], st));
    for (long r0 = 0; r0 < Mn; r0 += PSI_CHUNK) {
        const long rc = (Mn - r0 < PSI_CHUNK) ? (Mn - r0) : PSI_CHUNK;
        HIP_CHECK(hipMemcpyAsync(dMu, mu_new + r0 * D, sizeof(double) * rc * D, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(dS, S_new + r0 * D, sizeof(double) * rc * D, hipMemcpyHostToDevice, st));
        launch_psi_rows(st, dMu, dS, dA, rc, D, Qp, rd1, rd2, lg1, lg2);
        launch_psi1(st, rd1, lg1, dZp, rc, m, mpad, Qp, var, psi1, m);
        launch_rowdots(st, psi1, psi1, m, rc, m, s->vvec, Dy, mean, nullptr);
        if (bsum > 0.0 && !var_out) launch_psi_bias_pred(st, psi1, m, dU, dCst, dBsl, rc, m, Dy, nullptr, mean);
        if (!(bsum > 0.0 && var_out)) HIP_CHECK(hipMemcpyAsync(mean_out + r0 * Dy, mean, sizeof(double) * rc * Dy, hipMemcpyDeviceToHost, st));
        if (var_out) {
            const int ns = launch_psi2n_contract(st, rd2, lg2, dZp, dA, s->vvec, Dy, s->Winv, mp, rc, m, Qp, var * var, part);
            launch_sum_splits(st, part, rc * NC, ns, 0, C);
            if (bsum > 0.0) {
                launch_psi_bias_pred(st, psi1, m, dU, dCst, dBsl, rc, m, Dy, C, mean);
                HIP_CHECK(hipMemcpyAsync(mean_out + r0 * Dy, mean, sizeof(double) * rc * Dy, hipMemcpyDeviceToHost, st));
            }
            launch_psi_predvar(st, C, mean, psi0, rc, Dy, vout);
            HIP_CHECK(hipMemcpyAsync(var_out + r0 * Dy, vout, sizeof(double) * rc * Dy, hipMemcpyDeviceToHost, st));
        }
        HIP_CHECK(hipStreamSynchronize(st));                   // the chunk's buffers are reused
    }
    HIP_CHECK(hipEventRecord(s->ev[5], st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    float ms = 0.0f;
    HIP_CHECK(hipEventElapsedTime(&ms, s->ev[4], s->ev[5]));   // the chunks' uploads, kernels and copies back
    s->predict_ms = ms;
    return 0;
}

// Whether the inference and prediction entry points of this context take Linear (kind 9) parts; a new context does not
int mi355gp_sparse_set_linear(mi355gp_sparse* s, int on) {
    ARG_CHECK(s, "mi355gp_sparse_set_linear: NULL context");
    s->take_linear = on != 0;
    return 0;
}

// Whether mi355gp_vardtc_inference_sum, mi355gp_sparse_predict and mi355gp_sparse_kdiag of this context take Coregionalize
// (kind 8) parts (include/mi355gp_sparse_coreg.h); a new context does not.  On: the next set_data keeps the rows on the host
int mi355gp_sparse_set_coregionalize(mi355gp_sparse* s, int on) {
    ARG_CHECK(s, "mi355gp_sparse_set_coregionalize: NULL context");
    s->take_coreg = on != 0;
    return 0;
}

// The A/B switch of the second pass (include/mi355gp_debug_sparse_coreg.h): off, every part takes the unfused route
int mi355gp_dbg_sparse_set_fuse_cols(mi355gp_sparse* s, int on) {
    ARG_CHECK(s, "mi355gp_dbg_sparse_set_fuse_cols: NULL context");
    s->fuse_cols = on != 0;
    return 0;
}

// Whether the uncertain-input entry points of this context take one RBF or Linear part with Bias and White parts
// (include/mi355gp_psi_lin.h); on also switches Linear on (prediction at certain points needs it), off leaves that as it is
int mi355gp_sparse_set_psi_lin_bias(mi355gp_sparse* s, int on) {
    ARG_CHECK(s, "mi355gp_sparse_set_psi_lin_bias: NULL context");
    s->take_psi_lin = on != 0;
    if (on) s->take_linear = true;
    return 0;
}

// Kdiag of an expression at the context's rows and its weighted sums (include/mi355gp_sparse_diag.h): the kernels of
// kern_diag.hip on their own, for any expression of the sparse path's kinds with Linear (one without a by-point part is
// described to them all the same).  The expression is parsed into a list of its own: the context's part list, its description
// and coefficients, and with them the last result and what fetch / predict / an SVGP backward call derive from it, stay as
// they are.  Only scratch is shared (dKd, the weights, the block records).
int mi355gp_sparse_kdiag(mi355gp_sparse* s, int nparts, const mi355gp_part* parts, const double* w, double* kd_out,
                         double* sums_out, double* ddiag_out) {
    ARG_CHECK(s && s->n > 0, "mi355gp_sparse_kdiag: set_data first");
    ARG_CHECK(nparts >= 1 && nparts <= KDIAG_MAX_PARTS && parts, "mi355gp_sparse_kdiag: between 1 and 16 kernel parts");
    ARG_CHECK(!sharded(s), "mi355gp_sparse_kdiag: a row-sharded context is not supported (the sums would need a collective)");
    std::vector<PartSpec> ps((size_t)nparts);
    for (int i = 0; i < nparts; ++i) {
        if (int rc = parse_part(parts[i], s->D, KS_STATIONARY | KS_STATIC | KS_LINEAR | (s->take_coreg ? KS_COREG : 0u),
                                "mi355gp_sparse_kdiag", &ps[(size_t)i]))
            return rc;
        if (ps[(size_t)i].coreg())
            if (int rc = coreg_check_data(s, ps[(size_t)i])) return rc;
    }
    const Terms terms = group_terms(ps);
    DiagDesc ds;
    std::vector<double> coef, sums;
    describe_diag(ps, terms, s->D, &ds, &coef);
    HIP_CHECK(hipSetDevice(s->device));
    EngineShared gate(s->device);
    hipStream_t st = s->st;
    const long n = s->n;
    DevBuf dcoef;
    HIP_CHECK(dcoef.alloc(coef.size()));
    HIP_CHECK(hipMemcpyAsync(dcoef, coef.data(), sizeof(double) * coef.size(), hipMemcpyHostToDevice, st));
    if (w) {
        HIP_CHECK(s->diagW.need((size_t)n));
        HIP_CHECK(hipMemcpyAsync(s->diagW, w, sizeof(double) * n, hipMemcpyHostToDevice, st));
    }
    HIP_CHECK(s->dKd.need((size_t)n));
    if (int rc = run_kdiag(s, ds, dcoef, s->dX, n, w ? (const double*)s->diagW : nullptr, s->dKd, &sums)) return rc;
    if (kd_out) HIP_CHECK(hipMemcpyAsync(kd_out, s->dKd, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    if (w && sums_out) sums_out[0] = sums[0], sums_out[1] = sums[1];
    if (w && ddiag_out) {
        std::vector<double> g;
        diag_dtheta(ps, s->D, sums, 1.0, &g);
        for (size_t k = 0; k < g.size(); ++k) ddiag_out[k] = g[k];
    }
    return 0;
}

// HIP-event time of the stream work of the last mi355gp_sparse_predict_uncertain call, in milliseconds
int mi355gp_sparse_get_predict_ms(mi355gp_sparse* s, double* ms_out) {
    ARG_CHECK(s && ms_out, "mi355gp_sparse_get_predict_ms: bad arguments");
    *ms_out = s->predict_ms;
    return 0;
}

}  // extern "C"
