// kgpr.hip -- exact Gaussian GP regression on matrix-shaped data with the covariance K2 (x) K1 + sigma^2 I of two arbitrary kernels
// (C-ABI mi355gp_kgpr_*, include/mi355gp_kgpr.h; GPy/models/gp_kronecker_gaussian_regression.py).  DESIGN.md 6w.
//
// One evaluation, all on the context's stream:
//   eigh_device (eigh.hip) of K1 and of K2 -> U1, S1, U2, S2 (row stride P_d = N_d rounded up to 128, the padding zero, so that
//                   every product below is a launch_gemm on full tiles without a copy);
//   Y_ = U1^T Y U2  two launch_gemm;
//   k_kgpr_spectral one pass over Y_: Wi, Ytilde, the partial sums of the four scalars and of the two weighted marginals; the
//                   partials are combined in a fixed order (launch_reduce_partials, launch_sum_splits) and k_kgpr_weights lays
//                   out the weight strips of the next step;
//   T1 = U1 Ytilde, T2 = U2 Ytilde^T  two launch_gemm;
//   k_kgpr_wsyrk    dL_dK_d = 1/2 T_d diag(S_other) T_d^T - 1/2 U_d diag(r_d) U_d^T: a weighted symmetric rank-k update over two
//                   panels, the weight applied to the B fragment in registers (below).
// Prediction is four more launch_gemm pairs around two elementwise kernels.  Reproducibility: k ascending in every product, every
// partial sum in memory and added in a fixed order, lane trees by xor-shuffle, an integer flag; no floating-point atomics.
#include <cmath>
#include <vector>

#include "../../include/mi355gp_kgpr.h"
#include "eigh.h"
#include "gemm_tile.h"
#include "internal.h"

#define KS_ROWS 32            // rows of Y_ per workgroup of the spectral pass
#define KS_COLS 256           // columns: one per thread
#define KW_STRIP 32           // doubles of a weight strip in LDS: the slab's 16 and the 16 the same DMA brings along
#define KW_WOFF (4 * GT3_OP)  // the two strips lie behind the two operand stages
#define KW_LDS_BYTES (GT3_LDS_BYTES + 2 * KW_STRIP * 8)
#define KG_NEV 12             // events of one evaluation: 11 intervals

__device__ __forceinline__ double kg_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---- the spectral pass ----------------------------------------------------------------------------------------------------
// Workgroup (chunk, panel) owns rows [32 panel, +32) x columns [256 chunk, +256) of Y_ (N1 x N2, row stride ld); a thread owns a
// column and walks the rows, so that a row of the panel is one coalesced read and two coalesced writes.
//   Wi[i][j] = 1 / (S1[i] S2[j] + noise),  Yt = Y_ o Wi
//   spart[block][0..3] = sum log W, sum Y_ Yt, sum Wi, sum Yt^2 over the block
//   r1part[chunk][i]   = sum over the chunk's columns of Wi[i][j] S2[j]     (lane tree, then the four waves in order)
//   r2part[panel][j]   = sum over the panel's rows of Wi[i][j] S1[i]        (the thread's own running sum, rows ascending)
// A W that is not positive (or not finite) raises *flag; what the block computed from it is then never looked at.
__global__ __launch_bounds__(256) void k_kgpr_spectral(const double* __restrict__ Yr, long ld, long N1, long N2,
                                                       const double* __restrict__ S1, const double* __restrict__ S2, double noise,
                                                       double* __restrict__ Wi, double* __restrict__ Yt, double* __restrict__ spart,
                                                       double* __restrict__ r1part, long P1, double* __restrict__ r2part, long P2,
                                                       int* __restrict__ flag) {
    __shared__ double rw[KS_ROWS][4];
    __shared__ double sred[4][4];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const long j = (long)blockIdx.x * KS_COLS + t, i0 = (long)blockIdx.y * KS_ROWS;
    const bool in = j < N2;
    const double s2 = in ? S2[j] : 0.0;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, c2 = 0.0;
    int bad = 0;
    for (int ii = 0; ii < KS_ROWS; ++ii) {
        const long i = i0 + ii;
        double v = 0.0;
        if (i < N1 && in) {
            const double s1 = S1[i], W = s1 * s2 + noise;
            if (!(W > 0.0) || !(W < INFINITY)) bad = 1;
            const double wi = 1.0 / W, y = Yr[i * ld + j], yt = y * wi;
            Wi[i * ld + j] = wi;
            Yt[i * ld + j] = yt;
            a0 += log(W);
            a1 += y * yt;
            a2 += wi;
            a3 += yt * yt;
            c2 += wi * s1;
            v = wi * s2;
        }
        v = kg_wave_sum(v);
        if (lane == 0) rw[ii][w] = v;
    }
    if (j < P2) r2part[(long)blockIdx.y * P2 + j] = c2;
    a0 = kg_wave_sum(a0);
    a1 = kg_wave_sum(a1);
    a2 = kg_wave_sum(a2);
    a3 = kg_wave_sum(a3);
    if (lane == 0) {
        sred[w][0] = a0;
        sred[w][1] = a1;
        sred[w][2] = a2;
        sred[w][3] = a3;
    }
    if (bad) atomicOr(flag, 1);
    __syncthreads();
    if (t < KS_ROWS && i0 + t < P1) r1part[(long)blockIdx.x * P1 + i0 + t] = ((rw[t][0] + rw[t][1]) + rw[t][2]) + rw[t][3];
    if (t < 4) spart[((long)blockIdx.y * gridDim.x + blockIdx.x) * 4 + t] = ((sred[0][t] + sred[1][t]) + sred[2][t]) + sred[3][t];
}

// The weight strip of one k_kgpr_wsyrk launch: [sa[0 .. na) | zeros to a multiple of 16 | -r[0 .. nb) | zeros to a multiple of 16 | 16 zeros]
__global__ __launch_bounds__(256) void k_kgpr_weights(const double* __restrict__ sa, long na, const double* __restrict__ r, long nb,
                                                      double* __restrict__ wcat) {
    const long ka = (na + 15) / 16 * 16, kb = (nb + 15) / 16 * 16;
    const long s = (long)blockIdx.x * 256 + threadIdx.x;
    if (s >= ka + kb + 16) return;
    double v = 0.0;
    if (s < na) v = sa[s];
    else if (s >= ka && s - ka < nb) v = -r[s - ka];
    wcat[s] = v;
}

__global__ void k_kgpr_clear_flag(int* flag) { *flag = 0; }

// ---- the weighted symmetric rank-k update ------------------------------------------------------------------------------------
// C = 1/2 sum_s w[s] P[i][s] P[j][s], s running first over the nsa slabs of panel Pa, then over the nsb slabs of panel Pb (k-contiguous,
// row strides lda / ldb, zero-padded to whole slabs and to whole 128-row tiles; w = wcat of k_kgpr_weights, slab s at wcat + 16 s).
// Geometry of gemm_tile.h: one lower 128 x 128 tile (I >= J) per workgroup, four waves 2 x 2, 4 x 4 accumulators of
// v_mfma_f64_16x16x4 per wave, slabs of 16 through two LDS stages by LDS-DMA with the source-side swizzle gt3_h.  Its own k-loop:
//   * both operands of a slab come from the SAME panel (rows of tile I and rows of tile J); the slab counter rolls from panel a to
//     panel b without draining the pipeline, and a slab never straddles the two;
//   * the operands arrive by DMA, so the weight cannot be applied on the way in.  Wave 0 brings the slab's weights with a ninth
//     DMA (4 bytes per lane: 32 doubles, the slab's 16 and the next 16, which nobody reads) into a strip behind the operand
//     stages, under the same vmcnt(0) + barrier as the operands.  A lane holds B[k = 4 kq + 2 e + s][n] for its two slices of the
//     half-slab e, so it reads the four weights at 4 kq as two 16-byte words and scales its B fragments in registers: 16 v_mul_f64
//     against 64 MFMAs per slab and wave.  No scaled copy of a panel exists in memory.
// The epilogue halves the accumulators and stores an off-diagonal tile together with its transpose; a diagonal tile stores the
// elements with row >= column and mirrors them (its two triangles differ in rounding: a_i (w a_j) against a_j (w a_i)), so C is
// exactly symmetric.  C is np x np with np = 128 nt: every tile is whole.
__global__ __launch_bounds__(256, 2) void k_kgpr_wsyrk(const double* __restrict__ Pa, long lda, int nsa, const double* __restrict__ Pb,
                                                       long ldb, int nsb, const double* __restrict__ wcat, double* __restrict__ C,
                                                       long ldc) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int bid = blockIdx.x;
    int ti = (int)((sqrtf(8.0f * (float)bid + 1.0f) - 1.0f) * 0.5f);
    while ((long)ti * (ti + 1) / 2 > bid) --ti;
    while ((long)(ti + 1) * (ti + 2) / 2 <= bid) ++ti;
    const int tj = bid - (int)((long)ti * (ti + 1) / 2);
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, wr = w >> 1, wc = w & 1, kq = lane >> 4;
    const int nk = nsa + nsb;
    auto rsrc = [](const double* p) {
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(p), 0, 0x7fffffff, 0x00020000);
    };
    int va[4], vb[4];
    gt3_src_offsets<true>(lda, lane, w, va);
    gt3_src_offsets<true>(ldb, lane, w, vb);
    const double* Ai = Pa + (long)ti * NB * lda;
    const double* Aj = Pa + (long)tj * NB * lda;
    const double* Bi = Pb + (long)ti * NB * ldb;
    const double* Bj = Pb + (long)tj * NB * ldb;
    // slab s into stage st: the rows of tile I, the rows of tile J, the weights
    auto issue = [&](int s, int st) {
        double* dst = smem + st * 2 * GT3_OP;
        if (s < nsa) {
            gt3_issue<true>(rsrc(Ai + (long)s * 16), va, 0, dst, w);
            gt3_issue<true>(rsrc(Aj + (long)s * 16), va, 0, dst + GT3_OP, w);
        } else {
            gt3_issue<true>(rsrc(Bi + (long)(s - nsa) * 16), vb, 0, dst, w);
            gt3_issue<true>(rsrc(Bj + (long)(s - nsa) * 16), vb, 0, dst + GT3_OP, w);
        }
        if (w == 0) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc(wcat + (long)s * 16), smem + KW_WOFF + st * KW_STRIP, 4, lane * 4, 0, 0, 0);
    };
    const int arow = wr * 64 + (lane & 15), bcol = wc * 64 + (lane & 15);
    int fa0[4], fb0[4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
        fa0[mi] = (arow + mi * 16) * 16;
        fb0[mi] = (bcol + mi * 16) * 16;
    }
    const int ha = gt3_h(arow), hb = gt3_h(bcol);
    d4 acc[4][4];
    gt_zero<4>(acc);
    issue(0, 0);
    __builtin_amdgcn_s_waitcnt(0x0F70);                      // vmcnt(0): the DMAs have landed
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) issue(kt + 1, cur ^ 1);
        const double* a_s = smem + cur * 2 * GT3_OP;
        const double* b_s = a_s + GT3_OP;
        const double* w_s = smem + KW_WOFF + cur * KW_STRIP + 4 * kq;
#pragma unroll
        for (int e = 0; e < 2; ++e) {                        // slices 2e, 2e+1: physical k = 4 kq + 2 e + s
            d2 af[4], bf[4];
            const d2 wv = *reinterpret_cast<const d2*>(w_s + 2 * e);
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) af[mi] = *reinterpret_cast<const d2*>(a_s + fa0[mi] + 2 * ((2 * kq + e) ^ ha));
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) bf[ni] = *reinterpret_cast<const d2*>(b_s + fb0[ni] + 2 * ((2 * kq + e) ^ hb)) * wv;
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                    for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = mfma_f64(af[mi][s], bf[ni][s], acc[mi][ni]);
        }
        __builtin_amdgcn_s_waitcnt(0x0F70);                  // vmcnt(0) before the barrier: slab kt+1 is in LDS
        __syncthreads();
    }
    // element (mi, ni, r) of this lane: row wr 64 + mi 16 + 4 r + (lane >> 4), column wc 64 + ni 16 + (lane & 15) of the tile
    const long r0 = (long)ti * NB + wr * 64 + (lane >> 4), c0 = (long)tj * NB + wc * 64 + (lane & 15);
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long row = r0 + mi * 16 + 4 * r, col = c0 + ni * 16;
                const double v = 0.5 * acc[mi][ni][r];
                if (ti != tj || row >= col) {
                    C[row * ldc + col] = v;
                    C[col * ldc + row] = v;
                }
            }
}

static int launch_kgpr_wsyrk(hipStream_t st, const double* Pa, long lda, long ka16, const double* Pb, long ldb, long kb16,
                             const double* wcat, double* C, long np) {
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_kgpr_wsyrk), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  KW_LDS_BYTES));
    const long nt = np / NB;
    hipLaunchKernelGGL(k_kgpr_wsyrk, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(256), KW_LDS_BYTES, st, Pa, lda, (int)(ka16 / 16), Pb,
                       ldb, (int)(kb16 / 16), wcat, C, np);
    HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- prediction's two elementwise kernels -------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_kgpr_square(double* __restrict__ A, long cnt) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < cnt) A[i] = A[i] * A[i];
}

// mu[i + M1 j] = MU[i][j],  var[i + M1 j] = k1xx[i] k2xx[j] - V[i][j] + noise   (MU, V: row stride ld; a thread per (i, j), i fastest)
__global__ __launch_bounds__(256) void k_kgpr_pred_out(const double* __restrict__ MU, const double* __restrict__ V, long ld, long M1,
                                                       long M2, const double* __restrict__ k1xx, const double* __restrict__ k2xx,
                                                       double noise, double* __restrict__ mu, double* __restrict__ var) {
    const long f = (long)blockIdx.x * 256 + threadIdx.x;
    if (f >= M1 * M2) return;
    const long i = f % M1, j = f / M1;
    mu[f] = MU[i * ld + j];
    var[f] = k1xx[i] * k2xx[j] - V[i * ld + j] + noise;
}

// ---- the context ---------------------------------------------------------------------------------------------------------------
struct mi355gp_kgpr {
    int device = 0;
    hipStream_t st = nullptr;
    hipEvent_t ev[KG_NEV] = {};
    long N1 = 0, N2 = 0, P1 = 0, P2 = 0, Pm = 0;
    int nchunk = 0, npanel = 0;
    DevBuf Y, Z, Yr, Yt, Wi;                     // P1 x P2 each; Z is the work matrix (U1^T Y, then T1), Yr holds Y_ and then T2 (P2 x P1)
    DevBuf U1, U2, S1, S2, KG;                   // P1^2, P2^2, P1, P2, max(P1, P2)^2: K on the way in (dense), dL_dK on the way out
    DevBuf spart, scal, r1part, r2part, r1, r2, wc1, wc2;
    DevArr<int> flag;
    EighWs ws1, ws2;
    double noise = 0.0, ms[MI355GP_KGPR_NUM_MS] = {};
    bool have_data = false, solved = false;
};

static size_t kgpr_doubles(long N1, long N2) {
    const size_t P1 = round_up(N1, NB), P2 = round_up(N2, NB), L1 = round_up(N1, MI355GP_EIGH_B), L2 = round_up(N2, MI355GP_EIGH_B);
    const size_t Pm = P1 > P2 ? P1 : P2;
    return 2 * L1 * L1 + 2 * L2 * L2 + 1100 * (L1 + L2) + P1 * P1 + P2 * P2 + Pm * Pm + 5 * P1 * P2 + (P1 / KS_ROWS + 2) * P2 +
           (P2 / KS_COLS + 2) * P1;
}

static int kgpr_eigh(mi355gp_kgpr* c, const double* K, long n, double* S, double* U, long P, EighWs* ws, int which, int* sweeps) {
    HIP_CHECK(hipMemcpyAsync(c->KG, K, sizeof(double) * n * n, hipMemcpyHostToDevice, c->st));
    HIP_CHECK(hipEventRecord(c->ev[2 * which - 1], c->st));
    const int info = eigh_device(c->st, c->KG, n, n, S, U, P, ws, sweeps);
    if (info < 0) return info;
    if (info == 1) {
        mi355gp_set_error("mi355gp_kgpr_inference: the eigendecomposition of K%d (%ld x %ld) did not converge within the cap of %d sweeps",
                          which, n, n, MI355GP_EIGH_MAX_SWEEPS);
        return -3;
    }
    HIP_CHECK(hipEventRecord(c->ev[2 * which], c->st));
    return 0;
}

// dL_dK (n x n, host) = 1/2 T diag(sa) T^T - 1/2 U diag(r) U^T through KG; e: the index of the event before the launch
static int kgpr_grad(mi355gp_kgpr* c, const double* T, long ldt, long na, const double* U, long P, long n, const double* wcat,
                     double* out, int e) {
    if (int rc = launch_kgpr_wsyrk(c->st, T, ldt, round_up(na, 16), U, P, round_up(n, 16), wcat, c->KG, P)) return rc;
    HIP_CHECK(hipEventRecord(c->ev[e + 1], c->st));
    HIP_CHECK(hipMemcpy2DAsync(out, sizeof(double) * n, c->KG, sizeof(double) * P, sizeof(double) * n, n, hipMemcpyDeviceToHost, c->st));
    HIP_CHECK(hipEventRecord(c->ev[e + 2], c->st));
    return 0;
}

extern "C" {

int mi355gp_kgpr_create(int device, mi355gp_kgpr** out) {
    ARG_CHECK(out != nullptr, "mi355gp_kgpr_create: out is NULL");
    int n = 0;
    mi355gp_device_count(&n);
    if (device < 0 || device >= n) {
        mi355gp_set_error("mi355gp_kgpr_create: device %d not available (%d HIP devices visible)", device, n);
        return -2;
    }
    HIP_CHECK(hipSetDevice(device));
    mi355gp_kgpr* c = new mi355gp_kgpr();
    c->device = device;
    *out = c;                                    // destroy releases whatever was made if a later step fails
    HIP_CHECK(hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking));
    for (hipEvent_t& e : c->ev) HIP_CHECK(hipEventCreate(&e));
    HIP_CHECK(c->scal.alloc(4));
    HIP_CHECK(c->flag.alloc(1));
    return 0;
}

int mi355gp_kgpr_destroy(mi355gp_kgpr* c) {
    if (!c) return 0;
    (void)hipSetDevice(c->device);
    if (c->st) {
        (void)hipStreamSynchronize(c->st);
        (void)hipStreamDestroy(c->st);
    }
    for (hipEvent_t e : c->ev)
        if (e) (void)hipEventDestroy(e);
    delete c;
    return 0;
}

int mi355gp_kgpr_set_data(mi355gp_kgpr* c, const double* Y, int64_t N1, int64_t N2) {
    ARG_CHECK(c && Y, "mi355gp_kgpr_set_data: NULL argument");
    if (N1 < 1 || N2 < 1 || N1 > MI355GP_EIGH_MAX_N || N2 > MI355GP_EIGH_MAX_N) {
        mi355gp_set_error("mi355gp_kgpr_set_data: Y is %lld x %lld, each side has 1 to %d rows", (long long)N1,
                          (long long)N2, MI355GP_EIGH_MAX_N);
        return -1;
    }
    for (int64_t i = 0; i < N1 * N2; ++i)
        if (!std::isfinite(Y[i])) {
            mi355gp_set_error("mi355gp_kgpr_set_data: Y has an entry that is not finite (row %lld, column %lld)", (long long)(i / N2),
                              (long long)(i % N2));
            return -1;
        }
    HIP_CHECK(hipSetDevice(c->device));
    HIP_CHECK(hipStreamSynchronize(c->st));
    c->have_data = c->solved = false;
    DevBuf* all[] = {&c->Y, &c->Z, &c->Yr, &c->Yt, &c->Wi, &c->U1, &c->U2, &c->S1, &c->S2, &c->KG, &c->spart, &c->r1part, &c->r2part,
                     &c->r1, &c->r2, &c->wc1, &c->wc2};
    for (DevBuf* b : all) *b = DevBuf();         // what an earlier data set held is released before the new need is judged
    c->ws1 = EighWs();
    c->ws2 = EighWs();
    size_t free_b = 0, total_b = 0;
    HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    const size_t need = kgpr_doubles(N1, N2) * sizeof(double);
    if (need > free_b) {
        mi355gp_set_error("mi355gp_kgpr_set_data: the workspaces of a %lld x %lld problem need %zu bytes of device memory, %zu are free",
                          (long long)N1, (long long)N2, need, free_b);
        return -5;
    }
    const long P1 = round_up(N1, NB), P2 = round_up(N2, NB), Pm = P1 > P2 ? P1 : P2;
    c->N1 = N1;
    c->N2 = N2;
    c->P1 = P1;
    c->P2 = P2;
    c->Pm = Pm;
    c->nchunk = (int)((N2 + KS_COLS - 1) / KS_COLS);
    c->npanel = (int)((N1 + KS_ROWS - 1) / KS_ROWS);
    if (int rc = eigh_ws_alloc(&c->ws1, N1)) return rc;
    if (int rc = eigh_ws_alloc(&c->ws2, N2)) return rc;
    // zeroed once: the padding of these is never written afterwards (the GEMM outputs Z and Yr are written whole every time)
    struct { DevBuf* b; size_t cnt; } zeroed[] = {{&c->Y, (size_t)P1 * P2},  {&c->Yt, (size_t)P1 * P2}, {&c->Wi, (size_t)P1 * P2},
                                                  {&c->U1, (size_t)P1 * P1}, {&c->U2, (size_t)P2 * P2}, {&c->S1, (size_t)P1},
                                                  {&c->S2, (size_t)P2}};
    for (auto& z : zeroed) {
        HIP_CHECK(z.b->alloc(z.cnt));
        HIP_CHECK(hipMemsetAsync(*z.b, 0, sizeof(double) * z.cnt, c->st));
    }
    HIP_CHECK(c->Z.alloc((size_t)P1 * P2));
    HIP_CHECK(c->Yr.alloc((size_t)P1 * P2));
    HIP_CHECK(c->KG.alloc((size_t)Pm * Pm));
    HIP_CHECK(c->spart.alloc((size_t)c->nchunk * c->npanel * 4));
    HIP_CHECK(c->r1part.alloc((size_t)c->nchunk * P1));
    HIP_CHECK(c->r2part.alloc((size_t)c->npanel * P2));
    HIP_CHECK(c->r1.alloc(P1));
    HIP_CHECK(c->r2.alloc(P2));
    HIP_CHECK(c->wc1.alloc((size_t)P1 + P2 + 64));
    HIP_CHECK(c->wc2.alloc((size_t)P1 + P2 + 64));
    HIP_CHECK(hipMemcpy2DAsync(c->Y, sizeof(double) * P2, Y, sizeof(double) * N2, sizeof(double) * N2, N1, hipMemcpyHostToDevice, c->st));
    HIP_CHECK(hipStreamSynchronize(c->st));
    c->have_data = true;
    return 0;
}

int mi355gp_kgpr_inference(mi355gp_kgpr* c, const double* K1, const double* K2, double noise, double* scalars, double* dL_dK1,
                           double* dL_dK2, int* sweeps) {
    ARG_CHECK(c && K1 && K2 && scalars && dL_dK1 && dL_dK2, "mi355gp_kgpr_inference: NULL argument");
    ARG_CHECK(c->have_data, "mi355gp_kgpr_inference: no data (mi355gp_kgpr_set_data)");
    if (!(noise > 0.0) || !std::isfinite(noise)) {
        mi355gp_set_error("mi355gp_kgpr_inference: the noise variance must be positive and finite, got %g", noise);
        return -1;
    }
    HIP_CHECK(hipSetDevice(c->device));
    const long N1 = c->N1, N2 = c->N2, P1 = c->P1, P2 = c->P2;
    hipStream_t st = c->st;
    c->solved = false;
    c->noise = noise;
    HIP_CHECK(hipEventRecord(c->ev[0], st));
    if (int rc = kgpr_eigh(c, K1, N1, c->S1, c->U1, P1, &c->ws1, 1, sweeps)) return rc;                 // events 1, 2
    if (int rc = kgpr_eigh(c, K2, N2, c->S2, c->U2, P2, &c->ws2, 2, sweeps ? sweeps + 1 : nullptr)) return rc;   // events 3, 4
    launch_gemm(st, 1, 1, P1, P2, P1, c->U1, P1, c->Y, P2, c->Z, P2, 1.0, 0.0);                         // Z = U1^T Y
    launch_gemm(st, 0, 1, P1, P2, P2, c->Z, P2, c->U2, P2, c->Yr, P2, 1.0, 0.0);                        // Y_ = Z U2
    HIP_CHECK(hipEventRecord(c->ev[5], st));
    hipLaunchKernelGGL(k_kgpr_clear_flag, dim3(1), dim3(1), 0, st, (int*)c->flag);
    hipLaunchKernelGGL(k_kgpr_spectral, dim3(c->nchunk, c->npanel), dim3(256), 0, st, (const double*)c->Yr, P2, N1, N2,
                       (const double*)c->S1, (const double*)c->S2, noise, (double*)c->Wi, (double*)c->Yt, (double*)c->spart,
                       (double*)c->r1part, P1, (double*)c->r2part, P2, (int*)c->flag);
    launch_reduce_partials(st, c->spart, c->nchunk * c->npanel, 4, c->scal);
    launch_sum_splits(st, c->r1part, P1, c->nchunk, 0, c->r1);
    launch_sum_splits(st, c->r2part, P2, c->npanel, 0, c->r2);
    const long k1 = round_up(N1, 16), k2 = round_up(N2, 16);
    hipLaunchKernelGGL(k_kgpr_weights, dim3((unsigned)((k1 + k2 + 16 + 255) / 256)), dim3(256), 0, st, (const double*)c->S2, N2,
                       (const double*)c->r1, N1, (double*)c->wc1);
    hipLaunchKernelGGL(k_kgpr_weights, dim3((unsigned)((k1 + k2 + 16 + 255) / 256)), dim3(256), 0, st, (const double*)c->S1, N1,
                       (const double*)c->r2, N2, (double*)c->wc2);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(c->ev[6], st));
    launch_gemm(st, 0, 1, P1, P2, P1, c->U1, P1, c->Yt, P2, c->Z, P2, 1.0, 0.0);                        // T1 = U1 Ytilde      (P1 x P2)
    launch_gemm(st, 0, 0, P2, P1, P2, c->U2, P2, c->Yt, P2, c->Yr, P1, 1.0, 0.0);                       // T2 = U2 Ytilde^T    (P2 x P1)
    HIP_CHECK(hipEventRecord(c->ev[7], st));
    if (int rc = kgpr_grad(c, c->Z, P2, N2, c->U1, P1, N1, c->wc1, dL_dK1, 7)) return rc;               // events 8, 9
    if (int rc = kgpr_grad(c, c->Yr, P1, N1, c->U2, P2, N2, c->wc2, dL_dK2, 9)) return rc;              // events 10, 11
    double h[4];
    int flag = 0;
    HIP_CHECK(hipMemcpyAsync(h, c->scal, sizeof(h), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(&flag, c->flag, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (flag) {
        mi355gp_set_error("mi355gp_kgpr_inference: W = S1[i] S2[j] + sigma^2 is not positive somewhere (an eigenvalue at -tiny under the "
                          "noise variance %g): raise the noise variance", noise);
        return -4;
    }
    scalars[0] = -0.5 * (double)N1 * (double)N2 * log(2.0 * M_PI) - 0.5 * h[0] - 0.5 * h[1];
    scalars[1] = -0.5 * h[2] + 0.5 * h[3];
    // intervals between the events: 0 up, 1 eigh, 2 up, 3 eigh, 4 rot, 5 spectral, 6 rot, 7 wsyrk, 8 down, 9 wsyrk, 10 down
    static const int kind[KG_NEV - 1] = {4, 0, 4, 0, 1, 2, 1, 3, 4, 3, 4};
    for (int i = 0; i < 8; ++i) c->ms[i] = 0.0;             // [8] belongs to predict
    for (int i = 0; i + 1 < KG_NEV; ++i) {
        float t = 0.f;
        HIP_CHECK(hipEventElapsedTime(&t, c->ev[i], c->ev[i + 1]));
        c->ms[kind[i]] += t;
        c->ms[5] += t;
        if (i == 7) c->ms[6] = t;
        if (i == 9) c->ms[7] = t;
    }
    c->solved = true;
    return 0;
}

int mi355gp_kgpr_predict(mi355gp_kgpr* c, const double* k1xf, int64_t M1, const double* k2xf, int64_t M2, const double* k1xx,
                         const double* k2xx, double* mu, double* var) {
    ARG_CHECK(c && k1xf && k2xf && k1xx && k2xx && mu && var, "mi355gp_kgpr_predict: NULL argument");
    ARG_CHECK(c->solved, "mi355gp_kgpr_predict: no evaluation to predict from (mi355gp_kgpr_inference)");
    if (M1 < 1 || M2 < 1 || M1 > MI355GP_EIGH_MAX_N || M2 > MI355GP_EIGH_MAX_N) {
        mi355gp_set_error("mi355gp_kgpr_predict: %lld x %lld new points, each side takes 1 to %d", (long long)M1, (long long)M2,
                          MI355GP_EIGH_MAX_N);
        return -1;
    }
    HIP_CHECK(hipSetDevice(c->device));
    const long N1 = c->N1, N2 = c->N2, P1 = c->P1, P2 = c->P2, Q1 = round_up(M1, NB), Q2 = round_up(M2, NB);
    hipStream_t st = c->st;
    DevBuf F1, F2, A, B, AY, MU, V, d1, d2v, dmu, dvar;      // released on every return path
    HIP_CHECK(F1.alloc((size_t)Q1 * P1));
    HIP_CHECK(F2.alloc((size_t)Q2 * P2));
    HIP_CHECK(A.alloc((size_t)Q1 * P1));
    HIP_CHECK(B.alloc((size_t)Q2 * P2));
    HIP_CHECK(AY.alloc((size_t)Q1 * P2));
    HIP_CHECK(MU.alloc((size_t)Q1 * Q2));
    HIP_CHECK(V.alloc((size_t)Q1 * Q2));
    HIP_CHECK(d1.alloc(M1));
    HIP_CHECK(d2v.alloc(M2));
    HIP_CHECK(dmu.alloc((size_t)M1 * M2));
    HIP_CHECK(dvar.alloc((size_t)M1 * M2));
    HIP_CHECK(hipEventRecord(c->ev[0], st));
    HIP_CHECK(hipMemsetAsync(F1, 0, sizeof(double) * Q1 * P1, st));
    HIP_CHECK(hipMemsetAsync(F2, 0, sizeof(double) * Q2 * P2, st));
    HIP_CHECK(hipMemcpy2DAsync(F1, sizeof(double) * P1, k1xf, sizeof(double) * N1, sizeof(double) * N1, M1, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpy2DAsync(F2, sizeof(double) * P2, k2xf, sizeof(double) * N2, sizeof(double) * N2, M2, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(d1, k1xx, sizeof(double) * M1, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(d2v, k2xx, sizeof(double) * M2, hipMemcpyHostToDevice, st));
    launch_gemm(st, 0, 1, Q1, P1, P1, F1, P1, c->U1, P1, A, P1, 1.0, 0.0);                              // A = k1xf U1
    launch_gemm(st, 0, 1, Q2, P2, P2, F2, P2, c->U2, P2, B, P2, 1.0, 0.0);                              // B = k2xf U2
    launch_gemm(st, 0, 1, Q1, P2, P1, A, P1, c->Yt, P2, AY, P2, 1.0, 0.0);                              // A Ytilde
    launch_gemm(st, 0, 0, Q1, Q2, P2, AY, P2, B, P2, MU, Q2, 1.0, 0.0);                                 // (A Ytilde) B^T
    hipLaunchKernelGGL(k_kgpr_square, dim3((unsigned)((Q1 * P1 + 255) / 256)), dim3(256), 0, st, (double*)A, Q1 * P1);
    hipLaunchKernelGGL(k_kgpr_square, dim3((unsigned)((Q2 * P2 + 255) / 256)), dim3(256), 0, st, (double*)B, Q2 * P2);
    launch_gemm(st, 0, 1, Q1, P2, P1, A, P1, c->Wi, P2, AY, P2, 1.0, 0.0);                              // (A o A) Wi
    launch_gemm(st, 0, 0, Q1, Q2, P2, AY, P2, B, P2, V, Q2, 1.0, 0.0);                                  // ((A o A) Wi) (B o B)^T
    hipLaunchKernelGGL(k_kgpr_pred_out, dim3((unsigned)((M1 * M2 + 255) / 256)), dim3(256), 0, st, (const double*)MU, (const double*)V,
                       Q2, (long)M1, (long)M2, (const double*)d1, (const double*)d2v, c->noise, (double*)dmu, (double*)dvar);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(mu, dmu, sizeof(double) * M1 * M2, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(var, dvar, sizeof(double) * M1 * M2, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipEventRecord(c->ev[1], st));
    HIP_CHECK(hipStreamSynchronize(st));
    float t = 0.f;
    HIP_CHECK(hipEventElapsedTime(&t, c->ev[0], c->ev[1]));
    c->ms[8] = t;
    return 0;
}

int mi355gp_kgpr_fetch(mi355gp_kgpr* c, int which, double* out) {
    ARG_CHECK(c && out, "mi355gp_kgpr_fetch: NULL argument");
    ARG_CHECK(c->solved, "mi355gp_kgpr_fetch: no evaluation to fetch from (mi355gp_kgpr_inference)");
    HIP_CHECK(hipSetDevice(c->device));
    const double* src = nullptr;
    long rows = 1, cols = 0, ld = 0;
    switch (which) {
        case MI355GP_KGPR_FETCH_U1: src = c->U1, rows = cols = c->N1, ld = c->P1; break;
        case MI355GP_KGPR_FETCH_U2: src = c->U2, rows = cols = c->N2, ld = c->P2; break;
        case MI355GP_KGPR_FETCH_S1: src = c->S1, cols = ld = c->N1; break;
        case MI355GP_KGPR_FETCH_S2: src = c->S2, cols = ld = c->N2; break;
        case MI355GP_KGPR_FETCH_YTILDE: src = c->Yt, rows = c->N1, cols = c->N2, ld = c->P2; break;
        case MI355GP_KGPR_FETCH_WI: src = c->Wi, rows = c->N1, cols = c->N2, ld = c->P2; break;
        default:
            mi355gp_set_error("mi355gp_kgpr_fetch: which = %d names no result (0 .. 5)", which);
            return -1;
    }
    HIP_CHECK(hipMemcpy2DAsync(out, sizeof(double) * cols, src, sizeof(double) * ld, sizeof(double) * cols, rows, hipMemcpyDeviceToHost,
                               c->st));
    HIP_CHECK(hipStreamSynchronize(c->st));
    return 0;
}

int mi355gp_kgpr_get_ms(mi355gp_kgpr* c, double* ms_out) {
    ARG_CHECK(c && ms_out, "mi355gp_kgpr_get_ms: NULL argument");
    for (int i = 0; i < MI355GP_KGPR_NUM_MS; ++i) ms_out[i] = c->ms[i];
    return 0;
}

int mi355gp_kgpr_wsyrk(int device, int64_t n, const double* Pa, int64_t ka, const double* da, const double* Pb, int64_t kb,
                       const double* db, double* C, int reps, double* ms) {
    ARG_CHECK(Pa && da && Pb && db && C, "mi355gp_kgpr_wsyrk: NULL argument");
    if (n < 1 || n > MI355GP_EIGH_MAX_N || ka < 1 || kb < 1 || ka > 2 * MI355GP_EIGH_MAX_N || kb > 2 * MI355GP_EIGH_MAX_N) {
        mi355gp_set_error("mi355gp_kgpr_wsyrk: n = %lld (1 .. %d), ka = %lld, kb = %lld (1 .. %d)", (long long)n, MI355GP_EIGH_MAX_N,
                          (long long)ka, (long long)kb, 2 * MI355GP_EIGH_MAX_N);
        return -1;
    }
    HIP_CHECK(hipSetDevice(device));
    const long np = round_up(n, NB), ka16 = round_up(ka, 16), kb16 = round_up(kb, 16);
    std::vector<double> w(ka16 + kb16 + 16, 0.0);
    for (long s = 0; s < ka; ++s) w[s] = da[s];
    for (long s = 0; s < kb; ++s) w[ka16 + s] = db[s];
    DevBuf dA, dB, dW, dC;                                   // released on every return path
    HIP_CHECK(dA.alloc((size_t)np * ka16));
    HIP_CHECK(dB.alloc((size_t)np * kb16));
    HIP_CHECK(dW.alloc(w.size()));
    HIP_CHECK(dC.alloc((size_t)np * np));
    struct Events {
        hipEvent_t e[2] = {nullptr, nullptr};
        ~Events() {
            for (hipEvent_t ev : e)
                if (ev) (void)hipEventDestroy(ev);
        }
    } ev;
    HIP_CHECK(hipEventCreate(&ev.e[0]));
    HIP_CHECK(hipEventCreate(&ev.e[1]));
    HIP_CHECK(hipMemset(dA, 0, sizeof(double) * np * ka16));
    HIP_CHECK(hipMemset(dB, 0, sizeof(double) * np * kb16));
    HIP_CHECK(hipMemcpy2D(dA, sizeof(double) * ka16, Pa, sizeof(double) * ka, sizeof(double) * ka, n, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy2D(dB, sizeof(double) * kb16, Pb, sizeof(double) * kb, sizeof(double) * kb, n, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dW, w.data(), sizeof(double) * w.size(), hipMemcpyHostToDevice));
    if (reps < 1) reps = 1;
    HIP_CHECK(hipEventRecord(ev.e[0], 0));
    for (int i = 0; i < reps; ++i)
        if (int rc = launch_kgpr_wsyrk(0, dA, ka16, ka16, dB, kb16, kb16, dW, dC, np)) return rc;
    HIP_CHECK(hipEventRecord(ev.e[1], 0));
    HIP_CHECK(hipMemcpy2D(C, sizeof(double) * n, dC, sizeof(double) * np, sizeof(double) * n, n, hipMemcpyDeviceToHost));
    if (ms) {
        float t = 0.f;
        HIP_CHECK(hipEventElapsedTime(&t, ev.e[0], ev.e[1]));
        *ms = (double)t / reps;
    }
    return 0;
}

}   // extern "C"
