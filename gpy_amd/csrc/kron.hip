// kron.hip -- exact Gaussian GP regression on a full Cartesian grid (C-ABI mi355gp_kron_*, include/mi355gp_kron.h): the covariance
// is K_1 (x) ... (x) K_D, and everything of GPy/inference/latent_function_inference/gaussian_grid_inference.py:50-114 and of the
// prediction of GPy/core/gp_grid.py:87-116 is a chain of tensor mode products on N-vectors (N = prod G_d, 64-bit indices).  The
// context holds y, alpha and two ping-pong work vectors; nothing of size N x anything exists.  DESIGN.md 6q.
//
// One mode product (k_kron_mode) is one step of the reference's kron_mvprod (:35-48) with the transpose folded into the store: the
// current vector is a row-major P x G matrix x (the contracted index fastest), the factor A is R x G, the result is the row-major
// R x P matrix out[r][p] = sum_k A[r][k] x[p][k].  After D steps, last dimension first, the original ordering is back.
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/mi355gp_kron.h"
#include "common.h"

#define KM_PT 64          // p per workgroup: 16 per wave, the 16 columns of a v_mfma_f64_16x16x4 result
#define KM_RT 128         // output rows per workgroup: 8 MFMA row tiles, 8 accumulator quads per lane
#define KM_KS 32          // k per LDS slab: 8 MFMA steps
#define KM_LD (KM_KS + 1) // LDS row stride (doubles): odd, so the 16 rows a wave reads at one k start in 16 different banks
#define KR_MAXB 1024      // partial sums of stage one of every reduction
#define KR_NRED 2         // sums carried by one reduction launch, each as a pair (sum, error term)

// out[r][p] = sum_k A[r][k] x[p][k] for one (panel of 64 p, chunk of 128 r).  Wave w owns p = p0 + 16 w .. + 15 and all 128 rows:
// the MFMA's A operand is the factor (row = r, k), its B operand is x (k, col = p), so a lane holds out[r = (l >> 4) + 4 i + 16 t]
// [p = l & 15] and the 16 lanes of a row write 128 contiguous bytes.  Both operands go through LDS, read from memory k-contiguous
// and zero-filled outside (G, R, P), so any G, R, P >= 1 runs the same code.  Every output element accumulates its k in ascending
// order (slab after slab, four k per MFMA) whatever the grid: the bits do not depend on how panels are dealt out.
__global__ __launch_bounds__(256) void k_kron_mode(const double* __restrict__ A, int transA, const double* __restrict__ x,
                                                   double* __restrict__ out, long long P, int G, int R) {
    __shared__ double sa[KM_RT * KM_LD];
    __shared__ double sx[KM_PT * KM_LD];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const long long p0 = (long long)blockIdx.x * KM_PT;
    const int r0 = blockIdx.y * KM_RT;
    d4 acc[KM_RT / 16];
#pragma unroll
    for (int i = 0; i < KM_RT / 16; ++i) acc[i] = (d4){0.0, 0.0, 0.0, 0.0};
    const int kk = t & (KM_KS - 1), row = t >> 5;           // staging: 32 consecutive k of one row per 32 threads
    for (int k0 = 0; k0 < G; k0 += KM_KS) {
        __syncthreads();                                    // the previous slab's operand reads are done
        const int k = k0 + kk;
#pragma unroll
        for (int i = 0; i < KM_PT / 8; ++i) {
            const int pl = row + 8 * i;
            const long long p = p0 + pl;
            sx[pl * KM_LD + kk] = (p < P && k < G) ? x[p * G + k] : 0.0;
        }
        if (!transA) {
#pragma unroll
            for (int i = 0; i < KM_RT / 8; ++i) {
                const int rl = row + 8 * i, r = r0 + rl;
                sa[rl * KM_LD + kk] = (r < R && k < G) ? A[(long long)r * G + k] : 0.0;
            }
        } else {                                            // A is G x R in memory: r-contiguous reads
            for (int idx = t; idx < KM_RT * KM_KS; idx += 256) {
                const int rl = idx & (KM_RT - 1), kl = idx >> 7, r = r0 + rl, kq = k0 + kl;
                sa[rl * KM_LD + kl] = (r < R && kq < G) ? A[(long long)kq * R + r] : 0.0;
            }
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < KM_KS / 4; ++s) {
            const int ks = (lane >> 4) + 4 * s;
            const double b = sx[(w * 16 + (lane & 15)) * KM_LD + ks];
#pragma unroll
            for (int i = 0; i < KM_RT / 16; ++i) acc[i] = mfma_f64(sa[(i * 16 + (lane & 15)) * KM_LD + ks], b, acc[i]);
        }
    }
    const long long p = p0 + w * 16 + (lane & 15);
    if (p < P) {
#pragma unroll
        for (int i = 0; i < KM_RT / 16; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = r0 + i * 16 + (lane >> 4) + 4 * q;
                if (r < R) out[(long long)r * P + p] = acc[i][q];
            }
    }
}

static int launch_kron_mode(hipStream_t st, const double* A, int transA, const double* x, double* out, int64_t P, int64_t G,
                            int64_t R) {
    const int64_t nbx = (P + KM_PT - 1) / KM_PT, nby = (R + KM_RT - 1) / KM_RT;
    if (nbx > 2147483647LL || nby > 65535) {
        mi355gp_set_error("kron mode product: P = %lld, R = %lld is beyond one launch", (long long)P, (long long)R);
        return -1;
    }
    hipLaunchKernelGGL(k_kron_mode, dim3((unsigned)nbx, (unsigned)nby), dim3(256), 0, st, A, transA, x, out, (long long)P, (int)G,
                       (int)R);
    HIP_CHECK(hipGetLastError());
    return 0;
}

// The grid of a context as the kernels take it by value.
struct KronDims {
    int D;
    int G[MI355GP_KRON_MAX_D];
    int off[MI355GP_KRON_MAX_D];     // offset of dimension d in a concatenation of per-dimension vectors
};

// prod_d v[off_d + i_d] of the flat index i (last dimension fastest), multiplied from d = 0 up as numpy.kron nests it
__device__ __forceinline__ double kron_entry(const KronDims& kd, const double* __restrict__ v, long long i) {
    int id[MI355GP_KRON_MAX_D];
    for (int d = kd.D - 1; d >= 0; --d) {
        id[d] = (int)(i % kd.G[d]);
        i /= kd.G[d];
    }
    double r = v[kd.off[0] + id[0]];
    for (int d = 1; d < kd.D; ++d) r *= v[kd.off[d] + id[d]];
    return r;
}

// x_i /= V_i + noise after the Q^T pass
__global__ __launch_bounds__(256) void k_kron_scale(KronDims kd, const double* __restrict__ lam, double noise, double* __restrict__ x,
                                                    long long N) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < N) x[i] = x[i] / (kron_entry(kd, lam, i) + noise);
}

// w_i = 1 / (V_i + noise): the operand of the variance reduction of a prediction
__global__ __launch_bounds__(256) void k_kron_winv(KronDims kd, const double* __restrict__ lam, double noise, double* __restrict__ w,
                                                   long long N) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < N) w[i] = 1.0 / (kron_entry(kd, lam, i) + noise);
}

// Every sum of this file is carried as a pair (s, c): s the running float64 sum, c the sum of the rounding errors of its additions
// (Knuth's two-sum; products enter with the error of their rounding, fma(a, b, -p)), added once at the end.  The products are
// __dmul_rn so that no contraction folds them into the additions the error terms are taken from.
__device__ __forceinline__ void acc_add(double& s, double& c, double x) {
    const double t = s + x, bp = t - s;
    c += (s - (t - bp)) + (x - bp);
    s = t;
}

// the tree of a block's 256 pairs, in a fixed order; the pair of the whole block is in (s, c) of every thread afterwards
__device__ __forceinline__ void block_sum256(double& s, double& c, double* red) {
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = s;
    red[256 + t] = c;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) {
            double a = red[t], e = red[256 + t] + red[256 + t + h];
            acc_add(a, e, red[t + h]);
            red[t] = a;
            red[256 + t] = e;
        }
        __syncthreads();
    }
    s = red[0];
    c = red[256];
}

// Stage one of the two sums of a mode: block b takes the elements b * 256 + t + j * nb * 256 in ascending j (nb is a function of N
// alone), then the block's tree.  mode 0: (a_i b_i, log(V_i + noise));  mode 1: (a_i b_i, gamma_i / (V_i + noise)).  A partial is
// the pair of each sum: part[4 b ..] = s0, c0, s1, c1.
__global__ __launch_bounds__(256) void k_kron_reduce(int mode, KronDims kd, const double* __restrict__ a, const double* __restrict__ b,
                                                     const double* __restrict__ lam, const double* __restrict__ gam, double noise,
                                                     long long N, double* __restrict__ part) {
    __shared__ double red[512];
    double s0 = 0.0, c0 = 0.0, s1 = 0.0, c1 = 0.0;
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < N; i += stride) {
        const double p = __dmul_rn(a[i], b[i]);
        c0 += fma(a[i], b[i], -p);
        acc_add(s0, c0, p);
        const double v = kron_entry(kd, lam, i) + noise;
        acc_add(s1, c1, mode == 0 ? log(v) : kron_entry(kd, gam, i) / v);
    }
    block_sum256(s0, c0, red);
    block_sum256(s1, c1, red);
    if (threadIdx.x == 0) {
        double* o = part + (long long)blockIdx.x * 2 * KR_NRED;
        o[0] = s0;
        o[1] = c0;
        o[2] = s1;
        o[3] = c1;
    }
}

// Stage two: one block, thread t takes the partials t, t + 256, ... in ascending order, then the tree.
__global__ __launch_bounds__(256) void k_kron_reduce2(const double* __restrict__ part, int nb, double* __restrict__ out) {
    __shared__ double red[512];
    for (int q = 0; q < KR_NRED; ++q) {
        double s = 0.0, c = 0.0;
        for (int j = threadIdx.x; j < nb; j += 256) {
            c += part[(j * KR_NRED + q) * 2 + 1];
            acc_add(s, c, part[(j * KR_NRED + q) * 2]);
        }
        block_sum256(s, c, red);
        if (threadIdx.x == 0) out[q] = s + c;
    }
}

// Second step of a prediction: block m of a block of new points contracts its P-sized slice z[m][p] (p over the dimensions
// 0 .. D-2, last fastest) with prod_{d < D-1} f_d[m][p_d];  f_d is the M x G_d block at foff[d] of the concatenation, m0 the first
// point of the block.  D = 1: the slice is one number.
__global__ __launch_bounds__(256) void k_kron_point(KronDims kd, const double* __restrict__ z, long long P,
                                                    const double* __restrict__ f, const long long* __restrict__ foff, long long m0,
                                                    double* __restrict__ out) {
    __shared__ double red[512];
    const long long m = m0 + blockIdx.x;
    const double* zm = z + (long long)blockIdx.x * P;
    double s = 0.0, c = 0.0;
    for (long long p = threadIdx.x; p < P; p += 256) {
        double v = zm[p];
        long long i = p;
        for (int d = kd.D - 2; d >= 0; --d) {
            v = __dmul_rn(v, f[foff[d] + m * kd.G[d] + (i % kd.G[d])]);
            i /= kd.G[d];
        }
        acc_add(s, c, v);
    }
    block_sum256(s, c, red);
    if (threadIdx.x == 0) out[m] = s + c;
}

struct mi355gp_kron {
    int device = 0;
    hipStream_t st = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    KronDims kd{};
    int64_t N = 0, sumG = 0, sumG2 = 0;
    int64_t goff2[MI355GP_KRON_MAX_D] = {};      // offset of dimension d in a concatenation of per-dimension matrices
    DevBuf y, alpha, w0, w1;                     // the N-vectors
    DevBuf Q, lam, fac, gam, part, scal;         // sum G_d^2, sum G_d, sum G_d^2, sum G_d, the partial sums, their totals
    double noise = 0.0, ms = 0.0;
    bool have_data = false, solved = false;
};

#define KRON_VGRID(n) dim3((unsigned)(((n) + 255) / 256)), dim3(256)

static int red_blocks(int64_t N) {
    const int64_t nb = (N + 1023) / 1024;
    return (int)(nb < 1 ? 1 : (nb > KR_MAXB ? KR_MAXB : nb));
}

// (x)_d A_d applied to src (y, alpha or a work vector): D mode products, last dimension first, ping-pong between the two work
// vectors starting with the one src is not; the last product writes to `last` where that is given.  *res is where the result is.
// A_d = mats + goff2[d], read transposed with transA.
static int kron_apply(mi355gp_kron* c, const double* mats, int transA, const double* src, double* last, double** res) {
    const double* cur = src;
    double* bufs[2] = {c->w0, c->w1};
    int nxt = (src == bufs[0]) ? 1 : 0;
    for (int d = c->kd.D - 1; d >= 0; --d) {
        const int64_t G = c->kd.G[d];
        double* dst = (d == 0 && last) ? last : bufs[nxt];
        if (launch_kron_mode(c->st, mats + c->goff2[d], transA, cur, dst, c->N / G, G, G) != 0) return -1;
        cur = dst;
        nxt ^= 1;
    }
    *res = const_cast<double*>(cur);
    return 0;
}

// the two sums of a mode over (a, b) to host[0..1]
static int kron_sums(mi355gp_kron* c, int mode, const double* a, const double* b, const double* gam, double* host) {
    const int nb = red_blocks(c->N);
    hipLaunchKernelGGL(k_kron_reduce, dim3(nb), dim3(256), 0, c->st, mode, c->kd, a, b, (const double*)c->lam, gam, c->noise,
                       (long long)c->N, (double*)c->part);
    hipLaunchKernelGGL(k_kron_reduce2, dim3(1), dim3(256), 0, c->st, (const double*)c->part, nb, (double*)c->scal);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(host, c->scal, sizeof(double) * KR_NRED, hipMemcpyDeviceToHost, c->st));
    HIP_CHECK(hipStreamSynchronize(c->st));
    return 0;
}

extern "C" {

int mi355gp_kron_create(int device, mi355gp_kron** out) {
    ARG_CHECK(out != nullptr, "mi355gp_kron_create: out is NULL");
    int n = 0;
    mi355gp_device_count(&n);
    if (device < 0 || device >= n) {
        mi355gp_set_error("mi355gp_kron_create: device %d not available (%d HIP devices visible)", device, n);
        return -2;
    }
    HIP_CHECK(hipSetDevice(device));
    mi355gp_kron* c = new mi355gp_kron();
    c->device = device;
    *out = c;                                    // destroy releases whatever was made if a later step fails
    HIP_CHECK(hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking));
    HIP_CHECK(hipEventCreate(&c->ev0));
    HIP_CHECK(hipEventCreate(&c->ev1));
    HIP_CHECK(c->part.alloc(KR_MAXB * KR_NRED * 2));
    HIP_CHECK(c->scal.alloc(KR_NRED));
    return 0;
}

int mi355gp_kron_destroy(mi355gp_kron* c) {
    if (!c) return 0;
    (void)hipSetDevice(c->device);
    if (c->st) {
        (void)hipStreamSynchronize(c->st);
        (void)hipStreamDestroy(c->st);
    }
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    delete c;
    return 0;
}

int mi355gp_kron_set_data(mi355gp_kron* c, int D, const int64_t* G, const double* y) {
    ARG_CHECK(c && G && y, "mi355gp_kron_set_data: NULL argument");
    if (D < 1 || D > MI355GP_KRON_MAX_D) {
        mi355gp_set_error("mi355gp_kron_set_data: D = %d, the grid has 1 to %d dimensions", D, MI355GP_KRON_MAX_D);
        return -1;
    }
    int64_t N = 1, sumG = 0, sumG2 = 0;
    KronDims kd{};
    kd.D = D;
    for (int d = 0; d < D; ++d) {
        if (G[d] < 1 || G[d] > MI355GP_KRON_MAX_G) {
            mi355gp_set_error("mi355gp_kron_set_data: G[%d] = %lld, a grid dimension has 1 to %d points", d, (long long)G[d],
                              MI355GP_KRON_MAX_G);
            return -1;
        }
        if (N > (int64_t)1 << 40) {
            mi355gp_set_error("mi355gp_kron_set_data: the grid has more than 2^40 points");
            return -1;
        }
        kd.G[d] = (int)G[d];
        kd.off[d] = (int)sumG;
        c->goff2[d] = sumG2;
        N *= G[d];
        sumG += G[d];
        sumG2 += G[d] * G[d];
    }
    HIP_CHECK(hipSetDevice(c->device));
    HIP_CHECK(hipStreamSynchronize(c->st));
    c->have_data = c->solved = false;
    DevBuf* nv[4] = {&c->y, &c->alpha, &c->w0, &c->w1};
    for (DevBuf* b : nv) {
        *b = DevBuf();
        HIP_CHECK(b->alloc((size_t)N));
    }
    DevBuf* g2[2] = {&c->Q, &c->fac};
    for (DevBuf* b : g2) {
        *b = DevBuf();
        HIP_CHECK(b->alloc((size_t)sumG2));
    }
    DevBuf* g1[2] = {&c->lam, &c->gam};
    for (DevBuf* b : g1) {
        *b = DevBuf();
        HIP_CHECK(b->alloc((size_t)sumG));
    }
    c->kd = kd;
    c->N = N;
    c->sumG = sumG;
    c->sumG2 = sumG2;
    HIP_CHECK(hipMemcpyAsync(c->y, y, sizeof(double) * N, hipMemcpyHostToDevice, c->st));
    HIP_CHECK(hipStreamSynchronize(c->st));
    c->have_data = true;
    return 0;
}

int mi355gp_kron_solve(mi355gp_kron* c, const double* Q, const double* lam, double noise, double* scalars) {
    ARG_CHECK(c && Q && lam && scalars, "mi355gp_kron_solve: NULL argument");
    ARG_CHECK(c->have_data, "mi355gp_kron_solve: no data (mi355gp_kron_set_data first)");
    ARG_CHECK(std::isfinite(noise), "mi355gp_kron_solve: the noise term is not finite");
    HIP_CHECK(hipSetDevice(c->device));
    c->solved = false;
    c->noise = noise;
    HIP_CHECK(hipMemcpyAsync(c->Q, Q, sizeof(double) * c->sumG2, hipMemcpyHostToDevice, c->st));
    HIP_CHECK(hipMemcpyAsync(c->lam, lam, sizeof(double) * c->sumG, hipMemcpyHostToDevice, c->st));
    HIP_CHECK(hipEventRecord(c->ev0, c->st));
    double* t = nullptr;
    if (kron_apply(c, c->Q, 1, c->y, nullptr, &t) != 0) return -1;                // (x)Q_d^T y
    hipLaunchKernelGGL(k_kron_scale, KRON_VGRID(c->N), 0, c->st, c->kd, (const double*)c->lam, noise, t, (long long)c->N);
    HIP_CHECK(hipGetLastError());
    double* a = nullptr;
    if (kron_apply(c, c->Q, 0, t, c->alpha, &a) != 0) return -1;                  // (x)Q_d of it: the last product writes alpha
    HIP_CHECK(hipEventRecord(c->ev1, c->st));
    if (kron_sums(c, 0, c->y, c->alpha, nullptr, scalars) != 0) return -1;
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->ms = ms;
    c->solved = true;
    return 0;
}

int mi355gp_kron_quadforms(mi355gp_kron* c, int nmat, const double* factors, const double* gammas, double* out) {
    ARG_CHECK(c && factors && gammas && out, "mi355gp_kron_quadforms: NULL argument");
    ARG_CHECK(c->solved, "mi355gp_kron_quadforms: no alpha (mi355gp_kron_solve first)");
    ARG_CHECK(nmat >= 0, "mi355gp_kron_quadforms: nmat is negative");
    HIP_CHECK(hipSetDevice(c->device));
    for (int t = 0; t < nmat; ++t) {
        HIP_CHECK(hipMemcpyAsync(c->fac, factors + (int64_t)t * c->sumG2, sizeof(double) * c->sumG2, hipMemcpyHostToDevice, c->st));
        HIP_CHECK(hipMemcpyAsync(c->gam, gammas + (int64_t)t * c->sumG, sizeof(double) * c->sumG, hipMemcpyHostToDevice, c->st));
        HIP_CHECK(hipEventRecord(c->ev0, c->st));
        // a set of identities (the noise parameter): kappa is alpha, bit for bit what the D products would give
        bool ident = true;
        const double* F = factors + (int64_t)t * c->sumG2;
        for (int d = 0; d < c->kd.D && ident; ++d) {
            const int64_t G = c->kd.G[d];
            for (int64_t i = 0; i < G * G && ident; ++i) ident = F[c->goff2[d] + i] == ((i / G == i % G) ? 1.0 : 0.0);
        }
        double* kappa = c->alpha;
        if (!ident && kron_apply(c, c->fac, 0, c->alpha, nullptr, &kappa) != 0) return -1;
        HIP_CHECK(hipEventRecord(c->ev1, c->st));
        if (kron_sums(c, 1, c->alpha, kappa, c->gam, out + 2 * t) != 0) return -1;
        float ms = 0.f;
        HIP_CHECK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        c->ms += ms;
    }
    return 0;
}

int mi355gp_kron_predict(mi355gp_kron* c, int64_t M, const double* kx, const double* bx, double noise_pred, double* mu,
                         double* var_reduction) {
    ARG_CHECK(c && kx && mu, "mi355gp_kron_predict: NULL argument");
    ARG_CHECK(c->solved, "mi355gp_kron_predict: no alpha (mi355gp_kron_solve first)");
    ARG_CHECK(M >= 1, "mi355gp_kron_predict: no new points");
    ARG_CHECK(var_reduction == nullptr || bx != nullptr, "mi355gp_kron_predict: var_reduction needs bx");
    ARG_CHECK(std::isfinite(noise_pred), "mi355gp_kron_predict: the noise term is not finite");
    HIP_CHECK(hipSetDevice(c->device));
    const int D = c->kd.D;
    const int64_t GL = c->kd.G[D - 1], P = c->N / GL, tot = M * c->sumG;
    std::vector<long long> foff(D);
    for (int d = 0; d < D; ++d) foff[d] = (long long)M * c->kd.off[d];
    DevBuf dk, db, dmu, dvar;
    DevArr<long long> dfoff;
    HIP_CHECK(dk.alloc((size_t)tot));
    HIP_CHECK(dmu.alloc((size_t)M));
    HIP_CHECK(dfoff.alloc(D));
    HIP_CHECK(hipMemcpyAsync(dk, kx, sizeof(double) * tot, hipMemcpyHostToDevice, c->st));
    HIP_CHECK(hipMemcpyAsync(dfoff, foff.data(), sizeof(long long) * D, hipMemcpyHostToDevice, c->st));
    std::vector<double> b2;
    if (var_reduction) {
        b2.resize((size_t)tot);
        for (int64_t i = 0; i < tot; ++i) b2[i] = bx[i] * bx[i];
        HIP_CHECK(db.alloc((size_t)tot));
        HIP_CHECK(dvar.alloc((size_t)M));
        HIP_CHECK(hipMemcpyAsync(db, b2.data(), sizeof(double) * tot, hipMemcpyHostToDevice, c->st));
        // w0 = 1 / (V + noise_pred); the contracted slices go to w1
        hipLaunchKernelGGL(k_kron_winv, KRON_VGRID(c->N), 0, c->st, c->kd, (const double*)c->lam, noise_pred, (double*)c->w0,
                           (long long)c->N);
        HIP_CHECK(hipGetLastError());
    }
    // A block of new points contracts the last dimension as ONE mode product (R = the block), so alpha and 1 / (V + noise) are read
    // once per block; its R x P result must fit a work vector of N = P * G_last doubles: the block is min(64, G_last) points.
    const int64_t MB = GL < 64 ? GL : 64;
    for (int64_t m0 = 0; m0 < M; m0 += MB) {
        const int64_t mb = (M - m0 < MB) ? M - m0 : MB;
        if (launch_kron_mode(c->st, (const double*)dk + foff[D - 1] + m0 * GL, 0, (const double*)c->alpha, (double*)c->w1, P, GL, mb) != 0) return -1;
        hipLaunchKernelGGL(k_kron_point, dim3((unsigned)mb), dim3(256), 0, c->st, c->kd, (const double*)c->w1, (long long)P,
                           (const double*)dk, (const long long*)dfoff, (long long)m0, (double*)dmu);
        if (var_reduction) {
            if (launch_kron_mode(c->st, (const double*)db + foff[D - 1] + m0 * GL, 0, (const double*)c->w0, (double*)c->w1, P, GL, mb) != 0) return -1;
            hipLaunchKernelGGL(k_kron_point, dim3((unsigned)mb), dim3(256), 0, c->st, c->kd, (const double*)c->w1, (long long)P,
                               (const double*)db, (const long long*)dfoff, (long long)m0, (double*)dvar);
        }
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipMemcpyAsync(mu, dmu, sizeof(double) * M, hipMemcpyDeviceToHost, c->st));
    if (var_reduction) HIP_CHECK(hipMemcpyAsync(var_reduction, dvar, sizeof(double) * M, hipMemcpyDeviceToHost, c->st));
    HIP_CHECK(hipStreamSynchronize(c->st));
    return 0;
}

int mi355gp_kron_fetch(mi355gp_kron* c, int which, double* out) {
    ARG_CHECK(c && out, "mi355gp_kron_fetch: NULL argument");
    ARG_CHECK(c->solved, "mi355gp_kron_fetch: no alpha (mi355gp_kron_solve first)");
    ARG_CHECK(which == MI355GP_KRON_FETCH_ALPHA, "mi355gp_kron_fetch: unknown buffer id");
    HIP_CHECK(hipSetDevice(c->device));
    HIP_CHECK(hipMemcpyAsync(out, c->alpha, sizeof(double) * c->N, hipMemcpyDeviceToHost, c->st));
    HIP_CHECK(hipStreamSynchronize(c->st));
    return 0;
}

int mi355gp_kron_mode_probe(mi355gp_kron* c, int64_t P, int64_t G, int64_t R, int transA, const double* A, const double* x,
                            double* out, int reps, double* ms_out) {
    ARG_CHECK(c && A && x && out, "mi355gp_kron_mode_probe: NULL argument");
    ARG_CHECK(P >= 1 && G >= 1 && R >= 1 && G <= MI355GP_KRON_MAX_G && R <= ((int64_t)1 << 22) && P <= ((int64_t)1 << 40),
              "mi355gp_kron_mode_probe: P, G or R out of range");
    HIP_CHECK(hipSetDevice(c->device));
    DevBuf dA, dx, dout;
    HIP_CHECK(dA.alloc((size_t)(R * G)));
    HIP_CHECK(dx.alloc((size_t)(P * G)));
    HIP_CHECK(dout.alloc((size_t)(R * P)));
    HIP_CHECK(hipMemcpyAsync(dA, A, sizeof(double) * R * G, hipMemcpyHostToDevice, c->st));
    HIP_CHECK(hipMemcpyAsync(dx, x, sizeof(double) * P * G, hipMemcpyHostToDevice, c->st));
    if (reps < 1) reps = 1;
    HIP_CHECK(hipEventRecord(c->ev0, c->st));
    for (int i = 0; i < reps; ++i)
        if (launch_kron_mode(c->st, dA, transA ? 1 : 0, dx, dout, P, G, R) != 0) return -1;
    HIP_CHECK(hipEventRecord(c->ev1, c->st));
    HIP_CHECK(hipMemcpyAsync(out, dout, sizeof(double) * R * P, hipMemcpyDeviceToHost, c->st));
    HIP_CHECK(hipStreamSynchronize(c->st));
    if (ms_out) {
        float ms = 0.f;
        HIP_CHECK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
        *ms_out = (double)ms / reps;
    }
    return 0;
}

int mi355gp_kron_get_ms(mi355gp_kron* c, double* ms_out) {
    ARG_CHECK(c && ms_out, "mi355gp_kron_get_ms: NULL argument");
    *ms_out = c->ms;
    return 0;
}

}   // extern "C"
