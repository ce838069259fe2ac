// psi_missing.hip -- psi2 of the RBF kernel and its chain rule for SEVERAL row masks at once: the psi2 side of a Bayesian GPLVM
// with missing data (GPy/models/sparse_gp_minibatch.py:228-286).  Output columns of Y that share a set of observed rows form a
// group g with row weights w_g (0 / 1, N of them); the fit needs
//   psi2_g = sum_n w_ng psi2n                                  for every group, and
//   the row pass of the chain rule with the per-row weight  sum_g w_ng dL_g[m][o]   (dL_g = that group's symmetrised dL_dpsi2).
// The reference materialises psi2n (N x M x M) and slices it per group.  Here a launch carries up to PSI_GB groups: the exponential
// of a (n, m, o) triple is evaluated ONCE and weighted PSI_GB ways, where PSI_GB calls of k_psi2 / k_psi2_grad with weights w_g
// would evaluate it PSI_GB times.  The kernels are those two kernels' tilings (psi.hip) instantiated beside them; the row records,
// Ppart / Zpart, launch_psi2_combine, launch_psi_rowfinish and launch_psi2_zz are used as they are.  G > PSI_GB groups take
// ceil(G / PSI_GB) launches.  Every sum is combined in a fixed order -- groups ascending, chunks ascending, splits ascending --
// by plain launches on one stream: no workgroup waits on another and there are no floating-point atomics.
#include <cmath>
#include <vector>

#include "../../include/mi355gp_sparse_missing.h"
#include "../../include/mi355gp_debug_sparse_missing.h"
#include "internal.h"
#include "parts.h"
#include "psi_missing.h"

// psi2 partial sums of gb <= PSI_GB groups: part[g][split][mi][oj] = var^2 sum over the split's rows of w_ng psi2n[mi][oj] / var^2.
// k_psi2's tiling: thread = one (m, o) of a lower 16-tile, rows through LDS with their PSI_GB weights next to lgs.
template <int QP>
__global__ __launch_bounds__(256) void k_psi2_multi(const double2* __restrict__ rd2, const double* __restrict__ lg2,
                                                    const double* __restrict__ wt, long ldw, int gb, const double* __restrict__ Zp,
                                                    const double* __restrict__ ap, long rows, long rps, long m, double var2,
                                                    long ld, long gstride, double* __restrict__ part) {
    constexpr int RB = QP > 32 ? 32 : 64;                    // rows staged at a time
    __shared__ double2 rs[RB * QP];
    __shared__ double lgs[RB], ws[RB * PSI_GB];
    int ti, tj;
    psi_tile(blockIdx.x, &ti, &tj);
    const int t = threadIdx.x;
    const long mi = (long)ti * PSI_T2 + (t >> 4), oj = (long)tj * PSI_T2 + (t & 15);
    double zb[QP];
    double zd = 0.0;
#pragma unroll
    for (int q = 0; q < QP; ++q) {
        const double zm = Zp[mi * QP + q], zo = Zp[oj * QP + q], dz = zm - zo;
        zb[q] = 0.5 * (zm + zo);
        zd = fma(ap[q] * dz, dz, zd);
    }
    zd *= 0.25;
    const long r0 = (long)blockIdx.y * rps, r1 = (r0 + rps < rows) ? (r0 + rps) : rows;
    double acc[PSI_GB];
#pragma unroll
    for (int g = 0; g < PSI_GB; ++g) acc[g] = 0.0;
    for (long rb = r0; rb < r1; rb += RB) {
        for (int idx = t; idx < RB * QP; idx += 256) {
            const long n = rb + idx / QP;
            rs[idx] = (n < r1) ? rd2[n * QP + (idx % QP)] : make_double2(0.0, 0.0);
        }
        if (t < RB) {
            const long n = rb + t;
            lgs[t] = (n < r1) ? lg2[n] : 0.0;
        }
        for (int idx = t; idx < RB * PSI_GB; idx += 256) {   // (group-major in memory: a wave reads consecutive rows of one group)
            const int g = idx / RB, r = idx - g * RB;
            const long n = rb + r;
            ws[r * PSI_GB + g] = (g < gb && n < r1) ? wt[(long)g * ldw + n] : 0.0;
        }
        __syncthreads();
        for (int r = 0; r < RB; ++r) {
            double e = zd;
#pragma unroll
            for (int q = 0; q < QP; ++q) {
                const double2 v = rs[r * QP + q];
                const double d = v.x - zb[q];
                e = fma(v.y * d, d, e);
            }
            const double p = exp(lgs[r] - e);
#pragma unroll
            for (int g = 0; g < PSI_GB; ++g) acc[g] = fma(ws[r * PSI_GB + g], p, acc[g]);
        }
        __syncthreads();
    }
    if (mi < m && oj < m) {
        double* o = part + (long)blockIdx.y * ld * ld + mi * ld + oj;
#pragma unroll
        for (int g = 0; g < PSI_GB; ++g)
            if (g < gb) o[(long)g * gstride] = var2 * acc[g];
    }
}

// psi2 chain rule, row pass, for gb <= PSI_GB groups: L = (sum_g w_ng dL_g[m][o]) var^2 exp(lg2 - zd[m][o] - sum c2 d^2),
// d = mu - (z_m + z_o)/2; every dL_g symmetric, read as dL_g[o][m].  k_psi2_grad's tiling with the dL tiles of all the batch's
// groups staged (dLs[g][o][16]) and OC inducing points o at a time (psi_multi_oc).
// LDS (dynamic): zm 16 x (Qp + 1) | rows 16 x Qp double2 | zo OC x Qp | dLs PSI_GB x OC x 16 | zred 4 x 16 x QG
template <int QG>
__global__ __launch_bounds__(256) void k_psi2_grad_multi(const double2* __restrict__ rd, const double* __restrict__ lg2,
                                                         const double* __restrict__ wt, long ldw, int gb,
                                                         const double* __restrict__ Zp, const double* __restrict__ ap,
                                                         const double* __restrict__ dL, long dstride, long ldd, long rows, long m,
                                                         long mpad, int Qp, int OC, double var2, double* __restrict__ Ppart,
                                                         double* __restrict__ Zpart) {
    extern __shared__ __align__(16) double sm[];
    double* zm = sm;                                           // 16 x (Qp + 1)
    double2* rs = (double2*)(sm + 16 * (Qp + 2));              // 16 x Qp
    double* zo = (double*)(rs + 16 * Qp);                      // OC x Qp
    double* dLs = zo + OC * Qp;                                // PSI_GB x OC x 16: dL_g[o][m] var^2 exp(-zd[m][o])
    double* zred = dLs + PSI_GB * OC * 16;                     // 4 x 16 x QG
    const int t = threadIdx.x, ml = t & 15, nl = t >> 4, gz = blockIdx.z, qoff = gz * PSI_KDC;
    const long mcol = (long)blockIdx.x * 16 + ml, nb0 = (long)blockIdx.y * PSI_GROWS;
    const int RL = 1 + 2 * Qp;
    for (int idx = t; idx < 16 * Qp; idx += 256) {
        const int r = idx / Qp, q = idx - r * Qp;
        zm[r * (Qp + 1) + q] = Zp[((long)blockIdx.x * 16 + r) * Qp + q];
    }
    double zacc[QG];
#pragma unroll
    for (int q = 0; q < QG; ++q) zacc[q] = 0.0;
    for (int it = 0; it < PSI_GROWS / 16; ++it) {
        const long nbase = nb0 + it * 16;
        if (nbase >= rows) break;
        __syncthreads();
        for (int idx = t; idx < 16 * Qp; idx += 256) {
            const long n = nbase + idx / Qp;
            rs[idx] = (n < rows) ? rd[n * Qp + (idx % Qp)] : make_double2(0.0, 0.0);
        }
        const long n = nbase + nl;
        const bool nok = n < rows;
        const double lg = nok ? lg2[n] : 0.0;
        double wn[PSI_GB];
#pragma unroll
        for (int g = 0; g < PSI_GB; ++g) wn[g] = (nok && g < gb) ? wt[(long)g * ldw + n] : 0.0;
        double a0 = 0.0, g1[QG], g2[QG];
#pragma unroll
        for (int q = 0; q < QG; ++q) g1[q] = g2[q] = 0.0;
        for (long oc = 0; oc < m; oc += OC) {
            const int on = (m - oc < OC) ? (int)(m - oc) : OC;
            __syncthreads();                                   // (also orders the stores of zm / rs before their first use)
            for (int idx = t; idx < on * Qp; idx += 256) zo[idx] = Zp[oc * Qp + idx];
            __syncthreads();
            for (int idx = t; idx < on * 16; idx += 256) {
                const int o = idx >> 4, c = idx & 15;
                const long mc = (long)blockIdx.x * 16 + c;
                double zd = 0.0;
                for (int q = 0; q < Qp; ++q) {
                    const double dz = zm[c * (Qp + 1) + q] - zo[o * Qp + q];
                    zd = fma(ap[q] * dz, dz, zd);
                }
                const double ex = exp(-0.25 * zd);
#pragma unroll
                for (int g = 0; g < PSI_GB; ++g)
                    dLs[(g * OC + o) * 16 + c] = (mc < m && g < gb) ? dL[(long)g * dstride + (oc + o) * ldd + mc] * var2 * ex : 0.0;
            }
            __syncthreads();
            for (int o = 0; o < on; ++o) {
                double e = 0.0;
                for (int q = 0; q < Qp; ++q) {
                    const double2 v = rs[nl * Qp + q];
                    const double d = v.x - 0.5 * (zm[ml * (Qp + 1) + q] + zo[o * Qp + q]);
                    e = fma(v.y * d, d, e);
                }
                double f = 0.0;                                // the row's factor, formed before the one exponential
#pragma unroll
                for (int g = 0; g < PSI_GB; ++g) f = fma(wn[g], dLs[(g * OC + o) * 16 + ml], f);
                const double L = f * exp(lg - e);
                a0 += L;
#pragma unroll
                for (int q = 0; q < QG; ++q) {
                    const double d = rs[nl * Qp + qoff + q].x - 0.5 * (zm[ml * (Qp + 1) + qoff + q] + zo[o * Qp + qoff + q]);
                    const double Ld = L * d;
                    g1[q] += Ld;
                    g2[q] = fma(Ld, d, g2[q]);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < QG; ++q) zacc[q] = fma(rs[nl * Qp + qoff + q].y, g1[q], zacc[q]);
        psi_grad_emit<QG>(t, gz, Qp, n, nok, a0, g1, g2, Ppart + ((long)blockIdx.x * rows + (nok ? n : 0)) * RL);
    }
    __syncthreads();
    psi_grad_emit_z<QG>(t, gz, Qp, mcol, mpad, zacc, zred, Zpart + (long)blockIdx.y * mpad * Qp);
}

// out_g = (A_g + A_g^T) / 2 over m x m, g < G (rbf_psi_comp.py:109)
__global__ void k_psi_symmetrise_groups(const double* __restrict__ A, long m, double* __restrict__ out) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y, o = (long)blockIdx.z * m * m;
    if (j < m) out[o + i * m + j] = 0.5 * (A[o + i * m + j] + A[o + j * m + i]);
}

// ---- launchers ----------------------------------------------------------------------------------------------------
template <int QP>
static void launch_psi2_multi_t(hipStream_t st, const double* rd2, const double* lg2, const double* wt, long ldw, int gb,
                                const double* Zp, const double* ap, long rows, long m, double var2, long ld, int nsplit,
                                double* part) {
    const long nt = (m + PSI_T2 - 1) / PSI_T2, ntl = nt * (nt + 1) / 2;
    const long rps = round_up((rows + nsplit - 1) / nsplit, 64);
    hipLaunchKernelGGL((k_psi2_multi<QP>), dim3((unsigned)ntl, (unsigned)nsplit), dim3(256), 0, st, (const double2*)rd2, lg2, wt, ldw,
                       gb, Zp, ap, rows, rps, m, var2, ld, (long)nsplit * ld * ld, part);
}
int launch_psi2_multi(hipStream_t st, const double* rd2, const double* lg2, const double* wt, long ldw, int gb, const double* Zp,
                      const double* ap, long rows, long m, int Qp, double var2, long ld, double* part) {
    const int ns = psi2_nsplit(rows, m);
    switch (Qp) {
        case 1: launch_psi2_multi_t<1>(st, rd2, lg2, wt, ldw, gb, Zp, ap, rows, m, var2, ld, ns, part); break;
        case 2: launch_psi2_multi_t<2>(st, rd2, lg2, wt, ldw, gb, Zp, ap, rows, m, var2, ld, ns, part); break;
        case 4: launch_psi2_multi_t<4>(st, rd2, lg2, wt, ldw, gb, Zp, ap, rows, m, var2, ld, ns, part); break;
        case 8: launch_psi2_multi_t<8>(st, rd2, lg2, wt, ldw, gb, Zp, ap, rows, m, var2, ld, ns, part); break;
        case 16: launch_psi2_multi_t<16>(st, rd2, lg2, wt, ldw, gb, Zp, ap, rows, m, var2, ld, ns, part); break;
        case 32: launch_psi2_multi_t<32>(st, rd2, lg2, wt, ldw, gb, Zp, ap, rows, m, var2, ld, ns, part); break;
        default: launch_psi2_multi_t<64>(st, rd2, lg2, wt, ldw, gb, Zp, ap, rows, m, var2, ld, ns, part); break;
    }
    return ns;
}

static size_t psi_grad_multi_lds(int Qp, int QG, int OC) {
    return sizeof(double) * ((size_t)16 * (Qp + 2) + 2 * 16 * Qp + 4 * 16 * QG + (size_t)OC * Qp + (size_t)PSI_GB * OC * 16);
}
void launch_psi2_grad_multi(hipStream_t st, const double* rd2, const double* lg2, const double* wt, long ldw, int gb,
                            const double* Zp, const double* ap, const double* dL, long dstride, long ldd, long rows, long m,
                            long mpad, int Qp, double var2, double* Ppart, double* Zpart) {
    const int QG = Qp < PSI_KDC ? Qp : PSI_KDC, OC = psi_multi_oc(Qp);
    const dim3 grid((unsigned)((m + 15) / 16), (unsigned)((rows + PSI_GROWS - 1) / PSI_GROWS), (unsigned)(Qp / QG));
    const size_t lds = psi_grad_multi_lds(Qp, QG, OC);         // at most 53.5 KB (Qp = 64)
#define PSI_CALL(N) hipLaunchKernelGGL((k_psi2_grad_multi<N>), grid, dim3(256), lds, st, (const double2*)rd2, lg2, wt, ldw, gb, Zp, ap, dL, dstride, ldd, rows, m, mpad, Qp, OC, var2, Ppart, Zpart)
    switch (QG) {
        case 1: PSI_CALL(1); break;
        case 2: PSI_CALL(2); break;
        case 4: PSI_CALL(4); break;
        case 8: PSI_CALL(8); break;
        case 16: PSI_CALL(16); break;
        default: PSI_CALL(32); break;
    }
#undef PSI_CALL
}

// ---- the stateless pair ---------------------------------------------------------------------------------------------
namespace {
// what both entry points validate and upload: the kernel's parameters, Z (padded), the Gaussian inputs and the weights,
// transposed to group-major (G x N) so that one group's rows are contiguous for either route
struct GroupInputs {
    PartSpec spec;
    int D = 0, Qp = 0, G = 0;
    long N = 0, M = 0, mpad = 0, chunk = 0, ld = 0;
    double var = 0.0;
    std::vector<double> a;
    DevBuf dA, dZp, dMu, dS, dWt, rd1, rd2, lg1, lg2;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    double ms = 0.0;                                         // stream time between tic() and toc(), summed
    ~GroupInputs() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    int load(const char* where, double variance, const double* lengthscale, int ard, const double* Z, int64_t M_, const double* mu,
             const double* S, int64_t N_, int D_, const double* W, int G_) {
        if (!(lengthscale && Z && mu && S && W && M_ > 0 && N_ > 0 && D_ > 0 && G_ > 0)) PART_FAIL("%s: bad arguments", where);
        if (M_ > PSI_MMAX) PART_FAIL("%s: %lld inducing points; the psi-statistics kernels take at most %d", where, (long long)M_, PSI_MMAX);
        if (D_ > PSI_QMAX) PART_FAIL("%s: %d input dimensions; the psi-statistics kernels take at most %d", where, D_, PSI_QMAX);
        if (G_ > 65535) PART_FAIL("%s: %d groups; at most 65535", where, G_);
        std::vector<double> th(1 + (size_t)(ard ? D_ : 1));
        th[0] = variance;
        for (size_t k = 1; k < th.size(); ++k) th[k] = lengthscale[k - 1];
        const mi355gp_part part{MI355GP_RBF, ard ? 1 : 0, 0, nullptr, th.data(), 0};
        if (int rc = parse_part(part, D_, 1u << MI355GP_RBF, where, &spec)) return rc;
        for (int64_t i = 0; i < N_ * D_; ++i)
            if (!(S[i] > 0.0) || !std::isfinite(S[i]) || !std::isfinite(mu[i]))
                PART_FAIL("%s: input variance S[%lld][%lld] = %g (mean %g): every entry must be positive and finite", where,
                          (long long)(i / D_), (long long)(i % D_), S[i], mu[i]);
        for (int64_t i = 0; i < N_ * G_; ++i)
            if (!std::isfinite(W[i]))
                PART_FAIL("%s: weight W[%lld][%lld] is not finite", where, (long long)(i / G_), (long long)(i % G_));
        D = D_, N = N_, M = M_, G = G_;
        Qp = psi_qp(D);
        mpad = round_up(M, PSI_KT);
        ld = round_up(M, PSI_T2);
        chunk = N < PSI_CHUNK ? N : PSI_CHUNK;
        var = variance;
        a.assign((size_t)Qp, 0.0);
        for (int q = 0; q < D; ++q) a[(size_t)q] = spec.inv_ls[(size_t)q] * spec.inv_ls[(size_t)q];
        std::vector<double> zp((size_t)mpad * Qp, 0.0), wt((size_t)G * N);
        for (long i = 0; i < M; ++i)
            for (int q = 0; q < D; ++q) zp[(size_t)i * Qp + q] = Z[i * D + q];
        for (long n = 0; n < N; ++n)
            for (int g = 0; g < G; ++g) wt[(size_t)g * N + n] = W[n * G + g];
        HIP_CHECK(dA.alloc(Qp));
        HIP_CHECK(dZp.alloc(zp.size()));
        HIP_CHECK(dMu.alloc(N * D));
        HIP_CHECK(dS.alloc(N * D));
        HIP_CHECK(dWt.alloc(wt.size()));
        HIP_CHECK(rd1.alloc(2 * chunk * Qp));
        HIP_CHECK(rd2.alloc(2 * chunk * Qp));
        HIP_CHECK(lg1.alloc(chunk));
        HIP_CHECK(lg2.alloc(chunk));
        HIP_CHECK(hipMemcpy(dA, a.data(), sizeof(double) * Qp, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dZp, zp.data(), sizeof(double) * zp.size(), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dMu, mu, sizeof(double) * N * D, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dS, S, sizeof(double) * N * D, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dWt, wt.data(), sizeof(double) * wt.size(), hipMemcpyHostToDevice));
        HIP_CHECK(hipEventCreate(&e0));
        HIP_CHECK(hipEventCreate(&e1));
        return 0;
    }
    void fill(hipStream_t st, long r0, long rc) {
        launch_psi_rows(st, dMu + r0 * D, dS + r0 * D, dA, rc, D, Qp, rd1, rd2, lg1, lg2);
    }
    int tic(hipStream_t st) {
        HIP_CHECK(hipEventRecord(e0, st));
        return 0;
    }
    int toc(hipStream_t st) {
        float f = 0.f;
        HIP_CHECK(hipEventRecord(e1, st));
        HIP_CHECK(hipEventSynchronize(e1));
        HIP_CHECK(hipEventElapsedTime(&f, e0, e1));
        ms += f;
        return 0;
    }
    // psi2_g (M x M each, g < G) of all rows into out (device, G x M x M), chunk by chunk in row order; part: the partial
    // buffer of one batch.  loop: k_psi2 once per group with weights w_g instead of the multi kernel.  The psi2 kernels alone are timed.
    int psi2_all(hipStream_t st, int loop, double* part, double* out) {
        int nch = 0;
        for (long r0 = 0; r0 < N; r0 += PSI_CHUNK, ++nch) {
            const long rc = (N - r0 < PSI_CHUNK) ? (N - r0) : PSI_CHUNK;
            fill(st, r0, rc);
            for (int g0 = 0; g0 < G; g0 += PSI_GB) {
                const int gb = (G - g0 < PSI_GB) ? (G - g0) : PSI_GB;
                int ns = 0;
                if (int e = tic(st)) return e;
                if (loop)
                    for (int g = 0; g < gb; ++g)
                        ns = launch_psi2(st, rd2, lg2, dWt + (long)(g0 + g) * N + r0, dZp, dA, rc, M, Qp, var * var, ld,
                                         part + (size_t)g * psi2_nsplit(rc, M) * ld * ld);
                else ns = launch_psi2_multi(st, rd2, lg2, dWt + (long)g0 * N + r0, N, gb, dZp, dA, rc, M, Qp, var * var, ld, part);
                if (int e = toc(st)) return e;
                for (int g = 0; g < gb; ++g)
                    launch_psi2_combine(st, part + (size_t)g * ns * ld * ld, ld, M, ns, nch > 0, out + (size_t)(g0 + g) * M * M, M);
            }
        }
        return 0;
    }
};
}  // namespace

// psi2_g = sum_n W[n][g] psi2n for g < G (G x M x M out).  loop: the single-mask kernel once per group; ms_out: the kernels' stream time
static int psi2_groups(const char* where, int device, double variance, const double* lengthscale, int ard, const double* Z, int64_t M,
                       const double* mu, const double* S, int64_t N, int D, const double* W, int G, int loop, double* psi2_out,
                       double* ms_out) {
    if (!psi2_out) PART_FAIL("%s: NULL output", where);
    HIP_CHECK(hipSetDevice(device));
    GroupInputs in;
    if (int rc = in.load(where, variance, lengthscale, ard, Z, M, mu, S, N, D, W, G)) return rc;
    hipStream_t st = 0;
    DevBuf part, d2;
    HIP_CHECK(part.alloc((size_t)PSI_GB * psi2_nsplit(in.chunk, M) * in.ld * in.ld));
    HIP_CHECK(d2.alloc((size_t)G * M * M));
    if (int rc = in.psi2_all(st, loop, part, d2)) return rc;
    HIP_CHECK(hipMemcpy(psi2_out, d2, sizeof(double) * G * M * M, hipMemcpyDeviceToHost));
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipGetLastError());
    if (ms_out) *ms_out = in.ms;
    return 0;
}

// The five gradients of sum_g sum(sym(dL_dpsi2_g) * psi2_g), psi2_g = sum_n W[n][g] psi2n
static int psi_grad_groups(const char* where, int device, double variance, const double* lengthscale, int ard, const double* Z,
                           int64_t M, const double* mu, const double* S, int64_t N, int D, const double* W, int G,
                           const double* dL_dpsi2, int loop, double* dvar_out, double* dl_out, double* dZ_out, double* dmu_out,
                           double* dS_out, double* ms_out) {
    if (!(dL_dpsi2 && dvar_out && dl_out && dZ_out && dmu_out && dS_out)) PART_FAIL("%s: NULL argument", where);
    HIP_CHECK(hipSetDevice(device));
    GroupInputs in;
    if (int rc = in.load(where, variance, lengthscale, ard, Z, M, mu, S, N, D, W, G)) return rc;
    hipStream_t st = 0;
    const int Qp = in.Qp, RL = 1 + 2 * Qp;
    const long chunk = in.chunk, ld = in.ld, mpad = in.mpad, mt = (M + 15) / 16, nzb = (chunk + PSI_GROWS - 1) / PSI_GROWS;
    DevBuf dRaw, dL2, dPsi2, part, Ppart, P2s, Zpart, Zs2, dMuO, dSO, rowrec, rec, zz;
    std::vector<double> zs2((size_t)mpad * Qp, 0.0), zzh((size_t)M * 2 * Qp), zzs((size_t)M * 2 * Qp, 0.0);
    std::vector<double> sums((size_t)(1 + Qp), 0.0), csum((size_t)(1 + Qp));
    HIP_CHECK(part.alloc((size_t)PSI_GB * psi2_nsplit(chunk, M) * ld * ld));
    HIP_CHECK(dPsi2.alloc((size_t)G * M * M));
    HIP_CHECK(dRaw.alloc((size_t)G * M * M));
    HIP_CHECK(dL2.alloc((size_t)G * M * M));
    HIP_CHECK(Ppart.alloc((size_t)mt * chunk * RL));
    HIP_CHECK(P2s.alloc((size_t)chunk * RL));
    HIP_CHECK(Zpart.alloc((size_t)nzb * mpad * Qp));
    HIP_CHECK(hipMemset(Zpart, 0, sizeof(double) * nzb * mpad * Qp));       // the kernels write rows < round_up(M, 16) only
    HIP_CHECK(Zs2.alloc((size_t)mpad * Qp));
    HIP_CHECK(dMuO.alloc(chunk * D));
    HIP_CHECK(dSO.alloc(chunk * D));
    HIP_CHECK(rowrec.alloc((size_t)chunk * (1 + Qp)));
    HIP_CHECK(rec.alloc(1 + Qp));
    HIP_CHECK(zz.alloc((size_t)M * 2 * Qp));
    // psi2_g first (LS_g = dL_g * psi2_g carries the z_m - z_o terms, per group, added in group order), then the row passes
    if (int rc = in.psi2_all(st, loop, part, dPsi2)) return rc;
    in.ms = 0.0;                                                            // (this call reports its gradient kernels)
    HIP_CHECK(hipMemcpy(dRaw, dL_dpsi2, sizeof(double) * G * M * M, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_psi_symmetrise_groups, dim3((unsigned)((M + 255) / 256), (unsigned)M, (unsigned)G), dim3(256), 0, st,
                       dRaw.p, (long)M, dL2.p);
    for (int g = 0; g < G; ++g) {
        launch_psi2_zz(st, dL2 + (size_t)g * M * M, dPsi2 + (size_t)g * M * M, (long)M, in.dZp, (long)M, Qp, zz);
        HIP_CHECK(hipMemcpy(zzh.data(), zz, sizeof(double) * zzh.size(), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < zzh.size(); ++k) zzs[k] += zzh[k];
    }
    int nch = 0;
    for (long r0 = 0; r0 < N; r0 += PSI_CHUNK, ++nch) {
        const long rc = (N - r0 < PSI_CHUNK) ? (N - r0) : PSI_CHUNK;
        const int nb = (int)((rc + PSI_GROWS - 1) / PSI_GROWS);
        in.fill(st, r0, rc);
        if (loop) {
            for (int g = 0; g < G; ++g) {
                if (int e = in.tic(st)) return e;
                launch_psi2_grad(st, in.rd2, in.lg2, in.dWt + (long)g * N + r0, in.dZp, in.dA, dL2 + (size_t)g * M * M, M, rc, M,
                                 mpad, Qp, in.var * in.var, Ppart, Zpart);
                if (int e = in.toc(st)) return e;
                launch_sum_splits(st, Ppart, rc * RL, (int)mt, g > 0, P2s);
                launch_sum_splits(st, Zpart, mpad * Qp, nb, nch > 0 || g > 0, Zs2);
            }
        } else {
            for (int g0 = 0; g0 < G; g0 += PSI_GB) {
                const int gb = (G - g0 < PSI_GB) ? (G - g0) : PSI_GB;
                if (int e = in.tic(st)) return e;
                launch_psi2_grad_multi(st, in.rd2, in.lg2, in.dWt + (long)g0 * N + r0, N, gb, in.dZp, in.dA, dL2 + (size_t)g0 * M * M,
                                       (long)M * M, M, rc, M, mpad, Qp, in.var * in.var, Ppart, Zpart);
                if (int e = in.toc(st)) return e;
                launch_sum_splits(st, Ppart, rc * RL, (int)mt, g0 > 0, P2s);
                launch_sum_splits(st, Zpart, mpad * Qp, nb, nch > 0 || g0 > 0, Zs2);
            }
        }
        launch_psi_rowfinish(st, nullptr, P2s, in.dS + r0 * D, in.dA, rc, D, Qp, dMuO, dSO, rowrec);
        launch_reduce_partials(st, rowrec, (int)rc, 1 + Qp, rec);
        HIP_CHECK(hipMemcpy(dmu_out + r0 * D, dMuO, sizeof(double) * rc * D, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(dS_out + r0 * D, dSO, sizeof(double) * rc * D, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(csum.data(), rec, sizeof(double) * (1 + Qp), hipMemcpyDeviceToHost));
        for (int k = 0; k <= Qp; ++k) sums[(size_t)k] += csum[(size_t)k];                          // chunks in row order
    }
    HIP_CHECK(hipMemcpy(zs2.data(), Zs2, sizeof(double) * zs2.size(), hipMemcpyDeviceToHost));
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipGetLastError());
    // dZ = 2 sum_{n,o} c2 L2 d  -  a_q sum_o LS (z_m - z_o); variance and lengthscales through the reduction records (psi.hip)
    for (long i = 0; i < M; ++i)
        for (int q = 0; q < D; ++q) dZ_out[i * D + q] = 2.0 * zs2[(size_t)i * Qp + q] - in.a[(size_t)q] * zzs[(size_t)i * 2 * Qp + q];
    const int groups = (D + 31) / 32;
    std::vector<double> recs((size_t)groups * GP_STRIDE, 0.0), th(in.spec.theta.size());
    recs[0] = sums[0];
    for (int q = 0; q < D; ++q) {
        double zq = 0.0;
        for (long i = 0; i < M; ++i) zq += zzs[(size_t)i * 2 * Qp + Qp + q];
        const double lq = sums[(size_t)(1 + q)] + 0.5 * in.a[(size_t)q] * zq;
        recs[(size_t)(q / 32) * GP_STRIDE + 2 + (q % 32)] = -lq;
        recs[1] -= lq;
    }
    part_dtheta(in.spec, recs.data(), nullptr, th.data());
    *dvar_out = th[0];
    for (size_t k = 1; k < th.size(); ++k) dl_out[k - 1] = th[k];
    if (ms_out) *ms_out = in.ms;
    return 0;
}

extern "C" {

int mi355gp_psi_groups_batch(void) { return PSI_GB; }

int mi355gp_rbf_psi2_groups(int device, double variance, const double* lengthscale, int ard, const double* Z, int64_t M,
                            const double* mu, const double* S, int64_t N, int D, const double* W, int G, double* psi2_out) {
    return psi2_groups("mi355gp_rbf_psi2_groups", device, variance, lengthscale, ard, Z, M, mu, S, N, D, W, G, 0, psi2_out, nullptr);
}

int mi355gp_rbf_psi_grad_groups(int device, double variance, const double* lengthscale, int ard, const double* Z, int64_t M,
                                const double* mu, const double* S, int64_t N, int D, const double* W, int G,
                                const double* dL_dpsi2, double* dvar_out, double* dl_out, double* dZ_out, double* dmu_out,
                                double* dS_out) {
    return psi_grad_groups("mi355gp_rbf_psi_grad_groups", device, variance, lengthscale, ard, Z, M, mu, S, N, D, W, G, dL_dpsi2, 0,
                           dvar_out, dl_out, dZ_out, dmu_out, dS_out, nullptr);
}

// ---- diagnostics (include/mi355gp_debug_sparse_missing.h): the same calls with the replaced route and the kernels' stream time ----
int mi355gp_dbg_rbf_psi2_groups(int device, double variance, const double* lengthscale, int ard, const double* Z, int64_t M,
                                const double* mu, const double* S, int64_t N, int D, const double* W, int G, int loop,
                                double* psi2_out, double* ms_out) {
    return psi2_groups("mi355gp_dbg_rbf_psi2_groups", device, variance, lengthscale, ard, Z, M, mu, S, N, D, W, G, loop, psi2_out, ms_out);
}

int mi355gp_dbg_rbf_psi_grad_groups(int device, double variance, const double* lengthscale, int ard, const double* Z, int64_t M,
                                    const double* mu, const double* S, int64_t N, int D, const double* W, int G,
                                    const double* dL_dpsi2, int loop, double* dvar_out, double* dl_out, double* dZ_out,
                                    double* dmu_out, double* dS_out, double* ms_out) {
    return psi_grad_groups("mi355gp_dbg_rbf_psi_grad_groups", device, variance, lengthscale, ard, Z, M, mu, S, N, D, W, G, dL_dpsi2, loop,
                           dvar_out, dl_out, dZ_out, dmu_out, dS_out, ms_out);
}

}  // extern "C"
