// epdtc.hip -- EPDTC on the sparse context (C-ABI mi355gp_epdtc_*, include/mi355gp_epdtc.h): expectation propagation for the
// Bernoulli likelihood with the probit link over the DTC posterior
//   q(f) = N(mu, Sigma),  Sigma = Knm LLT^-1 Kmn,  LLT = Kmm + Kmn diag(tau) Knm,  mu = Sigma v
// (GPy/inference/latent_function_inference/expectation_propagation.py:145-185 posteriorParamsDTC, :436-578 EPDTC).
//
// The reference's sequential sweep refactors LLT and solves against all of Kmn after EVERY site (:149-156), O(N (M^3 + M^2 N))
// per sweep.  Here site i needs only Sigma_ii = k_i^T P k_i and mu_i = k_i^T gamma with P = LLT^-1 (M x M) and gamma = P Kmn v
// (M), and the sweep runs in blocks of EPB = 64 consecutive sites of the update order.  With K_b = K(X[block], Z) (rows k_j^T):
//   before   A0 = K_b P, G0 = A0 K_b^T (symmetrised), h = K_b gamma                                  (two tile GEMMs, a row kernel)
//   sites    ONE launch of ONE workgroup visits the block's sites in order (k_epdtc_sites): G = Sigma over the block and h = mu
//            over the block are kept current under the rank-one updates, and the change of P is collected as
//            R = sum_j c_j r_j r_j^T, r_j = e_j - R G0[:, j], the change of gamma as gc = sum_j kappa_j r_j
//   after    P -= A0^T R A0 as W1 = T^T A0 (T's column j is r_j) and P -= W1^T diag(c) W1; gamma += A0^T gc       (two tile GEMMs)
// c_j may be negative (a site whose precision falls), so no square roots are taken.  P and gamma are rebuilt from a
// factorisation of LLT by every mi355gp_epdtc_recompute (the reference's _recompute, :174-185, after every sweep), so rounding
// does not accumulate across sweeps.  One sweep is 4 N M^2 flops of tile GEMM and O(N EPB^2) of site work.
//
// EPB: the site kernel's state is two EPB x EPB fp64 matrices in LDS, G and U = R G0.  At 64 that is 64 KiB; at 128 it would be
// 256 KiB against the CU's 160 KiB, so 64 is what fits.
// A sweep is a plain sequence of launches on one stream; every reduction has a fixed order and nothing is accumulated
// atomically: the same inputs give the same bytes.
//
// Buffers of the context in use between begin and the last sweep: LB (LLT, then its factor), XB (its inverse), Bi (LLT^-1, lower
// tiles), psi2part / psi1Y / cvec (recompute's sums), Kfu / T (row chunks), dBeta / dV (tau, v).  Kmm, P, gamma and the
// buffers of a block belong to the EPDTC state.  Padding convention as in pep.hip.
#include <cmath>
#include <vector>

#include "../../include/mi355gp_epdtc.h"
#include "probit.h"
#include "sparse_ctx.h"

#define EPB 64                                     // sites per block
#define EP_SITE_LDS ((2 * EPB * EPB + 8 * EPB) * (int)sizeof(double))

struct EpdtcState {
    long mp = 0, chunk = 0, n = 0;
    bool begun = false, have_P = false;            // Kmm of the current parts and Z is in place / P and gamma of a recompute are
    DevBuf Kmm, P, gam;                            // mp x mp (lower tiles), mp x mp (both triangles), mp
    DevBuf Kc, A0, W1, W2, G0, Tm, blk;            // (chunk + 128) x mp; 128 x mp (three); 128 x 128 (two); [h | c | gc] (3 x 128)
    DevBuf Xg, site;                               // n x D inputs in sweep order; 8 N-vectors in sweep order
    DevArr<long long> order;                       // n
};

void epdtc_release(mi355gp_sparse* s) {
    delete s->epdtc;
    s->epdtc = nullptr;
}

static int epdtc_state(mi355gp_sparse* s) {
    EpdtcState* pp = s->epdtc;
    if (pp && pp->mp == s->mp && pp->chunk == s->chunk && pp->n == s->n) return 0;
    epdtc_release(s);
    pp = new EpdtcState();
    s->epdtc = pp;
    pp->mp = s->mp;
    pp->chunk = s->chunk;
    pp->n = s->n;
    const size_t mp = (size_t)s->mp;
    HIP_CHECK(pp->Kmm.alloc(mp * mp));
    HIP_CHECK(pp->P.alloc(mp * mp));
    HIP_CHECK(pp->gam.alloc(mp));
    HIP_CHECK(pp->Kc.alloc((size_t)(s->chunk + NB) * mp));
    HIP_CHECK(pp->A0.alloc(NB * mp));
    HIP_CHECK(pp->W1.alloc(NB * mp));
    HIP_CHECK(pp->W2.alloc(NB * mp));
    HIP_CHECK(pp->G0.alloc(NB * NB));
    HIP_CHECK(pp->Tm.alloc(NB * NB));
    HIP_CHECK(pp->blk.alloc(3 * NB));
    HIP_CHECK(pp->Xg.alloc((size_t)s->n * s->D));
    HIP_CHECK(pp->site.alloc((size_t)8 * s->n));
    HIP_CHECK(pp->order.alloc((size_t)s->n));
    return 0;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------
// LLT = Kmm + the split-K partial Grams in the order of the splits, on the lower tiles (what the factorisation reads)
__global__ void k_epdtc_llt(const double* __restrict__ Kmm, const double* __restrict__ part, long mp, int nsplit,
                            double* __restrict__ out) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (j >= mp || j / NB > i / NB) return;
    double v = Kmm[i * mp + j];
    for (int k = 0; k < nsplit; ++k) v += part[(long)k * mp * mp + i * mp + j];
    out[i * mp + j] = v;
}

// Xg[p][:] = X[order[p]][:]
__global__ void k_epdtc_gather(const double* __restrict__ X, const long long* __restrict__ order, long n, int D,
                               double* __restrict__ Xg) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * D) return;
    const long p = e / D, d = e % D;
    Xg[e] = X[(long)order[p] * D + d];
}

// The nb <= EPB sites at sweep positions p0 .. p0 + nb - 1, in order, by one workgroup.  LDS: G (Sigma over the block, kept
// bitwise symmetric: its row j is read for its column), Ut = (R G0)^T, h (mu over the block), the block's tau / v / labels, and
// the current site's g = G[:, j], r = e_j - U[:, j].  Per site (expectation_propagation.py:27-29, :52-68, bernoulli.py:73-79):
//   s = max(G_jj, eps) (+ 1e-8 for the first site of a run, :538), m = h_j; cavity, moments, site update with tau clipped at eps
//   c = dtau / (1 + dtau G_jj), kappa = dv - c (m + dv G_jj)
//   G -= c g g^T, h += kappa g, U += c r g^T (G0 r = g), gc += kappa r, T[:, j] = r
// Every thread does the scalar work of a site from the same LDS words (no broadcast, no second barrier); thread 0 stores it.
// The sums are elementwise: nothing is reduced across threads.  Outputs T (128 x 128, T[i][j] = r_j[i]), c and gc (128) are
// zero outside the block.
__global__ __launch_bounds__(256) void k_epdtc_sites(const double* __restrict__ G0, const double* __restrict__ h0, int nb, long p0,
                                                     int first, double eta, double delta, const double* __restrict__ ysign,
                                                     double* __restrict__ tau, double* __restrict__ v, double* __restrict__ cav_tau,
                                                     double* __restrict__ cav_v, double* __restrict__ logZ,
                                                     double* __restrict__ mu_hat, double* __restrict__ s2_hat,
                                                     double* __restrict__ Tout, double* __restrict__ cout, double* __restrict__ gcout) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* G = lds;
    double* Ut = G + EPB * EPB;
    double* h = Ut + EPB * EPB;
    double* g = h + EPB;
    double* r = g + EPB;
    double* gc = r + EPB;
    double* tl = gc + EPB;
    double* vl = tl + EPB;
    double* yl = vl + EPB;
    const int t = threadIdx.x;
    for (int e = t; e < EPB * EPB; e += 256) {
        const int i = e / EPB, k = e % EPB;
        G[e] = (i < nb && k < nb) ? 0.5 * (G0[i * NB + k] + G0[k * NB + i]) : 0.0;
        Ut[e] = 0.0;
    }
    for (int e = t; e < NB * NB; e += 256) Tout[e] = 0.0;
    if (t < NB) cout[t] = gcout[t] = 0.0;
    if (t < EPB) {
        const bool in = t < nb;
        h[t] = in ? h0[t] : 0.0;
        gc[t] = 0.0;
        tl[t] = in ? tau[p0 + t] : 0.0;
        vl[t] = in ? v[p0 + t] : 0.0;
        yl[t] = in ? ysign[p0 + t] : 1.0;
    }
    __syncthreads();
    const double eps = 2.220446049250313e-16;
    for (int j = 0; j < nb; ++j) {
        const double gjj = G[j * EPB + j], mj = h[j];
        double sjj = fmax(gjj, eps);
        if (first && p0 + j == 0) sjj += 1e-8;
        const double tau_prev = tl[j];
        const double ct = 1.0 / sjj - eta * tau_prev;
        const double cv = mj / sjj - eta * vl[j];
        const double sg = yl[j], q = ct * ct + ct, rq = sqrt(q);
        const double z = sg * cv / rq;
        double lZ, ratio;
        probit_logcdf(z, &lZ, &ratio);
        const double muh = cv / ct + sg * ratio / rq;
        const double s2h = 1.0 / ct - (ratio / q) * (z + ratio);
        double dtau = delta / eta * (1.0 / s2h - 1.0 / sjj);
        const double dv = delta / eta * (muh / s2h - mj / sjj);
        double tnew = tau_prev + dtau;
        if (tnew < eps) {
            tnew = eps;
            dtau = tnew - tau_prev;
        }
        const double c = dtau / (1.0 + dtau * gjj);
        const double kappa = dv - c * (mj + dv * gjj);
        if (t < EPB) {
            g[t] = G[j * EPB + t];
            r[t] = (t == j ? 1.0 : 0.0) - Ut[j * EPB + t];
        }
        __syncthreads();
        if (t < EPB) {
            h[t] = fma(kappa, g[t], h[t]);
            gc[t] = fma(kappa, r[t], gc[t]);
            Tout[t * NB + j] = r[t];
        }
        if (t == 0) {
            const long p = p0 + j;
            tau[p] = tnew;
            v[p] = vl[j] + dv;
            cav_tau[p] = ct;
            cav_v[p] = cv;
            logZ[p] = lZ;
            mu_hat[p] = muh;
            s2_hat[p] = s2h;
            cout[j] = c;
        }
        for (int e = t; e < EPB * EPB; e += 256) {
            const int i = e / EPB, k = e % EPB;
            G[e] = fma(-c, g[i] * g[k], G[e]);
            Ut[e] = fma(c, g[i] * r[k], Ut[e]);              // Ut[i][k] = U[k][i] += c r_k g_i
        }
        __syncthreads();
    }
    if (t < EPB) gcout[t] = gc[t];
}

// After a block: W2 = diag(c) W1 (128 x mp) and gamma += A0^T gc, one thread per column, the rows in order
__global__ void k_epdtc_block_end(const double* __restrict__ A0, const double* __restrict__ W1, const double* __restrict__ c,
                                  const double* __restrict__ gc, long mp, int nb, double* __restrict__ W2,
                                  double* __restrict__ gam) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= mp) return;
    double a = 0.0;
    for (int i = 0; i < NB; ++i) {
        W2[i * mp + j] = i < nb ? c[i] * W1[i * mp + j] : 0.0;
        if (i < nb) a = fma(A0[i * mp + j], gc[i], a);
    }
    gam[j] += a;
}

// ---- host helpers ----------------------------------------------------------------------------------------------------------
static long epdtc_rows_pad(const mi355gp_sparse* s, long rc) {
    const long a = round_up(rc, NB), b = round_up(rc, 16L * s->splitk);
    return a > b ? a : b;
}

static int epdtc_check(const mi355gp_sparse* s, const char* where) {
    if (!s || s->n <= 0) PART_FAIL("%s: set_data first", where);
    if (s->Dy != 1) PART_FAIL("%s: %d output columns; EPDTC takes one (expectation_propagation.py:442)", where, s->Dy);
    if (sharded(s)) PART_FAIL("%s: a row-sharded context is not supported by EPDTC", where);
    if (s->dSvar) PART_FAIL("%s: the context holds input variances; EPDTC takes certain inputs (mi355gp_sparse_set_data discards them)", where);
    return 0;
}

static int epdtc_check_vec(const double* x, long n, bool positive, const char* where, const char* name) {
    for (long i = 0; i < n; ++i)
        if (!std::isfinite(x[i]) || x[i] < 0.0 || (positive && !(x[i] > 0.0)))
            PART_FAIL("%s: %s[%ld] = %g: every entry must be finite and %s", where, name, i, x[i], positive ? "positive" : "not negative");
    return 0;
}

static void epdtc_ms(mi355gp_sparse* s, double* ms_out) {
    if (!ms_out) return;
    float ms = 0.0f;
    *ms_out = hipEventElapsedTime(&ms, s->ev[4], s->ev[5]) == hipSuccess ? ms : 0.0;
}

extern "C" {

int mi355gp_epdtc_begin(mi355gp_sparse* s, int nparts, const mi355gp_part* parts, const double* Z, int64_t M, double jitter) {
    const char* where = "mi355gp_epdtc_begin";
    if (int rc = epdtc_check(s, where)) return rc;
    ARG_CHECK(parts && Z && M > 0, "mi355gp_epdtc_begin: bad arguments");
    if (!(jitter >= 0.0) || !std::isfinite(jitter)) PART_FAIL("%s: jitter %g must be finite and not negative", where, jitter);
    EngineShared gate(s->device);
    if (int rc = sparse_open(s, nparts, parts, M)) return rc;
    if (int rc = epdtc_state(s)) return rc;
    EpdtcState* pp = s->epdtc;
    pp->begun = pp->have_P = false;
    hipStream_t st = s->st;
    const long mp = s->mp;
    s->mfma_prof.on = false;
    if (int rc = sparse_start(s, Z, nullptr, 0)) return rc;
    // Kmm = K(Z) + jitter I kept for every recompute; Lm = jitchol(Kmm) (:453-454) for its info
    auto rebuild_kmm = [&]() {
        build_kmm(s, pp->Kmm, s->T1, jitter, /*lower_only=*/1, st);
        (void)hipMemcpyAsync(s->Lm, pp->Kmm, sizeof(double) * mp * mp, hipMemcpyDeviceToDevice, st);
    };
    rebuild_kmm();
    if (int rc = potrf_checked(st, s->Lm, s->Xm, s->Tm, nullptr, mp, &s->ws, &s->h_info[0], rebuild_kmm)) return rc;
    if (int rc = sparse_finish(s, 0, nullptr)) return rc;          // (info > 0: the caller adds jitter)
    s->kmm_jitter = jitter;
    pp->begun = true;
    return 0;
}

int mi355gp_epdtc_recompute(mi355gp_sparse* s, const double* tau, const double* v, double* mu_out, double* sigdiag_out,
                            double* ms_out) {
    const char* where = "mi355gp_epdtc_recompute";
    if (int rc = epdtc_check(s, where)) return rc;
    EpdtcState* pp = s->epdtc;
    ARG_CHECK(pp && pp->begun && pp->mp == s->mp && pp->n == s->n, "mi355gp_epdtc_recompute: call mi355gp_epdtc_begin first");
    ARG_CHECK(tau && v && mu_out && sigdiag_out, "mi355gp_epdtc_recompute: NULL argument");
    const long n = s->n, m = s->m, mp = s->mp, chunk = s->chunk;
    if (int rc = epdtc_check_vec(tau, n, false, where, "tau")) return rc;
    for (long i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) PART_FAIL("%s: v[%ld] = %g is not finite", where, i, v[i]);
    HIP_CHECK(hipSetDevice(s->device));
    EngineShared gate(s->device);
    hipStream_t st = s->st;
    pp->have_P = false;
    s->h_info[0] = s->h_info[1] = 0;
    const bool one_chunk = (n <= chunk);
    HIP_CHECK(hipMemcpyAsync(s->dBeta, tau, sizeof(double) * n, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(s->dV, v, sizeof(double) * n, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipEventRecord(s->ev[4], st));
    // LLT = Kmm + Kmn diag(tau) Knm (:175) by the row-weighted split-K Gram, and Kmn v
    HIP_CHECK(hipMemsetAsync(s->psi1Y, 0, sizeof(double) * mp, st));
    int nch = 0;
    for (long r0 = 0; r0 < n; r0 += chunk, ++nch) {
        const long rc = (n - r0 < chunk) ? (n - r0) : chunk;
        const long rz = epdtc_rows_pad(s, rc);
        if (int rc2 = sparse_cross_rows(s, r0, rc, 0, rz, nullptr)) return rc2;
        HIP_CHECK(hipMemsetAsync(s->T + rc * mp, 0, sizeof(double) * (rz - rc) * mp, st));
        launch_rowscale_sqrt(st, s->Kfu, mp, rc, mp, s->dBeta + r0, s->T);
        launch_gram_splitk(st, s->T, mp, round_up(rc, 16L * s->splitk), mp, s->splitk, nch > 0, s->psi2part);
        const int ns = launch_colreduce_multi(st, s->Kfu, mp, rc, mp, s->dV + r0, 1, 1, 1, 0, s->colPart);
        launch_sum_splits(st, s->colPart, mp, ns, 1, s->psi1Y);
    }
    auto build_llt = [&]() {
        hipLaunchKernelGGL(k_epdtc_llt, grid2d(mp, mp), dim3(256), 0, st, (const double*)pp->Kmm, (const double*)s->psi2part, mp,
                           s->splitk, s->LB);
    };
    build_llt();
    // L = chol(LLT) (:176), XB = L^-1, Bi = LLT^-1 (lower tiles) -> P; gamma = L^-T L^-1 Kmn v
    if (int rc = potrf_checked(st, s->LB, s->XB, s->Tm, s->Bi, mp, &s->ws, &s->h_info[1], build_llt)) return rc;
    launch_mm_sym(st, s->Bi, mp, pp->P);
    launch_trmv_lower(st, s->XB, mp, mp, s->psi1Y, 1, s->cvec);
    launch_trmv_lower_T(st, s->XB, mp, mp, s->cvec, 1, pp->gam, s->trmvPart);
    // V = L^-1 Kmn (:177): Sigma_diag_n = |V[:, n]|^2, mu_n = V[:, n]^T (L^-1 Kmn v) (:181-183)
    double* dMu = pp->site;
    double* dSd = pp->site + n;
    for (long r0 = 0; r0 < n; r0 += chunk) {
        const long rc = (n - r0 < chunk) ? (n - r0) : chunk;
        if (!one_chunk)                                       // a single chunk is still resident
            if (int rc2 = sparse_cross_rows(s, r0, rc, 0, epdtc_rows_pad(s, rc), nullptr)) return rc2;
        launch_gemm(st, 0, 0, round_up(rc, NB), mp, mp, s->Kfu, mp, s->XB, mp, s->T, mp, 1.0, 0.0);
        launch_rowdots(st, s->T, s->T, mp, rc, m, s->cvec, 1, dMu + r0, dSd + r0);
    }
    HIP_CHECK(hipEventRecord(s->ev[5], st));
    HIP_CHECK(hipMemcpyAsync(mu_out, dMu, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(sigdiag_out, dSd, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    if (int rc = sparse_finish(s, 0, nullptr)) return rc;          // (info > 0: LLT is not positive definite)
    epdtc_ms(s, ms_out);
    pp->have_P = true;
    return 0;
}

int mi355gp_epdtc_sweep(mi355gp_sparse* s, const int64_t* order, const double* ysign, double eta, double delta, int first,
                        double* tau, double* v, double* cav_tau_out, double* cav_v_out, double* logZhat_out,
                        double* mu_hat_out, double* sigma2_hat_out, double* ms_out) {
    const char* where = "mi355gp_epdtc_sweep";
    if (int rc = epdtc_check(s, where)) return rc;
    EpdtcState* pp = s->epdtc;
    ARG_CHECK(pp && pp->begun && pp->have_P && pp->mp == s->mp && pp->n == s->n,
              "mi355gp_epdtc_sweep: no P and gamma are resident: call mi355gp_epdtc_recompute first");
    ARG_CHECK(order && ysign && tau && v && cav_tau_out && cav_v_out && logZhat_out && mu_hat_out && sigma2_hat_out,
              "mi355gp_epdtc_sweep: NULL argument");
    ARG_CHECK(std::isfinite(eta) && eta > 0.0 && std::isfinite(delta) && delta > 0.0, "mi355gp_epdtc_sweep: eta and delta must be positive");
    const long n = s->n, m = s->m, mp = s->mp, chunk = s->chunk;
    if (int rc = epdtc_check_vec(tau, n, false, where, "tau")) return rc;
    // the N-vectors travel in sweep order: position p holds site order[p]
    std::vector<double> hin((size_t)3 * n), hout((size_t)7 * n);
    {
        std::vector<char> seen((size_t)n, 0);
        for (long p = 0; p < n; ++p) {
            const int64_t i = order[p];
            if (i < 0 || i >= n || seen[(size_t)i]) PART_FAIL("%s: order is not a permutation of 0 .. N-1 (order[%ld] = %lld)", where, p, (long long)i);
            seen[(size_t)i] = 1;
            if (ysign[i] != 1.0 && ysign[i] != -1.0) PART_FAIL("%s: ysign[%lld] = %g is neither +1 nor -1", where, (long long)i, ysign[i]);
            if (!std::isfinite(v[i])) PART_FAIL("%s: v[%lld] = %g is not finite", where, (long long)i, v[i]);
            hin[(size_t)p] = tau[i];
            hin[(size_t)(n + p)] = v[i];
            hin[(size_t)(2 * n + p)] = ysign[i];
        }
    }
    static_assert(sizeof(long long) == sizeof(int64_t), "the order is uploaded as it is");
    HIP_CHECK(hipSetDevice(s->device));
    EngineShared gate(s->device);
    hipStream_t st = s->st;
    pp->have_P = false;                                        // (P and gamma are those of the sites after this sweep only on success)
    double* dv[8];
    for (int k = 0; k < 8; ++k) dv[k] = pp->site + (size_t)k * n;         // tau, v, ysign, cav tau, cav v, log Z_hat, mu_hat, sigma2_hat
    HIP_CHECK(hipMemcpyAsync(dv[0], hin.data(), sizeof(double) * 3 * n, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(pp->order, order, sizeof(int64_t) * n, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipEventRecord(s->ev[4], st));
    hipLaunchKernelGGL(k_epdtc_gather, dim3((unsigned)((n * s->D + 255) / 256)), dim3(256), 0, st, (const double*)s->dX,
                       (const long long*)pp->order, n, s->D, (double*)pp->Xg);
    static bool opted = false;
    if (!opted) {
        HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_epdtc_sites), hipFuncAttributeMaxDynamicSharedMemorySize, EP_SITE_LDS));
        opted = true;
    }
    double *h = pp->blk, *cc = pp->blk + NB, *gc = pp->blk + 2 * NB;
    for (long c0 = 0; c0 < n; c0 += chunk) {
        const long rc = (n - c0 < chunk) ? (n - c0) : chunk;
        // K(X[order[c0 ..]], Z) of the whole chunk once; the rows after it that a block's 128-row products read are zero
        scale_for_parts(s, pp->Xg + c0 * s->D, rc, chunk, false);
        HIP_CHECK(hipMemsetAsync(pp->Kc, 0, sizeof(double) * (rc + NB) * mp, st));
        build_cross_chunk(s, rc, pp->Kc, s->T);
        for (long o = 0; o < rc; o += EPB) {
            const int nb = (int)((rc - o < EPB) ? (rc - o) : EPB);
            const double* Kb = pp->Kc + o * mp;
            launch_gemm(st, 0, 1, NB, mp, mp, Kb, mp, pp->P, mp, pp->A0, mp, 1.0, 0.0);                  // A0 = K_b P
            launch_gemm(st, 0, 0, NB, NB, mp, pp->A0, mp, Kb, mp, pp->G0, NB, 1.0, 0.0);                 // G0 = A0 K_b^T
            launch_rowdots(st, Kb, nullptr, mp, nb, m, pp->gam, 1, h, nullptr);                          // h = K_b gamma
            hipLaunchKernelGGL(k_epdtc_sites, dim3(1), dim3(256), EP_SITE_LDS, st, (const double*)pp->G0, (const double*)h, nb,
                               c0 + o, first, eta, delta, (const double*)dv[2], dv[0], dv[1], dv[3], dv[4], dv[5], dv[6], dv[7],
                               (double*)pp->Tm, cc, gc);
            launch_gemm(st, 1, 1, NB, mp, NB, pp->Tm, NB, pp->A0, mp, pp->W1, mp, 1.0, 0.0);             // W1 = T^T A0
            hipLaunchKernelGGL(k_epdtc_block_end, dim3((unsigned)((mp + 255) / 256)), dim3(256), 0, st, (const double*)pp->A0,
                               (const double*)pp->W1, (const double*)cc, (const double*)gc, mp, nb, (double*)pp->W2, (double*)pp->gam);
            launch_gemm(st, 1, 1, mp, mp, NB, pp->W1, mp, pp->W2, mp, pp->P, mp, -1.0, 1.0);             // P -= W1^T diag(c) W1
        }
    }
    HIP_CHECK(hipEventRecord(s->ev[5], st));
    HIP_CHECK(hipMemcpyAsync(hout.data(), dv[0], sizeof(double) * 2 * n, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(hout.data() + 2 * n, dv[3], sizeof(double) * 5 * n, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    double* dst[7] = {tau, v, cav_tau_out, cav_v_out, logZhat_out, mu_hat_out, sigma2_hat_out};
    for (int k = 0; k < 7; ++k)
        for (long p = 0; p < n; ++p) dst[k][order[p]] = hout[(size_t)k * n + p];
    epdtc_ms(s, ms_out);
    pp->have_P = true;
    return 0;
}

int mi355gp_epdtc_inference(mi355gp_sparse* s, int nparts, const mi355gp_part* parts, const double* Z, int64_t M,
                            const double* tau, const double* v, double jitter, double* out_scalars, double* dtheta_out,
                            double* dZ_out, double* wv_out, double* dLdR_out, double* stage_ms) {
    const char* where = "mi355gp_epdtc_inference";
    if (int rc = epdtc_check(s, where)) return rc;
    ARG_CHECK(parts && Z && M > 0 && tau && v && out_scalars && dLdR_out, "mi355gp_epdtc_inference: bad arguments");
    if (!(jitter >= 0.0) || !std::isfinite(jitter)) PART_FAIL("%s: jitter %g must be finite and not negative", where, jitter);
    const long n = s->n;
    if (int rc = epdtc_check_vec(tau, n, true, where, "tau")) return rc;
    EngineShared gate(s->device);
    if (int rc = sparse_open(s, nparts, parts, M)) return rc;
    if (s->epdtc) s->epdtc->begun = s->epdtc->have_P = false;      // (the evaluation overwrites the buffers of a fit in progress)
    // the targets mu_tilde = v / tau (:482) take the place of the context's Y; the precisions are tau as they are (:487)
    std::vector<double> target((size_t)n), hbeta(tau, tau + n);
    double glob[3] = {0.0, 0.0, 0.0}, trYYT = 0.0;
    for (long i = 0; i < n; ++i) {
        if (!std::isfinite(v[i])) PART_FAIL("%s: v[%ld] = %g is not finite", where, i, v[i]);
        const double y = v[i] / tau[i], yy = y * y;
        target[(size_t)i] = y;
        s->rowYY[(size_t)i] = yy;
        trYYT += yy;
        glob[0] += tau[i];
        glob[1] += log(tau[i]);
        glob[2] += tau[i] * yy;
    }
    s->trYYT = s->trYYT_local = trYYT;
    HIP_CHECK(hipMemcpyAsync(s->dY, target.data(), sizeof(double) * n, hipMemcpyHostToDevice, s->st));
    HIP_CHECK(hipStreamSynchronize(s->st));                        // (target leaves scope with this call; sparse_start reads dY)
    if (int rc = vardtc_evaluate(s, Z, hbeta, glob, jitter, out_scalars, dtheta_out, dZ_out, wv_out, dLdR_out, nullptr, stage_ms))
        return rc;
    s->kmm_jitter = jitter;
    return 0;
}

}  // extern "C"
