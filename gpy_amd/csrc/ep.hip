// ep.hip -- expectation propagation for a non-Gaussian likelihood inside a Laplace session (C-ABI mi355gp_ep_*,
// include/mi355gp.h): the two parts of GPy/inference/latent_function_inference/expectation_propagation.py that are EP and
// nothing else.  Everything after convergence (alpha, the woodbury_inv, dL_dK, the kernel gradients, prediction) is the
// session's existing calls with W = tau_tilde, b = v_tilde.
//
//   mi355gp_ep_recompute   posteriorParams._recompute (:129-143) for a zero prior mean through the session's factor path:
//                          mu = K alpha, diag(Sigma), and (want_sigma) the full Sigma = K - V^T V into the context's A buffer
//   mi355gp_ep_sweep       one pass of _local_updates (:330-351) with parallel_updates=False: per site one small kernel (cavity,
//                          moment matching, site update, copy of row i of Sigma) and one wide kernel (rank-one update of Sigma
//                          and mu, :101-105), 2 N launches on one stream, no host synchronisation in between.  Launch
//                          boundaries are the only ordering; every update is elementwise, so a sweep gives the same bits
//                          from call to call.
//
// Buffers: K in the session's fourth buffer (untouched), A = B, then L_B, then S^1/2 K, then Sigma; B = X = L_B^-1 (kept: the
// session's stage 2); C = V = X S^1/2 K.  No further N x N allocation.  Vectors of the session during a sweep: LV_W tau,
// LV_B v, LV_KA mu, LV_T0 the copied row, LV_T1 / LV_T2 cavity tau / v, LV_U log Z_hat, LV_S the label signs, LV_A the order
// (int64), LV_DIAG diag(Sigma) on the way out; the scalar block carries the two coefficients of the rank-one update.
#include <cmath>
#include <cstring>
#include <vector>

#include "lap_session.h"
#include "probit.h"

#define EP_VGRID(n) dim3((unsigned)(((n) + 255) / 256)), dim3(256)
#define EP_ROWS 8                     // rows of Sigma per workgroup of the wide kernel: eight 16-byte loads in flight per lane

__global__ void k_ep_mul(const double* __restrict__ x, const double* __restrict__ y, long n, double* __restrict__ out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = x[i] * y[i];
}
__global__ void k_ep_sub_scaled(const double* __restrict__ x, const double* __restrict__ sw, const double* __restrict__ t, long n,
                                double* __restrict__ out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = x[i] - sw[i] * t[i];
}
// S[i][i] += add (add != 0), then d[i] = S[i][i]
__global__ void k_ep_diag(double* __restrict__ S, long ld, long n, double add, double* __restrict__ d) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = S[i * ld + i];
    if (add != 0.0) {
        s += add;
        S[i * ld + i] = s;
    }
    d[i] = s;
}
__global__ void k_ep_add_scalar(double* __restrict__ d, long n, double add) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) d[i] += add;
}

// One site (expectation_propagation.py:27-29, :52-68, bernoulli.py:73-79): every workgroup copies its piece of row i of Sigma
// aside (the wide kernel updates that row too, :102); thread 0 of workgroup 0 does the scalar work and leaves the coefficients
// of the rank-one update in coef: [0] = ci = delta_tau / (1 + delta_tau Sigma_ii), [1] = ci (mu_i + Sigma_ii delta_v) - delta_v
__global__ __launch_bounds__(256) void k_ep_site(const double* __restrict__ S, long ld, long n, const long long* __restrict__ order,
                                                 long s, const double* __restrict__ ysign, double eta, double delta,
                                                 const double* __restrict__ mu, double* __restrict__ tau, double* __restrict__ v,
                                                 double* __restrict__ cav_tau, double* __restrict__ cav_v,
                                                 double* __restrict__ logZ, double* __restrict__ row, double* __restrict__ coef) {
    const long i = (long)order[s];
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    if (c < ld) row[c] = c < n ? S[i * ld + c] : 0.0;
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const double sii = S[i * ld + i], mui = mu[i];
    const double ct = 1.0 / sii - eta * tau[i];
    const double cv = mui / sii - eta * v[i];
    cav_tau[i] = ct;
    cav_v[i] = cv;
    const double sg = ysign[i], q = ct * ct + ct, rq = sqrt(q);
    const double z = sg * cv / rq;
    double lZ, r;
    probit_logcdf(z, &lZ, &r);
    logZ[i] = lZ;
    const double mu_hat = cv / ct + sg * r / rq;
    const double sigma2_hat = 1.0 / ct - (r / q) * (z + r);
    double dtau = delta / eta * (1.0 / sigma2_hat - 1.0 / sii);
    const double dv = delta / eta * (mu_hat / sigma2_hat - mui / sii);
    const double tau_prev = tau[i], eps = 2.220446049250313e-16;
    double t = tau_prev + dtau;
    if (t < eps) {
        t = eps;
        dtau = t - tau_prev;
    }
    tau[i] = t;
    v[i] += dv;
    const double ci = dtau / (1.0 + dtau * sii);
    coef[0] = ci;
    coef[1] = ci * (mui + sii * dv) - dv;
}

// Sigma -= ci si si^T and mu -= coef[1] si (expectation_propagation.py:101-105): a streaming read-modify-write of n x ld
// doubles.  A workgroup takes EP_ROWS rows x 512 columns; a lane issues its EP_ROWS 16-byte loads before the first use.
// si is zero in the padding columns, so they keep their value.  ci (si_r si_c) is the same number for (r, c) and (c, r).
__global__ __launch_bounds__(256) void k_ep_rank1(double* __restrict__ S, long ld, long n, const double* __restrict__ si,
                                                  const double* __restrict__ coef, double* __restrict__ mu) {
    const long r0 = (long)blockIdx.y * EP_ROWS;
    if (blockIdx.x == 0 && threadIdx.x < EP_ROWS && r0 + threadIdx.x < n) {
        const long r = r0 + threadIdx.x;
        mu[r] = fma(-coef[1], si[r], mu[r]);
    }
    const double ci = coef[0];
    const long c = ((long)blockIdx.x * 256 + threadIdx.x) * 2;
    if (ci == 0.0 || c >= ld) return;                          // a site whose tau did not move leaves Sigma as it is
    const double2 sc = *reinterpret_cast<const double2*>(si + c);
    double2 x[EP_ROWS];
    double sr[EP_ROWS];
#pragma unroll
    for (int u = 0; u < EP_ROWS; ++u) {
        const long r = r0 + u;
        if (r < n) {
            x[u] = *reinterpret_cast<const double2*>(S + r * ld + c);
            sr[u] = si[r];
        }
    }
#pragma unroll
    for (int u = 0; u < EP_ROWS; ++u) {
        const long r = r0 + u;
        if (r < n) {
            x[u].x = fma(-ci, sr[u] * sc.x, x[u].x);
            x[u].y = fma(-ci, sr[u] * sc.y, x[u].y);
            *reinterpret_cast<double2*>(S + r * ld + c) = x[u];
        }
    }
}

static int check_tau(const double* tau, long n, const char* where) {
    for (long i = 0; i < n; ++i) {
        if (std::isnan(tau[i])) {
            mi355gp_set_error("%s: One or more element(s) of tau is NaN (element %ld)", where, i);
            return -1;
        }
        if (!(tau[i] >= 0.0) || std::isinf(tau[i])) {
            mi355gp_set_error("%s: tau[%ld] = %g is not a finite non-negative number (tau^1/2 is taken)", where, i, tau[i]);
            return -1;
        }
    }
    return 0;
}

extern "C" {

int mi355gp_ep_recompute(mi355gp_ctx* c, const double* tau, const double* v, double extra_jitter, double add_diag, int want_sigma,
                         double* mu_out, double* sigdiag_out, double* logdet_out, double* ms_out) {
    ARG_CHECK(c && c->n > 0 && c->lap && c->lap_stage >= 1, "mi355gp_ep_recompute: call mi355gp_laplace_begin first");
    ARG_CHECK(tau && v && mu_out && sigdiag_out, "mi355gp_ep_recompute: NULL argument");
    const long n = c->n, np = c->npad;
    if (int rc = check_tau(tau, n, "mi355gp_ep_recompute")) return rc;
    if (int rc = lap_check_vec(v, n, "mi355gp_ep_recompute", "v")) return rc;
    ARG_CHECK(std::isfinite(add_diag) && add_diag >= 0.0, "mi355gp_ep_recompute: add_diag must be finite and non-negative");
    HIP_CHECK(hipSetDevice(c->device));
    EngineShared gate(c->device);
    LaplaceSession* L = c->lap;
    hipStream_t st = c->st;
    c->lap_stage = 1;
    HIP_CHECK(hipMemcpyAsync(lvec(c, LV_W), tau, sizeof(double) * n, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(lvec(c, LV_B), v, sizeof(double) * n, hipMemcpyHostToDevice, st));
    L->host.resize((size_t)2 * np + 8);
    const int nt = (int)(np / NB);
    int info = 0;
    for (int attempt = 0;; ++attempt) {
        HIP_CHECK(hipEventRecord(c->ev[0], st));
        lap_enqueue_factor(c, extra_jitter);
        // alpha = v - S^1/2 B^-1 S^1/2 K v, mu = K alpha   (expectation_propagation.py:139-141, zero prior mean)
        launch_symv_lower(st, L->K, np, n, lvec(c, LV_B), nullptr, lvec(c, LV_T0), nullptr, L->part);
        hipLaunchKernelGGL(k_ep_mul, EP_VGRID(n), 0, st, lvec(c, LV_SW), lvec(c, LV_T0), n, lvec(c, LV_T1));
        lap_enqueue_Binv(c, lvec(c, LV_T1), lvec(c, LV_T2));
        hipLaunchKernelGGL(k_ep_sub_scaled, EP_VGRID(n), 0, st, lvec(c, LV_B), lvec(c, LV_SW), lvec(c, LV_T2), n, lvec(c, LV_A));
        launch_symv_lower(st, L->K, np, n, lvec(c, LV_A), nullptr, lvec(c, LV_KA), nullptr, L->part);
        // V = L_B^-1 S^1/2 K into C: the scaled K goes through A (L_B is spent once X exists); its padding rows are cleared
        // so that V's are zero and the product below may run over all npad rows
        launch_rowscale_sqrt(st, L->K, np, n, np, lvec(c, LV_W), c->A);
        if (np > n) HIP_CHECK(hipMemsetAsync(c->A + n * np, 0, sizeof(double) * (np - n) * np, st));
        launch_trmm_lower(st, c->B, np, c->A, np, c->C, np, nt, nt);
        if (want_sigma) {
            // Sigma = K - V^T V (:137), both triangles, into A; add_diag on its diagonal (:319, :326)
            HIP_CHECK(hipMemcpyAsync(c->A, L->K, sizeof(double) * np * np, hipMemcpyDeviceToDevice, st));
            launch_gemm_tn_sq(st, c->C, np, np, c->A, np, nt, -1.0, 1.0);
            hipLaunchKernelGGL(k_ep_diag, EP_VGRID(n), 0, st, c->A, np, n, add_diag, lvec(c, LV_DIAG));
        } else {
            launch_col_reduce_vec(st, c->C, np, n, n, lvec(c, LV_KD), lvec(c, LV_DIAG));
            if (add_diag != 0.0) hipLaunchKernelGGL(k_ep_add_scalar, EP_VGRID(n), 0, st, lvec(c, LV_DIAG), n, add_diag);
        }
        launch_scalars(st, lvec(c, LV_A), lvec(c, LV_A), nullptr, 0, n, 1, L->ws.logsum, L->ws.nblk, lscal(c), nullptr, L->ws.info);
        HIP_CHECK(hipEventRecord(c->ev[1], st));
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
    memcpy(mu_out, L->host.data(), sizeof(double) * n);
    memcpy(sigdiag_out, L->host.data() + np, sizeof(double) * n);
    if (logdet_out) *logdet_out = L->host[(size_t)2 * np + 3];
    if (ms_out) {
        float ms = 0.0f;
        HIP_CHECK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
        *ms_out = ms;
    }
    c->lap_stage = 2;
    L->ep_sigma = want_sigma != 0;
    return 0;
}

int mi355gp_ep_sweep(mi355gp_ctx* c, int lik, const int64_t* order, const double* ysign, double eta, double delta, double* tau,
                     double* v, double* cav_tau_out, double* cav_v_out, double* logZhat_out, double* mu_out, double* sigdiag_out,
                     double* ms_out) {
    ARG_CHECK(c && c->n > 0 && c->lap && c->lap_stage >= 1, "mi355gp_ep_sweep: call mi355gp_laplace_begin first");
    ARG_CHECK(order && ysign && tau && v && cav_tau_out && cav_v_out && logZhat_out && mu_out && sigdiag_out,
              "mi355gp_ep_sweep: NULL argument");
    if (lik != MI355GP_EP_BERNOULLI_PROBIT) {
        mi355gp_set_error("mi355gp_ep_sweep: unknown likelihood %d (moment matching exists for the Bernoulli likelihood with the "
                          "probit link, lik = %d, only)", lik, (int)MI355GP_EP_BERNOULLI_PROBIT);
        return -1;
    }
    LaplaceSession* L = c->lap;
    ARG_CHECK(L->ep_sigma, "mi355gp_ep_sweep: no Sigma is resident: call mi355gp_ep_recompute with want_sigma first (any other "
                           "session call in between overwrites it)");
    const long n = c->n, np = c->npad;
    ARG_CHECK(std::isfinite(eta) && eta > 0.0 && std::isfinite(delta) && delta > 0.0, "mi355gp_ep_sweep: eta and delta must be positive");
    if (int rc = check_tau(tau, n, "mi355gp_ep_sweep")) return rc;
    if (int rc = lap_check_vec(v, n, "mi355gp_ep_sweep", "v")) return rc;
    {
        std::vector<char> seen((size_t)n, 0);
        for (long s = 0; s < n; ++s) {
            if (order[s] < 0 || order[s] >= n || seen[(size_t)order[s]]) {
                mi355gp_set_error("mi355gp_ep_sweep: order is not a permutation of 0 .. N-1 (order[%ld] = %lld)", s, (long long)order[s]);
                return -1;
            }
            seen[(size_t)order[s]] = 1;
        }
        for (long i = 0; i < n; ++i)
            if (ysign[i] != 1.0 && ysign[i] != -1.0) {
                mi355gp_set_error("mi355gp_ep_sweep: ysign[%ld] = %g is neither +1 nor -1", i, ysign[i]);
                return -1;
            }
    }
    HIP_CHECK(hipSetDevice(c->device));
    EngineShared gate(c->device);
    hipStream_t st = c->st;
    double *dTau = lvec(c, LV_W), *dV = lvec(c, LV_B), *dMu = lvec(c, LV_KA), *dRow = lvec(c, LV_T0), *dCt = lvec(c, LV_T1),
           *dCv = lvec(c, LV_T2), *dLz = lvec(c, LV_U), *dYs = lvec(c, LV_S), *coef = lscal(c);
    long long* dOrder = reinterpret_cast<long long*>(lvec(c, LV_A));
    static_assert(sizeof(long long) == sizeof(double) && sizeof(int64_t) == sizeof(long long), "the order travels in a vector slot");
    HIP_CHECK(hipMemcpyAsync(dTau, tau, sizeof(double) * n, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(dV, v, sizeof(double) * n, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(dYs, ysign, sizeof(double) * n, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(dOrder, order, sizeof(int64_t) * n, hipMemcpyHostToDevice, st));
    // a site that the sweep visits leaves its cavity and log Z_hat; all of them are visited (order is a permutation)
    HIP_CHECK(hipEventRecord(c->ev[0], st));
    const dim3 gsite((unsigned)((np + 255) / 256)), gwide((unsigned)((np / 2 + 255) / 256), (unsigned)((n + EP_ROWS - 1) / EP_ROWS));
    for (long s = 0; s < n; ++s) {
        hipLaunchKernelGGL(k_ep_site, gsite, dim3(256), 0, st, c->A, np, n, dOrder, s, dYs, eta, delta, dMu, dTau, dV, dCt, dCv, dLz,
                           dRow, coef);
        hipLaunchKernelGGL(k_ep_rank1, gwide, dim3(256), 0, st, c->A, np, n, dRow, coef, dMu);
    }
    hipLaunchKernelGGL(k_ep_diag, EP_VGRID(n), 0, st, c->A, np, n, 0.0, lvec(c, LV_DIAG));
    HIP_CHECK(hipEventRecord(c->ev[1], st));
    L->host.resize((size_t)7 * np);
    double* h = L->host.data();
    double* src[7] = {dTau, dV, dCt, dCv, dLz, dMu, lvec(c, LV_DIAG)};
    for (int k = 0; k < 7; ++k) HIP_CHECK(hipMemcpyAsync(h + (size_t)k * np, src[k], sizeof(double) * n, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    double* dst[7] = {tau, v, cav_tau_out, cav_v_out, logZhat_out, mu_out, sigdiag_out};
    for (int k = 0; k < 7; ++k) memcpy(dst[k], h + (size_t)k * np, sizeof(double) * n);
    if (ms_out) {
        float ms = 0.0f;
        HIP_CHECK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
        *ms_out = ms;
    }
    return 0;
}

}  // extern "C"
