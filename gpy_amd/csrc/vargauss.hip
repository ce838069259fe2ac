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
