// predict.hip -- what a context answers after a successful evaluation, from the resident L^-1 and alpha: mi355gp_predict[_sum],
// mi355gp_predictive_gradients_sum, mi355gp_covariance_between_points.
#include "ctx.h"

extern "C" {

// G[i][j] = v[i * stride] for i < n, j < m (row-constant weights: dL_dK of the mean part of predictive_gradients)
__global__ void k_fill_rows(double* __restrict__ G, long ld, long n, long m, const double* __restrict__ v, int stride) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * m) return;
    const long i = idx / m, j = idx - i * m;
    G[i * ld + j] = v[i * stride];
}

int mi355gp_predict_sum(mi355gp_ctx* c, int nparts, const mi355gp_part* parts, const double* Xnew, int64_t M,
                        double* mu_out, double* var_out, int full_cov) {
    ARG_CHECK(c && c->n > 0 && c->have_factor && c->lap_stage == 0, "mi355gp_predict: run an inference call first");
    ARG_CHECK(Xnew && M > 0 && mu_out, "mi355gp_predict: bad arguments");
    HIP_CHECK(hipSetDevice(c->device));
    EngineShared gate(c->device);
    if (int rc = ctx_prepare_parts(c, nparts, parts)) return rc;
    if (int rc = ctx_coreg_check_points(c, Xnew, M, "prediction")) return rc;
    hipStream_t st = c->st;
    const long n = c->n, np = c->npad, mp = round_up(M, NB);
    // (re)scale the training inputs for these parameters (normally identical to the inference call's)
    c->have_kernel = true;
    ctx_scale_parts(c);
    PointSet xs;
    DevBuf dKx, dTmp, dMu, dVar;
    if (int rc = xs.load(st, Xnew, M, c->D)) return rc;
    HIP_CHECK(dKx.alloc(np * mp));
    HIP_CHECK(dTmp.alloc(np * mp));
    HIP_CHECK(dMu.alloc(M * c->Dy));
    HIP_CHECK(dVar.alloc((full_cov ? mp * mp : M)));
    HIP_CHECK(hipMemsetAsync(dKx, 0, sizeof(double) * np * mp, st));
    if (full_cov && var_out) HIP_CHECK(hipMemsetAsync(dVar, 0, sizeof(double) * mp * mp, st));
    const double kdiag = expression_kdiag(c->parts, c->terms);                   // Kdiag(X*): sum over terms of the product of variances
    DevBuf dKd;                                                 // ... or per point, with Coregionalize / Linear parts
    const bool kd_points = ctx_has_point_diag(c) && !full_cov && var_out;
    std::vector<double> kd;
    if (kd_points) {
        kd = ctx_kdiag_points(c, Xnew, M);
        HIP_CHECK(dKd.alloc(M));
        HIP_CHECK(hipMemcpyAsync(dKd, kd.data(), sizeof(double) * M, hipMemcpyHostToDevice, st));
    }
    DevBuf dScr1, dScr2;
    if (has_product(c->terms)) {
        HIP_CHECK(dScr1.alloc(np * mp));
        if (full_cov && var_out) HIP_CHECK(dScr2.alloc(mp * mp));
    }
    emit_cross(st, c->parts, c->terms, ctx_training_points(c), xs, dKx, mp, dScr1, true, 0);                // K(X, X*) (n x M)
    if (full_cov && var_out) emit_cross(st, c->parts, c->terms, xs, xs, dVar, mp, dScr2, true, /*diag_same=*/1);  // K(X*, X*)
    launch_col_reduce(st, dKx, mp, n, M, c->dAlpha, c->Dy, 0.0, 0, dMu);                  // mu = Kx^T alpha
    launch_trmm_lower(st, c->B, np, dKx, mp, dTmp, mp, (int)(np / NB), (int)(mp / NB));   // tmp = L^-1 Kx
    if (!full_cov) {
        if (var_out && kd_points) launch_col_reduce_vec(st, dTmp, mp, n, M, dKd, dVar);
        else if (var_out) launch_col_reduce(st, dTmp, mp, n, M, nullptr, 1, kdiag, 1, dVar);
    } else if (var_out) {
        launch_gemm_tn_sq(st, dTmp, mp, np, dVar, mp, (int)(mp / NB), -1.0, 1.0);         // - tmp^T tmp
    }
    HIP_CHECK(hipMemcpyAsync(mu_out, dMu, sizeof(double) * M * c->Dy, hipMemcpyDeviceToHost, st));
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

// GP.predictive_gradients (core/gp.py:418-474) for a sum of stationary (+ White / Bias) parts, everything N-sized on device:
//   dmu[m][q][d]  = sum_n alpha[n][d] dK(x*_m, x_n)/dx*_mq                         (kern.gradients_X(alpha_d^T, X*, X), :448-451)
//   dvar[m][q]    = dKdiag/dx* (= 0 for stationary kinds, stationary.py:360-361; 2 variance_q x*_mq for Linear; mlp.py:133-147 for MLP) - 2 sum_n (Ky^-1 K(X, X*))[n][m] dK(x*_m, x_n)/dx*_mq   (:454,462-465)
// with Ky^-1 K(X, X*) = X^T (X Kx), X = L^-1 resident from the inference call.  The reductions over n run as the column
// reductions H^T [x~ | 1] of the sparse path's dL/dZ (H = weights * (dK/dr)/r, k_grad + k_colreduce_multi), per part.
int mi355gp_predictive_gradients_sum(mi355gp_ctx* c, int nparts, const mi355gp_part* parts, const double* Xnew, int64_t M,
                                     double* dmu_out, double* dvar_out) {
    ARG_CHECK(c && c->n > 0 && c->have_factor, "mi355gp_predictive_gradients: run an inference call first");
    ARG_CHECK(Xnew && M > 0 && (dmu_out || dvar_out), "mi355gp_predictive_gradients: bad arguments");
    HIP_CHECK(hipSetDevice(c->device));
    EngineShared gate(c->device);
    if (int rc = ctx_prepare_parts(c, nparts, parts)) return rc;
    ARG_CHECK(!has_product(c->terms), "mi355gp_predictive_gradients: product kernels are not supported on the device");
    for (const auto& p : c->parts)
        ARG_CHECK(!p.coreg(), "mi355gp_predictive_gradients: Coregionalize (kind 8) parts are not supported on the device");
    for (const auto& p : c->parts)
        ARG_CHECK(!p.poly(), "mi355gp_predictive_gradients: Poly (kind 11) has no gradients_X (poly.py:45-49)");
    hipStream_t st = c->st;
    const long n = c->n, np = c->npad, D = c->D, Dy = c->Dy, mp = round_up(M, NB);
    c->have_kernel = true;
    ctx_scale_parts(c);
    PointSet xs;
    DevBuf dU, dT, dG, dH, dPart, dCol, dHX;
    if (int rc = xs.load(st, Xnew, M, c->D)) return rc;
    HIP_CHECK(dU.alloc(np * mp));
    HIP_CHECK(dT.alloc(np * mp));
    HIP_CHECK(dG.alloc(np * mp));
    HIP_CHECK(dH.alloc(np * mp));
    HIP_CHECK(dPart.alloc(2 * 2048 * GP_STRIDE * ((D + 31) / 32)));   // second records of RatQuad parts
    HIP_CHECK(dCol.alloc(64 * mp * (D + 1)));
    HIP_CHECK(dHX.alloc(mp * (D + 1)));
    if (dvar_out) {     // U = Ky^-1 K(X, X*)
        HIP_CHECK(hipMemsetAsync(dU, 0, sizeof(double) * np * mp, st));
        emit_cross(st, c->parts, c->terms, ctx_training_points(c), xs, dU, mp, nullptr, true, 0);
        launch_trmm_lower(st, c->B, np, dU, mp, dT, mp, (int)(np / NB), (int)(mp / NB));
        launch_trmm_lower_T(st, c->B, np, dT, mp, dU, mp, (int)(np / NB), (int)(mp / NB));
    }
    // one pass per weight matrix (Dy mean parts, one variance part) and stationary part
    std::vector<double> HX((size_t)M * (D + 1));
    const GradXScratch scratch{dH, mp, dPart, dCol, dHX, HX.data(), /*wt=*/1};
    const int npass = (dmu_out ? (int)Dy : 0) + (dvar_out ? 1 : 0);
    if (dmu_out) std::fill(dmu_out, dmu_out + (size_t)M * D * Dy, 0.0);
    if (dvar_out) std::fill(dvar_out, dvar_out + (size_t)M * D, 0.0);
    for (int pass = 0; pass < npass; ++pass) {
        const bool is_var = dvar_out && pass == npass - 1;
        const double* W = dU;
        if (!is_var) {
            const long cnt = n * M;
            hipLaunchKernelGGL(k_fill_rows, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, (double*)dG, mp, n, (long)M,
                               c->dAlpha + pass, (int)Dy);
            W = dG;
        }
        auto add = [&](long m, int q, double g) {
            if (is_var) dvar_out[m * D + q] += -2.0 * g;
            else dmu_out[((size_t)m * D + q) * Dy + pass] += g;
        };
        for (size_t pi = 0; pi < c->parts.size(); ++pi) {
            const mi355gp_ctx::Part& pt = c->parts[pi];
            if (pt.is_static()) continue;                                        // White / Bias: no dependence on X* (static.py)
            const double* xt = pt.linear() ? nullptr : xs.points(st, pt);         // (Linear reads the training side only)
            if (int rc = part_gradients_X(st, pt, W, mp, pt.dXt, np, n, xt, xs.ld, M, Xnew, (int)D, scratch, add)) return rc;
            if (is_var && pt.linear())                                           // dKdiag/dx*_mq = 2 variance_q x*_mq
                for (long m = 0; m < M; ++m)
                    for (size_t a = 0; a < pt.dims.size(); ++a)
                        dvar_out[m * D + pt.dims[a]] += 2.0 * pt.theta[pt.kp.ard ? a : 0] * Xnew[m * D + pt.dims[a]];
            if (is_var && pt.mlp())                                              // dKdiag/dx*_mq = 2 cd_m w_q x*_mq (mlp.py:133-147)
                for (long m = 0; m < M; ++m) {
                    const double cd = mlp_dkdiag_factor(pt, Xnew + m * D);
                    for (size_t a = 0; a < pt.dims.size(); ++a)
                        dvar_out[m * D + pt.dims[a]] += 2.0 * cd * pt.theta[1 + (pt.kp.ard ? a : 0)] * Xnew[m * D + pt.dims[a]];
                }
        }
    }
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    return 0;
}

// Posterior covariance between two point sets (Posterior.covariance_between_points, posterior.py:109-130):
//   K(X1, X2) - (L^-1 K(X, X1))^T (L^-1 K(X, X2)),  out: M1 x M2 row-major
int mi355gp_covariance_between_points(mi355gp_ctx* c, int nparts, const mi355gp_part* parts, const double* X1,
                                      int64_t M1, const double* X2, int64_t M2, double* out) {
    ARG_CHECK(c && c->n > 0 && c->have_factor, "mi355gp_covariance_between_points: run an inference call first");
    ARG_CHECK(X1 && X2 && M1 > 0 && M2 > 0 && out, "mi355gp_covariance_between_points: bad arguments");
    HIP_CHECK(hipSetDevice(c->device));
    EngineShared gate(c->device);
    if (int rc = ctx_prepare_parts(c, nparts, parts)) return rc;
    if (int rc = ctx_coreg_check_points(c, X1, M1, "X1")) return rc;
    if (int rc = ctx_coreg_check_points(c, X2, M2, "X2")) return rc;
    hipStream_t st = c->st;
    const long np = c->npad, m1p = round_up(M1, NB), m2p = round_up(M2, NB);
    c->have_kernel = true;
    ctx_scale_parts(c);
    PointSet x1, x2;
    DevBuf dK1, dK2, dT1, dT2, dC;
    if (int rc = x1.load(st, X1, M1, c->D)) return rc;
    if (int rc = x2.load(st, X2, M2, c->D)) return rc;
    HIP_CHECK(dK1.alloc(np * m1p));
    HIP_CHECK(dK2.alloc(np * m2p));
    HIP_CHECK(dT1.alloc(np * m1p));
    HIP_CHECK(dT2.alloc(np * m2p));
    HIP_CHECK(dC.alloc(m1p * m2p));
    HIP_CHECK(hipMemsetAsync(dK1, 0, sizeof(double) * np * m1p, st));
    HIP_CHECK(hipMemsetAsync(dK2, 0, sizeof(double) * np * m2p, st));
    HIP_CHECK(hipMemsetAsync(dC, 0, sizeof(double) * m1p * m2p, st));
    DevBuf dS1, dS2, dS3;
    if (has_product(c->terms)) {
        HIP_CHECK(dS1.alloc(np * m1p));
        HIP_CHECK(dS2.alloc(np * m2p));
        HIP_CHECK(dS3.alloc(m1p * m2p));
    }
    emit_cross(st, c->parts, c->terms, ctx_training_points(c), x1, dK1, m1p, dS1, true, 0);
    emit_cross(st, c->parts, c->terms, ctx_training_points(c), x2, dK2, m2p, dS2, true, 0);
    emit_cross(st, c->parts, c->terms, x1, x2, dC, m2p, dS3, true, 0);
    launch_trmm_lower(st, c->B, np, dK1, m1p, dT1, m1p, (int)(np / NB), (int)(m1p / NB));
    launch_trmm_lower(st, c->B, np, dK2, m2p, dT2, m2p, (int)(np / NB), (int)(m2p / NB));
    launch_gemm(st, 1, 1, m1p, m2p, np, dT1, m1p, dT2, m2p, dC, m2p, -1.0, 1.0);
    HIP_CHECK(hipMemcpy2DAsync(out, sizeof(double) * M2, dC, sizeof(double) * m2p, sizeof(double) * M2, M1,
                               hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    return 0;
}

int mi355gp_predict(mi355gp_ctx* c, int kind, int ard, const double* theta, const double* Xnew, int64_t M,
                    double* mu_out, double* var_out, int full_cov) {
    if (int rc = check_kind(kind, KS_STATIONARY | KS_EXT | KS_LINEAR | KS_DOT | KS_OSC, "mi355gp_predict")) return rc;
    const mi355gp_part part{kind, ard, 0, nullptr, theta};
    return mi355gp_predict_sum(c, 1, &part, Xnew, M, mu_out, var_out, full_cov);
}

}  // extern "C"
