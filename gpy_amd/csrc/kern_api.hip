// kern_api.hip -- the stateless kernel-function entry points: mi355gp_kern_K, mi355gp_kern_Kdiag,
// mi355gp_update_gradients_full, mi355gp_gradients_X (one part over all D columns of host points, no context).
#include "parts.h"

// The one part of a stateless call over all D columns of X, its inv_ls and pw on the device.  Coregionalize: D = 1, X / X2 are
// the output-index columns themselves (their indices validated here).
struct StatelessPart : DevicePart {
    int load(int kind, int ard, const double* theta, int D, KindSet accepted, const char* where, const double* X, int64_t N,
             const double* X2, int64_t M) {
        const int col0 = 0;
        const mi355gp_part in{kind, ard, kind == MI355GP_COREGIONALIZE ? 1 : 0, &col0, theta, 0};
        if (int rc = parse_part(in, D, accepted, where, this)) return rc;
        if (coreg()) {
            ARG_CHECK(D == 1, "Coregionalize (kind 8): D must be 1 (the output-index column)");
            if (int rc = coreg_check_index(X, N, 1, ard, "X")) return rc;
            if (X2)
                if (int rc = coreg_check_index(X2, M, 1, ard, "X2")) return rc;
        }
        return upload(0);
    }
    // X (n x D, host) uploaded into xs and scaled for this part
    int scaled(PointSet& xs, const double* X, int64_t n) const {
        if (int rc = xs.load(0, X, n, (int)inv_ls.size())) return rc;
        xs.points(0, *this);
        return 0;
    }
};

extern "C" {

int mi355gp_kern_K(int device, int kind, int ard, const double* theta, const double* X, int64_t N,
                   const double* X2, int64_t M, int D, double* K_out) {
    ARG_CHECK(X && K_out && N > 0 && D > 0, "mi355gp_kern_K: bad arguments");
    HIP_CHECK(hipSetDevice(device));
    const bool sym = (X2 == nullptr);
    if (sym) M = N;
    ARG_CHECK(M > 0, "mi355gp_kern_K: M must be positive");
    StatelessPart pt;
    if (int rc = pt.load(kind, ard, theta, D, KS_STATIONARY | KS_EXT | KS_COREG | KS_LINEAR | KS_DOT | KS_OSC, "mi355gp_kern_K", X, N, X2, M)) return rc;
    PointSet x1, x2;
    if (int rc = pt.scaled(x1, X, N)) return rc;
    if (!sym)
        if (int rc = pt.scaled(x2, X2, M)) return rc;
    const PointSet& y = sym ? x1 : x2;
    DevBuf dK;
    HIP_CHECK(dK.alloc(N * M));
    launch_kbuild_cross(0, pt.kp, x1.t, x1.ld, N, y.t, y.ld, M, dK, M);
    HIP_CHECK(hipMemcpy(K_out, dK, sizeof(double) * N * M, hipMemcpyDeviceToHost));
    HIP_CHECK(hipGetLastError());
    return 0;
}

int mi355gp_kern_Kdiag(int kind, const double* theta, int64_t N, double* out) {
    if (kind == MI355GP_LINEAR) {
        mi355gp_set_error("mi355gp_kern_Kdiag: the diagonal of a Linear (kind 9) part depends on the points (sum_q variance_q "
                          "x_q^2, linear.py:84-85) and this entry point takes no X");
        return -1;
    }
    if (kind_in(kind, KS_DOT)) {
        mi355gp_set_error("mi355gp_kern_Kdiag: the diagonal of a %s (kind %d) part depends on the points (%s) and this entry "
                          "point takes no X", kind_name(kind), kind,
                          kind == MI355GP_MLP ? "var (2/pi) asin(p / (p + 1)), mlp.py:61-64" : "var (scale |x|^2 + bias)^order, poly.py:33-34");
        return -1;
    }
    ARG_CHECK(kind_in(kind, KS_STATIONARY | KS_EXT | KS_OSC) && theta && out && N >= 0, "mi355gp_kern_Kdiag: bad arguments");
    // stationary (Cosine, Sinc, ExpQuadCosine included): K(x,x) = variance (stationary.py:170-173); StdPeriodic likewise (standard_periodic.py:105-109)
    for (int64_t i = 0; i < N; ++i) out[i] = theta[0];
    return 0;
}

// Coregionalize: S[a][b] = sum over i with idx_i = a, j with idx2_j = b of dL_dK[i][j] (every element once, no symmetric
// completion); GPy's dL_dK_small is its transpose (coregionalize.py:130-137)
int mi355gp_update_gradients_full(int device, int kind, int ard, const double* theta, const double* dL_dK,
                                  const double* X, int64_t N, const double* X2, int64_t M, int D,
                                  double* dtheta_out) {
    ARG_CHECK(dL_dK && X && dtheta_out && N > 0 && D > 0, "mi355gp_update_gradients_full: bad arguments");
    HIP_CHECK(hipSetDevice(device));
    const bool sym = (X2 == nullptr);
    if (sym) M = N;
    ARG_CHECK(kind != MI355GP_COREGIONALIZE || M > 0, "mi355gp_update_gradients_full: M must be positive");
    StatelessPart pt;
    if (int rc = pt.load(kind, ard, theta, D, KS_STATIONARY | KS_EXT | KS_COREG | KS_LINEAR | KS_DOT | KS_OSC, "mi355gp_update_gradients_full", X, N, X2, M))
        return rc;
    PointSet x1, x2;
    if (int rc = pt.scaled(x1, X, N)) return rc;
    if (!sym)
        if (int rc = pt.scaled(x2, X2, M)) return rc;
    const PointSet& y = sym ? x1 : x2;
    const int groups = (D + 31) / 32, nrec = pt.ext() ? 2 : 1;
    const size_t nsums = std::max((size_t)2 * groups * GP_STRIDE, (size_t)COREG_REC);
    DevBuf dG, dPart, dOut;
    HIP_CHECK(dG.alloc(N * M));
    // (RatQuad / StdPeriodic: two records per block and group)
    HIP_CHECK(dPart.alloc(std::max((size_t)2 * groups * 2048 * GP_STRIDE, (size_t)2048 * COREG_REC)));
    HIP_CHECK(dOut.alloc(nsums));
    HIP_CHECK(hipMemcpy(dG, dL_dK, sizeof(double) * N * M, hipMemcpyHostToDevice));
    if (pt.coreg()) {
        const int nb = launch_grad_coreg(0, false, pt.kp, x1.t, x1.ld, N, y.t, y.ld, M, dG, M, nullptr, 0, dPart);
        launch_reduce_partials(0, dPart, nb, ard * ard, dOut);
    } else {
        const int nb = grad_generic_num_blocks(N, M);
        launch_grad_generic(0, pt.kp, x1.t, x1.ld, N, y.t, y.ld, M, sym ? 1 : 0, dG, M, dPart);
        for (int r = 0; r < nrec; ++r)
            for (int g = 0; g < (pt.kp.ard ? groups : 1); ++g)
                launch_reduce_partials(0, dPart + ((long)r * groups + g) * nb * GP_STRIDE, nb, GP_STRIDE,
                                       dOut + ((long)r * groups + g) * GP_STRIDE);
    }
    std::vector<double> sums(nsums, 0.0);
    HIP_CHECK(hipMemcpy(sums.data(), dOut, sizeof(double) * (pt.coreg() ? ard * ard : nrec * groups * GP_STRIDE),
                        hipMemcpyDeviceToHost));
    HIP_CHECK(hipGetLastError());
    part_dtheta(pt, sums.data(), sums.data() + (size_t)groups * GP_STRIDE, dtheta_out);
    return 0;
}

// dL/dX from dL_dK: Stationary.gradients_X (kern/src/stationary.py:245-252,330-358; C kernel stationary_utils.c).
//   out[i][q] = sum_j T[i][j] (x_iq - x2_jq) / l_q^2,  T = dL_dK * dK/dr / r  (X2 == NULL: T + T^T against X itself)
// Runs as the column reduction H^T [X2~ | 1] of the transposed problem (the same kernels as the sparse path's dL/dZ);
// StdPeriodic.gradients_X (standard_periodic.py:574-580) as a row reduction of W = dL_dK (+ dL_dK^T against X itself).
int mi355gp_gradients_X(int device, int kind, int ard, const double* theta, const double* dL_dK, const double* X,
                        int64_t N, const double* X2, int64_t M, int D, double* out) {
    ARG_CHECK(dL_dK && X && out && N > 0 && D > 0, "mi355gp_gradients_X: bad arguments");
    HIP_CHECK(hipSetDevice(device));
    if (kind == MI355GP_POLY) {
        mi355gp_set_error("mi355gp_gradients_X: Poly (kind 11) has no gradients_X (the reference raises NotImplementedError, poly.py:45-46)");
        return -1;
    }
    StatelessPart pt;
    if (int rc = pt.load(kind, ard, theta, D, KS_STATIONARY | KS_EXT | KS_LINEAR | 1u << MI355GP_MLP | KS_OSC, "mi355gp_gradients_X", nullptr, 0, nullptr, 0)) return rc;
    const bool sym = (X2 == nullptr);
    if (sym) { M = N; X2 = X; }
    ARG_CHECK(M > 0, "mi355gp_gradients_X: M must be positive");
    PointSet xc, xr;                                         // X and X2
    if (int rc = pt.scaled(xc, X, N)) return rc;
    if (int rc = pt.scaled(xr, X2, M)) return rc;
    // the weights on the device: W (N x M) for StdPeriodic, transposed (M x N: rows = X2 points, columns = X points) otherwise
    const bool periodic = kind == MI355GP_STDPERIODIC;
    std::vector<double> G((size_t)N * M), HX((size_t)N * (D + 1));
    for (int64_t i = 0; i < N; ++i)
        for (int64_t j = 0; j < M; ++j)
            G[periodic ? (size_t)i * M + j : (size_t)j * N + i] = sym ? dL_dK[i * M + j] + dL_dK[j * M + i] : dL_dK[i * M + j];
    DevBuf dG, dPart, dCol, dHX;
    HIP_CHECK(dG.alloc(M * N));
    HIP_CHECK(dHX.alloc(N * (D + 1)));
    if (!periodic) {
        HIP_CHECK(dPart.alloc(2 * 2048 * GP_STRIDE * ((D + 31) / 32)));   // every group, and the second records of RatQuad
        HIP_CHECK(dCol.alloc(64 * N * (D + 1)));
    }
    HIP_CHECK(hipMemcpy(dG, G.data(), sizeof(double) * M * N, hipMemcpyHostToDevice));
    const GradXScratch scratch{dG, N, dPart, dCol, dHX, HX.data(), /*wt=*/0};           // H in place
    if (int rc = part_gradients_X(0, pt, dG, periodic ? M : N, xr.t, xr.ld, M, xc.t, xc.ld, N, X, D, scratch,
                                  [&](long i, int q, double g) { out[i * D + q] = g; }))
        return rc;
    HIP_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
