// dense.hip -- the standalone dense routines on a host matrix (mi355gp_potrf, mi355gp_pdinv, mi355gp_pdinv_full), the
// factorisation benchmark on a synthetic matrix (mi355gp_bench_factor) and that matrix (SyntheticSpd, also used by debug.hip).
#include <vector>

#include "../../include/mi355gp.h"
#include "../../include/mi355gp_debug.h"
#include "internal.h"

int SyntheticSpd::init(hipStream_t st, long N) {
    const int D = 4;
    n = N;
    np = round_up(N, NB);
    std::vector<double> X((size_t)N * D);
    unsigned long long state = 0x9E3779B97F4A7C15ull;
    for (double& v : X) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        v = ((double)(state >> 11) / 9007199254740992.0 - 0.5) * 4.0;
    }
    HIP_CHECK(dX.alloc(N * D));
    HIP_CHECK(dXt.alloc(D * np));
    HIP_CHECK(dIl.alloc(D));
    HIP_CHECK(dNoise.alloc(1));
    const double il[4] = {0.7, 0.7, 0.7, 0.7}, noise = 0.1;
    HIP_CHECK(hipMemcpy(dX, X.data(), sizeof(double) * N * D, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dIl, il, sizeof(il), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dNoise, &noise, sizeof(double), hipMemcpyHostToDevice));
    launch_scale_inputs(st, dX, N, D, dIl, 0, dXt, np);
    return 0;
}

void SyntheticSpd::build(hipStream_t st, double* A) const {
    const KernParams kp{MI355GP_RBF, 0, 4, 1.0};
    launch_kbuild_sym(st, kp, dXt, np, n, np, A, dNoise, 1, 1e-8, 1, 1);
}

static int dense_factor(int device, const double* A_host, int64_t N, bool invert, double* L_out, double* Ainv_out,
                        double* logdet, double* ms, double* Li_out = nullptr) {
    HIP_CHECK(hipSetDevice(device));
    const long np = round_up(N, NB);
    DevBuf A, B, C, tmp;                                      // released on every return path
    WorkspaceGuard<2> guard;                                  // ... and so are the workspace and the two events
    FactorWs& ws = guard.ws;
    HIP_CHECK(A.alloc((size_t)np * np));
    HIP_CHECK(tmp.alloc((size_t)N * N));
    if (invert) {
        HIP_CHECK(B.alloc((size_t)np * np));
        HIP_CHECK(C.alloc((size_t)np * np));
    }
    if (factor_ws_alloc(&ws, np) != 0) return -3;
    ws.scratchX = invert ? (double*)B : nullptr;              // both null without `invert`: trsm128-based panels
    ws.scratchT = invert ? (double*)C : nullptr;
    if (int rc = guard.create_events()) return rc;
    hipEvent_t e0 = guard.ev[0], e1 = guard.ev[1];
    HIP_CHECK(hipMemcpy(tmp, A_host, sizeof(double) * N * N, hipMemcpyHostToDevice));
    {
        const char* et = DIAG_ENV("DENSE_PERSIST_TEST");   // fault injection for the tests (see MI355GP_OPT_PERSIST_TEST)
        if (et && *et) ws.persist_test = atoi(et);
    }
    int info = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        launch_pad_from_dense(0, tmp, N, A, np, nullptr, 0, 0.0);
        HIP_CHECK(hipEventRecord(e0, 0));
        potrf_device(0, A, np, &ws);
        if (invert) {
            trtri_device(0, A, B, C, np, &ws);
            lauum_device(0, B, C, np, &ws);
        }
        HIP_CHECK(hipEventRecord(e1, 0));
        HIP_CHECK(hipMemcpy(&info, ws.info, sizeof(int), hipMemcpyDeviceToHost));
        HIP_CHECK(hipGetLastError());
        bool clean = false;
        if (!potrf_persist_aborted(info, &ws, &clean)) break;  // else: the persistent launch did not run -- redo on launches
        if (attempt == 1) {
            mi355gp_set_error("dense_factor: the factorisation aborted twice (info %d)", info);
            return -6;
        }
    }
    if (ms) {
        float t;
        HIP_CHECK(hipEventElapsedTime(&t, e0, e1));
        *ms = t;
    }
    if (info == 0) {
        auto extract = [&](const double* src, int mode, double* dst) -> int {
            launch_extract(0, src, np, N, mode, nullptr, 0, tmp, 0);
            HIP_CHECK(hipMemcpy(dst, tmp, sizeof(double) * N * N, hipMemcpyDeviceToHost));
            return 0;
        };
        int rc = L_out ? extract(A, 0, L_out) : 0;
        if (!rc && invert && Ainv_out) rc = extract(C, 1, Ainv_out);
        if (!rc && invert && Li_out) rc = extract(B, 0, Li_out);     // L^-1: the dtrtri result pdinv also returns (linalg.py:207)
        if (rc) return rc;
        if (logdet) {
            std::vector<double> ls(ws.nblk);
            HIP_CHECK(hipMemcpy(ls.data(), ws.logsum, sizeof(double) * ws.nblk, hipMemcpyDeviceToHost));
            double s = 0.0;
            for (double v : ls) s += v;
            *logdet = 2.0 * s;
        }
    }
    if (info > N) info = (int)N;
    return info;
}

extern "C" {

int mi355gp_potrf(int device, double* A, int64_t N, double* ms) {
    ARG_CHECK(A && N > 0, "mi355gp_potrf: bad arguments");
    return dense_factor(device, A, N, false, A, nullptr, nullptr, ms);
}

int mi355gp_pdinv(int device, const double* A, int64_t N, double* Ainv, double* L_out, double* logdet, double* ms) {
    ARG_CHECK(A && N > 0, "mi355gp_pdinv: bad arguments");
    return dense_factor(device, A, N, true, L_out, Ainv, logdet, ms);
}

int mi355gp_pdinv_full(int device, const double* A, int64_t N, double* Ainv, double* L_out, double* Li_out, double* logdet,
                       double* ms) {
    ARG_CHECK(A && N > 0, "mi355gp_pdinv_full: bad arguments");
    return dense_factor(device, A, N, true, L_out, Ainv, logdet, ms, Li_out);
}

int mi355gp_bench_factor(int device, int64_t N, int reps, double* ms_potrf, double* ms_trtri, double* ms_lauum) {
    ARG_CHECK(N >= NB && reps >= 1 && ms_potrf && ms_trtri && ms_lauum, "mi355gp_bench_factor: N >= 128, reps >= 1");
    HIP_CHECK(hipSetDevice(device));
    const long np = round_up(N, NB);
    hipStream_t st;
    if (factor_engine(device, &st, nullptr, nullptr) != 0) return -2;
    SyntheticSpd spd;                                          // rebuilt before every repetition
    DevBuf A, B, C;
    WorkspaceGuard<4> guard;
    FactorWs& ws = guard.ws;
    hipEvent_t* e = guard.ev;
    if (int rc = spd.init(st, N)) return rc;
    HIP_CHECK(A.alloc(np * np));
    HIP_CHECK(B.alloc(np * np));
    HIP_CHECK(C.alloc(np * np));
    if (factor_ws_alloc(&ws, np) != 0) return -3;
    ws.scratchX = B;
    ws.scratchT = C;
    if (int rc = guard.create_events()) return rc;
    double acc[3] = {0.0, 0.0, 0.0};
    int info = 0, first_info = 0, redone = 0;
    for (int r = -1; r < reps; ++r) {                          // r = -1: warm-up
        spd.build(st, A);
        HIP_CHECK(hipEventRecord(e[0], st));
        potrf_device(st, A, np, &ws);
        HIP_CHECK(hipEventRecord(e[1], st));
        trtri_device(st, A, B, C, np, &ws);
        HIP_CHECK(hipEventRecord(e[2], st));
        lauum_device(st, B, C, np, &ws);
        HIP_CHECK(hipEventRecord(e[3], st));
        HIP_CHECK(hipStreamSynchronize(st));
        HIP_CHECK(hipMemcpy(&info, ws.info, sizeof(int), hipMemcpyDeviceToHost));
        bool clean = false;
        if (potrf_persist_aborted(info, &ws, &clean)) {         // a called-off / aborted persistent launch factored nothing: the
            if (++redone > reps + 2) {                          // repetition does not count, the context is on launches now
                mi355gp_set_error("mi355gp_bench_factor: the persistent launch kept being called off");
                return -6;
            }
            --r;
            continue;
        }
        if (info > 0 && first_info == 0) first_info = info;
        if (r < 0) continue;
        for (int i = 0; i < 3; ++i) {
            float ms;
            HIP_CHECK(hipEventElapsedTime(&ms, e[i], e[i + 1]));
            acc[i] += ms;
        }
    }
    info = first_info;
    *ms_potrf = acc[0] / reps;
    *ms_trtri = acc[1] / reps;
    *ms_lauum = acc[2] / reps;
    HIP_CHECK(hipGetLastError());
    return info > 0 ? info : 0;
}

}  // extern "C"
