// debug.hip -- the mi355gp_dbg_* probes of include/mi355gp_debug.h, mi355gp_debug_lauum.h and mi355gp_debug_tileops.h: measurements and self-checks for tests and tools, nothing
// an evaluation calls.
#include <vector>

#include "../../include/mi355gp.h"
#include "../../include/mi355gp_debug.h"
#include "../../include/mi355gp_debug_lauum.h"
#include "../../include/mi355gp_debug_tileops.h"
#include "internal.h"
#include "lauum_policy.h"

int run_peaks(int device, double* out4);

extern "C" {

__global__ void k_count_lower_mismatch(const double* __restrict__ a, const double* __restrict__ b, long n, long ld,
                                       unsigned long long* __restrict__ count) {
    unsigned long long c = 0;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < n * n; idx += (long)gridDim.x * blockDim.x) {
        const long i = idx / n, j = idx - i * n;
        if (j <= i && __double_as_longlong(a[i * ld + j]) != __double_as_longlong(b[i * ld + j])) ++c;
    }
    if (c) atomicAdd(count, c);
}

int mi355gp_dbg_persist(int device, int64_t N, int reps, int kcap, double* out) {
    ARG_CHECK(N >= 2 * NB && reps >= 1 && out, "mi355gp_dbg_persist: N >= 256, reps >= 1");
    HIP_CHECK(hipSetDevice(device));
    const long np = round_up(N, NB);
    const int nt = (int)(np / NB);
    hipStream_t st;
    if (factor_engine(device, &st, nullptr, nullptr) != 0) return -2;
    EngineShared gate(device);
    SyntheticSpd spd;
    DevBuf A, B, dStamp, dCount;
    WorkspaceGuard<2> guard;
    FactorWs& ws = guard.ws;
    hipEvent_t* e = guard.ev;
    if (int rc = spd.init(st, N)) return rc;
    HIP_CHECK(A.alloc(np * np));
    HIP_CHECK(B.alloc(np * np));
    HIP_CHECK(dStamp.alloc(32 * nt));
    HIP_CHECK(dCount.alloc(1));
    HIP_CHECK(hipMemset(dStamp, 0, sizeof(double) * 32 * nt));
    HIP_CHECK(hipMemset(dCount, 0, sizeof(double)));
    if (factor_ws_alloc(&ws, np) != 0) return -3;
    ws.tri_overlap = 0;
    if (kcap > 0) ws.persist_kcap = kcap;
    ws.persist_max_nt = 64;
    ws.persist = 1;
    if (int rc = guard.create_events()) return rc;
    for (int i = 0; i < 8 + 32 * nt; ++i) out[i] = 0.0;
    int info[4] = {0, 0, 0, 0};
    for (int mode = 0; mode < 2; ++mode) {                      // 0: launch per step into B, 1: persistent into A
        double* M = mode == 0 ? (double*)B : (double*)A;
        ws.persist = mode;
        if (mode == 1 && !potrf_persist_eligible(np, &ws)) {
            mi355gp_set_error("mi355gp_dbg_persist: N = %ld is not eligible for the persistent factorisation", (long)N);
            return -1;
        }
        double acc = 0.0;
        for (int r = -1; r < reps; ++r) {                       // r = -1: warm-up
            spd.build(st, M);
            HIP_CHECK(hipEventRecord(e[0], st));
            if (mode == 1) launch_potrf_persist(st, M, np, &ws, reinterpret_cast<long long*>((double*)dStamp));
            else potrf_device(st, M, np, &ws);
            HIP_CHECK(hipEventRecord(e[1], st));
            HIP_CHECK(hipStreamSynchronize(st));
            if (r < 0) continue;
            float ms;
            HIP_CHECK(hipEventElapsedTime(&ms, e[0], e[1]));
            acc += ms;
        }
        out[mode] = acc / reps;
        if (mode == 1) {
            int sync[2] = {0, 0};
            HIP_CHECK(hipMemcpy(info, ws.info, sizeof(int) * 4, hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(sync, ws.persist_sync, sizeof(sync), hipMemcpyDeviceToHost));
            out[3] = info[0];
            out[4] = sync[1];
        }
    }
    hipLaunchKernelGGL(k_count_lower_mismatch, dim3(1024), dim3(256), 0, st, (const double*)A, (const double*)B, (long)N, np,
                       reinterpret_cast<unsigned long long*>((double*)dCount));
    unsigned long long cnt = 0;
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipMemcpy(&cnt, dCount, sizeof(cnt), hipMemcpyDeviceToHost));
    out[2] = (double)cnt;
    std::vector<long long> stamps((size_t)32 * nt);
    HIP_CHECK(hipMemcpy(stamps.data(), dStamp, sizeof(long long) * 32 * nt, hipMemcpyDeviceToHost));
    for (int i = 0; i < 32 * nt; ++i) out[8 + i] = (double)stamps[(size_t)i];
    HIP_CHECK(hipGetLastError());
    return 0;
}

// Diagnostic: the same build + factorisation sequence as mi355gp_bench_factor, once launched kernel by kernel and once
// replayed from a hipGraph captured from the same streams (main + look-ahead panel stream; sizes below the overlapped-inverse
// threshold use no CU-masked stream).  out3: ms per repetition launched / replayed, number of graph nodes.
int mi355gp_dbg_graph_factor(int device, int64_t N, int reps, double* out3) {
    ARG_CHECK(N >= NB && reps >= 1 && out3, "mi355gp_dbg_graph_factor: N >= 128, reps >= 1");
    HIP_CHECK(hipSetDevice(device));
    const long np = round_up(N, NB);
    hipStream_t st;
    if (factor_engine(device, &st, nullptr, nullptr) != 0) return -2;
    SyntheticSpd spd;
    DevBuf A, B, C;
    WorkspaceGuard<2> guard;
    FactorWs& ws = guard.ws;
    struct GraphGuard {
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        ~GraphGuard() {
            if (exec) (void)hipGraphExecDestroy(exec);
            if (graph) (void)hipGraphDestroy(graph);
        }
    } gg;
    if (int rc = spd.init(st, N)) return rc;
    HIP_CHECK(A.alloc(np * np));
    HIP_CHECK(B.alloc(np * np));
    HIP_CHECK(C.alloc(np * np));
    if (factor_ws_alloc(&ws, np) != 0) return -3;
    ws.tri_overlap = 0;                                        // no CU-masked side stream inside the captured region
    ws.scratchX = B;
    ws.scratchT = C;
    auto sequence = [&]() {
        spd.build(st, A);
        potrf_device(st, A, np, &ws);
        trtri_device(st, A, B, C, np, &ws);
        lauum_device(st, B, C, np, &ws);
    };
    sequence();                                                // warm-up: one-time function attributes, lazy module load
    HIP_CHECK(hipStreamSynchronize(st));
    if (int rc = guard.create_events()) return rc;
    hipEvent_t e0 = guard.ev[0], e1 = guard.ev[1];
    float ms;
    HIP_CHECK(hipEventRecord(e0, st));
    for (int r = 0; r < reps; ++r) sequence();
    HIP_CHECK(hipEventRecord(e1, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    out3[0] = ms / reps;
    HIP_CHECK(hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
    sequence();
    HIP_CHECK(hipStreamEndCapture(st, &gg.graph));
    size_t nnodes = 0;
    HIP_CHECK(hipGraphGetNodes(gg.graph, nullptr, &nnodes));
    out3[2] = (double)nnodes;
    HIP_CHECK(hipGraphInstantiate(&gg.exec, gg.graph, nullptr, nullptr, 0));
    HIP_CHECK(hipGraphLaunch(gg.exec, st));                    // warm-up replay
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipEventRecord(e0, st));
    for (int r = 0; r < reps; ++r) HIP_CHECK(hipGraphLaunch(gg.exec, st));
    HIP_CHECK(hipEventRecord(e1, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    out3[1] = ms / reps;
    HIP_CHECK(hipGetLastError());
    return 0;
}

int mi355gp_dbg_mfma(int device, const double* a, const double* b, double* d) {
    HIP_CHECK(hipSetDevice(device));
    DevBuf da, db, dd;
    HIP_CHECK(da.alloc(64));
    HIP_CHECK(db.alloc(64));
    HIP_CHECK(dd.alloc(256));
    HIP_CHECK(hipMemcpy(da, a, 64 * 8, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(db, b, 64 * 8, hipMemcpyHostToDevice));
    launch_dbg_mfma(0, da, db, dd);
    HIP_CHECK(hipMemcpy(d, dd, 256 * 8, hipMemcpyDeviceToHost));
    return 0;
}

int mi355gp_dbg_gemm(int device, int a_mcontig, int b_ncontig, int64_t M, int64_t N, int64_t K, const double* A,
                     const double* B, double* C, double alpha, double beta, int reps, double* ms) {
    ARG_CHECK(M % NB == 0 && N % NB == 0 && K % 16 == 0 && M > 0 && N > 0 && K > 0, "dbg_gemm: M,N % 128, K % 16");
    HIP_CHECK(hipSetDevice(device));
    DevBuf dA, dB, dC;
    HIP_CHECK(dA.alloc(M * K));
    HIP_CHECK(dB.alloc(N * K));
    HIP_CHECK(dC.alloc(M * N));
    HIP_CHECK(hipMemcpy(dA, A, sizeof(double) * M * K, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dB, B, sizeof(double) * N * K, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dC, C, sizeof(double) * M * N, hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
    launch_dbg_gemm(0, a_mcontig, b_ncontig, M, N, K, dA, dB, dC, alpha, beta);
    HIP_CHECK(hipMemcpy(C, dC, sizeof(double) * M * N, hipMemcpyDeviceToHost));
    if (reps > 0 && ms) {
        HIP_CHECK(hipEventRecord(e0, 0));
        for (int r = 0; r < reps; ++r) launch_dbg_gemm(0, a_mcontig, b_ncontig, M, N, K, dA, dB, dC, alpha, 0.0);
        HIP_CHECK(hipEventRecord(e1, 0));
        HIP_CHECK(hipEventSynchronize(e1));
        float t;
        HIP_CHECK(hipEventElapsedTime(&t, e0, e1));
        *ms = t / reps;
    }
    HIP_CHECK(hipGetLastError());
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return 0;
}

// Diagnostics: the trailing-update kernel of the blocked Cholesky ALONE on a resident matrix: C (lower triangle of nt x nt
// 128-tiles) -= P P^T with a K-column panel, for each K in ks[0..nk): out_ms[i] = average launch time.  What a deeper panel
// (fewer passes over C) would buy the kernel itself, without any schedule around it.
int mi355gp_dbg_update_nt(int device, int nt, const int* ks, int nk, int reps, double* out_ms) {
    return mi355gp_dbg_update_rect(device, nt, nt, ks, nk, reps, out_ms);
}

// the same for a rectangular region of ntr x ntc tiles below the diagonal (ntc < ntr: "part 1" of a step, the next panel's
// columns; ntc == ntr: the lower triangle)
int mi355gp_dbg_update_rect(int device, int ntr, int ntc, const int* ks, int nk, int reps, double* out_ms) {
    ARG_CHECK(ntr >= 1 && ntc >= 1 && ntc <= ntr && ks && nk >= 1 && reps >= 1 && out_ms, "mi355gp_dbg_update_rect: bad arguments");
    HIP_CHECK(hipSetDevice(device));
    const int nt = ntr;
    const long n = (long)nt * NB;
    long kmax = 0;
    for (int i = 0; i < nk; ++i) {
        ARG_CHECK(ks[i] >= 16 && ks[i] % 16 == 0, "mi355gp_dbg_update_nt: K % 16");
        if (ks[i] > kmax) kmax = ks[i];
    }
    DevBuf C, P;
    HIP_CHECK(C.alloc(n * n));
    HIP_CHECK(P.alloc(n * kmax));
    HIP_CHECK(hipMemset(C, 0, sizeof(double) * n * n));
    HIP_CHECK(hipMemset(P, 0, sizeof(double) * n * kmax));
    hipStream_t st;
    HIP_CHECK(hipStreamCreate(&st));
    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
    for (int i = 0; i < nk; ++i) {
        // rectangular case: rows [ntc, ntr) x columns [0, ntc) -- no tile above the diagonal
        const int r0 = (ntc == ntr) ? 0 : ntc, nr = (ntc == ntr) ? ntr : ntr - ntc;
        launch_update_nt(st, C + (long)r0 * NB * n, n, P + (long)r0 * NB * kmax, kmax, P, kmax, ks[i], nr, ntc, r0, 0);
        HIP_CHECK(hipEventRecord(e0, st));
        for (int r = 0; r < reps; ++r)
            launch_update_nt(st, C + (long)r0 * NB * n, n, P + (long)r0 * NB * kmax, kmax, P, kmax, ks[i], nr, ntc, r0, 0);
        HIP_CHECK(hipEventRecord(e1, st));
        HIP_CHECK(hipEventSynchronize(e1));
        float t;
        HIP_CHECK(hipEventElapsedTime(&t, e0, e1));
        out_ms[i] = t / reps;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipStreamDestroy(st);
    HIP_CHECK(hipGetLastError());
    return 0;
}

int mi355gp_dbg_peaks(int device, double* out4) { return run_peaks(device, out4); }

int mi355gp_dbg_gemm_clock(double* mhz, double* cycles) { return gemm_last_clock(mhz, cycles); }

// Host only: the X^T X work list of gemm.hip for nt x nt tiles (tests/test_host_logic.py checks that it covers every k range once).
int mi355gp_dbg_lauum_plan(int nt, int* items_out, int max_items, int* out4) {
    ARG_CHECK(nt >= 1 && nt <= 4096 && out4 && (items_out || max_items == 0), "mi355gp_dbg_lauum_plan: bad arguments");
    std::vector<LauumItem> items;
    std::vector<LauumSum> sums;
    int nparts = 0;
    lauum_split_plan(nt, items, sums, &nparts);
    int longest = 0;
    for (const LauumItem& it : items) longest = it.klen > longest ? it.klen : longest;
    out4[0] = (int)items.size();
    out4[1] = nparts;
    out4[2] = lauum_split_tile(nt);
    out4[3] = longest;
    if ((int)items.size() > max_items) return -1;
    for (size_t i = 0; i < items.size(); ++i) {
        const LauumItem& it = items[i];
        const int row[6] = {it.ti, it.tj, it.q, it.k0, it.klen, it.part};
        for (int j = 0; j < 6; ++j) items_out[6 * i + j] = row[j];
    }
    return 0;
}

// Host only: the work list of a k_lauum_wide launch for nt x nt tiles (lauum_policy.h; tests/test_lauum_wide_map.py checks that it
// covers every lower block once), and what the policy says for this nt.
int mi355gp_dbg_lauum_wide_map(int nt, int* items_out, int max_items, int* out4) {
    ARG_CHECK(nt >= 1 && nt <= 4096 && out4 && (items_out || max_items == 0), "mi355gp_dbg_lauum_wide_map: bad arguments");
    const long n = lauum_wide_items(nt);
    int nwide = 0;
    for (long b = 0; b < n; ++b) {
        int ti, tj, wide;
        lauum_wide_item(b, ti, tj, wide);
        nwide += wide;
        if (b < max_items) {
            const int row[4] = {ti, tj, wide ? 2 : 1, (nt - ti) * NB};
            for (int j = 0; j < 4; ++j) items_out[4 * b + j] = row[j];
        }
    }
    out4[0] = (int)n;
    out4[1] = lauum_wide_applies(nt, 0) ? 1 : 0;
    out4[2] = LAUUM_WIDE_MIN_NT;
    out4[3] = nwide;
    return n > max_items ? -1 : 0;
}

// lower-triangular test matrix of mi355gp_dbg_lauum when the caller passes none: entries in [-1, 1) from a hash of the index
__global__ void k_dbg_fill_lower(double* __restrict__ X, long n) {
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < n * n; idx += (long)gridDim.x * blockDim.x) {
        const long i = idx / n, j = idx - i * n;
        unsigned long long h = (unsigned long long)idx * 0x9E3779B97F4A7C15ull;
        h ^= h >> 29;
        h *= 0xBF58476D1CE4E5B9ull;
        h ^= h >> 32;
        X[idx] = j <= i ? (double)(h >> 11) * (2.0 / 9007199254740992.0) - 1.0 : 0.0;
    }
}

// Diagnostics: W = X^T X alone.  Variant 0 / 1: ONE whole-K launch on the tile of the caller's choice (0: 128 x 128, k_lauum; 1: 128 x 256,
// k_lauum_wide), whatever the policy would pick for this size, and its time.  Variant 2: what the policy picks -- lauum_device with a
// default workspace (k_lauum64, the split work list, k_lauum, k_lauum_wide by size); W starts as the caller's W, so tiles the
// launchers must not write come back as they went in.
int mi355gp_dbg_lauum(int device, int64_t n, const double* X_host, double* W_host, int variant, int reps, double* ms) {
    ARG_CHECK(n >= NB && n % NB == 0 && n <= 65536 && variant >= 0 && variant <= 2 && reps >= 0 && (reps == 0 || ms),
              "mi355gp_dbg_lauum: n a multiple of 128, variant 0, 1 or 2, reps >= 0");
    HIP_CHECK(hipSetDevice(device));
    const int nt = (int)(n / NB);
    DevBuf X, W;
    WorkspaceGuard<1> guard;
    hipStream_t st = 0;
    if (variant == 2) {
        if (factor_engine(device, &st, nullptr, nullptr) != 0) return -2;
        if (factor_ws_alloc(&guard.ws, n) != 0) return -3;
    }
    HIP_CHECK(X.alloc(n * n));
    HIP_CHECK(W.alloc(n * n));
    if (X_host) HIP_CHECK(hipMemcpy(X, X_host, sizeof(double) * n * n, hipMemcpyHostToDevice));
    else hipLaunchKernelGGL(k_dbg_fill_lower, dim3(4096), dim3(256), 0, 0, (double*)X, (long)n);
    if (variant == 2 && W_host) HIP_CHECK(hipMemcpy(W, W_host, sizeof(double) * n * n, hipMemcpyHostToDevice));
    else HIP_CHECK(hipMemset(W, 0, sizeof(double) * n * n));
    HIP_CHECK(hipDeviceSynchronize());
    auto launch = [&]() {
        if (variant == 2) lauum_device(st, X, W, n, &guard.ws);
        else launch_lauum_variant(st, X, W, n, nt, variant);
    };
    launch();
    HIP_CHECK(hipDeviceSynchronize());
    if (W_host) HIP_CHECK(hipMemcpy(W_host, W, sizeof(double) * n * n, hipMemcpyDeviceToHost));
    if (reps > 0) {
        hipEvent_t e0, e1;
        HIP_CHECK(hipEventCreate(&e0));
        HIP_CHECK(hipEventCreate(&e1));
        HIP_CHECK(hipEventRecord(e0, st));
        for (int r = 0; r < reps; ++r) launch();
        HIP_CHECK(hipEventRecord(e1, st));
        HIP_CHECK(hipEventSynchronize(e1));
        float t;
        HIP_CHECK(hipEventElapsedTime(&t, e0, e1));
        *ms = t / reps;
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
    }
    HIP_CHECK(hipGetLastError());
    return 0;
}

// Diagnostics: ONE launcher of the tile-GEMM family alone on the caller's operands (include/mi355gp_debug_tileops.h), with the
// leading dimensions the product passes.  Out goes to the device before the launch and comes back after it.
int mi355gp_dbg_tileop(int device, int op, const int64_t* dims, const double* X_host, const double* B_host, double* Out_host,
                       double alpha) {
    ARG_CHECK(dims && Out_host && op >= MI355GP_TILEOP_TRMM_LOWER && op <= MI355GP_TILEOP_UPDATE_NT, "mi355gp_dbg_tileop: bad arguments");
    const int64_t lim = 64;                                     // tiles per dimension: a test tool, not a benchmark
    long nx = 0, nb = 0, no = 0;                               // doubles of X, B, Out
    long n = 0, m = 0;
    switch (op) {
        case MI355GP_TILEOP_TRMM_LOWER:
        case MI355GP_TILEOP_TRMM_LOWER_T:
        case MI355GP_TILEOP_TRMM64:
            ARG_CHECK(dims[0] >= 1 && dims[0] <= lim && dims[1] >= 1 && dims[1] <= lim &&
                          (op != MI355GP_TILEOP_TRMM64 || (dims[2] >= 0 && dims[2] <= 3)) && X_host && B_host,
                      "mi355gp_dbg_tileop: trmm needs 1 <= nt, ntc <= 64, mode 0..3, X and B");
            n = dims[0] * NB;
            m = dims[1] * NB;
            nx = n * n;
            nb = no = n * m;
            break;
        case MI355GP_TILEOP_GRAM_SPLITK:
            ARG_CHECK(dims[0] >= 16 && dims[1] >= NB && dims[1] % NB == 0 && dims[1] <= lim * NB && dims[2] >= 1 && dims[2] <= 64 &&
                          dims[0] % (16 * dims[2]) == 0 && dims[0] <= (1 << 20) && X_host,
                      "mi355gp_dbg_tileop: gram_splitk needs rows % (16 S) == 0, mp % 128 == 0, the panel in X");
            n = dims[0];
            m = dims[1];
            nx = n * m;
            no = dims[2] * m * m;
            break;
        default:
            ARG_CHECK(dims[0] >= 16 && dims[0] % NB == 0 && dims[0] <= lim * NB && dims[1] >= 1 && dims[2] >= 1 && dims[3] >= 0 &&
                          dims[4] >= 0 && dims[3] + dims[1] <= lim && dims[4] + dims[2] <= lim,
                      "mi355gp_dbg_tileop: update_nt needs K % 128 == 0 and a region of at most 64 tiles per dimension");
            n = dims[0] + NB * (dims[3] + dims[1] > dims[4] + dims[2] ? dims[3] + dims[1] : dims[4] + dims[2]);
            no = n * n;
            break;
    }
    HIP_CHECK(hipSetDevice(device));
    DevBuf X, B, Out;
    if (nx) {
        HIP_CHECK(X.alloc(nx));
        HIP_CHECK(hipMemcpy(X, X_host, sizeof(double) * nx, hipMemcpyHostToDevice));
    }
    if (nb) {
        HIP_CHECK(B.alloc(nb));
        HIP_CHECK(hipMemcpy(B, B_host, sizeof(double) * nb, hipMemcpyHostToDevice));
    }
    HIP_CHECK(Out.alloc(no));
    HIP_CHECK(hipMemcpy(Out, Out_host, sizeof(double) * no, hipMemcpyHostToDevice));
    const int nt = (int)dims[0], nto = (int)dims[1];
    switch (op) {
        case MI355GP_TILEOP_TRMM_LOWER: launch_trmm_lower(0, X, n, B, m, Out, m, nt, nto); break;
        case MI355GP_TILEOP_TRMM_LOWER_T: launch_trmm_lower_T(0, X, n, B, m, Out, m, nt, nto); break;
        case MI355GP_TILEOP_TRMM64: {
            const long ldb = dims[2] < 2 ? m : n;              // B and Out: n x m for X B / X^T B, m x n for B X^T / B X
            launch_trmm64(0, (int)dims[2], X, n, B, ldb, Out, ldb, nt, nto, alpha);
            break;
        }
        case MI355GP_TILEOP_GRAM_SPLITK: launch_gram_splitk(0, X, m, n, m, (int)dims[2], (int)dims[3], Out); break;
        default: {
            const long K = dims[0], r0 = K + dims[3] * NB, c0 = K + dims[4] * NB;
            double* A = Out;
            launch_update_nt(0, A + r0 * n + c0, n, A + r0 * n, n, A + c0 * n, n, (int)K, (int)dims[1], (int)dims[2], (int)(r0 / NB),
                             (int)(c0 / NB));
            break;
        }
    }
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(Out_host, Out, sizeof(double) * no, hipMemcpyDeviceToHost));
    HIP_CHECK(hipGetLastError());
    return 0;
}

// Diagnostics: is a CU mask in force on a stream created with hipExtStreamCreateWithCUMask?  Times the same 4096^3 GEMM
// on a plain stream and on a stream masked to pct % of every XCD's CUs.  order: 0 = masked stream created first,
// 1 = plain stream first, 2 = four plain + three high-priority streams first (what a context has when it builds its
// factorisation workspace).  out: [ms plain, ms masked, ms masked again after use of both].
int mi355gp_dbg_mask_probe(int device, int pct, int order, double* out3) {
    ARG_CHECK(out3 && pct > 0 && pct <= 100, "mi355gp_dbg_mask_probe: bad arguments");
    HIP_CHECK(hipSetDevice(device));
    const long n = 4096;
    DevBuf A, B, C;
    HIP_CHECK(A.alloc(n * n));
    HIP_CHECK(B.alloc(n * n));
    HIP_CHECK(C.alloc(n * n));
    HIP_CHECK(hipMemset(A, 0, sizeof(double) * n * n));
    HIP_CHECK(hipMemset(B, 0, sizeof(double) * n * n));
    HIP_CHECK(hipMemset(C, 0, sizeof(double) * n * n));
    hipDeviceProp_t prop;
    HIP_CHECK(hipGetDeviceProperties(&prop, device));
    const int ncu = prop.multiProcessorCount, nx = 8, per = ncu / nx, keep = (per * pct + 50) / 100;
    std::vector<uint32_t> mask((size_t)(ncu + 31) / 32, 0u);
    for (int cu = 0; cu < ncu; ++cu)
        if (cu / nx < keep) mask[cu / 32] |= 1u << (cu % 32);
    int least = 0, greatest = 0;
    HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    hipStream_t plain = nullptr, masked = nullptr, extra[7] = {};
    auto mk_masked = [&]() { return hipExtStreamCreateWithCUMask(&masked, (uint32_t)mask.size(), mask.data()); };
    if (order == 0) {
        HIP_CHECK(mk_masked());
        HIP_CHECK(hipStreamCreate(&plain));
    } else {
        HIP_CHECK(hipStreamCreate(&plain));
        if (order == 2) {
            for (int i = 0; i < 4; ++i) HIP_CHECK(hipStreamCreateWithFlags(&extra[i], hipStreamNonBlocking));
            for (int i = 4; i < 7; ++i) HIP_CHECK(hipStreamCreateWithPriority(&extra[i], hipStreamNonBlocking, greatest));
        }
        if (order >= 1) launch_gemm(plain, 0, 1, n, n, n, A, n, B, n, C, n, 1.0, 0.0);   // the plain queue exists and has run
        HIP_CHECK(hipStreamSynchronize(plain));
        HIP_CHECK(mk_masked());
    }
    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
    hipStream_t order_s[3] = {plain, masked, masked};
    for (int i = 0; i < 3; ++i) {
        launch_gemm(order_s[i], 0, 1, n, n, n, A, n, B, n, C, n, 1.0, 0.0);
        HIP_CHECK(hipEventRecord(e0, order_s[i]));
        for (int r = 0; r < 3; ++r) launch_gemm(order_s[i], 0, 1, n, n, n, A, n, B, n, C, n, 1.0, 0.0);
        HIP_CHECK(hipEventRecord(e1, order_s[i]));
        HIP_CHECK(hipStreamSynchronize(order_s[i]));
        float ms = 0.f;
        HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
        out3[i] = ms / 3.0;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipStreamDestroy(plain);
    (void)hipStreamDestroy(masked);
    for (auto x : extra)
        if (x) (void)hipStreamDestroy(x);
    return 0;
}

}  // extern "C"
