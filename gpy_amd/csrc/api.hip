// api.hip -- the extern "C" boundary of libmi355gp.so (declared in include/mi355gp.h) and the
// orchestration of one exact-GP objective+gradient evaluation with everything N x N resident in HBM.
#include <functional>
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mi355gp.h"
#include "../../include/mi355gp_debug.h"
#include "internal.h"
#include "parts.h"

int run_peaks(int device, double* out4);

static thread_local std::string g_err;

void mi355gp_set_error(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
}

#define LOG_2_PI 1.8378770664093454836

#include "ctx.h"

// (re)applies the context's option overrides to its factorisation workspace (after every factor_ws_alloc and set_option)
static void apply_options(mi355gp_ctx* c) {
    FactorWs& w = c->ws;
    auto set = [&](int o, int* field) { if (c->opt[o] != INT_MIN) *field = c->opt[o]; };
    set(MI355GP_OPT_LOOKAHEAD, &w.lookahead);
    set(MI355GP_OPT_TRI_OVERLAP, &w.tri_overlap);
    set(MI355GP_OPT_TRI_MIN_NT, &w.tri_min_nt);
    set(MI355GP_OPT_TRI_H, &w.tri_h_override);
    set(MI355GP_OPT_TRI_WGS, &w.tri_wgs);
    set(MI355GP_OPT_TRI_HALF, &w.tri_half_ok);
    set(MI355GP_OPT_PART1_ON_PANEL, &w.part1_on_panel);
    set(MI355GP_OPT_NBO, &w.nbo_override);
    set(MI355GP_OPT_SOLVE_OVERLAP, &w.solve_overlap);
    set(MI355GP_OPT_DIAG_EXCL_FIRST, &w.diag_excl_first);
    set(MI355GP_OPT_PERSIST, &w.persist);
    set(MI355GP_OPT_AGG2, &w.agg2);
    if (c->opt[MI355GP_OPT_GRAPH] != INT_MIN) c->graph_enabled = c->opt[MI355GP_OPT_GRAPH] ? 1 : 0;
}

static void drop_graph(mi355gp_ctx* c) {
    if (c->fgraph) (void)hipGraphExecDestroy(c->fgraph);
    c->fgraph = nullptr;
    c->fgraph_calls = 0;
}

static void free_data(mi355gp_ctx* c) {
    drop_graph(c);                                            // every node holds pointers into the buffers freed below
    c->parts.clear();
    double** ptrs[] = {&c->dX, &c->dR, &c->dNoise, &c->A, &c->B, &c->C, &c->Mbuf,
                       &c->dTmp, &c->dTrmvPart, &c->dGradPart, &c->dGradOut, &c->dPack, &c->dCoregPart};
    for (auto p : ptrs) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
    if (c->hPack) (void)hipHostFree(c->hPack);
    c->hPack = nullptr;
    c->dAlpha = c->dScal = c->dDiag = c->dGradOutAll = nullptr;      // views into dPack
    c->hIdx.clear();
    c->hIdxCol = -1;
    laplace_session_free(c->lap);                             // the fourth N x N buffer and its vectors, if a session ever began
    c->lap = nullptr;
    c->lap_stage = 0;
    factor_ws_free(&c->ws);
    c->have_factor = c->have_kernel = false;
}

extern "C" {

const char* mi355gp_last_error(void) { return g_err.c_str(); }
const char* mi355gp_version(void) { return "mi355gp 0.1 (gfx950)"; }

int mi355gp_device_synchronize(int device) {
    HIP_CHECK(hipSetDevice(device));
    HIP_CHECK(hipDeviceSynchronize());
    return 0;
}

int mi355gp_device_count(int* count) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        n = 0;
    }
    *count = n;
    return 0;
}

int mi355gp_create(int device, mi355gp_ctx** out) {
    int n = 0;
    mi355gp_device_count(&n);
    if (device < 0 || device >= n) {
        mi355gp_set_error("mi355gp_create: device %d not available (%d HIP devices visible)", device, n);
        return -2;
    }
    HIP_CHECK(hipSetDevice(device));
    mi355gp_ctx* c = new mi355gp_ctx();
    c->device = device;
    for (int& o : c->opt) o = INT_MIN;
    if (factor_engine(device, &c->st, nullptr, nullptr) != 0) return -2;    // the device's shared main stream (factor.hip)
    for (auto& e : c->ev) HIP_CHECK(hipEventCreate(&e));
    {
        const char* e = PRODUCT_ENV("GRAPH");
        if (e && *e) c->graph_enabled = atoi(e) ? 1 : 0;
    }
    *out = c;
    return 0;
}

int mi355gp_destroy(mi355gp_ctx* c) {
    if (!c) return 0;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->st);
    free_data(c);
    for (auto& e : c->ev)
        if (e) (void)hipEventDestroy(e);
    if (c->st) (void)hipStreamSynchronize(c->st);                         // shared stream: never destroyed by a context
    delete c;
    return 0;
}

int mi355gp_set_data(mi355gp_ctx* c, const double* X, int64_t N, int D, const double* R, int Dy) {
    ARG_CHECK(c && X && R && N > 0 && D > 0 && Dy > 0, "mi355gp_set_data: bad arguments");
    HIP_CHECK(hipSetDevice(c->device));
    EngineShared gate(c->device);
    HIP_CHECK(hipStreamSynchronize(c->st));
    free_data(c);
    c->n = N;
    c->npad = round_up(N, NB);
    c->D = D;
    c->Dy = Dy;
    const long np = c->npad;
    HIP_CHECK(hipMalloc(&c->dX, sizeof(double) * N * D));
    HIP_CHECK(hipMalloc(&c->dR, sizeof(double) * N * Dy));
    HIP_CHECK(hipMalloc(&c->dNoise, sizeof(double) * N));
    HIP_CHECK(hipMalloc(&c->A, sizeof(double) * np * np));
    HIP_CHECK(hipMalloc(&c->B, sizeof(double) * np * np));
    HIP_CHECK(hipMalloc(&c->C, sizeof(double) * np * np));
    if (factor_ws_alloc(&c->ws, np) != 0) return -3;
    c->ws.can_calibrate = 1;
    {
        const int lookahead = c->ws.lookahead;
        const char* e = PRODUCT_ENV("GRAPH");
        c->graph_enabled = (e && *e) ? (atoi(e) ? 1 : 0) : 1;
        apply_options(c);
        if (c->opt[MI355GP_OPT_LOOKAHEAD] == INT_MIN) c->ws.lookahead = lookahead;
    }
    HIP_CHECK(hipMalloc(&c->dTmp, sizeof(double) * N * Dy));
    const long nchunks = (N + trmv_chunk_rows(N) - 1) / trmv_chunk_rows(N);
    HIP_CHECK(hipMalloc(&c->dTrmvPart, sizeof(double) * nchunks * N * Dy));
    const int groups = (D + 31) / 32;
    c->gradPartDoubles = 2L * groups * 2048 * GP_STRIDE;       // two records per block for RatQuad / StdPeriodic
    HIP_CHECK(hipMalloc(&c->dGradPart, sizeof(double) * c->gradPartDoubles));
    HIP_CHECK(hipMalloc(&c->dGradOut, sizeof(double) * groups * GP_STRIDE));
    c->offGrad = 8;
    c->offExt = c->offGrad + (size_t)16 * groups * GP_STRIDE;
    c->offAlpha = c->offExt + (size_t)16 * groups * GP_STRIDE;
    c->offDiag = c->offAlpha + (size_t)N * Dy;
    c->offCoreg = c->offDiag + (size_t)N;
    c->packDoubles = c->offCoreg + (size_t)16 * COREG_REC;
    HIP_CHECK(hipMalloc(&c->dPack, sizeof(double) * c->packDoubles));
    HIP_CHECK(hipHostMalloc(&c->hPack, sizeof(double) * c->packDoubles, hipHostMallocDefault));
    c->dScal = c->dPack;
    c->dGradOutAll = c->dPack + c->offGrad;
    c->dAlpha = c->dPack + c->offAlpha;
    c->dDiag = c->dPack + c->offDiag;
    HIP_CHECK(hipMemcpy(c->dX, X, sizeof(double) * N * D, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(c->dR, R, sizeof(double) * N * Dy, hipMemcpyHostToDevice));
    return 0;
}

int mi355gp_set_targets(mi355gp_ctx* c, const double* R, int Dy) {
    ARG_CHECK(c && R && c->n > 0 && Dy == c->Dy, "mi355gp_set_targets: set_data first / Dy mismatch");
    HIP_CHECK(hipSetDevice(c->device));
    EngineShared gate(c->device);
    HIP_CHECK(hipStreamSynchronize(c->st));
    HIP_CHECK(hipMemcpy(c->dR, R, sizeof(double) * c->n * Dy, hipMemcpyHostToDevice));
    return 0;
}

}  // extern "C"

// Shared tail: given Ky (lower) in c->A: factor, invert, alpha, scalars [, kernel gradients].
// rebuild(): re-enqueues the construction of Ky in c->A (needed only after a DIRTY abort of the persistent factorisation).
static int run_pipeline(mi355gp_ctx* c, EngineShared* gate, bool with_kernel_grads, double* out_scalars, double* alpha_out,
                        double* dtheta_out, double* diag_out, double* stage_ms,
                        const std::function<int()>& rebuild, double studentt_nu = 0.0, int attempt = 0) {
    hipStream_t st = c->st;
    const long n = c->n, np = c->npad;
    c->lap_stage = 0;                                        // A / B / C are this evaluation's from here on
    c->ws.prof.reset();
    c->ws.scratchX = c->B;                                   // free until trtri / lauum overwrite them
    c->ws.scratchT = c->C;
    // The factorisation region: potrf -> trtri -> (alpha solve on the side stream) || lauum.  `timing`: record the stage events.
    auto region = [&](bool timing) -> int {
        if (timing) HIP_CHECK(hipEventRecord(c->ev[1], st));
        potrf_device(st, c->A, np, &c->ws);
        if (timing) HIP_CHECK(hipEventRecord(c->ev[2], st));
        trtri_device(st, c->A, c->B, c->C, np, &c->ws);
        HIP_CHECK(hipEventRecord(c->ev[3], st));
        // alpha = X^T (X R) only needs X: the two bandwidth-bound triangular mat-vecs run on the side stream underneath the
        // compute-bound W = X^T X instead of after it
        hipStream_t side = (c->ws.st_tri && c->ws.solve_overlap) ? c->ws.st_tri : nullptr;
        if (side) {
            HIP_CHECK(hipStreamWaitEvent(side, c->ev[3], 0));
            launch_tri_matvec(side, c->B, np, n, c->dR, c->Dy, c->dTmp, c->dAlpha, c->dTrmvPart);
            HIP_CHECK(hipEventRecord(c->ws.ev_tri, side));
        }
        lauum_device(st, c->B, c->C, np, &c->ws);
        if (timing) HIP_CHECK(hipEventRecord(c->ev[4], st));
        if (side) HIP_CHECK(hipStreamWaitEvent(st, c->ws.ev_tri, 0));
        else launch_tri_matvec(st, c->B, np, n, c->dR, c->Dy, c->dTmp, c->dAlpha, c->dTrmvPart);
        return 0;
    };
    // hipGraph replay when nothing in the region needs a CU-masked stream (sizes below the overlapped-inverse threshold), no
    // stage timing was asked for and launch bracketing is off; the first evaluation of a context runs plain (one-time
    // function attributes), the second captures, every later one replays.
    const bool structural = c->graph_enabled && !c->ws.prof.on && c->ws.lookahead == 1 && c->ws.persist_skip == 0 &&
                            (!c->ws.tri_overlap || (int)(np / NB) < c->ws.tri_min_nt) && persist_early_h(np, &c->ws) == 0 &&
                            c->ws.sched_state != 1;           // (the calibration's evaluation on launches is timed: plain launches)
    if (c->fgraph && !structural) drop_graph(c);
    const bool graphable = structural && !stage_ms;          // a call that wants the stage timings runs plain, the graph stays
    if (!graphable) {
        if (int rc = region(true)) return rc;
    } else if (c->fgraph) {
        HIP_CHECK(hipGraphLaunch(c->fgraph, st));
    } else if (c->fgraph_calls++ == 0) {
        if (int rc = region(false)) return rc;
    } else {
        // The capture runs on the device's SHARED streams: while it is open, a launch that another host thread makes on
        // them would be recorded into this graph instead of executed.  Entry points hold the engine gate shared;
        // the capture window takes it exclusively (nothing inside the window waits for another thread).
        hipGraph_t g = nullptr;
        if (!gate->try_exclusive()) {                         // another thread is inside an entry point: capture next time
            --c->fgraph_calls;
            if (int rc = region(false)) return rc;
        } else {
            bool ok = hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed) == hipSuccess;
            if (ok) {
                const int rc = region(false);
                ok = (hipStreamEndCapture(st, &g) == hipSuccess) && rc == 0 && g != nullptr;
            }
            gate->share();
            if (ok) ok = hipGraphInstantiate(&c->fgraph, g, nullptr, nullptr, 0) == hipSuccess;
            if (g) (void)hipGraphDestroy(g);
            if (!ok) {                                        // capture not possible here: stay on plain launches
                (void)hipGetLastError();
                c->fgraph = nullptr;
                c->graph_enabled = 0;
                if (int rc = region(false)) return rc;
            } else {
                c->fgraph_lookahead = c->ws.lookahead;
                HIP_CHECK(hipGraphLaunch(c->fgraph, st));
            }
        }
    }
    launch_scalars(st, c->dAlpha, c->dR, c->C, np, n, c->Dy, c->ws.logsum, c->ws.nblk, c->dScal, c->dDiag, c->ws.info);
    if (studentt_nu > 0.0) launch_studentt_scale(st, c->dScal, studentt_nu, n, c->dScal + 4);
    HIP_CHECK(hipEventRecord(c->ev[5], st));
    const int groups = (c->D + 31) / 32;
    const size_t nparts = with_kernel_grads ? c->parts.size() : 0;
    if (nparts > 0) {
        HIP_CHECK(hipMemsetAsync(c->dGradOutAll, 0, sizeof(double) * nparts * groups * GP_STRIDE, st));
        HIP_CHECK(hipMemsetAsync(c->dPack + c->offExt, 0, sizeof(double) * nparts * groups * GP_STRIDE, st));
        const int nb = grad_num_blocks(n);
        for (size_t p = 0; p < nparts; ++p) {       // every part reduces the same dL_dK against its own dK/dtheta
            const mi355gp_ctx::Part& pt = c->parts[p];
            // factor of a product: dL_dK is weighted by the covariances of the term's other factors (prod.py:86-99),
            // rebuilt into Mbuf (lower tiles) by one K-build pass per other factor
            const bool prod = emit_other_factors(c->terms, pt.tix, p, c->Mbuf, [&](int g, double* dst, const double* mul, int, bool) {
                launch_kbuild_sym(st, c->parts[(size_t)g].kp, c->parts[(size_t)g].dXt, np, n, np, dst, nullptr, 0, 0.0,
                                  /*lower_only=*/1, /*add_diag=*/0, /*accumulate=*/0, mul);
            });
            const double* Mul = prod ? c->Mbuf : nullptr;
            if (pt.coreg()) {                                           // the bucketed gradient: S (P x P) per part
                const int P = pt.kp.ard;
                const int nbc = launch_grad_coreg(st, true, pt.kp, pt.dXt, np, n, pt.dXt, np, n, c->C, np, c->dAlpha, c->Dy,
                                                  c->dCoregPart, studentt_nu > 0.0 ? c->dScal + 4 : nullptr, Mul, np);
                launch_reduce_partials(st, c->dCoregPart, nbc, P * P, c->dPack + c->offCoreg + p * COREG_REC);
                continue;
            }
            launch_grad_fused(st, pt.kp, pt.dXt, np, n, c->C, np, c->dAlpha, c->Dy, c->dGradPart,
                              studentt_nu > 0.0 ? c->dScal + 4 : nullptr, Mul, np);
            for (int g = 0; g < (pt.kp.ard ? groups : 1); ++g)
                launch_reduce_partials(st, c->dGradPart + (long)g * nb * GP_STRIDE, nb, GP_STRIDE,
                                       c->dGradOutAll + ((long)p * groups + g) * GP_STRIDE);
            if (pt.ext())                                                  // their second record (k_grad_ext)
                for (int g = 0; g < (pt.kp.ard ? groups : 1); ++g)
                    launch_reduce_partials(st, c->dGradPart + ((long)groups + g) * nb * GP_STRIDE, nb, GP_STRIDE,
                                           c->dPack + c->offExt + ((long)p * groups + g) * GP_STRIDE);
        }
    }
    HIP_CHECK(hipEventRecord(c->ev[6], st));
    // ONE device -> pinned host copy of the prefix of the result block that the caller asked for
    bool coreg = false;
    for (size_t p = 0; p < nparts; ++p) coreg = coreg || c->parts[p].coreg();
    const size_t ncopy = coreg ? c->packDoubles : (diag_out ? c->offCoreg : (alpha_out ? c->offDiag : c->offAlpha));
    HIP_CHECK(hipMemcpyAsync(c->hPack, c->dPack, sizeof(double) * ncopy, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    const double* scal = c->hPack;
    int info[1] = {(int)c->hPack[6]};                          // written by k_scalars from the factorisation's info word
    const double* sumsp = c->hPack + c->offGrad;
    if (alpha_out) memcpy(alpha_out, c->hPack + c->offAlpha, sizeof(double) * n * c->Dy);
    if (diag_out) memcpy(diag_out, c->hPack + c->offDiag, sizeof(double) * n);
    if (stage_ms) {
        float ms;
        for (int i = 0; i < MI355GP_NUM_T; ++i) stage_ms[i] = 0.0;
        const int map[6] = {MI355GP_T_KBUILD, MI355GP_T_POTRF, MI355GP_T_TRTRI, MI355GP_T_LAUUM, MI355GP_T_SOLVE,
                            MI355GP_T_GRAD};
        for (int i = 0; i < 6; ++i) {
            HIP_CHECK(hipEventElapsedTime(&ms, c->ev[i], c->ev[i + 1]));
            stage_ms[map[i]] = ms;
        }
        HIP_CHECK(hipEventElapsedTime(&ms, c->ev[0], c->ev[6]));
        stage_ms[MI355GP_T_TOTAL] = ms;
    }
    bool clean = false;
    if (potrf_persist_aborted(info[0], &c->ws, &clean)) {
        // The persistent factorisation did not run: called off at its co-residency gate (something else held CUs: the matrix
        // is untouched) or, never seen in a sane run, aborted on a wait timeout (the matrix is rebuilt).  Redo the evaluation
        // here with the launch-per-step schedule (same bits); the caller never sees it, the jitter ladder never hears of it.
        c->have_factor = false;
        drop_graph(c);
        if (attempt == 0 && (clean || rebuild)) {
            if (!clean)
                if (int rc = rebuild()) return rc;
            return run_pipeline(c, gate, with_kernel_grads, out_scalars, alpha_out, dtheta_out, diag_out, stage_ms,
                                rebuild, studentt_nu, attempt + 1);
        }
        mi355gp_set_error("the persistent factorisation aborted and could not be redone (info %d); this context continues "
                          "with the launch-per-step schedule -- repeat the call", info[0]);
        return -6;
    }
    if (info[0] > 0) {
        c->have_factor = false;
        if (info[0] > n) info[0] = (int)n;
        if (c->ws.sched_state == 1) {                          // a calibration in progress does not survive a failed evaluation:
            c->ws.sched_state = c->ws.sched_force_steps = 0;   // start over (it used to stay in state 1 for good: no graph
            c->ws.sched_np = c->ws.sched_ns = 0;               // replay, never decided -- ADVICE r5)
        }
        return info[0];
    }
    c->have_factor = true;
    c->studentt = studentt_nu > 0.0;
    // schedule of a small factorisation by measurement (FactorWs::persist_auto): potrf .. lauum of this evaluation, device time.
    // Two warm samples of the persistent schedule (from the fourth evaluation on), then THREE evaluations on launches -- the
    // first untimed (that workspace's first run on that schedule pays one-time function attributes and cold caches), the
    // next two timed; the minima are compared.  One sample each on a shared GPU used to pin the wrong schedule.
    if (c->ws.persist_auto && c->ws.sched_state < 2 && !graphable && attempt == 0 && (int)(np / NB) >= c->ws.persist_tri_min_nt) {
        float ms = 0.f;
        FactorWs& w = c->ws;
        if (hipEventElapsedTime(&ms, c->ev[1], c->ev[4]) == hipSuccess) {
            if (w.sched_state == 0 && w.persist_used && w.evals_done >= 3) {     // persistent launch + early inverse, warm
                w.sched_ms_persist = (w.sched_np == 0 || ms < w.sched_ms_persist) ? ms : w.sched_ms_persist;
                if (++w.sched_np >= 2) {
                    w.sched_state = 1;
                    w.sched_force_steps = 3;
                    w.sched_ns = 0;
                }
            } else if (w.sched_state == 1 && !w.persist_used) {
                if (w.sched_ns++ > 0) w.sched_ms_steps = (w.sched_ns == 2 || ms < w.sched_ms_steps) ? ms : w.sched_ms_steps;
                if (w.sched_ns >= 3) {
                    w.sched_state = 2;
                    w.sched_force_steps = 0;
                    w.persist_auto_off = (w.sched_ms_steps < 0.97f * w.sched_ms_persist) ? 1 : 0;
                    if ((int)(np / NB) >= 21) persist_box_verdict(w.persist_auto_off);   // one vote for the process-wide verdict
                }
            }
        } else {
            (void)hipGetLastError();
        }
    }
    const double datafit = scal[0], alpha2 = scal[1], trw = scal[2], logdet = scal[3];
    const double Dy = (double)c->Dy;
    for (int i = 0; i < MI355GP_NUM_OUT; ++i) out_scalars[i] = 0.0;
    out_scalars[MI355GP_OUT_LML] = 0.5 * (-(double)n * Dy * LOG_2_PI - Dy * logdet - datafit);
    out_scalars[MI355GP_OUT_LOGDET] = logdet;
    out_scalars[MI355GP_OUT_DATAFIT] = datafit;
    out_scalars[MI355GP_OUT_DNOISE] = 0.5 * (alpha2 - Dy * trw);
    out_scalars[MI355GP_OUT_TRKINV] = trw;
    if (studentt_nu > 0.0) {
        // Student-t process (exact_studentt_inference.py:36-52): beta = sum(alpha * R)
        const double nu = studentt_nu, N = (double)n, beta = datafit;
        out_scalars[MI355GP_OUT_LML] = 0.5 * (-N * log((nu - 2.0) * M_PI) - logdet - (nu + N) * log(1.0 + beta / (nu - 2.0))) +
                                       lgamma(0.5 * (nu + N)) - lgamma(0.5 * nu);
        out_scalars[5] = (nu + N) / (nu + beta - 2.0);                       // factor of dL_dm = factor * alpha
        out_scalars[MI355GP_OUT_DNOISE] = 0.0;
    }
    if (nparts > 0 && dtheta_out) {                              // per part, concatenated in part order
        double* o = dtheta_out;
        for (size_t p = 0; p < nparts; ++p) {
            const double* rec = c->parts[p].coreg() ? c->hPack + c->offCoreg + p * COREG_REC : sumsp + p * (size_t)groups * GP_STRIDE;
            o += part_dtheta(c->parts[p], rec, c->hPack + c->offExt + p * (size_t)groups * GP_STRIDE, o);
        }
    }
    return 0;
}

static bool has_coreg(const mi355gp_ctx* c) {
    for (const auto& p : c->parts)
        if (p.coreg()) return true;
    return false;
}
// new points (M x D, host) against every Coregionalize part: their output indices must be valid
static int coreg_check_points(const mi355gp_ctx* c, const double* Xn, int64_t M, const char* what) {
    for (const auto& p : c->parts)
        if (p.coreg())
            if (int rc = coreg_check_index(Xn + p.kp.col, M, c->D, p.kp.ard, what)) return rc;
    return 0;
}
// a part whose diagonal depends on the point (Coregionalize, Linear, MLP, Poly): Kdiag of the expression is then no constant
static bool has_point_diag(const mi355gp_ctx* c) {
    for (const auto& p : c->parts)
        if (p.diag_by_point()) return true;
    return false;
}
// Kdiag of the expression at each new point: kd[m] = sum over terms of the product of the factors' diagonals -- B[idx_m][idx_m]
// of a Coregionalize factor (coregionalize.py:106-107), sum_q variance_q x_mq^2 over the active columns of a Linear factor
// (linear.py:84-85), var (2/pi) asin(p / (p + 1)) of an MLP factor (mlp.py:61-64), var (scale |x|^2 + bias)^order of a Poly factor
// (poly.py:33-34), the variance of any other
static std::vector<double> expression_kdiag_points(const mi355gp_ctx* c, const double* Xn, int64_t M) {
    std::vector<double> kd((size_t)M, 0.0);
    for (int64_t m = 0; m < M; ++m) {
        double s = 0.0;
        for (const auto& t : c->terms) {
            double v = 1.0;
            for (int f : t) {
                const mi355gp_ctx::Part& p = c->parts[(size_t)f];
                if (p.coreg()) {
                    const int a = (int)Xn[m * c->D + p.kp.col], P = p.kp.ard;
                    v *= p.theta[(size_t)(a * P + a)];
                } else if (p.linear()) {
                    double d = 0.0;
                    for (size_t a = 0; a < p.dims.size(); ++a) {
                        const double x = Xn[m * c->D + p.dims[a]];
                        d += p.theta[p.kp.ard ? a : 0] * x * x;
                    }
                    v *= d;
                } else if (p.mlp()) {
                    v *= mlp_kdiag(p, Xn + m * c->D);
                } else if (p.poly()) {
                    v *= poly_kdiag(p, Xn + m * c->D);
                } else {
                    v *= p.kp.variance;
                }
            }
            s += v;
        }
        kd[(size_t)m] = s;
    }
    return kd;
}

static int upload_noise(mi355gp_ctx* c, const double* noise, int64_t noise_len) {
    ARG_CHECK(noise != nullptr && (noise_len == 1 || noise_len == c->n),
              "noise must have 1 or N entries");
    HIP_CHECK(hipMemcpyAsync(c->dNoise, noise, sizeof(double) * noise_len, hipMemcpyHostToDevice, c->st));
    return 0;
}

// the helpers laplace.hip shares (ctx.h)
static int prepare_parts(mi355gp_ctx* c, int nparts, const mi355gp_part* parts);
static void scale_parts(mi355gp_ctx* c);
static Resident<mi355gp_ctx::Part> training_points(const mi355gp_ctx* c);
int ctx_prepare_parts(mi355gp_ctx* c, int nparts, const mi355gp_part* parts) { return prepare_parts(c, nparts, parts); }
void ctx_scale_parts(mi355gp_ctx* c) { scale_parts(c); }
Resident<mi355gp_ctx::Part> ctx_training_points(const mi355gp_ctx* c) { return training_points(c); }
int ctx_coreg_check_points(const mi355gp_ctx* c, const double* Xn, int64_t M, const char* what) { return coreg_check_points(c, Xn, M, what); }
bool ctx_has_point_diag(const mi355gp_ctx* c) { return has_point_diag(c); }
std::vector<double> ctx_kdiag_points(const mi355gp_ctx* c, const double* Xn, int64_t M) { return expression_kdiag_points(c, Xn, M); }

extern "C" {

// validates the part list and (re)builds the per-part device inputs
static int prepare_parts(mi355gp_ctx* c, int nparts, const mi355gp_part* parts) {
    ARG_CHECK(nparts >= 1 && nparts <= 16 && parts, "between 1 and 16 kernel parts");
    if ((int)c->parts.size() != nparts) {
        c->parts.clear();
        c->parts.resize((size_t)nparts);
        for (auto& p : c->parts) HIP_CHECK(p.dXt.alloc((size_t)c->D * c->npad));
    }
    for (int i = 0; i < nparts; ++i) {
        mi355gp_ctx::Part& p = c->parts[(size_t)i];
        if (int rc = parse_part(parts[i], c->D, KS_STATIONARY | KS_STATIC | KS_EXT | KS_COREG | KS_LINEAR | KS_DOT, "exact-GP path", &p)) return rc;
        if (p.coreg()) {
            const int col = p.kp.col;
            if (c->hIdxCol != col) {                     // the training indices of this column, validated once per upload
                c->hIdx.resize((size_t)c->n);
                HIP_CHECK(hipMemcpy2D(c->hIdx.data(), sizeof(double), c->dX + col, sizeof(double) * c->D, sizeof(double), c->n,
                                      hipMemcpyDeviceToHost));
                c->hIdxCol = col;
            }
            if (int rc = coreg_check_index(c->hIdx.data(), c->n, 1, p.kp.ard, "training")) return rc;
            if (!c->dCoregPart) HIP_CHECK(hipMalloc(&c->dCoregPart, sizeof(double) * grad_num_blocks(c->n) * COREG_REC));
        }
        if (int rc = p.upload(c->st)) return rc;
    }
    c->terms = group_terms(c->parts);
    if (has_product(c->terms) && !c->Mbuf) HIP_CHECK(hipMalloc(&c->Mbuf, sizeof(double) * c->npad * c->npad));
    return 0;
}

// scaled inputs of every part (inactive dimensions scaled by 0: they drop out of r), on the context's stream
static void scale_parts(mi355gp_ctx* c) {
    for (auto& p : c->parts) launch_scale_inputs(c->st, c->dX, c->n, c->D, p.dIl, /*per-dimension vector*/ 1, p.dXt, c->npad);
}
// the training inputs as one side of a cross-covariance (emit_cross)
static Resident<mi355gp_ctx::Part> training_points(const mi355gp_ctx* c) { return {&mi355gp_ctx::Part::dXt, c->npad, c->n}; }

int mi355gp_exact_inference_sum(mi355gp_ctx* c, int nparts, const mi355gp_part* parts, const double* noise,
                                int64_t noise_len, double jitter, double extra_jitter, double* out_scalars,
                                double* alpha_out, double* dtheta_out, double* diag_dLdK_out, double* stage_ms) {
    ARG_CHECK(c && c->n > 0, "mi355gp_exact_inference: set_data first");
    ARG_CHECK(out_scalars != nullptr, "out_scalars is NULL");
    HIP_CHECK(hipSetDevice(c->device));
    EngineShared gate(c->device);
    if (int rc = prepare_parts(c, nparts, parts)) return rc;
    if (int rc = upload_noise(c, noise, noise_len)) return rc;
    hipStream_t st = c->st;
    c->have_kernel = true;
    HIP_CHECK(hipEventRecord(c->ev[0], st));
    scale_parts(c);
    // Ky = sum_t prod_f K_f + (noise + jitter) I   (add.py:58-72, prod.py:58-65)
    auto build = [&]() -> int {
        emit_expression(c->terms, c->A, c->Mbuf, false, [&](int p, double* dst, const double* mul, int acc, bool first) {
            launch_kbuild_sym(st, c->parts[(size_t)p].kp, c->parts[(size_t)p].dXt, c->npad, c->n, c->npad, dst, c->dNoise,
                              noise_len, jitter + extra_jitter, /*lower_only=*/1, /*add_diag=*/first, acc, mul);
        });
        return 0;
    };
    build();
    return run_pipeline(c, &gate, true, out_scalars, alpha_out, dtheta_out, diag_dLdK_out, stage_ms, build);
}

// Student-t PROCESS inference (ExactStudentTInference.inference, exact_studentt_inference.py:20-52): the same pdinv +
// dpotrs skeleton with Ky = K + 1e-8 I and dL_dK = 0.5 ((nu+N)/(nu+beta-2) alpha alpha^T - Dy Ky^-1).
// out_scalars: LML (Student-t), LOGDET, DATAFIT (= beta), [5] = (nu+N)/(nu+beta-2); dL_dnu is O(1) host arithmetic on beta.
int mi355gp_exact_studentt_sum(mi355gp_ctx* c, int nparts, const mi355gp_part* parts, double nu, double jitter,
                               double extra_jitter, double* out_scalars, double* alpha_out, double* dtheta_out,
                               double* stage_ms) {
    ARG_CHECK(c && c->n > 0, "mi355gp_exact_studentt_sum: set_data first");
    ARG_CHECK(out_scalars != nullptr && nu > 2.0, "mi355gp_exact_studentt_sum: nu must exceed 2");
    HIP_CHECK(hipSetDevice(c->device));
    EngineShared gate(c->device);
    if (int rc = prepare_parts(c, nparts, parts)) return rc;
    const double zero = 0.0;
    if (int rc = upload_noise(c, &zero, 1)) return rc;
    hipStream_t st = c->st;
    c->have_kernel = true;
    HIP_CHECK(hipEventRecord(c->ev[0], st));
    scale_parts(c);
    auto build = [&]() -> int {
        emit_expression(c->terms, c->A, c->Mbuf, false, [&](int p, double* dst, const double* mul, int acc, bool first) {
            launch_kbuild_sym(st, c->parts[(size_t)p].kp, c->parts[(size_t)p].dXt, c->npad, c->n, c->npad, dst, c->dNoise, 1,
                              jitter + extra_jitter, 1, first, acc, mul);
        });
        return 0;
    };
    build();
    return run_pipeline(c, &gate, true, out_scalars, alpha_out, dtheta_out, nullptr, stage_ms, build, nu);
}

int mi355gp_exact_inference(mi355gp_ctx* c, int kind, int ard, const double* theta, const double* noise,
                            int64_t noise_len, double jitter, double extra_jitter, double* out_scalars,
                            double* alpha_out, double* dtheta_out, double* diag_dLdK_out, double* stage_ms) {
    if (int rc = check_kind(kind, KS_STATIONARY | KS_EXT | KS_LINEAR | KS_DOT, "mi355gp_exact_inference")) return rc;
    const mi355gp_part part{kind, ard, 0, nullptr, theta};
    return mi355gp_exact_inference_sum(c, 1, &part, noise, noise_len, jitter, extra_jitter, out_scalars, alpha_out,
                                       dtheta_out, diag_dLdK_out, stage_ms);
}

int mi355gp_inference_given_K(mi355gp_ctx* c, const double* K_host, const double* noise, int64_t noise_len,
                              double jitter, double extra_jitter, double* out_scalars, double* alpha_out,
                              double* diag_dLdK_out, double* stage_ms) {
    ARG_CHECK(c && c->n > 0, "mi355gp_inference_given_K: set_data first");
    ARG_CHECK(K_host && out_scalars, "NULL argument");
    HIP_CHECK(hipSetDevice(c->device));
    EngineShared gate(c->device);
    if (int rc = upload_noise(c, noise, noise_len)) return rc;
    hipStream_t st = c->st;
    c->have_kernel = false;
    // stage the dense n x n matrix in C (free until lauum), then pad + add the diagonal into A
    HIP_CHECK(hipEventRecord(c->ev[0], st));
    auto build = [&]() -> int {
        HIP_CHECK(hipMemcpyAsync(c->C, K_host, sizeof(double) * c->n * c->n, hipMemcpyHostToDevice, st));
        launch_pad_from_dense(st, c->C, c->n, c->A, c->npad, c->dNoise, noise_len, jitter + extra_jitter);
        return 0;
    };
    if (int rc = build()) return rc;
    return run_pipeline(c, &gate, false, out_scalars, alpha_out, nullptr, diag_dLdK_out, stage_ms, build);
}

int mi355gp_fetch(mi355gp_ctx* c, int which, double* out, int fortran_order) {
    ARG_CHECK(c && c->n > 0 && out, "mi355gp_fetch: bad arguments");
    HIP_CHECK(hipSetDevice(c->device));
    EngineShared gate(c->device);
    const long n = c->n, np = c->npad;
    hipStream_t st = c->st;
    DevBuf tmp, scratch;
    HIP_CHECK(tmp.alloc(n * n));
    if (c->lap_stage > 0) {                                   // the matrices of a Laplace session (laplace.hip)
        if (int rc = laplace_fetch(c, which, tmp)) return rc;
    } else if (which == MI355GP_FETCH_K) {
        if (!c->have_kernel) {
            mi355gp_set_error("mi355gp_fetch(K): no device kernel evaluation in this context");
            return -4;
        }
        if (has_product(c->terms)) HIP_CHECK(scratch.alloc(n * n));
        const auto x = training_points(c);                                                 // symmetric: no transpose needed
        emit_cross(st, c->parts, c->terms, x, x, tmp, n, scratch, false, /*diag_same=*/1);
    } else if (!c->have_factor) {
        mi355gp_set_error("mi355gp_fetch: no successful factorisation in this context");
        return -4;
    } else if (which == MI355GP_FETCH_L) {
        launch_extract(st, c->A, np, n, 0, nullptr, 0, tmp, fortran_order);
    } else if (which == MI355GP_FETCH_LINV) {
        launch_extract(st, c->B, np, n, 0, nullptr, 0, tmp, fortran_order);        // X = L^-1 (lower)
    } else if (which == MI355GP_FETCH_KINV) {
        launch_extract(st, c->C, np, n, 1, nullptr, 0, tmp, 0);
    } else if (which == MI355GP_FETCH_DLDK) {
        launch_extract(st, c->C, np, n, 2, c->dAlpha, c->Dy, tmp, 0, c->studentt ? c->dScal + 4 : nullptr);
    } else {
        mi355gp_set_error("mi355gp_fetch: unknown matrix id %d", which);
        return -1;
    }
    HIP_CHECK(hipMemcpyAsync(out, tmp, sizeof(double) * n * n, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}

// ---- stateless kernel-function entry points --------------------------------------------------------
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

int mi355gp_kern_K(int device, int kind, int ard, const double* theta, const double* X, int64_t N,
                   const double* X2, int64_t M, int D, double* K_out) {
    ARG_CHECK(X && K_out && N > 0 && D > 0, "mi355gp_kern_K: bad arguments");
    HIP_CHECK(hipSetDevice(device));
    const bool sym = (X2 == nullptr);
    if (sym) M = N;
    ARG_CHECK(M > 0, "mi355gp_kern_K: M must be positive");
    StatelessPart pt;
    if (int rc = pt.load(kind, ard, theta, D, KS_STATIONARY | KS_EXT | KS_COREG | KS_LINEAR | KS_DOT, "mi355gp_kern_K", X, N, X2, M)) return rc;
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
    ARG_CHECK(kind_in(kind, KS_STATIONARY | KS_EXT) && theta && out && N >= 0, "mi355gp_kern_Kdiag: bad arguments");
    // stationary: K(x,x) = variance (stationary.py:170-173); StdPeriodic likewise (standard_periodic.py:105-109)
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
    if (int rc = pt.load(kind, ard, theta, D, KS_STATIONARY | KS_EXT | KS_COREG | KS_LINEAR | KS_DOT, "mi355gp_update_gradients_full", X, N, X2, M))
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
// Runs as the column reduction H^T [X2~ | 1] of the transposed problem (the same kernels as the sparse path's dL/dZ).
int mi355gp_gradients_X(int device, int kind, int ard, const double* theta, const double* dL_dK, const double* X,
                        int64_t N, const double* X2, int64_t M, int D, double* out) {
    ARG_CHECK(dL_dK && X && out && N > 0 && D > 0, "mi355gp_gradients_X: bad arguments");
    HIP_CHECK(hipSetDevice(device));
    if (kind == MI355GP_POLY) {
        mi355gp_set_error("mi355gp_gradients_X: Poly (kind 11) has no gradients_X (the reference raises NotImplementedError, poly.py:45-46)");
        return -1;
    }
    StatelessPart pt;
    if (int rc = pt.load(kind, ard, theta, D, KS_STATIONARY | KS_EXT | KS_LINEAR | 1u << MI355GP_MLP, "mi355gp_gradients_X", nullptr, 0, nullptr, 0)) return rc;
    const bool sym = (X2 == nullptr);
    if (sym) { M = N; X2 = X; }
    ARG_CHECK(M > 0, "mi355gp_gradients_X: M must be positive");
    PointSet xc, xr;                                         // X and X2
    if (int rc = pt.scaled(xc, X, N)) return rc;
    if (int rc = pt.scaled(xr, X2, M)) return rc;
    if (kind == MI355GP_STDPERIODIC) {
        // StdPeriodic.gradients_X (standard_periodic.py:574-580): dX[i][q] = -pi / (2 T_q l_q^2) sum_j W_ij K_ij sin(2 Delta_ijq),
        // W = dL_dK (+ dL_dK^T against X itself), as a row reduction on the device (k_periodic_gradx)
        std::vector<double> W((size_t)N * M);
        for (int64_t i = 0; i < N; ++i)
            for (int64_t j = 0; j < M; ++j) W[(size_t)i * M + j] = sym ? dL_dK[i * M + j] + dL_dK[j * M + i] : dL_dK[i * M + j];
        DevBuf dW, dOut;
        HIP_CHECK(dW.alloc(N * M));
        HIP_CHECK(dOut.alloc(N * D));
        HIP_CHECK(hipMemcpy(dW, W.data(), sizeof(double) * N * M, hipMemcpyHostToDevice));
        launch_periodic_gradx(0, pt.kp, xc.t, xc.ld, N, xr.t, xr.ld, M, dW, M, 0, dOut);
        HIP_CHECK(hipMemcpy(out, dOut, sizeof(double) * N * D, hipMemcpyDeviceToHost));
        HIP_CHECK(hipGetLastError());
        gradx_periodic(pt.pw, N, D, out, [&](long i, int q, double g) { out[i * D + q] = g; });      // in place
        return 0;
    }
    // transposed weights G' (M x N): rows = X2 points, columns = X points
    std::vector<double> Gt((size_t)M * N);
    for (int64_t i = 0; i < N; ++i)
        for (int64_t j = 0; j < M; ++j)
            Gt[(size_t)j * N + i] = sym ? dL_dK[i * M + j] + dL_dK[j * M + i] : dL_dK[i * M + j];
    DevBuf dG, dPart, dCol, dHX;
    HIP_CHECK(dG.alloc(M * N));
    HIP_CHECK(dPart.alloc(2 * 2048 * GP_STRIDE * ((D + 31) / 32)));   // every group, and the second records of RatQuad
    HIP_CHECK(dCol.alloc(64 * N * (D + 1)));
    HIP_CHECK(dHX.alloc(N * (D + 1)));
    HIP_CHECK(hipMemcpy(dG, Gt.data(), sizeof(double) * M * N, hipMemcpyHostToDevice));
    if (pt.linear()) {
        // Linear.gradients_X (linear.py:108-114): out[i][q] = variance_q sum_j W_ij x2_jq -- the weights are dL_dK itself
        const int ns = launch_colreduce_multi(0, dG, N, M, N, xr.t, 1, xr.ld, D, 0, dCol);
        launch_sum_splits(0, dCol, N * D, ns, 0, dHX);
        std::vector<double> HX((size_t)N * D);
        HIP_CHECK(hipMemcpy(HX.data(), dHX, sizeof(double) * HX.size(), hipMemcpyDeviceToHost));
        HIP_CHECK(hipGetLastError());
        gradx_linear(pt.inv_ls, N, D, HX.data(), [&](long i, int q, double g) { out[i * D + q] = g; });
        return 0;
    }
    launch_grad_generic(0, pt.kp, xr.t, xr.ld, M, xc.t, xc.ld, N, 0, dG, N, dPart, dG, N);   // H in place
    const int ns = launch_colreduce_multi(0, dG, N, M, N, xr.t, 1, xr.ld, D, 1, dCol);
    launch_sum_splits(0, dCol, N * (D + 1), ns, 0, dHX);
    std::vector<double> HX((size_t)N * (D + 1));
    HIP_CHECK(hipMemcpy(HX.data(), dHX, sizeof(double) * HX.size(), hipMemcpyDeviceToHost));
    HIP_CHECK(hipGetLastError());
    if (pt.mlp()) {                                          // H = c (mlp.py:105; X2 == NULL: from dL_dK + dL_dK^T, i.e. c + c^T, :124-127)
        gradx_mlp(X, N, D, pt.inv_ls, pt.kp.bias, HX.data(), [&](long i, int q, double g) { out[i * D + q] = g; });
        return 0;
    }
    gradx_stationary(X, N, D, pt.inv_ls, HX.data(), [&](long i, int q, double g) { out[i * D + q] = g; });
    return 0;
}

// ---- standalone dense routines ------------------------------------------------------------------------
static int dense_factor(int device, const double* A_host, int64_t N, bool invert, double* L_out, double* Ainv_out,
                        double* logdet, double* ms, double* Li_out = nullptr) {
    HIP_CHECK(hipSetDevice(device));
    const long np = round_up(N, NB);
    DevBuf A, B, C, tmp;                                      // released on every return path
    struct WsGuard {                                          // ... and so are the workspace and the two events
        FactorWs ws;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~WsGuard() {
            factor_ws_free(&ws);
            if (e0) (void)hipEventDestroy(e0);
            if (e1) (void)hipEventDestroy(e1);
        }
    } guard;
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
    HIP_CHECK(hipEventCreate(&guard.e0));
    HIP_CHECK(hipEventCreate(&guard.e1));
    hipEvent_t e0 = guard.e0, e1 = guard.e1;
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
        if (L_out) {
            launch_extract(0, A, np, N, 0, nullptr, 0, tmp, 0);
            HIP_CHECK(hipMemcpy(L_out, tmp, sizeof(double) * N * N, hipMemcpyDeviceToHost));
        }
        if (invert && Ainv_out) {
            launch_extract(0, C, np, N, 1, nullptr, 0, tmp, 0);
            HIP_CHECK(hipMemcpy(Ainv_out, tmp, sizeof(double) * N * N, hipMemcpyDeviceToHost));
        }
        if (invert && Li_out) {                                   // L^-1: the dtrtri result pdinv also returns (linalg.py:207)
            launch_extract(0, B, np, N, 0, nullptr, 0, tmp, 0);
            HIP_CHECK(hipMemcpy(Li_out, tmp, sizeof(double) * N * N, hipMemcpyDeviceToHost));
        }
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

int mi355gp_predict_sum(mi355gp_ctx* c, int nparts, const mi355gp_part* parts, const double* Xnew, int64_t M,
                        double* mu_out, double* var_out, int full_cov) {
    ARG_CHECK(c && c->n > 0 && c->have_factor && c->lap_stage == 0, "mi355gp_predict: run an inference call first");
    ARG_CHECK(Xnew && M > 0 && mu_out, "mi355gp_predict: bad arguments");
    HIP_CHECK(hipSetDevice(c->device));
    EngineShared gate(c->device);
    if (int rc = prepare_parts(c, nparts, parts)) return rc;
    if (int rc = coreg_check_points(c, Xnew, M, "prediction")) return rc;
    hipStream_t st = c->st;
    const long n = c->n, np = c->npad, mp = round_up(M, NB);
    // (re)scale the training inputs for these parameters (normally identical to the inference call's)
    c->have_kernel = true;
    scale_parts(c);
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
    const bool kd_points = has_point_diag(c) && !full_cov && var_out;
    std::vector<double> kd;
    if (kd_points) {
        kd = expression_kdiag_points(c, Xnew, M);
        HIP_CHECK(dKd.alloc(M));
        HIP_CHECK(hipMemcpyAsync(dKd, kd.data(), sizeof(double) * M, hipMemcpyHostToDevice, st));
    }
    DevBuf dScr1, dScr2;
    if (has_product(c->terms)) {
        HIP_CHECK(dScr1.alloc(np * mp));
        if (full_cov && var_out) HIP_CHECK(dScr2.alloc(mp * mp));
    }
    emit_cross(st, c->parts, c->terms, training_points(c), xs, dKx, mp, dScr1, true, 0);                    // K(X, X*) (n x M)
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

// G[i][j] = v[i * stride] for i < n, j < m (row-constant weights: dL_dK of the mean part of predictive_gradients)
__global__ void k_fill_rows(double* __restrict__ G, long ld, long n, long m, const double* __restrict__ v, int stride) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * m) return;
    const long i = idx / m, j = idx - i * m;
    G[i * ld + j] = v[i * stride];
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
    if (int rc = prepare_parts(c, nparts, parts)) return rc;
    ARG_CHECK(!has_product(c->terms), "mi355gp_predictive_gradients: product kernels are not supported on the device");
    ARG_CHECK(!has_coreg(c), "mi355gp_predictive_gradients: Coregionalize (kind 8) parts are not supported on the device");
    for (const auto& p : c->parts)
        ARG_CHECK(!p.poly(), "mi355gp_predictive_gradients: Poly (kind 11) has no gradients_X (poly.py:45-49)");
    hipStream_t st = c->st;
    const long n = c->n, np = c->npad, D = c->D, Dy = c->Dy, mp = round_up(M, NB);
    c->have_kernel = true;
    scale_parts(c);
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
        emit_cross(st, c->parts, c->terms, training_points(c), xs, dU, mp, nullptr, true, 0);
        launch_trmm_lower(st, c->B, np, dU, mp, dT, mp, (int)(np / NB), (int)(mp / NB));
        launch_trmm_lower_T(st, c->B, np, dT, mp, dU, mp, (int)(np / NB), (int)(mp / NB));
    }
    // one pass per weight matrix (Dy mean parts, one variance part) and stationary part
    const size_t hx = (size_t)M * (D + 1);
    std::vector<double> HX(hx);
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
            if (pt.linear()) {
                // dK(x*_m, x_n)/dx*_mq = variance_q x_nq (linear.py:108-114): the column reduction W^T x~ of the weights themselves
                const int ns = launch_colreduce_multi(st, W, mp, n, M, pt.dXt, 1, np, (int)D, 0, dCol);
                launch_sum_splits(st, dCol, (long)M * D, ns, 0, dHX);
                HIP_CHECK(hipMemcpyAsync(HX.data(), dHX, sizeof(double) * M * D, hipMemcpyDeviceToHost, st));
                HIP_CHECK(hipStreamSynchronize(st));
                gradx_linear(pt.inv_ls, M, (int)D, HX.data(), add);
                if (is_var)                                                      // dKdiag/dx*_mq = 2 variance_q x*_mq
                    for (long m = 0; m < M; ++m)
                        for (size_t a = 0; a < pt.dims.size(); ++a)
                            dvar_out[m * D + pt.dims[a]] += 2.0 * pt.theta[pt.kp.ard ? a : 0] * Xnew[m * D + pt.dims[a]];
                continue;
            }
            const double* xt = xs.points(st, pt);
            if (pt.kp.kind == MI355GP_STDPERIODIC) {                    // not a function of r: the row reduction instead of H
                launch_periodic_gradx(st, pt.kp, xt, xs.ld, M, pt.dXt, np, n, W, mp, /*wt=*/1, dHX);
                HIP_CHECK(hipMemcpyAsync(HX.data(), dHX, sizeof(double) * M * D, hipMemcpyDeviceToHost, st));
                HIP_CHECK(hipStreamSynchronize(st));
                gradx_periodic(pt.pw, M, (int)D, HX.data(), add);
                continue;
            }
            launch_grad_generic(st, pt.kp, pt.dXt, np, n, xt, xs.ld, M, 0, W, mp, dPart, dH, mp);
            const int ns = launch_colreduce_multi(st, dH, mp, n, M, pt.dXt, 1, np, (int)D, 1, dCol);
            launch_sum_splits(st, dCol, (long)hx, ns, 0, dHX);
            HIP_CHECK(hipMemcpyAsync(HX.data(), dHX, sizeof(double) * hx, hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            if (pt.mlp()) {
                // H = c of the weights (k_grad_dot); dK(x*_m, x_n)/dx*_m from H^T [x~ | 1] (mlp.py:124-130, gradx_mlp)
                gradx_mlp(Xnew, M, (int)D, pt.inv_ls, pt.kp.bias, HX.data(), add);
                if (is_var)                                                      // dKdiag/dx*_mq = 2 cd_m w_q x*_mq (mlp.py:133-147)
                    for (long m = 0; m < M; ++m) {
                        const double cd = mlp_dkdiag_factor(pt, Xnew + m * D);
                        for (size_t a = 0; a < pt.dims.size(); ++a)
                            dvar_out[m * D + pt.dims[a]] += 2.0 * cd * pt.theta[1 + (pt.kp.ard ? a : 0)] * Xnew[m * D + pt.dims[a]];
                    }
                continue;
            }
            gradx_stationary(Xnew, M, (int)D, pt.inv_ls, HX.data(), add);       // (il = 0 outside active_dims)
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
    if (int rc = prepare_parts(c, nparts, parts)) return rc;
    if (int rc = coreg_check_points(c, X1, M1, "X1")) return rc;
    if (int rc = coreg_check_points(c, X2, M2, "X2")) return rc;
    hipStream_t st = c->st;
    const long np = c->npad, m1p = round_up(M1, NB), m2p = round_up(M2, NB);
    c->have_kernel = true;
    scale_parts(c);
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
    emit_cross(st, c->parts, c->terms, training_points(c), x1, dK1, m1p, dS1, true, 0);
    emit_cross(st, c->parts, c->terms, training_points(c), x2, dK2, m2p, dS2, true, 0);
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
    if (int rc = check_kind(kind, KS_STATIONARY | KS_EXT | KS_LINEAR | KS_DOT, "mi355gp_predict")) return rc;
    const mi355gp_part part{kind, ard, 0, nullptr, theta};
    return mi355gp_predict_sum(c, 1, &part, Xnew, M, mu_out, var_out, full_cov);
}

int mi355gp_set_option(mi355gp_ctx* c, int option, int value) {
    ARG_CHECK(c != nullptr, "mi355gp_set_option: NULL context");
    if (option == MI355GP_OPT_PROFILE) {
        c->ws.prof.on = (value != 0);
        c->ws.prof.mask = (value == 1) ? 0xffu : (unsigned)value >> 1;
        return 0;
    }
    if (option == MI355GP_OPT_PERSIST_TEST) {
#ifndef MI355GP_DIAG
        if (value != 0) {                  // the fault injectors exist in the diagnostics build only
            mi355gp_set_error("mi355gp_set_option: MI355GP_OPT_PERSIST_TEST is a test hook of the diagnostics build (libmi355gp_diag.so)");
            return -1;
        }
#endif
        c->ws.persist_test = value;
        if (value) c->ws.persist_skip = 0;
        drop_graph(c);
        return 0;
    }
    if (option < 0 || option >= MI355GP_OPT_NUM || option == MI355GP_OPT_PERSIST_ABORTS || option == MI355GP_OPT_PERSIST_SKIP ||
        option == MI355GP_OPT_PERSIST_SCHED) {
        mi355gp_set_error("mi355gp_set_option: unknown or read-only option %d", option);
        return -1;
    }
    if (option == MI355GP_OPT_LOOKAHEAD) value = (value == 0) ? 0 : 1;
    if (option == MI355GP_OPT_NBO && value > 0 && value % NB != 0) {
        mi355gp_set_error("mi355gp_set_option: NBO must be a multiple of %d", NB);
        return -1;
    }
    c->opt[option] = (value < 0) ? INT_MIN : value;
    if (value < 0) {
        // back to the process default: re-read what factor_ws_alloc reads (only the fields of this option are touched)
        FactorWs d;
#define env(name, dflt) diag_env_int(DIAG_ENV(name), dflt)
#define penv(name, dflt) diag_env_int(PRODUCT_ENV(name), dflt)
        switch (option) {
            case MI355GP_OPT_LOOKAHEAD: c->ws.lookahead = d.lookahead; break;
            case MI355GP_OPT_TRI_OVERLAP: c->ws.tri_overlap = penv("TRI_OVERLAP", d.tri_overlap) ? 1 : 0; break;
            case MI355GP_OPT_TRI_MIN_NT: c->ws.tri_min_nt = env("TRI_MIN_NT", d.tri_min_nt); break;
            case MI355GP_OPT_TRI_H: c->ws.tri_h_override = env("TRI_H", d.tri_h_override); break;
            case MI355GP_OPT_TRI_WGS: c->ws.tri_wgs = env("TRI_WGS", d.tri_wgs); break;
            case MI355GP_OPT_TRI_HALF: c->ws.tri_half_ok = env("TRI_HALF", d.tri_half_ok) ? 1 : 0; break;
            case MI355GP_OPT_PART1_ON_PANEL: c->ws.part1_on_panel = env("PART1_ON_PANEL", d.part1_on_panel) ? 1 : 0; break;
            case MI355GP_OPT_NBO: c->ws.nbo_override = env("NBO", d.nbo_override); break;
            case MI355GP_OPT_SOLVE_OVERLAP: c->ws.solve_overlap = env("SOLVE_OVERLAP", d.solve_overlap) ? 1 : 0; break;
            case MI355GP_OPT_DIAG_EXCL_FIRST: c->ws.diag_excl_first = env("DIAG_EXCL_FIRST", d.diag_excl_first) ? 1 : 0; break;
            case MI355GP_OPT_PERSIST: c->ws.persist = penv("PERSIST", d.persist); break;
            case MI355GP_OPT_AGG2: c->ws.agg2 = env("AGG2", d.agg2) ? 1 : 0; break;
            case MI355GP_OPT_GRAPH: c->graph_enabled = penv("GRAPH", 1) ? 1 : 0; break;
            default: break;
        }
#undef env
#undef penv
    }
    if (option == MI355GP_OPT_PERSIST) {  // an explicit choice ends the calibration by measurement, -1 re-opens it
        c->ws.persist_auto_off = 0;
        c->ws.sched_force_steps = 0;
        c->ws.sched_np = c->ws.sched_ns = 0;
        c->ws.sched_state = (value < 0) ? 0 : 2;
    }
    apply_options(c);
    drop_graph(c);                        // a captured factorisation region carries the old schedule
    return 0;
}

int mi355gp_get_option(mi355gp_ctx* c, int option, int* value) {
    ARG_CHECK(c && value && option > MI355GP_OPT_PROFILE && option < MI355GP_OPT_NUM, "mi355gp_get_option: bad arguments");
    const FactorWs& w = c->ws;
    const int v[MI355GP_OPT_NUM] = {0, w.lookahead, w.tri_overlap, w.tri_min_nt, w.tri_h_override, w.tri_wgs, w.tri_half_ok,
                                    w.part1_on_panel, w.nbo_override, w.solve_overlap, w.diag_excl_first, c->graph_enabled,
                                    w.persist, w.agg2, w.persist_test, w.persist_aborts, w.persist_skip,
                                    w.sched_state == 2 ? ((w.persist_auto_off || !w.persist) ? 2 : 1) : 0};
    *value = v[option];
    return 0;
}

int mi355gp_get_profile(mi355gp_ctx* c, double* ms, double* flops, int* launches) {
    ARG_CHECK(c && ms && flops && launches, "mi355gp_get_profile: NULL argument");
    HIP_CHECK(hipSetDevice(c->device));
    HIP_CHECK(hipStreamSynchronize(c->st));
    if (c->ws.st_panel) HIP_CHECK(hipStreamSynchronize(c->ws.st_panel));
    if (c->ws.prof.collect(ms, flops, launches) != 0) {
        mi355gp_set_error("mi355gp_get_profile: event timing failed");
        return -5;
    }
    return 0;
}

int mi355gp_bench_factor(int device, int64_t N, int reps, double* ms_potrf, double* ms_trtri, double* ms_lauum) {
    ARG_CHECK(N >= NB && reps >= 1 && ms_potrf && ms_trtri && ms_lauum, "mi355gp_bench_factor: N >= 128, reps >= 1");
    HIP_CHECK(hipSetDevice(device));
    const long np = round_up(N, NB);
    const int D = 4;
    // synthetic SPD matrix resident in HBM: RBF covariance of pseudo-random points + 0.1 I, rebuilt before every repetition
    std::vector<double> X((size_t)N * D);
    unsigned long long state = 0x9E3779B97F4A7C15ull;
    for (double& v : X) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        v = ((double)(state >> 11) / 9007199254740992.0 - 0.5) * 4.0;
    }
    DevBuf dX, dXt, dIl, dNoise, A, B, C;
    HIP_CHECK(dX.alloc(N * D));
    HIP_CHECK(dXt.alloc(D * np));
    HIP_CHECK(dIl.alloc(D));
    HIP_CHECK(dNoise.alloc(1));
    HIP_CHECK(A.alloc(np * np));
    HIP_CHECK(B.alloc(np * np));
    HIP_CHECK(C.alloc(np * np));
    const double il[4] = {0.7, 0.7, 0.7, 0.7}, noise = 0.1;
    HIP_CHECK(hipMemcpy(dX, X.data(), sizeof(double) * N * D, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dIl, il, sizeof(il), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dNoise, &noise, sizeof(double), hipMemcpyHostToDevice));
    hipStream_t st;
    if (factor_engine(device, &st, nullptr, nullptr) != 0) return -2;
    FactorWs ws;
    if (factor_ws_alloc(&ws, np) != 0) return -3;
    ws.scratchX = B;
    ws.scratchT = C;
    hipEvent_t e[4];
    for (auto& ev : e) HIP_CHECK(hipEventCreate(&ev));
    const KernParams kp{MI355GP_RBF, 0, D, 1.0};
    launch_scale_inputs(st, dX, N, D, dIl, 0, dXt, np);
    double acc[3] = {0.0, 0.0, 0.0};
    int info = 0, first_info = 0, redone = 0;
    for (int r = -1; r < reps; ++r) {                          // r = -1: warm-up
        launch_kbuild_sym(st, kp, dXt, np, N, np, A, dNoise, 1, 1e-8, 1, 1);
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
                for (auto& ev : e) (void)hipEventDestroy(ev);
                factor_ws_free(&ws);
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
    for (auto& ev : e) (void)hipEventDestroy(ev);
    factor_ws_free(&ws);
    HIP_CHECK(hipGetLastError());
    return info > 0 ? info : 0;
}

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
    const int nt = (int)(np / NB), D = 4;
    std::vector<double> X((size_t)N * D);
    unsigned long long state = 0x9E3779B97F4A7C15ull;
    for (double& v : X) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        v = ((double)(state >> 11) / 9007199254740992.0 - 0.5) * 4.0;
    }
    DevBuf dX, dXt, dIl, dNoise, A, B, dStamp, dCount;
    HIP_CHECK(dX.alloc(N * D));
    HIP_CHECK(dXt.alloc(D * np));
    HIP_CHECK(dIl.alloc(D));
    HIP_CHECK(dNoise.alloc(1));
    HIP_CHECK(A.alloc(np * np));
    HIP_CHECK(B.alloc(np * np));
    HIP_CHECK(dStamp.alloc(32 * nt));
    HIP_CHECK(dCount.alloc(1));
    const double il[4] = {0.7, 0.7, 0.7, 0.7}, noise = 0.1;
    HIP_CHECK(hipMemcpy(dX, X.data(), sizeof(double) * N * D, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dIl, il, sizeof(il), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dNoise, &noise, sizeof(double), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemset(dStamp, 0, sizeof(double) * 32 * nt));
    HIP_CHECK(hipMemset(dCount, 0, sizeof(double)));
    hipStream_t st;
    if (factor_engine(device, &st, nullptr, nullptr) != 0) return -2;
    EngineShared gate(device);
    FactorWs ws;
    if (factor_ws_alloc(&ws, np) != 0) return -3;
    ws.tri_overlap = 0;
    if (kcap > 0) ws.persist_kcap = kcap;
    ws.persist_max_nt = 64;
    hipEvent_t e[2];
    ws.persist = 1;
    for (auto& ev : e) HIP_CHECK(hipEventCreate(&ev));
    const KernParams kp{MI355GP_RBF, 0, D, 1.0};
    launch_scale_inputs(st, dX, N, D, dIl, 0, dXt, np);
    for (int i = 0; i < 8 + 32 * nt; ++i) out[i] = 0.0;
    int info[4] = {0, 0, 0, 0};
    for (int mode = 0; mode < 2; ++mode) {                      // 0: launch per step into B, 1: persistent into A
        double* M = mode == 0 ? (double*)B : (double*)A;
        ws.persist = mode;
        if (mode == 1 && !potrf_persist_eligible(np, &ws)) {
            mi355gp_set_error("mi355gp_dbg_persist: N = %ld is not eligible for the persistent factorisation", (long)N);
            for (auto& ev : e) (void)hipEventDestroy(ev);
            factor_ws_free(&ws);
            return -1;
        }
        double acc = 0.0;
        for (int r = -1; r < reps; ++r) {                       // r = -1: warm-up
            launch_kbuild_sym(st, kp, dXt, np, N, np, M, dNoise, 1, 1e-8, 1, 1);
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
    for (auto& ev : e) (void)hipEventDestroy(ev);
    factor_ws_free(&ws);
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
    const int D = 4;
    std::vector<double> X((size_t)N * D);
    unsigned long long state = 0x9E3779B97F4A7C15ull;
    for (double& v : X) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        v = ((double)(state >> 11) / 9007199254740992.0 - 0.5) * 4.0;
    }
    DevBuf dX, dXt, dIl, dNoise, A, B, C;
    HIP_CHECK(dX.alloc(N * D));
    HIP_CHECK(dXt.alloc(D * np));
    HIP_CHECK(dIl.alloc(D));
    HIP_CHECK(dNoise.alloc(1));
    HIP_CHECK(A.alloc(np * np));
    HIP_CHECK(B.alloc(np * np));
    HIP_CHECK(C.alloc(np * np));
    const double il[4] = {0.7, 0.7, 0.7, 0.7}, noise = 0.1;
    HIP_CHECK(hipMemcpy(dX, X.data(), sizeof(double) * N * D, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dIl, il, sizeof(il), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(dNoise, &noise, sizeof(double), hipMemcpyHostToDevice));
    hipStream_t st;
    if (factor_engine(device, &st, nullptr, nullptr) != 0) return -2;
    FactorWs ws;
    if (factor_ws_alloc(&ws, np) != 0) return -3;
    ws.tri_overlap = 0;                                        // no CU-masked side stream inside the captured region
    ws.scratchX = B;
    ws.scratchT = C;
    const KernParams kp{MI355GP_RBF, 0, D, 1.0};
    launch_scale_inputs(st, dX, N, D, dIl, 0, dXt, np);
    auto sequence = [&]() {
        launch_kbuild_sym(st, kp, dXt, np, N, np, A, dNoise, 1, 1e-8, 1, 1);
        potrf_device(st, A, np, &ws);
        trtri_device(st, A, B, C, np, &ws);
        lauum_device(st, B, C, np, &ws);
    };
    sequence();                                                // warm-up: one-time function attributes, lazy module load
    HIP_CHECK(hipStreamSynchronize(st));
    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
    float ms;
    HIP_CHECK(hipEventRecord(e0, st));
    for (int r = 0; r < reps; ++r) sequence();
    HIP_CHECK(hipEventRecord(e1, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    out3[0] = ms / reps;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    HIP_CHECK(hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
    sequence();
    HIP_CHECK(hipStreamEndCapture(st, &graph));
    size_t nnodes = 0;
    HIP_CHECK(hipGraphGetNodes(graph, nullptr, &nnodes));
    out3[2] = (double)nnodes;
    HIP_CHECK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    HIP_CHECK(hipGraphLaunch(exec, st));                       // warm-up replay
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipEventRecord(e0, st));
    for (int r = 0; r < reps; ++r) HIP_CHECK(hipGraphLaunch(exec, st));
    HIP_CHECK(hipEventRecord(e1, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    out3[1] = ms / reps;
    (void)hipGraphExecDestroy(exec);
    (void)hipGraphDestroy(graph);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    factor_ws_free(&ws);
    HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- diagnostics ------------------------------------------------------------------------------------------
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

int mi355gp_dbg_update_rect(int device, int ntr, int ntc, const int* ks, int nk, int reps, double* out_ms);
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
