// exact.hip -- one exact-GP objective + gradient evaluation with everything N x N resident in HBM, built from named phases
// ("The phases of an exact-GP evaluation"), and the entry points that run it: mi355gp_exact_inference[_sum],
// mi355gp_exact_studentt_sum, mi355gp_inference_given_K.
#include <cmath>
#include <cstring>
#include <functional>

#include "ctx.h"

#define LOG_2_PI 1.8378770664093454836

// What one evaluation was asked for.  Ky (lower) is in c->A when it starts.
struct Evaluation {
    bool with_kernel_grads;
    double nu;                          // > 0: Student-t process with nu degrees of freedom
    double *out_scalars, *alpha_out, *dtheta_out, *diag_out, *stage_ms;
    std::function<int()> rebuild;       // re-enqueues the construction of Ky in c->A (only after a DIRTY abort of the persistent factorisation)
    size_t nparts(const mi355gp_ctx* c) const { return with_kernel_grads ? c->parts.size() : 0; }
};

// The factorisation region: potrf -> trtri -> (alpha solve on the side stream) || lauum.  `timing`: record the stage events.
static int enqueue_factor_region(mi355gp_ctx* c, bool timing) {
    hipStream_t st = c->st;
    const long n = c->n, np = c->npad;
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
}

// The graph policy of the region.  hipGraph replay when nothing in the region needs a CU-masked stream (sizes below the
// overlapped-inverse threshold), no stage timing was asked for and launch bracketing is off; the first evaluation of a context
// runs plain (one-time function attributes), the second captures, every later one replays.  *graphable: this call was one of those.
static int run_factor_region(mi355gp_ctx* c, EngineShared* gate, const Evaluation& ev, bool* graphable) {
    hipStream_t st = c->st;
    const long np = c->npad;
    const bool structural = c->graph_enabled && !c->ws.prof.on && c->ws.lookahead == 1 && c->ws.persist_skip == 0 &&
                            (!c->ws.tri_overlap || (int)(np / NB) < c->ws.tri_min_nt) && persist_early_h(np, &c->ws) == 0 &&
                            c->ws.sched_state != 1;           // (the calibration's evaluation on launches is timed: plain launches)
    if (c->fgraph && !structural) drop_graph(c);
    *graphable = structural && !ev.stage_ms;                  // a call that wants the stage timings runs plain, the graph stays
    if (!*graphable) return enqueue_factor_region(c, true);
    if (c->fgraph) {
        HIP_CHECK(hipGraphLaunch(c->fgraph, st));
        return 0;
    }
    if (c->fgraph_calls++ == 0) return enqueue_factor_region(c, false);
    // The capture runs on the device's SHARED streams: while it is open, a launch that another host thread makes on
    // them would be recorded into this graph instead of executed.  Entry points hold the engine gate shared;
    // the capture window takes it exclusively (nothing inside the window waits for another thread).
    if (!gate->try_exclusive()) {                             // another thread is inside an entry point: capture next time
        --c->fgraph_calls;
        return enqueue_factor_region(c, false);
    }
    hipGraph_t g = nullptr;
    bool ok = hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed) == hipSuccess;
    if (ok) {
        const int rc = enqueue_factor_region(c, false);
        ok = (hipStreamEndCapture(st, &g) == hipSuccess) && rc == 0 && g != nullptr;
    }
    gate->share();
    if (ok) ok = hipGraphInstantiate(&c->fgraph, g, nullptr, nullptr, 0) == hipSuccess;
    if (g) (void)hipGraphDestroy(g);
    if (!ok) {                                                // capture not possible here: stay on plain launches
        (void)hipGetLastError();
        c->fgraph = nullptr;
        c->graph_enabled = 0;
        return enqueue_factor_region(c, false);
    }
    c->fgraph_lookahead = c->ws.lookahead;
    HIP_CHECK(hipGraphLaunch(c->fgraph, st));
    return 0;
}

// datafit, |alpha|^2, tr W, logdet, info and diag(dL_dK) into the result block [, the Student-t factor on alpha alpha^T]
static int enqueue_scalars(mi355gp_ctx* c, const Evaluation& ev) {
    hipStream_t st = c->st;
    launch_scalars(st, c->dAlpha, c->dR, c->C, c->npad, c->n, c->Dy, c->ws.logsum, c->ws.nblk, c->dScal, c->dDiag, c->ws.info);
    if (ev.nu > 0.0) launch_studentt_scale(st, c->dScal, ev.nu, c->n, c->dScal + 4);
    HIP_CHECK(hipEventRecord(c->ev[5], st));
    return 0;
}

// every part reduces the same dL_dK against its own dK/dtheta, into its records of the result block
static int enqueue_part_gradients(mi355gp_ctx* c, const Evaluation& ev) {
    hipStream_t st = c->st;
    const long n = c->n, np = c->npad;
    const int groups = (c->D + 31) / 32;
    const size_t nparts = ev.nparts(c);
    const double* aa_scale = ev.nu > 0.0 ? c->dScal + 4 : nullptr;
    if (nparts > 0) {
        HIP_CHECK(hipMemsetAsync(c->dGradOutAll, 0, sizeof(double) * nparts * groups * GP_STRIDE, st));
        HIP_CHECK(hipMemsetAsync(c->dPack + c->offExt, 0, sizeof(double) * nparts * groups * GP_STRIDE, st));
        const int nb = grad_num_blocks(n);
        for (size_t p = 0; p < nparts; ++p) {
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
                                                  c->dCoregPart, aa_scale, Mul, np);
                launch_reduce_partials(st, c->dCoregPart, nbc, P * P, c->dPack + c->offCoreg + p * COREG_REC);
                continue;
            }
            launch_grad_fused(st, pt.kp, pt.dXt, np, n, c->C, np, c->dAlpha, c->Dy, c->dGradPart, aa_scale, Mul, np);
            for (int r = 0; r < (pt.ext() ? 2 : 1); ++r)                   // r = 1: the second record of RatQuad / StdPeriodic (k_grad_ext)
                for (int g = 0; g < (pt.kp.ard ? groups : 1); ++g)
                    launch_reduce_partials(st, c->dGradPart + ((long)r * groups + g) * nb * GP_STRIDE, nb, GP_STRIDE,
                                           (r ? c->dPack + c->offExt : c->dGradOutAll) + ((long)p * groups + g) * GP_STRIDE);
        }
    }
    HIP_CHECK(hipEventRecord(c->ev[6], st));
    return 0;
}

// ONE device -> pinned host copy of the prefix of the result block that the caller asked for, then the stream drains.
// *info: written by k_scalars from the factorisation's info word.
static int fetch_results(mi355gp_ctx* c, const Evaluation& ev, int* info) {
    bool coreg = false;
    for (size_t p = 0; p < ev.nparts(c); ++p) coreg = coreg || c->parts[p].coreg();
    const size_t ncopy = coreg ? c->packDoubles : (ev.diag_out ? c->offCoreg : (ev.alpha_out ? c->offDiag : c->offAlpha));
    HIP_CHECK(hipMemcpyAsync(c->hPack, c->dPack, sizeof(double) * ncopy, hipMemcpyDeviceToHost, c->st));
    HIP_CHECK(hipStreamSynchronize(c->st));
    HIP_CHECK(hipGetLastError());
    *info = (int)c->hPack[6];
    if (ev.alpha_out) memcpy(ev.alpha_out, c->hPack + c->offAlpha, sizeof(double) * c->n * c->Dy);
    if (ev.diag_out) memcpy(ev.diag_out, c->hPack + c->offDiag, sizeof(double) * c->n);
    return 0;
}

// device time between the stage events ev[0..6] of a plain (timed) evaluation
static int read_stage_ms(mi355gp_ctx* c, double* stage_ms) {
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
    return 0;
}

// After the stream has drained: what the factorisation's info word means for this evaluation.  FACTOR_FAILED: *rc is what the
// entry point returns (LAPACK info > 0, or -6 with the error string set).  FACTOR_REDO_DIRTY: Ky has to be rebuilt first.
enum FactorOutcome { FACTOR_OK, FACTOR_REDO, FACTOR_REDO_DIRTY, FACTOR_FAILED };
static FactorOutcome factor_outcome(mi355gp_ctx* c, int info, int attempt, bool can_rebuild, int* rc) {
    bool clean = false;
    if (potrf_persist_aborted(info, &c->ws, &clean)) {
        // The persistent factorisation did not run: called off at its co-residency gate (something else held CUs: the matrix
        // is untouched) or, never seen in a sane run, aborted on a wait timeout (the matrix is rebuilt).  Redo the evaluation
        // here with the launch-per-step schedule (same bits); the caller never sees it, the jitter ladder never hears of it.
        c->have_factor = false;
        drop_graph(c);
        if (attempt == 0 && (clean || can_rebuild)) return clean ? FACTOR_REDO : FACTOR_REDO_DIRTY;
        mi355gp_set_error("the persistent factorisation aborted and could not be redone (info %d); this context continues "
                          "with the launch-per-step schedule -- repeat the call", info);
        *rc = -6;
        return FACTOR_FAILED;
    }
    if (info > 0) {
        c->have_factor = false;
        if (c->ws.sched_state == 1) {                          // a calibration in progress does not survive a failed evaluation:
            c->ws.sched_state = c->ws.sched_force_steps = 0;   // start over (it used to stay in state 1 for good: no graph
            c->ws.sched_np = c->ws.sched_ns = 0;               // replay, never decided -- ADVICE r5)
        }
        *rc = info > c->n ? (int)c->n : info;
        return FACTOR_FAILED;
    }
    return FACTOR_OK;
}

// the Gaussian scalars, then the Student-t overrides, then dtheta per part, concatenated in part order
static void write_scalars(const mi355gp_ctx* c, const Evaluation& ev) {
    const long n = c->n;
    const double* scal = c->hPack;
    double* out_scalars = ev.out_scalars;
    const double datafit = scal[0], alpha2 = scal[1], trw = scal[2], logdet = scal[3];
    const double Dy = (double)c->Dy;
    for (int i = 0; i < MI355GP_NUM_OUT; ++i) out_scalars[i] = 0.0;
    out_scalars[MI355GP_OUT_LML] = 0.5 * (-(double)n * Dy * LOG_2_PI - Dy * logdet - datafit);
    out_scalars[MI355GP_OUT_LOGDET] = logdet;
    out_scalars[MI355GP_OUT_DATAFIT] = datafit;
    out_scalars[MI355GP_OUT_DNOISE] = 0.5 * (alpha2 - Dy * trw);
    out_scalars[MI355GP_OUT_TRKINV] = trw;
    if (ev.nu > 0.0) {
        // Student-t process (exact_studentt_inference.py:36-52): beta = sum(alpha * R)
        const double nu = ev.nu, N = (double)n, beta = datafit;
        out_scalars[MI355GP_OUT_LML] = 0.5 * (-N * log((nu - 2.0) * M_PI) - logdet - (nu + N) * log(1.0 + beta / (nu - 2.0))) +
                                       lgamma(0.5 * (nu + N)) - lgamma(0.5 * nu);
        out_scalars[5] = (nu + N) / (nu + beta - 2.0);                       // factor of dL_dm = factor * alpha
        out_scalars[MI355GP_OUT_DNOISE] = 0.0;
    }
    if (ev.nparts(c) > 0 && ev.dtheta_out) {
        const size_t rec_len = (size_t)((c->D + 31) / 32) * GP_STRIDE;
        double* o = ev.dtheta_out;
        for (size_t p = 0; p < ev.nparts(c); ++p) {
            const double* rec = c->parts[p].coreg() ? c->hPack + c->offCoreg + p * COREG_REC : c->hPack + c->offGrad + p * rec_len;
            o += part_dtheta(c->parts[p], rec, c->hPack + c->offExt + p * rec_len, o);
        }
    }
}

// Shared tail: given Ky (lower) in c->A: factor, invert, alpha, scalars [, kernel gradients].  At most two attempts: the second
// redoes an evaluation whose persistent factorisation was called off, on the launch-per-step schedule.
static int evaluate(mi355gp_ctx* c, EngineShared* gate, const Evaluation& ev) {
    for (int attempt = 0;; ++attempt) {
        c->lap_stage = 0;                                        // A / B / C are this evaluation's from here on
        c->ws.prof.reset();
        c->ws.scratchX = c->B;                                   // free until trtri / lauum overwrite them
        c->ws.scratchT = c->C;
        bool graphable = false;
        if (int rc = run_factor_region(c, gate, ev, &graphable)) return rc;
        if (int rc = enqueue_scalars(c, ev)) return rc;
        if (int rc = enqueue_part_gradients(c, ev)) return rc;
        int info = 0, failed = 0;
        if (int rc = fetch_results(c, ev, &info)) return rc;
        if (ev.stage_ms)
            if (int rc = read_stage_ms(c, ev.stage_ms)) return rc;
        const FactorOutcome what = factor_outcome(c, info, attempt, (bool)ev.rebuild, &failed);
        if (what == FACTOR_FAILED) return failed;
        if (what == FACTOR_REDO_DIRTY)
            if (int rc = ev.rebuild()) return rc;
        if (what != FACTOR_OK) continue;                         // redo: on the launch-per-step schedule, same bits
        c->have_factor = true;
        c->studentt = ev.nu > 0.0;
        // schedule of a small factorisation by measurement (FactorWs::persist_auto): potrf .. lauum of this evaluation, device time
        FactorWs& w = c->ws;
        const int nt = (int)(c->npad / NB);
        if (w.persist_auto && w.sched_state < 2 && !graphable && attempt == 0 && nt >= w.persist_tri_min_nt) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, c->ev[1], c->ev[4]) == hipSuccess) calibrate_schedule(w, ms, nt);
            else (void)hipGetLastError();
        }
        write_scalars(c, ev);
        return 0;
    }
}

static int upload_noise(mi355gp_ctx* c, const double* noise, int64_t noise_len) {
    ARG_CHECK(noise != nullptr && (noise_len == 1 || noise_len == c->n),
              "noise must have 1 or N entries");
    HIP_CHECK(hipMemcpyAsync(c->dNoise, noise, sizeof(double) * noise_len, hipMemcpyHostToDevice, c->st));
    return 0;
}

// The body of the Gaussian (nu = 0) and Student-t process (nu > 2) entry points: Ky = sum_t prod_f K_f + (noise + jitter) I
// (add.py:58-72, prod.py:58-65), then the evaluation.
static int exact_sum(mi355gp_ctx* c, int nparts, const mi355gp_part* parts, const double* noise, int64_t noise_len, double jitter,
                     double nu, double* out_scalars, double* alpha_out, double* dtheta_out, double* diag_out, double* stage_ms) {
    HIP_CHECK(hipSetDevice(c->device));
    EngineShared gate(c->device);
    if (int rc = ctx_prepare_parts(c, nparts, parts)) return rc;
    if (int rc = upload_noise(c, noise, noise_len)) return rc;
    hipStream_t st = c->st;
    c->have_kernel = true;
    HIP_CHECK(hipEventRecord(c->ev[0], st));
    ctx_scale_parts(c);
    auto build = [&]() -> int {
        emit_expression(c->terms, c->A, c->Mbuf, false, [&](int p, double* dst, const double* mul, int acc, bool first) {
            launch_kbuild_sym(st, c->parts[(size_t)p].kp, c->parts[(size_t)p].dXt, c->npad, c->n, c->npad, dst, c->dNoise,
                              noise_len, jitter, /*lower_only=*/1, /*add_diag=*/first, acc, mul);
        });
        return 0;
    };
    build();
    return evaluate(c, &gate, Evaluation{true, nu, out_scalars, alpha_out, dtheta_out, diag_out, stage_ms, build});
}

extern "C" {

int mi355gp_exact_inference_sum(mi355gp_ctx* c, int nparts, const mi355gp_part* parts, const double* noise,
                                int64_t noise_len, double jitter, double extra_jitter, double* out_scalars,
                                double* alpha_out, double* dtheta_out, double* diag_dLdK_out, double* stage_ms) {
    ARG_CHECK(c && c->n > 0, "mi355gp_exact_inference: set_data first");
    ARG_CHECK(out_scalars != nullptr, "out_scalars is NULL");
    return exact_sum(c, nparts, parts, noise, noise_len, jitter + extra_jitter, 0.0, out_scalars, alpha_out, dtheta_out,
                     diag_dLdK_out, stage_ms);
}

// Student-t PROCESS inference (ExactStudentTInference.inference, exact_studentt_inference.py:20-52): the same pdinv +
// dpotrs skeleton with Ky = K + 1e-8 I and dL_dK = 0.5 ((nu+N)/(nu+beta-2) alpha alpha^T - Dy Ky^-1).
// out_scalars: LML (Student-t), LOGDET, DATAFIT (= beta), [5] = (nu+N)/(nu+beta-2); dL_dnu is O(1) host arithmetic on beta.
int mi355gp_exact_studentt_sum(mi355gp_ctx* c, int nparts, const mi355gp_part* parts, double nu, double jitter,
                               double extra_jitter, double* out_scalars, double* alpha_out, double* dtheta_out,
                               double* stage_ms) {
    ARG_CHECK(c && c->n > 0, "mi355gp_exact_studentt_sum: set_data first");
    ARG_CHECK(out_scalars != nullptr && nu > 2.0, "mi355gp_exact_studentt_sum: nu must exceed 2");
    const double zero = 0.0;
    return exact_sum(c, nparts, parts, &zero, 1, jitter + extra_jitter, nu, out_scalars, alpha_out, dtheta_out, nullptr, stage_ms);
}

int mi355gp_exact_inference(mi355gp_ctx* c, int kind, int ard, const double* theta, const double* noise,
                            int64_t noise_len, double jitter, double extra_jitter, double* out_scalars,
                            double* alpha_out, double* dtheta_out, double* diag_dLdK_out, double* stage_ms) {
    if (int rc = check_kind(kind, KS_STATIONARY | KS_EXT | KS_LINEAR | KS_DOT | KS_OSC, "mi355gp_exact_inference")) return rc;
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
    return evaluate(c, &gate, Evaluation{false, 0.0, out_scalars, alpha_out, nullptr, diag_dLdK_out, stage_ms, build});
}

}  // extern "C"
