// api.hip -- the extern "C" boundary of libmi355gp.so (declared in include/mi355gp.h) for the life of an exact-GP context:
// error string, version, create / destroy / set_data / set_targets, options, fetch, and the kernel-part helpers that the
// evaluation (exact.hip), prediction (predict.hip) and the Laplace session (laplace.hip) share through ctx.h.
#include <cstdarg>
#include <cstdio>
#include <climits>
#include <string>
#include <vector>

#include "ctx.h"

static thread_local std::string g_err;

void mi355gp_set_error(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
}

// (re)applies the context's option overrides to its factorisation workspace (after every factor_ws_alloc and set_option)
void apply_options(mi355gp_ctx* c) {
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

void drop_graph(mi355gp_ctx* c) {
    if (c->fgraph) (void)hipGraphExecDestroy(c->fgraph);
    c->fgraph = nullptr;
    c->fgraph_calls = 0;
}

void free_data(mi355gp_ctx* c) {
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

// ---- the kernel parts of a context (ctx.h) -------------------------------------------------------------------------------
// validates the part list and (re)builds the per-part device inputs
int ctx_prepare_parts(mi355gp_ctx* c, int nparts, const mi355gp_part* parts) {
    ARG_CHECK(nparts >= 1 && nparts <= 16 && parts, "between 1 and 16 kernel parts");
    if ((int)c->parts.size() != nparts) {
        c->parts.clear();
        c->parts.resize((size_t)nparts);
        for (auto& p : c->parts) HIP_CHECK(p.dXt.alloc((size_t)c->D * c->npad));
    }
    for (int i = 0; i < nparts; ++i) {
        mi355gp_ctx::Part& p = c->parts[(size_t)i];
        if (int rc = parse_part(parts[i], c->D, KS_STATIONARY | KS_STATIC | KS_EXT | KS_COREG | KS_LINEAR | KS_DOT | KS_OSC, "exact-GP path", &p)) return rc;
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
void ctx_scale_parts(mi355gp_ctx* c) {
    for (auto& p : c->parts) launch_scale_inputs(c->st, c->dX, c->n, c->D, p.dIl, /*per-dimension vector*/ 1, p.dXt, c->npad);
}
// the training inputs as one side of a cross-covariance (emit_cross)
Resident<mi355gp_ctx::Part> ctx_training_points(const mi355gp_ctx* c) { return {&mi355gp_ctx::Part::dXt, c->npad, c->n}; }

// new points (M x D, host) against every Coregionalize part: their output indices must be valid
int ctx_coreg_check_points(const mi355gp_ctx* c, const double* Xn, int64_t M, const char* what) {
    for (const auto& p : c->parts)
        if (p.coreg())
            if (int rc = coreg_check_index(Xn + p.kp.col, M, c->D, p.kp.ard, what)) return rc;
    return 0;
}
// a part whose diagonal depends on the point (Coregionalize, Linear, MLP, Poly): Kdiag of the expression is then no constant
bool ctx_has_point_diag(const mi355gp_ctx* c) {
    for (const auto& p : c->parts)
        if (p.diag_by_point()) return true;
    return false;
}
// Kdiag of the expression at each new point: kd[m] = sum over terms of the product of the factors' diagonals -- B[idx_m][idx_m]
// of a Coregionalize factor (coregionalize.py:106-107), sum_q variance_q x_mq^2 over the active columns of a Linear factor
// (linear.py:84-85), var (2/pi) asin(p / (p + 1)) of an MLP factor (mlp.py:61-64), var (scale |x|^2 + bias)^order of a Poly factor
// (poly.py:33-34), the variance of any other
std::vector<double> ctx_kdiag_points(const mi355gp_ctx* c, const double* Xn, int64_t M) {
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
        const auto x = ctx_training_points(c);                                             // symmetric: no transpose needed
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

}  // extern "C"
