// ctx.h -- the exact-GP context (mi355gp_ctx) and the helpers of api.hip that exact.hip, predict.hip and laplace.hip share.
#pragma once
#include <string>
#include <vector>

#include "../../include/mi355gp.h"
#include "internal.h"
#include "parts.h"

struct LaplaceSession;
void laplace_session_free(LaplaceSession* s);       // laplace.hip

struct mi355gp_ctx {
    int device = 0;
    hipStream_t st = nullptr;
    long n = 0, npad = 0;
    int D = 0, Dy = 0;
    double *dX = nullptr, *dR = nullptr, *dNoise = nullptr;
    double *A = nullptr, *B = nullptr, *C = nullptr;
    FactorWs ws;
    double *dAlpha = nullptr, *dTmp = nullptr, *dTrmvPart = nullptr, *dGradPart = nullptr, *dGradOut = nullptr,
           *dScal = nullptr, *dDiag = nullptr;
    long gradPartDoubles = 0;
    hipEvent_t ev[8] = {};
    // state of the last inference call (for fetch / predict)
    bool have_factor = false, have_kernel = false;
    bool studentt = false;              // the last call was a Student-t process: dL_dK's alpha alpha^T term is scaled by dScal[4]
    // The covariance function of the last fused call as a sum of products of parts (GPy/kern/src/add.py, prod.py)
    struct Part : DevicePart {
        DevBuf dXt;                     // D x npad scaled, dimension-major inputs of this part
    };
    std::vector<Part> parts;
    Terms terms;
    double* Mbuf = nullptr;             // npad x npad product of the OTHER factors of a term (allocated on first product kernel)
    // Everything an evaluation returns -- scalars, info, per-part gradient sums, alpha, diag(dL_dK) -- lives in ONE device
    // block and travels in ONE copy into ONE pinned host block (five small pageable copies cost ~80 us per evaluation:
    // 2 % at N = 4096).  Layout (doubles): [scal 8 | grads MAXP*groups*GP_STRIDE | second records of RatQuad / StdPeriodic
    // parts MAXP*groups*GP_STRIDE | alpha N*Dy | diag N]
    // The factorisation region of an evaluation (potrf -> trtri -> alpha solve || lauum: ~110 launches on up to three streams at
    // N = 4096, every argument a fixed pointer or size of this context) replayed from ONE hipGraph for the sizes whose
    // factorisation is launch- / latency-bound (no CU-masked overlap stream below the overlapped-inverse threshold, so nothing
    // a graph node cannot carry): N = 4096 3.37 -> 3.21 ms, N = 2048 1.33 -> 1.26, N = 512 0.31 -> 0.28 (mi355gp_dbg_graph_factor).
    hipGraphExec_t fgraph = nullptr;
    int fgraph_calls = 0, fgraph_lookahead = -1, graph_enabled = 1;     // MI355GP_GRAPH=0 turns it off
    double *dPack = nullptr, *hPack = nullptr;
    size_t packDoubles = 0, offGrad = 0, offExt = 0, offAlpha = 0, offDiag = 0;
    // schedule switches set through mi355gp_set_option (INT_MIN: the process default that factor_ws_alloc read)
    int opt[MI355GP_OPT_NUM];
    double* dGradOutAll = nullptr;      // = dPack + offGrad: [part][groups][GP_STRIDE]
    // Coregionalize (kind 8) parts: the P x P partial records of the bucketed gradient (allocated with the first such part),
    // the S of every part in the result block at offCoreg ([part][256], behind diag; copied only when a kind-8 part is present),
    // and a host copy of the training output-index column last validated (hIdxCol: its input column, -1 none)
    double* dCoregPart = nullptr;
    size_t offCoreg = 0;
    std::vector<double> hIdx;
    int hIdxCol = -1;
    // Laplace session (laplace.hip): everything it needs beyond A / B / C is allocated by its first mi355gp_laplace_begin, so a
    // context that never runs one keeps its footprint; lap_stage: 0 none, 1 begun (K resident), 2 Newton step factored,
    // 3 finished (B^-1 in C), 4 gradients done (dL_dK in A).  Any exact / Student-t / given-K evaluation resets it to 0.
    // mi355gp_vargauss_forward / _backward (vargauss.hip) leave it at 3 / 4 with the session's `vg` flag set.
    LaplaceSession* lap = nullptr;
    int lap_stage = 0;
};

// api.hip
MI355GP_LOCAL void apply_options(mi355gp_ctx* c);   // (re)applies the option overrides to the factorisation workspace
MI355GP_LOCAL void drop_graph(mi355gp_ctx* c);      // forgets the captured factorisation region (the next graphable call runs plain, the one after captures)
MI355GP_LOCAL void free_data(mi355gp_ctx* c);       // everything set_data allocated, the parts, the graph and a Laplace session
int ctx_prepare_parts(mi355gp_ctx* c, int nparts, const mi355gp_part* parts);   // validates the part list, (re)builds the per-part device inputs
void ctx_scale_parts(mi355gp_ctx* c);                                            // scaled training inputs of every part, on the context's stream
Resident<mi355gp_ctx::Part> ctx_training_points(const mi355gp_ctx* c);
int ctx_coreg_check_points(const mi355gp_ctx* c, const double* Xn, int64_t M, const char* what);
bool ctx_has_point_diag(const mi355gp_ctx* c);
std::vector<double> ctx_kdiag_points(const mi355gp_ctx* c, const double* Xn, int64_t M);
// laplace.hip: mi355gp_fetch of a context whose last evaluation was a Laplace session (tmp: n x n device, row-major)
int laplace_fetch(mi355gp_ctx* c, int which, double* tmp);
