// sparse_ctx.h -- the sparse context (mi355gp_sparse) and the helpers of sparse.hip that svgp.hip shares with it.
#pragma once
#include <functional>
#include <vector>

#include "../../include/mi355gp.h"
#include "internal.h"
#include "parts.h"

struct LoopGroup;              // the loopback rendezvous of the row-sharded mode (sparse.hip)
struct SvgpState;              // svgp.hip
struct PepState;               // pep.hip
struct EpdtcState;             // epdtc.hip
struct MissingState;           // sparse.hip: the output groups of a fit with missing data

struct SPart : DevicePart {
    DevBuf XtZ, XtC, HX, HZ, gradNM, gradMM;   // (HX / HZ of a Linear part: mp x D, no ones column)
    // a Coregionalize part: S (P x P in COREG_REC doubles) of update_gradients_full(dL_dKnm, X, Z), summed over the chunks in
    // chunk order, and of update_gradients_full(dL_dKmm, Z); S[a][b] = the weights over rows of output a and columns of output b
    DevBuf cgNM, cgMM;
};

// a device array that grows when more is asked of it and keeps its size otherwise
struct GrowBuf {
    DevBuf b;
    size_t cap = 0;
    hipError_t need(size_t count) {
        if (count <= cap) return hipSuccess;
        DevBuf nb;
        const hipError_t e = nb.alloc(count);
        if (e != hipSuccess) return e;
        b = std::move(nb);
        cap = count;
        return hipSuccess;
    }
    operator double*() const { return b.p; }
};

struct mi355gp_sparse {
    // MI355GP_SPARSE_KMM_OVERLAP: Kmm's build + Cholesky + inverse (they need only Z) on a side stream UNDERNEATH pass 1 when the
    // factorisation is the single persistent launch (~1.2 ms of latency-bound work that otherwise runs on an idle GPU)
    int kmm_overlap = 1;
    hipStream_t st_kmm = nullptr;
    hipEvent_t ev_z = nullptr, ev_kmm = nullptr;
    int fuse_cols = 1;            // MI355GP_SPARSE_FUSE_COLS: k_grad_cols (gradient pass + column reductions in one)
    int device = 0;
    hipStream_t st = nullptr;
    long n = 0, chunk = 0;
    int D = 0, Dy = 0, splitk = 8;
    double trYYT = 0.0, trYYT_local = 0.0;
    std::vector<double> rowYY;    // host: |R_n|^2 per row (heteroscedastic log likelihood)
    // row-sharded multi-GPU mode (the reference's MPI design: var_dtc_parallel.py:121-130,387-394):
    // this rank holds n of n_global rows; psi2 / psi1Y and the pass-2 sums are all-reduced, M x M algebra is replicated
    void* comm = nullptr;         // RCCL communicator
    LoopGroup* loop = nullptr;    // or the loopback rendezvous
    int world = 1, rank = 0;
    long n_global = 0;
    double* dSvar = nullptr;      // N x D input variances (mi355gp_sparse_set_input_variance): X is then the mean of q(x_n)
    MissingState* missing = nullptr;   // mi355gp_sparse_set_output_groups: the row masks of Y's columns (forgotten by set_data)
    double* dGam = nullptr;       // N x D slab probabilities (mi355gp_sparse_set_binary_prob): q(x_n) is then spike-and-slab
    bool uncertain_result = false; // the last result came from mi355gp_vardtc_inference_uncertain (no dL_dKnm then)
    double *dX = nullptr, *dY = nullptr, *dV = nullptr, *dBeta = nullptr, *dRowS = nullptr, *dRowT = nullptr, *dRowR = nullptr,
           *Kfu = nullptr,
           *T = nullptr;
    // M-dependent
    long m = 0, mp = 0;
    double *dZ = nullptr, *zero1 = nullptr;
    double *Lm = nullptr, *Xm = nullptr, *Tm = nullptr, *psi2part = nullptr, *psi2 = nullptr, *Amat = nullptr,
           *LB = nullptr, *XB = nullptr, *Bi = nullptr, *P = nullptr, *E = nullptr, *T1 = nullptr, *Q2 = nullptr,
           *dLdKmm = nullptr, *Winv = nullptr;
    double *psi1Y = nullptr, *vecA = nullptr, *vecB = nullptr, *cvec = nullptr, *wvec = nullptr, *vvec = nullptr,
           *trmvPart = nullptr, *colPart = nullptr, *gradPart = nullptr, *gradChunk = nullptr, *scal = nullptr,
           *redbuf = nullptr;
    std::vector<SPart> parts;
    Terms terms;                  // part indices per summand, in order of first appearance (one part, or the factors of a Prod)
    FactorWs ws;
    bool ws_ok = false, have_result = false, winv_ok = false;
    hipEvent_t ev[6] = {};
    int h_info[2] = {0, 0};       // LAPACK-style info of the two M x M factorisations (targets of async copies: not on the stack)
    double predict_ms = 0.0;      // stream time of the last mi355gp_sparse_predict_uncertain call (HIP events ev[4] .. ev[5])
    double beta_scalar = 0.0;     // homoscedastic precision of the last call (0: per-point)
    KernelProf mfma_prof;         // launch timing of the two MFMA kernels of a call: family 0 = T = Kfu dL_dpsi2, 1 = split-K Gram
    // SVGP session (svgp.hip): its M x M state, and whether the context's latest result is an SVGP one (the VarDTC fetch /
    // predict entry points describe VarDTC's result and refuse then, as fetch_dLdKnm does after an uncertain-input call)
    SvgpState* svgp = nullptr;
    bool svgp_result = false;
    // PEP / FITC (pep.hip): its chunk buffers, and whether the context's latest result is a PEP one.  It lies where VarDTC's
    // does (vvec, Winv, dLdKmm, Lm), so fetch and predict serve it unchanged; dL_dKnm's rows are formed by pep.hip, psi2 and
    // dL_dpsi2 do not exist.  kmm_jitter: what the call that left the result added to Kmm's diagonal (mi355gp_sparse_fetch, Kmm).
    PepState* pep = nullptr;
    bool pep_result = false;
    double kmm_jitter = 1e-8;
    // EPDTC (epdtc.hip): Kmm, P = LLT^-1 and gamma between its begin / recompute / sweep calls, the buffers of a site block
    EpdtcState* epdtc = nullptr;
    // The per-point diagonal: diag_pt is decided by every prepare_sparse_parts -- the expression of THIS call has
    // a diag_by_point() part (Linear), Kdiag is a vector and nothing of an earlier call's is read; otherwise it is the one
    // number expression_kdiag() and no code below looks at these members.
    bool diag_pt = false;
    bool take_linear = false;     // mi355gp_sparse_set_linear: the entry points take Linear parts (off: refused by name, as before)
    // mi355gp_sparse_set_psi_lin_bias: the uncertain-input entry points take one RBF or Linear part with Bias and White parts
    // (off: Bias and Linear are refused there by name, as before).  lin_dmu (device, n x D; NULL outside such a call): where
    // sparse_rows_gradients leaves a Linear part's gradient in the rows of the chunk that starts at lin_row0, with
    // lin_c0 = 2 dL_dpsi0 on the rows' own diagonal term (k_grad_rows_lin)
    bool take_psi_lin = false;
    double* lin_dmu = nullptr;
    long lin_row0 = 0;
    double lin_c0 = 0.0;
    // ... and what those calls keep between evaluations, so that an optimiser step allocates nothing: the Linear part's row
    // gradient (n x D) and E Z (m x D); for Bias parts next to an RBF part the psi1 column sums c (mp), colsum(V) (Dy),
    // t = 2 rowsum(dL_dpsi2) and b t (m each) and the RBF part's own psi2 (mp x mp)
    GrowBuf linDmu, linEZ, biasC, biasV, biasT, biasAdd, biasPsi2;
    DiagDesc diag;
    GrowBuf diagCoef, dKd, diagW, diagPart, diagSums;   // nparts x D coefficients; Kdiag(X) (n); a family's weights (n); records
    // mi355gp_sparse_set_coregionalize (include/mi355gp_sparse_coreg.h): mi355gp_vardtc_inference_sum and mi355gp_sparse_predict
    // take Coregionalize (kind 8) parts (off: refused by name, as before).  hX: set_data's X on the host, kept while the switch
    // is on, so that a call can check the index column its Coregionalize part names (coreg_check_index) before any launch;
    // coreg_ok: the (column, P) pairs already checked against it.  cgPart / cgChunk: the block records of the bucketed pass
    // (2048 x P x P) and their sum for one chunk.
    bool take_coreg = false;
    std::vector<double> hX;
    std::vector<std::pair<int, int>> coreg_ok;
    GrowBuf cgPart, cgChunk;
};

// ---- the per-point diagonal (sparse.hip) ---------------------------------------------------------------------------
// Kdiag of `rows` row-major points (device) into kd_out (device, optional) and, with weights w (device), the record of
// weighted sums (kdiag_slots doubles) on its way into host_sums (valid after the stream is synchronised)
int sparse_kdiag(mi355gp_sparse* s, const double* X, long rows, const double* w, double* kd_out, std::vector<double>* host_sums);
// Kdiag(X) of the context's own rows into s->dKd (and the weighted sums, as above)
int sparse_kdiag_data(mi355gp_sparse* s, const double* w, std::vector<double>* host_sums);
// update_gradients_diag of every part in theta order from a record of weighted sums, times `scale` (KernGrads::ddiag)
void sparse_diag_dtheta(const mi355gp_sparse* s, const std::vector<double>& sums, double scale, std::vector<double>* out);

// ---- sparse.hip ----------------------------------------------------------------------------------------------------
// doubles of one part's theta record (one GP_STRIDE record per 32 dimensions) and of its H^T [X~ | 1] sums
inline size_t rec_doubles(const mi355gp_sparse* s) { return (size_t)((s->D + 31) / 32) * GP_STRIDE; }
inline size_t hsum_doubles(const mi355gp_sparse* s) { return (size_t)s->mp * (s->D + 1); }
struct KernGrads {             // the parts' records and sums on the host (sparse_fetch_gradients)
    bool with_nm = true;
    std::vector<double> gnm, gmm, HX, HZ, Zs;
    // per-point diagonal: update_gradients_diag of every part in theta order (sparse_diag_dtheta); empty: Kdiag is one number
    // and sparse_assemble_gradients adds kdiag_coef to the variances
    std::vector<double> ddiag;
    // the S records of the Coregionalize parts (COREG_REC doubles per part; empty: the expression has none)
    std::vector<double> cnm, cmm;
};
struct NewPoints {             // K(Z, X*) and what a prediction derives from it (sparse_newpoints)
    PointSet xs;
    DevBuf Kx, Tmp, Kss, scr, Mu, Var;
    DevBuf kdv;                // Kdiag of the new points where it depends on the point (else NULL: kdiag)
    long Mn = 0, mnp = 0;
    double kdiag = 0.0;
    double* var = nullptr;     // where sparse_newpoints_var left its result
};
bool sharded(const mi355gp_sparse* s);
int alloc_m(mi355gp_sparse* s, long M);
// coreg: the entry point evaluates Coregionalize parts (VarDTC with certain inputs and its prediction); the others refuse them
// by name even on a context that was asked
int prepare_sparse_parts(mi355gp_sparse* s, int nparts, const mi355gp_part* parts, bool coreg = false);
double sparse_other_variances(const mi355gp_sparse* s, size_t p);
bool skip_white(const mi355gp_sparse* s, const std::vector<int>& t);
void scale_for_parts(mi355gp_sparse* s, const double* src, long rows, long ldt, bool inducing);
Resident<SPart> inducing_points(const mi355gp_sparse* s);
void build_cross_chunk(mi355gp_sparse* s, long rc, double* out, double* scratch);
void build_kmm(mi355gp_sparse* s, double* out, double* scratch, double jitter, int lower_only, hipStream_t st = nullptr);
dim3 grid2d(long cols, long rows);                                                   // 256 columns a block, one row each
void launch_mm_sym(hipStream_t st, const double* low, long mp, double* out);         // out = the lower triangle mirrored
void launch_mm_axpby(hipStream_t st, const double* A, double ca, const double* B, double cb, double ci, long mp, double* out);
extern "C" {       // (defined among the entry points of sparse.hip)
int potrf_checked(hipStream_t st, double* A, double* X, double* T, double* W, long mp, FactorWs* ws, int* info_host,
                  const std::function<void()>& rebuild);
void sparse_kmm_gradients(mi355gp_sparse* s);
void missing_release(mi355gp_sparse* s);   // frees the output groups of mi355gp_sparse_set_output_groups
// the phases an inference family is built from, in the order of a call (each is described where it is defined)
int sparse_open(mi355gp_sparse* s, int nparts, const mi355gp_part* parts, int64_t M, bool coreg = false);
int sparse_start(mi355gp_sparse* s, const double* Z, const double* beta, long nbeta);
int sparse_cross_rows(mi355gp_sparse* s, long r0, long rc, long z0, long z1, const double* V);
int sparse_rows_gradients_reset(mi355gp_sparse* s);
void sparse_rows_gradients(mi355gp_sparse* s, long rc, const double* W, double* scratch, const RankTerm& rk,
                           const std::function<void()>& form_times);
int sparse_fetch_gradients(mi355gp_sparse* s, bool with_nm, KernGrads* h);
int sparse_finish(mi355gp_sparse* s, int nstage, double* stage_ms);
void sparse_assemble_gradients(const mi355gp_sparse* s, const KernGrads& h, double kdiag_coef, double* dtheta_out, double* dZ_out);
int sparse_newpoints(mi355gp_sparse* s, const double* Xnew, int64_t Mn, bool want_cov, const double* wv, int ncol,
                     const char* where, NewPoints* q);
int sparse_newpoints_var(mi355gp_sparse* s, NewPoints* q, const double* Winv, bool full_cov, bool keep_kss);
}
// the VarDTC evaluation of an opened call with the precisions and Kmm's jitter as given (mi355gp_vardtc_inference_sum, EPDTC)
int vardtc_evaluate(mi355gp_sparse* s, const double* Z, const std::vector<double>& hbeta, double (&glob)[3], double kmm_jitter,
                    double* out_scalars, double* dtheta_out, double* dZ_out, double* wv_out, double* dnoise_rows_out,
                    double* dLdm_out, double* stage_ms);
// ---- svgp.hip ------------------------------------------------------------------------------------------------------
void svgp_release(mi355gp_sparse* s);      // frees the SVGP state (M-dependent: called by free_m)
// ---- pep.hip -------------------------------------------------------------------------------------------------------
void pep_release(mi355gp_sparse* s);       // frees the PEP state (M-dependent: called by free_m)
int pep_fetch_dLdKnm(mi355gp_sparse* s, long row0, long nrows, double* out);   // the PEP half of mi355gp_sparse_fetch_dLdKnm
// ---- epdtc.hip -----------------------------------------------------------------------------------------------------
void epdtc_release(mi355gp_sparse* s);     // frees the EPDTC state (M-dependent: called by free_m)
