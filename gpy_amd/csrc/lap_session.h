// lap_session.h -- the state of one Laplace session (laplace.hip) and the helpers that the EP calls (ep.hip) share with it.
#pragma once
#include <vector>

#include "ctx.h"

struct LaplaceSession {
    double* K = nullptr;            // npad x npad, symmetric, no noise, no jitter, exact Kdiag on the diagonal
    FactorWs ws;
    bool ws_ok = false;
    double* vec = nullptr;          // NVEC device vectors of npad doubles + 8 scalars
    double* part = nullptr;         // partials of launch_symv_lower
    double* coregPart = nullptr;    // 2048 P x P records of the unfused Coregionalize reduction (first kind-8 part)
    std::vector<double> host;       // staging of the small results
    bool ep_sigma = false;          // the context's A holds EP's Sigma and LV_KA its mu (mi355gp_ep_recompute with want_sigma)
    // VarGauss (vargauss.hip): the last factorisation was mi355gp_vargauss_forward's, so LV_SW holds the SIGNED beta and X is
    // the inverse factor of I + diag(beta) K diag(beta); vg_ai: the context's C holds Ai (lower tiles); vg_bwd: backward ran
    bool vg = false, vg_ai = false, vg_bwd = false;
    double* vgPart = nullptr;       // column / row partials of k_vg_assemble (vg_part_doubles)
};
enum { LV_W = 0, LV_SW, LV_B, LV_A, LV_KA, LV_T0, LV_T1, LV_T2, LV_KD, LV_DIAG, LV_U, LV_S, LV_NUM };

static inline double* lvec(const mi355gp_ctx* c, int which) { return c->lap->vec + (size_t)which * c->npad; }
static inline double* lscal(const mi355gp_ctx* c) { return c->lap->vec + (size_t)LV_NUM * c->npad; }

// laplace.hip
int lap_check_W(const double* W, long n, const char* where);
int lap_check_vec(const double* v, long n, const char* where, const char* name);
// W (device, LV_W) -> sw, B into A, L_B in place, X = L_B^-1 into the context's B buffer; all enqueued, nothing read back
void lap_enqueue_factor(mi355gp_ctx* c, double jit);
// the same from sw (device, LV_SW) on: what lap_enqueue_factor enqueues after its square root
void lap_enqueue_factor_sw(mi355gp_ctx* c, double jit);
// t = B^-1 r = X^T (X r)
void lap_enqueue_Binv(mi355gp_ctx* c, const double* r, double* t);
// after the stream has drained: 1 = redo (persistent launch called off), 0 = go on (*info_out: LAPACK info), < 0 error
int lap_factor_outcome(mi355gp_ctx* c, int info, int attempt, int* info_out);
// every part's dL/dtheta from the dL_dK resident in the context's A (both triangles), concatenated into dtheta_out; drains the stream
int lap_reduce_dtheta(mi355gp_ctx* c, double* dtheta_out);
