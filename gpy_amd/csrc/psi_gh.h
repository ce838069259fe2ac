// psi_gh.h -- launchers of the Gauss-Hermite psi-statistics kernels (psi_gh.hip) shared by the stateless entry points and the
// quadrature fit of the sparse context (sparse.hip).  Host code only; see psi_gh.hip for the formulas, the tiling and the buffer
// layouts.  The chunking (PSI_CHUNK), the split rule and the psi2 combine are psi.h's.
#pragma once
#include "psi.h"

#define GH_HMAX 32             // most quadrature nodes
#define GH_MT 64               // columns of one inducing-point tile; every M-sized operand is padded to a multiple of it
#define GH_RB 16               // rows of one row block: the k extent of four MFMAs (statistics) / their row extent (gradient)

struct GhQuad {                // nodes t_i and weights w_i on the host: tw = t[0 .. H) then w[0 .. H), the layout of GhKern::tw
    int H = 0;
    double tw[2 * GH_HMAX];
    double wsum = 0.0;         // sum_i w_i in node order
};
// validates nodes / weights / H (named in the error as `where`) and fills q
int gh_quad(const char* where, const double* nodes, const double* weights, int H, GhQuad* q);
struct GhKern {                // the part and the inducing inputs as the kernels see them
    int kind, D;               // MI355GP_RBF .. MI355GP_EXPONENTIAL; input dimensions
    double var;
    const double* il;          // device, D: 1 / l_q, 0 on a dimension the part does not see
    const double* Zt;          // device, D x mp: il_q z_mq, dimension-major, 0 in the padding
    long m, mp;                // inducing points, round_up(m, GH_MT)
    const double* tw;          // device, 2 H: the nodes, then the weights (GhQuad::tw)
    int H;
};

// Zt (D x mp) from Z (m x D row-major, device) and il
void launch_gh_zt(hipStream_t st, const double* Z, const double* il, long m, long mp, int D, double* Zt);
// psi1 (rows x m, ld ld1; optional) and the lower GH_MT tiles of the chunk's psi2 into part (nsplit x mp x mp; optional); returns
// the number of splits written (combine with launch_psi2_combine, ld = mp)
int launch_gh_stats(hipStream_t st, const GhKern& k, const double* mu, const double* S, long rows, double* psi1,
                    long ld1, double* part);
// doubles of the per-workgroup scratch the gradient kernel needs for `rows` rows (0: its row blocks live in LDS)
size_t gh_grad_scratch(long rows, long mp, int D);
// The gradient of one chunk.  G (rows x m, contiguous) or rk (G == NULL; rk.R == NULL: no dL_dpsi1) is dL_dpsi1; D2 (optional, ld ldd,
// zero outside the leading m x m up to mp) is dL_dpsi2 + dL_dpsi2^T.  Writes dmu, dS (rows x D, final), and per row
// block b: Zpart[b][q][mp] = sum W (x~_q - z~_q) (entries m.. untouched) and recpart[b][1 + D] = {sum G K, L_q}.  Returns the
// number of row blocks (sum them with launch_sum_splits).
int launch_gh_grad(hipStream_t st, const GhKern& k, const double* mu, const double* S, long rows, const double* G,
                   PsiRank rk, const double* D2, long ldd, double* scratch, double* dmu, double* dS,
                   double* Zpart, double* recpart);
