// grid_ctx.h -- the grid context (mi355gp_grid), its per-rank state (GridRank) and the transport calls of grid_comm.hip that
// the evaluation in grid.hip is written in.
#pragma once
#include <rccl/rccl.h>

#include <functional>
#include <vector>

#include "../../include/mi355gp.h"
#include "internal.h"

// Everything a rank allocates on the device is held by an owning member: a rank is reset by replacing it with a fresh one
// that keeps its identity (reset_rank, grid.hip), and is released with its context.
struct GridRank {
    int rank = 0, pr = 0, pc = 0;
    int TLr = 0, TLc = 0;            // local tile rows / cols actually owned
    long LR = 0, LC = 0;             // allocated local rows / cols (uniform over ranks)
    long nvr = 0, nvc = 0;           // local rows / cols whose global index is < n (a prefix of the local order)
    DevBuf A, X, W;
    // Panel stores (alloc_panel_stores):
    //   RPs: L_ik for the local row tiles with I > k          CPs: L_jk for the local column tiles with J > k
    //   XRs: X_kj for the local column tiles with J <= k      XRrs: X_ki for the local row tiles with I <= k
    // The L panels of a step are read only by the updates of its own group (near, part 1 on sc; bulk on st), and the
    // critical path of group g+2 starts after sc has waited for bulk(g): they live in a RING of 2 G full-height slots (panel
    // k in slot k % 2G), 2 G (N/Pr + N/Pc) nb doubles instead of ~N^2/2 (1/Pr + 1/Pc).  The X panels are also read by the
    // deferred W = X^T X on the low-priority stream, which may trail by any number of steps (all of them with GW = 0): every
    // step keeps its own, packed back to back.
    // hRP[k] .. are the panels' VIRTUAL bases (local tile l of panel k at base + l * nb * nb; only the tiles the panel holds
    // are ever addressed), dRP .. the same tables in device memory for k_grid_gemm_multi.
    DevBuf RPs, CPs, XRs, XRrs;
    long ring_slots = 0;             // L-panel ring slots the stores were sized for (2 G at allocation time)
    std::vector<double*> hRP, hCP, hXR, hXRr;
    DevArr<const double*> dRP, dCP, dXR, dXRr;
    DevBuf cpart;                    // column-reduction partials [row chunk][LC]
    DevBuf Dt, Dv, Ds;
    DevBuf bstage;                   // one-rank-per-process transports: packed tiles of a strided panel broadcast (grid_bcast_tile_runs)
    DevBuf XtR, XtC, XsR, XsC;       // scaled dimension-major / raw row-major
    DevArr<long> gR, gC;             // global index of every local row / col
    DevArr<int> dl_r, dl_c, dg;
    int ndiag = 0;
    DevBuf vloc, gvec2, alpha, ybuf, Rg;
    DevBuf scal, gradPart, gradOut, invls, noise;
    DevArr<int> info_g;
    // Log of the collectives this rank took part in during the current evaluation, per communicator (0 world, 1 process row,
    // 2 process column): count and an FNV-1a hash over (operation, root, doubles).  RCCL matches collectives by ORDER: two members
    // of a communicator that enqueue different sequences dead-lock or, worse, exchange the wrong panels.  check_seq compares
    // the logs of all members after every evaluation (mi355gp_grid_coll_log reads them).
    uint64_t coll_hash[3] = {0, 0, 0};
    long coll_count[3] = {0, 0, 0};
    DevBuf seqbuf;                   // 3 * max(world, Pr, Pc) doubles: the exchange buffer of the sequence check
    int seqbuf_members = 0;          // members it was sized for
    FactorWs ws;                     // factor_ws_alloc / factor_ws_free (set_data, reset_rank)
    hipStream_t st = nullptr;        // bulk updates and everything outside the factorisation loop
    hipStream_t sc = nullptr;        // the critical path of a step: diagonal tile, panel solves, all panel broadcasts
    hipStream_t sw = nullptr;        // W = X^T X updates
};

// loopback transport: one broadcast of an open group (an entry of the kernel arguments of k_bcast_batch)
#define BCAST_MAX_DST 8
struct BcastItem { const double* src; double* dst[BCAST_MAX_DST]; int nd; };

struct mi355gp_grid {
    int device = 0, world = 1, Pr = 1, Pc = 1, my_rank = 0;
    long nb = 512;
    bool loopback = true;
    std::vector<GridRank> ranks;     // logical ranks hosted by this process (loopback: all, RCCL: one)
    ncclComm_t comm_world = nullptr, comm_row = nullptr, comm_col = nullptr;
    hipStream_t st = nullptr;        // loopback: shared by all logical ranks
    hipStream_t sc = nullptr;        // second stream (high priority): panel factorisation + broadcasts, one step ahead
    hipStream_t sw = nullptr;        // third stream (low priority): the W = X^T X updates, which nothing waits for until the end
    hipEvent_t ev_w = nullptr;
    std::vector<hipEvent_t> ev_cr, ev_p1;   // [k]: panels of step k are in place / the part-1 updates of step k are done
    int lookahead = 1;               // MI355GP_GRID_LOOKAHEAD=0: everything in order on one stream
    int check_seq = 0;               // MI355GP_GRID_CHECK_SEQ=1: compare the collective logs of all ranks after every evaluation
    int G = 1;                       // MI355GP_GRID_G: steps per group of the two-level blocked factorisation (K = G * nb updates)
    int GW = 4;                      // MI355GP_GRID_GW: steps per W = X^T X update; 0 = one deep-K pass after the last step
    // diagnostics build, MI355GP_GRID_DBG_CRIT (WRONG RESULTS; tools/grid_crit_probe.py): 1 = every update (near / part1 / bulk /
    // W) skipped: the critical path of every step alone; 2 = ... and its broadcasts skipped; 3 = ... and only the diagonal tile
    // (its factorisation + inverse) left
    int dbg_crit = 0;
    long n = 0, npad = 0, T = 0;
    int D = 0, Dy = 0;
    hipEvent_t ev[6] = {};
    bool have_result = false;
    // Pr = Pc = 1 over the loopback transport degenerates to the dedicated single-GPU pipeline ("with Pr = Pc = 1
    // degenerate to the single-GPU path"): deep-K trtri / lauum tiles instead of three K = nb read-modify-write updates per
    // step (N=32768: 527 vs 623 ms).  MI355GP_GRID_FORCE_GENERIC=1 keeps the generic one-pass code (tests).
    mi355gp_ctx* single = nullptr;
    // loopback transport: the broadcasts of an open group, launched together at its end
    bool batching = false;
    size_t batch_count = 0;
    hipStream_t batch_stream = nullptr;
    std::vector<BcastItem> batch;
};

// ---- grid_comm.hip: the communicators and the two transports behind one set of calls -----------------------------------------
// RCCL (or its hipIpc stand-in) is bound on first use: -20 if it cannot be
int grid_comm_load();
// world communicator of rank r.rank, then the row (rank inside = pc) and column (rank inside = pr) communicators by CommSplit
int grid_comm_connect(mi355gp_grid* g, const GridRank& r, const void* id128);
void grid_comm_disconnect(mi355gp_grid* g);
// Broadcast inside one process row (group = GROUP_ROW, index = pr) or column (GROUP_COL, index = pc).
// `buf(rank, is_root)` returns the send pointer for the root and the receive pointer for everyone (the root's
// receive pointer may differ from its send pointer: out-of-place on the root, like ncclBroadcast).
enum { GROUP_ROW = 0, GROUP_COL = 1 };
typedef std::function<double*(GridRank&, bool)> BufFn;
int grid_bcast(mi355gp_grid* g, int group, int index, int root_coord, size_t count, const BufFn& buf);
// Runs of panel tiles that change hands between process rows / columns, one broadcast per (communicator, root): `n` tiles at
// local index s0 + m * ss of srcbase(root) to local index d0 + m * ds of dstbase(member)  (grid_comm.hip)
struct TileRun { int group, index, root, n; long s0, ss, d0, ds; };
typedef std::function<double*(GridRank&)> BaseFn;
int grid_bcast_tile_runs(mi355gp_grid* g, const std::vector<TileRun>& runs, size_t tile, const BaseFn& srcbase,
                         const BaseFn& dstbase);
// sum `count` doubles at `pick(rank)` over all ranks, result everywhere
int grid_allreduce(mi355gp_grid* g, size_t count, const BaseFn& pick);
// the collective logs: emptied before an evaluation, compared across the members of every communicator after it
void grid_coll_reset(mi355gp_grid* g);
int grid_check_sequences(mi355gp_grid* g);
