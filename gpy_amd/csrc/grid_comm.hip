// grid_comm.hip -- the communicators of the multi-GPU modes: the dlopen'ed RCCL entry points (or their hipIpc stand-in,
// ipc_comm.hip), the plain world communicator of the row-sharded sparse path (rccl_comm_*), and for the block-cyclic grid mode
// (grid.hip) the two transports behind one set of calls -- RCCL (one rank per process) and LOOPBACK (all Pr*Pc logical ranks in
// one process on one device, broadcasts are device copies) -- with the log of the collectives every rank took part in, its
// check, and a self-test of the bound transport.
#include <dlfcn.h>

#include <cmath>
#include <cstring>

#include "../../include/mi355gp_debug.h"
#include "grid_ctx.h"

// ---------------------------------------------------------------------------------------------------
// RCCL: types, enums and prototypes come from the installed <rccl/rccl.h>; the library itself is dlopen'ed (so the
// single-GPU library has no link-time RCCL dependency) and every entry point is bound through decltype(&ncclXxx): a
// signature change in RCCL is a compile error here, not silent ABI drift.
static_assert(sizeof(ncclUniqueId) == 128, "mi355gp_grid_unique_id hands out 128-byte ids");
// the second provider of the same entry points (ipc_comm.hip): ranks = processes sharing ONE GPU, MI355GP_TRANSPORT=ipc
ncclResult_t ipcGetUniqueId(ncclUniqueId* id);
ncclResult_t ipcCommInitRank(ncclComm_t* out, int nranks, ncclUniqueId id, int rank);
ncclResult_t ipcCommSplit(ncclComm_t parent, int color, int key, ncclComm_t* out, ncclConfig_t* cfg);
ncclResult_t ipcCommDestroy(ncclComm_t comm);
ncclResult_t ipcBroadcast(const void* send, void* recv, size_t count, ncclDataType_t type, int root, ncclComm_t comm, hipStream_t st);
ncclResult_t ipcAllReduce(const void* send, void* recv, size_t count, ncclDataType_t type, ncclRedOp_t op, ncclComm_t comm, hipStream_t st);
ncclResult_t ipcGroupStart();
ncclResult_t ipcGroupEnd();
const char* ipcGetErrorString(ncclResult_t r);

struct Rccl {
    void* h = nullptr;
    bool ipc = false;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommSplit) CommSplit = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclBroadcast) Broadcast = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    bool load() {
        if (h) return true;
        {
            const char* t = PRODUCT_ENV("TRANSPORT");
            if (t && strcmp(t, "ipc") == 0) {                // multi-process transport over hipIpc + shared memory (ipc_comm.hip)
                GetUniqueId = ipcGetUniqueId;
                CommInitRank = ipcCommInitRank;
                CommSplit = ipcCommSplit;
                CommDestroy = ipcCommDestroy;
                Broadcast = ipcBroadcast;
                AllReduce = ipcAllReduce;
                GroupStart = ipcGroupStart;
                GroupEnd = ipcGroupEnd;
                GetErrorString = ipcGetErrorString;
                ipc = true;
                h = (void*)this;
                return true;
            }
        }
        const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const char* n : names) {
            h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
            if (h) break;
        }
        if (!h) {
            mi355gp_set_error("cannot dlopen librccl.so: %s", dlerror());
            return false;
        }
#define SYM(field, name)                                                   \
    *(void**)(&field) = dlsym(h, name);                                    \
    if (!field) {                                                          \
        mi355gp_set_error("librccl.so lacks %s", name);                    \
        return false;                                                      \
    }
        SYM(GetUniqueId, "ncclGetUniqueId");
        SYM(CommInitRank, "ncclCommInitRank");
        SYM(CommSplit, "ncclCommSplit");
        SYM(CommDestroy, "ncclCommDestroy");
        SYM(Broadcast, "ncclBroadcast");
        SYM(AllReduce, "ncclAllReduce");
        SYM(GroupStart, "ncclGroupStart");
        SYM(GroupEnd, "ncclGroupEnd");
        SYM(GetErrorString, "ncclGetErrorString");
#undef SYM
        return true;
    }
};
static Rccl g_rccl;
#define NCCL_CHECK(expr)                                                                                  \
    do {                                                                                                  \
        ncclResult_t _r = (expr);                                                                         \
        if (_r != ncclSuccess) {                                                                          \
            mi355gp_set_error("%s failed: %s (%s:%d)", #expr, g_rccl.GetErrorString(_r), __FILE__, __LINE__); \
            return -(2000 + (int)_r);                                                                       \
        }                                                                                                 \
    } while (0)

// plain world communicator for the row-sharded sparse path (sparse.hip): one all-reduce per streaming pass
int rccl_comm_create(int rank, int world, const void* id128, void** comm) {
    if (!g_rccl.load()) return -20;
    ncclUniqueId id;
    memcpy(&id, id128, sizeof(id));
    ncclComm_t c = nullptr;
    NCCL_CHECK(g_rccl.CommInitRank(&c, world, id, rank));
    *comm = c;
    return 0;
}
int rccl_allreduce_sum(void* comm, double* buf, size_t count, hipStream_t st) {
    NCCL_CHECK(g_rccl.AllReduce(buf, buf, count, ncclFloat64, ncclSum, (ncclComm_t)comm, st));
    return 0;
}
void rccl_comm_destroy(void* comm) {
    if (comm && g_rccl.h) g_rccl.CommDestroy((ncclComm_t)comm);
}

// ---- the grid mode's communicators ---------------------------------------------------------------------------
int grid_comm_load() { return g_rccl.load() ? 0 : -20; }
int grid_comm_connect(mi355gp_grid* g, const GridRank& r, const void* id128) {
    ncclUniqueId id;
    memcpy(&id, id128, sizeof(id));
    NCCL_CHECK(g_rccl.CommInitRank(&g->comm_world, g->world, id, r.rank));
    NCCL_CHECK(g_rccl.CommSplit(g->comm_world, r.pr, r.pc, &g->comm_row, nullptr));   // rank inside = pc
    NCCL_CHECK(g_rccl.CommSplit(g->comm_world, r.pc, r.pr, &g->comm_col, nullptr));   // rank inside = pr
    return 0;
}
void grid_comm_disconnect(mi355gp_grid* g) {
    if (g->comm_row) g_rccl.CommDestroy(g->comm_row);
    if (g->comm_col) g_rccl.CommDestroy(g->comm_col);
    if (g->comm_world) g_rccl.CommDestroy(g->comm_world);
    g->comm_row = g->comm_col = g->comm_world = nullptr;
}

// ---- the collective log ----------------------------------------------------------------------------------------
void grid_coll_reset(mi355gp_grid* g) {
    for (GridRank& r : g->ranks)
        for (int c = 0; c < 3; ++c) {
            r.coll_hash[c] = 14695981039346656037ull;
            r.coll_count[c] = 0;
        }
}
static void coll_log(GridRank& r, int comm, int op, int root, size_t count) {
    uint64_t h = r.coll_hash[comm];
    const uint64_t words[3] = {(uint64_t)op, (uint64_t)(unsigned)root, (uint64_t)count};
    for (uint64_t w : words)
        for (int b = 0; b < 8; ++b) {
            h ^= (w >> (8 * b)) & 0xffu;
            h *= 1099511628211ull;
        }
    r.coll_hash[comm] = h;
    r.coll_count[comm] += 1;
}

// ---- transports ------------------------------------------------------------------------------------------
// loopback transport: destinations of one broadcast / the broadcasts of one group (kernel arguments of k_bcast_copy / k_bcast_batch)
#define BCAST_BATCH 24
struct BcastDst { double* p[BCAST_MAX_DST]; };
struct BcastBatch { BcastItem it[BCAST_BATCH]; };
// loopback transport: a broadcast is a device copy from the root's buffer into every other member's
__global__ __launch_bounds__(256) void k_bcast_copy(const double* __restrict__ src, BcastDst dst, int nd, long count) {
    const long n2 = count >> 1;                               // tiles and panels are 16-byte aligned and even-sized
    const d2* s2 = reinterpret_cast<const d2*>(src);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (long)gridDim.x * blockDim.x) {
        const d2 v = s2[i];
        for (int q = 0; q < nd; ++q) reinterpret_cast<d2*>(dst.p[q])[i] = v;
    }
    if ((count & 1) && blockIdx.x == 0 && threadIdx.x == 0)
        for (int q = 0; q < nd; ++q) dst.p[q][count - 1] = src[count - 1];
}
// a GROUP of loopback broadcasts (grid_group_start .. grid_group_end: the per-tile broadcasts of crit(k), up to k + 1 of them
// with different roots) as ONE launch per 24 of them instead of one per broadcast: blockIdx.y picks the broadcast
__global__ __launch_bounds__(256) void k_bcast_batch(BcastBatch b, long count) {
    const BcastItem& it = b.it[blockIdx.y];
    const long n2 = count >> 1;
    const d2* s2 = reinterpret_cast<const d2*>(it.src);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (long)gridDim.x * blockDim.x) {
        const d2 v = s2[i];
        for (int q = 0; q < it.nd; ++q) reinterpret_cast<d2*>(it.dst[q])[i] = v;
    }
    if ((count & 1) && blockIdx.x == 0 && threadIdx.x == 0)
        for (int q = 0; q < it.nd; ++q) it.dst[q][count - 1] = it.src[count - 1];
}
static void launch_bcast_copy(hipStream_t st, const double* src, const BcastDst& dst, int nd, size_t count) {
    long blocks = (long)((count / 2 + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_bcast_copy, dim3((unsigned)blocks), dim3(256), 0, st, src, dst, nd, (long)count);
}

// loopback transport: launch the broadcasts collected since grid_group_start
static int grid_flush_bcasts(mi355gp_grid* g) {
    const size_t n = g->batch.size();
    for (size_t i0 = 0; i0 < n; i0 += BCAST_BATCH) {
        BcastBatch b;
        const int m = (int)((n - i0 < BCAST_BATCH) ? n - i0 : BCAST_BATCH);
        for (int q = 0; q < m; ++q) b.it[q] = g->batch[i0 + (size_t)q];
        long blocks = (long)((g->batch_count / 2 + 255) / 256);
        if (blocks > 256) blocks = 256;
        if (blocks < 1) blocks = 1;
        hipLaunchKernelGGL(k_bcast_batch, dim3((unsigned)blocks, (unsigned)m), dim3(256), 0, g->batch_stream, b, (long)g->batch_count);
    }
    g->batch.clear();
    g->batch_count = 0;
    HIP_CHECK(hipGetLastError());
    return 0;
}
int grid_bcast(mi355gp_grid* g, int group, int index, int root_coord, size_t count, const BufFn& buf) {
    if (count == 0) return 0;
    hipStream_t lst = g->lookahead ? g->sc : g->st;            // every panel broadcast travels on the communication stream
    if (g->loopback) {
        GridRank* root = nullptr;
        for (GridRank& r : g->ranks) {
            const bool in = (group == GROUP_ROW) ? (r.pr == index) : (r.pc == index);
            const int coord = (group == GROUP_ROW) ? r.pc : r.pr;
            if (in && coord == root_coord) root = &r;
        }
        const double* src = buf(*root, true);
        if (g->batching && (g->batch_count != count || g->batch_stream != lst)) {
            if (int rc = grid_flush_bcasts(g)) return rc;      // (a group of equal-sized tiles in practice: one flush at its end)
        }
        BcastItem item;                                       // every member's copy in ONE launch (one blit per member cost the
        item.src = src;                                       // loopback run ~13,000 copy launches per evaluation at N = 32768)
        item.nd = 0;
        auto emit = [&]() {
            if (item.nd == 0) return;
            if (g->batching) {
                g->batch_count = count;
                g->batch_stream = lst;
                g->batch.push_back(item);
            } else {
                BcastDst dsts;
                for (int q = 0; q < item.nd; ++q) dsts.p[q] = item.dst[q];
                launch_bcast_copy(lst, src, dsts, item.nd, count);
            }
            item.nd = 0;
        };
        for (GridRank& r : g->ranks) {
            const bool in = (group == GROUP_ROW) ? (r.pr == index) : (r.pc == index);
            if (!in) continue;
            coll_log(r, group == GROUP_ROW ? 1 : 2, 1, root_coord, count);
            double* dst = buf(r, false);
            if (dst == src) continue;
            if (item.nd == BCAST_MAX_DST) emit();
            item.dst[item.nd++] = dst;
        }
        emit();
        return 0;
    }
    GridRank& r = g->ranks[0];
    const bool in = (group == GROUP_ROW) ? (r.pr == index) : (r.pc == index);
    if (!in) return 0;
    const int coord = (group == GROUP_ROW) ? r.pc : r.pr;
    const bool is_root = coord == root_coord;
    const double* send = is_root ? buf(r, true) : buf(r, false);
    coll_log(r, group == GROUP_ROW ? 1 : 2, 1, root_coord, count);
    NCCL_CHECK(g_rccl.Broadcast(send, buf(r, false), count, ncclFloat64, root_coord,
                                group == GROUP_ROW ? g->comm_row : g->comm_col, lst));
    return 0;
}
static int grid_group_start(mi355gp_grid* g) {
    if (!g->loopback) NCCL_CHECK(g_rccl.GroupStart());
    else g->batching = true;
    return 0;
}
static int grid_group_end(mi355gp_grid* g) {
    if (!g->loopback) {
        NCCL_CHECK(g_rccl.GroupEnd());
        return 0;
    }
    g->batching = false;
    return grid_flush_bcasts(g);
}
// ---- panel tiles that change hands between process rows / columns: ONE broadcast per (communicator, root) ----------------------
// Phases (e) and (i) of crit(k) move single tiles whose source and destination are both determined by the tile's GLOBAL index:
// tile j of a column panel lives on process row j % Pr (local tile j / Pr of the row panel there) and is wanted by process
// column j % Pc (local tile j / Pc of its column panel).  For one communicator and one root the tiles form an arithmetic
// progression in j with step lcm(Pr, Pc): a run of `n` tiles at local index s0 + m * ss on the root and d0 + m * ds on every
// member.  Rounds 2-5 sent every tile as its own broadcast inside a group (up to T - k - 1 of them per step: ~4,000 RCCL calls
// per evaluation at N = 32768); now a run travels as ONE broadcast of n tiles: packed into the staging buffer by one small kernel
// where the root's tiles are not contiguous (ss != 1), received in place where the members' are (ds == 1) and unpacked by one
// kernel where they are not.  On a Pr x Pc grid with Pr | Pc (2 x 4) a column panel needs no unpack and an X panel no pack.
// The loopback transport moves the same tiles with its batched copy kernel and LOGS the merged broadcast, so that the collective
// sequences of the two transports stay comparable (tests/test_gpu_multiproc.py).
__global__ __launch_bounds__(256) void k_tiles_restride(double* __restrict__ dst, long dstride, const double* __restrict__ src,
                                                        long sstride, long tile) {
    const d2* s2 = reinterpret_cast<const d2*>(src + (long)blockIdx.y * sstride);
    d2* q2 = reinterpret_cast<d2*>(dst + (long)blockIdx.y * dstride);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < (tile >> 1); i += (long)gridDim.x * blockDim.x) q2[i] = s2[i];
}
int grid_bcast_tile_runs(mi355gp_grid* g, const std::vector<TileRun>& runs, size_t tile, const BaseFn& srcbase,
                         const BaseFn& dstbase) {
    hipStream_t lst = g->lookahead ? g->sc : g->st;
    if (g->loopback) {
        if (int rc = grid_group_start(g)) return rc;
        for (const TileRun& tr : runs) {
            if (tr.n <= 0) continue;
            for (GridRank& r : g->ranks) {
                const bool in = (tr.group == GROUP_ROW) ? (r.pr == tr.index) : (r.pc == tr.index);
                if (in) coll_log(r, tr.group == GROUP_ROW ? 1 : 2, 1, tr.root, (size_t)tr.n * tile);
            }
            for (int m = 0; m < tr.n; ++m) {
                if (g->batch_count != tile || g->batch_stream != lst)
                    if (int rc = grid_flush_bcasts(g)) return rc;
                BcastItem item;
                item.nd = 0;
                item.src = nullptr;
                for (GridRank& r : g->ranks) {
                    const bool in = (tr.group == GROUP_ROW) ? (r.pr == tr.index) : (r.pc == tr.index);
                    const int coord = (tr.group == GROUP_ROW) ? r.pc : r.pr;
                    if (in && coord == tr.root) item.src = srcbase(r) + (tr.s0 + m * tr.ss) * (long)tile;
                }
                auto emit = [&]() {
                    if (item.nd == 0) return;
                    g->batch_count = tile;
                    g->batch_stream = lst;
                    g->batch.push_back(item);
                    item.nd = 0;
                };
                for (GridRank& r : g->ranks) {
                    const bool in = (tr.group == GROUP_ROW) ? (r.pr == tr.index) : (r.pc == tr.index);
                    if (!in) continue;
                    if (item.nd == BCAST_MAX_DST) emit();
                    item.dst[item.nd++] = dstbase(r) + (tr.d0 + m * tr.ds) * (long)tile;
                }
                emit();
            }
        }
        return grid_group_end(g);
    }
    GridRank& r = g->ranks[0];
    struct Mine { const TileRun* tr; bool is_root; const double* send; double* recv; double* stage; };
    std::vector<Mine> mine;
    long used = 0;
    for (const TileRun& tr : runs) {
        if (tr.n <= 0) continue;
        const bool in = (tr.group == GROUP_ROW) ? (r.pr == tr.index) : (r.pc == tr.index);
        if (!in) continue;
        Mine m;
        m.tr = &tr;
        m.is_root = ((tr.group == GROUP_ROW) ? r.pc : r.pr) == tr.root;
        const bool need_stage = (m.is_root && tr.ss != 1 && tr.n > 1) || (tr.ds != 1 && tr.n > 1);
        m.stage = need_stage ? r.bstage + used * (long)tile : nullptr;
        if (need_stage) used += tr.n;
        double* dst0 = dstbase(r) + tr.d0 * (long)tile;
        m.recv = (tr.ds != 1 && tr.n > 1) ? m.stage : dst0;
        m.send = m.recv;
        if (m.is_root) {
            const double* src0 = srcbase(r) + tr.s0 * (long)tile;
            if (tr.ss != 1 && tr.n > 1) {                    // pack the root's tiles
                hipLaunchKernelGGL(k_tiles_restride, dim3(64, (unsigned)tr.n), dim3(256), 0, lst, m.stage, (long)tile, src0,
                                   tr.ss * (long)tile, (long)tile);
                m.send = m.stage;
            } else {
                m.send = src0;
            }
        }
        mine.push_back(m);
    }
    if (mine.empty()) return 0;
    HIP_CHECK(hipGetLastError());
    if (mine.size() > 1) NCCL_CHECK(g_rccl.GroupStart());
    for (const Mine& m : mine) {
        coll_log(r, m.tr->group == GROUP_ROW ? 1 : 2, 1, m.tr->root, (size_t)m.tr->n * tile);
        NCCL_CHECK(g_rccl.Broadcast(m.send, m.recv, (size_t)m.tr->n * tile, ncclFloat64, m.tr->root,
                                    m.tr->group == GROUP_ROW ? g->comm_row : g->comm_col, lst));
    }
    if (mine.size() > 1) NCCL_CHECK(g_rccl.GroupEnd());
    for (const Mine& m : mine)
        if (m.tr->ds != 1 && m.tr->n > 1)                    // unpack into the members' panel
            hipLaunchKernelGGL(k_tiles_restride, dim3(64, (unsigned)m.tr->n), dim3(256), 0, lst,
                               dstbase(r) + m.tr->d0 * (long)tile, m.tr->ds * (long)tile, (const double*)m.stage, (long)tile, (long)tile);
    HIP_CHECK(hipGetLastError());
    return 0;
}
// ---- self-test of the bound transport (RCCL, or the hipIpc stand-in under MI355GP_TRANSPORT=ipc) --------------------------------
// Exactly the communicator set-up and the call patterns of the per-rank grid code, without the numerics: world communicator,
// row / column communicators by CommSplit (colour = own grid row / column, key = the other coordinate), then
//   (1) a world broadcast, (2) inside ONE group: `rounds` tile broadcasts on the row communicator with rotating roots (the
//   pattern of crit(k) step (i)), (3) the same on the column communicator (steps (d) / (f)), (4) a world all-reduce in place,
//   (5) a row-communicator all-reduce -- all on one non-default stream, every payload checked element by element.
// out4 = [mismatching doubles, checksum, rank inside the row communicator, rank inside the column communicator].
// This is the first thing to run on a node with more than one GPU (tools/rccl_first_light.sh): it separates "RCCL does not do
// what grid.hip assumes" (split numbering, several roots in one group, out-of-place broadcast on the root) from everything else.
extern "C" int mi355gp_dbg_comm_selftest(int device, const void* id128, int rank, int world, int Pr, int Pc, int64_t count,
                                         int rounds, double* out4) {
    if (!id128 || !out4 || world != Pr * Pc || count <= 0 || rounds < 1 || rank < 0 || rank >= world) {
        mi355gp_set_error("mi355gp_dbg_comm_selftest: invalid argument");
        return -1;
    }
    if (!g_rccl.load()) return -2;
    HIP_CHECK(hipSetDevice(device));
    ncclUniqueId id;
    memcpy(&id, id128, sizeof(id));
    ncclComm_t cw = nullptr, crow = nullptr, ccol = nullptr;
    NCCL_CHECK(g_rccl.CommInitRank(&cw, world, id, rank));
    const int pr = rank / Pc, pc = rank % Pc;
    NCCL_CHECK(g_rccl.CommSplit(cw, pr, pc, &crow, nullptr));
    NCCL_CHECK(g_rccl.CommSplit(cw, pc, pr, &ccol, nullptr));
    hipStream_t st;
    HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    const size_t n = (size_t)count, total = n * (size_t)(rounds + 1);
    double *dsend = nullptr, *drecv = nullptr;
    HIP_CHECK(hipMalloc(&dsend, sizeof(double) * total));
    HIP_CHECK(hipMalloc(&drecv, sizeof(double) * total));
    std::vector<double> hs(total), hr(total);
    double bad = 0.0, sum = 0.0;
    auto val = [](double tag, size_t i) { return tag + 1e-3 * (double)(i % 1000); };
    auto fill = [&](int slot, double tag) {
        for (size_t i = 0; i < n; ++i) hs[(size_t)slot * n + i] = val(tag, i);
    };
    auto upload = [&]() -> int {
        HIP_CHECK(hipMemcpyAsync(dsend, hs.data(), sizeof(double) * total, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemsetAsync(drecv, 0, sizeof(double) * total, st));
        return 0;
    };
    auto download = [&]() -> int {
        HIP_CHECK(hipMemcpyAsync(hr.data(), drecv, sizeof(double) * total, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        return 0;
    };
    auto expect = [&](int slot, double tag) {
        for (size_t i = 0; i < n; ++i) {
            const double got = hr[(size_t)slot * n + i];
            if (got != val(tag, i)) bad += 1.0;
            sum += got;
        }
    };
    // (1) world broadcast from the last rank, out of place everywhere (the root included, as grid_bcast does it)
    fill(0, 100.0 + rank);
    if (int rc = upload()) return rc;
    NCCL_CHECK(g_rccl.Broadcast(dsend, drecv, n, ncclFloat64, world - 1, cw, st));
    if (int rc = download()) return rc;
    expect(0, 100.0 + (world - 1));
    // (2) / (3): one GROUP of `rounds` broadcasts with rotating roots on the row, then on the column communicator
    for (int which = 0; which < 2; ++which) {
        const int size = which == 0 ? Pc : Pr, me = which == 0 ? pc : pr, line = which == 0 ? pr : pc;
        const ncclComm_t comm = which == 0 ? crow : ccol;
        for (int q = 0; q < rounds; ++q) fill(q, 1000.0 * (which + 1) + 10.0 * line + me + 0.25 * q);
        if (int rc = upload()) return rc;
        NCCL_CHECK(g_rccl.GroupStart());
        for (int q = 0; q < rounds; ++q)
            NCCL_CHECK(g_rccl.Broadcast(dsend + (size_t)q * n, drecv + (size_t)q * n, n, ncclFloat64, q % size, comm, st));
        NCCL_CHECK(g_rccl.GroupEnd());
        if (int rc = download()) return rc;
        for (int q = 0; q < rounds; ++q) expect(q, 1000.0 * (which + 1) + 10.0 * line + (q % size) + 0.25 * q);
    }
    // (4) world all-reduce in place: sum over ranks of (rank + pattern)
    fill(0, (double)rank);
    if (int rc = upload()) return rc;
    NCCL_CHECK(g_rccl.AllReduce(dsend, dsend, n, ncclFloat64, ncclSum, cw, st));
    HIP_CHECK(hipMemcpyAsync(hr.data(), dsend, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    for (size_t i = 0; i < n; ++i) {
        double want = 0.0;
        for (int r = 0; r < world; ++r) want += val((double)r, i);          // rank order = the order the loopback transport sums in
        if (fabs(hr[i] - want) > 1e-9 * fabs(want) + 1e-12) bad += 1.0;
        sum += hr[i];
    }
    // (5) row all-reduce out of place
    fill(0, 10.0 * rank);
    if (int rc = upload()) return rc;
    NCCL_CHECK(g_rccl.AllReduce(dsend, drecv, n, ncclFloat64, ncclSum, crow, st));
    if (int rc = download()) return rc;
    for (size_t i = 0; i < n; ++i) {
        double want = 0.0;
        for (int c = 0; c < Pc; ++c) want += val(10.0 * (pr * Pc + c), i);
        if (fabs(hr[i] - want) > 1e-9 * fabs(want) + 1e-12) bad += 1.0;
        sum += hr[i];
    }
    out4[0] = bad;
    out4[1] = sum;
    out4[2] = (double)pc;                                          // key of the row split = grid column: must be the rank inside crow
    out4[3] = (double)pr;
    (void)hipFree(dsend);
    (void)hipFree(drecv);
    (void)hipStreamDestroy(st);
    NCCL_CHECK(g_rccl.CommDestroy(crow));
    NCCL_CHECK(g_rccl.CommDestroy(ccol));
    NCCL_CHECK(g_rccl.CommDestroy(cw));
    return 0;
}

__global__ void k_grid_axpy(double* __restrict__ dst, const double* __restrict__ src, long cnt) {
    const long l = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (l < cnt) dst[l] += src[l];
}
// sum `count` doubles at `pick(rank)` over all ranks, result everywhere
int grid_allreduce(mi355gp_grid* g, size_t count, const BaseFn& pick) {
    for (GridRank& r : g->ranks) coll_log(r, 0, 2, 0, count);
    if (g->loopback) {
        double* acc = pick(g->ranks[0]);
        const unsigned nblk = (unsigned)((count + 255) / 256);
        for (size_t i = 1; i < g->ranks.size(); ++i)
            hipLaunchKernelGGL(k_grid_axpy, dim3(nblk), dim3(256), 0, g->st, acc, pick(g->ranks[i]), (long)count);
        for (size_t i = 1; i < g->ranks.size(); ++i)
            HIP_CHECK(hipMemcpyAsync(pick(g->ranks[i]), acc, count * sizeof(double), hipMemcpyDeviceToDevice, g->st));
        return 0;
    }
    GridRank& r = g->ranks[0];
    NCCL_CHECK(g_rccl.AllReduce(pick(r), pick(r), count, ncclFloat64, ncclSum, g->comm_world, r.st));
    return 0;
}

// Debug mode (MI355GP_GRID_CHECK_SEQ=1 / MI355GP_GRID_OPT_CHECK_SEQ): after an evaluation, every member of a communicator must
// have logged the SAME sequence of collectives on it.  Loopback: the logical ranks are compared on the host.  One rank per
// process: every member contributes (hash high, hash low, count) at its own position of a vector that is sum-all-reduced inside
// the communicator (the three numbers are integers below 2^32: exact in fp64), then compares all positions with its own.
int grid_check_sequences(mi355gp_grid* g) {
    if (g->loopback) {
        for (const GridRank& a : g->ranks)
            for (const GridRank& b : g->ranks) {
                const bool same[3] = {true, a.pr == b.pr, a.pc == b.pc};
                for (int c = 0; c < 3; ++c)
                    if (same[c] && (a.coll_hash[c] != b.coll_hash[c] || a.coll_count[c] != b.coll_count[c])) {
                        mi355gp_set_error("grid mode: ranks %d and %d logged different collective sequences on communicator %d "
                                          "(%ld vs %ld collectives)", a.rank, b.rank, c, a.coll_count[c], b.coll_count[c]);
                        return -7;
                    }
            }
        return 0;
    }
    GridRank& r = g->ranks[0];
    const ncclComm_t comms[3] = {g->comm_world, g->comm_row, g->comm_col};
    const int sizes[3] = {g->world, g->Pc, g->Pr}, me[3] = {r.rank, r.pc, r.pr};
    if (r.seqbuf_members < g->world) {                      // world >= Pr, Pc: one buffer serves the three communicators
        r.seqbuf = DevBuf();
        HIP_CHECK(r.seqbuf.alloc(3 * (size_t)g->world));
        r.seqbuf_members = g->world;
    }
    const uint64_t hash[3] = {r.coll_hash[0], r.coll_hash[1], r.coll_hash[2]};       // before the check's own collectives
    const long cnt[3] = {r.coll_count[0], r.coll_count[1], r.coll_count[2]};
    for (int c = 0; c < 3; ++c) {
        std::vector<double> v((size_t)3 * sizes[c], 0.0);
        v[(size_t)3 * me[c]] = (double)(hash[c] >> 32);
        v[(size_t)3 * me[c] + 1] = (double)(hash[c] & 0xffffffffull);
        v[(size_t)3 * me[c] + 2] = (double)cnt[c];
        HIP_CHECK(hipMemcpyAsync(r.seqbuf, v.data(), sizeof(double) * v.size(), hipMemcpyHostToDevice, r.st));
        NCCL_CHECK(g_rccl.AllReduce(r.seqbuf, r.seqbuf, v.size(), ncclFloat64, ncclSum, comms[c], r.st));
        HIP_CHECK(hipMemcpyAsync(v.data(), r.seqbuf, sizeof(double) * v.size(), hipMemcpyDeviceToHost, r.st));
        HIP_CHECK(hipStreamSynchronize(r.st));
        for (int m = 0; m < sizes[c]; ++m)
            for (int q = 0; q < 3; ++q)
                if (v[(size_t)3 * m + q] != v[(size_t)3 * me[c] + q]) {
                    mi355gp_set_error("grid mode: rank %d and member %d of communicator %d logged different collective sequences "
                                      "(%.0f vs %ld collectives)", r.rank, m, c, v[(size_t)3 * m + 2], cnt[c]);
                    return -7;
                }
    }
    return 0;
}

extern "C" {

int mi355gp_grid_unique_id(void* id128) {
    ARG_CHECK(id128 != nullptr, "mi355gp_grid_unique_id: NULL");
    if (!g_rccl.load()) return -20;
    ncclUniqueId id;
    NCCL_CHECK(g_rccl.GetUniqueId(&id));
    memcpy(id128, &id, sizeof(id));
    return 0;
}

// Collective log of logical rank `rank` of this process (loopback: any rank of the grid; one rank per process: its own, rank is
// ignored) for the LAST evaluation: out9 = [count world, row, column, then per communicator the hash as (high 32 bits, low 32 bits)].
int mi355gp_grid_coll_log(mi355gp_grid* g, int rank, double* out9) {
    ARG_CHECK(g && out9 && !g->single, "mi355gp_grid_coll_log: not available on the degenerate 1 x 1 grid");
    const GridRank* r = &g->ranks[0];
    if (g->loopback) {
        ARG_CHECK(rank >= 0 && rank < (int)g->ranks.size(), "mi355gp_grid_coll_log: bad rank");
        r = &g->ranks[(size_t)rank];
    }
    for (int c = 0; c < 3; ++c) {
        out9[c] = (double)r->coll_count[c];
        out9[3 + 2 * c] = (double)(r->coll_hash[c] >> 32);
        out9[4 + 2 * c] = (double)(r->coll_hash[c] & 0xffffffffull);
    }
    return 0;
}
}  // extern "C"
