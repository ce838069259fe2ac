"""What tests/test_oracle_sparse_shard.py (CPU) and tests/test_gpu_sparse_sharded.py (GPU) share: the row-sharded sparse (VarDTC)
path -- one context per rank, each with a slice of the rows, meeting at the all-reduces of csrc/sparse.hip -- driven over the
in-process loopback transport and put back together, so that tests/sparse_ld.py can judge it as it judges the unsharded context.
A sharded evaluation must return what the unsharded one returns: the reference is sparse_ld.reference(name), unchanged.

    splits(N, rows)            per-rank row counts -> [(lo, hi)]; an int: that many ranks by gpy_amd.grid.shard_rows
    run_ranks(world, fn)       fn(rank) on one host thread per rank -> the per-rank results
    rank_outputs(ctx, c, lo, hi)   one evaluation of a rank that holds rows [lo, hi): everything the judge names
    evaluate_sharded(case, rows)   a fresh group of fresh contexts over the loopback transport -> (per-rank outputs, spans)
    assemble(per_rank, spans, block)   the global form: row-indexed quantities stacked in rank order, the replicated ones from
                               rank 0, dL_dKnm_block cut from the stacked rows
    device_chunk(n, M)         the rows per chunk that alloc_m (csrc/sparse.hip) chooses for a context with n rows

Nothing here touches the device on import."""
import itertools
import threading
import time

import numpy as np

ROW = ("dL_dm", "dL_dKnm")                   # row-indexed on every rank; dnoise as well where the noise is per point
PREDICTIONS = ("mu1", "var1", "cov1", "mu129", "var129", "cov129")
REPLICATED = ("lml", "dtheta", "dZ", "woodbury_vector", "psi2", "dL_dKmm", "woodbury_inv") + PREDICTIONS
FETCH_STEP = 65536                           # a dL_dKnm fetch takes at most one chunk of rows
NB, SPLITK_MAX, CHUNK_MAX = 128, 16, 262144  # csrc/sparse.hip

# the loopback rendezvous never forgets a key, and a key met again with another world size is refused: every group its own
# (the keys of the other test files are below 10000)
_KEYS = itertools.count(700000)


def fresh_key():
    return next(_KEYS)


def splits(N, rows):
    """[(lo, hi)] per rank.  rows: a tuple of per-rank row counts that sum to N, or a number of ranks for the equal split of
    gpy_amd.grid.shard_rows."""
    if isinstance(rows, (int, np.integer)):
        from gpy_amd.grid import shard_rows
        return [tuple(int(v) for v in shard_rows(N, r, int(rows))) for r in range(int(rows))]
    rows = [int(r) for r in rows]
    assert rows and all(r >= 1 for r in rows) and sum(rows) == N, (N, rows)
    edges = np.concatenate([[0], np.cumsum(rows)])
    return [(int(edges[i]), int(edges[i + 1])) for i in range(len(rows))]


def _round_up(a, b):
    return (a + b - 1) // b * b


def device_splitk(M):
    """the split-K factor of the Gram kernel as alloc_m chooses it: the S <= 16 that fills whole rounds of 512 workgroup slots"""
    nt = _round_up(M, NB) // NB
    ntl = nt * (nt + 1) // 2
    best, beff = 1, 0.0
    for S in range(1, SPLITK_MAX + 1):
        wg = float(ntl * S)
        eff = wg / (np.ceil(wg / 512.0) * 512.0)
        if eff > beff + 1e-9 or (eff > beff - 0.02 and S < best):
            best, beff = S, eff
    return 1 if ntl >= 2048 else best


def device_chunk(n, M):
    """(rows per chunk, number of chunks) of a context that holds n rows: balanced chunks of at most CHUNK_MAX rows, every one
    a multiple of the granule 128 x split-K"""
    gran = NB * device_splitk(M)
    cmax = CHUNK_MAX // gran * gran
    nchunks = (n + cmax - 1) // cmax
    chunk = _round_up((n + nchunks - 1) // nchunks, gran)
    return chunk, (n + chunk - 1) // chunk


def two_chunk_split(N, M):
    """(rows of rank 0, rows of rank 1) for a case of N > CHUNK_MAX rows: rank 0 gets the smallest row count that alloc_m cuts
    in two -- one row more than the largest chunk, so a full chunk and a ragged second one --, rank 1 the rest, which must fit
    one chunk"""
    gran = NB * device_splitk(M)
    n0 = CHUNK_MAX // gran * gran + 1
    n1 = N - n0
    assert n1 >= 1, (N, n0)
    c0, k0 = device_chunk(n0, M)
    assert k0 == 2 and 0 < n0 - c0 < c0 and (n0 - c0) % gran != 0, (n0, c0, k0)
    assert device_chunk(n1, M)[1] == 1, n1
    return n0, n1


def run_ranks(world, fn, timeout=60.0):
    """fn(rank) on one host thread per rank; the results in rank order.

    A rank that raises leaves the others at the rendezvous of the next all-reduce, where they wait for good, and so does a rank
    that hangs.  There is nothing to do for them: after a device error, or when the ranks have not all returned `timeout`
    seconds after the start (or five seconds after one of them raised), the whole pytest run ends here with return code 3, as
    test_gpu_sparse_shapes._check ends it on a device error, and nothing more is started on the GPU.  An exception that every
    rank has returned from (an assertion on replicated state, say) is raised again."""
    import pytest
    from gpy_amd._lib import MI355GPError
    out, errs = [None] * world, [None] * world

    def work(rank):
        try:
            out[rank] = fn(rank)
        except BaseException as e:          # noqa: BLE001 -- looked at on the main thread
            errs[rank] = e
    ts = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(world)]
    for t in ts:
        t.start()
    end, grace = time.monotonic() + float(timeout), None
    while True:
        alive = [t for t in ts if t.is_alive()]
        if not alive:
            break
        alive[0].join(timeout=0.02)
        now = time.monotonic()
        if grace is None and any(e is not None for e in errs):
            grace = now + 5.0
        if now > end or (grace is not None and now > grace):
            break
    failed = [(r, e) for r, e in enumerate(errs) if e is not None]
    stuck = [r for r, t in enumerate(ts) if t.is_alive()]
    if stuck or any(isinstance(e, MI355GPError) for _, e in failed):
        pytest.exit("row-sharded run: ranks %s still at the rendezvous, errors %s; the run ends here"
                    % (stuck, ["rank %d: %r" % f for f in failed]), returncode=3)
    if failed:
        raise failed[0][1]
    return out


def rank_outputs(ctx, c, lo, hi):
    """Everything the judge names, from a context that holds rows [lo, hi) of case c (set_data done): what
    test_gpu_sparse_shapes._evaluate fetches, the row-indexed quantities for the local rows."""
    SC = type(ctx)
    n = hi - lo
    noise = c["noise"][lo:hi] if c["het"] else c["noise"]
    info, r = ctx.vardtc_sum(c["specs"], c["Z"], noise, want_dL_dm=True, per_point=c["het"])
    assert info == 0, info
    got = dict((q, r[q]) for q in ("lml", "dtheta", "dnoise", "dZ", "woodbury_vector", "dL_dm"))
    got["dL_dKnm"] = np.vstack([ctx.fetch_dL_dKnm(a, min(FETCH_STEP, n - a)) for a in range(0, n, FETCH_STEP)])
    got["psi2"] = ctx.fetch(SC.FETCH_PSI2)
    got["dL_dKmm"] = ctx.fetch(SC.FETCH_DLDKMM)
    got["woodbury_inv"] = ctx.fetch(SC.FETCH_WOODBURY_INV)
    for tag in ("1", "129"):
        got["mu" + tag], got["var" + tag] = ctx.predict(c["specs"], c["Xs" + tag])
        got["cov" + tag] = ctx.predict(c["specs"], c["Xs" + tag], full_cov=True)[1]
    return got


def evaluate_sharded(case, rows, group_key=None, timeout=60.0):
    """One evaluation of `case` (sparse_ld.make_case) on len(rows) fresh contexts of device 0 in a loopback group of its own.
    Returns (per-rank outputs, spans)."""
    from gpy_amd._lib import SparseContext
    spans = splits(case["N"], rows)
    key = fresh_key() if group_key is None else group_key

    def rank(r):
        lo, hi = spans[r]
        ctx = SparseContext(0)
        try:
            ctx.attach_loopback(r, len(spans), key)
            ctx.set_data(case["X"][lo:hi], case["R"][lo:hi])
            return rank_outputs(ctx, case, lo, hi)
        finally:
            ctx.close()
    return run_ranks(len(spans), rank, timeout), spans


def per_point(got):
    """whether a result's dnoise is by row (per-point noise) and not one number"""
    return np.ndim(got["dnoise"]) >= 1


def assemble(per_rank, spans, block=None):
    """The global form of per-rank outputs: dL_dm, dL_dKnm (and dnoise where it is per point) stacked in rank order -- every
    rank must have brought exactly its hi - lo rows --, everything else from rank 0; block = (row0, nrows): dL_dKnm_block cut
    from the stacked rows."""
    assert len(per_rank) == len(spans) and spans[0][0] == 0
    assert all(spans[i][1] == spans[i + 1][0] for i in range(len(spans) - 1)), spans
    rowq = ROW + (("dnoise",) if per_point(per_rank[0]) else ())
    out = dict((q, v) for q, v in per_rank[0].items() if q not in rowq)
    for q in rowq:
        parts = [np.asarray(g[q]) for g in per_rank]
        for p, (lo, hi) in zip(parts, spans):
            assert p.shape[0] == hi - lo, (q, p.shape, lo, hi)
        out[q] = np.concatenate(parts, axis=0)
    if block is not None:
        r0, nr = block
        assert 0 <= r0 and nr >= 1 and r0 + nr <= spans[-1][1], block
        out["dL_dKnm_block"] = out["dL_dKnm"][r0:r0 + nr]
    return out


def slice_rows(res, spans):
    """the inverse of `assemble` for a global result (the oracle's): per-rank outputs with the row-indexed quantities sliced"""
    rowq = ROW + (("dnoise",) if per_point(res) else ())
    return [dict((q, (np.array(v[lo:hi]) if q in rowq else v)) for q, v in res.items() if q != "dL_dKnm_block") for lo, hi in spans]


def replication_faults(per_rank):
    """the replicated quantities whose bytes differ between rank 0 and another rank: [(quantity, rank)]"""
    bad = []
    for r in range(1, len(per_rank)):
        for q in REPLICATED:
            a, b = np.asarray(per_rank[0][q]), np.asarray(per_rank[r][q])
            if a.shape != b.shape or a.tobytes() != b.tobytes():
                bad.append((q, r))
    return bad
