"""CPU: the plumbing that tests/test_gpu_sparse_sharded.py judges the row-sharded sparse path with (tests/sparse_shard.py), and
proof that the judge behind it can fail.

On a small case, n_edge-rbf_ard+bias-n257_m65_d3_dy2-hom, and its per-point twin, noise-rbf+white-n257_m65_d3_dy1-het:

(1) Neutral plumbing: the fp64 oracle's own outputs, sliced into per-rank results by `splits` and put back by `assemble`, are the
    oracle's outputs byte for byte and pass sparse_ld.judge with every quantity judged, at every split of the GPU sweep's
    shard-edge family.
(2) The judge rejects what a sharded evaluation can get wrong, each on the quantity it corrupts:
    (a) the oracle evaluated on rank 0's rows only (a missing all-reduce: everything replicated is off, the row-indexed
        quantities have rank 0's rows alone);
    (b) lml and the Bias / White entries of dtheta with rank 0's sum of precisions, not the global one, in the Kdiag terms
        (-Dy/2 sum_n beta_n psi0 of the bound, dL_dKdiag = -Dy beta_n / 2 of update_gradients_diag): lml and dtheta alone;
    (c) the per-point dnoise rows of rank 1 shifted by one row (a global offset where a local one is due): dnoise alone;
    (d) psi2 without the rows of the last rank, one row of 257: psi2 alone.
(3) `splits` and gpy_amd.grid.shard_rows agree on equal splits; `device_chunk` restates how a context cuts its rows into chunks
    (the chunk boundary of sparse_ld.CHUNK_BLOCKS, 133120, is what it gives), and `two_chunk_split` gives rank 0 a full chunk and
    a ragged one and rank 1 a single chunk; `run_ranks` returns in rank order and passes an exception on that every rank left
    behind."""
import numpy as np
import pytest

import kern_ld as KL
import sparse_ld as SL
import sparse_shard as SH
from oracle import gp_oracle as O

pytestmark = pytest.mark.skipif(not KL.HAVE_LD, reason="np.longdouble is not an extended format on this host")
HOM, HET = "n_edge-rbf_ard+bias-n257_m65_d3_dy2-hom", "noise-rbf+white-n257_m65_d3_dy1-het"
SPLITS = ((256, 1), (1, 256), (128, 129), (127, 1, 129), 8)


def _names(bad):
    return set(b.split(":")[0] for b in bad if not b.startswith("dZ column"))


@pytest.mark.parametrize("name", [HOM, HET])
@pytest.mark.parametrize("rows", SPLITS, ids=str)
def test_slicing_and_assembling_the_oracle_changes_nothing(name, rows):
    c, ref, r64, kappa = SL.reference(name)
    spans = SH.splits(c["N"], rows)
    per = SH.slice_rows(r64, spans)
    assert SH.per_point(r64) == c["het"] and not SH.replication_faults(per)
    got = SH.assemble(per, spans, c["block"])
    for q in SL.JUDGED:
        assert np.asarray(got[q]).tobytes() == np.asarray(r64[q]).tobytes(), q
    figs, bad = SL.judge(got, ref, r64, kappa)
    assert not bad and set(figs) == set(SL.JUDGED)


@pytest.mark.parametrize("name", [HOM, HET])
def test_judge_rejects_an_evaluation_of_rank_0_alone(name):
    c, ref, r64, kappa = SL.reference(name)
    lo, hi = SH.splits(c["N"], (128, 129))[0]
    c0 = dict(c, N=hi, X=c["X"][:hi], R=c["R"][:hi], noise=c["noise"][:hi] if c["het"] else c["noise"], block=(0, 1))
    figs, bad = SL.judge(SL.oracle64(c0), ref, r64, kappa)
    assert _names(bad) >= {"lml", "dtheta", "dnoise", "dZ", "woodbury_vector", "dL_dm", "dL_dKnm", "psi2", "dL_dKmm",
                           "woodbury_inv", "mu1", "mu129", "var129", "cov129"}, bad


@pytest.mark.parametrize("name", [HOM, HET])
def test_judge_rejects_rank_0s_precisions_in_the_kdiag_terms(name):
    c, ref, r64, kappa = SL.reference(name)
    hi = SH.splits(c["N"], (128, 129))[0][1]
    beta = 1.0 / np.fmax(np.broadcast_to(c["noise"], (c["N"],)), SL.JITTER)
    missing = float(beta[hi:].sum())                              # what rank 0's sum of precisions lacks
    psi0 = float(np.max(KL.Kdiag(c["specs"], c["X"][:1], np.float64)))
    got = dict(r64)
    got["lml"] = r64["lml"] + 0.5 * c["Dy"] * psi0 * missing
    got["dtheta"] = np.array(r64["dtheta"])
    first = np.cumsum([0] + [KL.n_params(s) for s in c["specs"]])[:-1]
    static = [i for i, s in enumerate(c["specs"]) if s[0] in ("white", "bias")]
    assert static
    for i in static:
        got["dtheta"][first[i]] += 0.5 * c["Dy"] * missing
    figs, bad = SL.judge(got, ref, r64, kappa)
    assert _names(bad) == {"lml", "dtheta"}, bad


def test_judge_rejects_per_point_noise_rows_shifted_by_one():
    c, ref, r64, kappa = SL.reference(HET)
    spans = SH.splits(c["N"], (130, 127))
    per = SH.slice_rows(r64, spans)
    per[1]["dnoise"] = np.roll(per[1]["dnoise"], 1, axis=0)
    figs, bad = SL.judge(SH.assemble(per, spans, c["block"]), ref, r64, kappa)
    assert _names(bad) == {"dnoise"}, bad


@pytest.mark.parametrize("name", [HOM, HET])
def test_judge_rejects_psi2_without_the_last_ranks_one_row(name):
    c, ref, r64, kappa = SL.reference(name)
    lo = SH.splits(c["N"], (256, 1))[-1][0]
    psi1 = O.sum_kern_K(c["parts"], c["X"][:lo], c["Z"])
    got = dict(r64)
    got["psi2"] = (psi1 / np.fmax(c["noise"][:lo], SL.JITTER)[:, None]).T @ psi1 if c["het"] else psi1.T @ psi1
    figs, bad = SL.judge(got, ref, r64, kappa)
    assert _names(bad) == {"psi2"}, bad


def test_assemble_counts_every_ranks_rows():
    c, ref, r64, kappa = SL.reference(HET)
    spans = SH.splits(c["N"], (130, 127))
    per = SH.slice_rows(r64, spans)
    per[1]["dL_dm"] = per[1]["dL_dm"][:-1]
    with pytest.raises(AssertionError):
        SH.assemble(per, spans, c["block"])
    per = SH.slice_rows(r64, spans)
    per[1]["dtheta"] = per[1]["dtheta"] * (1.0 + 2.0 ** -52)
    assert SH.replication_faults(per) == [("dtheta", 1)]


def test_splits_agree_with_shard_rows_and_chunks_with_the_case_list():
    from gpy_amd.grid import shard_rows
    for N in (2, 257, 2049, 266240):
        for world in (1, 2, 3, 8):
            if world > N:
                continue
            want = [tuple(shard_rows(N, r, world)) for r in range(world)]
            assert SH.splits(N, world) == want
            assert SH.splits(N, tuple(hi - lo for lo, hi in want)) == want
            assert want[0][0] == 0 and want[-1][1] == N
    assert SH.splits(257, (127, 1, 129)) == [(0, 127), (127, 128), (128, 257)]
    for rows in ((128, 128), (257, 0), ()):
        with pytest.raises(AssertionError):
            SH.splits(257, rows)
    # the chunk boundaries that sparse_ld's `chunks` family is built around
    big = "chunks-rbf_ard+bias-n266240_m3_d2_dy2-het"
    assert SH.device_splitk(3) == 16 and SH.device_chunk(266240, 3) == (133120, 2)
    r0, nr = SL.CHUNK_BLOCKS[big]
    assert r0 < 133120 < r0 + nr
    chunk, k = SH.device_chunk(262145, 128)
    assert k == 2 and 0 < 262145 - chunk < chunk
    assert SH.device_chunk(1, 65)[1] == 1 and SH.device_chunk(2049, 65)[1] == 1
    n0, n1 = SH.two_chunk_split(266240, 3)
    assert (n0, n1) == (262145, 4095) and SH.device_chunk(n0, 3) == (133120, 2) and SH.device_chunk(n1, 3) == (4096, 1)
    assert r0 < SH.device_chunk(n0, 3)[0] < r0 + nr            # the judged block still lies across rank 0's chunk boundary


def test_run_ranks_keeps_rank_order_and_passes_a_common_exception_on():
    assert SH.run_ranks(3, lambda r: 10 * r) == [0, 10, 20]
    assert len(set([SH.fresh_key(), SH.fresh_key(), SH.fresh_key()])) == 3

    def fails(r):
        raise ValueError("rank %d" % r)
    with pytest.raises(ValueError, match="rank 0"):
        SH.run_ranks(2, fails)
