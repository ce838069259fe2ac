"""GPU (-m gpu): the ROW-SHARDED sparse (VarDTC) path -- one context per rank with a slice of the rows, the all-reduces of
mi355gp_sparse_set_data (N, tr YY^T), vardtc_pass1 (psi2, psi1^T V), vardtc_pass2 (the parts' gradient records) and
vardtc_evaluate (three per-point sums), everything M x M replicated -- at shard edges, judged against the long-double
restatement tests/sparse_ld.py.  A sharded evaluation must return what the unsharded one returns, so the references, the fp64
oracle and the judge are those of tests/test_gpu_sparse_shapes.py, unchanged (tests/test_oracle_sparse_shard.py shows that the
plumbing of tests/sparse_shard.py is neutral and that the judge rejects what sharding can get wrong):

    err(q) = max |got - q_ld| / max |q_ld| <= max(32 e64(q), 256 eps64 kappa),

e64 = the fp64 oracle's distance from long double on the same input, never the device's figure.  Every quantity of
sparse_ld.JUDGED must be there; dL_dm, dL_dKnm and a per-point dnoise are assembled from the ranks' local rows, dL_dKnm_block is
cut from the assembled rows; dL_dKmm is symmetric to 1e-13 of its largest entry.  For every case ALL ranks return identical
bytes for lml, dtheta, dZ, woodbury_vector, psi2, dL_dKmm, woodbury_inv and every prediction (`replicated M x M algebra`,
csrc/sparse.hip; it holds by construction for the loopback's sum in rank order).

Ranks are host threads over the loopback transport, every group with fresh contexts and a key of its own.  Families (cases are
sparse_ld names; rows per rank):
    lone       n_edge N = 2, both kernels: (1, 1) -- every rank one row, n < M
    edges      n_edge N = 257, both kernels: (256, 1) (1, 256) (128, 129) (127, 1, 129) and eight ranks by shard_rows
    granule    n_edge N = 2049, both kernels: (2048, 1) (1, 2048) (1024, 1025) -- ranks that hold different numbers of granules
    m_edge     rbf_ard M = 1 | 127 | 128 | 129 | 257: (129, 128); rbf + white and the product at M = 128 | 129: three ranks
    noise      all twelve per-point-noise cases: N = 257 (130, 127), N = 129 (1, 128)
    dispatch   the subset case on three ranks; the fourteen (D, Dy) dispatch cases: (97, 96)
    stale      sparse_ld.STALE in order on two ranks, one attach and one set_data, no set_data between the members: M and mp
               change (every M x M buffer and the packed all-reduce buffer are reallocated), so do the part list and the noise
    chunks     chunks-rbf_ard+bias-n266240_m3_d2_dy2-het: M = 3 gives split-K 16, a granule of 2048 rows and chunks of at most
               262144; rank 0 gets 262145 rows, the fewest that are cut in two (133120 + 129025, the second ragged), rank 1 the
               other 4095 (one chunk of 4096).  The judged block, rows 133000 ... 133299, still lies across rank 0's chunk
               boundary; a second block, rows 261995 ... 262294, takes rows from both ranks.
Further: determinism (sparse_ld.DETERMINISM twice on (127, 1, 129), fresh contexts and groups, every output identical bytes);
a group of ONE rank passes the judge, and its distance from the unsharded context's bytes is printed, not asserted (nothing in
the code promises that the two dispatch alike); the refusals of a sharded context by message, on a one-rank group, after which
the same context still passes the judge; and one case with REAL ranks, two processes over the hipIpc transport as in
tests/test_gpu_multiproc.py, noise-prod-n257_m65_d3_dy3-het split (1, 256), each rank's outputs through an .npz to the same
assembly and judge.

Not tested, on purpose: one rank refused or failing while the others proceed.  The others would wait at the rendezvous for
good (the transports have no time limit of their own over the loopback), so sparse_shard.run_ranks ends the whole pytest run
(return code 3) when it sees that, and every refusal here is made where no other rank exists.

The fault the sweep found, and its fix.  noise-exponential_iso-n129_m128_d3_dy1-het split (1, 128), as the code stood: lml
4.1e+00 against a bound of 6.5e-13, dtheta 5.9e+00, dZ 1.3e+00, woodbury_vector 8.5e-01, dnoise of the wrong shape; every per-point
case with a lone-row rank alike.  mi355gp_vardtc_inference_sum told per-point from scalar noise by noise_len > 1, so a rank with
ONE row and its one variance took the scalar reading (psi2 = Kuf Kfu, the precision applied afterwards) while the other ranks
summed beta_n k_n k_n^T into the same all-reduce.  On an unsharded context the two readings of one row are the same model; on a
sharded one every rank must take the same reading, and a rank cannot see from its own row what the others hold.  Now a rank
that holds one row states per-point noise by passing dnoise_rows_out (SparseContext.vardtc_sum(..., per_point=True)); the
count of per-point ranks travels in a fourth entry of the call's last all-reduce, and a mixed group is refused on every rank
alike (test_ranks_that_read_the_noise_differently_are_refused_alike).  An unsharded context computes what it computed.

Measured on an MI355X after the fix, worst err(q) per family (a record, never a reason to tighten a bound; wv =
woodbury_vector, Winv = woodbury_inv; the prediction columns are those at 129 points; err/bound = the worst ratio of a figure to
its bound over the family; world1 / refusals / processes: the one-rank group, the context after its refusals, the two processes):

    family         lml  dtheta  dnoise      dZ      wv   dL_dm dL_dKnm    psi2 dL_dKmm    Winv      mu     var     cov  err/bound
    lone         6e-16   1e-15   9e-16   2e-15   6e-15   1e-16   1e-15   3e-16   2e-15   6e-15   4e-15   9e-16   9e-16      0.007
    edges        8e-16   8e-15   9e-16   7e-14   6e-14   3e-15   7e-14   5e-16   3e-14   1e-14   7e-14   3e-15   4e-15      0.015
    granule      7e-16   4e-15   9e-16   6e-14   7e-14   2e-15   6e-14   6e-16   3e-14   3e-15   6e-14   3e-15   3e-15      0.014
    m_edge       1e-15   8e-16   2e-15   3e-14   5e-14   5e-16   4e-14   1e-15   6e-15   4e-14   2e-14   5e-15   5e-15      0.044
    noise        4e-16   1e-15   5e-15   1e-14   3e-14   3e-16   5e-14   8e-16   8e-15   2e-14   1e-14   3e-15   3e-15      0.036
    dispatch     7e-16   3e-15   2e-15   5e-14   3e-14   5e-16   2e-14   1e-15   6e-15   8e-15   1e-14   1e-14   1e-14      0.011
    stale        7e-16   2e-14   3e-15   1e-13   3e-13   6e-15   2e-13   4e-16   8e-14   9e-14   7e-14   2e-14   2e-14      0.024
    chunks       1e-15   5e-15   7e-16   2e-14   2e-15   1e-16   1e-15   8e-16   6e-15   7e-16   2e-15   8e-16   1e-15      0.059
    world1       6e-16   4e-15   4e-17   5e-14   6e-14   2e-15   5e-14   3e-16   1e-14   7e-15   5e-14   2e-15   2e-15      0.010
    refusals     4e-16   1e-15   1e-15   2e-14   2e-14   2e-16   2e-14   6e-16   3e-15   9e-15   9e-15   2e-15   2e-15      0.013
    processes    5e-16   6e-16   2e-15   1e-14   3e-14   3e-16   3e-14   4e-16   3e-15   4e-15   9e-15   1e-15   1e-15      0.023

The dL_dKnm blocks and the one-point prediction stay within 3e-13; dL_dKmm differs from its transpose by at most 5e-14 of its
largest entry; no replicated quantity differed between ranks in any case.  The one-rank group returned the unsharded context's
bytes in every output (max |diff| 0: printed, not asserted).  The whole file: 61 tests, 16 s of wall time with its long-double
references (the two-chunk case 2 s, the four stale members 1.7 s together, every other case under 1.2 s).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from gpy_amd import _lib as L

import kern_ld as KL
import sparse_ld as SL
import sparse_shard as SH
from test_gpu_multiproc import ROOT, _need_gpu_processes

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not KL.HAVE_LD, reason="np.longdouble is not an extended format on this host")]
SC = L.SparseContext
BIG = "chunks-rbf_ard+bias-n266240_m3_d2_dy2-het"


def _n_edge(N):
    return ["n_edge-%s-n%d_m65_d3_dy2-hom" % (k, N) for k in ("matern52_iso", "rbf_ard+bias")]


def _sweep():
    out = [("lone", n, (1, 1)) for n in _n_edge(2)]
    out += [("edges", n, rows) for n in _n_edge(257) for rows in ((256, 1), (1, 256), (128, 129), (127, 1, 129), 8)]
    out += [("granule", n, rows) for n in _n_edge(2049) for rows in ((2048, 1), (1, 2048), (1024, 1025))]
    out += [("m_edge", "m_edge-rbf_ard-n257_m%d_d2_dy1-hom" % M, (129, 128)) for M in (1, 127, 128, 129, 257)]
    out += [("m_edge", "m_edge-%s-n257_m%d_d2_dy1-hom" % (k, M), 3) for k in ("rbf+white", "prod") for M in (128, 129)]
    noise = [c["name"] for c in SL.CASES if c["family"] == "noise"]
    out += [("noise", n, (130, 127) if SL.BY_NAME[n]["N"] == 257 else (1, 128)) for n in noise]
    out += [("dispatch", c["name"], 3) for c in SL.CASES if c["family"] == "subset"]
    out += [("dispatch", c["name"], (97, 96)) for c in SL.CASES if c["family"] == "dispatch"]
    return out


SWEEP = _sweep()
assert len(SWEEP) == 2 + 10 + 6 + 9 + 12 + 15 and all(n in SL.BY_NAME for _, n, _ in SWEEP)


def _tag(rows):
    return "w%d" % rows if isinstance(rows, int) else "x".join(str(r) for r in rows)


def _judge(family, name, tag, got, block=None):
    """print every figure, then hold it to its bound; block: judge this (row0, nrows) of dL_dKnm in place of the case's own"""
    c, ref, r64, kappa = SL.reference(name)
    if block is not None:
        r0, nr = block
        ref, r64 = dict(ref), dict(r64)
        ref["dL_dKnm_block"], r64["dL_dKnm_block"] = ref["dL_dKnm"][r0:r0 + nr], r64["dL_dKnm"][r0:r0 + nr]
    figs, bad = SL.judge(got, ref, r64, kappa)
    print()
    for q in SL.JUDGED:
        if q in figs:
            print("FIG %s %s %s %s %.2e (bound %.2e)" % (family, name, tag, q, figs[q][0], figs[q][1]))
    dK = got["dL_dKmm"]
    asym = float(np.abs(dK - dK.T).max() / np.abs(dK).max())
    print("FIG %s %s %s dL_dKmm_asym %.2e" % (family, name, tag, asym))
    assert not bad, bad
    assert set(figs) == set(SL.JUDGED)
    assert asym <= 1e-13


def _check(family, name, rows, timeout=60.0, more_blocks=()):
    c = SL.reference(name)[0]
    per, spans = SH.evaluate_sharded(c, rows, timeout=timeout)
    faults = SH.replication_faults(per)
    _judge(family, name, _tag(rows), SH.assemble(per, spans, c["block"]))
    for blk in more_blocks:
        assert spans[0][1] > blk[0] and spans[0][1] < blk[0] + blk[1]          # rows of both ranks
        _judge(family, name, _tag(rows) + "+block%d" % blk[0], SH.assemble(per, spans, blk), block=blk)
    assert not faults, faults
    return per, spans


@pytest.mark.parametrize("family,name,rows", SWEEP, ids=["%s-%s" % (n, _tag(r)) for _, n, r in SWEEP])
def test_sharded_shape_edges(family, name, rows):
    _check(family, name, rows)


def test_sharded_rank_with_two_chunks_beside_a_rank_with_one():
    c = SL.reference(BIG)[0]
    rows = SH.two_chunk_split(c["N"], c["M"])
    assert rows == (262145, 4095) and SH.device_chunk(rows[0], c["M"]) == (133120, 2)
    _check("chunks", BIG, rows, timeout=300.0, more_blocks=[(rows[0] - 150, 300)])


def test_sharded_stale_state_between_calls():
    """one attach and one set_data per rank, then the members of sparse_ld.STALE in order"""
    cases = [SL.reference(n)[0] for n in SL.STALE]
    rows = (130, 127)
    spans = SH.splits(cases[0]["N"], rows)
    key = SH.fresh_key()

    def rank(r):
        lo, hi = spans[r]
        ctx = SC(0)
        try:
            ctx.attach_loopback(r, len(spans), key)
            ctx.set_data(cases[0]["X"][lo:hi], cases[0]["R"][lo:hi])
            return [SH.rank_outputs(ctx, c, lo, hi) for c in cases]
        finally:
            ctx.close()
    res = SH.run_ranks(len(spans), rank, timeout=120.0)
    for i, c in enumerate(cases):
        per = [res[r][i] for r in range(len(spans))]
        _judge("stale", c["name"], _tag(rows), SH.assemble(per, spans, c["block"]))
        assert not SH.replication_faults(per), (c["name"], SH.replication_faults(per))


def test_sharded_is_deterministic_across_fresh_contexts_and_groups():
    c = SL.make_case(SL.DETERMINISM)
    a, spans = SH.evaluate_sharded(c, (127, 1, 129))
    b, _ = SH.evaluate_sharded(c, (127, 1, 129))
    for r in range(len(spans)):
        assert set(a[r]) == set(b[r])
        for q in a[r]:
            assert np.asarray(a[r][q]).tobytes() == np.asarray(b[r][q]).tobytes(), (r, q)


def test_group_of_one_rank():
    name = "n_edge-rbf_ard+bias-n257_m65_d3_dy2-hom"
    c = SL.reference(name)[0]
    per, spans = _check("world1", name, (c["N"],))
    ctx = SC(0)
    try:
        ctx.set_data(c["X"], c["R"])
        plain = SH.rank_outputs(ctx, c, 0, c["N"])
    finally:
        ctx.close()
    print()
    for q in sorted(plain):                  # a record: the code does not promise that the two are the same bytes
        d = float(np.max(np.abs(np.asarray(plain[q]) - np.asarray(per[0][q]))))
        print("FIG world1-vs-unsharded %s max|diff| %.2e" % (q, d))


def test_sharded_context_refuses_by_message_and_still_works():
    """on a group of ONE rank: no other rank is left waiting when a call is refused"""
    name = "noise-rbf_ard-n257_m65_d3_dy1-het"
    c = SL.reference(name)[0]
    N, M, D = c["N"], c["M"], c["D"]
    X, Z, specs = c["X"], c["Z"], c["specs"]
    rbf2 = ("rbf", 0, np.array([1.0, 1.0]), np.array([0, 1], dtype=np.int32), 1)
    coreg = ("coregionalize", 2, np.eye(2).ravel(), np.array([2], dtype=np.int32), 1)
    linear = ("linear", 0, np.array([1.0]), None, 0)
    plain_rbf = [("rbf", 0, np.array([1.0, 1.0]), None, 0)]
    S, gamma = np.full(X.shape, 0.01), np.full(X.shape, 0.5)
    key = SH.fresh_key()
    ctx = SC(0)
    try:
        ctx.attach_loopback(0, 1, key)
        ctx.set_linear(True)
        ctx.set_coregionalize(True)
        ctx.set_data(X, c["R"])
        assert ctx.vardtc_sum(specs, Z, c["noise"])[0] == 0                       # (predict_uncertain asks for a result first)
        refused = [                          # (predict_uncertain first: every later call forgets the result)
            ("predict_uncertain", lambda: ctx.predict_uncertain(specs, c["Xs1"], np.full((1, D), 0.01)),
             "predict_uncertain: a row-sharded context is not supported"),
            ("Linear", lambda: ctx.vardtc_sum(specs + [linear], Z, c["noise"]), r"Linear \(kind 9\) part is not supported by a row-sharded"),
            ("Coregionalize", lambda: ctx.vardtc_sum([rbf2, coreg], Z, c["noise"]),
             r"Coregionalize \(kind 8\) part is not supported by a row-sharded"),
            ("set_input_variance", lambda: ctx.set_input_variance(S), "set_input_variance: uncertain inputs are not supported by a row-sharded"),
            ("set_inputs", lambda: ctx.set_inputs(X, S), "set_inputs: replacing the inputs of a row-sharded"),
            ("set_binary_prob", lambda: ctx.set_binary_prob(gamma), "set_binary_prob: spike-and-slab inputs are not supported by a row-sharded"),
            ("set_inputs_ss", lambda: ctx.set_inputs_ss(X, S, gamma), "set_inputs_ss: replacing the inputs of a row-sharded"),
            ("set_output_groups", lambda: ctx.set_output_groups(np.zeros(1, dtype=np.int32), np.ones((N, 1))),
             "set_output_groups: a row-sharded context is not supported"),
            ("vardtc_uncertain", lambda: ctx.vardtc_uncertain(plain_rbf, Z, 0.1), "inference_uncertain: a row-sharded context is not supported"),
            ("vardtc_ss", lambda: ctx.vardtc_ss(plain_rbf, Z, 0.1), "inference_ss: a row-sharded context is not supported"),
            ("vardtc_missing", lambda: ctx.vardtc_missing(plain_rbf, Z, 0.1), "inference_missing: a row-sharded context is not supported"),
            ("kdiag", lambda: ctx.kdiag(specs), "sparse_kdiag: a row-sharded context is not supported"),
            ("svgp_forward", lambda: ctx.svgp_forward(specs, Z, np.zeros((M, 1)), np.eye(M)[None]), "svgp_forward: a row-sharded context is not supported by SVGP"),
            ("pep", lambda: ctx.pep(specs, Z, 0.1, 0.5, 1e-8), "pep_inference: a row-sharded context is not supported by PEP / FITC"),
            ("epdtc_begin", lambda: ctx.epdtc_begin(specs, Z), "epdtc_begin: a row-sharded context is not supported by EPDTC"),
        ]
        for what, call, message in refused:
            with pytest.raises(L.MI355GPError, match=message):
                call()
        other = SC(0)
        try:
            with pytest.raises(L.MI355GPError, match="attach_loopback: the group exists with a different world size"):
                other.attach_loopback(0, 2, key)
        finally:
            other.close()
        got = SH.rank_outputs(ctx, c, 0, N)
    except L.MI355GPError as e:              # none of the above: an error of the runtime, nothing more on this device
        pytest.exit("device error on the one-rank context, the run ends here: %s" % e, returncode=3)
    finally:
        ctx.close()
    _judge("refusals", name, _tag((N,)), SH.assemble([got], [(0, N)], c["block"]))


def test_ranks_that_read_the_noise_differently_are_refused_alike():
    """Rank 0 holds ONE row and does not say that its one variance is per-point noise; rank 1 passes 128 variances.  psi2 is
    then a sum over two readings (positive semi-definite still: both factorisations go through, and every rank reaches every
    collective).  The count of per-point ranks travels with the call's last all-reduce, so BOTH ranks refuse, by message, and
    nobody is left waiting."""
    c = SL.reference("noise-exponential_iso-n129_m128_d3_dy1-het")[0]
    spans = SH.splits(c["N"], (1, 128))
    key = SH.fresh_key()

    def rank(r):
        lo, hi = spans[r]
        ctx = SC(0)
        try:
            ctx.attach_loopback(r, len(spans), key)
            ctx.set_data(c["X"][lo:hi], c["R"][lo:hi])
            try:
                ctx.vardtc_sum(c["specs"], c["Z"], c["noise"][lo:hi])
            except L.MI355GPError as e:
                return str(e)
            return "no error"
        finally:
            ctx.close()
    said = SH.run_ranks(len(spans), rank)
    for r, msg in enumerate(said):
        assert "1 of the 2 ranks of this row-sharded context passed per-point noise" in msg, (r, msg)


_WORKER = r"""
import os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np
from gpy_amd import _lib as L, grid as G
import sparse_ld as SL
import sparse_shard as SH
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
c = SL.make_case(%(name)r)
lo, hi = SH.splits(c["N"], %(rows)r)[rank]
idb = G.unique_id() if rank == 0 else b"\0" * G.ID_BYTES
idb = G.exchange_id_file(idb, rank, os.path.join(os.environ["MI355GP_ID_DIR"], "sparse_id"), world=world)
ctx = L.SparseContext(0)
ctx.attach_comm(rank, world, idb)
ctx.set_data(c["X"][lo:hi], c["R"][lo:hi])
got = SH.rank_outputs(ctx, c, lo, hi)
ctx.close()
np.savez(os.path.join(os.environ["MI355GP_ID_DIR"], "rank%%d.npz" %% rank), **got)
print("RESULT done")
"""


def test_sharded_with_one_process_per_rank(tmp_path):
    """REAL ranks: two processes over the hipIpc transport (the environment and time limits of tests/test_gpu_multiproc.py),
    rank 0 with ONE row; product kernel + White, per-point noise, three output columns"""
    name, rows, world = SL.DETERMINISM, (1, 256), 2
    assert name == "noise-prod-n257_m65_d3_dy3-het"
    _need_gpu_processes(world)
    c = SL.reference(name)[0]
    script = tmp_path / "worker.py"
    script.write_text(_WORKER % dict(root=ROOT, name=name, rows=rows))
    env = dict(os.environ, WORLD_SIZE=str(world), LOCAL_RANK="0", MI355GP_TRANSPORT="ipc", MI355GP_ID_DIR=str(tmp_path),
               MI355GP_JOB_NONCE="h%d" % os.getpid(), MI355GP_IPC_TIMEOUT_S="240", HSA_ENABLE_IPC_MODE_LEGACY="0",
               MASTER_PORT=str(29000 + os.getpid() % 2000))
    env.pop("TORCHELASTIC_RUN_ID", None)
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for r in range(world)]
    for r, p in enumerate(procs):
        so, se = p.communicate(timeout=900)
        assert p.returncode == 0 and "RESULT done" in so, "rank %d failed:\n%s" % (r, se[-3000:])
    per = []
    for r in range(world):
        d = dict(np.load(str(tmp_path / ("rank%d.npz" % r)), allow_pickle=False))
        d["lml"] = float(d["lml"])
        per.append(d)
    spans = SH.splits(c["N"], rows)
    _judge("processes", name, _tag(rows), SH.assemble(per, spans, c["block"]))
    assert not SH.replication_faults(per), SH.replication_faults(per)
