"""GPU (-m gpu): the sparse (VarDTC) device path -- mi355gp_vardtc_inference_sum with its Gram and GEMM kernels, the fused and
unfused gradient passes, mi355gp_sparse_predict and the fetches -- at every shape edge, judged against the long-double
restatement tests/sparse_ld.py (80-bit; tests/test_oracle_sparse_ld.py is its own proof).

Judge (sparse_ld.judge): err(q) = max |got - q_ld| / max |q_ld| <= max(32 e64(q), 256 eps64 kappa), e64 = the distance of the
fp64 oracle (oracle/sparse_oracle.py) from long double on the same input (never the device's figure), kappa = cond2(Kmm + 1e-8 I).
The inputs (Z on a jittered grid, lengthscales of 0.75 grid spacings) keep kappa <= 303 and e64 <= 2e-12, so no bound exceeds
3.2e-10, against the standing 1e-9 ... 1e-4 of tests/test_gpu_sparse.py.  dZ columns outside every part's active_dims must be
exactly zero.  Judged per case: lml, dtheta, dnoise, dZ, woodbury_vector, dL_dm, dL_dKnm (all rows and one interior block),
psi2, dL_dKmm (also symmetric to 1e-13 of its largest entry), woodbury_inv, and the prediction (mean, variance, covariance) at
1 and at 129 new points.

One module-scoped context serves the whole sweep in list order (sparse_ld.CASES): whatever a case leaves in the device buffers
is there for the next one.  Families (N, M, D, Dy):
    m_edge    N = 257, D = 2, Dy = 1, M = 1 | 127 | 128 (m == mp) | 129 (persistent Kmm launch on the side stream) | 257 (three
              tiles); 128 | 129 also as rbf + white (unfused pass 1) and as rbf[0] x matern32[1] + white (D = 2 leaves the
              product one column each)
    n_edge    M = 65, D = 3, Dy = 2, N = 1 | 2 | 127 | 128 | 129 (128-row GEMM padding) | 255 | 256 | 257 (256-row Gram rounding)
              | 2049 (chunk granule), matern52_iso (fused) and rbf_ard + bias (unfused); N < M on purpose
    noise     per-point noise, Dy = 1 | 3, at 257/65 and 129/128: one stationary part (rbf_ard | exponential_iso), rbf + white,
              rbf[0,1] x matern32[2] + white
    subset    rbf_ard on columns 0 and 2 of three
    dispatch  N = 193, M = 65, (D, Dy) = (16,4) (16,5) (17,1) (32,4) (32,5) (33,1) (1,1), rbf_ard and matern32_ard
    stale     no set_data between: product + per-point noise, Dy = 3, M = 129 -> rbf_ard, scalar noise, M = 129 -> M = 128 -> new
              Z and theta
    wide      N = 70, M = 20, Dy = 1, rbf_ard at D = 240 | 241: eight theta records of 34 doubles; D = 241 is the first to use
              entry 256 (the lengthscale sum of q = 240), which one 256-thread block does not reach (the shipped code before
              the row-gradient step became shared failed it: dtheta 8.6e-07 against a bound of 2.0e-12)
    chunks    blocked reference: 262145/128/2/1 rbf_ard (fused, m == mp, ragged second chunk), 266240/3/2/2 rbf_ard + bias
              with per-point noise and dL_dm (two full chunks with m < mp: no memset; unfused; dL_dKnm rows 133000 ... 133299
              straddle the chunk boundary), 262145/65/3/1 product + white
Determinism: one case twice in fresh contexts, identical bytes.

Measured on an MI355X, worst err(q) per family (never a reason to tighten a bound; wv = woodbury_vector, Winv = woodbury_inv;
the prediction columns are those at 129 points; err/bound = the worst ratio of a figure to its bound over the family):

    family        lml  dtheta  dnoise      dZ      wv   dL_dm dL_dKnm    psi2 dL_dKmm    Winv      mu     var     cov  err/bound
    m_edge      2e-15   8e-16   4e-15   3e-14   6e-14   4e-16   5e-14   1e-15   5e-15   5e-14   2e-14   6e-15   6e-15     0.059
    n_edge      2e-15   1e-14   3e-15   8e-14   2e-13   5e-15   2e-13   8e-16   3e-14   5e-14   1e-13   2e-14   2e-14     0.058
    noise       7e-16   1e-15   5e-15   2e-14   2e-14   3e-16   2e-14   8e-16   9e-15   3e-14   2e-14   5e-15   5e-15     0.024
    subset      4e-16   9e-16   2e-16   2e-14   1e-14   3e-16   9e-15   4e-16   2e-15   2e-15   6e-15   2e-15   2e-15     0.006
    dispatch    4e-15   3e-15   4e-15   6e-14   3e-14   1e-15   4e-14   1e-15   7e-15   7e-15   3e-14   9e-15   9e-15     0.022
    stale       1e-15   1e-14   3e-15   2e-13   2e-13   6e-15   3e-13   5e-16   1e-13   1e-13   7e-14   1e-14   2e-14     0.028
    chunks      6e-14   5e-15   6e-14   7e-14   3e-14   8e-16   3e-14   3e-15   1e-14   3e-15   3e-14   3e-15   4e-15     0.047

The interior dL_dKnm block and the one-point prediction stay within 3e-13; dL_dKmm differs from its transpose by at most 3e-14
of its largest entry.  Every case passed as the code stood: the sweep found no fault in the device path, and no product code
changed with it.  The whole file: 64 cases, about 30 s of wall time, most of it the long-double references (the two
262145-row cases take 4 ... 6 s each, the blocked reference and the fp64 oracle on a quarter of a million rows).
"""
import numpy as np
import pytest

from gpy_amd import _lib as L

import kern_ld as KL
import sparse_ld as SL

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not KL.HAVE_LD, reason="np.longdouble is not an extended format on this host")]
SC = L.SparseContext


@pytest.fixture(scope="module")
def sctx():
    c = SC(0)
    c.held = None                        # the (X, R) the context holds
    yield c
    c.close()


def _evaluate(sctx, c):
    """everything the judge names, from the device"""
    N = c["N"]
    if sctx.held is None or not (np.array_equal(sctx.held[0], c["X"]) and np.array_equal(sctx.held[1], c["R"])):
        sctx.set_data(c["X"], c["R"])
        sctx.held = (c["X"], c["R"])
    info, r = sctx.vardtc_sum(c["specs"], c["Z"], c["noise"], want_dL_dm=True)
    assert info == 0
    got = dict((q, r[q]) for q in ("lml", "dtheta", "dnoise", "dZ", "woodbury_vector", "dL_dm"))
    step = 65536                         # a fetch takes at most one chunk of rows: the sweep's single-chunk cases in one piece
    got["dL_dKnm"] = np.vstack([sctx.fetch_dL_dKnm(a, min(step, N - a)) for a in range(0, N, step)])
    r0, nr = c["block"]
    if N >= 3:
        got["dL_dKnm_block"] = sctx.fetch_dL_dKnm(r0, nr)
    got["psi2"] = sctx.fetch(SC.FETCH_PSI2)
    got["dL_dKmm"] = sctx.fetch(SC.FETCH_DLDKMM)
    got["woodbury_inv"] = sctx.fetch(SC.FETCH_WOODBURY_INV)
    for tag in ("1", "129"):
        got["mu" + tag], got["var" + tag] = sctx.predict(c["specs"], c["Xs" + tag])
        got["cov" + tag] = sctx.predict(c["specs"], c["Xs" + tag], full_cov=True)[1]
    return got


def _check(sctx, name):
    c, ref, r64, kappa = SL.reference(name)
    try:
        got = _evaluate(sctx, c)
    except L.MI355GPError as e:          # nothing more on this device after an error of the runtime
        pytest.exit("device error in %s, the sweep ends here: %s" % (name, e), returncode=3)
    figs, bad = SL.judge(got, ref, r64, kappa)
    print()
    for q in SL.JUDGED:
        if q in figs:
            print("FIG %s %s %.2e (bound %.2e)" % (name, q, figs[q][0], figs[q][1]))
    dK = got["dL_dKmm"]
    asym = float(np.abs(dK - dK.T).max() / np.abs(dK).max())
    print("FIG %s dL_dKmm_asym %.2e" % (name, asym))
    assert not bad, bad
    assert set(figs) == set(SL.JUDGED) - (set() if c["N"] >= 3 else {"dL_dKnm_block"})
    assert asym <= 1e-13


@pytest.mark.parametrize("name", SL.PLAIN)
def test_sparse_shape_edges(name, sctx):
    _check(sctx, name)


@pytest.mark.parametrize("name", SL.BLOCKED)
def test_sparse_several_chunks(name, sctx):
    _check(sctx, name)


# Entry 256 of a part's theta record (eight records of 34 doubles, one per 32 dimensions) is the lengthscale sum of dimension
# q = 240: D = 241 is the smallest D that uses it, D = 240 the largest that does not.  Rows accumulate into the record one
# chunk at a time with a launch that must cover all of it, not its first 256 entries.  N = 70, M = 20, Dy = 1, scalar noise;
# not in sparse_ld.CASES (the CPU sweep and the bit dumps of tools/sparse_bits.py walk that list): known by name to
# sparse_ld.make_case for the length of the test.
WIDE = [SL._case("dispatch", "rbf_ard", 70, 20, D, 1) for D in (240, 241)]


@pytest.mark.parametrize("case", WIDE, ids=lambda c: c["name"])
def test_sparse_theta_record_past_256_entries(case, sctx, monkeypatch):
    monkeypatch.setitem(SL.BY_NAME, case["name"], case)
    _check(sctx, case["name"])


def test_sparse_is_deterministic_across_fresh_contexts():
    c = SL.make_case(SL.DETERMINISM)
    out = []
    for _ in range(2):
        ctx = SC(0)
        try:
            ctx.set_data(c["X"], c["R"])
            info, r = ctx.vardtc_sum(c["specs"], c["Z"], c["noise"], want_dL_dm=True)
            assert info == 0
            out.append(r)
        finally:
            ctx.close()
    assert out[0]["lml"] == out[1]["lml"]
    for q in ("dtheta", "dZ", "woodbury_vector"):
        assert np.asarray(out[0][q]).tobytes() == np.asarray(out[1][q]).tobytes(), q
