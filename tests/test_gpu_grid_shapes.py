"""GPU (-m gpu): the 2D block-cyclic grid evaluation (csrc/grid.hip, grid_comm.hip, gpy_amd/grid.py) at the edges of its layout,
every logical rank on one device (GridContext.loopback), judged against the long-double restatement of tests/grid_ld.py (80-bit;
kernels, Cholesky and solves of tests/kern_ld.py).  The multi-process runs are held bit for bit to this loopback
(tests/test_gpu_multiproc.py), so what is judged here is judged for both.

Families (default Matern-5/2 ARD, D = 3, Dy = 2, one noise variance; T = ceil(N / nb)) and the code each edge reaches:

    n_edge   2 x 2, nb = 128, N = 1 | 2 | 127 | 128: T = 1, three ranks with TLr = 0 or TLc = 0 and nvr = 0 (the skipped branches of
             grid_build_K and grid_gradient, alloc_panel_stores' `slots * TLr + 1`, broadcasts of no tiles); 129 | 255 | 256: T = 2,
             rank (0, 1) holds only the tile above the diagonal (GridPred / GridRowTab leave it no live tile), a last tile with one
             real row, an exact multiple; 257 | 385 | 513: T = 3, 4, 5
    layout   nb = 128, N = 257 and 513 on 1x2, 2x1, 1x3, 3x1, 3x2, 2x3, 3x3, 2x4, 4x2, 1x7: T < P (1x7 and 4x2 at N = 257 have empty
             process columns / rows), T == P, wrap-around, a row communicator of seven
    subtile  nb = 256 on 2x2 and 3x2 (q = 2: the q x q sub-tiling of k_grid_gemm_multi, c_tm / a_tm tile-major addressing), N = 128
             (one whole 128-sub-tile of the only tile is identity padding) | 129 | 255 | 256 | 257 | 513; nb = 384 (q = 3) at N = 385
    d_edge   D = 1 | 32 | 33 | 65, ARD and iso: one, two, three ARD groups in gradPart / gradOut, reduced per group and all-reduced
    dy       Dy = 1 | 4 | 5: k_grid_row_reduce / k_grid_col_reduce_part / k_grid_scatter once per output column, k_grid_dldk
    kinds    RBF, Matern-3/2, Exponential, iso and ARD, on 3x2
    noise    one variance per point next to padding (k_grid_fix_diag: noise[g] by global index, 1.0 on padding): N = 257 at nb = 256,
             N = 129 at nb = 128; dnoise is the vector diag(dL_dK), the scalar the device reports is judged as its sum
    options  every (G, GW, lookahead) of test_gpu_grid.BLOCKING_OPTIONS at N = 513 (T = 5) on 2x2 and 4x2 (an empty process row at
             every step's panel), one context per layout, the options set between evaluations

Per case: set_data, exact_inference(want_diag=True) with info == 0, both fetches; every quantity held to

    err(q) = max |got - q_ld| / max |q_ld|  <=  max(32 e64(q), 256 eps64 kappa),   every dtheta entry inside kern_ld.grad_tol,

e64 from the fp64 restatement of the same input (never a device figure), kappa = cond2(K + noise + jitter) <= 1e4; L by
|A - L L^T| <= gamma_{n+1} |L||L^T| + 1e-13 v at 1.0 of the bound (fp64: of twice the bound), Linv by the two figures of
dense_ld.inv_figures at 8 times the larger reference figure on the same L; strict upper triangles exactly zero; no NaN; a second
evaluation returns the same bytes.  n_edge and layout run with check_seq = 1, and the collectives every logical rank logged are
counted against grid.expected_collectives.  tests/test_oracle_grid_ld.py shows on the CPU that this judge accepts the fp64
restatement with LAPACK's factors and rejects six planted faults, and that kappa <= 1e4 everywhere.

Then: a stale-state walk of one 2 x 2 context through N = 513, 1, 257 and N = 129 at D = 33, Dy = 5, each step judged and equal
byte for byte to a fresh context; N = 385 on 3x2 twice in fresh contexts, byte for byte; the generic code at world size 1
(diagnostics library, MI355GP_GRID_FORCE_GENERIC=1) at N = 1 | 129 | 257 (nb = 128) and 257 (nb = 256).

Measured on an MI355X: worst err(q) over each family and, in brackets, the worst err(q) / bound(q) (not necessarily from the same case);
chol, Linv L, L Linv: the worst figure and the worst figure / limit.  A record, never a reason to tighten a bound; the bounds come from
the rule above and the long-double reference alone.  lml, logdet, datafit, dnoise and trKinv are left out of the table: at most
5.6e-15 and 0.018 of the bound everywhere.

    family               alpha       diag_dL_dK           dtheta             chol           Linv L           L Linv
    n_edge     1.5e-14 (0.008)  8.9e-15 (0.005)  5.0e-16 (0.004)  1.7e-02 (0.017)  5.4e-01 (0.309)  5.5e-01 (0.295)
    layout     1.2e-14 (0.000)  8.7e-15 (0.000)  3.2e-16 (0.000)  1.5e-02 (0.015)  1.1e-01 (0.118)  2.3e-02 (0.076)
    subtile    2.1e-14 (0.001)  1.4e-14 (0.001)  2.9e-16 (0.000)  1.7e-02 (0.017)  1.8e-01 (0.267)  4.2e-02 (0.085)
    d_edge     3.0e-14 (0.007)  2.6e-14 (0.011)  2.4e-15 (0.000)  1.9e-02 (0.019)  3.2e+01 (0.201)  3.6e-02 (0.137)
    dy         1.3e-14 (0.001)  9.3e-15 (0.001)  2.4e-16 (0.000)  1.4e-02 (0.014)  9.4e-02 (0.146)  3.8e-02 (0.100)
    kinds      1.8e-14 (0.000)  1.6e-14 (0.001)  7.4e-16 (0.000)  1.4e-02 (0.014)  1.4e-01 (0.208)  2.9e-02 (0.149)
    noise      8.0e-15 (0.001)  5.6e-15 (0.000)  2.1e-16 (0.000)  1.5e-02 (0.015)  1.5e-01 (0.235)  3.2e-02 (0.088)
    options    1.2e-14 (0.000)  8.7e-15 (0.000)  2.2e-16 (0.000)  1.2e-02 (0.012)  8.6e-02 (0.118)  2.0e-02 (0.076)
    stale      1.2e-14 (0.008)  8.7e-15 (0.011)  2.2e-16 (0.001)  1.5e-02 (0.015)  1.1e-01 (0.125)  4.7e-02 (0.125)
    generic    8.1e-15 (0.008)  7.2e-15 (0.001)  2.9e-16 (0.001)  1.6e-02 (0.016)  1.8e-01 (0.267)  3.7e-02 (0.125)

Every collective count equals grid.expected_collectives; every second evaluation, the stale walk and the two fresh N = 385 runs are
byte-identical.  The whole file: 85 tests, 54 s wall on the GPU host, most of it the long-double references (the slowest test, the
first at N = 513, 2.4 s).

One case failed as the code stood, and one change to csrc/grid.hip came of it.  N = 1 (the n_edge case, and the N = 1 members of the
stale walk and of the generic-code test) missed the Linv rule alone: the device returned L = 1.18321596, Linv = 0.84515425 with
|Linv L - 1| / (n u |Linv| |L|) = 2.3477 on both sides against a limit of 8 x 0.0190 = 0.152 (dtrtri and the transcription both
return fl(1 / L)); N = 2 stood at 1.17 of a limit of 1.74.  Cause, read from csrc/potf2_asm.h (the 16 x 16 factorisation): a pivot a
gives y = rsq(a) refined by one second-order Newton step, L = a y and 1 / L = y, each about one ulp off and rounded on its own, so
D_ii L_ii - 1 is a few u where a division leaves at most one.  grid_step_diag now sets the diagonal of D = L_kk^-1 to 1 / L_ii of the
stored factor (k_grid_inv_diag, nb divisions per step); N = 1 then gives 0.0190, N = 2 0.54.  The factorisation and the triangular
inverse that every other path shares are untouched.
"""
import signal

import numpy as np
import pytest

import grid_ld as GL
import kern_ld as KL
from conftest import diag_lib
from gpy_amd import grid as G
from test_gpu_grid import _generic_1x1

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not KL.HAVE_LD, reason="np.longdouble is not an extended format on this host")]
LIMIT_S = 240
COLUMNS = GL.QUANTITIES + ("chol", "LinvL", "LLinv")
OUTPUTS = ("lml", "logdet", "datafit", "dnoise", "trKinv", "alpha", "dtheta", "diag_dL_dK")


@pytest.fixture(autouse=True)
def _time_limit():
    def stop(signum, frame):
        raise TimeoutError("test exceeded its %d s limit" % LIMIT_S)
    old = signal.signal(signal.SIGALRM, stop)
    signal.alarm(LIMIT_S)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


@pytest.fixture(scope="module")
def worst():
    """{(family, column): (worst err, worst err / bound)}, printed as the docstring's table when the module is done"""
    w = {}
    yield w
    print("\n    family    " + "".join("%19s" % q for q in COLUMNS))
    for f in GL.FAMILIES + ("stale", "generic"):
        if any(k[0] == f for k in w):
            print("    %-10s" % f + "".join("%19s" % ("%.1e (%.3f)" % w[(f, q)] if (f, q) in w else "-") for q in COLUMNS))


@pytest.fixture(scope="module")
def option_ctxs():
    """one context per layout of the options family, holding the data of its first case"""
    held = {}
    try:
        yield held
    finally:
        for g in held.values():
            g.close()


def evaluate(g, c, inp):
    """one evaluation and both fetches: (raw outputs, what the judge takes)"""
    info, res = g.exact_inference(c["kind"], c["ARD"], inp["theta"], inp["noise"], want_diag=True)
    assert info == 0
    raw = dict((q, np.array(res[q])) for q in OUTPUTS)
    raw["L"], raw["Linv"] = g.fetch(G.FETCH_L), g.fetch(G.FETCH_LINV)
    got = dict(raw)
    if c["het"]:
        got["dnoise"], got["dnoise_sum"] = raw["diag_dL_dK"], raw["dnoise"]
    return raw, got


def same_bytes(a, b):
    return sorted(a) == sorted(b) and all(a[q].shape == b[q].shape and a[q].tobytes() == b[q].tobytes() for q in a)


def judged(c, got, worst=None, failures=None):
    """judge one result; `failures`: a list that collects what failed instead of stopping at it (the walks below go on to
    their next step, and fail at their end)"""
    inp, ref, r64, kappa, A = GL.reference(c)
    figs, bad = GL.judge(got, ref, r64, kappa, A, inp["var"])
    print(GL.figures_line(c["name"], kappa, figs))
    if worst is not None:
        for q, (e, b) in figs.items():
            old = worst.get((c["family"], q), (0.0, 0.0))
            worst[(c["family"], q)] = (max(old[0], e), max(old[1], e / b))
    if failures is not None:
        failures += [(c["name"], b) for b in bad]
        return
    assert not bad, (c["name"], bad)


def check_collectives(g, c):
    for rank in range(c["Pr"] * c["Pc"]):
        log = g.coll_log(rank)
        assert dict((k, v[0]) for k, v in log.items()) == G.expected_collectives(c["N"], c["nb"], c["Pr"], c["Pc"], rank, c["Dy"], c["D"]), \
            (c["name"], rank, log)


# ---- the sweep ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GL.NAMES)
def test_case(name, worst, option_ctxs):
    c = GL.BY_NAME[name]
    inp = GL.reference(c)[0]
    if c["options"] is not None:
        key = (c["Pr"], c["Pc"])
        if key not in option_ctxs:
            option_ctxs[key] = G.GridContext.loopback(c["Pr"], c["Pc"], c["nb"])
            option_ctxs[key].set_data(inp["X"], inp["Y"])
        g = option_ctxs[key]
        for opt, v in zip(("G", "GW", "lookahead"), c["options"]):
            g.set_option(opt, v)
        assert (g.get_option("G"), g.get_option("GW"), g.get_option("lookahead")) == tuple(c["options"])
        raw, got = evaluate(g, c, inp)
        judged(c, got, worst)
        assert same_bytes(raw, evaluate(g, c, inp)[0])
        return
    g = G.GridContext.loopback(c["Pr"], c["Pc"], c["nb"])
    try:
        counted = c["family"] in ("n_edge", "layout")
        if counted:
            g.set_option("check_seq", 1)
        g.set_data(inp["X"], inp["Y"])
        raw, got = evaluate(g, c, inp)
        if counted:
            check_collectives(g, c)
        judged(c, got, worst)
        assert same_bytes(raw, evaluate(g, c, inp)[0])                             # buffers are re-initialised every evaluation
        if counted:
            check_collectives(g, c)
    finally:
        g.close()


# ---- stale state ---------------------------------------------------------------------------------------------------------------
def test_stale_walk_of_one_context_is_judged_and_equals_fresh_contexts(worst):
    """N = 513, then N = 1 (every store shrinks to one tile, three ranks lose all of theirs), then N = 257, then N = 129 with
    D = 33 (a second ARD group) and Dy = 5: each step with new data on the same 2 x 2 context."""
    g = G.GridContext.loopback(2, 2, 128)
    failures = []
    try:
        for c in GL.STALE:
            inp = GL.reference(c)[0]
            g.set_data(inp["X"], inp["Y"])
            raw, got = evaluate(g, c, inp)
            judged(c, got, worst, failures)
            f = G.GridContext.loopback(2, 2, 128)
            try:
                f.set_data(inp["X"], inp["Y"])
                fresh = evaluate(f, c, inp)[0]
            finally:
                f.close()
            assert same_bytes(raw, fresh), c["name"]
    finally:
        g.close()
    assert not failures, failures


# ---- determinism ---------------------------------------------------------------------------------------------------------------
def test_n385_on_3x2_twice_in_fresh_contexts_gives_the_same_bytes():
    c = GL.DETERMINISM
    assert (c["N"], c["Pr"], c["Pc"]) == (385, 3, 2)
    inp = GL.make_inputs(c)
    runs = []
    for _ in range(2):
        g = G.GridContext.loopback(c["Pr"], c["Pc"], c["nb"])
        try:
            g.set_data(inp["X"], inp["Y"])
            runs.append(evaluate(g, c, inp)[0])
        finally:
            g.close()
    assert sorted(runs[0]) == sorted(OUTPUTS + ("L", "Linv")) and same_bytes(runs[0], runs[1])


# ---- the generic code at world size 1 -------------------------------------------------------------------------------------------
@diag_lib
def test_the_generic_code_on_a_1x1_grid_at_the_padding_edges(worst):
    _generic_1x1(True)
    failures = []
    try:
        for c in GL.GENERIC:
            inp = GL.reference(c)[0]
            g = G.GridContext.loopback(1, 1, c["nb"])
            try:
                g.set_option("check_seq", 1)
                g.set_data(inp["X"], inp["Y"])
                raw, got = evaluate(g, c, inp)
                check_collectives(g, c)                                            # fails on the single-GPU pipeline: it keeps no log
                judged(c, got, worst, failures)
                assert same_bytes(raw, evaluate(g, c, inp)[0])
            finally:
                g.close()
    finally:
        _generic_1x1(False)
    assert not failures, failures
