"""CPU: the cases, the reference and the judge of tests/grid_ld.py (what tests/test_gpu_grid_shapes.py holds the block-cyclic grid
evaluation to) are what the table says, are neither vacuous nor wrong, and the host-side index algebra of gpy_amd/grid.py holds at
every edge of the table.

Condition  kappa = cond2(K + noise + jitter) <= 1e4 for every case, so that the 256 eps64 kappa arm of the bound stays below
           6e-10 and cannot hide a wrong tile.
Accept     the fp64 restatement, with LAPACK's Cholesky factor and dtrtri's inverse in the place of the fetched L and L^-1,
           passes the judge for every reference with N <= 257 and for the one at N = 513.
Reject     planted into a copy of that result at N = 257 (nb = 128, 2 x 2; the per-point noise case at nb = 256):
               one nb-tile of Ki missing from trKinv / diag_dL_dK        one padding row counted in logdet
               alpha without one rank's partial sum                     one ARD group (dimensions 32 ..) dropped from dtheta (D = 33)
               noise[0] used for every row (per-point noise)            one 16-term k-slab missing from one 128 x 128 tile of L
Index      for every (N, nb, Pr, Pc) of the table: local_tiles / tile_owner / global_index / count_le partition tiles and
           indices exactly once, empty ranks included; expected_collectives is never negative, equals a count by plain
           enumeration of the tiles, and agrees between the members of one process row (row communicator) and of one process
           column (column communicator), who take part in the same broadcasts."""
import numpy as np
import pytest

import grid_ld as GL
import kern_ld as KL
from gpy_amd import grid as G
from test_gpu_grid import BLOCKING_OPTIONS

needs_ld = pytest.mark.skipif(not KL.HAVE_LD, reason="np.longdouble is not an extended format on this host")


def test_the_case_list_is_the_one_the_issue_tables():
    fam = {}
    for c in GL.CASES:
        fam[c["family"]] = fam.get(c["family"], 0) + 1
    assert fam == {"n_edge": 10, "layout": 20, "subtile": 13, "d_edge": 8, "dy": 3, "kinds": 6, "noise": 2,
                   "options": 2 * len(BLOCKING_OPTIONS)}
    assert tuple(fam) == GL.FAMILIES
    assert max(c["N"] for c in GL.CASES + GL.STALE + GL.GENERIC) <= GL.MAX_N and max(c["Pr"] * c["Pc"] for c in GL.CASES) == 9
    assert [c["N"] for c in GL.STALE] == [513, 1, 257, 129] and (GL.STALE[3]["D"], GL.STALE[3]["Dy"]) == (33, 5)
    for name in (GL.FAULT_CASE, GL.FAULT_CASE_D33, GL.FAULT_CASE_HET, GL.ACCEPT_513):
        assert name in GL.BY_NAME
    # the reference never depends on the layout: at most three distinct ones at N = 513 (here: one)
    big = set(GL.ref_key(c) for c in GL.CASES + GL.STALE + GL.GENERIC + [GL.DETERMINISM] if c["N"] == 513)
    assert 1 <= len(big) <= 3
    assert len(set(GL.ref_key(c) for c in GL.CASES if c["family"] in ("layout", "options"))) == 2
    # what the edges are there for
    T = lambda c: -(-c["N"] // c["nb"])                                          # noqa: E731
    assert any(T(c) == 1 and c["Pr"] * c["Pc"] == 4 for c in GL.CASES)          # three ranks without a tile
    assert any(T(c) < c["Pc"] for c in GL.CASES) and any(T(c) < c["Pr"] for c in GL.CASES) and any(T(c) == c["Pr"] == c["Pc"] for c in GL.CASES)
    assert any(c["N"] % c["nb"] == 1 and c["nb"] == 256 for c in GL.CASES) and any(c["nb"] == 384 for c in GL.CASES)
    assert all(T(c) == 5 for c in GL.CASES if c["options"]) and any(2 * o[0] > 5 and 5 % o[0] for o in BLOCKING_OPTIONS)


@pytest.mark.parametrize("name", GL.NAMES + [c["name"] for c in GL.STALE + GL.GENERIC])
def test_kappa_stays_below_1e4(name):
    c = dict((x["name"], x) for x in GL.CASES + GL.STALE + GL.GENERIC)[name]
    kappa = GL.kappa_of(c)
    assert 1.0 <= kappa <= GL.KAPPA_MAX, kappa
    assert 256.0 * KL.EPS64 * kappa < 6e-10


def _accept_keys():
    seen, out = set(), []
    for c in GL.CASES + GL.STALE + GL.GENERIC:
        k = GL.ref_key(c)
        if k not in seen and (c["N"] <= 257 or c["name"] == GL.ACCEPT_513):
            seen.add(k)
            out.append(c["name"])
    return out


ALL = dict((c["name"], c) for c in GL.CASES + GL.STALE + GL.GENERIC)


@needs_ld
@pytest.mark.parametrize("name", _accept_keys())
def test_the_judge_accepts_the_fp64_restatement_with_lapack_factors(name):
    c = ALL[name]
    inp, ref, r64, kappa, A = GL.reference(c)
    got = GL.lapack_result(c)
    figs, bad = GL.judge(got, ref, r64, kappa, A, inp["var"])
    assert not bad, (bad, GL.figures_line(name, kappa, figs))
    assert sorted(q for q in figs if q in GL.QUANTITIES) == sorted(GL.QUANTITIES)
    assert figs["chol"][0] <= 1.0 and (c["N"] < 2 or figs["chol"][0] > 0.0)      # LAPACK's own rounding is seen, inside the bound
    if c["het"]:
        assert np.shape(ref["dnoise"]) == (c["N"],) and "dnoise_sum" in figs
    # the bound is the rule, not a figure of this run: the larger of its two arms, e64 from the two restatements alone
    for q in GL.QUANTITIES:
        assert figs[q][1] == max(32.0 * GL.rel_err(r64[q], ref[q]), 256.0 * KL.EPS64 * kappa)


@needs_ld
@pytest.mark.parametrize("fault", list(GL.FAULTS))
def test_the_judge_rejects_every_planted_fault(fault):
    name, plant = GL.FAULTS[fault]
    c = GL.BY_NAME[name]
    assert c["N"] == 257 and (c["Pr"], c["Pc"]) == (2, 2)
    inp, ref, r64, kappa, A = GL.reference(c)
    good = GL.lapack_result(c)
    assert not GL.judge(good, ref, r64, kappa, A, inp["var"])[1]
    bad = plant(c, inp, r64, good)
    figs, why = GL.judge(bad, ref, r64, kappa, A, inp["var"])
    assert why, (fault, GL.figures_line(name, kappa, figs))
    print(fault, "->", why)
    assert not GL.judge(good, ref, r64, kappa, A, inp["var"])[1]                 # planting did not touch the good copy


@needs_ld
def test_a_nan_a_stored_upper_element_and_a_missing_quantity_are_refused():
    c = GL.BY_NAME[GL.FAULT_CASE]
    inp, ref, r64, kappa, A = GL.reference(c)
    for q, idx in (("alpha", (5, 1)), ("L", (200, 3)), ("Linv", (256, 256))):
        bad = GL.lapack_result(c)
        bad[q][idx] = np.nan
        assert GL.judge(bad, ref, r64, kappa, A, inp["var"])[1]
    for q in ("L", "Linv"):
        bad = GL.lapack_result(c)
        bad[q][3, 200] = 1e-300
        assert GL.judge(bad, ref, r64, kappa, A, inp["var"])[1]
    bad = GL.lapack_result(c)
    bad["trKinv"] = None
    assert GL.judge(bad, ref, r64, kappa, A, inp["var"])[1]


# ---- index algebra at the edges ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,nb,Pr,Pc", GL.shapes())
def test_the_tile_maps_partition_tiles_and_indices_exactly_once(N, nb, Pr, Pc):
    T = -(-N // nb)
    owned = {}
    for rank in range(Pr * Pc):
        pr, pc = G.rank_coords(rank, Pc)
        rows, cols = G.local_tiles(T, pr, Pr), G.local_tiles(T, pc, Pc)
        assert len(rows) == G.count_le(T - 1, pr, Pr) and len(cols) == G.count_le(T - 1, pc, Pc)        # 0 on an empty rank
        for li, I in enumerate(rows):
            assert I % Pr == pr and li == G.count_le(I, pr, Pr) - 1
            for lj, J in enumerate(cols):
                assert G.tile_owner(I, J, Pr, Pc) == rank
                assert (I, J) not in owned
                owned[(I, J)] = rank
    assert sorted(owned) == [(I, J) for I in range(T) for J in range(T)]
    for P in (Pr, Pc):
        seen = []
        for p in range(P):
            n_loc = len(G.local_tiles(T, p, P)) * nb
            g = [G.global_index(l, p, P, nb) for l in range(n_loc)]
            assert g == sorted(g)                                                     # the real rows are a prefix of the local order
            seen += g
        assert sorted(seen) == list(range(T * nb))


def _enumerated_collectives(N, nb, Pr, Pc, rank):
    """the count of expected_collectives from a plain enumeration of the tiles (csrc/grid.hip, steps (b), (d), (e), (h), (i))"""
    T = -(-N // nb)
    pr, pc = G.rank_coords(rank, Pc)
    row = col = 0
    for k in range(T):
        col += pc == k % Pc                                                           # (b)
        row += pr == k % Pr
        row += any(I % Pr == pr for I in range(k + 1, T))                             # (d)
        col += len(set(J % Pr for J in range(k + 1, T) if J % Pc == pc))              # (e) one per root process row
        col += any(J % Pc == pc for J in range(k + 1))                                # (h)
        row += len(set(I % Pc for I in range(k + 1) if I % Pr == pr))                 # (i) one per root process column
    return {"world": 5, "row": int(row), "col": int(col)}


@pytest.mark.parametrize("N,nb,Pr,Pc", GL.shapes())
def test_expected_collectives_is_consistent_at_every_edge(N, nb, Pr, Pc):
    exp = [G.expected_collectives(N, nb, Pr, Pc, r, 2, 3) for r in range(Pr * Pc)]
    T = -(-N // nb)
    for r, e in enumerate(exp):
        assert e["world"] == 5 and e["row"] >= 0 and e["col"] >= 0
        assert e == _enumerated_collectives(N, nb, Pr, Pc, r)
        assert e == G.expected_collectives(N, nb, Pr, Pc, r, 5, 65)                   # not a matter of Dy or D
        assert e["row"] <= T * (2 + Pc) and e["col"] <= T * (2 + Pr)
    for pr in range(Pr):                                                              # one row communicator: the same broadcasts
        assert len(set(exp[pr * Pc + pc]["row"] for pc in range(Pc))) == 1
    for pc in range(Pc):
        assert len(set(exp[pr * Pc + pc]["col"] for pr in range(Pr))) == 1
    # every step broadcasts D once down one process column and once along one process row
    assert sum(e["col"] for e in exp) >= T * Pr and sum(e["row"] for e in exp) >= T * Pc
