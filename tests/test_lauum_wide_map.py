"""CPU: the work list of X^T X on 128 x 256 tiles (gpy_amd/csrc/lauum_policy.h, `k_lauum_wide` in gemm.hip) through the host-only
entry `mi355gp_dbg_lauum_wide_map`: every 128-block on or below the diagonal exactly once, none above it, K uniform inside an item
and equal to the rows below the item's tile row, longest K first; and the policy keeps the 128 x 128 tile below its threshold."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from gpy_amd import _lib as L


def test_the_binding_table_states_the_prototypes_of_the_lauum_debug_header():
    """`_lib.DEBUG_LAUUM_ABI` against include/mi355gp_debug_lauum.h: the same functions in the same order, every parameter of the
    ctypes class that passes the declared C type, every one exported by the built library."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi355gp_debug_lauum.h")).read(), flags=re.S)
    protos = re.findall(r"\bint\s+(mi355gp_\w+)\s*\(([^)]*)\)\s*;", text)
    assert [n for n, _ in protos] == list(L.DEBUG_LAUUM_ABI) and not set(L.DEBUG_LAUUM_ABI) & set(L.ABI)
    classes = {"int": (ctypes.c_int,), "int64_t": (ctypes.c_int64,), "int*": (ctypes.POINTER(ctypes.c_int),),
               "double*": (ctypes.POINTER(ctypes.c_double),)}
    for name, params in protos:
        types = [re.sub(r"\bconst\b|\s|\w+$", "", re.sub(r"\s*\*\s*", "* ", " ".join(p.split()))) for p in params.split(",")]
        bound = L.DEBUG_LAUUM_ABI[name]
        assert len(types) == len(bound), name
        for c, b in zip(types, bound):
            assert b in classes[c], (name, c, b)
        assert hasattr(L.lib(), name)


@pytest.mark.parametrize("nt", range(1, 41))
def test_every_lower_block_exactly_once(nt):
    items, _, _ = L.lauum_wide_map(nt)
    seen = np.zeros((nt, nt), dtype=int)
    for ti, tj, ncb, K in items:
        assert ncb in (1, 2) and 0 <= tj and tj + ncb - 1 <= ti < nt, (ti, tj, ncb)
        assert K == (nt - ti) * 128
        assert tj % 2 == 0                                       # a pair is {2j, 2j + 1}
        if ncb == 1:
            assert tj == ti and ti % 2 == 0                      # alone: the diagonal block of an even tile row
        seen[ti, tj:tj + ncb] += 1
    assert np.array_equal(seen, np.tril(np.ones((nt, nt), dtype=int)))
    assert np.all(np.diff(items[:, 3]) <= 0), "items are enumerated longest K first"
    assert len(items) == sum(ti // 2 + 1 for ti in range(nt))


def test_policy_keeps_the_shipped_tile_below_its_threshold():
    _, _, thr = L.lauum_wide_map(1)
    assert thr > 44, "the 64 x 64 quadrants (nt <= 32) and the split work list (nt <= 44) keep their ranges"
    for nt in range(1, thr):
        assert L.lauum_wide_map(nt)[1] is False
    for nt in (thr, thr + 1, 128, 256):
        assert L.lauum_wide_map(nt)[1] is True
