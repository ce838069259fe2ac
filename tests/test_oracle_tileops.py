"""CPU: the judges of tests/dense_ld.py are neither vacuous nor wrong, and the binding of the debug entry they drive states its header.

Accept: for EVERY case of tests/test_gpu_tileops.py (both operand kinds) and of tests/test_gpu_dense_ld.py the judges accept the
numpy / LAPACK fp64 result of the same operation -- every element of every mask, every element of the lower triangle.
Reject: in a copy of that result, each of
    one 16-term k-slab missing from one tile             one tile computed with the neighbouring tile's k range
    one operand rounded through fp32 (one tile)          one element moved by 4 gamma mag
    one NaN                                              one changed sentinel (one bit)
Where a case has no place for a fault, nothing is planted: fp32 and 4 gamma on integer operands (integers in [-4, 4] are fp32
numbers; the integer judgement has no bound), the neighbour's range on a one-tile output (every tile of a GEMM, an update or a
Gram partial walks the same k range: there the neighbouring tile's operand rows / columns are used, the wrong tile map), a
sentinel where every output tile is computed.  A planter that returns nothing is held to exactly these reasons (NO_PLACE)."""
import ctypes
import os
import re

import numpy as np
import pytest

import dense_ld as D
from conftest import ROOT
from gpy_amd import _lib as L

CASES = D.cases()
_integers = (lambda prep: prep.kind == "int")
NO_PLACE = {"missing 16-term k-slab": lambda prep: False, "one NaN": lambda prep: False,
            "operand through fp32": _integers, "element moved by 4 gamma mag": _integers,
            "neighbour's k range": lambda prep: len(prep.pieces[-1].tiles()) == 1,
            "changed sentinel": lambda prep: bool(prep.covered.all())}


def test_the_binding_table_states_the_prototype_of_the_tileops_debug_header():
    """`_lib.DEBUG_TILEOPS_ABI` against include/mi355gp_debug_tileops.h (as tests/test_lauum_wide_map.py does for its header); the op
    numbers of `_lib.TILEOPS` against the header's MI355GP_TILEOP_* macros."""
    raw = open(os.path.join(ROOT, "include", "mi355gp_debug_tileops.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    protos = re.findall(r"\bint\s+(mi355gp_\w+)\s*\(([^)]*)\)\s*;", text)
    assert [n for n, _ in protos] == list(L.DEBUG_TILEOPS_ABI)
    assert not set(L.DEBUG_TILEOPS_ABI) & (set(L.ABI) | set(L.DEBUG_LAUUM_ABI))
    classes = {"int": (ctypes.c_int,), "int64_t": (ctypes.c_int64,), "int64_t*": (ctypes.POINTER(ctypes.c_int64),),
               "double": (ctypes.c_double,), "double*": (ctypes.POINTER(ctypes.c_double),)}
    for name, params in protos:
        types = [re.sub(r"\bconst\b|\s|\w+$", "", re.sub(r"\s*\*\s*", "* ", " ".join(p.split()))) for p in params.split(",")]
        bound = L.DEBUG_TILEOPS_ABI[name]
        assert len(types) == len(bound), name
        for c, b in zip(types, bound):
            assert b in classes[c], (name, c, b)
        assert hasattr(L.lib(), name)
    macros = {m.lower(): int(v) for m, v in re.findall(r"#define\s+MI355GP_TILEOP_(\w+)\s+(\d+)", text)}
    assert macros == {k.lower(): v for k, v in L.TILEOPS.items()}
    assert _lib_rebuild_sources_include("mi355gp_debug_tileops.h")


def _lib_rebuild_sources_include(header):
    import inspect
    return header in inspect.getsource(L.build) and header in open(os.path.join(ROOT, "gpy_amd", "csrc", "Makefile")).read()


def test_the_case_list_is_the_one_the_issue_tables():
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids))
    fam = {}
    for c in CASES:
        fam[c.family.split()[0]] = fam.get(c.family.split()[0], 0) + 1
    assert fam == {"gemm": 4 * 2 * 5 * 3, "trmm_lower": 8, "trmm_lower_T": 8, "trmm64": 4 * 4 * 2 * 2, "gram_splitk": 2 * 8 * 2,
                   "update_nt": 3 * 7, "lauum": 8}


def test_fp64_blas_on_the_integer_operands_is_the_int64_product():
    """the exactness argument of A1, checked: numpy's fp64 BLAS product of integers in [-4, 4] equals the int64 product"""
    rng = np.random.default_rng(0)
    A, B = D.draw("int", rng, (384, 3072)), D.draw("int", rng, (3072, 256))
    assert np.array_equal((A @ B).astype(np.int64), A.astype(np.int64) @ B.astype(np.int64))
    assert np.abs(A).max() == 4 and np.abs(A @ B).max() < 2 ** 53


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_judges_accept_numpy_and_reject_every_planted_fault(case):
    for kind in case.kinds:
        prep, _ = case.prepare(kind)
        good = prep.numpy_result()
        v = prep.verdict(good)
        assert D.accepts(v), (kind, v)
        assert prep.covered.any() and all(p.mask.any() for p in prep.pieces)
        if kind == "real" and D.HAVE_LD:
            assert v["ld"] is not None and 0.0 < v["ld"] <= 1.0, v     # numpy's own rounding error is seen and is inside the bound
        for name, plant in D.FAULTS.items():
            bad = plant(prep, good)
            if bad is None:                                                # nothing to plant: only for the reason given above
                assert NO_PLACE[name](prep), (kind, name)
                continue
            vb = prep.verdict(bad)
            assert not D.accepts(vb), (kind, name, vb)
            assert D.accepts(prep.verdict(good))                       # planting did not touch the good copy


# ---- part B --------------------------------------------------------------------------------------------------------
def _spd(n, shift):
    """stand-in for the Matern-5/2 ARD Gram matrix of test_gpu_linalg._spd, from numpy alone"""
    rng = np.random.default_rng(n)
    X = rng.uniform(-2.0, 2.0, (n, 3)) / np.array([0.8, 1.1, 1.9])
    r = np.sqrt(np.maximum(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1), 0.0))
    return 1.3 * (1.0 + np.sqrt(5.0) * r + 5.0 / 3.0 * r * r) * np.exp(-np.sqrt(5.0) * r) + shift * np.eye(n)


def _lapack_chain(A):
    Lf = np.linalg.cholesky(A)
    Li = D.trtri_lapack(Lf)
    Ai = Li.T @ Li
    Ai = np.tril(Ai) + np.tril(Ai, -1).T
    return Ai, Lf, Li, 2.0 * np.log(np.diag(Lf)).sum()


@pytest.mark.parametrize("n,shift", D.DENSE_CASES)
def test_dense_judges_accept_lapack_and_reject_planted_faults(n, shift):
    A = _spd(n, shift)
    Ai, Lf, Li, ld = _lapack_chain(A)
    r = D.dense_report(A, Ai, Lf, Li, ld)
    assert D.dense_accepts(r), D.report_line(r)
    assert D.potrf_accepts(A, Lf)[0]

    def rejected(Ai, Lf, Li, ld):
        return not D.dense_accepts(D.dense_report(A, Ai, Lf, Li, ld, base=r))
    assert np.allclose(D.trtri_blocked(Lf), Li, rtol=0, atol=1e-9 * np.abs(Li).max())      # the transcription inverts
    if n < 2:
        return
    i, j = n - 1, (n - 1) // 2
    # a factor with one element off by 16 roundings of its own size
    L2 = Lf.copy()
    L2[i, j] *= 1.0 + 16 * n * 2.0 ** -52
    assert rejected(Ai, L2, Li, ld)
    # an inverse factor rounded through fp32; one that lost its last block row's k range beyond the first 16 columns
    assert rejected(Ai, Lf, Li.astype(np.float32).astype(np.float64), ld)
    if n > 16:
        Li2 = Li.copy()
        Li2[i, :j] += Li[i, j] * Lf[j, :j] / Lf[j, j] * 1e-9
        assert rejected(Ai, Lf, Li2, ld)
    # A^-1 with one element moved by four bounds, with an asymmetric last bit, with a NaN; a factor with a stored upper element
    Ai2 = Ai.copy()
    Ai2[i, j] += 4.0 * float(D.gamma(n + 35)) * (np.abs(Li).T @ np.abs(Li))[i, j]
    Ai2[j, i] = Ai2[i, j]
    assert rejected(Ai2, Lf, Li, ld)
    Ai3 = Ai.copy()
    Ai3[j, i] = np.nextafter(Ai3[j, i], np.inf)
    assert rejected(Ai3, Lf, Li, ld)
    Ai4 = Ai.copy()
    Ai4[i, j] = Ai4[j, i] = np.nan
    assert rejected(Ai4, Lf, Li, ld)
    L3 = Lf.copy()
    L3[j, i] = 1e-300
    assert rejected(Ai, L3, Li, ld)
    assert rejected(Ai, Lf, Li, ld * (1.0 + 64 * n * 2.0 ** -52) + 1e-300)
