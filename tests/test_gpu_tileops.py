"""GPU (-m gpu): every launcher of the fp64 tile-GEMM family (gpy_amd/csrc/gemm.hip) ALONE, on operands the test supplies, through
the debug entries that call the product's own launchers with the product's leading dimensions: `mi355gp_dbg_gemm` (launch_gemm's
four layouts), `mi355gp_dbg_tileop` (launch_trmm_lower[_T], launch_trmm64 modes 0-3, launch_gram_splitk, launch_update_nt) and
`mi355gp_dbg_lauum` variant 2 (X^T X as `lauum_device` launches it with a default workspace: k_lauum64 up to nt = 8, the split work
list on quadrants for nt = 9, 10, 17, on 128-tiles for nt = 24).

Each case is judged three ways (tests/dense_ld.py states the bounds; tests/test_oracle_tileops.py shows on the CPU that the judges
accept numpy's result of every case and reject one lost 16-term k-slab, a neighbour's k range, an fp32 operand, one element off by
4 gamma mag, one NaN, one changed sentinel bit):
  A1  integers in [-4, 4], alpha / beta powers of two: the device equals the exact result under np.array_equal;
  A2  standard normal rows scaled by 10^U(-3, 3): every element within 2 gamma_{K+S+3} (|alpha| |A||B| + |beta| |C|) of numpy's fp64
      BLAS, sampled rows / columns {0, 15, 16, 63, 64, 127} of every tile within gamma_{K+S+3} (...) of long double;
  A3  NaN in every tile that must not be read, known values in every tile that must not be written (bit-identical afterwards), no
      NaN in what was to be computed -- in both runs.

No case failed when the file was written; the kernels are unchanged.  Measured on an MI355X (the last test prints this table under
-s), worst figure over the real-valued cases of each launcher / variant, 1.0 being the limit of either column:

    launcher / variant   cases   max err / (2 bound) against fp64 BLAS   max err / bound against long double (sample)
    gemm (4 layouts)       120                 0.183                                  0.303
    gram_splitk             32                 0.160                                  0.346
    lauum k_lauum64          4                 0.030                                  0.078
    lauum split 64           3                 0.030                                  0.080
    lauum split 128          1                 0.036                                  0.092     (sample: rows / columns 0 and 127)
    trmm64 mode 0           16                 0.025                                  0.053
    trmm64 mode 1           16                 0.031                                  0.085
    trmm64 mode 2           16                 0.019                                  0.028
    trmm64 mode 3           16                 0.022                                  0.063
    trmm_lower               8                 0.025                                  0.053
    trmm_lower_T             8                 0.031                                  0.085
    update_nt 64            15                 0.082                                  0.149
    update_nt 128            6                 0.088                                  0.157

All 221 integer runs were exact; no NaN, no changed tile outside an output.
"""
import pytest

import dense_ld as D
from gpy_amd import _lib as L

pytestmark = pytest.mark.gpu

CASES = D.cases()
WORST = {}                                                        # family -> [cases, worst fp64 figure, worst long-double figure]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_launcher_alone_exact_rounding_poison(case):
    for kind in case.kinds:
        prep, run = case.prepare(kind)
        out = run(L)
        v = prep.verdict(out)
        print("%s %s: %s" % (case.id, kind, {k: v[k] for k in ("exact", "fp64", "ld", "no_nan", "untouched")}))
        assert out.shape == prep.out0.shape
        assert v["no_nan"], "%s (%s): NaN in what was to be computed (a poisoned tile was read, or an element was not written)" % (case.id, kind)
        assert v["untouched"], "%s (%s): a tile outside the launcher's output changed" % (case.id, kind)
        if kind == "int":
            assert v["exact"] is True, "%s: the integer result is not exact" % case.id
            continue
        w = WORST.setdefault(case.family, [0, 0.0, 0.0])
        w[0] += 1
        w[1] = max(w[1], v["fp64"])
        w[2] = max(w[2], v["ld"] or 0.0)
        assert v["fp64"] <= 1.0, "%s: an element is %.3f times 2 gamma mag from numpy's fp64 result" % (case.id, v["fp64"])
        if D.HAVE_LD:
            assert v["ld"] is not None and v["ld"] <= 1.0, "%s: a sampled element is %.3f times gamma mag from long double" % (case.id, v["ld"])
            assert prep.local == (D.THIN if case.id == "lauum-24" else D.SAMPLE)


def test_zz_table_of_worst_figures():
    """prints the table of this file's docstring (run with -s): worst err / bound per launcher and variant"""
    if not WORST:                                                 # selected alone: nothing to print
        return
    print("\nlauncher / variant            cases   max err/(2 bound) vs fp64   max err/bound vs long double")
    for fam in sorted(WORST):
        n, a, b = WORST[fam]
        print("%-28s %5d   %24.3f   %28.3f" % (fam, n, a, b))
    assert all(w[1] <= 1.0 and w[2] <= 1.0 for w in WORST.values())
