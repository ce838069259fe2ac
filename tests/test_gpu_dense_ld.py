"""GPU (-m gpu): the dense chain of `pdinv_full` -- L, L^-1, A^-1, log-determinant -- each stage judged against the DEVICE'S OWN input
to it, so that no bound has to absorb an earlier stage's error (tests/dense_ld.py, part B; tests/test_oracle_tileops.py shows on the
CPU that these judges accept LAPACK's chain and reject planted faults).  Over the lower triangle:

  L       |A - L L^T| <= gamma_{n+1} |L| |L^T| (Higham, Theorem 10.3); the strict upper triangle exactly zero.  `potrf` alone too.
  Li      the figures max |Li L - I| / (n u |Li| |L|) and the same for L Li, at most 8 times the larger of the same figure of LAPACK's
          dtrtri and of an fp64 numpy transcription of the device's recursion (128-blocks, pairwise levels), both run on the
          device's L in the same test.
  Ai      |Ai - Li^T Li| <= gamma_{n+35} |Li|^T |Li| with the device's Li; Ai == Ai.T bitwise.
  logdet  |logdet - 2 sum log L_ii| <= 2 gamma_{n+4} sum |log L_ii|, the sum in long double.

Every element of the lower triangle is held against numpy's fp64 BLAS at twice the bound; in long double at the bound itself every
element up to n = 640, above that rows and columns {0, 15, 16, 63, 64, 127} of every 128-tile and the last.  Matrix: the
Matern-5/2 ARD Gram matrix of test_gpu_linalg._spd plus shift I, shift 0.5 (and 1e-6 at n = 640, 1025).  Sizes: padding by one row
and by 127, the second outer panel, nt = 9 and 10 (the split X^T X; a trtri level with a lone trailing block).

One more test runs n = 640 and 1153 in a fresh child process on the diagnostics library with MI355GP_TRI64_MAX=0,
MI355GP_LAUUM64_MAX=0, MI355GP_UPD64_MAX=0: the 128 x 128 kernels k_trtri_stage<., 4>, k_lauum<4> take the place of their 64 x 64
forms -- and, since the persistent factorisation takes these sizes and launches no update kernel at all, once more with
MI355GP_PERSIST=0, where k_update_nt<4, true> does the trailing updates.  Same four checks.

No case failed when the file was written; the kernels are unchanged.  Measured on an MI355X (every test prints its line under -s).
chol / ainv: worst err / (2 bound) against fp64 BLAS over every element, then worst err / bound in long double; logdet: err / bound;
Li: the device's two figures (Li L, L Li), then the references' on the device's L.  Limit 1.0, for Li 8 times the larger reference.

       n  shift   chol          ainv          logdet   Li device        dtrtri           transcription
       1  0.5     0.000 0.028   0.000 0.012   0.065    0.1299 0.1299    0.1299 0.1299    0.1299 0.1299
       2  0.5     0.000 0.112   0.000 0.020   0.066    0.1895 0.1895    0.1895 0.1895    0.1895 0.1895
      64  0.5     0.061 0.066   0.022 0.065   0.002    0.0474 0.0526    0.0370 0.0557    0.0539 0.0535
     127  0.5     0.058 0.049   0.020 0.047   0.000    0.0764 0.0438    0.0217 0.0450    0.0396 0.0353
     128  0.5     0.049 0.062   0.016 0.086   0.001    0.0384 0.0365    0.0274 0.0297    0.0408 0.0307
     129  0.5     0.052 0.054   0.015 0.061   0.003    0.0415 0.0362    0.0219 0.0266    0.0427 0.0330
     255  0.5     0.037 0.041   0.010 0.058   0.001    0.0274 0.0264    0.0181 0.0190    0.0259 0.0249
     257  0.5     0.035 0.042   0.009 0.042   0.001    0.0329 0.0254    0.0213 0.0225    0.0293 0.0270
     511  0.5     0.027 0.022   0.016 0.036   0.001    0.0225 0.0191    0.0113 0.0196    0.0220 0.0178
     513  0.5     0.027 0.035   0.017 0.039   0.000    0.0294 0.0152    0.0097 0.0119    0.0265 0.0135
     640  0.5     0.025 0.025   0.013 0.032   0.000    0.0247 0.0159    0.0093 0.0130    0.0263 0.0159
    1025  0.5     0.019 0.010   0.011 0.019   0.000    0.0111 0.0089    0.0056 0.0071    0.0094 0.0078
    1153  0.5     0.016 0.012   0.010 0.022   0.001    0.0192 0.0106    0.0050 0.0064    0.0115 0.0091
     640  1e-6    0.025 0.019   0.016 0.035   0.002    0.0652 0.0212    0.0102 0.0534    0.0709 0.0225
    1025  1e-6    0.019 0.007   0.011 0.022   0.000    0.0378 0.0125    0.0069 0.0533    0.0411 0.0126

`potrf` alone: at most 0.061 (fp64) and 0.112 (long double) of the bound, the same figures as the chol column.  The child runs on
the 128 x 128 kernels, with and without the persistent factorisation, returned the default run's L, Li, Ai and log-determinant
bit for bit at both sizes (printed, not asserted: only the update kernel promises it), hence the figures of rows 640 and 1153.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import dense_ld as D
from conftest import DIAG_LIB, ROOT
from gpy_amd import _lib as L
from test_gpu_linalg import _spd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def chains():
    """(n, shift) -> (A, Ai, L, Li, logdet) of the device: computed once, never modified"""
    out = {}
    for n, shift in D.DENSE_CASES:
        A = _spd(n, seed=n, cond_shift=shift)
        Ai, Lf, Li, logdet, info = L.pdinv_full(A)
        assert info == 0
        for a in (A, Ai, Lf, Li):
            a.setflags(write=False)
        out[n, shift] = (A, Ai, Lf, Li, logdet)
    return out


def _judge(A, Ai, Lf, Li, logdet, tag=""):
    r = D.dense_report(A, Ai, Lf, Li, logdet)
    print(tag + D.report_line(r))
    n = A.shape[0]
    assert not np.isnan(Lf).any() and not np.isnan(Li).any() and not np.isnan(Ai).any()
    assert r["L_upper_zero"] and np.all(np.triu(Li, 1) == 0.0)
    for key, what in (("chol", "|A - L L^T| / (gamma_{n+1} |L||L^T|)"), ("ainv", "|Ai - Li^T Li| / (gamma_{n+35} |Li|^T|Li|)")):
        f64, ld = r[key]
        assert f64 <= 1.0, "n=%d: %s = %.3f of twice the bound against fp64 BLAS" % (n, what, f64)
        assert ld is None or ld <= 1.0, "n=%d: %s = %.3f in long double" % (n, what, ld)
    assert r["Ai_symmetric"]
    assert r["logdet"] <= 1.0, "n=%d: log-determinant %.3f of its bound" % (n, r["logdet"])
    for side, name in ((0, "Li L - I"), (1, "L Li - I")):
        ref = max(r["inv_ref"][0][side], r["inv_ref"][1][side])
        assert r["inv"][side] <= 8.0 * ref, "n=%d: %s figure %.4f, references %.4f (dtrtri) %.4f (transcription)" % (
            n, name, r["inv"][side], r["inv_ref"][0][side], r["inv_ref"][1][side])
    return r


@pytest.mark.parametrize("n,shift", D.DENSE_CASES)
def test_each_stage_of_pdinv_against_its_own_input(chains, n, shift):
    _judge(*chains[n, shift])


@pytest.mark.parametrize("n", D.DENSE_SIZES)
def test_potrf_alone_meets_the_componentwise_bound(n):
    A = _spd(n, seed=n)
    Lf, info, _ = L.potrf(A)
    assert info == 0
    ok, (f64, ld) = D.potrf_accepts(A, Lf)
    print("potrf n=%d: %.3f of twice the bound (fp64), %s of the bound (long double)" % (n, f64, ld))
    assert ok


CHILD = """import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
from gpy_amd import _lib as L
from test_gpu_linalg import _spd
out = {}
for n in (640, 1153):
    Ai, Lf, Li, logdet, info = L.pdinv_full(_spd(n, seed=n))
    assert info == 0
    out.update({"Ai%%d" %% n: Ai, "L%%d" %% n: Lf, "Li%%d" %% n: Li, "ld%%d" %% n: np.array(logdet)})
np.savez(sys.argv[1], **out)
"""


@pytest.mark.parametrize("persist", ["default", "0"])
def test_the_128_tile_kernels_at_small_sizes_in_a_child_on_the_diagnostics_library(chains, tmp_path, persist):
    f = str(tmp_path / "chain.npz")
    env = dict(os.environ, MI355GP_LIB=DIAG_LIB, MI355GP_TRI64_MAX="0", MI355GP_LAUUM64_MAX="0", MI355GP_UPD64_MAX="0")
    if persist != "default":
        env["MI355GP_PERSIST"] = persist
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests")), f], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(f)
    for n in (640, 1153):
        A, Ai0, L0, Li0, ld0 = chains[n, 0.5]
        Ai, Lf, Li, ld = got["Ai%d" % n], got["L%d" % n], got["Li%d" % n], float(got["ld%d" % n])
        print("n=%d, 128-tile kernels (persist %s): bit-identical to the default run: L %s, Li %s, Ai %s, logdet %s" % (
            n, persist, np.array_equal(Lf, L0), np.array_equal(Li, Li0), np.array_equal(Ai, Ai0), ld == ld0))
        _judge(A, Ai, Lf, Li, ld, tag="child ")
