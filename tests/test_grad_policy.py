"""CPU: which launches of the gradient pass take the tile-GEMM kernel (gpy_amd/csrc/grad_policy.h, `grad_tilegemm_applies`).
The header is plain C++; a stand-alone program built with the host compiler prints the decision for a table of cases."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpy_amd", "csrc")
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")

RBF, M52, M32, EXPONENTIAL, WHITE, BIAS, RATQUAD, LINEAR = 0, 1, 2, 3, 4, 5, 6, 9
#        fused kind ard mul hout rank w_addr ldw force_old   taken
TABLE = [(1, RBF, 1, 0, 0, 0, 4096, 16384, 0, 1),
         (1, M52, 1, 0, 0, 0, 4096, 128, 0, 1),
         (1, M32, 1, 0, 0, 0, 64, 64, 0, 1),
         (1, M52, 1, 0, 0, 0, 4096, 16384, 1, 0),          # the A/B switch
         (0, M52, 1, 0, 0, 0, 4096, 16384, 0, 0),          # generic / sparse pass
         (1, M52, 0, 0, 0, 0, 4096, 16384, 0, 0),          # iso
         (1, EXPONENTIAL, 1, 0, 0, 0, 4096, 16384, 0, 0),  # stays on k_grad (registers)
         (1, WHITE, 1, 0, 0, 0, 4096, 16384, 0, 0),
         (1, BIAS, 1, 0, 0, 0, 4096, 16384, 0, 0),
         (1, RATQUAD, 1, 0, 0, 0, 4096, 16384, 0, 0),
         (1, LINEAR, 1, 0, 0, 0, 4096, 16384, 0, 0),
         (1, RBF, 1, 1, 0, 0, 4096, 16384, 0, 0),          # factor of a product
         (1, RBF, 1, 0, 1, 0, 4096, 16384, 0, 0),          # gradients_X weights go out
         (1, RBF, 1, 0, 0, 1, 4096, 16384, 0, 0),          # rank term
         (1, RBF, 1, 0, 0, 0, 4096 + 8, 16384, 0, 0),      # weights not 32-byte aligned
         (1, RBF, 1, 0, 0, 0, 4096 + 16, 16384, 0, 0),
         (1, RBF, 1, 0, 0, 0, 4096, 130, 0, 0)]            # rows not 32-byte aligned

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "grad_policy.h"
int main(int argc, char** argv) {
    for (int i = 1; i + 8 < argc; i += 9) {
        GradLaunchCase c{atoi(argv[i]), atoi(argv[i + 1]), atoi(argv[i + 2]), atoi(argv[i + 3]), atoi(argv[i + 4]), atoi(argv[i + 5]),
                         (uintptr_t)atol(argv[i + 6]), atol(argv[i + 7]), atoi(argv[i + 8])};
        std::printf("%d\n", grad_tilegemm_applies(c) ? 1 : 0);
    }
    return 0;
}
"""


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_tilegemm_policy_table(tmp_path):
    src = tmp_path / "policy_main.cpp"
    src.write_text(MAIN)
    exe = str(tmp_path / "policy_main")
    r = subprocess.run([CXX, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    args = [str(v) for row in TABLE for v in row[:9]]
    out = subprocess.run([exe] + args, capture_output=True, text=True, check=True).stdout.split()
    assert [int(o) for o in out] == [row[9] for row in TABLE]
