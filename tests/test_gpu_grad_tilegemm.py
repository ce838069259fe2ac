"""GPU (-m gpu): the fused ARD gradient pass in its tile-GEMM form (csrc/kern.hip `k_grad_tilegemm`: interior-tile fast path,
per-dimension reduction expanded about a per-tile centre with P = T V on the fp64 MFMA) against the long-double restatement
tests/kern_ld.py.

Quantity: max |grad - ref| / max |ref| over (variance, lengthscales, noise), through `Context.exact_inference` and through
`GPRegression`; bound 1e-8, the project's gradient gate.

Shapes: N in {64, 65, 128, 129, 192, 200} (192, 200: interior tiles; 129, 200: edge tiles; every N: diagonal tiles), D in {1, 15,
16, 17, 32, 33, 40} (one / two blocks of 16 dimensions with and without zero padding, a second launch group), Dy in {1, 3}, kinds
rbf / matern32 / matern52, ARD.  The whole N x D grid runs with (kind, Dy, data) rotating through their 18 combinations; all 18
run at (200, 33) and (192, 32).

Data that attack the centring:
  offset : every dimension 1e4 + N(0, 1) -- the expansion u^2 R + v^2 C - 2 u P cancels catastrophically unless centred per tile
  sorted : 100 + 3 N(0, 1), points sorted along dimension 0 -- tiles are compact and far from the origin
  dups   : N(0, 1) with exact duplicates (inside a tile and across tiles) and pairs 1e-9 apart

Reproducibility: two fresh contexts give identical bytes; with MI355GP_GRAD_TILEGEMM=0 (diagnostics build) the launch takes
`k_grad` and gives the bytes recorded from the parent build (tests/golden/grad_tilegemm/parent.npz).

Measured on an MI355X, worst figure per data set, new path / parent build: profiles/grad_tilegemm_bits.txt."""
import os

import numpy as np
import pytest

import gpy_amd
from gpy_amd import _lib as L

import kern_ld as KL
from conftest import diag_lib

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not KL.HAVE_LD, reason="np.longdouble is not an extended format on this host")]
HERE = os.path.dirname(os.path.abspath(__file__))
PARENT = os.path.join(HERE, "golden", "grad_tilegemm", "parent.npz")
TOL = 1e-8
NS, DS, DYS = (64, 65, 128, 129, 192, 200), (1, 15, 16, 17, 32, 33, 40), (1, 3)
KINDS, DATA = ("rbf", "matern32", "matern52"), ("offset", "sorted", "dups")
COMBOS = [(k, dy, d) for k in KINDS for dy in DYS for d in DATA]
CASES = [(n, d) + COMBOS[(7 * i + j) % len(COMBOS)] for i, n in enumerate(NS) for j, d in enumerate(DS)]
CASES += [(n, d) + c for n, d in ((200, 33), (192, 32)) for c in COMBOS if (n, d) + c not in CASES]
IDS = ["n%d_d%d_%s_dy%d_%s" % c for c in CASES]
REPRO = [(200, 33, "matern52", 1, "offset"), (192, 32, "rbf", 3, "sorted"), (129, 17, "matern32", 1, "dups")]
CLS = {"rbf": gpy_amd.RBF, "matern32": gpy_amd.Matern32, "matern52": gpy_amd.Matern52}


def make(case):
    """(X, Y, theta = [variance, lengthscales], noise) of one case, seeded by the case"""
    n, d, kind, dy, data = case
    rng = np.random.default_rng([n, d, KINDS.index(kind), dy, DATA.index(data)])
    X = rng.standard_normal((n, d))
    if data == "offset":
        X = X + 1e4
    elif data == "sorted":
        X = 100.0 + 3.0 * X
        X = X[np.argsort(X[:, 0])]
    else:
        X[1] = X[0]                            # duplicates: neighbours in a tile, and rows of different tiles
        X[n - 1] = X[3]
        X[5] = X[4] + 1e-9                     # pairs 1e-9 apart: inside a tile and across tiles
        X[n - 2] = X[n // 2 - 1] + 1e-9
    scale = 3.0 if data == "sorted" else 1.0
    theta = np.concatenate([[1.3], scale * np.sqrt(d) * rng.uniform(0.8, 1.6, d)])
    return X, rng.standard_normal((n, dy)), theta, 0.1


_REF = {}


def reference(case):
    """[dvariance, dlengthscales, dnoise] in long double, computed once per case"""
    if case not in _REF:
        X, Y, theta, noise = make(case)
        ex = KL.exact([(case[2], 1, theta, np.arange(case[1]), 0)], X, Y, noise, max_n=200)
        _REF[case] = np.concatenate([np.asarray(ex["dtheta"]).ravel(), [ex["dnoise"]]])
    return _REF[case]


def device(ctx, case):
    X, Y, theta, noise = make(case)
    ctx.set_data(X, Y)
    info, r = ctx.exact_inference(case[2], True, theta, noise)
    assert info == 0
    return np.concatenate([r["dtheta"], [r["dnoise"]]])


def figure(got, ref):
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gradient_against_long_double(case, ctx):
    ref = reference(case)
    f_ctx = figure(device(ctx, case), ref)
    X, Y, theta, noise = make(case)
    m = gpy_amd.GPRegression(X, Y, CLS[case[2]](case[1], variance=theta[0], lengthscale=theta[1:], ARD=True), noise_var=noise)
    f_model = figure(np.asarray(m.gradient), ref)
    print("FIG %s context %.2e model %.2e" % ("n%d_d%d_%s_dy%d_%s" % case, f_ctx, f_model))
    assert f_ctx <= TOL and f_model <= TOL


@pytest.mark.parametrize("case", REPRO, ids=["n%d_d%d_%s_dy%d_%s" % c for c in REPRO])
def test_two_fresh_contexts_give_identical_bytes(case):
    out = []
    for _ in range(2):
        c = L.Context(0)
        out.append(device(c, case).tobytes())
        c.close()
    assert out[0] == out[1]


@diag_lib
def test_forced_old_path_gives_the_parent_builds_bytes():
    os.environ["MI355GP_GRAD_TILEGEMM"] = "0"          # read once, at the first gradient launch of this (child) process
    gold = np.load(PARENT)
    c = L.Context(0)
    try:
        for case in REPRO:
            got = device(c, case)
            assert got.tobytes() == gold["n%d_d%d_%s_dy%d_%s" % case].tobytes(), case
    finally:
        c.close()
