"""GPU: the Kronecker grid path (csrc/kron.hip, gpy_amd/kron.py) on an MI355X.

1. The mode product alone (`mi355gp_kron_mode_probe`): G in {1, 2, 3, 15, 16, 17, 63, 64, 65, 129, 257} x P in {1, 5, 63, 64, 65,
   257} with R = G, and R in {1, 16, 17} != G; Q^T read in place (transA).  Integer-valued operands small enough to be exact in
   float64 come back exact (`array_equal`); real operands are judged against long double.
2. The whole evaluation (solve, quadforms, predict, fetch) against the long-double restatement tests/kron_ld.py GIVEN THE SAME HOST
   Q AND lam, on the grids of the issue.
3. `GPRegressionGrid` against the reference's fixtures, against the dense device path on a non-integer grid, checkgrad, two
   fresh contexts, one optimize(), prediction at M in {1, 15, 16, 17, 33}.

Bounds, none of them from the device's own figures:
  * 2. and the real operands of 1.: per quantity, ten times the distance of the FLOAT64 restatement from the long-double one on
    the same inputs, computed here.
  * fixtures: per quantity, ten times the distance of the long-double restatement from the fixture, the restatement being given
    what the device is given: the model's own grid values, K_d, eigh and factors (the reference's `np.linalg.eig` vectors differ
    from eigh's by its backward error, which the fixture carries and the bound therefore has to see).
  * dense device path: ten times the distance between the two float64 CPU restatements (kron_ld and oracle/gp_oracle).

Measured on an MI355X (worst over the cases; a record, never a reason to tighten a bound): mode product 1.4e-15 (P 1, G = R = 257;
4.6 times its float64 figure at worst); whole evaluation alpha 9.6e-16, the two scalars 2.8e-16, q 3.4e-16 (8.2 times its float64
figure, the 17-point grid, the closest any quantity comes to its bound), s 1.3e-16, mu 4.8e-14, variance reduction 4.5e-16; the
model against the fixtures alpha 1.2e-14, lml 8.2e-16, gradients 1.5e-14, mu 2.1e-14, var 1.5e-13; against the dense device path
lml 4.0e-16, alpha 1.2e-14, gradients 2.2e-15, mu 3.4e-15, var 1.7e-8 (the two noise conventions).  Every case passed as the code
stood at its first run.  The whole file: 43 tests, 2 s."""
import os
import signal
import sys

import numpy as np
import pytest

import gpy_amd
from gpy_amd import _lib as L

import kron_ld as KR
from test_oracle_kron import eig_inputs, fixture_figures, model_of, model_results

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = KR.LD
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not KR.HAVE_LD, reason="np.longdouble is not an extended format on this host")]
LIMIT_S = 120


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
def ctx():
    c = L.KronContext(0)
    yield c
    c.close()


def judge(tag, got, ref_ld, ref_64, bad):
    """err(q) = max |got - q_ld| / max |q_ld| <= 10 e64(q), e64 the same figure of the float64 restatement"""
    for q in ref_ld:
        err, e64 = KR.rel_err(np.asarray(got[q], dtype=np.float64), ref_ld[q]), KR.rel_err(np.asarray(ref_64[q], dtype=np.float64), ref_ld[q])
        print("%s %-7s err %.2e  e64 %.2e  bound %.2e" % (tag, q, err, e64, 10 * e64))
        if not err <= 10 * e64:
            bad.append("%s %s: err %.3e > 10 x e64 %.3e" % (tag, q, err, e64))


# ---- 1. the mode product alone -------------------------------------------------------------------------------------------------
GS = [1, 2, 3, 15, 16, 17, 63, 64, 65, 129, 257]
PS = [1, 5, 63, 64, 65, 257]


def mode_shapes(G):
    return [(P, G, G) for P in PS] + [(P, G, R) for R in (1, 16, 17) if R != G for P in (5, 65)]


@pytest.mark.parametrize("G", GS)
def test_mode_product_of_integers_is_exact(ctx, G):
    rng = np.random.default_rng(G)
    for P, G, R in mode_shapes(G):
        A = rng.integers(-7, 8, (R, G)).astype(np.float64)
        x = rng.integers(-9, 10, (P, G)).astype(np.float64)
        want = A.astype(np.int64).dot(x.astype(np.int64).T).astype(np.float64)
        got, _ = ctx.mode_probe(A, x)
        assert got.shape == (R, P) and np.array_equal(got, want), (P, G, R)
        if R == G:
            gotT, _ = ctx.mode_probe(np.ascontiguousarray(A.T), x, transA=True)
            assert np.array_equal(gotT, want), (P, G, R, "transA")


@pytest.mark.parametrize("G", GS)
def test_mode_product_against_long_double(ctx, G):
    rng = np.random.default_rng(1000 + G)
    bad = []
    for P, G, R in mode_shapes(G):
        A, x = rng.standard_normal((R, G)), rng.standard_normal((P, G))
        ld, f64 = KR.mode(A, x, LD), KR.mode(A, x, np.float64)
        got, _ = ctx.mode_probe(A, x)
        judge("P %d G %d R %d" % (P, G, R), {"out": got}, {"out": ld}, {"out": f64}, bad)
        if R == G:
            gotT, _ = ctx.mode_probe(np.ascontiguousarray(A.T), x, transA=True)
            assert gotT.tobytes() == got.tobytes(), (P, G, R, "transA gives other bytes")
    assert not bad, "\n".join(bad)


# ---- 2. the whole evaluation, given the same host Q and lam ----------------------------------------------------------------------
GRIDS = [(1,), (17,), (129,), (16, 17), (65, 3), (3, 65), (1, 5, 1), (2, 3, 5, 7), (129, 2, 33), (64, 64, 64)]
MS = [1, 15, 16, 17, 33]


def grid_case(G, seed):
    """a grid of non-integer coordinates, its host inputs (float64 K_d, eigh, factors, gammas) and new points, some on the grid"""
    rng = np.random.default_rng(seed)
    xg = [np.sort(rng.choice(4 * g + 3, g, replace=False) * 0.37 + 0.01 * rng.random(g)) for g in G]
    D = len(G)
    ls = 1.5 + 2.0 * rng.random(D)
    variance, noise = 1.3, 0.11
    N = int(np.prod(G))
    y = rng.standard_normal(N)
    Qs, lams, factors, gammas = eig_inputs(xg, variance, ls)
    return dict(xg=xg, ls=ls, variance=variance, noise=noise, y=y, Qs=Qs, lams=lams, factors=factors, gammas=gammas, rng=rng)


def new_points(c, M):
    rng = c["rng"]
    D = len(c["xg"])
    lo, hi = np.array([x[0] for x in c["xg"]]), np.array([x[-1] for x in c["xg"]])
    Xs = lo + (hi - lo) * rng.random((M, D))
    for m in range(0, M, 3):                                    # every third point is a grid point
        Xs[m] = [x[rng.integers(x.size)] for x in c["xg"]]
    kx = KR.cross_blocks(c["xg"], Xs, c["variance"], c["ls"], np.float64)
    return Xs, kx, [k.dot(Q) for k, Q in zip(kx, c["Qs"])]


def device_evaluation(c, preds):
    """one fresh context: dict of every output, predictions included"""
    k = L.KronContext(0)
    try:
        k.set_data([x.size for x in c["xg"]], c["y"])
        yTa, sumlog = k.solve(c["Qs"], c["lams"], c["noise"] + 1e-8)
        q, s = k.quadforms(c["factors"], c["gammas"])
        out = dict(alpha=k.fetch_alpha(), yTa=yTa, sumlog=sumlog, q=q, s=s)
        for M, (_, kx, bx) in preds.items():
            out["mu%d" % M], out["red%d" % M] = k.predict(kx, bx, c["noise"])
        return out
    finally:
        k.close()


def restated(c, preds, dt):
    r = KR.evaluate(c["Qs"], c["lams"], c["y"], dt(c["noise"]) + dt(1e-8), c["factors"], c["gammas"], dt)
    out = dict((q, r[q]) for q in ("alpha", "yTa", "sumlog", "q", "s"))
    for M, (_, kx, bx) in preds.items():
        out["mu%d" % M], out["red%d" % M] = KR.predict(r["alpha"], c["lams"], kx, bx, c["noise"], dt)
    return out


def quantities(out):
    """the judged quantities of the issue's list: alpha, the two scalars, q, s, mu and the variance reduction (every M together)"""
    dt = np.result_type(*[np.asarray(v).dtype for v in out.values()])
    cat = lambda keys: np.concatenate([np.asarray(out[k], dtype=dt).ravel() for k in keys])        # noqa: E731
    return dict(alpha=out["alpha"], scalars=cat(["yTa", "sumlog"]), q=out["q"], s=out["s"],
                mu=cat(sorted(k for k in out if k.startswith("mu"))), red=cat(sorted(k for k in out if k.startswith("red"))))


@pytest.mark.parametrize("G", GRIDS, ids=lambda G: "x".join(str(g) for g in G))
def test_whole_evaluation_against_long_double(G):
    c = grid_case(G, 7 + len(G) + sum(G))
    big = int(np.prod(G)) > 100000
    preds = dict((M, new_points(c, M)) for M in ((17,) if big else MS))
    got = device_evaluation(c, preds)
    bad = []
    judge("x".join(str(g) for g in G), quantities(got), quantities(restated(c, preds, LD)), quantities(restated(c, preds, np.float64)), bad)
    assert not bad, "\n".join(bad)
    if not big:                                                # two fresh contexts give the same bytes for every output
        again = device_evaluation(c, preds)
        assert sorted(again) == sorted(got)
        for q in got:
            assert np.asarray(again[q]).tobytes() == np.asarray(got[q]).tobytes(), q


def test_sizes_out_of_range_are_refused_by_name():
    k = L.KronContext(0)
    try:
        with pytest.raises(L.MI355GPError, match=r"G\[1\] = 8193, a grid dimension has 1 to 8192 points"):
            L.check(L.lib().mi355gp_kron_set_data(k._h, 2, np.array([2, 8193], dtype=np.int64), np.zeros(4)), "mi355gp_kron_set_data")
        with pytest.raises(L.MI355GPError, match="D = 17, the grid has 1 to 16 dimensions"):
            L.check(L.lib().mi355gp_kron_set_data(k._h, 17, np.ones(17, dtype=np.int64), np.zeros(4)), "mi355gp_kron_set_data")
        with pytest.raises(L.MI355GPError, match="no data"):
            L.check(L.lib().mi355gp_kron_solve(k._h, np.zeros(1), np.zeros(1), 0.1, np.zeros(2)), "mi355gp_kron_solve")
        k.set_data([2, 2, 2, 2, 2, 2, 2, 2], np.arange(256.0))                 # D = 8 runs
        e = [np.linalg.eigh(np.array([[1.0, 0.5], [0.5, 1.0]])) for _ in range(8)]
        yTa, sumlog = k.solve([q for _, q in e], [lam for lam, _ in e], 0.1)
        assert np.isfinite(yTa) and np.isfinite(sumlog)
    finally:
        k.close()


# ---- 3. the model -----------------------------------------------------------------------------------------------------------------
def restated_like_the_model(g):
    """the long-double restatement of a fixture GIVEN WHAT THE DEVICE IS GIVEN: sorted grid values, float64 K_d, eigh, factors"""
    D = g["X"].shape[1]
    xg = [np.unique(g["X"][:, d]) for d in range(D)]
    ls = g["lengthscale"] if g["lengthscale"].size == D else np.full(D, g["lengthscale"][0])
    Qs, lams, factors, gammas = eig_inputs(xg, float(g["variance"]), ls)
    r = KR.evaluate(Qs, lams, g["Y"], LD(float(g["noise"])) + LD(1e-8), factors, gammas, LD)
    kx = KR.cross_blocks(xg, g["Xs"], float(g["variance"]), ls, np.float64)
    mu, red = KR.predict(r["alpha"], lams, kx, [k.dot(Q) for k, Q in zip(kx, Qs)], float(g["noise"]), LD)
    return dict(alpha=r["alpha"].reshape(-1, 1), lml=KR.lml_of(r, g["X"].shape[0]), grad=KR.grad_of(r), mu=mu.reshape(-1, 1),
                var=(LD(float(g["variance"])) - red).reshape(-1, 1))


@pytest.mark.parametrize("name", KR.FIXTURES)
def test_model_against_the_reference_fixtures(name):
    g = KR.load_fixture(name)
    own = fixture_figures(g, restated_like_the_model(g))
    m = model_of(g)
    figs = fixture_figures(g, model_results(m, g))
    print("fixture %-20s" % name, "  ".join("%s %.1e (bound %.1e)" % (q, figs[q], 10 * own[q]) for q in figs))
    for q in figs:
        assert figs[q] <= 10 * own[q], (q, figs[q], own[q])


@pytest.fixture(scope="module")
def nonint_pair():
    """GPRegressionGrid and the dense GPRegression on one non-integer 6 x 5 x 4 grid, noise 0.08 x variance"""
    sys.path.insert(0, ROOT)
    from oracle import gp_oracle as O
    rng = np.random.default_rng(42)
    xg = [np.array([0.1, 0.9, 1.4, 2.2, 3.1, 3.3]), np.array([0.0, 0.7, 1.1, 2.0, 2.9]), np.array([-0.5, 0.3, 1.2, 1.9])]
    X = KR.grid_of(xg)
    Y = np.sin(X[:, :1]) * np.cos(0.7 * X[:, 1:2]) + 0.3 * X[:, 2:3] + 0.25 * rng.standard_normal((X.shape[0], 1))
    variance, ls, noise = 1.5, np.array([1.1, 1.6, 0.9]), 0.12
    Xs = X.min(0) + (X.max(0) - X.min(0)) * rng.random((11, 3))
    grid = gpy_amd.GPRegressionGrid(X, Y, gpy_amd.RBF(3, variance=variance, lengthscale=ls, ARD=True))
    grid.likelihood.variance[:] = noise
    grid.parameters_changed()
    dense = gpy_amd.GPRegression(X, Y, gpy_amd.RBF(3, variance=variance, lengthscale=ls, ARD=True), noise_var=noise)
    return dict(O=O, xg=xg, X=X, Y=Y, variance=variance, ls=ls, noise=noise, Xs=Xs, grid=grid, dense=dense)


def test_model_against_the_dense_device_path(nonint_pair):
    p = nonint_pair
    O, X, Y, Xs = p["O"], p["X"], p["Y"], p["Xs"]
    # the two float64 CPU restatements on these inputs
    Qs, lams, factors, gammas = eig_inputs(p["xg"], p["variance"], p["ls"])
    r = KR.evaluate(Qs, lams, Y, p["noise"] + 1e-8, factors, gammas, np.float64)
    kx = KR.cross_blocks(p["xg"], Xs, p["variance"], p["ls"], np.float64)
    mu, red = KR.predict(r["alpha"], lams, kx, [k.dot(Q) for k, Q in zip(kx, Qs)], p["noise"], np.float64)
    a = dict(lml=KR.lml_of(r, X.shape[0], np.float64), alpha=r["alpha"].reshape(-1, 1), grad=KR.grad_of(r, np.float64),
             mu=mu.reshape(-1, 1), var=(p["variance"] - red).reshape(-1, 1) + p["noise"])
    o = O.parameters_changed("rbf", X, Y, p["variance"], p["ls"], True, p["noise"])
    omu, ovar = O.predict("rbf", X, Xs, o["L"], o["alpha"], p["variance"], p["ls"], True, noise=p["noise"])
    b = dict(lml=o["lml"], alpha=o["alpha"], grad=np.concatenate([o["dlen"], [o["dvar"]], [o["dL_dnoise"]]]), mu=omu, var=ovar)
    # the two device paths
    grid, dense = p["grid"], p["dense"]
    gm, gv = grid.predict(Xs)
    dm, dv = dense.predict(Xs)
    dg = dense.gradient                                         # [variance, lengthscales, noise]
    dev_a = dict(lml=grid.log_likelihood(), alpha=grid.posterior.alpha, mu=gm, var=gv,
                 grad=np.concatenate([grid.kern.lengthscale.gradient, grid.kern.variance.gradient, grid.likelihood.variance.gradient]))
    dev_b = dict(lml=dense.log_likelihood(), alpha=np.asarray(dense.posterior.woodbury_vector), mu=dm, var=dv,
                 grad=np.concatenate([dg[1:4], dg[:1], dg[4:]]))
    bad = []
    for q in a:
        cpu = KR.rel_err(np.asarray(a[q], dtype=np.float64).reshape(np.shape(b[q])), np.asarray(b[q], dtype=np.float64))
        dev = KR.rel_err(np.asarray(dev_a[q], dtype=np.float64).reshape(np.shape(dev_b[q])), np.asarray(dev_b[q], dtype=np.float64))
        print("dense %-6s device paths differ by %.2e, CPU restatements by %.2e (bound %.2e)" % (q, dev, cpu, 10 * cpu))
        if not dev <= 10 * cpu:
            bad.append("%s: %.3e > 10 x %.3e" % (q, dev, cpu))
    assert not bad, "\n".join(bad)


def test_checkgrad_on_the_non_integer_grid(nonint_pair):
    np.random.seed(3)
    assert nonint_pair["grid"].checkgrad(verbose=True)


def test_optimize_raises_the_log_marginal():
    rng = np.random.default_rng(8)
    xg = [np.linspace(0.0, 4.0, 19) + 0.01 * rng.random(19), np.linspace(-1.0, 2.0, 14)]
    X = KR.grid_of([np.sort(x) for x in xg])
    Y = (np.sin(1.3 * X[:, 0]) * np.cos(0.9 * X[:, 1]))[:, None] + 0.1 * rng.standard_normal((X.shape[0], 1))
    m = gpy_amd.GPRegressionGrid(X, Y, gpy_amd.RBF(2, ARD=True))
    start = m.log_likelihood()
    m.optimize(max_iters=60)
    end = m.log_likelihood()
    print("optimize: log marginal %.6f -> %.6f, noise %.4f, lengthscales %s" % (start, end, float(m.likelihood.variance[0]),
                                                                               np.asarray(m.kern.lengthscale)))
    assert end > start + 1.0 and float(m.likelihood.variance[0]) < 0.1
    mu, var = m.predict(np.array([[1.0, 0.5], [2.2, 1.1]]))
    assert np.abs(mu.ravel() - np.sin(1.3 * np.array([1.0, 2.2])) * np.cos(0.9 * np.array([0.5, 1.1]))).max() < 0.15 and (var > 0).all()


def test_the_model_never_makes_an_exact_context(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("GPRegressionGrid made an exact (N x N) context")
    monkeypatch.setattr(L.Context, "__init__", refuse)
    g = KR.load_fixture("d2_6x5_ard")
    m = model_of(g)
    m.predict(g["Xs"])
    assert m.checkgrad()
