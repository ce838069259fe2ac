"""GPU (-m gpu): what an exact-GP context answers after an evaluation (csrc/predict.hip: mi355gp_predict_sum,
mi355gp_predictive_gradients_sum, mi355gp_covariance_between_points) at the boundaries the code has, judged against the
long-double restatement tests/predict_ld.py (80-bit; kernels, Cholesky and solves of tests/kern_ld.py).

Families (N, M, D, Dy) and the boundary each size is there for (inputs: kern_ld.make_case with its edges -- a duplicated training
row, a new point equal to a training point, a zero row for Linear / MLP, a pair one period apart for StdPeriodic):

    kinds   (65, 63, 33, 1) alone and (129, 130, 5, 4) next to a White on active_dims {0, 2, 3}: every kind with gradients_X,
            iso and ARD (RBF, Matern52, Matern32, Exponential, RatQuad with its second records, StdPeriodic, Linear, MLP, and
            Cosine / Sinc / ExpQuadCosine on one column)
    m_edge  N = 65, D = 3, M = 1 | 63 | 64 | 65 (64 columns per workgroup of k_colreduce_multi), 128 | 129 (mp = round_up(M, 128),
            the rectangular launch_trmm_lower / _T), 257; one variant per route of part_gradients_X: rbf_ard and mlp_iso
            (generic, two host finishes), linear_ard (the weights reduced directly), stdperiodic_ard (launch_periodic_gradx, wt = 1)
    n_edge  M = 65, D = 3, Dy = 2, N = 1 | 2 | 127 | 128 | 129 (npad), 255 | 256 | 257 (the 256-row staging block), 512 | 513
            (nsplit = 1 | 2: 257 + 256 rows, combined by k_sum_splits); N < M on purpose; also the longest k_col_reduce and
            launch_gemm_tn_sq K of predict_sum that is judged in long double
    d_edge  N = 129, M = 65, D = 8 | 9, 16 | 17, 32 | 33 (template width 9 / 17 / 33 over D + 1; Linear: over D), 64 | 65
            (several launches of 32 columns; the ones column rides with the last)
    dy      N = M = 65, D = 2, Dy = 1 | 2 | 4 | 5 (k_fill_rows reads alpha[i * Dy + pass])
    sum     rbf[0, 1] + matern32_ard[1, 2, 3] + linear[0] + white + bias at (129, 65, 5, 2); column 4 belongs to no part
    covb    N = 129, D = 3, (M1, M2) = (1, 1), (1, 129), (129, 1), (63, 65), (128, 129), (130, 257), and (65, 65) at N = 513:
            launch_gemm with m1p != m2p and the copy-out with pitch m2p; RBF, Matern32 times an RBF (scratch buffers), Linear

One module-scoped context serves the sweep in list order (174 cases): whatever a call leaves behind meets the next case.  Per
case: set_data, exact_inference_sum (info == 0), predict_sum with and without full_cov, predictive_gradients with and without
the variance pass (dmu: the same bytes), covariance_between_points for the covb family; every quantity is held to

    err(q) = max |got - q_ld| / max |q_ld|  <=  max(32 e64(q), 256 eps64 kappa)

with e64 the distance of the fp64 restatement from long double on the same input (never a device figure) and kappa = cond2(Ky);
columns of dmu / dvar outside every non-static part's active_dims must be exactly 0.  tests/test_oracle_predict_ld.py shows on
the CPU that this bound never exceeds the standing 1e-9 (mu, var, cov, covb) / 1e-8 (dmu, dvar), that the restatement matches
the reference's fixtures, and that the judge rejects a dropped row, a dropped split, a lost ones column and seven more planted
faults.  Then: a stale-state sequence against fresh contexts byte for byte, the N = 513 case twice in fresh contexts byte for
byte (every reduction here is fixed-order), and the refusals by message.

Measured on an MI355X: worst err(q) over each family and, in brackets, worst err(q) / bound(q) -- the two need not come from the
same case (n_edge's 0.073 is N = 1, where kappa = 1 and the bound is 5.7e-14).  A record, never a reason to tighten a bound:

    family                    mu               var               cov               dmu              dvar              covb
    kinds       1.90e-13 (0.009)  2.20e-13 (0.011)  4.46e-13 (0.023)  2.65e-13 (0.010)  1.54e-12 (0.007)                 -
    m_edge      1.63e-13 (0.016)  3.82e-14 (0.005)  6.87e-14 (0.008)  3.32e-14 (0.009)  4.73e-14 (0.005)                 -
    n_edge      3.99e-13 (0.011)  2.60e-14 (0.014)  7.20e-14 (0.014)  8.88e-14 (0.073)  3.97e-13 (0.073)                 -
    d_edge      7.77e-14 (0.008)  1.03e-14 (0.001)  2.63e-14 (0.003)  4.99e-14 (0.015)  4.56e-14 (0.004)                 -
    dy          4.66e-14 (0.010)  1.03e-14 (0.004)  2.58e-14 (0.009)  2.20e-14 (0.008)  1.46e-14 (0.004)                 -
    sum         1.74e-14 (0.002)  2.21e-15 (0.000)  3.77e-15 (0.000)  4.49e-15 (0.000)  1.57e-15 (0.000)                 -
    covb        2.41e-13 (0.019)  8.99e-14 (0.008)  2.96e-13 (0.017)  1.48e-13 (0.021)  1.00e-13 (0.002)  6.56e-13 (0.032)

Every case passed as the code stood; no kernel or host finish needed a change.  The whole file: 177 tests, 38 s wall, nearly all of
it the long-double references (the slowest test, N = 512 with StdPeriodic, 2.3 s).  That the sweep notices mistakes on the device,
not only on the CPU's planted arrays, was tried once by hand on a scratch build with two mistakes at once: k_fill_rows reading
alpha[i] failed dmu of every case with Dy > 1 (and of none with Dy = 1), and the last row of every full 256-row block skipped in
k_colreduce_multi failed dmu and dvar of the N = 513, Dy = 1 cases.
"""
import numpy as np
import pytest

from gpy_amd import _lib as L

import kern_ld as KL
import predict_ld as P

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not KL.HAVE_LD, reason="np.longdouble is not an extended format on this host")]


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def worst():
    """{(family, q): (worst err, worst err / bound)}, printed as the docstring's table when the module is done"""
    w = {}
    yield w
    print("\n    family    " + "".join("%22s" % q for q in P.QUANTITIES))
    for f in P.FAMILIES:
        print("    %-10s" % f + "".join("%22s" % ("%.2e (%.3f)" % w[(f, q)] if (f, q) in w else "-") for q in P.QUANTITIES))


def answers(ctx, c, want_covb=True):
    """every answer of a context that holds the data and the factor of case c: dict(mu, var, cov[, dmu, dvar][, covb])"""
    dev, Xs = c["dev"], c["Xs"]
    mu, var = ctx.predict_sum(dev, Xs)
    mu2, cov = ctx.predict_sum(dev, Xs, full_cov=True)
    assert mu.tobytes() == mu2.tobytes()
    got = dict(mu=mu, var=var, cov=cov)
    if not P.has_product(c["specs"]):
        got["dmu"], got["dvar"] = ctx.predictive_gradients(dev, Xs)
    if want_covb and "X1" in c:
        got["covb"] = ctx.covariance_between_points(dev, c["X1"], c["X2"])
    return got


def fit(ctx, c):
    ctx.set_data(c["X"], c["Y"])
    info, r = ctx.exact_inference_sum(c["dev"], c["noise"])
    assert info == 0
    return r


def same_bytes(a, b):
    return sorted(a) == sorted(b) and all(a[q].shape == b[q].shape and a[q].tobytes() == b[q].tobytes() for q in a)


# ---- the sweep ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", P.NAMES)
def test_sweep(name, ctx, worst):
    c, ref, r64, kappa = P.reference(name)
    fit(ctx, c)
    got = answers(ctx, c)
    assert sorted(got) == sorted(q for q in P.QUANTITIES if q in ref)
    if "dmu" in got:                                                             # without the variance pass: the same bytes
        dmu, none = ctx.predictive_gradients(c["dev"], c["Xs"], want_var=False)
        assert none is None and dmu.tobytes() == got["dmu"].tobytes()
    figs, bad = P.judge(got, ref, r64, kappa)
    print(P.figures_line(name, kappa, figs))
    for q, (e, b) in figs.items():
        old = worst.get((c["family"], q), (0.0, 0.0))
        worst[(c["family"], q)] = (max(old[0], e), max(old[1], e / b))
    assert not bad, bad


# ---- stale state ---------------------------------------------------------------------------------------------------------------
def test_stale_state_sequence_equals_fresh_contexts(ctx):
    """predict (M = 129), predictive_gradients (M = 1), covariance_between_points (1, 129) on one context; a new inference with
    another kind (Linear: another route) on the same data; then a smaller data set and predictive_gradients (M = 65).  Every
    answer equals, byte for byte, the answer of a fresh context that did nothing else."""
    a = P.make_case("covb-rbf_ard-alone-n129_m1_d3_dy1_mm129")
    b = dict(a, **dict((k, P.make_case("covb-linear_ard-alone-n129_m1_d3_dy1_mm129")[k]) for k in ("specs", "dev")))
    s = P.make_case("m_edge-stdperiodic_ard-alone-n65_m65_d3_dy1")
    steps = [("predict", a, lambda x, c: dict(zip(("mu", "var"), x.predict_sum(c["dev"], c["X2"])))),
             ("gradients", a, lambda x, c: dict(zip(("dmu", "dvar"), x.predictive_gradients(c["dev"], c["X1"])))),
             ("covb", a, lambda x, c: dict(covb=x.covariance_between_points(c["dev"], c["X1"], c["X2"]))),
             ("predict", b, lambda x, c: dict(zip(("mu", "cov"), x.predict_sum(c["dev"], c["X2"], full_cov=True)))),
             ("gradients", b, lambda x, c: dict(zip(("dmu", "dvar"), x.predictive_gradients(c["dev"], c["X1"])))),
             ("gradients", s, lambda x, c: dict(zip(("dmu", "dvar"), x.predictive_gradients(c["dev"], c["Xs"]))))]
    stale, holds = [], None
    for what, c, call in steps:
        if holds is a and c is b:                                                # a new inference, no set_data
            info, r = ctx.exact_inference_sum(c["dev"], c["noise"])
            assert info == 0
        elif holds is not c:
            fit(ctx, c)
        holds = c
        stale.append(call(ctx, c))
    for (what, c, call), old in zip(steps, stale):
        f = L.Context(0)
        try:
            fit(f, c)
            new = call(f, c)
        finally:
            f.close()
        assert same_bytes(old, new), (what, c["name"], c["specs"][0][0])


# ---- determinism ---------------------------------------------------------------------------------------------------------------
def test_n513_twice_in_fresh_contexts_gives_the_same_bytes():
    c = P.make_case(P.DETERMINISM)
    assert c["N"] == 513
    runs = []
    for _ in range(2):
        f = L.Context(0)
        try:
            fit(f, c)
            runs.append(answers(f, c))
        finally:
            f.close()
    assert sorted(runs[0]) == ["cov", "dmu", "dvar", "mu", "var"] and same_bytes(runs[0], runs[1])


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_by_message_and_the_context_still_answers():
    rng = np.random.default_rng(12)
    N, M = 65, 7
    X, Xs = rng.standard_normal((N, 3)), rng.standard_normal((M, 3))
    X[:, 2], Xs[:, 2] = rng.integers(0, 3, N), rng.integers(0, 3, M)
    Y = rng.standard_normal((N, 1))
    rbf = lambda term: ("rbf", 1, np.array([1.1, 0.9, 1.4]), np.array([0, 1]), term)
    coreg = lambda term: ("coregionalize", 3, (np.eye(3) + 0.25).ravel(), np.array([2]), term)
    poly = ("poly", 0, np.array([0.8, 0.1, 2.0, 3.0]), np.array([0, 1]), 0)
    f = L.Context(0)
    try:
        f.set_data(X, Y)
        with pytest.raises(L.MI355GPError, match="mi355gp_predict: run an inference call first"):
            f.predict_sum([rbf(0)], Xs)
        with pytest.raises(L.MI355GPError, match="mi355gp_predictive_gradients: run an inference call first"):
            f.predictive_gradients([rbf(0)], Xs)
        with pytest.raises(L.MI355GPError, match="mi355gp_covariance_between_points: run an inference call first"):
            f.covariance_between_points([rbf(0)], Xs, Xs)
        info, r = f.exact_inference_sum([rbf(0)], 0.1)
        assert info == 0
        first = f.predictive_gradients([rbf(0)], Xs)
        with pytest.raises(L.MI355GPError, match="product kernels are not supported on the device"):
            f.predictive_gradients([rbf(1), coreg(1)], Xs)
        with pytest.raises(L.MI355GPError, match="Coregionalize .kind 8. parts are not supported on the device"):
            f.predictive_gradients([rbf(0), coreg(0)], Xs)
        with pytest.raises(L.MI355GPError, match="Poly .kind 11. has no gradients_X"):
            f.predictive_gradients([rbf(0), poly], Xs)
        again = f.predictive_gradients([rbf(0)], Xs)
        assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
        mu, var = f.predict_sum([rbf(0)], Xs)
        assert np.all(np.isfinite(mu)) and np.all(var > 0)
    finally:
        f.close()
