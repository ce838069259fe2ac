"""CPU: the long-double restatement of the sparse evaluations with a Linear part (tests/sparse_lin_ld.py) proves itself three ways
before the GPU test judges the device by it:

 (a) central differences of its own bound in long double, for every parameter class -- stationary theta, the Linear variances,
     White, the noise, Z -- for VarDTC (scalar and per-point noise), PEP / FITC, and SVGP (of S = sum dF_dmu mu + sum dF_dv v - KL
     at fixed weights, whose gradient the backward pass is).  Step h = 1e-5 |parameter| (1e-6, absolute, for Z, whose scale is a
     lengthscale of 0.4): the truncation error of a central difference is h^2 times a third derivative over 6, 1e-10 relative
     or so, the rounding error eps_ld / h ~ 1e-13; held to 1e-8 of the largest gradient entry of the class.  Observed here: at
     most 3.1e-9 (the White variance of the SVGP case, whose gradient is small against the class's), 1.2e-10 elsewhere.
 (b) the fixtures of the reference's own VarDTC / FITC / PEP / SVGP / EPDTC (recorded update orders) evaluations (tests/golden/sparse_lin/*.npz), restated at fp64:
     1e-9 of each quantity's largest entry (both sides are fp64 evaluations of problems with kappa <= 181; observed at most 6e-13).
 (c) a lone Linear part with M <= D against a dense evaluation of the same model, log N(y | 0, Qnn + s2 I) - tr(Knn - Qnn) / (2 s2)
     with Qnn = Knm (Kmm + 1e-8 I)^-1 Kmn from N x N factorisations in long double: 1e-13 (observed 4e-16); and, since Z spans the
     input space, Qnn = Knn up to the jitter and the bound is the exact GP's log marginal to 1e-6.

It also shows what the helper is for: sparse_ld.vardtc with "linear" admitted and nothing else changed gives the Linear variances
a gradient that central differences contradict."""
import numpy as np
import pytest

import kern_ld as KL
import sparse_ld as SL
import sparse_lin_ld as LL
import svgp_np as SN

LD = KL.LD
need_ld = pytest.mark.skipif(not KL.HAVE_LD, reason="np.longdouble is not an extended format on this host")
CD_TOL = 1e-8


def _problem(het=False, Dy=1):
    rng = np.random.default_rng(17)
    N, M, D = 40, 9, 3
    X, Z = rng.uniform(-0.5, 0.5, (N, D)), rng.uniform(-0.5, 0.5, (M, D))
    allq = np.arange(D, dtype=np.int32)
    specs = [("rbf", 1, np.array([1.3, 0.4, 0.5, 0.6]), allq, 0), LL.linear_part(allq, 1), ("linear", 0, np.array([0.3]), allq[:2], 1),
             ("matern32", 0, np.array([0.8, 0.7]), allq[2:], 1), ("white", 0, np.array([0.05]), allq, 0)]
    Y = np.sin(3 * X[:, :1]) + X[:, 1:2] + 0.1 * rng.standard_normal((N, Dy))
    noise = 0.03 + 0.1 * rng.uniform(0, 1, N) if het else 0.07
    return specs, X, Z, Y, noise


def _with_theta(specs, flat):
    out, k = [], 0
    for s in specs:
        n = KL.n_params(s)
        out.append((s[0], s[1], np.array(flat[k:k + n], dtype=np.float64), s[3], s[4]))
        k += n
    return out


def _central(f, x, h):
    """d f / d x_i by central differences in long double; x is fp64 (the restatements take fp64 inputs), the steps are exact"""
    x = np.asarray(x, np.float64)
    g = np.zeros(x.size, dtype=LD)
    for i in range(x.size):
        e = np.zeros(x.size)
        e[i] = h * max(abs(x.flat[i]), 1e-300) if h < 0 else h
        step = abs(e[i])
        hi, lo = (x.ravel() + e).reshape(x.shape), (x.ravel() - e).reshape(x.shape)
        g[i] = (LD(f(hi)) - LD(f(lo))) / (LD(hi.ravel()[i]) - LD(lo.ravel()[i]))
        assert step > 0
    return g


def _held(name, got, fd, classes):
    worst = 0.0
    for cls, idx in classes.items():
        err = float(np.max(np.abs(KL._a(got, LD)[idx] - fd[idx])) / np.max(np.abs(fd[idx])))
        print("CD %s %s %.2e" % (name, cls, err))
        assert err <= CD_TOL, (name, cls, err)
        worst = max(worst, err)
    return worst


THETA_CLASSES = {"stationary": np.r_[0:4, 8:10], "linear_variances": np.r_[4:8], "white": np.r_[10:11]}


@need_ld
@pytest.mark.parametrize("het,Dy", [(False, 1), (True, 1), (True, 2)])
def test_vardtc_gradients_agree_with_central_differences(het, Dy):
    specs, X, Z, Y, noise = _problem(het, Dy)
    r = LL.vardtc(specs, X, Z, Y, noise)
    th = np.concatenate([s[2] for s in specs])
    fd = _central(lambda t: LL.vardtc(_with_theta(specs, t), X, Z, Y, noise)["lml"], th, -1e-5)
    _held("vardtc", r["dtheta"], fd, THETA_CLASSES)
    fdZ = _central(lambda z: LL.vardtc(specs, X, z, Y, noise)["lml"], Z, 1e-6)
    _held("vardtc", r["dZ"].ravel(), fdZ, {"Z": np.r_[0:Z.size]})
    if het and Dy > 1:
        return                           # (var_dtc.py:240-256 as written is no derivative of the bound for several columns: the
                                         #  restatement follows the reference there, and the fixtures hold it to that)
    if het:
        fdn = _central(lambda s2: LL.vardtc(specs, X, Z, Y, np.concatenate([s2, noise[6:]]))["lml"], noise[:6], -1e-5)
        _held("vardtc", _dnoise_dvar(r)[:6], fdn, {"noise": np.r_[0:6]})
    else:
        fdn = _central(lambda s2: LL.vardtc(specs, X, Z, Y, float(s2[0]))["lml"], np.array([noise]), -1e-5)
        _held("vardtc", np.atleast_1d(_dnoise_dvar(r)), fdn, {"noise": np.r_[0:1]})


def _dnoise_dvar(r):
    """d lml / d (noise variance) from dL_dR (var_dtc.py:240-261 differentiates in the variance; its callers hand the result to
    exact_inference_gradients): one number, or per point the sum over the output columns"""
    d = KL._a(r["dnoise"], LD)
    return np.sum(d, axis=1) if d.ndim == 2 else d


@need_ld
@pytest.mark.parametrize("alpha", [1.0, 0.5])
def test_pep_gradients_agree_with_central_differences(alpha):
    specs, X, Z, Y, noise = _problem()
    r = LL.pep(specs, X, Z, Y, noise, alpha)
    th = np.concatenate([s[2] for s in specs])
    fd = _central(lambda t: LL.pep(_with_theta(specs, t), X, Z, Y, noise, alpha)["lml"], th, -1e-5)
    _held("pep a=%g" % alpha, r["dtheta"], fd, THETA_CLASSES)
    fdZ = _central(lambda z: LL.pep(specs, X, z, Y, noise, alpha)["lml"], Z, 1e-6)
    _held("pep a=%g" % alpha, r["dZ"].ravel(), fdZ, {"Z": np.r_[0:Z.size]})
    fdn = _central(lambda s2: LL.pep(specs, X, Z, Y, float(s2[0]), alpha)["lml"], np.array([noise]), -1e-5)
    _held("pep a=%g" % alpha, np.atleast_1d(r["dnoise"]), fdn, {"noise": np.r_[0:1]})


@need_ld
def test_svgp_backward_agrees_with_central_differences_of_the_linearised_bound():
    specs, X, Z, Y, noise = _problem()
    c = dict(N=X.shape[0], M=Z.shape[0], D=X.shape[1], R=Y)
    f = LL.family_inputs(c, L=2)
    dF = f["dF"]
    r = LL.svgp(specs, X, Z, f["q_mean"], f["q_L"], dF)

    def S(sp, z):
        with LL.linear_admitted():
            st = SN.forward(sp, X, z, f["q_mean"], f["q_L"], dt=LD)
        return np.sum(KL._a(dF[0], LD) * st["mu"]) + np.sum(KL._a(dF[1], LD) * st["v"]) - st["KL"]
    th = np.concatenate([s[2] for s in specs])
    fd = _central(lambda t: S(_with_theta(specs, t), Z), th, -1e-5)
    _held("svgp", r["dtheta"], fd, THETA_CLASSES)
    fdZ = _central(lambda z: S(specs, z), Z, 1e-6)
    _held("svgp", r["dZ"].ravel(), fdZ, {"Z": np.r_[0:Z.size]})


@need_ld
def test_sparse_ld_alone_is_wrong_for_the_linear_variances():
    """what the helper exists for: with "linear" admitted and its diag term left where sparse_ld puts it, the variances of the
    Linear parts get a gradient that central differences contradict, and nothing else does"""
    specs, X, Z, Y, noise = _problem()
    sup = SL.SUPPORTED
    SL.SUPPORTED = tuple(sup) + ("linear",)
    try:
        plain = SL.vardtc(specs, X, Z, Y, noise)
    finally:
        SL.SUPPORTED = sup
    right = LL.vardtc(specs, X, Z, Y, noise)
    lin = THETA_CLASSES["linear_variances"]
    others = np.setdiff1d(np.arange(right["dtheta"].size), lin)
    assert np.array_equal(plain["dtheta"][others], right["dtheta"][others]) and plain["lml"] == right["lml"]
    assert np.max(np.abs(plain["dtheta"][lin] - right["dtheta"][lin])) > 0.1 * np.max(np.abs(right["dtheta"][lin]))


@need_ld
@pytest.mark.parametrize("name", LL.FIXTURES)
def test_restatement_matches_the_reference_fixtures(name):
    fx = LL.load_fixture(name)
    assert float(fx["cond_Kmm"]) <= 1e3 and fx["X"].shape[0] <= 60 and fx["Z"].shape[0] <= 12
    r = LL.restate_fixture(fx)
    if fx["family"] == "epdtc":
        assert r.pop("sweeps") == fx["sweeps"] and not fx["clamped"]
    figs = LL.fixture_figures(r, fx)
    print(name, {q: "%.1e" % e for q, (e, _) in figs.items()})
    assert {"dtheta", "dZ", "woodbury_vector", "pred_mu", "pred_var"} <= set(figs)
    for q, (e, _) in figs.items():
        assert e <= 1e-9, (q, e)


def test_the_fixture_set_covers_what_it_should():
    fams = [LL.load_fixture(n) for n in LL.FIXTURES]
    assert 8 <= len(fams) <= 10
    assert {f["family"] for f in fams} == {"vardtc", "pep", "svgp", "epdtc"}
    assert all("orders" in f and len(f["orders"]) == f["sweeps"] for f in fams if f["family"] == "epdtc")
    kinds = [[s[0] for s in f["specs"]] for f in fams]
    assert all("linear" in k for k in kinds)
    assert any(np.ndim(f.get("noise", 0.0)) == 1 for f in fams) and any(f["Y"].shape[1] == 2 for f in fams)
    assert any(any(s[0] == "linear" and s[4] != 0 for s in f["specs"]) for f in fams)                 # a Prod factor
    assert any(any(s[0] == "linear" and len(s[3]) < f["X"].shape[1] for s in f["specs"]) for f in fams)   # a strict column subset


@need_ld
def test_a_lone_linear_part_against_the_dense_evaluation():
    rng = np.random.default_rng(5)
    N, D, s2 = 40, 4, 0.07
    X = rng.uniform(-0.5, 0.5, (N, D))
    Y = X @ np.array([[1.0], [-0.5], [0.3], [0.8]]) + 0.2 * rng.standard_normal((N, 1))
    specs = [LL.linear_part(np.arange(D), 1)]
    for M in (4, 2):
        Z = 0.5 * np.eye(D)[:M] + 0.05 * rng.standard_normal((M, D))
        r = LL.vardtc(specs, X, Z, Y, s2)
        Knm, Knn = KL.K(specs, X, Z, LD), KL.K(specs, X, None, LD)
        Lm = KL.cholesky(KL.K(specs, Z, None, LD) + LD(1e-8) * np.eye(M, dtype=LD), 257)
        V = KL.solve_lower(Lm, Knm.T.copy())
        Qnn = KL.matmul(V.T.copy(), V)

        def logN(C):
            Lc = KL.cholesky(C, 257)
            a = KL.solve_lower(Lc, KL._a(Y, LD))
            return -N * np.log(2 * KL._c(LD)["pi"]) / 2 - np.sum(np.log(np.diag(Lc))) - np.sum(a * a) / 2
        dense = logN(Qnn + LD(s2) * np.eye(N, dtype=LD)) - np.sum(np.diag(Knn - Qnn)) / (2 * LD(s2))
        err = float(abs(r["lml"] - dense) / abs(dense))
        print("lone linear M = %d: bound against the dense DTC evaluation %.1e" % (M, err))
        assert err <= 1e-13
        if M == D:                                                # Z spans the input space: the bound is the exact GP's log marginal
            exact = logN(Knn + LD(s2) * np.eye(N, dtype=LD))
            assert abs(r["lml"] - exact) <= 1e-6 * abs(exact)
        else:
            assert r["lml"] < logN(Knn + LD(s2) * np.eye(N, dtype=LD))
