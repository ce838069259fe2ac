"""CPU: the long-double restatement of VarDTC with Coregionalize factors (tests/sparse_coreg_ld.py) proves itself before the GPU
test judges the device by it:

 (a) central differences of its own bound in long double for every parameter class -- the stationary factors' theta, W and kappa
     of every Coregionalize factor (through B and through the diagonal term), Bias, White, the noise per point, and Z in its
     spatial columns -- with scalar and per-point noise.  Step h = 1e-5 |parameter| (1e-6, absolute, for Z): the truncation
     error of a central difference is h^2 times a third derivative over 6, 1e-10 relative or so, the rounding error
     eps_ld / h ~ 1e-13; held to 1e-8 of the largest gradient entry of the class.  The index column of Z has no derivative (the
     kernel is a lookup there); the restatement's dZ is exactly zero in it.
 (b) the fixtures of the reference's own VarDTC evaluations (tests/golden/sparse_coreg/*.npz, made by
     tools/make_golden_sparse_coreg.py), restated at fp64: 1e-9 of each quantity's largest entry (both sides are fp64
     evaluations of problems with kappa <= 16).
 (c) the device's S convention: S[a][b] = the sum of the weights over rows of output a and columns of output b, taken to W and
     kappa by `kern_ld.chain_coreg` (dkappa = diag S, dW = (S + S^T) W), is the derivative the restatement takes through B.

It also shows what the helper is for: sparse_ld.vardtc with "coregionalize" admitted and nothing else changed gives W and kappa a
gradient that central differences contradict.  And every case of the GPU sweep stays inside the conditioning cap of the judge
(cond2(Kmm + 1e-8 I) <= 1e4), checked here with the restatement alone."""
import numpy as np
import pytest

import kern_ld as KL
import sparse_coreg_ld as CL
import sparse_ld as SL

LD = KL.LD
need_ld = pytest.mark.skipif(not KL.HAVE_LD, reason="np.longdouble is not an extended format on this host")
CD_TOL = 1e-8


def _problem(het=False, Dy=1):
    """LCM of two (ranks 1 and 2) + Coregionalize * Bias + White, P = 3, unsorted rows"""
    rng = np.random.default_rng(23)
    N, M, D, P = 45, 9, 3, 3
    X, Z = rng.uniform(-0.5, 0.5, (N, D)), rng.uniform(-0.5, 0.5, (M, D))
    X[:, 2] = rng.permutation(np.arange(N) % P)
    Z[:, 2] = np.arange(M) % P
    sp, allq = np.arange(2, dtype=np.int32), np.arange(D, dtype=np.int32)
    specs = [("rbf", 1, np.array([1.3, 0.4, 0.5]), sp, 1), CL.coreg_part(P, 2, rank=1, term=1),
             ("matern32", 0, np.array([0.8, 0.6]), sp, 2), CL.coreg_part(P, 2, rank=2, term=2, seed=1),
             CL.coreg_part(P, 2, rank=1, term=3, seed=2), ("bias", 0, np.array([0.3]), allq, 3), ("white", 0, np.array([0.05]), allq, 0)]
    Y = np.sin(3 * X[:, :1] + X[:, 2:3]) + X[:, 1:2] + 0.1 * rng.standard_normal((N, Dy))
    noise = (0.03 + 0.1 * rng.uniform(0, 1, N)) if het else 0.07
    return specs, X, Z, Y, noise


def _with_theta(specs, flat):
    out, k = [], 0
    for s in specs:
        n = KL.n_params(s)
        out.append((s[0], s[1], np.array(flat[k:k + n], dtype=np.float64), s[3], s[4]))
        k += n
    return out


def _central(f, x, h, only=None):
    x = np.asarray(x, np.float64)
    g = np.zeros(x.size, dtype=LD)
    for i in (range(x.size) if only is None else only):
        e = np.zeros(x.size)
        e[i] = -h * max(abs(x.flat[i]), 1e-300) if h < 0 else h
        hi, lo = (x.ravel() + e).reshape(x.shape), (x.ravel() - e).reshape(x.shape)
        g[i] = (LD(f(hi)) - LD(f(lo))) / (LD(hi.ravel()[i]) - LD(lo.ravel()[i]))
    return g


def _held(name, got, fd, classes):
    for cls, idx in classes.items():
        err = float(np.max(np.abs(KL._a(got, LD)[idx] - fd[idx])) / np.max(np.abs(fd[idx])))
        print("CD %s %s %.2e" % (name, cls, err))
        assert err <= CD_TOL, (name, cls, err)


# link order: rbf (3) | W 3 kappa 3 | matern32 (2) | W 6 kappa 3 | W 3 kappa 3 | bias | white
THETA_CLASSES = {"stationary": np.r_[0:3, 9:11], "W": np.r_[3:6, 11:17, 20:23], "kappa": np.r_[6:9, 17:20, 23:26], "bias": np.r_[26:27],
                 "white": np.r_[27:28]}


@need_ld
@pytest.mark.parametrize("het,Dy", [(False, 1), (True, 1), (False, 2)])
def test_vardtc_gradients_agree_with_central_differences(het, Dy):
    specs, X, Z, Y, noise = _problem(het, Dy)
    r = CL.vardtc(specs, X, Z, Y, noise)
    th = np.concatenate([s[2] for s in specs])
    assert th.size == 28
    fd = _central(lambda t: CL.objective(_with_theta(specs, t), X, Z, Y, noise), th, -1e-5)
    _held("vardtc", r["dtheta"], fd, THETA_CLASSES)
    spatial = [i for i in range(Z.size) if i % 3 != 2]
    fdZ = _central(lambda z: CL.objective(specs, X, z, Y, noise), Z, 1e-6, only=spatial)
    _held("vardtc", r["dZ"].ravel(), fdZ, {"Z": np.array(spatial)})
    assert np.all(KL.f64(r["dZ"])[:, 2] == 0.0) and r["dZ_zero_cols"] == [2]
    if het:
        fdn = _central(lambda s2: CL.objective(specs, X, Z, Y, np.concatenate([s2, noise[6:]])), noise[:6], -1e-5)
        _held("vardtc", KL._a(r["dnoise"], LD)[:6], fdn, {"noise": np.r_[0:6]})
    else:
        fdn = _central(lambda s2: CL.objective(specs, X, Z, Y, float(s2[0])), np.array([noise]), -1e-5)
        _held("vardtc", np.atleast_1d(r["dnoise"]), fdn, {"noise": np.r_[0:1]})


@need_ld
def test_without_the_helper_the_diagonal_term_of_W_and_kappa_is_wrong():
    specs, X, Z, Y, noise = _problem()
    th = np.concatenate([s[2] for s in specs])
    keep = SL.SUPPORTED
    SL.SUPPORTED = tuple(keep) + ("coregionalize",)
    try:
        plain = SL.vardtc(specs, X, Z, Y, noise)["dtheta"]
    finally:
        SL.SUPPORTED = keep
    fd = _central(lambda t: CL.objective(_with_theta(specs, t), X, Z, Y, noise), th, -1e-5, only=list(THETA_CLASSES["kappa"]))
    idx = THETA_CLASSES["kappa"]
    assert float(np.max(np.abs(KL._a(plain, LD)[idx] - fd[idx])) / np.max(np.abs(fd[idx]))) > 1e-2


@need_ld
def test_the_device_convention_S_chains_to_the_restatements_W_and_kappa():
    """S[a][b] = sum of dL_dK over rows of output a and columns of output b, of both update_gradients_full calls, plus the
    per-output dL_dKdiag sums on its diagonal; `chain_coreg` of it is the restatement's gradient in W and kappa"""
    specs, X, Z, Y, noise = _problem(het=True)
    r = CL.vardtc(specs, X, Z, Y, noise)
    lvn, lvm = KL.leaves(specs, X, Z, LD), KL.leaves(specs, Z, None, LD)
    Wn, Wm = KL._weights(specs, lvn, KL._a(r["dL_dKnm"], LD)), KL._weights(specs, lvm, KL._a(r["dL_dKmm"], LD))
    others = SL._diag_weights(specs, X, LD)
    xi, zi = X[:, 2].astype(int), Z[:, 2].astype(int)
    first = np.cumsum([0] + [KL.n_params(s) for s in specs])
    for i, s in enumerate(specs):
        if s[0] != "coregionalize":
            continue
        P = s[1] % 100
        S = np.zeros((P, P), dtype=LD)
        for a in range(P):
            for b in range(P):
                S[a, b] = np.sum(Wn[i][xi == a][:, zi == b]) + np.sum(Wm[i][zi == a][:, zi == b])
            S[a, a] += np.sum((KL._a(r["dL_dKdiag"], LD) * others[i])[xi == a])
        got = KL.chain_coreg([s], KL.f64(S).ravel())
        want = KL.f64(r["dtheta"][first[i]:first[i + 1]])
        assert np.max(np.abs(got - want)) <= 1e-13 * np.max(np.abs(want)), (i, got, want)


def test_the_fixtures_are_there_and_small():
    import os
    assert len(CL.FIXTURES) == 8
    for name in CL.FIXTURES:
        fx = CL.load_fixture(name)
        assert os.path.getsize(os.path.join(CL.GOLDEN, name + ".npz")) < 64 * 1024
        assert fx["X"].shape[0] <= 60 and fx["Z"].shape[0] <= 12 and float(fx["cond_Kmm"]) <= 1e3
        assert any(s[0] == "coregionalize" for s in fx["specs"])
    un = CL.load_fixture("icm_rbf_unsorted_p3_n57_m12_d3")
    assert np.any(np.diff(un["X"][:, int(un["idx_col"])]) < 0)


@pytest.mark.parametrize("name", CL.FIXTURES)
def test_restatement_reproduces_the_reference_fixtures(name):
    fx = CL.load_fixture(name)
    figs = CL.fixture_figures(CL.restate_fixture(fx, np.float64), fx)
    for q, (e, _) in sorted(figs.items()):
        print("FIX %s %s %.2e" % (name, q, e))
    assert set(figs) >= {"lml", "dtheta", "dZ", "dL_dKmm", "dL_dKnm", "dL_dthetaL", "woodbury_vector", "woodbury_inv", "pred_mu",
                         "pred_var", "pred_cov"}
    bad = dict((q, e) for q, (e, _) in figs.items() if not e <= 1e-9)
    assert not bad, bad


@need_ld
@pytest.mark.parametrize("name", CL.PLAIN + sorted(set(CL.STALE)))
def test_every_case_of_the_sweep_stays_inside_the_conditioning_cap(name):
    c, ref, r64, kappa = CL.reference(name)              # (asserts kappa <= 1e4)
    print("kappa %s %.1f" % (name, kappa))
    assert np.all(KL.f64(ref["dZ"])[:, c["idx_col"]] == 0.0)
    e64 = max(SL.rel_err(r64[q], ref[q]) for q in SL.JUDGED if q in ref)
    assert e64 < 1e-9, e64                               # the fp64 restatement is a usable yardstick on these inputs
