"""CPU: the long-double restatement of the Laplace / EP device session, tests/laplace_ld.py, and the judge that
tests/test_gpu_laplace_shapes.py holds the device to.

(1) The restatement in fp64 reproduces the reference's own output: every fixture of tests/golden/laplace at its stored mode (the
    pieces of the log marginal, Ki_fhat, woodbury_inv, dL_dK, dtheta, the predictions) and every fixture of tests/golden/ep at
    its stored sites (alpha, the log marginal, Wi, dL_dK, dtheta, the predictions) and, following the stored update orders from
    the cold start, the site and cavity parameters and log Z_tilde -- at those files' own tolerances (laplace_np.load, ep_np.load).
(2) In long double it agrees with tests/laplace_np.py and tests/ep_np.py (LAPACK and BLAS in fp64), run live on the n_edge
    family: within the judge's bound in every judged quantity, and strictly within 32 e64 (e64 = the distance of the fp64
    restatement from long double) in all of them but the predictions, where laplace_np evaluates another formula.
(3) The inputs of the sweep are what the bound rests on: every case keeps kappa = cond2(B) <= 1e4 and every judged quantity has
    e64 finite and below 1e-10; the fp64 restatement itself passes the judge with every quantity judged.  The separated-classes
    cases reach z < -8 and z > 8 and the clamp of tau at eps64.
(4) log Phi and phi / Phi from mpmath give the moments stored from the reference (tests/golden/ep/bernoulli_ep_moments.npz).
(5) The judge rejects one entry of a vector, of K_Wi_i or of dL_dK at the last row off by 1e-9 of the largest, one gradient
    entry off by 1e-9 of its cond, and a sweep that skipped its last site.

The whole file: 75 tests, 71 ... 90 s of wall time on a CPU-only machine, 55 s of it the long-double and fp64 references of
the 41 cases (N = 1025: 20 s, N = 512 and 513: 9 s each)."""
import os

import numpy as np
import pytest

import gpy_amd
import ep_np as EP
import kern_ld as KL
import laplace_ld as LL
import laplace_lik_np as LLN
import laplace_np as LP
import sparse_ld as SL

pytestmark = pytest.mark.skipif(not KL.HAVE_LD, reason="np.longdouble is not an extended format on this host")
F64 = np.float64
ALL = [c["name"] for c in LL.CASES]


# ---- (1) the reference's own output ------------------------------------------------------------------------------------------
def _rest(specs, X, Xs, K, W, a, s, fac):
    """finish, gradients and both predictions in fp64 at given W, woodbury vector a and dL_dfhat s"""
    d, logdet, KWi = LL.finish(K, W, F64, fac)
    _, G, dth, _ = LL.gradients(specs, X, K, KWi, a, s, F64)
    mu, var = LL.predict(specs, X, Xs, a, W, fac[1], False, F64)
    _, cov = LL.predict(specs, X, Xs, a, W, fac[1], True, F64)
    return d, logdet, KWi, G, dth, mu, var, cov


@pytest.mark.parametrize("name", LP.CASES)
def test_fp64_restatement_against_the_laplace_fixtures(name):
    g = LP.load(name)
    specs, X, Y, Xs = g["specs"], g["X"], g["Y"], g["Xs"]
    lik, y, f = gpy_amd.Bernoulli(), Y[:, 0], g["f_hat"][:, 0]
    K = KL.K(specs, X, None, F64)
    W = -lik.d2logpdf_df2(f, y)
    fac = LL.factor(K, W, F64)
    a, Ka, logdet = LL.newton(K, W, W * f + lik.dlogpdf_df(f, y), F64, fac)       # at the mode a = Ki_fhat and K a = f_hat
    d = LL.finish(K, W, F64, fac, want_matrix=False)[0]
    s = -0.5 * d * (-lik.d3logpdf_df3(f, y))                                      # dL_dfhat (laplace.py:251-255)
    d, logdet2, KWi, G, dth, mu, var, cov = _rest(specs, X, Xs, K, W, a, s, fac)
    lml = -0.5 * np.dot(a, Ka) + np.sum(lik.logpdf(Ka, y)) - 0.5 * logdet2
    got = dict(lml=lml, f_hat=Ka[:, None], Ki_fhat=a[:, None], dtheta=dth, dL_dK=G, woodbury_inv=KWi, pred_mu=mu, pred_var=var,
               pred_cov=cov, pred_p=lik.predictive_mean(mu, var))
    ref = dict(g, dL_dK=0.5 * (g["dL_dK"] + g["dL_dK"].T))
    fig = {q: (abs(got[q] - ref[q]) / abs(ref[q]) if q == "lml" else LP.rel(got[q], ref[q])) for q in LP.STANDING}
    print(name, {q: "%.1e (tol %.1e)" % (fig[q], g["tol"][q]) for q in fig})
    assert logdet == logdet2
    for q in LP.STANDING:
        assert fig[q] <= g["tol"][q], (q, fig[q], g["tol"][q])


def _follow_the_orders(g, K):
    """`expectation_propagation` (:279-310) through recompute and sweep in fp64, from the cold start along the stored orders"""
    n = K.shape[0]
    sign, eta, delta = EP.ysign(g["Y"]), g["eta"], g["delta"]
    tau, v = np.zeros(n), np.zeros(n)
    par = g["parallel_updates"]
    mu, sd, _, Sigma = LL.recompute(K, tau, v, 1e-7, not par, F64)
    for it in range(g["sweeps"]):
        if par:                                                  # every site sees the same q(f): the formulas of `sweep` on vectors
            ct, cv = 1.0 / sd - eta * tau, mu / sd - eta * v
            lz, mu_hat, s2_hat, _ = LL.moments(sign, ct, cv, F64)
            tau, v = (np.maximum(tau + delta / eta * (1.0 / s2_hat - 1.0 / sd), KL.EPS64),
                      v + delta / eta * (mu_hat / s2_hat - mu / sd))
            r = dict(tau=tau, v=v, cav_tau=ct, cav_v=cv, log_Z_hat=lz)
        else:
            r = LL.sweep(Sigma, mu, g["orders"][it], sign, eta, delta, tau, v, F64)
            tau, v = r["tau"], r["v"]
        mu, sd, _, Sigma = LL.recompute(K, tau, v, 0.0, not par, F64)
    return dict(tau_tilde=tau, v_tilde=v, cav_tau=r["cav_tau"], cav_v=r["cav_v"],
                log_Z_tilde=EP.log_Z_tilde(r["log_Z_hat"], tau, v, r["cav_tau"], r["cav_v"]))


@pytest.mark.parametrize("name", EP.CASES)
def test_fp64_restatement_against_the_ep_fixtures(name):
    g = EP.load(name)
    specs, X, Xs = g["specs"], g["X"], g["Xs"]
    K = KL.K(specs, X, None, F64)
    tau, v = g["tau_tilde"], g["v_tilde"]
    fac = LL.factor(K, tau, F64)
    alpha, mu_f, logdet = LL.newton(K, tau, v, F64, fac)
    _, _, Wi, G, dth, mu, var, cov = _rest(specs, X, Xs, K, tau, alpha, np.zeros_like(alpha), fac)
    lml = 0.5 * (-tau.size * np.log(2 * np.pi) - logdet + np.dot(v, mu_f)) + g["log_Z_tilde"]
    got = dict(lml=lml, alpha=alpha[:, None], Wi=Wi, dL_dK=G, dtheta=dth, pred_mu=mu, pred_var=var, pred_cov=cov,
               pred_p=gpy_amd.Bernoulli().predictive_mean(mu, var))
    got.update(_follow_the_orders(g, K))
    fig = EP.figures(g, got)
    assert set(fig) == set(EP.STANDING)
    for q in fig:
        assert fig[q] <= g["tol"][q], (q, fig[q], g["tol"][q])


# ---- (2) long double against LAPACK in fp64, live ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", LL.NAMES["n_edge"])
def test_long_double_against_the_numpy_restatements_live(name):
    c, ref, r64, kappa = LL.reference(name)
    specs, X, W, full = c["specs"], c["X"], c["W"], c["full"]
    K, dKs = LP.expr(specs, X)
    got = {}
    got["a"], got["Ka"], got["logdet_newton"] = LP.newton(K, W, c["b"])
    got["diag"], got["logdet_finish"], KWi = LP.finish(K, W)
    got["s"] = LLN.implicit_vector(K, KWi, c["dL_dfhat"])
    if full:
        got["K"], got["K_Wi_i"] = K, KWi
        got["dL_dK"] = LP.dL_dK_sym(K, c["Ki_f"], c["dL_dfhat"], KWi)
        got["dtheta"] = np.array([np.sum(got["dL_dK"] * dK) for dK in dKs])
    for M in c["Ms"]:
        r = {"Ki_fhat": c["Ki_f"][:, None], "woodbury_inv": KWi}
        got["mu%d" % M], got["var%d" % M] = LP.predict(specs, X, r, c["Xs%d" % M])
        got["cov%d" % M] = LP.predict(specs, X, r, c["Xs%d" % M], full_cov=True)[1]
    got["ep_mu_diag_only"], got["ep_sd_diag_only"], got["ep_logdet"], _ = EP.recompute(K, c["tau"], c["v"], c["add_diag"], False)
    if full:
        got["ep_mu"], got["ep_sd"], _, Sigma = EP.recompute(K, c["tau"], c["v"], c["add_diag"], True)
        r = EP.sweep(Sigma, got["ep_mu"], c["order"], c["ysign"], c["eta"], c["delta"], c["tau"], c["v"])
        got.update(("sw_" + q, r[q]) for q in LL.SWEEP_KEYS)
        got["again_mu"], got["again_sd"] = EP.recompute(K, r["tau"], r["v"], 0.0, True)[:2]
    figs, bad = LL.judge(c, got, ref, r64, kappa)
    assert not bad, bad
    assert set(figs) == set(LL.judged(c)) | ({"dtheta"} if full else set())
    # strictly within 32 e64 where both sides evaluate the same formulas; laplace_np.predict goes through the explicit K_Wi_i
    # (K** - Kx^T K_Wi_i Kx), and the variance at one point is one number, whose e64 is 1e-17 when the fp64 rounding happens to
    # cancel (found: 3.3e-16 against 32 x 1.0e-17 at N = 63): the predictions are held to the judge's bound above only
    e64 = dict((q, SL.rel_err(r64[q], ref[q])) for q in LL.judged(c) + (("dtheta",) if full else ()) if q not in LL.pred_q(c))
    err = dict((q, SL.rel_err(got[q], ref[q])) for q in e64)
    print(name, "  ".join("%s %.1e/%.1e" % (q, err[q], e64[q]) for q in e64))
    over = ["%s: %.3e > 32 x %.3e" % (q, err[q], e64[q]) for q in e64 if not err[q] <= 32.0 * e64[q]]
    assert not over, over


# ---- (3) the inputs ----------------------------------------------------------------------------------------------------------
def test_the_case_list_names_every_edge():
    have = set((c["family"], c["kern"], c["N"], c["variant"]) for c in LL.CASES)
    for N in (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 512, 513, 1025):
        assert ("n_edge", "rbf_ard+bias", N, "") in have
    assert [c["N"] for c in LL.CASES if not c["full"]] == [1025]
    for N in (129, 257):
        for v in ("zeros", "clip", "tauzero", "cold", "separated"):
            assert ("weights", "rbf_iso", N, v) in have
    assert len(LL.NAMES["kernels"]) == 10 and len(LL.NAMES["points"]) == 2 and len(LL.NAMES["stale"]) == 5
    assert all(LL.BY_NAME[n]["Ms"] == (1, 127, 128, 129, 257) for n in LL.NAMES["points"])
    assert all(n in LL.BY_NAME for n in LL.SCHEDULES)
    s = [LL.make_case(n) for n in LL.NAMES["stale"]]
    assert [c["N"] for c in s] == [257, 129, 129, 129, 129] and [c["action"] for c in s][2:] == ["set_targets", None, "exact_inference_sum"]
    assert all(np.array_equal(c["X"], s[1]["X"]) for c in s[2:]) and np.array_equal(s[3]["Y"], s[2]["Y"])
    assert not np.array_equal(s[2]["Y"], s[1]["Y"]) and len(s[2]["specs"]) == 2 and s[2]["specs"][0][4] == s[2]["specs"][1][4] == 1
    zeros, clip, tz, cold = (LL.make_case("weights-rbf_iso-n257-" + v) for v in ("zeros", "clip", "tauzero", "cold"))
    assert np.sum(zeros["W"] == 0) == 25 and np.sum(tz["tau"] == 0) == 25 and not cold["tau"].any() and cold["add_diag"] == 1e-7
    assert 100 <= np.sum(clip["W"] == 1e-6) <= 157 and 40 < clip["W"].max() <= 50
    for k in ("rbf_x_coreg_r1", "rbf_x_coreg_r2"):
        c = LL.make_case("kernels-%s-n65" % k)
        idx = c["Xs129"][:, 2]
        assert set(idx) == {0.0, 1.0, 2.0} and set(c["X"][:, 2]) == {0.0, 1.0, 2.0}
    assert LL.make_case("kernels-rbf_ard_d33-n129")["X"].shape == (129, 33)
    for c in (LL.make_case(n) for n in ALL if LL.BY_NAME[n]["N"] >= 2):
        assert np.array_equal(c["X"][0], c["X"][1])


@pytest.mark.parametrize("name", ALL)
def test_inputs_are_well_conditioned_and_fp64_is_within_1e_10(name):
    c, ref, r64, kappa = LL.reference(name)
    assert kappa and all(k <= 1e4 for k in kappa.values()), kappa
    for q in LL.judged(c):
        e64 = SL.rel_err(r64[q], ref[q])
        assert np.isfinite(e64) and e64 < 1e-10, (q, e64)
    if c["laplace"] and c["full"]:
        e64 = np.abs(KL._a(r64["dtheta"], KL.LD) - ref["dtheta"])
        assert np.all(np.isfinite(e64)) and np.all(e64 < 1e-10 * np.max(np.abs(ref["dtheta"])))
    figs, bad = LL.judge(c, r64, ref, r64, kappa)               # the fp64 restatement itself passes, with all quantities judged
    assert not bad and set(figs) == set(LL.judged(c)) | ({"dtheta"} if c["laplace"] and c["full"] else set())
    if c["variant"] == "separated":
        assert ref["sw_z"].min() < -8 and ref["sw_z"].max() > 8 and len(ref["sw_clamped"]) >= 1
        assert np.all(KL.f64(ref["sw_tau"])[ref["sw_clamped"]] == KL.EPS64)
    if c["variant"] == "cold":
        assert "again_mu" not in LL.judged(c)


# ---- (4) the probit moments ---------------------------------------------------------------------------------------------------
def test_mpmath_moments_against_values_stored_from_the_reference():
    z = np.load(os.path.join(EP.GOLDEN, "bernoulli_ep_moments.npz"))
    tau, v = z["tau"], z["v"]
    for yv in (0, 1):
        sign = 1.0 if yv else -1.0
        ld = dict(zip(("log_Z_hat", "mu_hat", "sigma2_hat"), LL.moments(sign, tau, v, KL.LD)[:3]))
        d64 = dict(zip(("log_Z_hat", "mu_hat", "sigma2_hat"), LL.moments(sign, tau, v, F64)[:3]))
        for q in ld:
            want, bound = z["%s_y%d" % (q, yv)], 10.0 * float(z["ref_vs_scipy_" + q])
            for tag, a in (("mpmath", KL.f64(ld[q])), ("scipy", d64[q])):
                err = np.max(np.abs(a - want) / np.where(want != 0, np.abs(want), 1.0))
                print("%s %s y=%d: %.2e (bound %.2e)" % (tag, q, yv, err, bound))
                assert np.isfinite(a).all() and err <= bound, (tag, q, yv, err, bound)
    lz, r = LL.probit(KL.LD(-40), KL.LD)                        # far tails: no underflow, no cancellation
    series = 1.0 - 1.0 / 40.0 ** 2 + 3.0 / 40.0 ** 4 - 15.0 / 40.0 ** 6 + 105.0 / 40.0 ** 8     # Phi(-z) = phi(z) / z x series
    assert abs(float(r) - 40.0 / series) < 1e-9
    assert abs(float(lz) - (-800.0 - np.log(40.0 * np.sqrt(2.0 * np.pi)) + np.log(series))) < 1e-9
    lz, r = LL.probit(KL.LD(40), KL.LD)
    assert lz < 0 and lz > -1e-300 and 0 < r < 1e-300


# ---- (5) the judge bites ------------------------------------------------------------------------------------------------------
def test_judge_rejects_small_faults():
    name = "n_edge-rbf_ard+bias-n129"
    c, ref, r64, kappa = LL.reference(name)
    N = c["N"]

    def damaged(q, idx, rel):
        got = dict(r64)
        got[q] = np.array(r64[q])
        got[q][idx] += rel * np.max(np.abs(r64[q]))
        return LL.judge(c, got, ref, r64, kappa)[1]
    for q, idx in (("a", N - 1), ("Ka", 64), ("s", 128), ("K_Wi_i", (N - 1, 0)), ("dL_dK", (N - 1, 63)), ("cov129", (128, 0)),
                   ("sw_mu", 128), ("ep_sd", 0)):
        bad = damaged(q, idx, 1e-9)
        assert len(bad) == 1 and bad[0].startswith(q + ":"), (q, bad)
    got = dict(r64)
    got["dtheta"] = np.array(r64["dtheta"])
    got["dtheta"][1] += 1e-9 * float(ref["dtheta_cond"][1])
    bad = LL.judge(c, got, ref, r64, kappa)[1]
    assert len(bad) == 1 and bad[0].startswith("dtheta:"), bad
    # a sweep that skipped the last site of its order
    Sigma = LL.recompute(KL.K(c["specs"], c["X"], None, F64), c["tau"], c["v"], 0.0, True, F64)[3]
    r = LL.sweep(Sigma, r64["ep_mu"], c["order"][:-1], c["ysign"], c["eta"], c["delta"], c["tau"], c["v"], F64)
    got = dict(r64)
    got.update(("sw_" + q, r[q]) for q in LL.SWEEP_KEYS)
    bad = LL.judge(c, got, ref, r64, kappa)[1]
    assert any(b.startswith("sw_tau:") for b in bad) and any(b.startswith("sw_mu:") for b in bad), bad
    del got["sw_mu"]
    assert any(b.startswith("sw_mu: missing") for b in LL.judge(c, got, ref, r64, kappa)[1])
