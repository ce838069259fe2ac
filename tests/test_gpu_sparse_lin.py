"""GPU (-m gpu): the Linear kernel (C-ABI kind 9) on the sparse device path -- VarDTC, prediction, PEP / FITC, SVGP, EPDTC and
`mi355gp_sparse_kdiag` alone -- judged in long double at the shapes where each mechanism engages (tests/sparse_lin_ld.py).

The rule is sparse_ld.judge's: err(q) = max |device - q_ld| / max |q_ld| <= max(32 e64(q), 256 eps64 kappa), e64(q) the
distance of THE RESTATEMENT RUN AT fp64 from its long-double value on the same input (never the device's own figure), kappa =
cond2(Kmm + 1e-8 I) <= 1e3 (asserted per case; measured at most 252 over the sweep).

    m_edge    N = 257, D = 2, rbf_ard + linear_ard, M = 1 | 63 | 64 | 65 | 128 | 129 | 257: the 64-column tiles of k_grad_cols_lin
    n_edge    M = 65, D = 3, Dy = 2, N = 1 | 2 | 63 | 64 | 65 | 129 | 257 | 2049: a row tile, a row split, the chunk granule, N < M
    dispatch  N = 193, M = 65, (D, Dy) = (16, 4) | (16, 5) | (17, 1) | (33, 1) | (1, 1), matern32_ard + linear_ard | linear_iso:
              D = 16 is the last shape of k_grad_cols_lin (rank term in registers at Dy = 4, per element at 5), D = 17 the first
              with the weights formed in memory (launch_grad launches nothing for kind 9 with a rank term), D = 33 two ARD groups
    forms     a lone Linear with M <= D; linear[0..D-2] * rbf[D-1] + white; rbf + linear * bias; Linear on columns (0, 2) of
              three (dZ column 1 exactly 0, two variance gradients); an all-zero input row
    noise     per-point noise, Dy = 1 | 3, at 257 / 65 and 129 / 128
    families  PEP at alpha = 1 (FITC) and 0.5, SVGP with L = 1 | 2 and Bernoulli weights, EPDTC recompute + sweep + inference,
              each at one m_edge shape (M = 129, D = 2) and one dispatch shape (D = 17)
    stale     one context, no set_data between: rbf + bias -> rbf + linear -> rbf + bias -> rbf + linear at other theta
    chunks    N = 262145, M = 65, D = 3 (blocked reference): a ragged second chunk; kd and the weighted sums cross the edge
    kdiag     mi355gp_sparse_kdiag alone: exact on integer inputs with power-of-two variances; the weighted sums against long
              double at N = 1 | 255 | 256 | 257 | 2049
    determinism  one case in two fresh contexts, identical bytes

Measured on one MI355X, the worst figure per family (the one with the largest figure / bound), a record and never a bound:

    family            worst quantity     figure     bound      family            worst quantity     figure     bound
    m_edge            mu129              1.3e-13    6.7e-12    stale             woodbury_vector    2.7e-13    7.8e-12
    n_edge            woodbury_inv       1.2e-13    5.4e-12    chunks            mu1                3.5e-14    1.5e-12
    dispatch          dZ (D = 1)         4.8e-14    1.3e-12    PEP / FITC        mu1 (D = 17)       6.1e-14    1.2e-12
    forms             dZ (lone Linear)   3.8e-15    1.8e-13    SVGP              cov1 (L = 2)       2.2e-14    6.8e-12
    noise             woodbury_vector    8.1e-14    3.9e-12    EPDTC sweep       sigma2_hat         3.2e-14    1.2e-10
                                                               EPDTC inference   woodbury_vector    1.1e-14    6.8e-12

The whole file takes about 30 s, the blocked N = 262145 case 4 s of them.  (README.md, "Linear on the sparse path", holds the
same table next to the timing record profiles/sparse_lin_time_*.json.)
"""
import numpy as np
import pytest

import epdtc_np as E
import kern_ld as KL
import pep_np as PN
import sparse_ld as SL
import sparse_lin_ld as LL
import svgp_np as SN
from gpy_amd import _lib as L

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not KL.HAVE_LD, reason="np.longdouble is not an extended format on this host")]
SC = L.SparseContext
LD = KL.LD
WORST = {}                               # family: (figure / bound, case, quantity), printed as the file goes


@pytest.fixture(scope="module")
def sctx():
    c = SC(0)
    c.set_linear(True)                   # (a new context refuses kind 9 until it is asked: test_a_context_that_was_not_asked...)
    c.held = None                        # the (X, R) the context holds
    yield c
    c.close()


def _hold(sctx, X, R):
    if sctx.held is None or not (np.array_equal(sctx.held[0], X) and np.array_equal(sctx.held[1], R)):
        sctx.set_data(X, R)
        sctx.held = (X, R)


def _predictions(got, fn, c):
    for tag in ("1", "129"):
        got["mu" + tag], got["var" + tag] = fn(c["Xs" + tag], False)
        got["cov" + tag] = fn(c["Xs" + tag], True)[1]
    return got


def _evaluate(sctx, c):
    """everything sparse_ld.JUDGED names, from the device"""
    N = c["N"]
    _hold(sctx, c["X"], c["R"])
    info, r = sctx.vardtc_sum(c["specs"], c["Z"], c["noise"], want_dL_dm=True)
    assert info == 0
    got = dict((q, r[q]) for q in ("lml", "dtheta", "dnoise", "dZ", "woodbury_vector", "dL_dm"))
    if not c["blocked"]:
        got["dL_dKnm"] = sctx.fetch_dL_dKnm(0, N)
    r0, nr = c["block"]
    if N >= 3:
        got["dL_dKnm_block"] = sctx.fetch_dL_dKnm(r0, nr)
    got["psi2"] = sctx.fetch(SC.FETCH_PSI2)
    got["dL_dKmm"] = sctx.fetch(SC.FETCH_DLDKMM)
    got["woodbury_inv"] = sctx.fetch(SC.FETCH_WOODBURY_INV)
    return _predictions(got, lambda Xs, full: sctx.predict(c["specs"], Xs, full_cov=full), c)


def _report(family, name, figs, bad):
    for q, (e, b) in figs.items():
        print("FIG %s %s %.2e (bound %.2e)" % (name, q, e, b))
        if e / b > WORST.get(family, (0.0,))[0] or family not in WORST:
            WORST[family] = (e / b, name, q, e, b)
    w = WORST[family]
    print("WORST %s: %s of %s, %.2e against a bound of %.2e" % (family, w[2], w[1], w[3], w[4]))
    assert not bad, "%s: %s" % (name, "; ".join(bad))


def _check(sctx, name):
    c, ref, r64, kappa = LL.reference(name)
    try:
        got = _evaluate(sctx, c)
    except L.MI355GPError as e:          # nothing more on this device after an error of the runtime
        pytest.exit("device error in %s, the sweep ends here: %s" % (name, e), returncode=3)
    figs, bad = LL.judge(got, ref, r64, kappa)
    print("\nkappa %s %.1f" % (name, kappa))
    _report("vardtc-" + c["family"], name, figs, bad)
    want = set(SL.JUDGED) - (set() if c["N"] >= 3 else {"dL_dKnm_block"}) - ({"dL_dKnm"} if c["blocked"] else set())
    assert set(figs) == want
    return c, got


@pytest.mark.parametrize("name", LL.PLAIN)
def test_sparse_linear_shape_edges(name, sctx):
    c, got = _check(sctx, name)
    if c["form"] == "subset":            # Linear on columns (0, 2): two variance gradients after the RBF part's three
        assert got["dtheta"].size == 3 + 2 and np.all(got["dZ"][:, 1] == 0.0)
    if c["form"] == "zero_row":
        kd = sctx.kdiag(c["specs"])
        assert kd[c["N"] // 2] == c["specs"][0][2][0]                 # the RBF variance alone: the Linear part's Kdiag is 0 there


@pytest.mark.parametrize("name", LL.BLOCKED)
def test_sparse_linear_several_chunks(name, sctx):
    _check(sctx, name)


def test_stale_sequence_never_reads_an_earlier_per_point_vector(sctx):
    """stationary only -> rbf + linear -> stationary only with the same part count -> other theta, one context, one set_data"""
    uploads = []
    real = sctx.set_data
    sctx.set_data = lambda X, Y: (uploads.append(1), real(X, Y))
    sctx.held = None
    try:
        for name in LL.STALE:
            _check(sctx, name)
    finally:
        del sctx.set_data
    assert len(uploads) == 1


def test_two_fresh_contexts_give_identical_bytes():
    c = LL.make_case(LL.DETERMINISM)
    out = []
    for _ in range(2):
        ctx = SC(0)
        try:
            ctx.set_linear(True)
            ctx.set_data(c["X"], c["R"])
            info, r = ctx.vardtc_sum(c["specs"], c["Z"], c["noise"], want_dL_dm=True)
            assert info == 0
            rows = ctx.fetch_dL_dKnm(0, c["N"])
            r["kdiag"] = np.concatenate(ctx.kdiag(c["specs"], w=np.cos(np.arange(c["N"]))))
            # mi355gp_sparse_kdiag works on a part list of its own, here one with another part count: the call's result and
            # what is derived from it afterwards are those of the inference call
            ctx.kdiag(_kdiag_specs(c["D"]), w=np.ones(c["N"]))
            assert ctx.fetch_dL_dKnm(0, c["N"]).tobytes() == rows.tobytes()
            r["var129"] = ctx.predict(c["specs"], c["Xs129"])[1]
            out.append(r)
        finally:
            ctx.close()
    assert out[0]["lml"] == out[1]["lml"]
    for q in ("dtheta", "dnoise", "dZ", "woodbury_vector", "dL_dm", "kdiag", "var129"):
        assert np.asarray(out[0][q]).tobytes() == np.asarray(out[1][q]).tobytes(), q


def test_a_context_that_was_not_asked_refuses_linear_by_name_and_stays_usable():
    c = LL.make_case("forms-subset-n257_m65_d3_dy2-hom")
    f = LL.family_inputs(c)
    ctx = SC(0)
    try:
        ctx.set_data(c["X"], f["Y"])                                         # (one output column: PEP and EPDTC take no more)
        for call in (lambda: ctx.vardtc_sum(c["specs"], c["Z"], c["noise"]),
                     lambda: ctx.pep(c["specs"], c["Z"], 0.05, 1.0, 1e-6),
                     lambda: ctx.svgp_forward(c["specs"], c["Z"], f["q_mean"], f["q_L"]),
                     lambda: ctx.epdtc_begin(c["specs"], c["Z"], 0.0)):
            with pytest.raises(L.MI355GPError, match=r"sparse path: covariance kind 9 \(Linear\) is not supported here"):
                call()
        info, r0 = ctx.vardtc_sum(c["specs"][:1], c["Z"], c["noise"])        # the stationary part alone is served
        assert info == 0
        ctx.set_linear(True)
        info, r1 = ctx.vardtc_sum(c["specs"], c["Z"], c["noise"])
        assert info == 0 and r1["lml"] != r0["lml"]
        ctx.set_linear(False)
        with pytest.raises(L.MI355GPError, match="Linear"):
            ctx.predict(c["specs"], c["Xs1"])
    finally:
        ctx.close()


# ---- mi355gp_sparse_kdiag alone ----------------------------------------------------------------------------------------------
def _kdiag_specs(D):
    allq = np.arange(D, dtype=np.int32)
    return [("rbf", 1, np.concatenate([[2.0], np.full(D, 0.7)]), allq, 0), ("linear", 1, 2.0 ** (np.arange(D) % 3 - 1), allq, 0),
            ("linear", 0, np.array([0.25]), allq[:-1], 1), ("bias", 0, np.array([4.0]), allq, 1), ("white", 0, np.array([0.5]), allq, 0)]


def test_kdiag_is_exact_on_integer_inputs():
    D, N = 3, 300
    X = np.random.default_rng(2).integers(-9, 10, (N, D)).astype(np.float64)
    specs = _kdiag_specs(D)
    ctx = SC(0)
    try:
        ctx.set_data(X, np.zeros((N, 1)))
        kd = ctx.kdiag(specs)
    finally:
        ctx.close()
    want = 2.0 + (X * X) @ specs[1][2] + 0.25 * (X[:, :2] ** 2).sum(1) * 4.0 + 0.5       # every operation exact in fp64
    assert np.array_equal(kd, want)
    assert np.array_equal(kd, KL.f64(KL.Kdiag(specs, X, LD)))


@pytest.mark.parametrize("N", [1, 255, 256, 257, 2049])
def test_kdiag_weighted_sums_against_long_double(N):
    """sum w kd, sum w^2 kd and update_gradients_diag(w) of every part: N above and below the 256-row block.  The sums are
    sums of N products of fp64 numbers of mixed sign: the bound is the rounding of a length-N sum in any order, N eps64 times
    the sum of the absolute terms (plus 8 eps64 for the terms' own roundings); kd itself: at most 2 D + 6 = 12 roundings of
    half an ulp each, of partial results no larger than the largest entry -- 8 eps64 of it"""
    D = 3
    rng = np.random.default_rng(N)
    X, w = rng.uniform(-1.0, 1.0, (N, D)), rng.standard_normal(N)
    specs = _kdiag_specs(D)
    ctx = SC(0)
    try:
        ctx.set_data(X, np.zeros((N, 1)))
        kd, sums, dd = ctx.kdiag(specs, w=w)
    finally:
        ctx.close()
    kd_ld, wl = KL._a(KL.Kdiag(specs, X, LD), LD), KL._a(w, LD)
    assert np.abs(kd - kd_ld).max() <= 8 * KL.EPS64 * np.abs(kd_ld).max()
    eps_n = (N + 8) * KL.EPS64
    for got, terms in ((sums[0], wl * kd_ld), (sums[1], wl * wl * kd_ld)):
        assert abs(got - np.sum(terms)) <= eps_n * np.sum(np.abs(terms))
    x2 = np.square(KL._a(X, LD))
    lin_b = 0.25 * np.sum(x2[:, :2], axis=1)                     # Kdiag of the Linear factor of the product with Bias(4)
    want = np.concatenate([[np.sum(wl)], np.zeros(D), np.sum(wl[:, None] * x2, axis=0), [np.sum(wl * 4.0 * np.sum(x2[:, :2], axis=1))],
                           [np.sum(wl * lin_b)], [np.sum(wl)]])
    mag = np.concatenate([[np.sum(np.abs(wl))], np.ones(D), np.sum(np.abs(wl)[:, None] * x2, axis=0),
                          [np.sum(np.abs(wl) * 4.0 * np.sum(x2[:, :2], axis=1))], [np.sum(np.abs(wl) * lin_b)], [np.sum(np.abs(wl))]])
    assert dd.shape == want.shape
    assert np.all(np.abs(dd - want) <= eps_n * mag), (dd, want)
    assert np.all(dd[1:1 + D] == 0.0)                            # the lengthscales of the RBF part


# ---- the other families at one m_edge and one dispatch shape -------------------------------------------------------------
@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("name", LL.FAMILY_SHAPES)
def test_pep_with_a_linear_part(name, alpha, sctx):
    c = LL.reference(name)[0]
    f = LL.family_inputs(c)
    ref = LL.pep(c["specs"], c["X"], c["Z"], f["Y"], c["noise"], alpha)
    PN.with_predictions(ref, c, lambda Xs, full: LL.predict(c["specs"], c["Z"], Xs, ref, full))
    r64 = LL.pep(c["specs"], c["X"], c["Z"], f["Y"], c["noise"], alpha, dt=np.float64)
    PN.with_predictions(r64, c, lambda Xs, full: LL.predict(c["specs"], c["Z"], Xs, r64, full, dt=np.float64))
    kappa = float(np.linalg.cond(KL.f64(ref["Kmm"])))
    assert kappa <= LL.KAPPA_CAP
    _hold(sctx, c["X"], f["Y"])
    info, r = sctx.pep(c["specs"], c["Z"], c["noise"], alpha, PN.JITTER)
    assert info == 0
    got = dict(lml=r["lml"], dtheta=r["dtheta"], dnoise=r["dnoise"], dZ=r["dZ"], woodbury_vector=r["woodbury_vector"])
    r0, nr = c["block"]
    got["dL_dKnm_block"] = sctx.fetch_dL_dKnm(r0, nr)
    got["dL_dKmm"] = sctx.fetch(SC.FETCH_DLDKMM)
    got["woodbury_inv"] = sctx.fetch(SC.FETCH_WOODBURY_INV)
    _predictions(got, lambda Xs, full: sctx.predict(c["specs"], Xs, full_cov=full), c)
    figs, bad = PN.judge(got, ref, r64, kappa)
    assert set(figs) == set(PN.JUDGED)
    _report("pep", "%s a=%g" % (name, alpha), figs, bad)
    fig_dR = LL.rel_err(r["dL_dR"], ref["dL_dR"])
    assert fig_dR <= LL.bound("dL_dR", ref, r64, kappa), fig_dR


@pytest.mark.parametrize("lat", [1, 2, "bernoulli"])
@pytest.mark.parametrize("name", LL.FAMILY_SHAPES)
def test_svgp_with_a_linear_part(name, lat, sctx):
    c = LL.reference(name)[0]
    nl = 1 if lat == "bernoulli" else lat
    f = LL.family_inputs(c, L=nl)
    Xs = {"1": c["Xs1"], "129": c["Xs129"]}
    dF = f["dF"]
    if lat == "bernoulli":               # the weights of a full batch of labels at the restatement's own marginals (svgp.py:77)
        import gpy_amd
        with LL.linear_admitted():
            st = SN.forward(c["specs"], c["X"], c["Z"], f["q_mean"], f["q_L"], dt=np.float64)
        labels = (f["Y"] > np.median(f["Y"])).astype(np.float64)
        _, dFm, dFv, _ = gpy_amd.Bernoulli().variational_expectations(labels, KL.f64(st["mu"]), KL.f64(st["v"]))
        dF = (np.ascontiguousarray(dFm), np.ascontiguousarray(dFv))
    ref = LL.svgp(c["specs"], c["X"], c["Z"], f["q_mean"], f["q_L"], dF, Xs=Xs)
    r64 = LL.svgp(c["specs"], c["X"], c["Z"], f["q_mean"], f["q_L"], dF, dt=np.float64, Xs=Xs)
    kappa = float(np.linalg.cond(KL.f64(ref["Kmm"])))
    assert kappa <= LL.KAPPA_CAP, kappa   # (SVGP's Kmm carries no jitter, svgp.py:37,40: the stationary part keeps it regular)
    _hold(sctx, c["X"], np.ascontiguousarray(np.tile(f["Y"], (1, nl))))
    info, fw = sctx.svgp_forward(c["specs"], c["Z"], f["q_mean"], f["q_L"])
    assert info == 0
    bw = sctx.svgp_backward(dF[0], dF[1])
    wv, wi = sctx.svgp_woodbury()
    got = dict(mu=fw["mu"], v=fw["v"], KL=fw["KL"], dtheta=bw["dtheta"], dZ=bw["dZ"], dL_dm=bw["dL_dm"], dL_dchol=bw["dL_dchol"],
               woodbury_vector=wv, woodbury_inv=wi)
    for tag, P in Xs.items():
        got["mu" + tag], got["var" + tag] = sctx.svgp_predict(c["specs"], P, full_cov=False)
        got["cov" + tag] = sctx.svgp_predict(c["specs"], P, full_cov=True)[1]
    figs, bad = SN.judge(got, ref, r64, kappa)
    assert set(figs) == set(SN.JUDGED)
    _report("svgp", "%s L=%s" % (name, lat), figs, bad)


@pytest.mark.parametrize("name", LL.FAMILY_SHAPES)
def test_epdtc_with_a_linear_part(name, sctx, monkeypatch):
    """one recompute, one sweep and the final VarDTC evaluation of the sites (per-point precision tau, targets v / tau, no
    jitter on Kmm: expectation_propagation.py:484-492)"""
    c = LL.reference(name)[0]
    N = c["N"]
    rng = np.random.default_rng([11, N, c["M"]])
    sign = np.where(c["R"][:, 0] > np.median(c["R"][:, 0]), 1.0, -1.0)
    tau, v = rng.uniform(0.5, 1.5, N), sign * rng.uniform(0.2, 1.0, N)
    order = rng.permutation(N)
    Kmm, Kmn = E.covariances(c["specs"], c["X"], c["Z"], LD)
    mu_ld, sd_ld = E.recompute(Kmm, Kmn, tau, v, LD)
    sweep_ld = E.ref_sweep(Kmm, Kmn, order, sign, 1.0, 1.0, tau, v, True, LD)
    _hold(sctx, c["X"], np.ascontiguousarray(sign[:, None]))
    info, _ = sctx.epdtc_begin(c["specs"], c["Z"], 0.0)
    assert info == 0
    info, mu, sd = sctx.epdtc_recompute(tau, v)
    assert info == 0
    r = sctx.epdtc_sweep(order, sign, tau, v, 1.0, 1.0, first=True)
    # the judge's rule with the restatement at fp64 as e64 and kappa of the matrix that is factored, Kmm + Kmn diag(tau) Knm
    mu_64, sd_64 = E.recompute(Kmm, Kmn, tau, v, np.float64)
    sweep_64 = E.ref_sweep(Kmm, Kmn, order, sign, 1.0, 1.0, tau, v, True, np.float64)
    kappa_llt = float(np.linalg.cond(KL.f64(Kmm) + (KL.f64(Kmn) * tau) @ KL.f64(Kmn).T))
    gote = dict(r, mu=mu, Sigma_diag=sd)
    refe, r64e = dict(sweep_ld, mu=mu_ld, Sigma_diag=sd_ld), dict(sweep_64, mu=mu_64, Sigma_diag=sd_64)
    figs = {k: (E.rel(gote[k], refe[k]), max(32.0 * E.rel(r64e[k], refe[k]), 256.0 * KL.EPS64 * kappa_llt)) for k in refe}
    _report("epdtc-sweep", name, figs, ["%s: %.3e > %.3e" % (k, e, b) for k, (e, b) in figs.items() if not e <= b])
    # the final evaluation at the swept sites: this file's VarDTC restatement with the jitter constant zero for the call
    t2, v2 = np.ascontiguousarray(r["tau"]), np.ascontiguousarray(r["v"])
    monkeypatch.setattr(SL, "JITTER", 0.0)
    tgt = (v2 / t2)[:, None]
    ref = LL.vardtc(c["specs"], c["X"], c["Z"], tgt, 1.0 / t2)
    r64 = LL.vardtc(c["specs"], c["X"], c["Z"], tgt, 1.0 / t2, dt=np.float64)
    kappa = float(np.linalg.cond(KL.f64(ref["Kmm"])))
    assert kappa <= LL.KAPPA_CAP
    info, ev = sctx.epdtc_inference(c["specs"], c["Z"], t2, v2, 0.0)
    assert info == 0
    sctx.held = None                     # (the context's targets are v / tau now)
    got = dict(lml=ev["lml"], dtheta=ev["dtheta"], dZ=ev["dZ"], woodbury_vector=ev["woodbury_vector"], dnoise=ev["dL_dR"])
    figs, bad = LL.judge(got, ref, r64, kappa)
    assert set(figs) == {"lml", "dtheta", "dZ", "woodbury_vector", "dnoise"}
    _report("epdtc", name, figs, bad)


# ---- the reference's own evaluations (tests/golden/sparse_lin/*.npz) at the tolerances of the stationary kinds' fixtures -------
@pytest.mark.parametrize("name", LL.FIXTURES)
def test_device_meets_the_reference_fixtures(name, sctx, monkeypatch):
    fx = LL.load_fixture(name)
    if fx["family"] == "epdtc":
        return _epdtc_fixture(fx, monkeypatch)
    specs, Z, Xs = fx["specs"], fx["Z"], fx["Xs"]
    _hold(sctx, fx["X"], fx["Y"])
    if fx["family"] == "svgp":
        info, fw = sctx.svgp_forward(specs, Z, fx["q_mean"], fx["q_L"])
        assert info == 0
        bw = sctx.svgp_backward(np.ascontiguousarray(fx["dF_dmu"]), np.ascontiguousarray(fx["dF_dv"]))
        M = Z.shape[0]
        flat = np.stack([bw["dL_dchol"][d][np.tril_indices(M)] for d in range(fx["q_L"].shape[0])], axis=1)
        mu, var = sctx.svgp_predict(specs, Xs, full_cov=False)
        got = dict(bound=float(np.sum(fx["F"])) - fw["KL"], mu=fw["mu"], v=fw["v"], dtheta=bw["dtheta"], dZ=bw["dZ"], dL_dm=bw["dL_dm"],
                   dL_dchol=flat, woodbury_vector=sctx.svgp_woodbury()[0], pred_mu=mu, pred_var=var,
                   pred_cov=sctx.svgp_predict(specs, Xs, full_cov=True)[1])
    else:
        if fx["family"] == "pep":
            info, r = sctx.pep(specs, Z, fx["noise"], float(fx["alpha"]), PN.JITTER)
            dthL = np.atleast_1d(r["dnoise"])
        else:
            info, r = sctx.vardtc_sum(specs, Z, fx["noise"])
            dthL = np.atleast_1d(r["dnoise"])
        assert info == 0
        mu, var = sctx.predict(specs, Xs)
        got = dict(lml=r["lml"], dtheta=r["dtheta"], dZ=r["dZ"], dL_dthetaL=dthL, woodbury_vector=r["woodbury_vector"],
                   dL_dKnm=sctx.fetch_dL_dKnm(0, fx["X"].shape[0]), dL_dKmm=sctx.fetch(SC.FETCH_DLDKMM),
                   woodbury_inv=sctx.fetch(SC.FETCH_WOODBURY_INV), pred_mu=mu, pred_var=var, pred_cov=sctx.predict(specs, Xs, full_cov=True)[1])
    figs = LL.fixture_figures(got, fx)
    print(name, {q: "%.1e" % e for q, (e, _) in figs.items()})
    assert set(figs) == set(got)
    for q, (e, tol) in figs.items():
        assert e <= tol, (q, e, tol)


def _epdtc_fixture(fx, monkeypatch):
    """the reference's EPDTC run with its recorded update orders, through `EPDTC(linear=True).inference`, at the tolerances of
    tests/test_gpu_epdtc.py: the sites and cavity parameters to epdtc_np.DEVICE_BOUND, what follows from them to
    epdtc_np.DOWNSTREAM, dL_dKmm and woodbury_inv to 1e-4"""
    import gpy_amd
    from gpy_amd.epdtc import EPDTC
    it = iter([np.asarray(o) for o in fx["orders"]])
    monkeypatch.setattr(np.random, "permutation", lambda n: next(it))
    inf = EPDTC(eta=fx["eta"], delta=fx["delta"], parallel_updates=fx["parallel_updates"], max_iters=100, linear=True)
    kern = LL.make_kernel(fx)
    post, lml, gd = inf.inference(kern, fx["X"], fx["Z"], gpy_amd.Bernoulli(), fx["Y"])
    assert inf.iterations == fx["sweeps"]
    _, ga, lzt = inf._ep_approximation
    mu, var = post._raw_predict(kern, fx["Xs"], fx["Z"])
    got = dict(lml=lml, log_Z_tilde=lzt, tau=ga.tau, v=ga.v, cav_tau=inf._cav_params.tau, cav_v=inf._cav_params.v,
               dtheta=gd["fused"]["dtheta"], dZ=gd["fused"]["dZ"], woodbury_vector=post.woodbury_vector, pred_mu=mu, pred_var=var)
    ref = dict(fx, tau=fx["tau_tilde"], v=fx["v_tilde"])
    fig = {q: (abs(got[q] - ref[q]) / abs(ref[q]) if q in ("lml", "log_Z_tilde") else E.rel(got[q], ref[q])) for q in got}
    print(fx["name"], {q: "%.1e" % e for q, e in fig.items()})
    for q, e in fig.items():
        assert e <= (E.DEVICE_BOUND[q] if q in E.DEVICE_BOUND else E.DOWNSTREAM[q]), (q, e)
    assert E.rel(np.asarray(gd["dL_dKmm"]), fx["dL_dKmm"]) <= 1e-4 and E.rel(np.asarray(post.woodbury_inv), fx["woodbury_inv"]) <= 1e-4


# ---- the host package: SparseGPRegression, SparseGP(FITC / PEP), SVGP and SparseGPClassification with RBF + Linear ---------------
def _toy(N=120, seed=0):
    rng = np.random.default_rng(seed)
    X = np.sort(rng.uniform(-1.0, 1.0, (N, 1)), 0)
    return X, np.sin(4.0 * X) + 1.5 * X + 0.1 * rng.standard_normal((N, 1)), rng


def _kern():
    import gpy_amd
    return gpy_amd.RBF(1, 1.0, 0.3) + gpy_amd.Linear(1, 0.5) + gpy_amd.Bias(1, 0.1)


def _checkgrad(m, step=1e-6, tol=1e-5):
    """central differences of the objective in the optimiser's parameters against the model's gradient"""
    x0 = m.optimizer_array.copy()
    g = m._grads(x0)
    fd = np.zeros_like(x0)
    for i in range(x0.size):
        e = np.zeros_like(x0)
        e[i] = step * max(1.0, abs(x0[i]))
        m.optimizer_array = x0 + e
        fp = m.objective_function()
        m.optimizer_array = x0 - e
        fd[i] = (fp - m.objective_function()) / (2 * e[i])
    m.optimizer_array = x0
    assert np.abs(g - fd).max() <= tol * max(1.0, np.abs(fd).max()), (g, fd)


def test_sparse_gp_regression_with_rbf_plus_linear_predicts_extrapolates_and_fits():
    import gpy_amd
    X, Y, rng = _toy()
    Z = np.linspace(-1.0, 1.0, 12)[:, None]
    k = gpy_amd.RBF(1, 1.0, 0.3) + gpy_amd.Linear(1, 2.0) + gpy_amd.Bias(1, 0.1)
    m = gpy_amd.SparseGPRegression(X, Y, kernel=k, Z=Z, noise_var=0.05, linear=True)
    _checkgrad(m)
    Xs = np.array([[-0.5], [0.25], [2.0]])
    mu, var = m.predict(Xs)
    mu0, var0 = m.predict_noiseless(Xs)
    assert np.allclose(mu, mu0) and np.all(var > var0) and np.all(var0 > 0)
    # the device prediction is the posterior's own formula with Kdiag by point (posterior.py:240-248), far outside Z as well
    post = m.posterior
    Kx = m.kern.K(m.Z.values, Xs)
    want_mu = np.dot(Kx.T, post.woodbury_vector)
    want = m.kern.Kdiag(Xs) - np.sum(np.dot(np.asarray(post.woodbury_inv).T, Kx) * Kx, 0)
    assert np.abs(mu0 - want_mu).max() <= 1e-9 * np.abs(want_mu).max()
    assert np.abs(var0[:, 0] - want).max() <= 1e-9 * np.abs(want).max()
    # six lengthscales and more past the inducing inputs the RBF part's K(Z, x*) is below 1e-9: what is left of the mean is
    # the Linear and Bias parts', affine in x* with the data's upward slope, and the variance grows with x*^2
    far = np.array([[3.0], [4.0], [5.0]])
    mf, vf = m.predict_noiseless(far)
    assert abs(mf[2, 0] - 2.0 * mf[1, 0] + mf[0, 0]) <= 1e-7 * abs(mf[1, 0]) and mf[1, 0] - mf[0, 0] > 0.1
    assert vf[2, 0] > vf[1, 0] > vf[0, 0] > var0[1, 0]
    S = m.posterior_samples_f(Xs, size=3)
    assert np.all(np.isfinite(S)) and S.shape == (3, 1, 3)
    mj, vj = m.predictive_gradients(Xs)                        # host side: kern.gradients_X / gradients_X_diag with Linear
    h = 1e-6
    fd = (m.predict_noiseless(Xs + h)[0] - m.predict_noiseless(Xs - h)[0]) / (2 * h)
    fdv = (m.predict_noiseless(Xs + h)[1] - m.predict_noiseless(Xs - h)[1]) / (2 * h)
    assert np.abs(mj[:, :, 0] - fd).max() <= 1e-5 * np.abs(fd).max() and np.abs(vj - fdv).max() <= 1e-5 * max(1.0, np.abs(fdv).max())
    l0 = m.log_likelihood()
    m.optimize(max_iters=60)
    assert m.log_likelihood() > l0
    # At the optimum central differences of the fp64 bound are no yardstick: kappa = cond2(Kmm + 1e-8 I) is of order 1e7 to 1e8
    # there, and a difference with h = 1e-6 carries |bound| kappa eps64 / h, of order 0.1, of rounding -- more than the gradient,
    # which is near zero.  The long-double restatement is: the bound, the kernel parameters' gradient and the Woodbury vector at
    # the optimised parameters under the judge's rule, with that kappa.  dZ is printed and not judged there: it is 1e-3 against
    # dL_dKmm entries of 1e3, the difference of terms six orders larger, and the rule's relative bound does not describe it.
    # Measured on an MI355X: kappa 2.45e8, lml 8.0e-10, dtheta 9.1e-6 (bound 1.4e-5), woodbury_vector 1.5e-5 (4.7e-4), dZ 1.4e-1 of
    # max |dZ| = 3.1e-3; the SAME fit with RBF + Bias alone, whose device code and bytes are what they were before Linear was
    # taken, ends at kappa 4.4e7 with dZ 1.8e-1 of max |dZ| = 1.4e-3: the loss is the sparse path's at an ill-conditioned
    # optimum, not the Linear part's.
    specs = [(s[0], int(bool(s[1])), np.asarray(s[2], np.float64), np.arange(1, dtype=np.int32) if s[3] is None else np.asarray(s[3]),
              s[4]) for s in m.kern.part_specs()]
    Zo, s2 = np.ascontiguousarray(m.Z.values), float(np.ravel(m.likelihood.variance.values)[0])
    ref, r64 = LL.vardtc(specs, X, Zo, Y, s2), LL.vardtc(specs, X, Zo, Y, s2, dt=np.float64)
    kappa = float(np.linalg.cond(KL.f64(ref["Kmm"])))
    fused = m.grad_dict["fused"]
    figs, bad = LL.judge(dict(lml=m.log_likelihood(), dtheta=fused["dtheta"], woodbury_vector=m.posterior.woodbury_vector), ref, r64,
                         kappa)
    print("at the optimum: kappa %.2e" % kappa, {q: "%.1e (bound %.1e)" % eb for q, eb in figs.items()},
          "dZ %.1e of max |dZ| = %.1e" % (LL.rel_err(fused["dZ"], ref["dZ"]), float(np.abs(KL.f64(ref["dZ"])).max())))
    assert not bad and set(figs) == {"lml", "dtheta", "woodbury_vector"}, bad


@pytest.mark.parametrize("inf", ["fitc", "pep"])
def test_sparse_gp_with_fitc_and_pep_and_a_linear_part(inf):
    import gpy_amd
    X, Y, rng = _toy(seed=1)
    Z = np.linspace(-1.0, 1.0, 10)[:, None]
    method = gpy_amd.FITC(linear=True) if inf == "fitc" else gpy_amd.PEP(0.5, linear=True)
    m = gpy_amd.SparseGP(X, Y, Z, _kern(), gpy_amd.Gaussian(variance=0.05), inference_method=method)
    _checkgrad(m)
    mu, var = m.predict(np.array([[0.3], [1.5]]))
    assert np.all(np.isfinite(mu)) and np.all(var > 0)


def test_svgp_and_sparse_classification_models_with_a_linear_part():
    import gpy_amd
    X, Y, rng = _toy(seed=2)
    Z = np.linspace(-1.0, 1.0, 8)[:, None]
    m = gpy_amd.SVGP(X, Y, Z, _kern(), gpy_amd.Gaussian(variance=0.05), linear=True)
    _checkgrad(m, tol=1e-4)
    mu, var = m.predict(np.array([[0.3], [1.5]]))
    assert np.all(np.isfinite(mu)) and np.all(var > 0)
    labels = (Y > np.median(Y)).astype(float)
    c = gpy_amd.SparseGPClassification(X, labels, kernel=_kern(), Z=Z, inference_method=gpy_amd.EPDTC(linear=True))
    p, _ = c.predict(np.array([[-0.9], [0.9]]))
    assert np.all((p >= 0) & (p <= 1)) and np.isfinite(c.log_likelihood()) and np.all(np.isfinite(c.gradient))
