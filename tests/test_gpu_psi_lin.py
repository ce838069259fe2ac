"""GPU: Linear and Bias psi-statistics on the sparse context (`mi355gp_sparse_set_psi_lin_bias`, include/mi355gp_psi_lin.h):
the uncertain-input fit and the prediction at uncertain points for ONE input-dependent part, Linear or RBF, with Bias and
White parts, against the long-double restatement of tests/psi_lin_ld.py.

Linear path: every judged quantity is held to `sparse_ld.bound`, err <= max(32 e64, 256 eps64 kappa), e64 the distance of the
fp64 restatement from the long-double one on the same inputs and kappa = cond2(Kmm + 1e-8 I) of the case.  Every case
carries a White part of at least 0.1 and the test asserts kappa <= 1e4.  Shapes, one at a time around N = 257, M = 17, D = 3,
Dy = 1: M across the 64-column tile of k_grad_rows_lin and the 128 padding granule, N across the 16 rows of a wave and the
64 rows of a workgroup, D across the fused / plain edge at 16 and the record groups of 32, and one case across the row-chunk
edge of the sparse context (N = 262145).

RBF + Bias path: N across PSI_GROWS (256) and PSI_CHUNK (2048), M across the 16- and 64-wide psi tiles, Q across the padded
dimension groups.  Bound per quantity: ten times the fp64 restatement's own distance from long double, the worst over the
cases of the sweep -- the rule of tests/test_gpu_psi.py and tests/test_gpu_bgplvm.py, whose constants are the worst figure
over their cases; one case's e64 alone is a random draw that can be far below the family's.

The row kernel alone (`mi355gp_dbg_psi_lin_rows`, include/mi355gp_debug_psi_lin.h) is exact on integer-valued operands.
"""
import numpy as np
import pytest

import psi_lin_ld as L
import sparse_ld as SL
from gpy_amd import _lib

pytestmark = pytest.mark.gpu

LD = np.longdouble
TOL_LML, TOL_FIT, TOL_VAR = 1e-9, 1e-6, 1e-5          # the fixtures' tolerances (tests/test_gpu_psi.py)
JUDGED = ("lml", "dtheta", "dnoise", "dZ", "dmu", "dS", "woodbury_vector", "psi2", "dL_dKmm", "pred_mean", "pred_var")
NPRED = 9


def _lin_case(name, N=257, M=17, D=3, Dy=1, ARD=True, dims=None, bias=(0.7,), white=(0.2,)):
    return dict(name=name, P="linear", N=N, M=M, D=D, Dy=Dy, ARD=ARD, dims=dims, bias=bias, white=white)


LINEAR_CASES = ([_lin_case("M%d" % M, M=M) for M in (1, 16, 17, 127, 128, 129, 257)] +
                [_lin_case("N%d" % N, N=N) for N in (1, 15, 16, 17, 255, 256, 257)] +
                [_lin_case("D%d" % D, D=D) for D in (1, 15, 16, 17, 32, 33, 64)] +
                [_lin_case("Dy3", Dy=3), _lin_case("iso", ARD=False), _lin_case("subset", D=4, dims=(0, 2, 3)),
                 _lin_case("two_bias", bias=(0.7, 0.3)), _lin_case("alone_white", bias=()),
                 _lin_case("chunk_edge", N=262145, M=3, D=2)])


def _rbf_case(name, N=257, M=17, D=3, Dy=2, ARD=True, bias=(0.7,), white=(0.1,)):
    return dict(name=name, P="rbf", N=N, M=M, D=D, Dy=Dy, ARD=ARD, dims=None, bias=bias, white=white)


RBF_SWEEP = ([_rbf_case("N%d" % N) for N in (1, 255, 256, 257, 2047, 2048, 2049)] +
             [_rbf_case("M%d" % M, M=M) for M in (15, 16, 17, 63, 64, 65)] +
             [_rbf_case("Q%d" % Q, D=Q) for Q in (1, 16, 17, 32, 33, 64)])
# two Bias parts (the reference has no exact evaluation of them, so no fixture can): held to the sweep's bounds, not adding to them
RBF_CASES = RBF_SWEEP + [_rbf_case("two_bias", bias=(0.7, 0.3)), _rbf_case("two_bias_dy1_m65", bias=(0.4, 0.9), Dy=1, M=65)]
_REF = {}


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _reference(c):
    """(problem, long-double reference, fp64 reference) of a case, computed once and left unchanged"""
    key = (c["P"], c["name"])
    if key not in _REF:
        seed = 1000 + sum(ord(ch) for ch in c["P"] + c["name"])
        p = L.problem(c["P"], c["N"], c["M"], c["D"], c["Dy"], seed, ARD=c["ARD"], bias=c["bias"], white=c["white"], dims=c["dims"])
        r = np.random.default_rng(seed + 1)
        p["mu_new"], p["S_new"] = r.uniform(-2, 2, (NPRED, c["D"])), r.uniform(0.05, 0.5, (NPRED, c["D"]))
        out = []
        for dt in (LD, np.float64):
            ref = L.evaluate(p["k"], p["Z"], p["mu"], p["S"], p["Y"], p["noise"], dt)
            ref["pred_mean"], ref["pred_var"] = L.predict(p["k"], p["Z"], ref, p["mu_new"], p["S_new"], dt)
            out.append(_freeze(ref))
        _REF[key] = (_freeze(p), out[0], out[1])
    return _REF[key]


def _device(p, want_pred=True):
    """one fit and one prediction at uncertain points in a fresh context"""
    specs = L.part_specs(p["k"])
    ctx = _lib.SparseContext(0)
    ctx.set_psi_lin_bias(True)
    ctx.set_data(p["mu"], p["Y"])
    ctx.set_input_variance(p["S"])
    rc, r = ctx.vardtc_uncertain(specs, p["Z"], p["noise"])
    assert rc == 0
    got = dict(lml=r["lml"], dtheta=r["dtheta"], dnoise=np.atleast_1d(r["dnoise"]), dZ=r["dZ"], dmu=r["dmu"], dS=r["dS"],
               woodbury_vector=r["woodbury_vector"], psi2=ctx.fetch(ctx.FETCH_PSI2), dL_dKmm=ctx.fetch(ctx.FETCH_DLDKMM))
    if want_pred:
        got["pred_mean"], got["pred_var"] = ctx.predict_uncertain(specs, p["mu_new"], p["S_new"])
    return got, ctx


def _as_ref(ref):
    d = dict(ref)
    d["dnoise"] = np.atleast_1d(ref["dnoise"])
    return d


@pytest.mark.parametrize("c", LINEAR_CASES, ids=[c["name"] for c in LINEAR_CASES])
def test_linear_path_meets_the_long_double_restatement(c):
    p, ref, r64 = _reference(c)
    kappa = ref["kappa"]
    assert kappa <= 1e4, "case %s: cond2(Kmm + 1e-8 I) = %.3g exceeds the cap of the sweep" % (c["name"], kappa)
    got, _ = _device(p)
    ref, r64 = _as_ref(ref), _as_ref(r64)
    bad = []
    for q in JUDGED:
        e, b = SL.rel_err(got[q], ref[q]), SL.bound(q, ref, r64, kappa)
        print("%s %-16s err %.3e bound %.3e" % (c["name"], q, e, b))
        if not e <= b:
            bad.append("%s: %.3e > %.3e" % (q, e, b))
    if c["dims"] is not None:                                   # columns the part does not see get no gradient
        rest = [d for d in range(c["D"]) if d not in c["dims"]]
        assert not got["dZ"][:, rest].any() and not got["dmu"][:, rest].any() and not got["dS"][:, rest].any()
    assert not bad, "kappa %.3g; %s" % (kappa, "; ".join(bad))


def _family_e64(cases):
    """per judged quantity the worst distance of the fp64 restatement from the long-double one over the family"""
    worst = dict((q, 0.0) for q in JUDGED)
    for c in cases:
        _, ref, r64 = _reference(c)
        ref, r64 = _as_ref(ref), _as_ref(r64)
        for q in JUDGED:
            worst[q] = max(worst[q], SL.rel_err(r64[q], ref[q]))
    return worst


@pytest.mark.parametrize("c", RBF_CASES, ids=[c["name"] for c in RBF_CASES])
def test_rbf_plus_bias_path_meets_the_long_double_restatement(c):
    p, ref, _ = _reference(c)
    e64 = _family_e64(RBF_SWEEP)
    got, _ = _device(p)
    ref = _as_ref(ref)
    bad = []
    for q in JUDGED:
        e, b = SL.rel_err(got[q], ref[q]), 10.0 * e64[q]
        print("%s %-16s err %.3e bound %.3e (kappa %.3g)" % (c["name"], q, e, b, ref["kappa"]))
        if not e <= b:
            bad.append("%s: %.3e > %.3e" % (q, e, b))
    assert not bad, "; ".join(bad)


def _int_problem(rows, M, D, seed):
    r = np.random.default_rng(seed)
    i = lambda *s: r.integers(-3, 4, s).astype(np.float64)
    return dict(W=i(rows, M), Y=i(rows, 2), V=i(M, 2), X=i(rows, D), Z=i(M, D), rs=r.integers(1, 3, rows).astype(np.float64),
                var=r.choice([1.0, 4.0], D))


@pytest.mark.parametrize("D", [1, 16, 17, 64])
@pytest.mark.parametrize("M", [1, 17, 129])
@pytest.mark.parametrize("rows", [1, 17, 257])
def test_row_kernel_alone_is_exact_on_integers(rows, M, D):
    """integer-valued W, Y, V, Z, X, row scales and square-rooted variances: every product and sum is an integer far below
    2^53, so the result is exact whatever the order.  D <= 16: k_grad_rows_lin with the weights formed on the fly; above, the
    weights in memory and the plain kernel (the path the fit takes there)."""
    q = _int_problem(rows, M, D, 7 + rows + M + D)
    beta, gscale, c0 = 2.0, 2.0, -3.0
    g = q["rs"][:, None] * (gscale * q["W"] + beta * q["Y"] @ q["V"].T)
    want = q["var"] * (g @ q["Z"] + c0 * q["X"])
    got = _lib.psi_lin_rows_probe(q["W"], q["X"], q["Z"], q["var"], c0=c0, Y=q["Y"], V=q["V"], rowscale=q["rs"], beta=beta,
                                  gscale=gscale, fused=D <= 16)
    assert np.array_equal(got, want)
    plain = q["var"] * (q["W"] @ q["Z"] + c0 * q["X"])         # no rank term: the weights as given
    assert np.array_equal(_lib.psi_lin_rows_probe(q["W"], q["X"], q["Z"], q["var"], c0=c0, fused=D <= 16), plain)
    if D <= 16:                                                 # the plain kernel at the fused kernel's sizes as well
        assert np.array_equal(_lib.psi_lin_rows_probe(q["W"], q["X"], q["Z"], q["var"], c0=c0, Y=q["Y"], V=q["V"], rowscale=q["rs"],
                                                      beta=beta, gscale=gscale, fused=False), want)


@pytest.mark.parametrize("bias", [(0.7,), (0.7, 0.3)], ids=["one_bias", "two_bias"])
@pytest.mark.parametrize("P", ["linear", "rbf"])
def test_two_fits_and_predictions_in_fresh_contexts_give_identical_bytes(P, bias):
    """N = 4097 is across two PSI_CHUNK edges (RBF) and is 65 workgroups of the row kernel (Linear); with one Bias part and
    with two (every Bias part gets its own gradient from the shared sums)"""
    c = dict(name="bytes%d" % len(bias), P=P, N=4097, M=17, D=3, Dy=2, ARD=True, dims=None, bias=bias, white=(0.2,))
    p, ref, _ = _reference(c)
    a, _ = _device(p)
    b, _ = _device(p)
    for q in JUDGED:
        assert np.array_equal(np.asarray(a[q]), np.asarray(b[q])), q
    ref = _as_ref(ref)
    assert SL.rel_err(a["lml"], ref["lml"]) <= TOL_LML
    for q in JUDGED[1:]:
        assert SL.rel_err(a[q], ref[q]) <= (TOL_VAR if q == "pred_var" else TOL_FIT), q


def test_switch_off_refuses_as_before_and_the_last_result_still_predicts():
    c = _lin_case("switch", N=40, M=6)
    p, ref, _ = _reference(c)
    got, ctx = _device(p)
    specs = L.part_specs(p["k"])
    mu0, var0 = ctx.predict(specs, p["mu_new"])
    ctx.set_psi_lin_bias(False)
    with pytest.raises(_lib.MI355GPError, match="Linear.*uncertain inputs take one RBF part and White parts only"):
        ctx.predict_uncertain(specs, p["mu_new"], p["S_new"])
    mu1, var1 = ctx.predict(specs, p["mu_new"])                # the refusal left the result alone
    assert np.array_equal(mu0, mu1) and np.array_equal(var0, var1)
    with pytest.raises(_lib.MI355GPError, match="Linear.*uncertain inputs take one RBF part and White parts only"):
        ctx.vardtc_uncertain(specs, p["Z"], p["noise"])
    rbf = ("rbf", True, np.array([1.3, 1.0, 1.2, 0.9]), None, 0)
    with pytest.raises(_lib.MI355GPError, match="Bias.*uncertain inputs take one RBF part and White parts only"):
        ctx.vardtc_uncertain([rbf, ("bias", False, np.array([0.5]), None, 0)], p["Z"], p["noise"])
    ctx.set_psi_lin_bias(True)
    for bad, pat in (([rbf, specs[0]], "both input-dependent"), ([rbf, rbf], "both input-dependent"),
                     ([rbf[:4] + (1,), specs[1][:4] + (1,)], "product"),
                     ([("matern52", False, np.array([1.0, 1.0]), None, 0), specs[1]], "Matern52"),
                     ([specs[1], specs[2]], "no RBF or Linear part")):
        with pytest.raises(_lib.MI355GPError, match=pat):
            ctx.vardtc_uncertain(bad, p["Z"], p["noise"])
    with pytest.raises(_lib.MI355GPError, match="per-point noise"):
        ctx.vardtc_uncertain(specs, p["Z"], np.full(c["N"], 0.1))
    rc, r = ctx.vardtc_uncertain(specs, p["Z"], p["noise"])     # the context is still good, with the same bytes
    assert rc == 0 and r["lml"] == got["lml"] and np.array_equal(r["dmu"], got["dmu"])


def test_bayesian_gplvm_with_linear_ard_plus_bias_plus_white():
    """N = 60, Q = 3, Dy = 5: checkgrad at the start; after 30 L-BFGS-B steps the bound and every gradient against the
    long-double restatement at the optimised parameters (`sparse_ld.bound` with the kappa found there, no central differences:
    at an optimum the gradients are differences of large terms); prediction at uncertain points on the live posterior against
    the host fallback through `Linear.psi*` / `Bias.psi*` / `Add.psi*(psi_lin_bias=True)`."""
    import gpy_amd
    r = np.random.default_rng(5)
    N, Q, Dy = 60, 3, 5
    Xt = r.standard_normal((N, 2))
    Y = Xt @ r.standard_normal((2, Dy)) + 0.5 + 0.1 * r.standard_normal((N, Dy))
    k = gpy_amd.Linear(Q, variances=r.uniform(0.5, 1.5, Q), ARD=True) + gpy_amd.Bias(Q, variance=0.5) + gpy_amd.White(Q, variance=0.2)
    m = gpy_amd.BayesianGPLVM(Y, Q, X=r.standard_normal((N, Q)), X_variance=r.uniform(0.1, 0.5, (N, Q)), Z=r.uniform(-2, 2, (8, Q)),
                              kernel=k, psi_lin_bias=True)
    assert [p.name for p in m.flattened_parameters()] == ["mean", "variance", "inducing inputs", "variances", "variance", "variance",
                                                          "variance"]
    assert m.checkgrad()
    m.optimize(max_iters=30)
    kd = dict(P="linear", D=Q, dims=list(range(Q)), ARD=True, v=k.parts[0].variances.values.copy(),
              bias=[float(k.parts[1].variance.values[0])], white=[float(k.parts[2].variance.values[0])])
    args = (kd, m.Z.values, m.X.mean.values, m.X.variance.values, Y, float(m.likelihood.variance.values[0]))
    ref, r64 = _as_ref(L.evaluate(*args, dt=LD)), _as_ref(L.evaluate(*args, dt=np.float64))
    kappa = ref["kappa"]
    f = m.grad_dict["fused"]
    KL = m.variational_prior.KL_divergence(m.X)
    got = dict(lml=m.log_likelihood() + KL, dtheta=f["dtheta"], dnoise=np.atleast_1d(m.grad_dict["dL_dthetaL"]), dZ=f["dZ"],
               dmu=f["dmu"], dS=f["dS"], woodbury_vector=m.posterior.woodbury_vector)
    bad = []
    for q in got:
        e, b = SL.rel_err(got[q], ref[q]), SL.bound(q, ref, r64, kappa)
        print("optimum %-16s err %.3e bound %.3e (kappa %.3g)" % (q, e, b, kappa))
        if not e <= b:
            bad.append("%s: %.3e > %.3e" % (q, e, b))
    assert not bad, "kappa %.3g; %s" % (kappa, "; ".join(bad))
    qn = gpy_amd.NormalPosterior(r.uniform(-1, 1, (7, Q)), r.uniform(0.05, 0.4, (7, Q)))
    mu_d, var_d = m.predict(qn, include_likelihood=False)
    assert m.posterior._live(m.kern)
    post = m.posterior
    mu_h, var_h = post._raw_predict_uncertain(m.kern, qn, m.Z.values, False, None)      # the host fallback
    assert SL.rel_err(mu_d, mu_h) <= TOL_FIT and SL.rel_err(var_d, var_h) <= TOL_VAR


# ---- the reference's own fixtures (tests/golden/psi_lin, tools/make_golden_psi_lin.py) through the device -------------------------
import glob  # noqa: E402
import os  # noqa: E402

from test_oracle_psi_lin import fixture_description  # noqa: E402

FIXTURES = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "psi_lin", "*.npz")))
FIX_IDS = [os.path.basename(f)[:-4] for f in FIXTURES]


def _check_fit(tag, g, lml, wv, dtheta, dnoise, dZ, dmu, dS):
    figs = {"lml": abs(lml - float(g["lml"])) / abs(float(g["lml"]))}
    for name, x, y in (("woodbury_vector", wv, g["woodbury_vector"]), ("dtheta", dtheta, g["dtheta"]),
                       ("dnoise", np.atleast_1d(dnoise), g["dnoise"]), ("dZ", dZ, g["dZ"]), ("dmu", dmu, g["dmu"]), ("dS", dS, g["dS"])):
        figs[name] = SL.rel_err(x, np.asarray(y, dtype=LD))
    print(tag, {k: "%.2e" % v for k, v in figs.items()})
    assert figs.pop("lml") <= TOL_LML
    for name, e in figs.items():
        assert e <= TOL_FIT, (name, e)


@pytest.mark.parametrize("path", FIXTURES, ids=FIX_IDS)
def test_fixture_through_the_c_abi_the_inference_class_and_the_models(path):
    import gpy_amd
    from gpy_amd.likelihoods import Gaussian
    from gpy_amd.sparse import VarDTC
    g = np.load(path)
    k = fixture_description(g)
    dims, specs = k["dims"], L.part_specs(k)
    noise = float(g["noise"])
    # the C-ABI: the full-width arrays, the parts carry their active dimensions
    ctx = _lib.SparseContext(0)
    ctx.set_psi_lin_bias(True)
    ctx.set_data(g["mu"], g["Y"])
    ctx.set_input_variance(g["S"])
    rc, r = ctx.vardtc_uncertain(specs, g["Z"], noise)
    assert rc == 0
    rest = [d for d in range(k["D"]) if d not in dims]
    assert not r["dZ"][:, rest].any() and not r["dmu"][:, rest].any() and not r["dS"][:, rest].any()
    _check_fit("c-abi", g, r["lml"], r["woodbury_vector"], r["dtheta"], r["dnoise"], r["dZ"][:, dims], r["dmu"][:, dims], r["dS"][:, dims])
    mu, var = ctx.predict(specs, g["Xs"])
    um, uv = ctx.predict_uncertain(specs, g["Xs"], g["Ss"])
    assert SL.rel_err(mu, g["pred_mu"].astype(LD)) <= TOL_FIT and SL.rel_err(var, g["pred_var"].astype(LD)) <= TOL_VAR
    assert SL.rel_err(um, g["upred_mu"].astype(LD)) <= TOL_FIT and SL.rel_err(uv, g["upred_var"].astype(LD)) <= TOL_VAR
    assert SL.rel_err(ctx.fetch(ctx.FETCH_DLDKMM), g["dL_dKmm"].astype(LD)) <= 1e-4          # (as tests/test_gpu_sparse.py)
    # VarDTC.inference
    q = gpy_amd.NormalPosterior(g["mu"], g["S"])
    kern = L.make_kernel(k)
    post, lml, gd = VarDTC(psi_lin_bias=True).inference(kern, q, g["Z"], Gaussian(variance=noise), g["Y"])
    f = gd["fused"]
    pick = slice(None) if f["dZ"].shape[1] == len(dims) else dims
    _check_fit("VarDTC", g, lml, post.woodbury_vector, f["dtheta"], gd["dL_dthetaL"], f["dZ"][:, pick], f["dmu"][:, pick], f["dS"][:, pick])
    assert SL.rel_err(np.asarray(gd["dL_dpsi1"]), g["dL_dpsi1"].astype(LD)) <= TOL_FIT
    assert SL.rel_err(np.asarray(gd["dL_dpsi2"]), g["dL_dpsi2"].astype(LD)) <= 1e-4
    # SparseGPRegression(X_variance=) and BayesianGPLVM: [Z, kernel, noise] and [X.mean, X.variance, Z, kernel, noise]
    M, D = g["Z"].shape
    N = g["mu"].shape[0]
    m = gpy_amd.SparseGPRegression(g["mu"], g["Y"], kernel=L.make_kernel(k), Z=g["Z"], noise_var=noise, X_variance=g["S"], psi_lin_bias=True)
    grad = m.gradient
    fm = m.grad_dict["fused"]
    pk = slice(None) if fm["dmu"].shape[1] == len(dims) else dims
    _check_fit("SparseGPRegression", g, m.log_likelihood(), m.posterior.woodbury_vector, grad[M * D:-1], grad[-1:],
               grad[:M * D].reshape(M, D)[:, dims], fm["dmu"][:, pk], fm["dS"][:, pk])
    mu, var = m.predict(g["Xs"], include_likelihood=False)
    assert SL.rel_err(mu, g["pred_mu"].astype(LD)) <= TOL_FIT and SL.rel_err(var, g["pred_var"].astype(LD)) <= TOL_VAR
    b = gpy_amd.BayesianGPLVM(g["Y"], D, X=g["mu"], X_variance=g["S"], Z=g["Z"], kernel=L.make_kernel(k),
                              likelihood=Gaussian(variance=noise), psi_lin_bias=True)
    # (the model's KL term runs over every column of X, the fixture's over the active ones the reference was given)
    KL = 0.5 * ((g["mu"] ** 2).sum() + (g["S"] - np.log(g["S"])).sum() - g["mu"].size)
    bound = float(g["bound"]) if len(dims) == D else float(g["lml"]) - KL
    assert abs(b.log_likelihood() - bound) <= TOL_LML * abs(bound)
    gb = b.gradient
    assert SL.rel_err(gb[:N * D].reshape(N, D)[:, dims], g["Xmean_grad"].astype(LD)) <= TOL_FIT
    assert SL.rel_err(gb[N * D:2 * N * D].reshape(N, D)[:, dims], g["Xvar_grad"].astype(LD)) <= TOL_FIT
    assert SL.rel_err(gb[2 * N * D + M * D:-1], g["dtheta"].astype(LD)) <= TOL_FIT
    um, uv = b.predict(gpy_amd.NormalPosterior(g["Xs"], g["Ss"]), include_likelihood=False)
    assert SL.rel_err(um, g["upred_mu"].astype(LD)) <= TOL_FIT and SL.rel_err(uv, g["upred_var"].astype(LD)) <= TOL_VAR


@pytest.mark.parametrize("path", [f for f in FIXTURES if os.path.basename(f).startswith("rbf")],
                         ids=[i for i in FIX_IDS if i.startswith("rbf")])
def test_host_psi_statistics_of_rbf_plus_bias_meet_the_reference(path):
    """`Add.psi*(psi_lin_bias=True)` over an RBF part (its own statistics come from the device) with the three gradient methods"""
    import gpy_amd
    g = np.load(path)
    k = fixture_description(g)
    dims = k["dims"]
    q, q4 = gpy_amd.NormalPosterior(g["mu"][:, dims], g["S"][:, dims]), gpy_amd.NormalPosterior(g["mu"][:4, dims], g["S"][:4, dims])
    Z = g["Z"][:, dims]
    kern = L.make_kernel(k)
    kw = dict(psi_lin_bias=True)
    for name, x in (("psi0", kern.psi0(Z, q, **kw)), ("psi1", kern.psi1(Z, q, **kw)), ("psi2", kern.psi2(Z, q, **kw)),
                    ("psi2n", kern.psi2n(Z, q4, **kw))):
        assert SL.rel_err(x, g["ks_" + name].astype(LD)) <= 1e-12, name
    assert SL.rel_err(kern.psi2n(Z, q, **kw).sum(0), kern.psi2(Z, q, **kw).astype(LD)) <= 1e-13
    d0, d1, d2 = g["k_d0"], g["k_d1"], g["k_d2"]
    kern.update_gradients_expectations(d0, d1, d2, Z, q, **kw)
    got = np.concatenate([np.atleast_1d(np.asarray(p.gradient, dtype=float)).ravel() for p in kern.flattened_parameters()])
    assert SL.rel_err(got, g["ks_dtheta"].astype(LD)) <= 1e-10
    assert SL.rel_err(kern.gradients_Z_expectations(d0, d1, d2, Z, q, **kw), g["ks_dZ"].astype(LD)) <= 1e-10
    gm, gs = kern.gradients_qX_expectations(d0, d1, d2, Z, q, **kw)
    assert SL.rel_err(gm, g["ks_dmu"].astype(LD)) <= 1e-10 and SL.rel_err(gs, g["ks_dS"].astype(LD)) <= 1e-10


def test_host_psi_statistics_of_rbf_plus_two_bias_parts_meet_the_long_double_restatement():
    """`Add.psi*(psi_lin_bias=True)` and the three gradient methods over RBF + Bias + Bias + White (the RBF part's own statistics
    come from the device) against tests/psi_lin_ld.py in long double; the reference has no exact evaluation of two Bias parts"""
    import gpy_amd
    from test_oracle_psi_lin import two_bias_yardstick
    p = L.problem("rbf", 23, 6, 3, 2, 17, bias=(0.7, 0.3), white=(0.2,))
    kern = L.make_kernel(p["k"])
    want, d = two_bias_yardstick(p)
    q = gpy_amd.NormalPosterior(p["mu"], p["S"])
    kw = dict(psi_lin_bias=True)
    for name, x in (("psi0", kern.psi0(p["Z"], q, **kw)), ("psi1", kern.psi1(p["Z"], q, **kw)), ("psi2", kern.psi2(p["Z"], q, **kw)),
                    ("psi2n", kern.psi2n(p["Z"], q, **kw))):
        assert SL.rel_err(x, want[name]) <= 1e-12, name
    kern.update_gradients_expectations(d[0], d[1], d[2], p["Z"], q, **kw)
    got = np.concatenate([np.atleast_1d(np.asarray(t.gradient, dtype=float)).ravel() for t in kern.flattened_parameters()])
    assert SL.rel_err(got, want["dtheta"]) <= 1e-10
    assert SL.rel_err(kern.gradients_Z_expectations(d[0], d[1], d[2], p["Z"], q, **kw), want["dZ"]) <= 1e-10
    gm, gs = kern.gradients_qX_expectations(d[0], d[1], d[2], p["Z"], q, **kw)
    assert SL.rel_err(gm, want["dmu"]) <= 1e-10 and SL.rel_err(gs, want["dS"]) <= 1e-10
