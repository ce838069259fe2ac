"""GPU: the group-batched psi2 kernels (csrc/psi_missing.hip) through the stateless pair of include/mi355gp_sparse_missing.h,
against the long-double restatement of tests/missing_ld.py.

psi2_g (per group, relative to the group's largest entry) and the five gradients (relative to max |value|) are held to ten times
the distance of the float64 restatement from the long-double one that tests/test_oracle_missing.py measures on the same shapes
(`F64_DISTANCE`):
    psi2 1.7e-14   dvar 3.3e-14   dl 1.2e-14   dZ 1.7e-14   dmu 7.0e-14   dS 6.6e-14
The shapes (`CASES`) sit on the edges of the kernels' tilings; their masks hold a group observed in every row, a group observed
in the last row only (row 2048 of 2049: the first chunk is all zero for it) and a row in no group."""
import numpy as np
import pytest

import missing_ld as ML
from test_oracle_missing import CASES, F64_DISTANCE, GB, GRADS, reference, rel, rel_groups

pytestmark = pytest.mark.gpu


def _dev(p, ARD, loop=False):
    from gpy_amd import _lib
    a = (p["var"], p["ls"], ARD, p["Z"], p["mu"], p["S"], p["W"])
    return _lib.rbf_psi2_groups(*a, loop=loop), dict(zip(GRADS, _lib.rbf_psi_grad_groups(*a, p["dL"], loop=loop)))


def test_the_library_batches_eight_groups():
    from gpy_amd import _lib
    assert _lib.psi_groups_batch() == GB


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_group_statistics_and_gradients_against_long_double(case):
    name, N, M, Q, G, ARD = case
    p, r2, rg = reference(name)
    p2, g = _dev(p, ARD)
    figs = dict(psi2=rel_groups(p2, r2))
    figs.update((k, rel(g[k], rg[k])) for k in GRADS)
    print(name, "  ".join("%s %.1e" % kv for kv in figs.items()))
    for k in ("psi2",) + GRADS:
        assert figs[k] <= 10 * F64_DISTANCE[k], (k, figs[k])
    assert all(np.array_equal(x, x.T) for x in p2)                    # every psi2_g bitwise symmetric
    none = ~p["W"].any(1)                                             # rows in no group: exactly zero
    assert not np.any(g["dmu"][none]) and not np.any(g["dS"][none])
    q2, h = _dev(p, ARD)                                              # two evaluations, the same bytes
    assert np.array_equal(p2, q2) and all(np.array_equal(g[k], h[k]) for k in GRADS)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_psi2_groups_against_the_single_mask_kernel_once_per_group(case):
    """`mi355gp_rbf_psi` with weights = W[:, g], the kernel the batched one stands beside, under the same rule; and the loop route
    of the group calls (that kernel inside the same call), which the gradients are held to as well"""
    from gpy_amd import _lib
    name, N, M, Q, G, ARD = case
    p, r2, rg = reference(name)
    p2, g = _dev(p, ARD)
    for k in range(G):
        _, one = _lib.rbf_psi(p["var"], p["ls"], ARD, p["Z"], p["mu"], p["S"], weights=p["W"][:, k], want_psi1=False)
        assert rel(p2[k], one) <= 10 * F64_DISTANCE["psi2"], (k, rel(p2[k], one))
    l2, lg = _dev(p, ARD, loop=True)
    assert rel_groups(l2, r2) <= 10 * F64_DISTANCE["psi2"] and rel_groups(p2, l2) <= 10 * F64_DISTANCE["psi2"]
    for k in GRADS:
        assert rel(lg[k], rg[k]) <= 10 * F64_DISTANCE[k] and rel(g[k], lg[k]) <= 10 * F64_DISTANCE[k], k


def test_one_group_of_ones_is_the_unweighted_gradient_call():
    from gpy_amd import _lib
    p = ML.group_problem(65, 17, 3, 1, 5, True, edge_masks=False)
    p["W"][:] = 1.0
    a = (p["var"], p["ls"], True, p["Z"], p["mu"], p["S"])
    g = _lib.rbf_psi_grad_groups(*a, p["W"], p["dL"])
    h = _lib.rbf_psi_grad(*a, dL_dpsi2=p["dL"][0])
    for x, y, k in zip(g, h, GRADS):
        assert rel(x, y) <= 10 * F64_DISTANCE[k], k
    assert rel(_lib.rbf_psi2_groups(*a, p["W"])[0], _lib.rbf_psi(*a, want_psi1=False)[1]) <= 10 * F64_DISTANCE["psi2"]


def test_a_non_symmetric_dL_equals_its_symmetrisation_byte_for_byte():
    from gpy_amd import _lib
    p = ML.group_problem(63, 17, 2, 3, 7, False)
    a = (p["var"], p["ls"], False, p["Z"], p["mu"], p["S"], p["W"])
    sym = 0.5 * (p["dL"] + np.transpose(p["dL"], (0, 2, 1)))
    x, y = _lib.rbf_psi_grad_groups(*a, p["dL"]), _lib.rbf_psi_grad_groups(*a, sym)
    assert all(np.array_equal(u, v) for u, v in zip(x, y)) and not np.array_equal(p["dL"], sym)


def test_refusals_name_what_they_refuse():
    from gpy_amd import _lib
    p = ML.group_problem(5, 3, 2, 2, 0, True)
    a = [p["var"], p["ls"], True, p["Z"], p["mu"], p["S"]]
    W = p["W"].copy()
    W[3, 1] = np.nan
    with pytest.raises(_lib.MI355GPError, match=r"W\[3\]\[1\]"):
        _lib.rbf_psi2_groups(*a, W)
    with pytest.raises(_lib.MI355GPError, match=r"W\[3\]\[1\]"):
        _lib.rbf_psi_grad_groups(*a, W, p["dL"])
    S = p["S"].copy()
    S[2, 0] = 0.0
    with pytest.raises(_lib.MI355GPError, match=r"S\[2\]\[0\]"):
        _lib.rbf_psi2_groups(a[0], a[1], True, a[3], a[4], S, p["W"])
    r = np.random.default_rng(0)
    with pytest.raises(_lib.MI355GPError, match="65 input dimensions.*at most 64"):
        _lib.rbf_psi2_groups(1.0, np.ones(65), True, r.uniform(size=(3, 65)), r.uniform(size=(4, 65)), np.ones((4, 65)), np.ones((4, 1)))


# ---- the fit: mi355gp_sparse_set_output_groups + mi355gp_vardtc_inference_missing ------------------------------------------------
FIT_JUDGED = ("lml", "dtheta", "dnoise", "dZ", "dmu", "dS", "woodbury_vector", "woodbury_inv", "psi2", "dL_dKmm", "lml_g", "dnoise_g",
              "pred_mu", "pred_var", "upred_mu", "upred_var")


def _specs(p):
    import psi_ss_ld
    return psi_ss_ld.specs_of(p["k"])


def _fit(p, ctx=None, via_set_inputs=False):
    """(ctx, results) of one evaluation through the C-ABI, with every group's woodbury_inv and psi2 fetched"""
    from gpy_amd import _lib
    gof, W, Y0 = _lib.output_groups(p["Y"])
    ctx = ctx or _lib.SparseContext(0)
    if via_set_inputs:                                                # other inputs first: set_inputs keeps Y and the groups
        ctx.set_data(p["mu"] + 1.0, Y0)
        ctx.set_input_variance(2.0 * p["S"])
        ctx.set_output_groups(gof, W)
        ctx.set_inputs(p["mu"], p["S"])
    else:
        ctx.set_data(p["mu"], Y0)
        ctx.set_input_variance(p["S"])
        ctx.set_output_groups(gof, W)
    rc, r = ctx.vardtc_missing(_specs(p), p["Z"], p["noise"])
    assert rc == 0
    r["dL_dKmm"] = ctx.fetch(ctx.FETCH_DLDKMM)
    wi, p2 = [], []
    for g in range(W.shape[1]):
        ctx.select_output_group(g)
        wi.append(ctx.fetch(ctx.FETCH_WOODBURY_INV))
        p2.append(ctx.fetch(ctx.FETCH_PSI2))
    r.update(woodbury_inv=np.array(wi), psi2=np.array(p2), lml_g=r["group_scalars"][:, 0], dnoise_g=r["group_scalars"][:, 1])
    return ctx, r


def _judge(r, ref, r64):
    import sparse_ld as SL
    ref, r64 = dict(ref, lml=ref["bound"]), dict(r64, lml=r64["bound"])
    bad = []
    for q in FIT_JUDGED:
        if q not in r:
            continue
        e, b = SL.rel_err(r[q], np.asarray(ref[q], dtype=np.longdouble)), SL.bound(q, ref, r64, ref["kappa"])
        print("  %-16s err %.2e  bound %.2e" % (q, e, b))
        if not e <= b:
            bad.append("%s: %.3e > %.3e" % (q, e, b))
    return bad


@pytest.mark.parametrize("case", ML.FIT_CASES, ids=[c[0] for c in ML.FIT_CASES])
def test_fit_against_long_double(case):
    from test_oracle_missing import fit_reference
    p, ref, r64, Xs, Ss = fit_reference(case[0])
    assert ref["kappa"] <= 1e4
    ctx, r = _fit(p)
    r["pred_mu"], r["pred_var"] = ctx.predict_missing(_specs(p), Xs)
    r["upred_mu"], r["upred_var"] = ctx.predict_missing(_specs(p), Xs, Ss)
    bad = _judge(r, ref, r64)
    assert not bad, bad
    none = ~ref["W"].any(1)                                           # a row no output observes: exactly 0 from the fit
    assert not np.any(r["dmu"][none]) and not np.any(r["dS"][none])
    # two fresh contexts give the same bytes; set_inputs against a fresh set_data + groups likewise
    _, r2 = _fit(p)
    _, r3 = _fit(p, via_set_inputs=True)
    for q in ("lml", "dtheta", "dnoise", "dZ", "dmu", "dS", "woodbury_vector", "woodbury_inv", "psi2", "dL_dKmm", "group_scalars"):
        assert np.array_equal(r[q], r2[q]) and np.array_equal(r[q], r3[q]), q


def test_an_all_observed_mask_is_the_complete_data_evaluation():
    """G = 1, all ones: held to mi355gp_vardtc_inference_uncertain on the same data under the judge rule (bytes need not match)"""
    from gpy_amd import _lib
    import psi_np
    import sparse_ld as SL
    p = ML.lattice_problem(65, 17, 3, 5, 7, patterns=1)
    p["Y"] = np.nan_to_num(p["Y"], nan=0.3)                           # (the masks drop row 1 everywhere: fill it in)
    ctx, r = _fit(p)
    c2 = _lib.SparseContext(0)
    c2.set_data(p["mu"], p["Y"])
    c2.set_input_variance(p["S"])
    rc, u = c2.vardtc_uncertain(_specs(p), p["Z"], p["noise"])
    ev = lambda dt: psi_np.vardtc_uncertain(p["var"], p["ls"], True, p["white"], p["Z"], p["mu"], p["S"], p["Y"], p["noise"], dt)
    ref, r64 = ev(np.longdouble), ev(np.float64)
    kappa = ML.evaluate(p["var"], p["ls"], True, p["white"], p["Z"], p["mu"], p["S"], p["Y"], p["noise"])["kappa"]
    # each entry is held to the judge rule against long double; the two then differ by at most the sum of their two errors,
    # which is why the entry-against-entry comparison allows twice the bound
    for q in ("lml", "dnoise", "dZ", "dmu", "dS", "woodbury_vector"):
        b = SL.bound(q, ref, r64, kappa)
        assert SL.rel_err(r[q], np.asarray(ref[q], dtype=np.longdouble)) <= b and SL.rel_err(r[q], u[q]) <= 2 * b, q
    ref["dtheta"] = np.concatenate([np.ravel(ref["dvar"]), np.ravel(ref["dl"]), np.ravel(ref["dwhite"])])
    r64["dtheta"] = np.concatenate([np.ravel(r64["dvar"]), np.ravel(r64["dl"]), np.ravel(r64["dwhite"])])
    b = SL.bound("dtheta", ref, r64, kappa)
    assert SL.rel_err(r["dtheta"], ref["dtheta"]) <= b and SL.rel_err(u["dtheta"], ref["dtheta"]) <= b


def test_groups_are_cleared_by_g0_and_forgotten_by_set_data_and_the_gaussian_entry_is_unchanged():
    from gpy_amd import _lib
    p = ML.lattice_problem(63, 17, 2, 5, 7, patterns=3)
    gof, W, Y0 = _lib.output_groups(p["Y"])
    specs = _specs(p)
    fresh = _lib.SparseContext(0)
    fresh.set_data(p["mu"], Y0)
    fresh.set_input_variance(p["S"])
    with pytest.raises(_lib.MI355GPError, match="no output groups"):
        fresh.vardtc_missing(specs, p["Z"], p["noise"])
    rc, before = fresh.vardtc_uncertain(specs, p["Z"], p["noise"])
    ctx, r = _fit(p)
    with pytest.raises(_lib.MI355GPError, match="holds output groups"):
        ctx.vardtc_uncertain(specs, p["Z"], p["noise"])
    ctx.set_output_groups(None, None)                                 # G = 0
    rc, after = ctx.vardtc_uncertain(specs, p["Z"], p["noise"])
    for q in ("lml", "dtheta", "dnoise", "dZ", "dmu", "dS", "woodbury_vector"):
        assert np.array_equal(before[q], after[q]), q
    assert r["lml"] != before["lml"]
    ctx.set_output_groups(gof, W)
    ctx.set_data(p["mu"], Y0)                                         # set_data forgets the groups (and the variances)
    ctx.set_input_variance(p["S"])
    with pytest.raises(_lib.MI355GPError, match="no output groups"):
        ctx.vardtc_missing(specs, p["Z"], p["noise"])


def test_refusals_of_the_session_name_what_they_refuse():
    from gpy_amd import _lib
    p = ML.lattice_problem(33, 9, 2, 5, 7, patterns=2)
    gof, W, Y0 = _lib.output_groups(p["Y"])
    rbf, white = _specs(p)
    ctx = _lib.SparseContext(0)
    ctx.set_data(p["mu"], Y0)
    with pytest.raises(_lib.MI355GPError, match="no input variances"):
        ctx.set_output_groups(gof, W)
    ctx.set_input_variance(p["S"])
    bad = Y0.copy()
    bad[1, 3] = 0.7                                                   # row 1 is observed by nothing
    ctx.set_data(p["mu"], bad)
    ctx.set_input_variance(p["S"])
    with pytest.raises(_lib.MI355GPError, match=r"Y\[1\]\[3\]"):
        ctx.set_output_groups(gof, W)
    ctx.set_data(p["mu"], Y0)
    ctx.set_input_variance(p["S"])
    W0 = W.copy()
    W0[:, 1] = 0.0
    with pytest.raises(_lib.MI355GPError, match=r"group 1 \(first output 1\) has no observed row"):
        ctx.set_output_groups(gof, W0)
    ctx.set_output_groups(gof, W)
    for specs, pat in (([rbf, ("bias", False, np.array([0.5]), None, 0)], "Bias"), ([("linear", False, np.array([1.0]), None, 0)], "Linear"),
                       ([white], "no RBF part")):
        with pytest.raises(_lib.MI355GPError, match=pat):
            ctx.vardtc_missing(specs, p["Z"], p["noise"])
    with pytest.raises(_lib.MI355GPError, match="per-point noise"):
        ctx.vardtc_missing([rbf, white], p["Z"], np.full(33, 0.1))
    ctx.set_binary_prob(np.full(p["mu"].shape, 0.5))
    with pytest.raises(_lib.MI355GPError, match="slab probabilities"):
        ctx.vardtc_missing([rbf, white], p["Z"], p["noise"])
    with pytest.raises(_lib.MI355GPError, match="holds output groups"):
        ctx.vardtc_ss([rbf, white], p["Z"], p["noise"])
    ctx.set_binary_prob(None)
    lin = _lib.SparseContext(0)
    lin.set_psi_lin_bias(True)
    lin.set_data(p["mu"], Y0)
    lin.set_input_variance(p["S"])
    with pytest.raises(_lib.MI355GPError, match="psi_lin_bias"):
        lin.set_output_groups(gof, W)
    sh = _lib.SparseContext(0)
    sh.attach_loopback(0, 1, 7811)
    sh.set_data(p["mu"], Y0)
    with pytest.raises(_lib.MI355GPError, match="row-sharded"):
        sh.set_output_groups(gof, W)
    sh.close()
    rc, r = ctx.vardtc_missing([rbf, white], p["Z"], p["noise"])      # the context is still good
    assert rc == 0 and np.isfinite(r["lml"])


# ---- VarDTC.inference(missing_data=True) and BayesianGPLVMMiniBatch ------------------------------------------------------------
def _model(p, **kw):
    import gpy_amd
    Q = p["mu"].shape[1]
    kern = gpy_amd.RBF(Q, variance=p["var"], lengthscale=p["ls"], ARD=True) + gpy_amd.White(Q, variance=p["white"][0])
    return gpy_amd.BayesianGPLVMMiniBatch(p["Y"], Q, X=p["mu"], X_variance=p["S"], Z=p["Z"], kernel=kern,
                                          likelihood=gpy_amd.Gaussian(p["noise"]), missing_data=True, **kw)


def _model_against_restatement(m, Y):
    import sparse_ld as SL
    a = (float(m.kern.parts[0].variance.values[0]), m.kern.parts[0].lengthscale.values.copy(), True,
         [float(m.kern.parts[1].variance.values[0])], m.Z.values.copy(), m.X.mean.values.copy(), m.X.variance.values.copy(), Y,
         float(m.likelihood.variance.values[0]))
    ref, r64 = ML.evaluate(*a, dtype=np.longdouble), ML.evaluate(*a, dtype=np.float64)
    N, Q, M = m.num_data, m.input_dim, m.num_inducing
    g, o = m.gradient, 2 * N * Q
    got = dict(bound=m.log_likelihood(), dmu=m.X.mean.gradient, dS=m.X.variance.gradient, dZ=g[o:o + M * Q].reshape(M, Q),
               dtheta=g[o + M * Q:-1], dnoise=g[-1])
    for d in (ref, r64):
        d.update(dmu=d["dmu"] - d["kl_dmu"], dS=d["dS"] - d["kl_dS"],
                 dtheta=np.concatenate([np.ravel(d["dvar"]), np.ravel(d["dl"]), np.ravel(d["dwhite"])]))
    print("kappa %.3e" % ref["kappa"])
    bad = []
    for q in got:
        e, b = SL.rel_err(got[q], np.asarray(ref[q], dtype=np.longdouble)), SL.bound(q, ref, r64, ref["kappa"])
        print("  %-8s err %.2e  bound %.2e" % (q, e, b))
        if not e <= b:
            bad.append("%s: %.3e > %.3e" % (q, e, b))
    return ref, bad


def test_inference_keyword_posterior_and_grad_dict():
    import gpy_amd
    from test_oracle_missing import fit_reference
    p, ref, r64, Xs, Ss = fit_reference("n63_m65_q2_dy5_g3")
    kern = gpy_amd.RBF(2, variance=p["var"], lengthscale=p["ls"], ARD=True) + gpy_amd.White(2, variance=p["white"][0])
    q = gpy_amd.NormalPosterior(p["mu"], p["S"])
    inf = gpy_amd.VarDTC()
    post, lml, gd = inf.inference(kern, q, p["Z"], gpy_amd.Gaussian(p["noise"]), p["Y"], missing_data=True)
    f = gd["fused"]
    r = dict(lml=lml, dtheta=f["dtheta"], dnoise=gd["dL_dthetaL"], dZ=f["dZ"], dmu=f["dmu"], dS=f["dS"], woodbury_vector=post.woodbury_vector,
             dL_dKmm=np.asarray(gd["dL_dKmm"]), lml_g=f["group_scalars"][:, 0])
    r["pred_mu"], r["pred_var"] = post._raw_predict(kern, Xs, p["Z"])
    r["upred_mu"], r["upred_var"] = post._raw_predict(kern, gpy_amd.NormalPosterior(Xs, Ss), p["Z"])
    assert not _judge(r, ref, r64)
    Wi = post.woodbury_inv                                            # M x M x Dy, expanded from the G matrices
    assert Wi.shape == (65, 65, 5) and np.array_equal(Wi[:, :, 0], Wi[:, :, 3]) and not np.array_equal(Wi[:, :, 0], Wi[:, :, 1])
    import sparse_ld as SL
    assert SL.rel_err(np.moveaxis(Wi, 2, 0)[:3], np.asarray(ref["woodbury_inv"])) <= SL.bound("woodbury_inv", ref, r64, ref["kappa"])
    import pickle
    twin = pickle.loads(pickle.dumps(post))                           # no device handle travels; the copy predicts on the host
    assert twin._device is None and isinstance(twin.K, np.ndarray) and np.array_equal(twin.woodbury_inv, Wi)
    tm, tv = twin._raw_predict(kern, gpy_amd.NormalPosterior(Xs, Ss), p["Z"])
    assert SL.rel_err(tm, r["upred_mu"]) <= 1e-10 and SL.rel_err(tv, r["upred_var"]) <= 1e-9
    fresh, _, _ = gpy_amd.VarDTC().inference(kern, q, p["Z"], gpy_amd.Gaussian(p["noise"]), p["Y"], missing_data=True)
    assert np.array_equal(pickle.loads(pickle.dumps(fresh)).woodbury_inv, Wi)      # (expanded while it still can be)
    assert sorted(gd) == ["dL_dKmm", "dL_dpsi0", "dL_dpsi1", "dL_dthetaL", "fused"]
    assert SL.rel_err(gd["dL_dpsi0"], ref["dL_dpsi0"]) <= 1e-14 and SL.rel_err(np.asarray(gd["dL_dpsi1"]), ref["dL_dpsi1"]) <= 1e-10
    # stale: after the next evaluation the host route serves the posterior from the expanded woodbury_inv
    hm, hv = None, None
    inf.inference(kern, q, p["Z"], gpy_amd.Gaussian(2 * p["noise"]), p["Y"], missing_data=True)
    hm, hv = post._raw_predict(kern, Xs, p["Z"])
    assert SL.rel_err(hm, r["pred_mu"]) <= 1e-10 and SL.rel_err(hv, r["pred_var"]) <= 1e-9
    um, uv = post._raw_predict(kern, gpy_amd.NormalPosterior(Xs, Ss), p["Z"])
    assert SL.rel_err(um, r["upred_mu"]) <= 1e-10 and SL.rel_err(uv, r["upred_var"]) <= 1e-9
    # the same class without the keyword is the complete-data path again (the groups are cleared on the context)
    Yc = np.nan_to_num(p["Y"], nan=0.1)
    _, lml_c, _ = inf.inference(kern, q, p["Z"], gpy_amd.Gaussian(p["noise"]), Yc)
    _, lml_f, _ = gpy_amd.VarDTC().inference(kern, q, p["Z"], gpy_amd.Gaussian(p["noise"]), Yc)
    assert lml_c == lml_f


def test_model_checkgrad_optimisation_and_prediction():
    import gpy_amd
    p = ML.lattice_problem(40, 9, 3, 6, 5, patterns=3)
    assert ML.groups_of(p["Y"])[1].shape[1] == 3
    m = _model(p)
    assert [x.size for x in m.flattened_parameters()][:3] == [120, 120, 27]      # [X.mean, X.variance, Z, kernel, noise]
    np.random.seed(0)
    assert m.checkgrad()
    _, bad = _model_against_restatement(m, p["Y"])
    assert not bad, bad
    f0 = m.objective_function()
    m.optimize(max_iters=30)
    assert m.objective_function() < f0
    ref, bad = _model_against_restatement(m, p["Y"])                  # kappa at the optimum is printed, not judged
    assert not bad, bad
    r = np.random.default_rng(2)
    Xs, Ss = r.uniform(-0.5, 2.5, (11, 3)), r.uniform(0.05, 0.3, (11, 3))
    a = (float(m.kern.parts[0].variance.values[0]), m.kern.parts[0].lengthscale.values.copy(), [float(m.kern.parts[1].variance.values[0])],
         m.Z.values.copy(), ref)
    mu, var = m.predict_noiseless(Xs)
    rmu, rvar = ML.predict(*a, Xs, None, np.longdouble)
    assert mu.shape == var.shape == (11, 6) and rel(mu, rmu) <= 1e-6 and rel(var, rvar) <= 1e-5
    mu, var = m.predict_noiseless(gpy_amd.NormalPosterior(Xs, Ss))
    rmu, rvar = ML.predict(*a, Xs, Ss, np.longdouble)
    assert rel(mu, rmu) <= 1e-6 and rel(var, rvar) <= 1e-5
    with pytest.raises(NotImplementedError, match="infer_newX"):
        m.infer_newX(p["Y"][:2])
    # the removed entries, predicted at the learned q(X): finite, and of the outputs' scale
    mu, _ = m.predict_noiseless(m.X)
    assert np.all(np.isfinite(mu[np.isnan(p["Y"])]))


# ---- the reference's fixtures (tests/golden/missing) through the C-ABI, VarDTC.inference and the model ----------------------------
from test_oracle_missing import FIXTURES, FIXTURE_IDS, check_against_fixture, fixture_problem  # noqa: E402


@pytest.mark.parametrize("path", FIXTURES, ids=FIXTURE_IDS)
def test_fit_against_the_references_composed_loop(path):
    """at the sparse path's tolerances: 1e-9 bound, 1e-6 gradients and means, 1e-5 variances"""
    import gpy_amd
    g = np.load(path)
    p = fixture_problem(g)
    Q, (N, Dy), M = p["mu"].shape[1], p["Y"].shape, p["Z"].shape[0]
    p["k"] = dict(var=p["var"], ls=p["ls"], D=Q, dims=list(range(Q)), ARD=p["ARD"], white=p["white"])
    # the C-ABI
    ctx, r = _fit(p)
    assert np.array_equal(ctx.group_of_output, g["group_of_output"])
    pm, pv = ctx.predict_missing(_specs(p), g["Xs"])
    um, uv = ctx.predict_missing(_specs(p), g["Xs"], g["Ss"])
    Wi = np.moveaxis(r["woodbury_inv"][g["group_of_output"]], 0, 2)
    check_against_fixture(dict(lml=r["lml"], lml_g=r["lml_g"], woodbury_vector=r["woodbury_vector"], woodbury_inv=Wi, dL_dKmm=r["dL_dKmm"],
                               dnoise=np.ravel(r["dnoise"]), dtheta=r["dtheta"], dZ=r["dZ"], dmu=r["dmu"], dS=r["dS"], pred_mu=pm,
                               pred_var=pv, upred_mu=um, upred_var=uv), g)
    # VarDTC.inference(missing_data=True)
    mk = lambda: (lambda rbf: rbf if not p["white"] else gpy_amd.Add([rbf] + [gpy_amd.White(Q, variance=w) for w in p["white"]]))(
        gpy_amd.RBF(Q, variance=p["var"], lengthscale=p["ls"], ARD=p["ARD"]))
    kern = mk()
    post, lml, gd = gpy_amd.VarDTC().inference(kern, gpy_amd.NormalPosterior(p["mu"], p["S"]), p["Z"], gpy_amd.Gaussian(p["noise"]),
                                               p["Y"], missing_data=True)
    f = gd["fused"]
    pm, pv = post._raw_predict(kern, g["Xs"], p["Z"])
    um, uv = post._raw_predict(kern, gpy_amd.NormalPosterior(g["Xs"], g["Ss"]), p["Z"])
    check_against_fixture(dict(lml=lml, lml_g=f["group_scalars"][:, 0], woodbury_vector=post.woodbury_vector, woodbury_inv=post.woodbury_inv,
                               dL_dKmm=np.asarray(gd["dL_dKmm"]), dL_dpsi0=gd["dL_dpsi0"], dnoise=np.ravel(gd["dL_dthetaL"]),
                               dtheta=f["dtheta"], dZ=f["dZ"], dmu=f["dmu"], dS=f["dS"], pred_mu=pm, pred_var=pv, upred_mu=um,
                               upred_var=uv), g)
    # the model
    m = gpy_amd.BayesianGPLVMMiniBatch(p["Y"], Q, X=p["mu"], X_variance=p["S"], Z=p["Z"], kernel=mk(),
                                       likelihood=gpy_amd.Gaussian(p["noise"]), missing_data=True)
    grad, o = m.gradient, 2 * N * Q
    pm, pv = m.predict_noiseless(g["Xs"])
    um, uv = m.predict_noiseless(gpy_amd.NormalPosterior(g["Xs"], g["Ss"]))
    check_against_fixture(dict(bound=m.log_likelihood(), Xmean_grad=m.X.mean.gradient, Xvar_grad=m.X.variance.gradient,
                               dZ=grad[o:o + M * Q].reshape(M, Q), dtheta=grad[o + M * Q:-1], dnoise=grad[-1:], pred_mu=pm, pred_var=pv,
                               upred_mu=um, upred_var=uv), g)


def test_the_reference_side_binding_on_the_real_library():
    """integration/gpy_mi355x.py `make_missing_data_loop` bound to libmi355gp.so, against a fixture of the reference's own loop"""
    import os
    import sys
    import types
    from gpy_amd import _lib as L
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "integration"))
    import gpy_mi355x
    from test_missing_binding import _model
    g = np.load([f for f in FIXTURES if "white_dy12" in f][0])
    p = fixture_problem(g)
    loop = gpy_mi355x.make_missing_data_loop(gpy_mi355x.bind(L.LIB_PATH), gpy=types.SimpleNamespace(Posterior=lambda **kw: types.SimpleNamespace(**kw)))
    m = _model(p)
    m._outer_values_update = lambda fv: loop.outer_values_update(m, fv)
    loop.outer_loop(m)
    rbf, white = m.kern.parts
    check_against_fixture(dict(lml=m._log_marginal_likelihood, woodbury_vector=m.posterior.woodbury_vector,
                               woodbury_inv=m.posterior.woodbury_inv, dL_dKmm=m.full_values["dL_dKmm"], dL_dpsi0=m.full_values["dL_dpsi0"],
                               dnoise=np.ravel(m.likelihood.grad),
                               dtheta=np.concatenate([rbf.variance.gradient, rbf.lengthscale.gradient, white.variance.gradient]),
                               dZ=m.Z.gradient, dmu=m.X.mean.gradient, dS=m.X.variance.gradient), g)
    m.X.mean.values = p["mu"] + 0.01                                   # a second evaluation: set_inputs, the groups stay
    lml0 = m._log_marginal_likelihood
    loop.outer_loop(m)
    assert np.isfinite(m._log_marginal_likelihood) and m._log_marginal_likelihood != lml0
