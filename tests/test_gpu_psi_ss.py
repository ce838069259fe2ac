"""GPU: the spike-and-slab RBF psi-statistics (csrc/psi_ss.hip), the fit that stands on them (`mi355gp_vardtc_inference_ss`) and
`SSGPLVM`, against the long-double restatement of tests/psi_ss_ld.py and the reference's fixtures in tests/golden/psi_ss (statistics
and gradients, and three whole fits composed from the reference's pieces, held to the sparse path's tolerances).

Bounds of the stateless calls: psi1 <= 1e-13 variance absolute (the project's tolerance for K); psi2 and the six gradients,
relative to max |value|, ten times the distance of the fp64 restatement from the long-double one that
tests/test_oracle_psi_ss.py measures on the same shapes (`F64_DISTANCE`):
    psi2 2.3e-14   dvar 7.8e-15   dl 2.0e-13   dZ 3.8e-14   dmu 6.4e-14   dS 6.7e-14   dgamma 6.0e-13
Measured on the device, worst over the shapes: psi1 3.3e-15 absolute, psi2 1.9e-15, dvar 2.0e-15, dl 1.1e-15, dZ 1.5e-15,
dmu 1.3e-15, dS 2.1e-15, dgamma 1.2e-14.
The fit is judged by tests/sparse_ld.py's rule, max(32 e64(q), 256 eps64 kappa) per quantity, on inputs with kappa <= 1e4 (the CPU
test asserts the cap)."""
import os

import numpy as np
import pytest

import psi_ss_ld as P
import sparse_ld as SL
from test_oracle_psi_ss import F64_DISTANCE, FIT_FIXTURES, FIT_IDS, GRADS, check_fit_against_fixture

pytestmark = pytest.mark.gpu
LD = np.longdouble
HERE = os.path.dirname(os.path.abspath(__file__))
TOL_LML, TOL_FIT, TOL_VAR = 1e-9, 1e-6, 1e-5       # the sparse path's tolerances (tests/test_gpu_sparse.py)
FIT_JUDGED = ("lml", "dtheta", "dnoise", "dZ", "dmu", "dS", "dgamma", "woodbury_vector")


def _rel(x, ref):
    ref = np.asarray(ref, dtype=LD)
    return float(np.abs(np.asarray(x, dtype=LD) - ref).max() / max(float(np.abs(ref).max()), 1e-300))


def _dev(c, ARD, dL=("dL0", "dL1", "dL2"), weights=True):
    from gpy_amd import _lib
    a = (c["variance"], c["lengthscale"], ARD, c["Z"], c["mu"], c["S"], c["gamma"])
    w = c["weights"] if weights else None
    p1, p2 = _lib.ssrbf_psi(*a, weights=w)
    g = _lib.ssrbf_psi_grad(*a, dL_dpsi0=None if dL[0] is None else c[dL[0]], dL_dpsi1=None if dL[1] is None else c[dL[1]],
                            dL_dpsi2=None if dL[2] is None else c[dL[2]], weights=w)
    return p1, p2, dict(zip(GRADS, g))


def _ref(c, dL=("dL0", "dL1", "dL2"), dtype=LD):
    kw = dict((k, c[k]) for k in ("variance", "lengthscale", "Z", "mu", "S", "gamma", "weights"))
    _, p1, p2 = P.stats(dtype=dtype, **kw)
    g = P.grads(dL_dpsi0=None if dL[0] is None else c[dL[0]], dL_dpsi1=None if dL[1] is None else c[dL[1]],
                dL_dpsi2=None if dL[2] is None else c[dL[2]], dtype=dtype, **kw)
    return p1, p2, g


@pytest.mark.parametrize("case", P.CASES, ids=[c[0] for c in P.CASES])
def test_stateless_statistics_and_gradients_against_long_double(case):
    name, N, M, Q, ARD, wt = case
    c = P.make_case(N, M, Q, ARD, wt)
    p1, p2, g = _dev(c, ARD)
    r1, r2, rg = _ref(c)
    figs = dict(psi1=float(np.abs(p1 - r1).max()) / c["variance"], psi2=_rel(p2, r2))
    figs.update((k, _rel(g[k], rg[k])) for k in GRADS)
    print(name, "  ".join("%s %.1e" % kv for kv in figs.items()))
    assert figs["psi1"] <= 1e-13
    for k in ("psi2",) + GRADS:
        assert figs[k] <= 10 * F64_DISTANCE[k], (k, figs[k])
    assert np.array_equal(p2, p2.T)                                   # bitwise symmetric
    q1, q2, h = _dev(c, ARD)                                          # two evaluations, the same bytes
    assert np.array_equal(p1, q1) and np.array_equal(p2, q2) and all(np.array_equal(g[k], h[k]) for k in GRADS)


@pytest.mark.parametrize("dL", [("dL0", None, None), (None, "dL1", None), (None, None, "dL2")], ids=["psi0", "psi1", "psi2"])
def test_each_dL_input_alone(dL):
    c = P.make_case(65, 17, 3, True, True)
    _, _, g = _dev(c, True, dL)
    _, _, rg = _ref(c, dL)
    for k in GRADS:
        ref = np.asarray(rg[k], dtype=LD)
        if not np.any(ref):
            assert not np.any(g[k]), k                                # psi0 alone: only the variance moves
        else:
            assert _rel(g[k], ref) <= 10 * F64_DISTANCE[k], (k, _rel(g[k], ref))


def test_a_non_symmetric_dL_dpsi2_equals_its_symmetrisation_byte_for_byte():
    c = P.make_case(63, 17, 2, False, True)
    _, _, a = _dev(c, False, ("dL0", "dL1", "dL2_raw"))
    c["sym"] = 0.5 * (c["dL2_raw"] + c["dL2_raw"].T)
    _, _, b = _dev(c, False, ("dL0", "dL1", "sym"))
    assert all(np.array_equal(a[k], b[k]) for k in GRADS)
    assert not np.array_equal(c["dL2_raw"], c["sym"])


def test_the_far_inducing_point_gives_exact_zeros_and_everything_finite():
    import gpy_amd
    g = np.load(os.path.join(HERE, "golden", "psi_ss", "far.npz"))
    far = int(g["M"]) // 2
    k = gpy_amd.RBF(2, variance=float(g["variance"]), lengthscale=g["lengthscale"], ARD=True)
    q = gpy_amd.SpikeAndSlabPosterior(g["mu"], g["S"], g["gamma"])
    p1, p2 = k.psi1(g["Z"], q), k.psi2(g["Z"], q)
    assert np.all(p1[:, far] == 0) and np.all(p2[far] == 0) and np.all(p2[:, far] == 0)
    d = (g["dL0"], g["dL1"], g["dL2"])
    dZ = k.gradients_Z_expectations(*d, g["Z"], q)
    gq = k.gradients_qX_expectations(*d, g["Z"], q)
    k.update_gradients_expectations(*d, g["Z"], q)
    assert np.all(dZ[far] == 0)
    for x in (p1, p2, dZ, k.variance.gradient, k.lengthscale.gradient) + tuple(gq):
        assert np.all(np.isfinite(x))
    assert _rel(dZ, g["dZ"]) <= TOL_FIT and _rel(gq[2], g["dgamma"]) <= TOL_FIT


@pytest.mark.parametrize("name", ["ard", "iso", "subset"])
def test_kernel_methods_match_the_reference_and_unseen_dimensions_are_exactly_zero(name):
    import gpy_amd
    g = np.load(os.path.join(HERE, "golden", "psi_ss", name + ".npz"))
    dims, D = [int(x) for x in g["dims"]], int(g["D"])
    k = gpy_amd.RBF(len(dims), variance=float(g["variance"]), lengthscale=g["lengthscale"], ARD=bool(g["ARD"]),
                    active_dims=None if len(dims) == D else dims)
    q = gpy_amd.SpikeAndSlabPosterior(g["mu"], g["S"], g["gamma"])
    assert _rel(k.psi1(g["Z"], q), g["psi1"]) <= 1e-12 and _rel(k.psi2(g["Z"], q), g["psi2"]) <= 1e-12
    d = (g["dL0"], g["dL1"], g["dL2"])
    dZ = k.gradients_Z_expectations(*d, g["Z"], q)
    dmu, dS, dg = k.gradients_qX_expectations(*d, g["Z"], q)
    k.update_gradients_expectations(*d, g["Z"], q)
    off = [x for x in range(D) if x not in dims]
    for got, key in ((dZ, "dZ"), (dmu, "dmu"), (dS, "dS"), (dg, "dgamma")):
        assert _rel(got[:, dims], g[key]) <= 1e-12, key
        assert not np.any(got[:, off]), key
    assert _rel(k.variance.gradient, g["dvar"]) <= 1e-12 and _rel(k.lengthscale.gradient, g["dl"]) <= 1e-12


def test_refusals_of_the_stateless_calls_name_what_they_refuse():
    from gpy_amd import _lib
    c = P.make_case(5, 3, 2, True, False)
    a = [c["variance"], c["lengthscale"], True, c["Z"], c["mu"], c["S"], c["gamma"]]
    r = np.random.default_rng(0)
    with pytest.raises(_lib.MI355GPError, match="65 input dimensions.*at most 64"):
        _lib.ssrbf_psi(1.0, np.ones(65), True, r.uniform(size=(3, 65)), r.uniform(size=(4, 65)), np.ones((4, 65)), np.full((4, 65), 0.5))
    for bad in (0.0, 1.0, np.nan, -0.1):
        gam = c["gamma"].copy()
        gam[3, 1] = bad
        with pytest.raises(_lib.MI355GPError, match=r"gamma\[3\]\[1\]"):
            _lib.ssrbf_psi(*(a[:6] + [gam]))
        with pytest.raises(_lib.MI355GPError, match=r"gamma\[3\]\[1\]"):
            _lib.ssrbf_psi_grad(*(a[:6] + [gam]), dL_dpsi0=c["dL0"])


# ---- the fit ------------------------------------------------------------------------------------------------------------------
def _fit(c, ctx=None):
    from gpy_amd import _lib
    ctx = ctx or _lib.SparseContext(0)
    ctx.set_data(c["mu"], c["Y"])
    ctx.set_input_variance(c["S"])
    ctx.set_binary_prob(c["gamma"])
    rc, r = ctx.vardtc_ss(P.specs_of(c["k"]), c["Z"], c["noise"])
    assert rc == 0
    return ctx, r


def _judge(r, c, block_dtype=None):
    ev = lambda dt, **kw: P.evaluate(c["k"], c["Z"], c["mu"], c["S"], c["gamma"], c["Y"], c["noise"], dt, **kw)
    ref, r64 = ev(LD, block_dtype=block_dtype), ev(np.float64)
    assert ref["kappa"] <= 1e4
    bad = []
    for q in FIT_JUDGED:
        e, b = SL.rel_err(r[q], np.asarray(ref[q], dtype=LD)), SL.bound(q, ref, r64, ref["kappa"])
        print("  %-16s err %.2e  bound %.2e" % (q, e, b))
        if not e <= b:
            bad.append("%s: %.3e > %.3e" % (q, e, b))
    return ref, bad


@pytest.mark.parametrize("path", FIT_FIXTURES, ids=FIT_IDS)
def test_fit_against_the_references_composed_fit(path):
    """through the C-ABI, `VarDTC.inference` and `SSGPLVM`, prediction included, at the sparse path's tolerances"""
    import gpy_amd
    g = np.load(path)
    c = P.fixture_problem(g)
    k, dims, D = c["k"], c["k"]["dims"], c["k"]["D"]
    # the C-ABI (the context takes the kernel's columns; a part's active_dims then index them)
    ctx, r = _fit(c)
    Wi = ctx.fetch(ctx.FETCH_WOODBURY_INV)
    pm, pv = ctx.predict(P.specs_of(k), g["Xs"])
    um, uv = ctx.predict_uncertain(P.specs_of(k), g["Xs"], g["Ss"])
    check_fit_against_fixture(dict(r, woodbury_inv=Wi), g, dict(pred_mu=pm, pred_var=pv, upred_mu=um, upred_var=uv))
    # VarDTC.inference
    rbf = gpy_amd.RBF(len(dims), variance=k["var"], lengthscale=k["ls"], ARD=k["ARD"], active_dims=None if len(dims) == D else dims)
    kern = rbf if not k["white"] else gpy_amd.Add([rbf] + [gpy_amd.White(D, variance=w) for w in k["white"]])
    q = gpy_amd.SpikeAndSlabPosterior(g["mu"], g["S"], g["gamma"])
    post, lml, gd = gpy_amd.VarDTC().inference(kern, q, g["Z"], gpy_amd.Gaussian(c["noise"]), g["Y"])
    f = gd["fused"]
    wide = lambda x: x if x.shape[1] == D else P.widen(x, g)
    check_fit_against_fixture(dict(lml=lml, woodbury_vector=post.woodbury_vector, woodbury_inv=np.asarray(post.woodbury_inv),
                                   dtheta=f["dtheta"], dnoise=gd["dL_dthetaL"], dZ=wide(f["dZ"]), dmu=wide(f["dmu"]), dS=wide(f["dS"]),
                                   dgamma=wide(f["dgamma"])), g)
    # SSGPLVM
    m = gpy_amd.SSGPLVM(g["Y"], D, X=g["mu"], X_variance=g["S"], Gamma=g["gamma"], Z=g["Z"], kernel=kern,
                        likelihood=gpy_amd.Gaussian(c["noise"]), pi=c["pi"])
    N, M = g["mu"].shape[0], g["Z"].shape[0]
    grad, o = m.gradient, 3 * N * D
    pm, pv = m.predict_noiseless(g["Xs"])
    um, uv = m.predict_noiseless(gpy_amd.NormalPosterior(g["Xs"], g["Ss"]))
    check_fit_against_fixture(dict(bound=m.log_likelihood(), Xmean_grad=m.X.mean.gradient, Xvar_grad=m.X.variance.gradient,
                                   Xgamma_grad=m.X.binary_prob.gradient, dZ=grad[o:o + M * D].reshape(M, D), dtheta=grad[o + M * D:-1],
                                   dnoise=grad[-1:]), g, dict(pred_mu=pm, pred_var=pv, upred_mu=um, upred_var=uv))


@pytest.mark.parametrize("case", P.FIT_CASES, ids=[c[0] for c in P.FIT_CASES])
def test_fit_against_long_double(case):
    name, N, M, Q, Dy, ARD, dims = case
    c = P.lattice_problem(N, M, Q, Dy, 7, ARD=ARD, dims=dims)
    ctx, r = _fit(c)
    ref, bad = _judge(r, c)
    assert not bad, bad
    if dims is not None:
        off = [q for q in range(Q) if q not in dims]
        assert all(not np.any(r[q][:, off]) for q in ("dZ", "dmu", "dS", "dgamma"))
    # two fresh contexts, equal bytes; set_inputs_ss against a fresh set_data likewise
    from gpy_amd import _lib
    ctx2 = _lib.SparseContext(0)
    ctx2.set_data(c["mu"] + 1.0, c["Y"])
    ctx2.set_input_variance(2.0 * c["S"])
    ctx2.set_inputs_ss(c["mu"], c["S"], c["gamma"])
    rc, r2 = ctx2.vardtc_ss(P.specs_of(c["k"]), c["Z"], c["noise"])
    assert all(np.array_equal(r[q], r2[q]) for q in FIT_JUDGED)


def test_fit_across_the_row_chunk_edge_at_n_262145():
    c = P.lattice_problem(262145, 8, 2, 1, 11)
    ctx, r = _fit(c)
    ref, bad = _judge(r, c, block_dtype=np.float64)                   # row blocks in fp64, their sums and everything M x M in long double
    assert not bad, bad


def test_gaussian_entry_refuses_gamma_and_is_unchanged_by_setting_and_clearing_it():
    from gpy_amd import _lib
    c = P.lattice_problem(63, 17, 2, 3, 7)
    specs = P.specs_of(c["k"])
    ctx = _lib.SparseContext(0)
    ctx.set_data(c["mu"], c["Y"])
    ctx.set_input_variance(c["S"])
    with pytest.raises(_lib.MI355GPError, match="no slab probabilities"):
        ctx.vardtc_ss(specs, c["Z"], c["noise"])
    rc, before = ctx.vardtc_uncertain(specs, c["Z"], c["noise"])
    ctx.set_binary_prob(c["gamma"])
    with pytest.raises(_lib.MI355GPError, match="holds slab probabilities"):
        ctx.vardtc_uncertain(specs, c["Z"], c["noise"])
    rc, ss = ctx.vardtc_ss(specs, c["Z"], c["noise"])
    ctx.set_binary_prob(None)
    rc, after = ctx.vardtc_uncertain(specs, c["Z"], c["noise"])
    for q in ("lml", "dtheta", "dnoise", "dZ", "dmu", "dS", "woodbury_vector"):
        assert np.array_equal(before[q], after[q]), q
    assert ss["lml"] != before["lml"]
    ctx.set_binary_prob(c["gamma"])
    ctx.set_data(c["mu"], c["Y"])                                     # set_data forgets gamma (and the variances)
    ctx.set_input_variance(c["S"])
    with pytest.raises(_lib.MI355GPError, match="no slab probabilities"):
        ctx.vardtc_ss(specs, c["Z"], c["noise"])


def test_refusals_through_the_c_abi():
    from gpy_amd import _lib
    c = P.lattice_problem(33, 9, 2, 2, 7)
    ctx, r = _fit(c)
    rbf, white = P.specs_of(c["k"])
    Z, noise = c["Z"], c["noise"]
    for bad, pat in (([rbf, ("bias", False, np.array([0.5]), None, 0)], "Bias"), ([("linear", False, np.array([1.0]), None, 0)], "Linear"),
                     ([("matern52", False, np.array([1.0, 1.0]), None, 0), white], "Matern52"), ([rbf, rbf], "both RBF"),
                     ([rbf[:4] + (1,), ("bias", False, np.array([0.5]), None, 1)], "product"), ([white], "no RBF part")):
        with pytest.raises(_lib.MI355GPError, match=pat):
            ctx.vardtc_ss(bad, Z, noise)
    with pytest.raises(_lib.MI355GPError, match="per-point noise"):
        ctx.vardtc_ss([rbf, white], Z, np.full(33, 0.1))
    gam = c["gamma"].copy()
    gam[4, 1] = 1.0
    with pytest.raises(_lib.MI355GPError, match=r"gamma\[4\]\[1\]"):
        ctx.set_binary_prob(gam)
    with pytest.raises(_lib.MI355GPError, match=r"gamma\[4\]\[1\]"):
        ctx.set_inputs_ss(c["mu"], c["S"], gam)
    fresh = _lib.SparseContext(0)
    fresh.set_data(c["mu"], c["Y"])
    with pytest.raises(_lib.MI355GPError, match="no input variances"):
        fresh.set_binary_prob(c["gamma"])
    sh = _lib.SparseContext(0)                                        # a row-sharded context: all three entries refuse it
    sh.attach_loopback(0, 1, 7801)
    sh.set_data(c["mu"], c["Y"])
    for call in (lambda: sh.set_binary_prob(c["gamma"]), lambda: sh.set_inputs_ss(c["mu"], c["S"], c["gamma"]),
                 lambda: sh.vardtc_ss([rbf, white], Z, noise)):
        with pytest.raises(_lib.MI355GPError, match="row-sharded"):
            call()
    sh.close()
    wide = _lib.SparseContext(0)
    r65 = np.random.default_rng(0)
    wide.set_data(r65.uniform(size=(4, 65)), c["Y"][:4])
    wide.set_input_variance(np.ones((4, 65)))
    wide.set_binary_prob(np.full((4, 65), 0.5))
    with pytest.raises(_lib.MI355GPError, match="at most 64 input dimensions"):
        wide.vardtc_ss([("rbf", False, np.array([1.0, 1.0]), None, 0)], r65.uniform(size=(3, 65)), 0.1)
    rc, again = ctx.vardtc_ss([rbf, white], Z, noise)                 # the context is still good, with the same bytes
    assert all(np.array_equal(r[q], again[q]) for q in FIT_JUDGED)


# ---- VarDTC.inference and SSGPLVM ----------------------------------------------------------------------------------------------
def _model(c, **kw):
    import gpy_amd
    k = c["k"]
    Q = k["D"]
    rbf = gpy_amd.RBF(len(k["dims"]), variance=k["var"], lengthscale=k["ls"], ARD=k["ARD"],
                      active_dims=None if len(k["dims"]) == Q else k["dims"])
    kern = rbf + gpy_amd.White(Q, variance=k["white"][0])
    return gpy_amd.SSGPLVM(c["Y"], Q, X=c["mu"], X_variance=c["S"], Gamma=c["gamma"], Z=c["Z"], kernel=kern,
                           likelihood=gpy_amd.Gaussian(c["noise"]), **kw)


def _model_against_restatement(m, kappa_cap=None):
    k = dict(var=float(m.kern.parts[0].variance.values[0]), ls=m.kern.parts[0].lengthscale.values.copy(), D=m.input_dim,
             dims=list(range(m.input_dim)), ARD=True, white=[float(m.kern.parts[1].variance.values[0])])
    c = dict(k=k, Z=m.Z.values.copy(), mu=m.X.mean.values.copy(), S=m.X.variance.values.copy(), gamma=m.X.binary_prob.values.copy(),
             Y=np.asarray(m.Y), noise=float(m.likelihood.variance.values[0]))
    ev = lambda dt: P.evaluate(c["k"], c["Z"], c["mu"], c["S"], c["gamma"], c["Y"], c["noise"], dt)
    ref, r64 = ev(LD), ev(np.float64)
    N, Q, M = m.num_data, m.input_dim, m.num_inducing
    g = m.gradient
    o = 3 * N * Q
    got = dict(bound=m.log_likelihood(), dmu=m.X.mean.gradient, dS=m.X.variance.gradient, dgamma=m.X.binary_prob.gradient,
               dZ=g[o:o + M * Q].reshape(M, Q), dtheta=g[o + M * Q:-1], dnoise=g[-1])
    for d in (ref, r64):
        d.update(dmu=d["dmu"] - d["kl_dmu"], dS=d["dS"] - d["kl_dS"], dgamma=d["dgamma"] - d["kl_dgamma"])
    print("kappa %.3e" % ref["kappa"])
    bad = []
    for q in got:
        e, b = SL.rel_err(got[q], np.asarray(ref[q], dtype=LD)), SL.bound(q, ref, r64, ref["kappa"])
        print("  %-8s err %.2e  bound %.2e" % (q, e, b))
        if not e <= b:
            bad.append("%s: %.3e > %.3e" % (q, e, b))
    return c, ref, bad


def test_ssgplvm_checkgrad_optimisation_and_prediction():
    import gpy_amd
    c = P.lattice_problem(40, 9, 3, 4, 5)
    c["gamma"] = np.clip(c["gamma"], 0.05, 0.95)                      # checkgrad steps the flat parameters, gamma included
    m = _model(c)
    np.random.seed(0)
    assert m.checkgrad()
    _, _, bad = _model_against_restatement(m)
    assert not bad, bad
    f0 = m.objective_function()
    m.optimize(max_iters=30)
    assert m.objective_function() < f0
    g = m.X.binary_prob.values
    assert np.all((g > 0) & (g < 1))
    cm, ref, bad = _model_against_restatement(m)                      # kappa at the optimum is printed, not judged
    assert not bad, bad
    # prediction at certain points and at NormalPosterior points, against the restatement's posterior
    import psi_lin_ld as PL
    kl = dict(P="rbf", D=3, dims=[0, 1, 2], ARD=True, var=cm["k"]["var"], ls=cm["k"]["ls"], white=cm["k"]["white"])
    r = np.random.default_rng(2)
    Xs, Ss = r.uniform(-0.5, 2.5, (23, 3)), r.uniform(0.05, 0.3, (23, 3))
    mu, var = m.predict_noiseless(Xs)
    rmu, rvar = PL.predict_certain(kl, cm["Z"], ref, Xs, LD)
    assert _rel(mu, rmu) <= TOL_FIT and _rel(var, rvar) <= TOL_VAR
    mu, var = m.predict_noiseless(gpy_amd.NormalPosterior(Xs, Ss))
    rmu, rvar = PL.predict(kl, cm["Z"], ref, Xs, Ss, LD)
    assert _rel(mu, rmu) <= TOL_FIT and _rel(var, rvar) <= TOL_VAR
    with pytest.raises(NotImplementedError, match="spike-and-slab new points"):
        m.predict(gpy_amd.SpikeAndSlabPosterior(Xs, Ss, np.full(Xs.shape, 0.5)))


def test_vardtc_inference_with_a_subset_kernel_scatters_exact_zeros():
    import gpy_amd
    c = P.lattice_problem(40, 16, 5, 4, 7, dims=[0, 2, 3])
    m = _model(c)
    ref = P.evaluate(c["k"], c["Z"], c["mu"], c["S"], c["gamma"], c["Y"], c["noise"], LD)
    assert abs(m.log_likelihood() - float(ref["bound"])) <= TOL_LML * abs(float(ref["bound"]))
    assert _rel(m.X.binary_prob.gradient, ref["dgamma"] - ref["kl_dgamma"]) <= TOL_FIT
    assert _rel(m.Z.gradient, ref["dZ"]) <= TOL_FIT and not np.any(m.Z.gradient[:, [1, 4]])
    fused = m.grad_dict["fused"]
    assert sorted(fused) == ["dS", "dZ", "dgamma", "dmu", "dtheta"]
