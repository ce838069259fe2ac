"""GPU: the Gauss-Hermite psi-statistics (csrc/psi_gh.hip), the fit that stands on them (`mi355gp_vardtc_inference_gh`,
`VarDTC(psi_gh=True)`) and a Bayesian GPLVM with a Matern52 kernel, against the long-double restatement of tests/gh_ld.py.

Stateless statistics and gradients.  Tolerance per quantity = max(16 x d, 64 eps64), d = the largest relative distance (max-abs
norm) of gh_ld.py run in fp64 from gh_ld.py run in long double over `gh_ld.CASES`, measured on the CPU:
    quantity   psi0      psi1      psi2      dtheta    dZ        dmu       dS
    d          1.2e-16   3.8e-16   2.3e-15   7.1e-16   4.0e-16   8.4e-16   4.6e-16
    tolerance  1.4e-14   1.4e-14   3.7e-14   1.4e-14   1.4e-14   1.4e-14   1.4e-14
Measured on the device, worst over the cases: psi0 5.6e-17, psi1 4.4e-16, psi2 1.3e-15, dtheta 1.5e-15, dZ 4.1e-16, dmu 1.7e-15,
dS 6.1e-16.

The fit is judged by tests/sparse_ld.py's rule, max(32 e64(q), 256 eps64 kappa) per quantity with e64 from gh_ld.fit in fp64, and
held to the sparse path's TOL_LML / TOL_FIT as well (prediction: TOL_FIT for the mean, TOL_VAR for the variance).  Its inputs are built like sparse_ld.make_case (Z on a jittered grid,
lengthscale 0.75 grid spacings); the largest kappa(Kmm + 1e-8 I) over `gh_ld.FIT_CASES` is 10.0 (cap 1e4, asserted on the CPU by
tests/test_psi_gh_host.py)."""
import numpy as np
import pytest

import gh_ld as G
import sparse_ld as SL

pytestmark = pytest.mark.gpu
TOL_LML, TOL_FIT, TOL_VAR = 1e-9, 1e-6, 1e-5       # the sparse path's tolerances (tests/test_gpu_sparse.py)
FIT_JUDGED = ("lml", "dtheta", "dnoise", "dZ", "dmu", "dS", "woodbury_vector")


def _dev(k, dL=("dL0", "dL1", "dL2"), rank=None):
    from gpy_amd import _lib
    a = tuple(k["spec"][:3]) + (k["Z"], k["mu"], k["S"])
    d0, d1, d2 = (None if x is None else k[x] for x in dL)
    return dict(zip(G.QUANTITIES, _lib.gh_psi(*a, degree=k["H"]) + _lib.gh_psi_grad(*a, d0, d1, d2, degree=k["H"], rank=rank)))


def _judge(got, ref, names=G.QUANTITIES):
    figs = dict((q, G.rel(got[q], ref[q])) for q in names)
    print("  ".join("%s %.1e" % kv for kv in figs.items()))
    for q in names:
        assert figs[q] <= G.tolerance(q), (q, figs[q], G.tolerance(q))


@pytest.mark.parametrize("case", G.CASES, ids=G.ident)
def test_stateless_statistics_and_gradients_against_long_double(case):
    k = G.make_case(case)
    got = _dev(k)
    _judge(got, G.all_quantities(k))
    assert np.array_equal(got["psi2"], got["psi2"].T)                 # bitwise symmetric
    again = _dev(k)                                                   # two evaluations, the same bytes
    assert all(np.array_equal(got[q], again[q]) for q in G.QUANTITIES)


@pytest.mark.parametrize("dL", [("dL0", None, None), (None, "dL1", None), (None, None, "dL2")], ids=["psi0", "psi1", "psi2"])
def test_each_dL_input_alone(dL):
    k = G.make_case(G.CASES[2])
    got, ref = _dev(k, dL), G.all_quantities(k, dL=dL)
    for q in ("dtheta", "dZ", "dmu", "dS"):
        if not np.any(ref[q]):
            assert not np.any(got[q]), q                              # psi0 alone: only the variance moves
    _judge(got, ref, [q for q in ("dtheta", "dZ", "dmu", "dS") if np.any(ref[q])])


def test_a_non_symmetric_dL_dpsi2_gives_the_bytes_of_its_symmetrisation_and_the_rank_form_agrees_with_the_matrix():
    k = G.make_case(G.CASES[8])
    k["sym"] = 0.5 * (k["dL2_raw"] + k["dL2_raw"].T)
    a, b = _dev(k, ("dL0", "dL1", "dL2_raw")), _dev(k, ("dL0", "dL1", "sym"))
    assert not np.array_equal(k["dL2_raw"], k["sym"]) and all(np.array_equal(a[q], b[q]) for q in G.QUANTITIES)
    k["outer"] = 0.7 * k["R"].dot(k["v"].T)                           # dL_dpsi1 = beta R v^T as a matrix and in rank form
    m, r = _dev(k, ("dL0", "outer", "dL2")), _dev(k, ("dL0", None, "dL2"), rank=(0.7, k["R"], k["v"]))
    ref = G.grads(k["spec"], k["Z"], k["mu"], k["S"], k["dL0"], k["outer"], k["dL2"], H=k["H"])
    _judge(m, ref, ("dtheta", "dZ", "dmu", "dS"))
    _judge(r, ref, ("dtheta", "dZ", "dmu", "dS"))


def _judge_fit(got, ref, ref64, kappa, cols=None):
    """cols: `got` holds these columns of dZ, dmu and dS only (the active_dims of a kernel object)"""
    for q in FIT_JUDGED:
        r = ref[q][:, cols] if cols is not None and q in ("dZ", "dmu", "dS") else ref[q]
        e, b = SL.rel_err(got[q], r), SL.bound(q, ref, ref64, kappa)
        print("%s %.1e (bound %.1e)" % (q, e, b))
        assert e <= b and e <= (TOL_LML if q == "lml" else TOL_FIT), (q, e, b)
    for col in ([] if cols is not None else ref["zero_cols"]):       # full-width results: exactly 0 outside active_dims
        assert not np.any(got["dZ"][:, col]) and not np.any(got["dmu"][:, col]) and not np.any(got["dS"][:, col])


def _kernel(GPy, specs, D):
    names = {"matern52": "Matern52", "matern32": "Matern32", "exponential": "Exponential"}
    parts = [GPy.kern.White(D, variance=th[0]) if kind == "white" else getattr(GPy.kern, names[kind])(
        len(dims), variance=th[0], lengthscale=th[1:], ARD=bool(ard), active_dims=None if len(dims) == D else [int(d) for d in dims])
        for kind, ard, th, dims, _ in specs]
    return parts[0] if len(parts) == 1 else GPy.kern.Add(parts)


@pytest.mark.parametrize("case", G.FIT_CASES, ids=G.ident)
def test_the_fit_through_the_c_abi_and_through_vardtc_against_long_double(case):
    import gpy_amd as GPy
    from gpy_amd import _lib
    k = G.make_fit_case(case)
    a = (k["specs"], k["Z"], k["mu"], k["S"], k["R"], k["noise"], k["H"])
    ref, ref64 = G.fit(*a), G.fit(*a, dt=np.float64)
    kappa = float(np.linalg.cond(np.asarray(ref["Kmm"], dtype=np.float64)))
    ctx = _lib.SparseContext(0)
    ctx.set_data(k["mu"], k["R"])
    ctx.set_input_variance(k["S"])
    rc, got = ctx.vardtc_gh(k["specs"], k["Z"], k["noise"], degree=k["H"])
    assert rc == 0 and _judge_fit(got, ref, ref64, kappa) is None
    inf = GPy.inference.latent_function_inference.VarDTC(psi_gh=k["H"])
    post, lml, gd = inf.inference(_kernel(GPy, k["specs"], k["mu"].shape[1]), GPy.NormalPosterior(k["mu"], k["S"]), k["Z"],
                                  GPy.likelihoods.Gaussian(variance=k["noise"]), k["R"])
    got2 = dict(gd["fused"], lml=lml, dnoise=float(np.ravel(gd["dL_dthetaL"])[0]), woodbury_vector=post.woodbury_vector)
    _judge_fit(got2, ref, ref64, kappa, cols=[int(d) for d in k["specs"][0][3]])


def test_sparse_gp_regression_with_x_variance_and_a_matern_kernel_bound_and_prediction_against_long_double():
    import gpy_amd as GPy
    k = G.make_fit_case(G.FIT_CASES[1])
    ref = G.fit(k["specs"], k["Z"], k["mu"], k["S"], k["R"], k["noise"], k["H"])
    m = GPy.models.SparseGPRegression(k["mu"], k["R"], kernel=_kernel(GPy, k["specs"], 1), Z=k["Z"], noise_var=k["noise"],
                                      X_variance=k["S"], psi_gh=k["H"])
    assert abs(m.log_likelihood() - float(ref["lml"])) <= TOL_LML * abs(float(ref["lml"]))
    Xs = np.linspace(-0.6, 0.6, 37)[:, None]
    (mu, var), (rmu, rvar) = m.predict(Xs, include_likelihood=False), SL.predict(k["specs"], k["Z"], Xs, ref)
    print("mean %.1e  variance %.1e" % (G.rel(mu, rmu), G.rel(var, rvar)))
    assert G.rel(mu, rmu) <= TOL_FIT and G.rel(var, rvar) <= TOL_VAR


def test_bayesian_gplvm_with_a_matern52_kernel_checkgrad_optimiser_steps_and_prediction():
    import gpy_amd as GPy
    rng = np.random.default_rng(5)
    t = rng.uniform(-1, 1, (40, 2))
    Y = np.hstack([np.sin(2 * t), np.cos(3 * t[:, :1]), t[:, :1] * t[:, 1:]]) + 0.05 * rng.standard_normal((40, 4))
    m = GPy.models.BayesianGPLVM(Y, 3, num_inducing=9, kernel=GPy.kern.Matern52(3, ARD=True),
                                 inference_method=GPy.inference.latent_function_inference.VarDTC(psi_gh=True))
    f0 = m.objective_function()
    assert np.all(np.isfinite(m.gradient)) and np.any(m.X.variance.gradient)
    assert m.checkgrad(verbose=True)
    m.optimize(max_iters=5)
    assert m.objective_function() < f0                                # a few steps increase the bound
    mu, var = m.predict(m.X.mean.values[:5])
    assert mu.shape == (5, 4) and np.all(np.isfinite(mu)) and np.all(var > 0)
    with pytest.raises(NotImplementedError, match="NormalPosterior Xnew"):
        m.predict(GPy.NormalPosterior(m.X.mean.values[:5], m.X.variance.values[:5]))
