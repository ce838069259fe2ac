"""GPU (-m gpu): EPDTC on the device -- mi355gp_epdtc_begin / _recompute / _sweep / _inference (gpy_amd/csrc/epdtc.hip), the
classes `EPDTC` and `SparseGPClassification` over them.

One recompute and one sweep against the long-double restatement tests/epdtc_np.py, given the same sites, order, eta = 0.9,
delta = 0.8 and the first-site flag, at the shapes epdtc_np.SHAPES: N in {1, 63, 64, 65, 129} (the 64-site block: below it, at
it, one and two blocks and a site) with M and D small; M in {1, 63, 65, 129, 257} (the 128 tile and its padding) and D in
{1, 17, 33} (the dimension groups) once each with the others small.  The other boundary of the implementation is the row
chunk (at most 262144 rows; larger N is cut into equal chunks): N = 262144 and 262145 at M = 1, where recompute is held to long
double directly and the sweep's cavity parameters of every site to the long-double recurrence that M = 1 allows
(1 / P = Kmm + sum_n tau_n k_n^2 and Kmn v as running sums over the device's own site updates): they are right only if P and
gamma were carried correctly through every block and across the chunk edge.

Bounds: epdtc_np.DEVICE_BOUND, ten times the float64 restatement's own distance from long double over the same cases
(tests/test_oracle_epdtc.py has the measurement), relative to max |value|: tau 5.7e-11, v 9.5e-14, cav_tau 3.2e-14, cav_v 1.4e-13,
log Z_hat 3.5e-14, mu_hat 5.2e-14, sigma2_hat 4.8e-14, mu 7.2e-15, Sigma_diag 1.5e-14.  tau stands apart because
1 / sigma2_hat - 1 / Sigma_ii cancels where a site is nearly uninformative.
Device figures (one MI355X, worst over the shape cases): see DEVICE_FIGURES below.

Every fixture of tests/golden/epdtc (the reference's own EPDTC with recorded orders) through `EPDTC.inference` and through
`SparseGPClassification`: the sites at the bound above, everything downstream at the sparse path's tolerances
(tests/test_gpu_sparse.py): log marginal 1e-9, gradients, Woodbury vector and predictive mean 1e-6, predictive variance 1e-5.
Two sweeps and two whole inference calls give the same bytes.  `optimize()` on the toy problem reaches the fixture's optimum to
1e-3 of the bound (the tolerance tests/test_gpu_ep.py holds its toy problem's bound to).  Prediction, `sparse_fetch` and the
lazy views of `grad_dict` work after an EPDTC call.
"""
import os

import numpy as np
import pytest

import epdtc_np as E
import gpy_amd
import kern_ld as KL
import svgp_np as S
from gpy_amd import _lib as L
from gpy_amd.epdtc import EPDTC

pytestmark = pytest.mark.gpu
LD = np.longdouble
# measured on one MI355X, worst over epdtc_np.SHAPES and the second sweep of each (a record, never a bound).  The two chunk-edge
# cases: cav_tau 3.8e-15, cav_v 5.2e-15, mu 3.9e-16, Sigma_diag 4.9e-16.  The eight fixtures: sites 3.7e-14 (tau of the product
# kernel), cavity parameters 1.4e-14, log marginal 1.1e-15, gradients 4.0e-14, Woodbury vector 5.0e-15, prediction 8.7e-15; the toy
# optimisation ends at a bound of -37.733244 against the reference's -37.733243.  The whole file: 27 cases in about 5 s.
DEVICE_FIGURES = {"tau": 5.6e-12, "v": 8.6e-15, "cav_tau": 5.1e-15, "cav_v": 1.4e-14, "log_Z_hat": 4.0e-15, "mu_hat": 1.4e-15,
                  "sigma2_hat": 7.1e-15, "mu": 1.1e-15, "Sigma_diag": 1.7e-15}
DOWNSTREAM = E.DOWNSTREAM


@pytest.fixture(scope="module")
def ctx():
    c = L.SparseContext(0)
    yield c
    c.close()


def _begin(ctx, c):
    dev = KL.cabi_specs(c["specs"])
    ctx.set_data(c["X"], c["sign"][:, None])
    info, _ = ctx.epdtc_begin(dev, c["Z"], 0.0)
    assert info == 0
    return dev


def _held(got, ref, keys):
    fig = {k: E.rel(got[k], ref[k]) for k in keys}
    print({k: "%.1e (bound %.1e)" % (fig[k], E.DEVICE_BOUND[k]) for k in keys})
    for k in keys:
        assert fig[k] <= E.DEVICE_BOUND[k], (k, fig[k], E.DEVICE_BOUND[k])


@pytest.mark.parametrize("name", [s[0] for s in E.SHAPES])
def test_recompute_and_sweep_match_the_long_double_restatement(ctx, name):
    KL.require_ld()
    c, ref = E.reference(name)
    _begin(ctx, c)
    info, mu, sd = ctx.epdtc_recompute(c["tau"], c["v"])
    assert info == 0
    _held(dict(mu=mu, Sigma_diag=sd), ref, ("mu", "Sigma_diag"))
    r = ctx.epdtc_sweep(c["order"], c["sign"], c["tau"], c["v"], c["eta"], c["delta"], first=True)
    _held(r, ref, E.SWEEP_KEYS)
    # the same sweep again from the same recompute: the same bytes
    info, mu2, sd2 = ctx.epdtc_recompute(c["tau"], c["v"])
    r2 = ctx.epdtc_sweep(c["order"], c["sign"], c["tau"], c["v"], c["eta"], c["delta"], first=True)
    assert mu.tobytes() == mu2.tobytes() and sd.tobytes() == sd2.tobytes()
    assert all(r[k].tobytes() == r2[k].tobytes() for k in E.SWEEP_KEYS)
    # a sweep without a recompute continues from the first one's P and gamma: its result differs, and without the first-site flag
    # the first site does not see the 1e-8
    r3 = ctx.epdtc_sweep(c["order"], c["sign"], r["tau"], r["v"], c["eta"], c["delta"], first=False)
    Kmm, Kmn = E.covariances(c["specs"], c["X"], c["Z"], LD)
    ref3 = E.ref_sweep(Kmm, Kmn, c["order"], c["sign"], c["eta"], c["delta"], ref["tau"], ref["v"], False, LD)
    _held(r3, ref3, E.SWEEP_KEYS)


@pytest.mark.parametrize("N", [262144, 262145])
def test_row_chunk_edge(ctx, N):
    """the row chunk (at most 262144 rows): one chunk, and two equal chunks"""
    KL.require_ld()
    rng = np.random.default_rng(N)
    X = rng.uniform(0, 1, (N, 1))
    Z = np.array([[0.5]])
    specs = [("rbf", 0, np.array([1.2, 0.8]), np.arange(1), 0)]
    sign = np.where(np.sin(7 * X[:, 0]) + 0.3 * rng.standard_normal(N) > 0, 1.0, -1.0)
    tau, v = rng.uniform(1e-6, 2e-6, N), sign * rng.uniform(1e-6, 2e-6, N)        # (sum_n tau_n k_n^2 of order Kmm)
    order = rng.permutation(N)
    c = dict(specs=specs, X=X, Z=Z, sign=sign)
    _begin(ctx, c)
    info, mu, sd = ctx.epdtc_recompute(tau, v)
    assert info == 0
    k = np.asarray(KL.K(specs, Z, X, LD), dtype=LD)[0]
    kmm = LD(1.2)
    llt0, s0 = kmm + np.sum(LD(1) * tau * k * k), np.sum(LD(1) * v * k)
    _held(dict(mu=mu, Sigma_diag=sd), dict(mu=k * s0 / llt0, Sigma_diag=k * k / llt0), ("mu", "Sigma_diag"))
    eta, delta = 0.9, 0.8
    r = ctx.epdtc_sweep(order, sign, tau, v, eta, delta, first=True)
    assert all(np.isfinite(r[q]).all() for q in E.SWEEP_KEYS) and r["tau"].min() >= np.finfo(float).eps
    # M = 1: what site p sees follows from the updates of the sites before it, as running sums in long double
    ko = k[order]
    dtau, dv = (LD(1) * r["tau"] - tau)[order], (LD(1) * r["v"] - v)[order]
    llt = llt0 + np.concatenate([[LD(0)], np.cumsum(dtau * ko * ko)[:-1]])
    s = s0 + np.concatenate([[LD(0)], np.cumsum(dv * ko)[:-1]])
    S, m = ko * ko / llt, ko * s / llt
    S[0] += LD(1e-8)
    ref = dict(cav_tau=np.empty(N, dtype=LD), cav_v=np.empty(N, dtype=LD))
    ref["cav_tau"][order] = 1 / S - LD(eta) * tau[order]
    ref["cav_v"][order] = m / S - LD(eta) * v[order]
    _held(r, ref, ("cav_tau", "cav_v"))


def _fixture_results(fx, inf, kern, post, lml, gd):
    _, ga, lzt = inf._ep_approximation
    mu, var = post._raw_predict(kern, fx["Xs"], fx["Z"])
    return dict(lml=lml, log_Z_tilde=lzt, tau=ga.tau, v=ga.v, cav_tau=inf._cav_params.tau, cav_v=inf._cav_params.v,
                dtheta=gd["fused"]["dtheta"], dZ=gd["fused"]["dZ"], woodbury_vector=post.woodbury_vector, pred_mu=mu, pred_var=var)


def _judge_fixture(got, fx):
    ref = dict(fx, tau=fx["tau_tilde"], v=fx["v_tilde"])
    fig = {q: (abs(got[q] - ref[q]) / abs(ref[q]) if q in ("lml", "log_Z_tilde") else E.rel(got[q], ref[q])) for q in got}
    print(fx["name"], {q: "%.1e" % e for q, e in fig.items()})
    for q, e in fig.items():
        assert e <= (E.DEVICE_BOUND[q] if q in E.DEVICE_BOUND else DOWNSTREAM[q]), (q, e)


def _replay(monkeypatch, orders):
    it = iter([np.asarray(o) for o in orders])
    monkeypatch.setattr(np.random, "permutation", lambda n: next(it))


@pytest.mark.parametrize("name", E.FIXTURES)
def test_fixture_through_the_inference_class(monkeypatch, name):
    fx = E.load(name)
    inf = EPDTC(eta=fx["eta"], delta=fx["delta"], parallel_updates=fx["parallel_updates"], max_iters=100)
    if "warm_specs" in fx:
        _replay(monkeypatch, list(fx["warm_orders"]) + list(fx["orders"]))
        inf.inference(S.make_kernel(dict(fx, specs=fx["warm_specs"])), fx["X"], fx["Z"], gpy_amd.Bernoulli(), fx["Y"])
        inf.on_optimization_start()
    else:
        _replay(monkeypatch, fx["orders"])
    kern = S.make_kernel(fx)
    post, lml, gd = inf.inference(kern, fx["X"], fx["Z"], gpy_amd.Bernoulli(), fx["Y"])
    assert inf.iterations == fx["sweeps"]
    _judge_fixture(_fixture_results(fx, inf, kern, post, lml, gd), fx)
    # the lazy views and the fetches after an EPDTC call
    C = L.SparseContext
    M, N = fx["Z"].shape[0], fx["X"].shape[0]
    assert E.rel(np.asarray(gd["dL_dKmm"]), fx["dL_dKmm"]) <= 1e-4 and E.rel(np.asarray(post.woodbury_inv), fx["woodbury_inv"]) <= 1e-4
    Kmm = inf._ctx.fetch(C.FETCH_KMM)
    assert E.rel(Kmm, np.asarray(KL.K(fx["specs"], fx["Z"], None, np.float64), dtype=np.float64)) <= 1e-13      # no jitter on it
    Lm = np.asarray(post.K_chol)
    assert E.rel(Lm @ Lm.T, Kmm) <= 1e-12
    G = np.asarray(gd["dL_dKnm"])
    ref = E.final(fx["specs"], fx["X"], fx["Z"], fx["tau_tilde"], fx["v_tilde"], 0.0, np.float64)["dL_dKnm"]
    assert G.shape == (N, M) and E.rel(G, ref) <= 1e-6
    assert E.rel(inf._ctx.fetch_dL_dKnm(3, 40), ref[3:43]) <= 1e-6
    _, cov = post._raw_predict(kern, fx["Xs"], fx["Z"], full_cov=True)
    assert cov.shape == (13, 13) and E.rel(np.diag(cov)[:, None], fx["pred_var"]) <= DOWNSTREAM["pred_var"]


@pytest.mark.parametrize("name", ["rbf_white_n130_m16_d2", "parallel_rbf_iso_n150_m16_d2"])
def test_fixture_through_the_model(monkeypatch, name):
    fx = E.load(name)
    _replay(monkeypatch, fx["orders"])
    inf = EPDTC(parallel_updates=fx["parallel_updates"], max_iters=100)
    m = gpy_amd.SparseGPClassification(fx["X"], fx["Y"], kernel=S.make_kernel(fx), Z=fx["Z"], inference_method=inf)
    got = _fixture_results(fx, inf, m.kern, m.posterior, m.log_likelihood(), m.grad_dict)
    _judge_fixture(got, fx)
    assert E.rel(m.gradient, np.concatenate([fx["dZ"].ravel(), fx["dtheta"]])) <= DOWNSTREAM["dtheta"]
    p, _ = m.predict(fx["Xs"])
    assert E.rel(p, fx["pred_p"]) <= DOWNSTREAM["pred_mu"]
    assert m.checkgrad()
    assert m.posterior_samples_f(fx["Xs"], size=2).shape == (13, 1, 2)


def test_two_whole_inference_calls_give_the_same_bytes():
    fx = E.load("matern52_ard_n140_m25_d3")
    out = []
    for _ in range(2):
        np.random.seed(5)
        inf = EPDTC(max_iters=100)
        kern = S.make_kernel(fx)
        post, lml, gd = inf.inference(kern, fx["X"], fx["Z"], gpy_amd.Bernoulli(), fx["Y"])
        mu, var = post._raw_predict(kern, fx["Xs"], fx["Z"])
        _, ga, lzt = inf._ep_approximation
        out.append([np.float64(lml), np.float64(lzt), ga.tau, ga.v, gd["fused"]["dtheta"], gd["fused"]["dZ"], post.woodbury_vector, mu, var,
                    np.asarray(gd["dL_dKmm"]), np.asarray(post.woodbury_inv)])
    for a, b in zip(*out):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()


def test_optimize_reaches_the_fixture_optimum():
    z = np.load(os.path.join(E.GOLDEN, "toy_1d_optimize.npz"))
    np.random.seed(2)
    m = gpy_amd.SparseGPClassification(z["X"], z["Y"], kernel=gpy_amd.RBF(1, variance=z["theta0"][0], lengthscale=z["theta0"][1]),
                                       Z=z["Z0"])
    start = m.log_likelihood()
    assert abs(start - float(z["lml_start"])) <= 1e-3 * abs(float(z["lml_start"]))            # shipped epsilon 1e-6, another order
    m.optimize()
    end = m.log_likelihood()
    print("bound %.6f -> %.6f (reference %.6f -> %.6f), theta %s (reference %s)" % (start, end, float(z["lml_start"]),
                                                                                      float(z["lml_end"]), m.kern.param_array, z["theta_end"]))
    assert abs(end - float(z["lml_end"])) <= 1e-3 * abs(float(z["lml_end"]))
    p, _ = m.predict(z["X"])
    assert float(np.mean((p > 0.5) == (z["Y"] == 1))) > 0.8


def test_error_paths_return_a_message(ctx):
    c, _ = E.reference("n65")
    dev = KL.cabi_specs(c["specs"])
    ctx.set_data(c["X"], np.hstack([c["sign"][:, None]] * 2))
    with pytest.raises(L.MI355GPError, match="2 output columns"):
        ctx.epdtc_begin(dev, c["Z"], 0.0)
    ctx.set_data(c["X"], c["sign"][:, None])
    with pytest.raises(L.MI355GPError, match="mi355gp_epdtc_begin first"):
        ctx.epdtc_recompute(c["tau"], c["v"])
    assert ctx.epdtc_begin(dev, c["Z"], 0.0)[0] == 0
    with pytest.raises(L.MI355GPError, match="mi355gp_epdtc_recompute first"):
        ctx.epdtc_sweep(c["order"], c["sign"], c["tau"], c["v"])
    assert ctx.epdtc_recompute(c["tau"], c["v"])[0] == 0
    bad = c["order"].copy()
    bad[0] = bad[1]
    with pytest.raises(L.MI355GPError, match="not a permutation"):
        ctx.epdtc_sweep(bad, c["sign"], c["tau"], c["v"])
    with pytest.raises(L.MI355GPError, match="tau\\[0\\]"):
        ctx.epdtc_recompute(np.where(np.arange(c["N"]) == 0, -1.0, c["tau"]), c["v"])
    with pytest.raises(L.MI355GPError, match="positive"):
        ctx.epdtc_inference(dev, c["Z"], np.zeros(c["N"]), c["v"], 0.0)
    # Kmm that is not positive definite comes back as info, for the caller's jitter ladder: three equal inducing points under
    # a unit variance make every entry of Kmm exactly one, so the second pivot is exactly zero
    unit = KL.cabi_specs([("rbf", 0, np.array([1.0, 0.5]), np.arange(c["D"]), 0)])
    Zdup = np.tile(c["Z"][:1], (3, 1))
    assert ctx.epdtc_begin(unit, Zdup, 0.0)[0] == 2
    assert ctx.epdtc_begin(unit, Zdup, 1e-6)[0] == 0
