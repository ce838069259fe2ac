"""CPU: the condition numbers of the fit cases of tests/test_gpu_psi_gh.py are held under the sparse path's cap, and everything
`VarDTC(psi_gh=...)` refuses before any device work names what it refuses."""
import numpy as np
import pytest

import gh_ld as G
import kern_ld as KL

@pytest.mark.parametrize("case", G.FIT_CASES, ids=G.ident)
def test_fit_cases_are_well_conditioned(case):
    k = G.make_fit_case(case)
    Kmm = KL.K(k["specs"], k["Z"], None, np.float64) + 1e-8 * np.eye(k["Z"].shape[0])
    assert np.linalg.cond(np.asarray(Kmm, dtype=np.float64)) <= 1e4


def _infer(inf, kern, qX, N=6, M=3, noise=0.1, **kw):
    import gpy_amd as GPy
    rng = np.random.default_rng(0)
    lik = GPy.likelihoods.Gaussian(variance=noise)
    return inf.inference(kern, qX, rng.uniform(0, 1, (M, 2)), lik, rng.standard_normal((N, 1)), **kw)


def test_every_refusal_names_what_it_refuses():
    import gpy_amd as GPy
    rng = np.random.default_rng(1)
    VarDTC, k = GPy.inference.latent_function_inference.VarDTC, GPy.kern
    mu, S = rng.uniform(0, 1, (6, 2)), rng.uniform(0.1, 0.2, (6, 2))
    qX = GPy.NormalPosterior(mu, S)
    m52 = lambda: k.Matern52(2, name="m52")
    with pytest.raises(NotImplementedError, match="'m52' \\(Matern52\\) has no psi-statistics on the MI355X sparse path"):
        _infer(VarDTC(), m52(), qX)                                   # without the opt-in: today's message
    for other, what in ((k.Bias(2, name="b"), "'b' \\(Bias\\)"), (k.Linear(2, name="lin"), "'lin' \\(Linear\\)"),
                        (k.RBF(2, name="r"), "'r' \\(RBF\\)")):
        with pytest.raises(NotImplementedError, match="psi_gh.*%s beside the quadrature part 'm52'" % what):
            _infer(VarDTC(psi_gh=True), k.Add([m52(), other]), qX)
    with pytest.raises(NotImplementedError, match="exactly one input-dependent part is covered, got 2 \\('m52': Matern52, 'e': Exponential\\)"):
        _infer(VarDTC(psi_gh=True), k.Add([m52(), k.Exponential(2, name="e")]), qX)
    with pytest.raises(NotImplementedError, match="SpikeAndSlabPosterior.*'m52' \\(Matern52\\)"):
        _infer(VarDTC(psi_gh=True), m52(), GPy.SpikeAndSlabPosterior(mu, S, np.full((6, 2), 0.5)))
    with pytest.raises(NotImplementedError, match="missing_data.*psi_gh"):
        _infer(VarDTC(psi_gh=True), m52(), qX, missing_data=True)
    with pytest.raises(NotImplementedError, match="per-point\\) noise"):
        _infer(VarDTC(psi_gh=True), m52(), qX, noise=np.full(6, 0.1), precision=np.full(6, 10.0))
    with pytest.raises(NotImplementedError, match="dL_dpsi2 as M x M"):
        m52().gradients_Z_expectations(None, None, np.zeros((6, 3, 3)), np.zeros((3, 2)), qX)
    with pytest.raises(ValueError, match="between 1 and 32"):
        VarDTC(psi_gh=33)
    sharded = VarDTC(psi_gh=True)
    sharded._ctx = type("Ctx", (), {"sharded": True})()
    with pytest.raises(NotImplementedError, match="row-sharded"):
        _infer(sharded, m52(), qX)
