"""CPU: the NumPy restatement of Coregionalize / MixedNoise (coreg_np.py) against the fixtures that the reference's own code
produced (tests/golden/coreg, tools/make_golden_coreg.py) and against central differences, plus the host-side logic of the
multi-output path: build_XY / ICM / LCM, the S -> (dW, dkappa) chain rule, MixedNoise bookkeeping, to_dict strings,
active_dims=[-1], the optimiser's parameter transform and the C-ABI header."""
import glob
import os

import numpy as np
import pytest

import gpy_amd
from gpy_amd import models
from gpy_amd.kern import Coregionalize, Prod
from gpy_amd.likelihoods import Gaussian, MixedNoise
from gpy_amd.util import multioutput

import coreg_np as C

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(HERE, "golden", "coreg", "*.npz")))


def _load(name):
    z = np.load(os.path.join(HERE, "golden", "coreg", name + ".npz"))
    g = {k: z[k] for k in z.files}
    g["specs"] = C.load_specs(g["specs"])
    g["nu"] = None if float(g["nu"]) < 0 else float(g["nu"])
    rng = np.random.default_rng(1000 + int(g["gseed"]))
    g["G"] = rng.standard_normal((g["X"].shape[0],) * 2)
    g["G2"] = rng.standard_normal((g["X"].shape[0], g["Xs"].shape[0]))
    return g


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def test_fixtures_present():
    assert len(NAMES) == 6


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference_fixture(name):
    g = _load(name)
    lml, alpha, dL_dK, Ki, dn = C.exact(g["specs"], g["X"], g["Y"], g["noises"], g["nu"])
    assert abs(lml - g["lml"]) <= 1e-10 * abs(g["lml"])
    assert _rel(alpha, g["alpha"]) <= 1e-9
    assert _rel(C.gpy_dtheta(g["specs"], g["X"], dL_dK), g["dtheta"]) <= 1e-8
    if g["nu"] is None:
        assert _rel(dn, g["dnoise"]) <= 1e-8
    assert _rel(C.expr_K(g["specs"], g["X"])[0], g["K_row0"]) <= 1e-13
    mu, var = C.predict(g["specs"], g["X"], alpha, Ki, g["Xs"], nu=g["nu"])
    assert _rel(mu, g["pred_mu"]) <= 1e-9 and _rel(var, g["pred_var"]) <= 1e-9
    _, cov = C.predict(g["specs"], g["X"], alpha, Ki, g["Xs"], full_cov=True, nu=g["nu"])
    assert _rel(cov, g["pred_cov"]) <= 1e-9
    spec = [s for s in g["specs"] if s[0] == "coregionalize"][0]
    W, _, _ = C.coreg_WkB(spec)
    P = spec[1] % 100
    idx, idxs = g["X"][:, -1].astype(int), g["Xs"][:, -1].astype(int)
    dW, dk = C.chain_W_kappa(C.bucket_S(g["G"], idx, idx, P), W)
    assert _rel(np.concatenate([dW.ravel(), dk]), g["ug"]) <= 1e-8
    dW, dk = C.chain_W_kappa(C.bucket_S(g["G2"], idx, idxs, P), W)
    assert _rel(np.concatenate([dW.ravel(), dk]), g["ug2"]) <= 1e-8


def _with_theta(specs, i, th):
    out = list(specs)
    s = out[i]
    out[i] = (s[0], s[1], th, s[3], s[4])
    return out


@pytest.mark.parametrize("name", ["icm_rbfard_p3_noises_n135", "lcm_m52_rbf_p2_r2_n110", "studentt_icm_m52_p3_n120"])
def test_restatement_against_central_differences(name):
    """W, kappa (and B through S), and the per-output noises"""
    g = _load(name)
    specs, h = g["specs"], 1e-6
    f = lambda sp, nz=g["noises"]: C.exact(sp, g["X"], g["Y"], nz, g["nu"])[0]   # noqa: E731
    _, _, dL_dK, _, dn = C.exact(specs, g["X"], g["Y"], g["noises"], g["nu"])
    grads = C.gpy_dtheta(specs, g["X"], dL_dK)
    S_all = C.leaf_grads(specs, g["X"], dL_dK)
    k = 0
    for i, s in enumerate(specs):
        n = s[2].size
        if s[0] == "coregionalize":
            for j in range(n):
                tp, tm = s[2].copy(), s[2].copy()
                tp[j] += h
                tm[j] -= h
                num = (f(_with_theta(specs, i, tp)) - f(_with_theta(specs, i, tm))) / (2 * h)
                assert abs(num - grads[k + j]) <= 1e-5 * max(1.0, abs(num)), (i, j, num, grads[k + j])
            # S against symmetric perturbations of B: B[a][b] and B[b][a] together move L by S[a][b] + S[b][a]
            P = s[1] % 100
            B0 = C.coreg_WkB(s)[2]
            S = S_all[i]
            for a, b in [(0, 0), (P - 1, P - 1), (0, P - 1)]:
                E = np.zeros((P, P))
                E[a, b] = E[b, a] = h
                Bp = [("coregionalize_B", P, (B0 + sgn * E).ravel(), s[3], s[4]) for sgn in (1, -1)]
                num = (f(_with_part(specs, i, Bp[0])) - f(_with_part(specs, i, Bp[1]))) / (2 * h)
                ana = S[a, a] if a == b else S[a, b] + S[b, a]
                assert abs(num - ana) <= 1e-5 * max(1.0, abs(num)), (a, b, num, ana)
        k += n
    if g["nu"] is None:
        for j in range(len(g["noises"])):
            npl, nmi = g["noises"].copy(), g["noises"].copy()
            npl[j] += h
            nmi[j] -= h
            num = (f(specs, npl) - f(specs, nmi)) / (2 * h)
            assert abs(num - dn[j]) <= 1e-5 * max(1.0, abs(num))


def _with_part(specs, i, part):
    out = list(specs)
    out[i] = part
    return out


def test_build_XY_ICM_LCM_shapes_and_names():
    X1, X2 = np.arange(6.0).reshape(3, 2), np.arange(8.0).reshape(4, 2)
    Y1, Y2 = np.ones((3, 1)), 2 * np.ones((4, 1))
    X, Y, I = multioutput.build_XY([X1, X2], [Y1, Y2])
    assert X.shape == (7, 3) and Y.shape == (7, 1) and I.shape == (7, 1)
    assert np.array_equal(X[:, -1], [0, 0, 0, 1, 1, 1, 1]) and np.array_equal(I[:, 0], X[:, -1])
    X, _, I = multioutput.build_XY([X1, X2], index=[3, 5])
    assert np.array_equal(I[:, 0], [3, 3, 3, 5, 5, 5, 5])
    assert multioutput.get_slices([X1, X2]) == [slice(0, 3), slice(3, 7)]
    assert multioutput.index_to_slices(np.array([0, 0, 1, 1, 0, 2, 2, 2, 1, 1])) == [
        [slice(0, 2), slice(4, 5)], [slice(2, 4), slice(8, 10)], [slice(5, 8)]]
    k = multioutput.ICM(2, 3, gpy_amd.RBF(2), W_rank=2)
    assert isinstance(k, Prod) and k.name == "ICM"
    assert [p.name for p in k.parts] == ["rbf", "B"]
    B = k.parts[1]
    assert B.W.shape == (3, 2) and B.kappa.shape == (3,) and list(B.active_dims) == [2]
    lcm = multioutput.LCM(1, 2, [gpy_amd.Matern52(1), gpy_amd.RBF(1)], W_rank=1)
    assert [p.name for p in lcm.parts] == ["ICM0", "ICM1"]
    specs = lcm.part_specs()
    assert [s[0] for s in specs] == ["matern52", "coregionalize", "rbf", "coregionalize"]
    assert [s[4] for s in specs] == [1, 1, 2, 2] and specs[1][1] == 2 and specs[1][2].size == 4
    lik = multioutput.build_likelihood([Y1, Y2], I)
    assert isinstance(lik, MixedNoise) and [l.name for l in lik.likelihoods_list] == ["Gaussian_noise_0", "Gaussian_noise_1"]


def test_coregionalize_parameters_and_chain_rule():
    np.random.seed(1)
    k = Coregionalize(1, 3, rank=2)
    assert k.W.shape == (3, 2) and np.allclose(k.kappa, 0.5)
    assert k.W.positive is False and k.kappa.positive is True
    assert k.parameter_names() == ["W[0]", "W[1]", "W[2]", "W[3]", "W[4]", "W[5]", "kappa[0]", "kappa[1]", "kappa[2]"]
    W = k.W.values.copy()
    B = W @ W.T + np.diag(k.kappa.values)
    assert np.allclose(k.B, B) and np.array_equal(k._theta(), (0.5 * (B + B.T)).ravel())
    k.W[0, 0] = 2.0                                          # an in-place edit reaches the device theta
    assert k._theta()[0] == 4.0 + k.W.values[0, 1] ** 2 + 0.5
    S = np.arange(9.0).reshape(3, 3)
    k._install_gradients(S.ravel())
    assert np.allclose(k.kappa.gradient, [0, 4, 8])
    assert np.allclose(k.W.gradient, (S + S.T) @ k.W.values)
    X = np.array([[0.3, 2.0], [1.0, 0.0], [2.0, 1.0], [5.0, 2.0]])
    kk = Coregionalize(1, 3, W=np.ones((3, 1)), kappa=np.array([1.0, 2.0, 3.0]), active_dims=[-1])   # the last column
    assert np.allclose(kk.Kdiag(X), [4.0, 2.0, 3.0, 4.0])
    kk.update_gradients_diag(np.array([1.0, 2.0, 3.0, 4.0]), X)
    assert np.allclose(kk.kappa.gradient, [2.0, 3.0, 5.0]) and np.allclose(kk.W.gradient, 2 * np.array([[2.0], [3.0], [5.0]]))
    assert np.array_equal(kk.gradients_X(np.ones((4, 4)), X), np.zeros((4, 2)))
    with pytest.raises(ValueError, match="output index"):
        kk.Kdiag(np.array([[0.5, 1.5]]))
    with pytest.raises(AssertionError):
        Coregionalize(2, 3)


def test_to_dict_strings():
    np.random.seed(0)
    k = Coregionalize(1, 2, rank=1, active_dims=[3])
    d = k.to_dict()
    assert d["class"] == "GPy.kern.Coregionalize" and d["output_dim"] == 2 and d["active_dims"] == [3]
    assert np.allclose(d["W"], k.W.values) and d["kappa"] == [0.5, 0.5]
    k2 = Coregionalize.from_dict(d)
    assert np.array_equal(k2._theta(), k._theta())
    lik = MixedNoise([Gaussian(0.1, name="Gaussian_noise_0"), Gaussian(0.2, name="Gaussian_noise_1")])
    d = lik.to_dict()
    assert d["class"] == "GPy.likelihoods.MixedNoise" and d["name"] == "mixed_noise"
    assert [e["variance"] for e in d["likelihoods_list"]] == [[0.1], [0.2]]


def test_mixed_noise_bookkeeping():
    lik = MixedNoise([Gaussian(0.1), Gaussian(0.2), Gaussian(0.3)])
    meta = {"output_index": np.array([[0], [2], [2], [1], [0]])}
    assert np.allclose(lik.gaussian_variance(meta), [0.1, 0.3, 0.3, 0.2, 0.1])
    assert lik.parameter_names() == ["Gaussian_noise.variance"] * 3
    assert np.allclose(lik.exact_inference_gradients(np.array([1.0, 2.0, 3.0, 4.0, 5.0]), meta), [6.0, 4.0, 5.0])
    lik.update_gradients(np.array([6.0, 4.0, 5.0]))
    assert np.allclose(lik.gradient, [6.0, 4.0, 5.0])
    mu, var = np.zeros((5, 1)), np.ones((5, 1))
    _, v = lik.predictive_values(mu, var, Y_metadata=meta)
    assert np.allclose(v[:, 0], [1.1, 1.3, 1.3, 1.2, 1.1]) and np.all(var == 1.0)
    _, c = lik.predictive_values(mu, np.eye(5), full_cov=True, Y_metadata=meta)
    assert np.allclose(np.diag(c), [1.1, 1.3, 1.3, 1.2, 1.1])
    assert np.allclose(lik.predictive_variance(mu, 2.0, meta), [4.1, 4.3, 4.3, 4.2, 4.1])
    lo, hi = lik.predictive_quantiles(mu, var, (2.5, 97.5), meta)
    from scipy import stats
    assert np.allclose(hi[:, 0], stats.norm.ppf(0.975) * np.sqrt([1.1, 1.3, 1.3, 1.2, 1.1]))
    lpd = lik.log_predictive_density(np.ones((5, 1)), mu, var, meta)
    assert np.allclose(lpd[:, 0], stats.norm.logpdf(1.0, scale=np.sqrt([1.1, 1.3, 1.3, 1.2, 1.1])))
    np.random.seed(0)
    assert lik.samples(np.zeros((5, 1)), meta).shape == (5, 1)
    with pytest.raises(NotImplementedError):
        MixedNoise([gpy_amd.HeteroscedasticGaussian({"output_index": np.arange(3)[:, None]})])


def test_combination_specs_carry_P_and_B():
    np.random.seed(2)
    B = Coregionalize(1, 4, rank=1, active_dims=[2])
    k = gpy_amd.RBF(2) * B
    (s0, s1) = k.part_specs()
    assert s1[0] == "coregionalize" and s1[1] == 4 and s1[2].size == 16 and list(s1[3]) == [2] and s1[4] == 1
    from gpy_amd._lib import KIND_IDS, ard_id, make_parts
    assert KIND_IDS["coregionalize"] == 8 and ard_id("coregionalize", 4) == 4
    arr, _, ntheta = make_parts(k.part_specs())
    assert arr[1].kind == 8 and arr[1].ard == 4 and arr[1].n_active == 1 and ntheta == 1 + 1 + 16
    neg = gpy_amd.RBF(1) * Coregionalize(1, 2, active_dims=[-1])
    with pytest.raises(ValueError, match="non-negative"):
        neg.part_specs()


class _Quad(models.GP):
    """a model without the device: f(x) = sum (x - c)^2 over its parameters"""

    def __init__(self, params, c):
        from gpy_amd.param import Parameterized
        Parameterized.__init__(self, "quad")
        self.c = c
        for p in params:
            self.link_parameter(p)
        self.calls = []

    def parameters_changed(self):
        self.calls.append(self.param_array.copy())

    def objective_function(self):
        return float(np.sum((self.param_array - self.c) ** 2))

    def objective_function_gradients(self):
        return 2 * (self.param_array - self.c)


def test_optimize_transform():
    from gpy_amd.param import Param
    # every parameter positive: the log transform, exactly as before (the first evaluation is at exp(log(x0)))
    m = _Quad([Param("a", [2.0, 3.0])], np.array([1.0, 5.0]))
    m.optimize(max_iters=50)
    assert np.allclose(m.param_array, [1.0, 5.0], atol=1e-5)
    assert np.array_equal(m.calls[0], np.exp(np.log(np.array([2.0, 3.0]))))
    # a positive=False parameter (Coregionalize's W) is optimised untransformed: it may cross zero
    m = _Quad([Param("W", [0.5, -0.2], positive=False), Param("kappa", [0.5])], np.array([-1.0, 0.7, 2.0]))
    m.optimize(max_iters=100)
    assert np.allclose(m.param_array, [-1.0, 0.7, 2.0], atol=1e-5)


def test_header_declares_kind_8():
    h = open(os.path.join(ROOT, "include", "mi355gp.h")).read()
    assert "MI355GP_COREGIONALIZE = 8" in h


def test_sparse_rejects_coregionalize_on_the_host():
    from gpy_amd.kern import exact_only_leaves
    np.random.seed(0)
    k = multioutput.ICM(1, 2, gpy_amd.RBF(1))
    assert exact_only_leaves(k) == ["Coregionalize"]
