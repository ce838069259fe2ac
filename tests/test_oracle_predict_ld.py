"""CPU: the long-double restatement of the exact path's prediction side (tests/predict_ld.py) and its judge, before the GPU
sweep (tests/test_gpu_predict_shapes.py) relies on either.

(1) The restatement is right: mu / var through the quantiles, cov, dmu and dvar against every fixture made by the reference's
    own kernel / posterior objects (`test_oracle_predict.load_predict_golden`), at the tolerances tests/test_gpu_predict.py
    holds the device to.
(2) The ceiling: for every case of the sweep and every quantity, max(32 e64, 256 eps64 kappa) stays at or below the standing
    tolerance (1e-9 for mu / var / cov / covb, 1e-8 for dmu / dvar), so no case is judged more loosely than the older tests
    judge.  This is a condition on the inputs: a case that breaks it gets other inputs, never another ceiling.
(3) The judge accepts an independent fp64 pipeline -- SciPy cho_factor / cho_solve / solve_triangular, BLAS products, the
    kernels of oracle/gp_oracle.py (`predictive_gradients` where a case is one stationary part), tests/periodic_np.py and
    tests/mlp_np.py -- on one case of every family.
(4) The judge rejects planted faults on the fp64 result, each written as an edit of a correct array or of the reduction that
    formed it (the unedited reconstruction is accepted first, so a rejection is the fault's):
      a  the last row of a 256-row block left out of the reduction over n (n = 257: row 255; n = 513: row 256)
      b  the second row split dropped (n = 513: rows 257 ...)
      c  the ones column, the x*_q sum_j H_ij term of the stationary finish, dropped
      d  dimension 32 taken from dimension 0's record (D = 33)
      e  alpha[i] read for alpha[i * Dy + d] (Dy = 2)
      f  the weights transposed for StdPeriodic at M = N = 65
      g  the dKdiag term of Linear and of MLP omitted
      h  covb written with pitch M1 instead of M2 ((63, 65))
      i  new point 64 given new point 63's values
      j  a coincident pair contributing its unmasked term (Exponential: (dK/dr) / r at r = 0)
      and a non-zero in a column that belongs to no part.
"""
import numpy as np
import pytest
from scipy.linalg import cho_factor, cho_solve, solve_triangular

from oracle import gp_oracle as O

import kern_ld as KL
import mlp_np as MN
import periodic_np as PN
import predict_ld as P
from test_oracle_predict import load_predict_golden, predict_golden_names

pytestmark = pytest.mark.skipif(not KL.HAVE_LD, reason="np.longdouble is not an extended format on this host")
O_KINDS = ("rbf", "matern52", "matern32", "exponential")


# ---- (1) the restatement against the reference's fixtures --------------------------------------------------------------------
@pytest.mark.parametrize("name", predict_golden_names())
def test_restatement_matches_reference_golden(name):
    g = load_predict_golden(name)
    D = g["X"].shape[1]
    specs = [(g["kind"], int(g["ARD"]), np.concatenate([[g["variance"]], g["ls"]]), np.arange(D), 0)]
    X9 = g["Xs"][:9]
    for dt in (KL.LD, np.float64):
        r = P.evaluate(specs, g["X"], g["Y"], g["noise"], g["Xs"], X9, X9, dt=dt, max_n=g["X"].shape[0])
        q = O.predictive_quantiles(KL.f64(r["mu"]), KL.f64(r["var"]), g["noise"], (2.5, 50.0, 97.5))
        assert np.abs(np.stack(q) - g["quantiles"]).max() <= 1e-9 * np.abs(g["quantiles"]).max()
        assert np.abs(KL.f64(r["mu"]) - g["mu"]).max() <= 1e-9 * np.abs(g["mu"]).max()
        assert np.abs(KL.f64(r["var"]) - g["var"]).max() <= 1e-9 * np.abs(g["var"]).max()
        assert r["dmu"].shape == g["mean_jac"].shape and r["dvar"].shape == g["var_jac"].shape
        assert np.abs(KL.f64(r["dmu"]) - g["mean_jac"]).max() <= 1e-8 * np.abs(g["mean_jac"]).max()
        assert np.abs(KL.f64(r["dvar"]) - g["var_jac"]).max() <= 1e-7 * np.abs(g["var_jac"]).max()
        assert np.abs(KL.f64(r["covb"]) - g["cov"]).max() <= 1e-9
        assert np.abs(KL.f64(r["cov"])[:9, :9] - g["cov"]).max() <= 1e-9


def test_dKdiag_dX_is_the_derivative_of_Kdiag():
    """the one formula predict_ld states itself, against central differences of kern_ld.Kdiag in long double"""
    rng = np.random.default_rng(4)
    Xs = rng.standard_normal((7, 4))
    specs = [("linear", 1, np.array([0.3, 0.9]), np.array([0, 2]), 0), ("mlp", 1, np.array([1.2, 0.4, 0.7, 0.2, 0.4]), np.array([1, 2, 3]), 0),
             ("mlp", 0, np.array([0.8, 0.6, 0.1]), np.array([0, 3]), 0), ("rbf", 0, np.array([1.0, 1.0]), np.arange(4), 0),
             ("bias", 0, np.array([0.5]), np.arange(4), 0)]
    g = P.dKdiag_dX(specs, Xs)
    h = KL.LD(1e-6)
    for q in range(4):
        Xp, Xm = KL._a(Xs, KL.LD).copy(), KL._a(Xs, KL.LD).copy()
        Xp[:, q] += h
        Xm[:, q] -= h
        fd = (KL.Kdiag(specs, Xp) - KL.Kdiag(specs, Xm)) / (2 * h)
        assert np.max(np.abs(fd - g[:, q])) <= 1e-10 * np.max(np.abs(g))


# ---- (2) the ceiling ---------------------------------------------------------------------------------------------------------
def test_the_sweep_has_every_family_and_shape_edge():
    assert set(c["family"] for c in P.CASES) == set(P.FAMILIES)
    assert sorted(set(P.BY_NAME[n]["N"] for n in P.by_family("n_edge"))) == [1, 2, 127, 128, 129, 255, 256, 257, 512, 513]
    assert sorted(set(P.BY_NAME[n]["M"] for n in P.by_family("m_edge"))) == [1, 63, 64, 65, 128, 129, 257]
    assert sorted(set(P.BY_NAME[n]["D"] for n in P.by_family("d_edge"))) == [8, 9, 16, 17, 32, 33, 64, 65]
    assert sorted(set(P.BY_NAME[n]["Dy"] for n in P.by_family("dy"))) == [1, 2, 4, 5]
    assert len(P.by_family("kinds")) == 2 * (16 + 6) and len(P.by_family("covb")) == 21
    assert sum(1 for c in P.CASES if c["N"] >= 512) == 11 and max(c["N"] for c in P.CASES) == P.MAX_N
    assert P.DETERMINISM in P.BY_NAME


@pytest.mark.parametrize("name", P.NAMES)
def test_bound_stays_at_or_below_the_standing_tolerance(name):
    c, ref, r64, kappa = P.reference(name)
    b = P.bounds(name)
    print("CEIL %s kappa %.3g " % (name, kappa) + " ".join("%s %.2e" % (q, b[q]) for q in b))
    want = ("mu", "var", "cov") + (() if P.has_product(c["specs"]) else ("dmu", "dvar")) + (("covb",) if c["family"] == "covb" else ())
    assert tuple(q for q in P.QUANTITIES if q in b) == tuple(q for q in P.QUANTITIES if q in want)
    for q in b:
        assert b[q] <= P.CEILING[q], (q, b[q])
    # the fp64 restatement is inside its own bound, with the exact zeros
    figs, bad = P.judge(r64, ref, r64, kappa)
    assert not bad, bad


def test_inputs_keep_their_deliberate_edges():
    c = P.make_case("n_edge-stdperiodic_ard-plus_white-n257_m65_d3_dy2")
    X, Xs, T = c["X"], c["Xs"], c["specs"][0][2][1]
    assert np.array_equal(X[0], X[1]) and np.array_equal(Xs[0], X[-1]) and X[-1, 0] - X[2, 0] == T
    c = P.make_case("d_edge-linear_ard-plus_white-n129_m65_d33_dy1")
    assert np.all(c["X"][3] == 0) and np.all(np.any(np.delete(c["X"], 3, axis=0) != 0, axis=1))   # the zero row: moved off N // 2
    assert np.array_equal(c["Xs"][0], c["X"][-1]) and np.array_equal(c["X"][0], c["X"][1])
    c = P.make_case("covb-matern32_iso-times_rbf-n129_m63_d3_dy1_mm65")
    assert c["X"].shape == (129, 5) and c["X1"].shape == (63, 5) and c["X2"].shape == (65, 5) and np.array_equal(c["X2"][-1], c["X1"][0])
    c = P.make_case("sum-rbf+matern32_ard+linear+white+bias-sum-n129_m65_d5_dy2")
    assert P.zero_cols(c["specs"], 5) == [4]
    c = P.make_case("kinds-cosine_ard-plus_white-n129_m130_d5_dy4")
    assert P.zero_cols(c["specs"], 5) == [0, 1, 3, 4]


# ---- (3) an independent fp64 pipeline ----------------------------------------------------------------------------------------
def _scatter(g, dims, D):
    out = np.zeros((g.shape[0], D))
    out[:, dims] = g
    return out


def _leaf64(spec, A, B):
    """(K(A, B), G -> gradients_X(G, A, B)) of one part in fp64: gp_oracle for the four stationary kinds, periodic_np for
    RatQuad / StdPeriodic, mlp_np (and linear_np under it) for Linear, MLP, White and Bias"""
    kind, ard, th, dims, _ = spec
    if kind in O_KINDS:
        a, b = A[:, dims], None if B is None else B[:, dims]
        return (O.kern_K(kind, a, b, th[0], th[1:], bool(ard)),
                lambda G: _scatter(O.gradients_X(kind, G, a, b, th[0], th[1:], bool(ard)), dims, A.shape[1]))
    K, _, dX = (PN if kind in ("ratquad", "stdperiodic") else MN).leaf_parts(spec, A, B)
    return K, lambda G: np.einsum("ij,ijq->iq", G, dX)


def _K64(specs, A, B=None):
    out = 0.0
    for t in KL.terms(specs):
        out = out + np.prod([_leaf64(specs[i], A, B)[0] for i in t], axis=0)
    return out


def _gX64(specs, G, A, B):
    return sum(_leaf64(s, A, B)[1](G) for s in specs)


def independent64(c):
    specs, X, Y, Xs = c["specs"], c["X"], c["Y"], c["Xs"]
    N, (M, D) = X.shape[0], Xs.shape
    Ky = _K64(specs, X) + (c["noise"] + P.JITTER) * np.eye(N)
    cf = cho_factor(Ky, lower=True)
    L = np.tril(cf[0])
    alpha, Ki = cho_solve(cf, Y), cho_solve(cf, np.eye(N))
    Kx = _K64(specs, X, Xs)
    T = solve_triangular(L, Kx, lower=True)
    out = dict(mu=Kx.T @ alpha, var=(MN.Kdiag(specs, Xs) - np.sum(T * T, 0))[:, None], cov=_K64(specs, Xs) - T.T @ T)
    moving = [s for s in specs if s[0] not in P.STATIC]
    if not P.has_product(specs):
        if len(moving) == 1 and moving[0][0] in O_KINDS and all(s[0] == "white" for s in specs if s is not moving[0]):
            kind, ard, th, dims, _ = moving[0]                                   # one stationary part: the oracle's own caller
            mj, vj = O.predictive_gradients(kind, X[:, dims], Xs[:, dims], alpha, Ki, th[0], th[1:], bool(ard))
            out["dmu"] = np.stack([_scatter(mj[:, :, d], dims, D) for d in range(Y.shape[1])], axis=2)
            out["dvar"] = _scatter(vj, dims, D)
        else:
            out["dmu"] = np.stack([_gX64(specs, np.ones((M, 1)) * alpha[:, d][None, :], Xs, X) for d in range(Y.shape[1])], axis=2)
            dkd = np.zeros((M, D))
            for s in moving:
                if s[0] == "linear":
                    dkd[:, s[3]] += 2.0 * np.broadcast_to(s[2], (len(s[3]),)) * Xs[:, s[3]]
                elif s[0] == "mlp":
                    dkd += MN.mlp_diag_grads(s, np.ones(M), Xs)[1]
            out["dvar"] = _gX64(specs, -2.0 * Kx.T @ Ki, Xs, X) + dkd
    if "X1" in c:
        T1, T2 = solve_triangular(L, _K64(specs, X, c["X1"]), lower=True), solve_triangular(L, _K64(specs, X, c["X2"]), lower=True)
        out["covb"] = _K64(specs, c["X1"], c["X2"]) - T1.T @ T2
    return out


# (no Exponential case: gp_oracle takes r^2 from |x|^2 + |z|^2 - 2 x.z, which leaves r = 1e-8 at the coincident pairs of these
# inputs, and exp(-r) is not smooth there -- its answer is 1e-8 off, as kern_ld.make_case(edges=False) exists to say)
INDEPENDENT = ["kinds-matern52_ard-plus_white-n129_m130_d5_dy4", "kinds-ratquad_iso-alone-n65_m63_d33_dy1",
               "m_edge-stdperiodic_ard-alone-n65_m129_d3_dy1", "n_edge-mlp_iso-plus_white-n257_m65_d3_dy2",
               "d_edge-ratquad_ard-plus_white-n129_m65_d33_dy1", "dy-linear_iso-alone-n65_m65_d2_dy5",
               "sum-rbf+matern32_ard+linear+white+bias-sum-n129_m65_d5_dy2", "covb-matern32_iso-times_rbf-n129_m63_d3_dy1_mm65",
               "covb-rbf_ard-alone-n129_m130_d3_dy1_mm257", "covb-linear_ard-alone-n129_m1_d3_dy1_mm129"]


def test_independent_cases_cover_every_family():
    assert set(P.BY_NAME[n]["family"] for n in INDEPENDENT) == set(P.FAMILIES)


@pytest.mark.parametrize("name", INDEPENDENT)
def test_judge_accepts_an_independent_fp64_pipeline(name):
    c, ref, r64, kappa = P.reference(name)
    got = independent64(c)
    figs, bad = P.judge(got, ref, r64, kappa)
    print(P.figures_line(name, kappa, figs))
    assert set(figs) == set(q for q in P.QUANTITIES if q in ref)
    assert not bad, bad


# ---- (4) planted faults ------------------------------------------------------------------------------------------------------
class Pieces(object):
    """the fp64 pieces of a case's gradients: T[m, n, q] = dK(x*_m, x_n)/dx*_mq, alpha (N x Dy), A2 = -2 K(X*, X) Ky^-1"""

    def __init__(self, name):
        self.name = name
        self.c, self.ref, self.r64, self.kappa = P.reference(name)
        c = self.c
        self.T = P.dx_tensor(c["specs"], c["Xs"], c["X"], np.float64)
        self.alpha = self.r64["alpha"]
        self.A2 = -2.0 * np.asarray(KL.K(c["specs"], c["Xs"], c["X"], np.float64)) @ self.r64["Ki"]
        self.dkd = P.dKdiag_dX(c["specs"], c["Xs"], np.float64)

    def dmu(self, T=None, alpha=None, rows=slice(None)):
        T, alpha = self.T if T is None else T, self.alpha if alpha is None else alpha
        return np.einsum("mnq,nd->mqd", T[:, rows], alpha[rows])

    def dvar(self, T=None, A2=None, rows=slice(None), dkd=True):
        T, A2 = self.T if T is None else T, self.A2 if A2 is None else A2
        return np.einsum("mnq,mn->mq", T[:, rows], A2[:, rows]) + (self.dkd if dkd else 0.0)

    def bad(self, **got):
        return P.judge(got, self.ref, self.r64, self.kappa)[1]

    def accepted(self):
        """the unedited reconstruction passes, so that a rejection below is the fault's"""
        bad = self.bad(dmu=self.dmu(), dvar=self.dvar())
        assert not bad, bad
        return self

    def rejects(self, **got):
        bad = self.bad(**got)
        for q in got:
            assert any(b.startswith(q + ":") or b.startswith(q + " column") for b in bad), (self.name, q, bad)


def _n_edge(v, N):
    return "n_edge-%s-plus_white-n%d_m65_d3_dy2" % (v, N)


@pytest.mark.parametrize("variant", P.REPS)
@pytest.mark.parametrize("N,row", [(257, 255), (513, 256)])
def test_fault_a_last_row_of_a_block_left_out(variant, N, row):
    p = Pieces(_n_edge(variant, N)).accepted()
    keep = np.delete(np.arange(N), row)
    p.rejects(dmu=p.dmu(rows=keep), dvar=p.dvar(rows=keep))


@pytest.mark.parametrize("variant", P.REPS)
def test_fault_b_second_row_split_dropped(variant):
    p = Pieces(_n_edge(variant, 513)).accepted()
    p.rejects(dmu=p.dmu(rows=slice(0, 257)), dvar=p.dvar(rows=slice(0, 257)))


def test_fault_c_ones_column_dropped():
    """the stationary finish: (x*_q sum_n H_mn - sum_n H_mn x_nq) / l_q^2 with H = weights x (dK/dr) / r; without the ones
    column the first sum is missing"""
    p = Pieces("m_edge-rbf_ard-alone-n65_m65_d3_dy1").accepted()
    c = p.c
    lf = KL._Leaf(c["specs"][0], c["Xs"], c["X"], np.float64)
    ls2 = np.square(np.asarray(lf.ls, dtype=np.float64))
    for weights, q in ((np.ones((65, 1)) * p.alpha[:, 0][None, :], "dmu"), (p.A2, "dvar")):
        H = weights * lf.dK_dr * lf.inv
        full = (c["Xs"] * np.sum(H, axis=1)[:, None] - H @ c["X"]) / ls2
        lost = (-H @ c["X"]) / ls2
        shape = lambda a: a[:, :, None] if q == "dmu" else a
        assert not p.bad(**{q: shape(full)})
        p.rejects(**{q: shape(lost)})


def test_fault_d_dimension_32_from_dimension_0s_record():
    p = Pieces("d_edge-rbf_ard-plus_white-n129_m65_d33_dy1").accepted()
    dmu, dvar = p.dmu(), p.dvar()
    dmu[:, 32], dvar[:, 32] = dmu[:, 0].copy(), dvar[:, 0].copy()
    p.rejects(dmu=dmu, dvar=dvar)


@pytest.mark.parametrize("variant", ("rbf_iso", "linear_iso"))
def test_fault_e_alpha_read_without_its_stride(variant):
    p = Pieces("dy-%s-alone-n65_m65_d2_dy2" % variant).accepted()
    flat = np.concatenate([p.alpha.ravel(), [0.0]])
    wrong = np.stack([flat[d:d + 65] for d in range(2)], axis=1)                 # v[i] of alpha + d, not v[i * Dy]
    p.rejects(dmu=p.dmu(alpha=wrong))


def test_fault_f_weights_transposed_for_stdperiodic():
    p = Pieces("m_edge-stdperiodic_ard-alone-n65_m65_d3_dy1").accepted()
    p.rejects(dvar=p.dvar(A2=p.A2.T.copy()))
    p.rejects(dmu=np.einsum("mnq,md->mqd", p.T, p.alpha))                         # G[m][n] = alpha[m]


@pytest.mark.parametrize("variant", ("linear_ard", "mlp_iso"))
def test_fault_g_dKdiag_term_omitted(variant):
    p = Pieces("m_edge-%s-alone-n65_m65_d3_dy1" % variant).accepted()
    assert np.max(np.abs(p.dkd)) > 0
    p.rejects(dvar=p.dvar(dkd=False))


@pytest.mark.parametrize("variant,label", [("rbf_ard", "alone"), ("matern32_iso", "times_rbf"), ("linear_ard", "alone")])
def test_fault_h_covb_written_with_the_pitch_of_the_other_side(variant, label):
    name = "covb-%s-%s-n129_m63_d3_dy1_mm65" % (variant, label)
    c, ref, r64, kappa = P.reference(name)
    C = KL.f64(r64["covb"])
    M1, M2 = C.shape
    assert (M1, M2) == (63, 65) and not P.judge(dict(covb=C), ref, r64, kappa)[1]
    buf = np.zeros(M1 * M2 + M2)
    for i in range(M1):
        buf[i * M1:i * M1 + M2] = C[i]
    bad = P.judge(dict(covb=buf[:M1 * M2].reshape(M1, M2)), ref, r64, kappa)[1]
    assert bad and bad[0].startswith("covb:")
    assert P.judge(dict(covb=C.T), ref, r64, kappa)[1]                            # and a transposed answer: another shape


def test_fault_i_new_point_64_given_new_point_63s_values():
    p = Pieces("m_edge-rbf_ard-alone-n65_m65_d3_dy1").accepted()
    got = dict(mu=KL.f64(p.r64["mu"]).copy(), var=KL.f64(p.r64["var"]).copy(), cov=KL.f64(p.r64["cov"]).copy(), dmu=p.dmu(), dvar=p.dvar())
    assert not p.bad(**got)
    for q in ("mu", "var", "dmu", "dvar"):
        got[q][64] = got[q][63]
    got["cov"][64, :] = got["cov"][63, :]
    got["cov"][:, 64] = got["cov"][:, 63]
    p.rejects(**got)


def test_fault_j_coincident_pair_unmasked():
    """Exponential: (dK/dr) / r = -K / r has no limit at r = 0; unmasked, the pair (new point 0, the last training point) gives
    inf x 0.  The judge must not let a NaN through."""
    p = Pieces("kinds-exponential_iso-alone-n65_m63_d33_dy1").accepted()
    c = p.c
    lf = KL._Leaf(c["specs"][0], c["Xs"], c["X"], np.float64)
    assert lf.r[0, 64] == 0.0 and np.all(p.T[0, 64] == 0.0)
    T = p.T.copy()
    with np.errstate(divide="ignore", invalid="ignore"):
        for q in range(33):
            T[:, :, q] = lf.dK_dr / lf.r * lf._diff(q) / lf.ls[q] ** 2
    assert np.isnan(T[0, 64]).all() and np.allclose(np.delete(T, 0, axis=0), np.delete(p.T, 0, axis=0), rtol=1e-13, atol=0)
    p.rejects(dmu=p.dmu(T=T), dvar=p.dvar(T=T))


def test_fault_nonzero_in_a_column_of_no_part():
    p = Pieces("sum-rbf+matern32_ard+linear+white+bias-sum-n129_m65_d5_dy2").accepted()
    dmu, dvar = p.dmu(), p.dvar()
    assert np.all(dmu[:, 4] == 0) and np.all(dvar[:, 4] == 0)
    dmu[17, 4, 1] = 1e-300
    dvar[64, 4] = -1e-300
    bad = p.bad(dmu=dmu, dvar=dvar)
    assert len(bad) == 2 and all("column 4" in b for b in bad)
