"""CPU: the long-double restatement of the sparse (VarDTC) evaluation, tests/sparse_ld.py, and the judge that
tests/test_gpu_sparse_shapes.py holds the device to.

(1) The inputs of the sweep are what the tight bound rests on: for every case with a full long-double reference
    cond2(Kmm + 1e-8 I) <= 1e3 and the fp64 oracle (oracle/sparse_oracle.py) lies within 1e-11 of long double in every judged
    quantity, so bound(q) = max(32 e64(q), 256 eps64 kappa) never exceeds 3.2e-10.  Found: kappa 1 ... 303, e64 at most
    2e-12 (the D = 1 cases, whose scaled coordinates reach 43 in the oracle's |x|^2 + |z|^2 - 2 x.z), 5e-13 elsewhere.
(2) The restatement reproduces every sparse_*, sparse2_* and sparse3_* golden vector (the reference's own output) at the
    tolerances of tests/test_oracle_sparse.py.
(3) The blocked mode (fp64 per 4096-row block, long double across blocks and in everything M x M) against the full long-double
    evaluation at N = 9000, M = 65, D = 3, Dy = 2 (three blocks, the last one ragged), scalar | per-point noise: lml 9e-17 | 6e-16,
    dtheta 2e-15 | 1e-15, dnoise 5e-19 | 2e-14, dZ 4e-14 | 5e-14, woodbury_vector 7e-13 | 7e-13, dL_dm 5e-15 | 3e-15, dL_dKnm
    1e-13 | 1e-13, psi2 3e-16 | 3e-16, dL_dKmm 9e-15 | 8e-15, woodbury_inv 5e-17 | 6e-17 (relative to the largest entry); the bound
    asserted is the judge's floor 256 eps64 kappa = 4.8e-12: what the blocks round away is of relative size eps64 in psi2 and
    psi1V, and the M x M phase cannot amplify it by more than the condition of what it factorises.
(4) The judge rejects, at every case: one dZ entry off by 1e-9 of itself, the last row of X dropped, the last inducing point's
    column of psi1 zeroed, and (where the noise is per point) the noise replaced by its mean.
(5) Central differences (step 1e-6) of the long-double lml against dtheta, dZ and dnoise for the product + White case with
    per-point noise: agreement 1e-9."""
import numpy as np
import pytest

import kern_ld as KL
import sparse_ld as SL
from oracle import sparse_oracle as S
from test_oracle_sparse import (check_sparse, check_sparse2, load_sparse2_golden, load_sparse_golden, sparse2_golden_names,
                                sparse_golden_names)

pytestmark = pytest.mark.skipif(not KL.HAVE_LD, reason="np.longdouble is not an extended format on this host")
CORE = ("lml", "dtheta", "dnoise", "dZ", "woodbury_vector", "dL_dm", "dL_dKnm", "psi2", "dL_dKmm", "woodbury_inv")


# ---- (1) the inputs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SL.PLAIN)
def test_inputs_are_well_conditioned_and_fp64_is_within_1e_11(name):
    c, ref, r64, kappa = SL.reference(name)
    assert c["Z"].shape == (c["M"], c["D"]) and c["X"].shape == (c["N"], c["D"]) and c["R"].shape == (c["N"], c["Dy"])
    assert kappa <= 1e3
    for q in SL.JUDGED:
        e64 = SL.rel_err(r64[q], ref[q])
        assert e64 <= 1e-11, (q, e64)
        assert SL.bound(q, ref, r64, kappa) <= 3.2e-10
    figs, bad = SL.judge(r64, ref, r64, kappa)                 # the fp64 oracle itself passes, with all quantities judged
    assert not bad and set(figs) == set(SL.JUDGED)


def test_the_case_list_names_every_edge():
    shapes = set((c["family"], c["kern"], c["N"], c["M"], c["D"], c["Dy"], c["het"]) for c in SL.CASES)
    assert len(SL.BY_NAME) == len(SL.CASES)
    for M in (1, 127, 128, 129, 257):
        assert ("m_edge", "rbf_ard", 257, M, 2, 1, False) in shapes
    for N in (1, 2, 127, 128, 129, 255, 256, 257, 2049):
        for k in ("matern52_iso", "rbf_ard+bias"):
            assert ("n_edge", k, N, 65, 3, 2, False) in shapes
    for D, Dy in ((16, 4), (16, 5), (17, 1), (32, 4), (32, 5), (33, 1), (1, 1)):
        for k in ("rbf_ard", "matern32_ard"):
            assert ("dispatch", k, 193, 65, D, Dy, False) in shapes
    assert [SL.BY_NAME[n]["M"] for n in SL.STALE] == [129, 129, 128, 128] and SL.DETERMINISM in SL.BY_NAME
    a, b = SL.make_case(SL.STALE[0]), SL.make_case(SL.STALE[-1])
    assert np.array_equal(a["X"], b["X"]) and np.array_equal(a["R"], b["R"])     # no set_data between the members
    sub = SL.make_case("subset-rbf_ard_subset-n257_m65_d3_dy2-hom")
    assert SL.reference(sub["name"])[1]["dZ_zero_cols"] == [1]


# ---- (2) the reference's own output -----------------------------------------------------------------------------------------
def _specs_of_parts(parts):
    return [(p[0], int(bool(p[1])), np.concatenate([[p[2]], np.atleast_1d(p[3])]) if p[3] is not None else np.array([p[2]]),
             np.asarray(p[4], dtype=np.int32), p[5] if len(p) > 5 else 0) for p in parts]


def _f64(res):
    return dict((k, KL.f64(v)) for k, v in res.items() if k != "dZ_zero_cols")


@pytest.mark.parametrize("name", sparse_golden_names())
def test_restatement_matches_reference_golden(name):
    g = load_sparse_golden(name)
    D = g["X"].shape[1]
    ls = g["lengthscale"] if g["ARD"] else g["lengthscale"][:1]
    specs = _specs_of_parts([(g["kind"], g["ARD"], g["variance"], ls, list(range(D)))])
    res = _f64(SL.vardtc(specs, g["X"], g["Z"], g["Y"], g["noise"]))
    res["lml"], res["dnoise"] = float(res["lml"]), float(res["dnoise"])
    check_sparse(res, g)
    assert np.abs(res["woodbury_inv"] - g["woodbury_inv"]).max() <= 1e-4 * np.abs(g["woodbury_inv"]).max()


@pytest.mark.parametrize("name", sparse2_golden_names())
def test_restatement_matches_general_reference_golden(name):
    g = load_sparse2_golden(name)
    specs = _specs_of_parts(g["parts"])
    ld = SL.vardtc(specs, g["X"], g["Z"], g["R"], g["noise"])
    res = _f64(ld)
    res["lml"] = float(res["lml"])
    check_sparse2(res, g)
    assert np.abs(res["dL_dm"] - g["dL_dm"]).max() <= 1e-7 * np.abs(g["dL_dm"]).max()
    assert np.abs(res["dL_dKnm"][g["rows"]] - g["dL_dKnm_rows"]).max() <= 1e-6 * np.abs(g["dL_dKnm_rows"]).max()
    assert np.abs(res["dL_dKmm"] - g["dL_dKmm"]).max() <= 1e-4 * np.abs(g["dL_dKmm"]).max()
    mu, var = SL.predict(specs, g["Z"], g["Xs"], ld)
    _, cov = SL.predict(specs, g["Z"], g["Xs"], ld, full_cov=True)
    assert np.abs(KL.f64(mu) - g["pred_mu"]).max() <= 1e-6 * np.abs(g["pred_mu"]).max()
    assert np.abs(KL.f64(var) - g["pred_var"]).max() <= 1e-5 * np.abs(g["pred_var"]).max()
    assert np.abs(KL.f64(cov) - g["pred_cov"]).max() <= 1e-5 * np.abs(g["pred_cov"]).max()


# ---- (3) the blocked mode ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("het", [False, True], ids=["scalar_noise", "per_point_noise"])
def test_blocked_mode_against_full_long_double(het):
    c = SL.make_case("n_edge-rbf_ard+bias-n2049_m65_d3_dy2-hom")             # its Z and kernel, 9000 rows of its own
    rng = np.random.default_rng(5)
    N = 9000
    X = rng.uniform(0.0, 1.0, (N, 3))
    R = np.sin(3.0 * X[:, :2]) + 0.2 * rng.standard_normal((N, 2))
    noise = 0.03 + 0.1 * rng.uniform(0.0, 1.0, N) if het else 0.07
    full = SL.vardtc(c["specs"], X, c["Z"], R, noise)
    blk = SL.vardtc(c["specs"], X, c["Z"], R, noise, block=4096)
    kappa = float(np.linalg.cond(KL.f64(full["Kmm"])))
    for q in CORE:
        d = SL.rel_err(blk[q], full[q])
        print("blocked vs full %s: %.2e" % (q, d))
        assert d <= 256.0 * KL.EPS64 * kappa, q


# ---- (4) the judge bites -----------------------------------------------------------------------------------------------------
def _drop_last_column(P):
    P = P.copy()
    P[:, -1] = 0
    return P


@pytest.mark.parametrize("name", SL.PLAIN)
def test_judge_rejects_small_faults(name):
    c, ref, r64, kappa = SL.reference(name)
    core = lambda res: dict((q, res[q]) for q in CORE)           # noqa: E731
    # one dZ entry off by 1e-9 of itself
    got = core(r64)
    got["dZ"] = np.array(r64["dZ"])
    i = np.unravel_index(np.argmax(np.abs(got["dZ"])), got["dZ"].shape)
    got["dZ"][i] *= 1.0 + 1e-9
    figs, bad = SL.judge(got, ref, r64, kappa)
    assert len(bad) == 1 and bad[0].startswith("dZ:"), bad
    # the last row of X dropped (blocked mode with one block: the fp64 restatement of the N-row operations)
    n1 = c["N"] - 1
    got = SL.vardtc(c["specs"], c["X"][:n1], c["Z"], c["R"][:n1], c["noise"][:n1] if c["het"] else c["noise"], block=max(n1, 1))
    figs, bad = SL.judge(core(got), ref, r64, kappa)
    assert any(b.startswith("lml:") for b in bad) and any(b.startswith("psi2:") for b in bad), bad
    # the last inducing point's column of psi1 zeroed
    got = SL.vardtc(c["specs"], c["X"], c["Z"], c["R"], c["noise"], block=c["N"], psi1_hook=_drop_last_column)
    figs, bad = SL.judge(core(got), ref, r64, kappa)
    assert any(b.startswith("lml:") for b in bad) and any(b.startswith("psi2:") for b in bad), bad
    # per-point noise replaced by its mean
    if c["het"]:
        got = S.vardtc_general(c["parts"], c["X"], c["Z"], c["R"], np.full(c["N"], np.mean(c["noise"])))
        figs, bad = SL.judge(dict((q, got[q]) for q in CORE if q != "psi2"), ref, r64, kappa)
        assert any(b.startswith("lml:") for b in bad) and any(b.startswith("dnoise:") for b in bad), bad
    # a dZ column outside every part's active_dims must be exactly zero
    for col in ref["dZ_zero_cols"]:
        got = core(r64)
        got["dZ"] = np.array(r64["dZ"])
        got["dZ"][0, col] = 1e-300
        assert SL.judge(got, ref, r64, kappa)[1]


# ---- (5) finite differences in long double -----------------------------------------------------------------------------------
def test_long_double_gradients_by_central_differences():
    c, ref, _, _ = SL.reference("noise-prod-n257_m65_d3_dy1-het")
    h = 1e-6
    lml = lambda specs, Z, noise: SL.vardtc(specs, c["X"], Z, c["R"], noise)["lml"]     # noqa: E731

    def check(what, fd, g):
        print("%s: central difference %.12e, gradient %.12e" % (what, float(fd), float(g)))
        assert abs(fd - g) <= 1e-9 * max(abs(g), 1), what
    k = 0
    for i, s in enumerate(c["specs"]):
        for j in range(len(s[2])):
            def at(d):
                th = np.array(s[2], dtype=np.float64)
                th[j] += d
                return c["specs"][:i] + [(s[0], s[1], th, s[3], s[4])] + c["specs"][i + 1:], KL.LD(th[j])
            (sp, tp), (sm, tm) = at(h), at(-h)
            check("dtheta[%d]" % k, (lml(sp, c["Z"], c["noise"]) - lml(sm, c["Z"], c["noise"])) / (tp - tm), ref["dtheta"][k])
            k += 1
    for m, q in ((0, 0), (c["M"] - 1, 2)):
        Zp, Zm = c["Z"].copy(), c["Z"].copy()
        Zp[m, q] += h
        Zm[m, q] -= h
        check("dZ[%d, %d]" % (m, q), (lml(c["specs"], Zp, c["noise"]) - lml(c["specs"], Zm, c["noise"])) / KL.LD(Zp[m, q] - Zm[m, q]),
              ref["dZ"][m, q])
    for n in (0, c["N"] - 1):
        p, m_ = c["noise"].copy(), c["noise"].copy()
        p[n] += h
        m_[n] -= h
        check("dnoise[%d]" % n, (lml(c["specs"], c["Z"], p) - lml(c["specs"], c["Z"], m_)) / KL.LD(p[n] - m_[n]), ref["dnoise"][n])
