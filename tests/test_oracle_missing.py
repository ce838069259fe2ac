"""CPU: the restatement of the missing-data loop (tests/missing_ld.py) and the host side of the group-batched psi2 kernels.

1. `missing_ld.psi2_groups` / `psi_grad_groups` (the restatement of the stateless pair of include/mi355gp_sparse_missing.h) in
   float64 against long double on the shapes the device is judged on (`CASES`), relative to the largest entry (psi2: per group):
       psi2 1.7e-15   dvar 3.3e-15   dl 1.2e-15   dZ 1.7e-15   dmu 7.0e-15   dS 6.6e-15
   worst over the shapes, rounded up in the last digit (`F64_DISTANCE`; the test prints the figures and holds them to twice these: NumPy's exp differs by an ulp between its SIMD
   dispatches).  Times ten they bound the device in tests/test_gpu_missing.py.
2. The gradients of the restatement against central differences of its own objective in long double, for the stateless pair and
   for the whole bound (KL included).
3. `missing_ld.evaluate` with nothing missing is `psi_np.vardtc_uncertain`; grouping and its order.
4. `_lib.MISSING_ABI` / `DEBUG_MISSING_ABI` against the prototypes of include/mi355gp_sparse_missing.h and its debug header.
5. The restatement against fixtures made by the reference's own loop (tests/golden/missing, tools/make_golden_missing.py), and the
   host classes over a recording context: grouping, uploads, parameter order, refusals, pickling."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import missing_ld as ML
import psi_np as P

LD = np.longdouble
HERE = os.path.dirname(os.path.abspath(__file__))
GB = 8                                                                  # PSI_GB of csrc/psi_missing.h (the GPU test asserts it)
GRADS = ("dvar", "dl", "dZ", "dmu", "dS")
# (name, N, M, Q, G, ARD): the edges of the kernels' tilings -- 16-tiles of (m, o), 16 / 32 / 64 staged rows, 2048-row chunks,
# padded dimension counts 1 .. 64 with the 32-wide accumulator groups, and group batches G = 1, 2, GB, GB + 1, 2 GB + 1
CASES = [
    ("n1_m1_q1_g1", 1, 1, 1, 1, True),
    ("n15_m15_q3_g2", 15, 15, 3, 2, False),
    ("n17_m17_q16_g8", 17, 17, 16, GB, True),
    ("n63_m65_q17_g9", 63, 65, 17, GB + 1, True),
    ("n65_m17_q33_g17", 65, 17, 33, 2 * GB + 1, True),
    ("n257_m130_q2_g2", 257, 130, 2, 2, True),
    ("n2049_m17_q3_g9", 2049, 17, 3, GB + 1, True),
    ("n63_m15_q64_g1", 63, 15, 64, 1, False),
    ("n17_m65_q1_g8", 17, 65, 1, GB, True),
]
F64_DISTANCE = dict(psi2=1.7e-15, dvar=3.3e-15, dl=1.2e-15, dZ=1.7e-15, dmu=7.0e-15, dS=6.6e-15)


def rel(x, ref):
    ref = np.asarray(ref, dtype=LD)
    return float(np.abs(np.asarray(x, dtype=LD) - ref).max() / max(float(np.abs(ref).max()), 1e-300))


def rel_groups(x, ref):
    """worst over the groups, each relative to ITS largest entry (a group observed in one row is small next to one observed in all)"""
    return max(rel(a, b) for a, b in zip(x, ref))


@functools.lru_cache(maxsize=None)
def reference(name, dtype=LD):
    """(problem, psi2_g, dict of the five gradients) of a case in `dtype`, computed once per process"""
    _, N, M, Q, G, ARD = next(c for c in CASES if c[0] == name)
    p = ML.group_problem(N, M, Q, G, 11, ARD)
    a = (p["var"], p["ls"], p["Z"], p["mu"], p["S"], p["W"])
    psi2 = ML.psi2_groups(*a, dtype=dtype)
    g = ML.psi_grad_groups(p["var"], p["ls"], ARD, p["Z"], p["mu"], p["S"], p["W"], p["dL"], dtype=dtype)
    return p, psi2, dict(zip(GRADS, g))


def test_case_masks_cover_the_edges():
    for name, N, M, Q, G, ARD in CASES:
        W = ML.group_problem(N, M, Q, G, 11, ARD)["W"]
        assert W.shape == (N, G) and set(np.unique(W)) <= {0.0, 1.0} and W.any(0).all()
        if G > 1:
            assert W[:, 0].all() and W[:, 1].sum() == 1 and W[N - 1, 1] == 1   # every row; the last row only
        if N > 1:
            assert not W[0, 1:].any() and (G > 1 or not W[0].any())              # G == 1: a row in no group
    W = ML.group_problem(2049, 17, 3, GB + 1, 11, True)["W"]
    assert not W[:2048, 1].any()                                                 # the first 2048-row chunk is all zero for group 1


def test_float64_restatement_distance_from_long_double():
    worst = dict.fromkeys(F64_DISTANCE, 0.0)
    for c in CASES:
        _, a2, ga = reference(c[0], LD)
        _, b2, gb = reference(c[0], np.float64)
        d = dict(psi2=rel_groups(b2, a2))
        d.update((k, rel(gb[k], ga[k])) for k in GRADS)
        print("%-18s %s" % (c[0], "  ".join("%s %.1e" % kv for kv in d.items())))
        worst = dict((k, max(worst[k], d[k])) for k in worst)
    print("worst              %s" % "  ".join("%s %.1e" % kv for kv in worst.items()))
    for k, v in worst.items():
        assert v <= 2 * F64_DISTANCE[k], (k, v)


def _objective(p, dtype=LD, **over):
    q = dict(p, **over)
    psi2 = ML.psi2_groups(q["var"], q["ls"], q["Z"], q["mu"], q["S"], q["W"], dtype=dtype)
    sym = 0.5 * (np.asarray(q["dL"], dtype=dtype) + np.transpose(np.asarray(q["dL"], dtype=dtype), (0, 2, 1)))
    return (sym * psi2).sum()


def test_group_gradients_against_central_differences_in_long_double():
    p = ML.group_problem(9, 5, 2, 3, 3, True)
    dvar, dl, dZ, dmu, dS = ML.psi_grad_groups(p["var"], p["ls"], True, p["Z"], p["mu"], p["S"], p["W"], p["dL"], dtype=LD)
    h = LD(1e-8)
    cd = lambda k, xp, xm: (_objective(p, **{k: xp}) - _objective(p, **{k: xm})) / (2 * h)
    ok = lambda a, b: abs(a - b) <= 1e-7 * max(1.0, abs(float(b)))
    assert ok(cd("var", LD(p["var"]) + h, LD(p["var"]) - h), dvar)
    for name, grad in (("ls", dl), ("Z", dZ), ("mu", dmu), ("S", dS)):
        x = np.asarray(p[name], dtype=LD)
        for i in ([(0,), (1,)] if x.ndim == 1 else [(0, 0), (2, 1), (x.shape[0] - 1, 1)]):
            xp, xm = x.copy(), x.copy()
            xp[i] += h
            xm[i] -= h
            assert ok(cd(name, xp, xm), grad[i]), (name, i)
    q = dict(p, W=p["W"].copy())                                        # a row in NO group: exactly zero
    q["W"][0] = 0.0
    g = ML.psi_grad_groups(q["var"], q["ls"], True, q["Z"], q["mu"], q["S"], q["W"], q["dL"], dtype=LD)
    assert not np.any(g[3][0]) and not np.any(g[4][0])


def test_grouping_follows_the_first_output_index():
    Y = np.arange(30.0).reshape(5, 6)
    Y[1, [0, 3]] = np.nan
    Y[[2, 4], 2] = np.nan
    Y[1, 5] = np.nan
    gof, W = ML.groups_of(Y)
    assert list(gof) == [0, 1, 2, 0, 1, 0]
    assert np.array_equal(W, np.array([[1, 1, 1], [0, 1, 1], [1, 1, 0], [1, 1, 1], [1, 1, 0]], dtype=float))


def test_evaluate_without_missing_entries_is_the_complete_data_evaluation():
    p = P.fit_problem(23, 7, 2, 3, 5, white=[0.02])
    a = ML.evaluate(p["var"], p["ls"], True, p["white"], p["Z"], p["mu"], p["S"], p["Y"], p["noise"], LD, kl=False)
    b = P.vardtc_uncertain(p["var"], p["ls"], True, p["white"], p["Z"], p["mu"], p["S"], p["Y"], p["noise"], LD)
    assert list(a["group_of_output"]) == [0, 0, 0] and a["W"].all()
    assert abs(a["bound"] - b["lml"]) <= 1e-15 * abs(b["lml"])
    for k in ("woodbury_vector", "dL_dKmm", "dnoise", "dvar", "dl", "dZ", "dmu", "dS"):
        assert rel(a[k], b[k]) <= 1e-15, k


def test_bound_gradients_against_central_differences_in_long_double():
    p = ML.fit_problem(9, 4, 2, 5, 3, patterns=3, white=[0.03])
    ev = lambda **o: ML.evaluate(*[dict(p, **o)[k] for k in ("var", "ls", "ARD", "white", "Z", "mu", "S", "Y", "noise")], dtype=LD)
    r = ev()
    assert r["W"].shape[1] == 3 and r["W"][:, 2].sum() == 1 and r["kappa"] <= 1e4
    h = LD(1e-8)
    ok = lambda a, b: abs(a - b) <= 1e-7 * max(1.0, abs(float(b)))
    for name, grad in (("Z", r["dZ"]), ("mu", r["dmu"] - r["kl_dmu"]), ("S", r["dS"] - r["kl_dS"]), ("ls", r["dl"])):
        x = np.asarray(p[name], dtype=LD)
        for i in ([(0,), (1,)] if x.ndim == 1 else [(0, 0), (1, 1), (x.shape[0] - 1, 1)]):
            xp, xm = x.copy(), x.copy()
            xp[i] += h
            xm[i] -= h
            assert ok((ev(**{name: xp})["bound"] - ev(**{name: xm})["bound"]) / (2 * h), grad[i]), (name, i)
    for name, grad in (("var", r["dvar"]), ("noise", r["dnoise"])):
        x = LD(p[name])
        assert ok((ev(**{name: x + h})["bound"] - ev(**{name: x - h})["bound"]) / (2 * h), grad), name
    w = LD(p["white"][0])
    assert ok((ev(white=[w + h])["bound"] - ev(white=[w - h])["bound"]) / (2 * h), r["dwhite"][0])


@functools.lru_cache(maxsize=None)
def fit_reference(name):
    """(problem, long-double evaluation, float64 evaluation, new points) of a fit case, computed once per process"""
    _, N, M, Q, Dy, patterns, ARD = next(c for c in ML.FIT_CASES if c[0] == name)
    p = ML.lattice_problem(N, M, Q, Dy, 7, patterns, ARD)
    ev = lambda dt: ML.evaluate(p["var"], p["ls"], ARD, p["white"], p["Z"], p["mu"], p["S"], p["Y"], p["noise"], dt, kl=False)
    r = np.random.default_rng(3)
    Xs, Ss = r.uniform(p["Z"].min(0), p["Z"].max(0) + 1e-9, (7, Q)), r.uniform(0.05, 0.4, (7, Q))
    out = []
    for dt in (LD, np.float64):
        e = ev(dt)
        e["dtheta"] = np.concatenate([np.ravel(e["dvar"]), np.ravel(e["dl"]), np.ravel(e["dwhite"])])
        e["pred_mu"], e["pred_var"] = ML.predict(p["var"], p["ls"], p["white"], p["Z"], e, Xs, None, dt)
        e["upred_mu"], e["upred_var"] = ML.predict(p["var"], p["ls"], p["white"], p["Z"], e, Xs, Ss, dt)
        out.append(e)
    return p, out[0], out[1], Xs, Ss


@pytest.mark.parametrize("case", ML.FIT_CASES, ids=[c[0] for c in ML.FIT_CASES])
def test_fit_inputs_are_well_conditioned_and_cover_the_mask_edges(case):
    name, N, M, Q, Dy, patterns, ARD = case
    p, ref, r64, _, _ = fit_reference(name)
    assert ref["kappa"] <= 1e4, ref["kappa"]
    W, gof = ref["W"], ref["group_of_output"]
    assert W.shape[1] == min(patterns, Dy) and list(gof) == [d % patterns for d in range(Dy)]
    if N > 2:
        assert not W[1].any()                                          # a row nothing observes
    if patterns > 2 and Dy >= patterns:
        assert W[:, patterns - 1].sum() == 1                           # a group observed in one row only
    assert rel(r64["bound"], ref["bound"]) <= 1e-11


def test_prediction_with_the_3d_woodbury_inv_reduces_to_the_2d_one_per_group():
    p = ML.fit_problem(12, 4, 2, 4, 9, patterns=2)
    r = ML.evaluate(p["var"], p["ls"], True, p["white"], p["Z"], p["mu"], p["S"], p["Y"], p["noise"], LD)
    rs = np.random.default_rng(1)
    Xs, Ss = rs.uniform(-2, 2, (5, 2)), rs.uniform(0.05, 0.4, (5, 2))
    mu, var = ML.predict(p["var"], p["ls"], p["white"], p["Z"], r, Xs, None, LD)
    um, uv = ML.predict(p["var"], p["ls"], p["white"], p["Z"], r, Xs, Ss, LD)
    assert mu.shape == var.shape == um.shape == uv.shape == (5, 4)
    assert np.array_equal(var[:, 0], var[:, 2]) and not np.array_equal(var[:, 0], var[:, 1])    # outputs 0, 2 share a group
    _, small = ML.predict(p["var"], p["ls"], p["white"], p["Z"], r, Xs, 1e-12 * np.ones_like(Ss), LD)
    assert rel(small, var) <= 1e-9                                     # S -> 0: the uncertain branch meets the certain one


# ---- the C-ABI table ------------------------------------------------------------------------------------------------------
def test_the_binding_tables_match_the_headers_and_the_library_exports_them():
    from gpy_amd import _lib
    names = {"mi355gp_sparse_missing.h": ("MISSING_ABI", ["mi355gp_psi_groups_batch", "mi355gp_rbf_psi2_groups", "mi355gp_rbf_psi_grad_groups",
                                                          "mi355gp_sparse_set_output_groups", "mi355gp_vardtc_inference_missing",
                                                          "mi355gp_sparse_select_output_group", "mi355gp_sparse_fetch_group_scalars"]),
             "mi355gp_debug_sparse_missing.h": ("DEBUG_MISSING_ABI", ["mi355gp_dbg_rbf_psi2_groups", "mi355gp_dbg_rbf_psi_grad_groups"])}
    _lib.build()
    for header, (table_name, expected) in names.items():
        table = getattr(_lib, table_name)
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(HERE, "..", "include", header)).read(), flags=re.S)
        protos = re.findall(r"\bint\s+(mi355gp_\w+)\s*\(([^;]*?)\)\s*;", text)
        assert [p[0] for p in protos] == list(table) == expected
        for name, params in protos:
            params = [] if params.strip() == "void" else [" ".join(p.split()) for p in params.split(",")]
            bound = table[name]
            assert len(bound) == len(params), name
            for c, b in zip(params, bound):
                if "double*" in c:
                    assert getattr(b, "_dtype_", None) == np.dtype(np.float64) or b is ctypes.POINTER(ctypes.c_double), (name, c)
                elif c.startswith("int64_t"):
                    assert b is ctypes.c_int64, (name, c)
                elif c.startswith("double"):
                    assert b is ctypes.c_double, (name, c)
                elif c.startswith("mi355gp_sparse*"):
                    assert b is ctypes.c_void_p, (name, c)
                elif "mi355gp_part*" in c:
                    assert b is ctypes.POINTER(_lib.Part), (name, c)
                elif "int*" in c:
                    assert b is ctypes.POINTER(ctypes.c_int), (name, c)
                else:
                    assert c.startswith("int ") and b is ctypes.c_int, (name, c)
            assert name not in _lib.ABI                               # not in mi355gp.h: its prototype count stays
            assert hasattr(_lib.lib(), name), "libmi355gp.so does not export %s" % name
        assert table_name in __import__("inspect").getsource(_lib.lib)
    # the group calls are the single-mask pair with (W, G) for `weights`; the diagnostics add the loop switch and the stream time
    one, grp, dbg = _lib.ABI["mi355gp_rbf_psi"], _lib.MISSING_ABI["mi355gp_rbf_psi2_groups"], _lib.DEBUG_MISSING_ABI["mi355gp_dbg_rbf_psi2_groups"]
    assert grp[:10] == one[:10] and len(grp) == len(one) and dbg[:12] == grp[:12] and len(dbg) == len(grp) + 2
    # the fit takes the arguments of the complete-data uncertain entry
    assert _lib.MISSING_ABI["mi355gp_vardtc_inference_missing"] == _lib.ABI["mi355gp_vardtc_inference_uncertain"]


# ---- the host classes (nothing here reaches a device) -------------------------------------------------------------------------
def test_the_model_is_exported_where_the_reference_has_it():
    import gpy_amd as GPy
    assert hasattr(GPy.models, "BayesianGPLVMMiniBatch")
    assert GPy.models.bayesian_gplvm_minibatch.BayesianGPLVMMiniBatch is GPy.models.BayesianGPLVMMiniBatch is GPy.BayesianGPLVMMiniBatch
    assert issubclass(GPy.BayesianGPLVMMiniBatch, GPy.BayesianGPLVM) and GPy.BayesianGPLVMMiniBatch.kl_factr == 1


def test_output_groups_of_the_binding_follow_the_restatement_and_store_zeros():
    from gpy_amd import _lib
    p = ML.fit_problem(12, 4, 2, 7, 3, patterns=3)
    gof, W, Y0 = _lib.output_groups(p["Y"])
    rg, rW = ML.groups_of(p["Y"])
    assert list(gof) == list(rg) == [0, 1, 2, 0, 1, 2, 0] and np.array_equal(W, rW) and gof.dtype == np.int32
    assert not np.isnan(Y0).any() and np.all(Y0[np.isnan(p["Y"])] == 0) and np.array_equal(Y0[~np.isnan(p["Y"])], p["Y"][~np.isnan(p["Y"])])


class _NoContext(object):
    """stands where the device context would be made: any use is a failure of the test"""
    def __getattr__(self, name):
        raise AssertionError("the refusal came after the context was touched (%s)" % name)


def test_refusals_come_by_name_before_any_context_is_touched(monkeypatch):
    import gpy_amd
    from gpy_amd import _lib
    monkeypatch.setattr(_lib, "SparseContext", lambda *a, **k: _NoContext())
    p = ML.fit_problem(12, 4, 2, 4, 3, patterns=2)
    q = gpy_amd.NormalPosterior(p["mu"], p["S"])
    rbf, lik = gpy_amd.RBF(2, ARD=True), gpy_amd.Gaussian(0.1)
    inf = lambda **kw: gpy_amd.VarDTC(**kw).inference
    for call, exc, pat in (
            (lambda: inf()(rbf, p["mu"], p["Z"], lik, p["Y"], missing_data=True), NotImplementedError, "certain inputs"),
            (lambda: inf()(rbf, gpy_amd.SpikeAndSlabPosterior(p["mu"], p["S"], 0.5 * np.ones_like(p["S"])), p["Z"], lik, p["Y"], missing_data=True),
             NotImplementedError, "spike-and-slab"),
            (lambda: inf(psi_lin_bias=True)(rbf, q, p["Z"], lik, p["Y"], missing_data=True), NotImplementedError, "psi_lin_bias"),
            (lambda: inf()(rbf + gpy_amd.Bias(2), q, p["Z"], lik, p["Y"], missing_data=True), NotImplementedError, "Bias"),
            (lambda: inf()(gpy_amd.Matern52(2), q, p["Z"], lik, p["Y"], missing_data=True), NotImplementedError, "Matern52"),
            (lambda: inf()(rbf, q, p["Z"], lik, p["Y"], missing_data=True, precision=np.ones(12)), NotImplementedError, "per-point"),
            (lambda: inf()(rbf, q, p["Z"], lik, p["Y"], missing_data=True, psi2=np.ones((4, 4))), NotImplementedError, "precomputed"),
            (lambda: inf()(rbf, q, p["Z"], lik, np.where(np.arange(4) == 2, np.nan, p["Y"]), missing_data=True), ValueError, "column 2 has no observed"),
    ):
        with pytest.raises(exc, match=pat):
            call()
    M = gpy_amd.BayesianGPLVMMiniBatch
    X = p["mu"]
    for kw, exc, pat in ((dict(stochastic=True), NotImplementedError, "stochastic"), (dict(batchsize=2), NotImplementedError, "batchsize"),
                         (dict(normalizer=True), NotImplementedError, "normalizer"), (dict(X_variance=False), NotImplementedError, "sparse GPLVM"),
                         (dict(likelihood=gpy_amd.Bernoulli()), NotImplementedError, "Bernoulli"),
                         (dict(inference_method=gpy_amd.VarDTC(psi_lin_bias=True)), NotImplementedError, "plain VarDTC"),
                         (dict(missing_data=False), ValueError, "pass missing_data=True"), (dict(missing_data=True, X=None), ValueError, "pass X")):
        with pytest.raises(exc, match=pat):
            M(p["Y"], 2, **dict(dict(X=X, missing_data=True), **kw))
    with pytest.raises(NotImplementedError, match="BayesianGPLVMMiniBatch takes missing_data=True"):
        gpy_amd.BayesianGPLVM(np.nan_to_num(p["Y"]), 2, X=X, missing_data=True)


# ---- the reference's own numbers (tests/golden/missing, tools/make_golden_missing.py) -------------------------------------------
import glob  # noqa: E402

FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "missing", "*.npz")))
FIXTURE_IDS = [os.path.basename(f)[:-4] for f in FIXTURES]
TOL_LML, TOL_FIT, TOL_VAR = 1e-9, 1e-6, 1e-5                          # the sparse path's tolerances (tests/test_gpu_sparse.py)
FIXTURE_TOL = dict(bound=TOL_LML, lml=TOL_LML, lml_g=TOL_LML, pred_var=TOL_VAR, upred_var=TOL_VAR)


def check_against_fixture(got, g):
    """every quantity of `got` that the fixture holds, at 1e-9 (bounds), 1e-5 (variances) or 1e-6 (everything else)"""
    for k, v in got.items():
        e = rel(v, g[k]) if np.shape(v) == np.shape(g[k]) else float("inf")
        assert e <= FIXTURE_TOL.get(k, TOL_FIT), (k, e)


def fixture_problem(g):
    return dict(var=float(g["variance"]), ls=np.asarray(g["ls"], float), ARD=bool(g["ARD"]), white=[float(x) for x in g["white"]],
                Z=g["Z"], mu=g["mu"], S=g["S"], Y=g["Y"], noise=float(g["noise"]))


def test_the_fixtures_cover_what_the_issue_names():
    assert len(FIXTURES) >= 4
    gs = [np.load(f) for f in FIXTURES]
    assert any(bool(g["ARD"]) for g in gs) and any(not bool(g["ARD"]) for g in gs) and any(len(g["white"]) for g in gs)
    for g in gs:
        W, gof = g["W"], g["group_of_output"]
        assert float(g["cond"]) <= 1e4
        assert max(np.bincount(gof)) > 1                               # several columns in a group
        assert not W[1].any()                                          # a row nothing observes
        assert W[:, -1].sum() == 1                                     # a group observed in one row only
        assert g["woodbury_inv"].shape == (g["Z"].shape[0],) * 2 + (g["Y"].shape[1],)


@pytest.mark.parametrize("path", FIXTURES, ids=FIXTURE_IDS)
def test_restatement_meets_the_references_composed_loop(path):
    g = np.load(path)
    p = fixture_problem(g)
    r = ML.evaluate(p["var"], p["ls"], p["ARD"], p["white"], p["Z"], p["mu"], p["S"], p["Y"], p["noise"], np.float64)
    assert list(r["group_of_output"]) == list(g["group_of_output"]) and np.array_equal(r["W"], g["W"])
    pm, pv = ML.predict(p["var"], p["ls"], p["white"], p["Z"], r, g["Xs"], None)
    um, uv = ML.predict(p["var"], p["ls"], p["white"], p["Z"], r, g["Xs"], g["Ss"])
    Wi = np.moveaxis(r["woodbury_inv"][r["group_of_output"]], 0, 2)   # M x M x Dy, the reference's layout
    check_against_fixture(dict(bound=r["bound"], lml=r["lml"], lml_g=r["lml_g"], woodbury_vector=r["woodbury_vector"], woodbury_inv=Wi,
                               dL_dKmm=r["dL_dKmm"], dL_dpsi0=r["dL_dpsi0"], dnoise=np.ravel(r["dnoise"]),
                               dtheta=np.concatenate([np.ravel(r["dvar"]), np.ravel(r["dl"]), np.ravel(r["dwhite"])]), dZ=r["dZ"],
                               dmu=r["dmu"], dS=r["dS"], Xmean_grad=r["dmu"] - r["kl_dmu"], Xvar_grad=r["dS"] - r["kl_dS"],
                               pred_mu=pm, pred_var=pv, upred_mu=um, upred_var=uv), g)


# ---- host logic over a recording context ----------------------------------------------------------------------------------------
class RecordingContext(object):
    """stands where `_lib.SparseContext` does: records what the host classes upload and answers a fit from the float64 restatement"""
    FETCH_DLDKMM, FETCH_WOODBURY_INV, FETCH_LM, FETCH_KMM, FETCH_PSI2, FETCH_DLDPSI2_BETA = 0, 1, 2, 3, 4, 5
    made = []

    def __init__(self, device=0):
        self.calls, self.G = [], 0
        RecordingContext.made.append(self)

    def set_data(self, X, Y):
        assert not np.isnan(Y).any()
        self.mu, self.Y0, self.G = np.array(X), np.array(Y), 0
        self.calls.append("set_data")

    def set_input_variance(self, S):
        self.S = np.array(S)
        self.calls.append("set_input_variance")

    def set_inputs(self, X, S=None):
        self.mu, self.S = np.array(X), np.array(S)
        self.calls.append("set_inputs")

    def set_output_groups(self, gof, W):
        self.calls.append("set_output_groups" if gof is not None else "clear_output_groups")
        self.G = 0 if gof is None else W.shape[1]
        self.group_of_output, self.W = (None, None) if gof is None else (np.array(gof), np.array(W))

    def vardtc_missing(self, specs, Z, noise, extra_jitter=0.0, want_stage_ms=False):
        assert self.G > 0 and [s[0] for s in specs] == ["rbf", "white"]
        th = specs[0][2]
        Y = np.where(self.W[:, self.group_of_output] > 0, self.Y0, np.nan)
        r = ML.evaluate(th[0], th[1:], bool(specs[0][1]), [specs[1][2][0]], Z, self.mu, self.S, Y, float(noise[0]), kl=False)
        self.calls.append("vardtc_missing")
        gs = np.zeros((self.G, 8))
        gs[:, 0], gs[:, 1] = r["lml_g"], r["dnoise_g"]
        return 0, dict(lml=float(r["lml"]), dnoise=float(r["dnoise"]), dZ=r["dZ"], dmu=r["dmu"], dS=r["dS"], group_scalars=gs,
                       dtheta=np.concatenate([np.ravel(r["dvar"]), np.ravel(r["dl"]), np.ravel(r["dwhite"])]),
                       woodbury_vector=r["woodbury_vector"])

    def vardtc_uncertain(self, specs, Z, noise, extra_jitter=0.0, want_stage_ms=False):
        assert self.G == 0, "the Gaussian entry on a context that holds groups"
        self.calls.append("vardtc_uncertain")
        N, Q = self.mu.shape
        return 0, dict(lml=0.0, dnoise=0.0, dZ=np.zeros(Z.shape), dmu=np.zeros((N, Q)), dS=np.zeros((N, Q)), dtheta=np.zeros(Q + 2),
                       woodbury_vector=np.zeros((Z.shape[0], self.Y0.shape[1])))


@pytest.fixture
def recording(monkeypatch):
    from gpy_amd import _lib
    RecordingContext.made = []
    monkeypatch.setattr(_lib, "SparseContext", RecordingContext)
    return RecordingContext


def _host_model(g):
    import gpy_amd
    p = fixture_problem(g)
    Q = p["mu"].shape[1]
    kern = gpy_amd.RBF(Q, variance=p["var"], lengthscale=p["ls"], ARD=p["ARD"]) + gpy_amd.White(Q, variance=p["white"][0])
    return p, gpy_amd.BayesianGPLVMMiniBatch(p["Y"], Q, X=p["mu"], X_variance=p["S"], Z=p["Z"], kernel=kern,
                                             likelihood=gpy_amd.Gaussian(p["noise"]), missing_data=True)


def test_model_over_a_recording_context_parameter_order_uploads_and_the_references_numbers(recording):
    import pickle
    import gpy_amd
    g = np.load([f for f in FIXTURES if "white_dy12" in f][0])
    p, m = _host_model(g)
    (ctx,) = recording.made
    assert ctx.calls == ["set_data", "set_input_variance", "set_output_groups", "vardtc_missing"]
    assert np.array_equal(ctx.group_of_output, g["group_of_output"]) and np.array_equal(ctx.W, g["W"])
    assert np.all(ctx.Y0[np.isnan(p["Y"])] == 0)                       # NaN -> 0 with the mask
    N, Q, M = m.num_data, m.input_dim, m.num_inducing
    # flat parameter order [X.mean, X.variance, Z, kernel (variance, lengthscale, white), noise]
    names = [q.name for q in m.flattened_parameters()]
    assert [q.size for q in m.flattened_parameters()] == [N * Q, N * Q, M * Q, 1, Q, 1, 1] and names[2] == "inducing inputs"
    x = m.param_array
    assert np.array_equal(x[:N * Q].reshape(N, Q), p["mu"]) and np.array_equal(x[N * Q:2 * N * Q].reshape(N, Q), p["S"])
    assert np.array_equal(x[2 * N * Q:2 * N * Q + M * Q].reshape(M, Q), p["Z"]) and x[-1] == p["noise"] and x[-2] == p["white"][0]
    grad, o = m.gradient, 2 * N * Q
    check_against_fixture(dict(bound=m.log_likelihood(), Xmean_grad=grad[:N * Q].reshape(N, Q), Xvar_grad=grad[N * Q:o].reshape(N, Q),
                               dZ=grad[o:o + M * Q].reshape(M, Q), dtheta=grad[o + M * Q:-1], dnoise=grad[-1:],
                               dL_dpsi0=m.grad_dict["dL_dpsi0"]), g)
    assert m.kl_factr == 1
    # a step of q(X): the inputs alone travel
    n0 = len(ctx.calls)
    x = m.param_array.copy()
    x[:N * Q] += 0.01
    m.param_array = x
    assert ctx.calls[n0:] == ["set_inputs", "vardtc_missing"]
    # the inference class without the keyword on the same context: the groups are cleared first
    inf = m.inference_method
    n1 = len(ctx.calls)
    inf.inference(m.kern, m.X, m.Z.values, m.likelihood, np.nan_to_num(p["Y"]))
    assert "clear_output_groups" in ctx.calls[n1:] and ctx.calls[-1] == "vardtc_uncertain"
    # pickling drops the context and everything that names what it holds: the copy starts afresh, with or without the keyword
    inf.inference(m.kern, m.X, m.Z.values, m.likelihood, p["Y"], missing_data=True)
    twin = pickle.loads(pickle.dumps(inf))
    assert twin._ctx is None and twin._groups_of is None and twin._groups_mask is None
    twin.inference(m.kern, m.X, m.Z.values, m.likelihood, np.nan_to_num(p["Y"]))
    assert recording.made[-1].calls[-1] == "vardtc_uncertain" and "clear_output_groups" not in recording.made[-1].calls


def test_a_nan_that_becomes_an_observed_zero_uploads_the_mask_again(recording):
    import gpy_amd
    g = np.load(FIXTURES[0])
    p = fixture_problem(g)
    Q = p["mu"].shape[1]
    kern = gpy_amd.RBF(Q, variance=p["var"], lengthscale=p["ls"], ARD=p["ARD"]) + gpy_amd.White(Q, variance=0.1)
    q, lik, inf = gpy_amd.NormalPosterior(p["mu"], p["S"]), gpy_amd.Gaussian(p["noise"]), gpy_amd.VarDTC()
    _, a, _ = inf.inference(kern, q, p["Z"], lik, p["Y"], missing_data=True)
    (ctx,) = recording.made
    Y = p["Y"].copy()
    i = tuple(np.argwhere(np.isnan(Y))[-1])                            # an unobserved entry becomes an observed exact 0.0: the
    Y[i] = 0.0                                                         # zero-filled Y is the same array, the mask is not
    n0 = len(ctx.calls)
    _, b, _ = inf.inference(kern, q, p["Z"], lik, Y, missing_data=True)
    assert "set_output_groups" in ctx.calls[n0:] and ctx.W.sum() == g["W"].sum() + 1 or ctx.W.shape[1] != g["W"].shape[1]
    r = ML.evaluate(p["var"], p["ls"], p["ARD"], [0.1], p["Z"], p["mu"], p["S"], Y, p["noise"], kl=False)
    assert a != b and abs(b - float(r["lml"])) <= 1e-12 * abs(b)


def test_certain_input_missing_data_is_refused_where_the_reference_has_its_class():
    import gpy_amd as GPy
    with pytest.raises(NotImplementedError, match="SparseGPMiniBatch.*BayesianGPLVMMiniBatch"):
        GPy.models.SparseGPMiniBatch
    for name in ("MRD", "GPLVM"):
        with pytest.raises(NotImplementedError, match=name):
            getattr(GPy.models, name)
