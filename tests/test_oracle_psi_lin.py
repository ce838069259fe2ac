"""CPU: the long-double restatement of tests/psi_lin_ld.py and the host psi-statistics of `Linear`, `Bias` and
`Add(..., psi_lin_bias=True)` against the reference's own evaluation in tests/golden/psi_lin/*.npz (tools/make_golden_psi_lin.py):
`VarDTC.inference` with a `NormalPosterior`, the three `*_expectations` gradients plus the Kmm gradients, `_raw_predict` at
certain and at uncertain points, and the kernel-level psi0 / psi1 / psi2 / psi2n with their chain rule.

Tolerances are those tests/test_gpu_psi.py holds the reference's fixtures to: log marginal 1e-9, gradients, Woodbury vector
and predictive mean 1e-6, predictive variance 1e-5.  The restatement's analytic gradients are also held to central differences
of its own long-double bound (step 1e-7: truncation 1e-14 relative, rounding 1e-19 / 1e-7 = 1e-12 of the bound's magnitude,
so 1e-8 relative to the largest entry has two digits in hand).  The kernel-level RBF statistics need the device and are in
tests/test_gpu_psi_lin.py.
"""
import glob
import os

import numpy as np
import pytest

import psi_lin_ld as L

LD = np.longdouble
TOL_LML, TOL_FIT, TOL_VAR = 1e-9, 1e-6, 1e-5
FIXTURES = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "psi_lin", "*.npz")))
FIX_IDS = [os.path.basename(f)[:-4] for f in FIXTURES]
LINEAR_FIXTURES = [f for f in FIXTURES if os.path.basename(f).startswith("lin")]


def fixture_description(g):
    """the kernel description of tests/psi_lin_ld.py for a fixture"""
    dims = [int(d) for d in g["dims"]]
    k = dict(P=str(g["P"]), D=g["mu"].shape[1], dims=dims, ARD=bool(g["ARD"]), bias=[float(b) for b in g["bias"]],
             white=[float(w) for w in g["white"]])
    if k["P"] == "linear":
        k["v"] = np.asarray(g["theta"], dtype=float)
    else:
        k["var"], k["ls"] = float(g["theta"][0]), np.asarray(g["theta"][1:], dtype=float)
    return k


def _rel(x, ref):
    ref = np.asarray(ref, dtype=LD)
    return float(np.abs(np.asarray(x, dtype=LD) - ref).max() / np.abs(ref).max())


def test_there_are_fixtures_of_both_kinds():
    assert len(FIXTURES) >= 8 and 4 <= len(LINEAR_FIXTURES) < len(FIXTURES)


@pytest.mark.parametrize("path", FIXTURES, ids=FIX_IDS)
def test_long_double_restatement_meets_the_reference(path):
    g = np.load(path)
    k = fixture_description(g)
    dims = k["dims"]
    assert float(g["cond"]) <= 1e4
    r = L.evaluate(k, g["Z"], g["mu"], g["S"], g["Y"], float(g["noise"]), LD)
    figs = {"lml": abs(float(r["lml"]) - float(g["lml"])) / abs(float(g["lml"]))}
    for name, x, y in (("woodbury_vector", r["woodbury_vector"], g["woodbury_vector"]), ("dtheta", r["dtheta"], g["dtheta"]),
                       ("dnoise", np.atleast_1d(r["dnoise"]), g["dnoise"]), ("dZ", r["dZ"][:, dims], g["dZ"]),
                       ("dmu", r["dmu"][:, dims], g["dmu"]), ("dS", r["dS"][:, dims], g["dS"]), ("dL_dKmm", r["dL_dKmm"], g["dL_dKmm"]),
                       ("dL_dpsi1", r["dL_dpsi1"], g["dL_dpsi1"]), ("dL_dpsi2", r["dL_dpsi2"], g["dL_dpsi2"]),
                       ("woodbury_inv", r["woodbury_inv"], g["woodbury_inv"])):
        figs[name] = _rel(x, y)
    pm, pv = L.predict_certain(k, g["Z"], r, g["Xs"], LD)
    um, uv = L.predict(k, g["Z"], r, g["Xs"], g["Ss"], LD)
    figs.update(pred_mu=_rel(pm, g["pred_mu"]), upred_mu=_rel(um, g["upred_mu"]))
    var = {"pred_var": _rel(pv, g["pred_var"]), "upred_var": _rel(uv, g["upred_var"])}
    print({n: "%.2e" % v for n, v in list(figs.items()) + list(var.items())})
    assert figs.pop("lml") <= TOL_LML
    for name, e in figs.items():
        assert e <= TOL_FIT, (name, e)
    for name, e in var.items():
        assert e <= TOL_VAR, (name, e)
    rest = [d for d in range(k["D"]) if d not in dims]
    assert not np.asarray(r["dZ"])[:, rest].any() and not np.asarray(r["dmu"])[:, rest].any()
    # the KL pieces of the BayesianGPLVM composition
    KL = 0.5 * ((g["mu"][:, dims] ** 2).sum() + (g["S"][:, dims] - np.log(g["S"][:, dims])).sum() - g["mu"][:, dims].size)
    assert abs(KL - float(g["KL"])) <= 1e-12 * abs(KL) and abs(float(r["lml"]) - KL - float(g["bound"])) <= TOL_LML * abs(float(g["bound"]))
    assert _rel(np.asarray(r["dmu"], float)[:, dims] - g["mu"][:, dims], g["Xmean_grad"]) <= TOL_FIT
    assert _rel(np.asarray(r["dS"], float)[:, dims] - 0.5 * (1.0 - 1.0 / g["S"][:, dims]), g["Xvar_grad"]) <= TOL_FIT


@pytest.mark.parametrize("P,kw", [("linear", dict(bias=(0.7,), white=(0.2,))), ("rbf", dict(bias=(0.7,), white=())),
                                  ("rbf", dict(bias=(0.5, 0.3), white=(0.2,))), ("linear", dict(bias=(0.4, 0.3), white=(0.2,), ARD=False))],
                         ids=["linear+bias+white", "rbf+bias", "rbf+two_bias+white", "linear_iso+two_bias+white"])
def test_restatement_gradients_agree_with_central_differences_of_its_own_bound(P, kw):
    p = L.problem(P, 14, 5, 3, 2, 3, **kw)
    k = p["k"]
    r = L.evaluate(k, p["Z"], p["mu"], p["S"], p["Y"], p["noise"], LD)
    h = LD(1e-7)

    def bound(**ch):
        q = dict((x, np.array(p[x], dtype=LD)) for x in ("Z", "mu", "S"))
        kk = dict(k)
        noise = LD(p["noise"])
        for key, (idx, d) in ch.items():
            if key in q:
                q[key][idx] += d
            elif key == "noise":
                noise = noise + d
            else:
                a = np.array(np.atleast_1d(kk[key]), dtype=LD).copy()
                a[idx] += d
                kk[key] = a if key != "var" else a[0]
        return L.bound_only(kk, q["Z"], q["mu"], q["S"], p["Y"], noise, LD)

    def fd(key, idx):
        return (bound(**{key: (idx, h)}) - bound(**{key: (idx, -h)})) / (2 * h)
    worst = 0.0
    for key, ana in (("Z", r["dZ"]), ("mu", r["dmu"]), ("S", r["dS"])):
        for idx in ((0, 0), (3, 1), (4, 2)):
            worst = max(worst, abs(float(fd(key, idx) - ana[idx])) / float(np.abs(ana).max()))
    names = ([("v", i) for i in range(np.size(k["v"]))] if P == "linear" else [("var", 0)] + [("ls", i) for i in range(np.size(k["ls"]))])
    names += [("bias", i) for i in range(len(k["bias"]))] + [("white", i) for i in range(len(k["white"]))]
    num = np.array([float(fd(key, i)) for key, i in names])
    worst = max(worst, float(np.abs(num - np.asarray(r["dtheta"], float)).max() / np.abs(np.asarray(r["dtheta"], float)).max()))
    worst = max(worst, abs(float(fd("noise", 0) - r["dnoise"])) / abs(float(r["dnoise"])))
    print("worst relative distance from central differences %.2e" % worst)
    assert worst <= 1e-8


def _host_kernels(g):
    import gpy_amd
    k = fixture_description(g)
    Q = len(k["dims"])
    lone = gpy_amd.Linear(Q, variances=k["v"], ARD=k["ARD"])
    parts = [gpy_amd.Linear(Q, variances=k["v"], ARD=k["ARD"])] + [gpy_amd.Bias(Q, variance=b, name="bias%d" % i) for i, b in enumerate(k["bias"])] + \
        [gpy_amd.White(Q, variance=w, name="white%d" % i) for i, w in enumerate(k["white"])]
    return lone, (parts[0] if len(parts) == 1 else gpy_amd.Add(parts))


def _theta_grad(kern):
    return np.concatenate([np.atleast_1d(np.asarray(p.gradient, dtype=float)).ravel() for p in kern.flattened_parameters()])


@pytest.mark.parametrize("path", LINEAR_FIXTURES, ids=[os.path.basename(f)[:-4] for f in LINEAR_FIXTURES])
def test_host_psi_statistics_of_linear_bias_and_their_sum_meet_the_reference(path):
    """`Linear.psi*`, `Bias.psi*` and `Add.psi*(psi_lin_bias=True)` with the three gradient methods, on the fixture's active
    columns as the reference was given them"""
    import gpy_amd
    g = np.load(path)
    dims = [int(d) for d in g["dims"]]
    q = gpy_amd.NormalPosterior(g["mu"][:, dims], g["S"][:, dims])
    q4 = gpy_amd.NormalPosterior(g["mu"][:4, dims], g["S"][:4, dims])
    Z = g["Z"][:, dims]
    d0, d1, d2 = g["k_d0"], g["k_d1"], g["k_d2"]
    lone, total = _host_kernels(g)
    bias = gpy_amd.Bias(len(dims), variance=float(g["kb_variance"]))
    for tag, kern in (("kp", lone), ("ks", total), ("kb", bias)):
        kw = {"psi_lin_bias": True} if isinstance(kern, gpy_amd.Add) else {}
        for name, x in (("psi0", kern.psi0(Z, q, **kw)), ("psi1", kern.psi1(Z, q, **kw)), ("psi2", kern.psi2(Z, q, **kw)),
                        ("psi2n", kern.psi2n(Z, q4, **kw))):
            assert _rel(x, g["%s_%s" % (tag, name)]) <= 1e-12, (tag, name)
        assert _rel(kern.psi2n(Z, q, **kw).sum(0), kern.psi2(Z, q, **kw)) <= 1e-13, tag
        kern.update_gradients_expectations(d0, d1, d2, Z, q, **kw)
        assert _rel(_theta_grad(kern), g[tag + "_dtheta"]) <= 1e-11, tag
        gz = kern.gradients_Z_expectations(d0, d1, d2, Z, q, **kw)
        gm, gs = kern.gradients_qX_expectations(d0, d1, d2, Z, q, **kw)
        if tag != "kb":
            assert _rel(gz, g[tag + "_dZ"]) <= 1e-11 and _rel(gm, g[tag + "_dmu"]) <= 1e-11 and _rel(gs, g[tag + "_dS"]) <= 1e-11, tag
        else:                                                    # Bias: nothing depends on Z or on q(X)
            assert not g["kb_dZ"].any() and not g["kb_dmu"].any() and not g["kb_dS"].any()
            assert not gz.any() and not gm.any() and not gs.any()


def test_host_psi_statistics_refuse_what_is_out_of_scope_by_name():
    import gpy_amd
    q = gpy_amd.NormalPosterior(np.zeros((3, 2)), np.ones((3, 2)))
    Z = np.zeros((2, 2))
    lin, rbf, bias = gpy_amd.Linear(2), gpy_amd.RBF(2), gpy_amd.Bias(2)
    with pytest.raises(NotImplementedError, match="linear.*Linear.*psi_lin_bias=True"):
        (lin + bias).psi1(Z, q)                                  # without the keyword: as before, and told how to ask
    with pytest.raises(NotImplementedError, match="ONE input-dependent part.*RBF.*Linear"):
        (rbf + lin).psi2(Z, q, psi_lin_bias=True)
    with pytest.raises(NotImplementedError, match="ONE input-dependent part"):
        (rbf + gpy_amd.RBF(2, name="rbf2")).psi0(Z, q, psi_lin_bias=True)
    with pytest.raises(NotImplementedError, match="Mat52"):
        (gpy_amd.Matern52(2) + bias).psi0(Z, q, psi_lin_bias=True)
    with pytest.raises(NotImplementedError, match="Prod"):
        (lin * bias + gpy_amd.White(2)).psi0(Z, q, psi_lin_bias=True)
    with pytest.raises(NotImplementedError, match="per data point"):
        lin.update_gradients_expectations(np.zeros(3), np.zeros((3, 2)), np.zeros((3, 2, 2)), Z, q)
    with pytest.raises(NotImplementedError, match="per data point"):
        bias.update_gradients_expectations(np.zeros(3), np.zeros((3, 2)), np.zeros((3, 2, 2)), Z, q)


# ---- two Bias parts: the reference leaves its exact psi-statistics for quadrature then (add.py:33-44), so the yardstick of
# `Add.psi*(psi_lin_bias=True)` is the long-double restatement, itself held to central differences of its own objective ----------
def two_bias_yardstick(p, seed=91):
    """(psi_lin_ld.expectations in long double for seeded dL_dpsi0 / 1 / 2, (d0, d1, d2)); d2 is NOT symmetric"""
    r = np.random.default_rng(seed)
    N, M = p["mu"].shape[0], p["Z"].shape[0]
    d = (r.standard_normal(N), r.standard_normal((N, M)), r.standard_normal((M, M)))
    return L.expectations(p["k"], p["Z"], p["mu"], p["S"], d[0], d[1], d[2], LD), d


@pytest.mark.parametrize("P", ["linear", "rbf"])
def test_two_bias_yardstick_agrees_with_central_differences_of_its_objective(P):
    p = L.problem(P, 9, 4, 3, 1, 5, bias=(0.7, 0.3), white=(0.2,), ARD=(P == "rbf"))
    k = p["k"]
    want, d = two_bias_yardstick(p)
    h = LD(1e-7)

    def obj(**ch):
        q = dict((x, np.array(p[x], dtype=LD)) for x in ("Z", "mu", "S"))
        kk = dict(k)
        for key, (idx, step) in ch.items():
            if key in q:
                q[key][idx] += step
            else:
                a = np.array(np.atleast_1d(kk[key]), dtype=LD).copy()
                a[idx] += step
                kk[key] = a if key != "var" else a[0]
        return L.expectations_objective(kk, q["Z"], q["mu"], q["S"], d[0], d[1], d[2], LD)

    def fd(key, idx):
        return (obj(**{key: (idx, h)}) - obj(**{key: (idx, -h)})) / (2 * h)
    worst = 0.0
    for key, ana in (("Z", want["dZ"]), ("mu", want["dmu"]), ("S", want["dS"])):
        for idx in ((0, 0), (2, 1), (3, 2)):
            worst = max(worst, abs(float(fd(key, idx) - ana[idx])) / float(np.abs(ana).max()))
    names = ([("v", i) for i in range(np.size(k["v"]))] if P == "linear" else [("var", 0)] + [("ls", i) for i in range(np.size(k["ls"]))])
    names += [("bias", 0), ("bias", 1), ("white", 0)]
    num = np.array([float(fd(key, i)) for key, i in names])
    worst = max(worst, float(np.abs(num - np.asarray(want["dtheta"], float)).max() / np.abs(np.asarray(want["dtheta"], float)).max()))
    assert worst <= 1e-8, worst
    assert _rel(want["psi2n"].sum(0), want["psi2"]) <= 1e-16 * 100


@pytest.mark.parametrize("ARD,dims", [(True, None), (False, None), (True, (2, 0))], ids=["ard", "iso", "subset"])
def test_host_psi_statistics_of_linear_plus_two_bias_parts_meet_the_long_double_restatement(ARD, dims):
    """`Add.psi0 / psi1 / psi2 / psi2n (psi_lin_bias=True)` and the three gradient methods over Linear + Bias + Bias + White: the
    pairs of Bias parts in psi2 (N (b^2 - sum b_i^2) on top of the parts' own), every Bias part seeing the OTHER Bias part's psi1"""
    import gpy_amd
    p = L.problem("linear", 23, 6, 3, 2, 17, bias=(0.7, 0.3), white=(0.2,), ARD=ARD, dims=dims)
    kern = L.make_kernel(p["k"])
    want, d = two_bias_yardstick(p)
    q = gpy_amd.NormalPosterior(p["mu"], p["S"])
    kw = dict(psi_lin_bias=True)
    for name, x in (("psi0", kern.psi0(p["Z"], q, **kw)), ("psi1", kern.psi1(p["Z"], q, **kw)), ("psi2", kern.psi2(p["Z"], q, **kw)),
                    ("psi2n", kern.psi2n(p["Z"], q, **kw))):
        assert _rel(x, want[name]) <= 1e-13, name
    kern.update_gradients_expectations(d[0], d[1], d[2], p["Z"], q, **kw)
    assert _rel(_theta_grad(kern), want["dtheta"]) <= 1e-12
    assert _rel(kern.gradients_Z_expectations(d[0], d[1], d[2], p["Z"], q, **kw), want["dZ"]) <= 1e-12
    gm, gs = kern.gradients_qX_expectations(d[0], d[1], d[2], p["Z"], q, **kw)
    assert _rel(gm, want["dmu"]) <= 1e-12 and _rel(gs, want["dS"]) <= 1e-12
