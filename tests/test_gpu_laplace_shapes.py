"""GPU (-m gpu): the Laplace / EP session on the exact context -- mi355gp_laplace_begin / newton / finish / gradients / implicit /
predict, mi355gp_ep_recompute / mi355gp_ep_sweep and the three fetches, i.e. csrc/laplace.hip with its session
kernels and csrc/ep.hip -- at every shape edge, judged against the long-double restatement tests/laplace_ld.py
(80-bit; tests/test_oracle_laplace_ld.py is its own proof).

Judge (laplace_ld.judge): err(q) = max |got - q_ld| / max |q_ld| <= max(32 e64(q), 256 eps64 kappa), e64 = the distance of the
same formulas in fp64 from long double on the same input (never the device's figure), kappa = cond2(B), B = I + W^1/2 K W^1/2
in fp64 (W = tau for the EP quantities); every dtheta entry within kern_ld.grad_tol = max(32 e64, 256 eps64 cond), cond = the
sum of the absolute terms of that entry.  Every case keeps kappa <= 1e4, so the kappa term stays at or below 6e-10.  Judged per
case: a, K a, log det B (newton); diag(Ki_W_i), log det B (finish); K, K_Wi_i and dL_dK (fetched; each bitwise symmetric);
dtheta; s (implicit; the same bytes before and after gradients); mu, var and cov at 1 and at 129 new points; mu, diag(Sigma) of
ep_recompute with want_sigma on and off (the same bytes of mu) and log det B; the swept tau, v, cavity tau and v, log Z_hat, mu
and diag(Sigma); and a second ep_recompute on the swept sites, which must give the swept mu and diag(Sigma) again (a rank-one
update that drifts from Sigma(tau) shows there).

Families (laplace_ld.CASES), one module-scoped context each, in list order:
    n_edge     RBF-ARD + Bias, D = 3: N = 1 | 2 | 63 | 64 | 65 | 127 | 128 | 129 | 255 | 256 | 257 | 512 | 513; N = 1025 with
               vectors only (newton, diag and log det of finish, implicit, prediction, recompute without Sigma)
    weights    RBF iso, D = 2, N = 129 | 257: W with 10 % exact zeros; W = 1e-6 on half the sites and up to 50 on the rest; tau
               with exact zeros; the cold start tau = v = 0 with add_diag = 1e-7; well-separated classes with |z| > 8 on both
               sides and the clamp of tau at eps64
    kernels    N = 129 (Coregionalize with P = 3: N = 65): RBF-ARD at D = 32 | 33, Matern32-ARD on a subset of the columns,
               StdPeriodic-ARD, RatQuad-ARD, Linear + Bias, MLP x RBF, Poly of order 3, RBF x Coregionalize of rank 1 | 2
    points     N = 129, M = 1 | 127 | 128 | 129 | 257 new points, diagonal and full_cov, RBF + Bias and Linear + Bias
    stale      one context, no fresh one between the steps: N = 257; set_data at N = 129; set_targets and a product; the first
               part list again; the same after an exact_inference_sum on the context
    schedules  N = 129 | 257 | 513 of n_edge in a fresh child process with MI355GP_PERSIST=0: judged alike, and the bytes of a,
               diag(Ki_W_i), the predicted mean and the EP mu equal this process's

One case needed a fix: the fetched woodbury_inv K_Wi_i (MI355GP_FETCH_KINV) was not bitwise symmetric, at every N of the sweep
from 63 up and with every kernel and W.  `k_lap_extract_kwi` (csrc/laplace.hip) reads the lower tiles of B^-1 on both sides of
the diagonal but multiplied sw_i B^-1 sw_j from the left in either case, so (i, j) got (sw_i x) sw_j and (j, i) got (sw_j x) sw_i,
which differ in the last bit; the accuracy was never in question (3e-15 before and after).  It now takes the two products in the
order of the lower triangle on both sides, which is also the order `k_laplace_dLdK` uses.  Every other case passed as the code
stood.

Teeth, checked once on a copy of the sources and not kept: `k_symv_finish` starting its column sum at cj + 1 for the last
chunk fails n_edge at N = 2, 63, 64, 127, 128, 255 and 256 (a, K a, dL_dK, s, the EP mu: 0.2 ... 80 against bounds of 1e-12;
at N = 1, 65, 129 and 257 the last chunk is one row and has nothing below its diagonal); `k_laplace_dLdK` without the
`diag &&` of its mirror fails it at every N from 65 up (dL_dK 0.73 against 2.2e-12 at N = 129, and not symmetric).

Measured on an MI355X: the worst err(q) per family and quantity -- a record, never a reason to tighten a bound (logdet = the three
log det B; mu* / var* / cov* = the prediction at every M of the family; ep_mu / ep_sd with want_sigma on and off; sweep = the
worst of the seven swept vectors; again = the second recompute; dtheta = the worst entry in units of its own bound;
err/bound = the worst ratio of a figure to its bound over the family):

    family           a      Ka  logdet    diag       K  K_Wi_i   dL_dK       s     mu*    var*    cov*   ep_mu   ep_sd   sweep   again  dtheta  err/bound
    n_edge       4e-14   2e-14   2e-15   4e-15   3e-16   3e-15   8e-16   9e-15   2e-15   1e-14   3e-14   6e-15   3e-15   4e-14   7e-15  0.0042      0.021
    weights      2e-13   9e-14   3e-15   1e-14   2e-16   2e-14   2e-14   7e-14   1e-15   7e-14   1e-13   1e-15   1e-15   2e-13   9e-15  0.0007      0.040
    kernels      6e-14   5e-14   1e-15   2e-14   5e-16   4e-15   4e-15   3e-14   1e-14   8e-14   3e-14       -       -       -       -  0.0011      0.009
    points       1e-14   4e-15   5e-16   1e-14   2e-16   2e-15   6e-16   1e-14   5e-16   1e-14   3e-14       -       -       -       -  0.0001      0.009
    stale        6e-15   8e-15   7e-16   1e-15   4e-16   2e-15   5e-16   4e-15   1e-15   2e-15   5e-15   2e-15   2e-15   2e-14   6e-15  0.0002      0.011
    schedules    1e-14   9e-15   4e-16   3e-15   3e-16   3e-15   8e-16   6e-15   1e-15   1e-15   3e-15   4e-15   3e-15   4e-14   4e-15  0.0001      0.012

kappa runs from 1 to 1041 (W up to 50 at N = 257), the bounds from 5.7e-14 to 9.0e-11.  The whole file: 38 tests (44 cases), 27 s
of wall time, nearly all of it the long-double references (N = 1025: 10 s, N = 512 and 513: 4 s each; the device calls of a case
take 0.04 s at most, the child process of `schedules` 1.1 s).
"""
import os
import signal
import subprocess
import sys
import time

import numpy as np
import pytest

from gpy_amd import _lib as L

import kern_ld as KL
import laplace_ld as LL

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not KL.HAVE_LD, reason="np.longdouble is not an extended format on this host")]
LIMIT_S = 240                         # the slowest case is N = 513 or N = 1025: about 20 s of long-double reference
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(autouse=True)
def _time_limit():
    def stop(signum, frame):
        raise TimeoutError("test exceeded its %d s limit" % LIMIT_S)
    old = signal.signal(signal.SIGALRM, stop)
    signal.alarm(LIMIT_S)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


@pytest.fixture(scope="module")
def ctxs():
    """one context per family, made when the family's first case runs"""
    held = {}
    yield held
    for c in held.values():
        c.close()


def family_ctx(ctxs, family):
    if family not in ctxs:
        ctxs[family] = L.Context(0)
    return ctxs[family]


def evaluate(ctx, c, action="set_data"):
    """every device call of a case: ({quantity: value}, [what a structural assertion found])"""
    specs, full = c["dev_specs"], c["full"]
    got, bad = {}, []
    if action == "set_data":
        ctx.set_data(c["X"], c["Y"])
    elif action == "set_targets":
        ctx.set_targets(c["Y"])
    elif action == "exact_inference_sum":
        rc, _ = ctx.exact_inference_sum(specs, 0.1, want_diag=True)
        assert rc == 0
    ctx.laplace_begin(specs)
    if c["laplace"]:
        if full:
            got["K"] = ctx.fetch(L.FETCH_K)
        info, got["a"], got["Ka"], got["logdet_newton"] = ctx.laplace_newton(c["W"], c["b"])
        assert info == 0
        info, got["diag"], got["logdet_finish"] = ctx.laplace_finish(c["W"])
        assert info == 0
        got["s"] = ctx.laplace_implicit(c["dL_dfhat"])
        if full:
            got["K_Wi_i"] = ctx.fetch(L.FETCH_KINV)
            got["dtheta"] = KL.chain_coreg(c["specs"], ctx.laplace_gradients(c["Ki_f"], c["dL_dfhat"]))
            got["dL_dK"] = ctx.fetch(L.FETCH_DLDK)
            if ctx.laplace_implicit(c["dL_dfhat"]).tobytes() != got["s"].tobytes():
                bad.append("the implicit vector changed with a resident dL_dK")
            if ctx.fetch(L.FETCH_KINV).tobytes() != got["K_Wi_i"].tobytes():
                bad.append("K_Wi_i changed with a resident dL_dK")
            for q in LL.SYMMETRIC:
                if not np.array_equal(got[q], got[q].T):
                    bad.append("%s is not bitwise symmetric" % q)
        for M in c["Ms"]:
            Xs = c["Xs%d" % M]
            got["mu%d" % M], got["var%d" % M] = ctx.laplace_predict(specs, Xs, c["Ki_f"])
            mu, got["cov%d" % M] = ctx.laplace_predict(specs, Xs, c["Ki_f"], full_cov=True)
            if mu.tobytes() != got["mu%d" % M].tobytes():
                bad.append("mu%d differs between the diagonal and the full_cov call" % M)
    if c["ep"]:
        tau, v, add = c["tau"], c["v"], c["add_diag"]
        info, got["ep_mu_diag_only"], got["ep_sd_diag_only"], got["ep_logdet"] = ctx.ep_recompute(tau, v, add_diag=add, want_sigma=False)
        assert info == 0
        if full:
            info, got["ep_mu"], got["ep_sd"], ld = ctx.ep_recompute(tau, v, add_diag=add, want_sigma=True)
            assert info == 0
            if got["ep_mu"].tobytes() != got["ep_mu_diag_only"].tobytes() or ld != got["ep_logdet"]:
                bad.append("ep_recompute with and without want_sigma disagree on mu or log det B")
            r = ctx.ep_sweep(c["order"], c["ysign"], tau, v, c["eta"], c["delta"])
            for q in LL.SWEEP_KEYS:
                got["sw_" + q] = r[q]
            if LL.judged_again(c):
                info, got["again_mu"], got["again_sd"], _ = ctx.ep_recompute(r["tau"], r["v"], want_sigma=True)
                assert info == 0
    return got, bad


def _report(name, c, got, bad0, kappa, ref, r64, t_ref, t_dev):
    figs, bad = LL.judge(c, got, ref, r64, kappa)
    print()
    print("%-36s kappa %s  ref %.1f s dev %.2f s  " % (name, "/".join("%.0f" % kappa[k] for k in sorted(kappa)), t_ref, t_dev)
          + "  ".join("%s %.1e/%.1e" % (q, e, b) for q, (e, b) in figs.items()))
    assert all(k <= 1e4 for k in kappa.values()), kappa
    assert not bad0, bad0
    assert not bad, bad
    assert set(figs) == set(LL.judged(c)) | ({"dtheta"} if c["laplace"] and c["full"] else set())
    return figs


def _check(ctxs, name, action="set_data"):
    t0 = time.time()
    c, ref, r64, kappa = LL.reference(name)
    t1 = time.time()
    try:
        got, bad0 = evaluate(family_ctx(ctxs, c["family"]), c, action)
    except L.MI355GPError as e:          # nothing more on this device after an error of the runtime
        pytest.exit("device error in %s, the sweep ends here: %s" % (name, e), returncode=3)
    return _report(name, c, got, bad0, kappa, ref, r64, t1 - t0, time.time() - t1)


@pytest.mark.parametrize("name", LL.NAMES["n_edge"])
def test_n_edge(name, ctxs):
    _check(ctxs, name)


@pytest.mark.parametrize("name", LL.NAMES["weights"])
def test_weights(name, ctxs):
    _check(ctxs, name)
    if name.endswith("separated"):
        ref = LL.reference(name)[1]
        assert ref["sw_z"].min() < -8 and ref["sw_z"].max() > 8 and ref["sw_clamped"]


@pytest.mark.parametrize("name", LL.NAMES["kernels"])
def test_kernels(name, ctxs):
    _check(ctxs, name)


@pytest.mark.parametrize("name", LL.NAMES["points"])
def test_points(name, ctxs):
    _check(ctxs, name)


def test_stale_state_of_one_context(ctxs):
    """the steps in order on one context; every step is judged, a failing one does not hide the later ones"""
    failed = []
    for name in LL.NAMES["stale"]:
        try:
            _check(ctxs, name, LL.BY_NAME[name]["action"])
        except AssertionError as e:
            failed.append("%s: %s" % (name, e))
    assert not failed, failed


def child(names, path):
    """the device's quantities of some cases, written to an .npz (what the child process of the schedules test runs)"""
    ctx = L.Context(0)
    out = {}
    for name in names:
        got, bad = evaluate(ctx, LL.make_case(name))
        assert not bad, bad
        for q, val in got.items():
            out[name + "/" + q] = np.asarray(val)
    np.savez(path, **out)


def test_schedules_without_the_persistent_launch(tmp_path):
    """the session's factorisation takes its schedule from the process default (MI355GP_PERSIST): a fresh child process with the
    persistent launch switched off is judged against the same references, and returns the bytes of a, diag(Ki_W_i) and the EP
    mu that this process gets with it on"""
    path = str(tmp_path / "child.npz")
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_laplace_shapes as T; T.child(%r, %r)"
            % (HERE, os.path.dirname(HERE), LL.SCHEDULES, path))
    t0 = time.time()
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MI355GP_PERSIST="0"), capture_output=True, text=True,
                       timeout=180)
    assert r.returncode == 0, r.stderr
    t_child = time.time() - t0
    z = np.load(path)
    ctx = L.Context(0)
    try:
        for name in LL.SCHEDULES:
            t0 = time.time()
            c, ref, r64, kappa = LL.reference(name)
            t1 = time.time()
            got = dict((k.split("/", 1)[1], z[k] if z[k].ndim else z[k].item()) for k in z.files if k.startswith(name + "/"))
            _report(name + " (child)", c, got, [], kappa, ref, r64, t1 - t0, t_child)
            here, bad = evaluate(ctx, c)
            assert not bad, bad
            for q in ("a", "diag", "mu129", "ep_mu"):
                assert np.asarray(got[q]).tobytes() == here[q].tobytes(), (name, q)
    finally:
        ctx.close()
