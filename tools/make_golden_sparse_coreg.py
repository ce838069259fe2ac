"""Fixtures tests/golden/sparse_coreg/*.npz FROM THE REFERENCE'S OWN CODE for multi-output kernels on the sparse path (what
GPy/models/sparse_gp_coregionalized_regression.py evaluates): `VarDTC.inference` (GPy/inference/latent_function_inference/
var_dtc.py) with per-point noise variances -- one per output, as MixedNoise hands them over -- the kernels'
`update_gradients_diag` / `update_gradients_full` / `gradients_X` assembled as GPy/core/sparse_gp.py:108-119 does for certain
inputs, and `Posterior._raw_predict` at 7 new points with `full_cov` both ways, executed through oracle/ref_loader.py (imported,
unchanged).  Only data goes into the fixtures.

Inputs: per output its own inducing inputs on a jittered regular grid over the spatial columns (lengthscales 0.75 grid
spacings, the unit cube centred at the origin), an index column that says which output a row or an inducing input belongs to,
N <= 60, M <= 12.  A fixture is REFUSED when cond2(Kmm + 1e-8 I) exceeds 1e3, and when the run would have entered jitchol's
ladder: `jitchol` is replaced by a plain Cholesky factorisation for the run, which raises instead of adding jitter.

    python tools/make_golden_sparse_coreg.py
"""
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import ref_loader  # noqa: E402
import make_golden_sparse_lin as GL  # noqa: E402
import make_golden_svgp as GS  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "sparse_coreg")
COND_CAP = 1e3
MAX_BYTES = 1 << 20
GS.NAMES["Coregionalize"] = ("W", "kappa")
_leaf, _assemble = GS.leaf, GS.assemble


def leaf(ns, spec):
    kind, ard, th, dims, _ = spec
    if kind == "coregionalize":                    # (kind, 100 rank + P, [W.ravel(), kappa], [index column], term)
        P, rank = ard % 100, ard // 100
        th = np.asarray(th, dtype=float)
        return ns.Coregionalize(1, P, rank=rank, W=th[:P * rank].reshape(P, rank), kappa=th[P * rank:], active_dims=dims, name="B")
    return _leaf(ns, spec)


def assemble(ns, specs):
    top, leaves = _assemble(ns, specs)
    for k in leaves:
        if type(k).__name__ == "Coregionalize":
            k.parameters_changed()                 # B = W W^T + diag(kappa) on the copies that evaluate
    return top, leaves


GS.leaf, GS.assemble = leaf, assemble


def indices(n, P, order):
    """sorted runs as build_XY stacks them, or n mod P shuffled ("unsorted")"""
    idx = np.sort(np.arange(n) % P)
    return idx if order == "sorted" else np.random.default_rng(n).permutation(np.arange(n) % P)


def coreg(P, col, rank, term, rng):
    W = 0.4 * rng.uniform(0.5, 1.0, (P, rank)) * np.where(rng.uniform(size=(P, rank)) < 0.3, -1.0, 1.0) / np.sqrt(rank)
    return ("coregionalize", 100 * rank + P, list(W.ravel()) + list(0.6 + 0.2 * rng.uniform(size=P)), [col], term)


def inputs(N, M, D, P, kern, order, seed):
    """D columns, the last one the output index"""
    rng = np.random.default_rng(seed)
    col, sp = D - 1, list(range(D - 1))
    X = rng.uniform(-0.5, 0.5, (N, D))
    X[:, col] = indices(N, P, order)
    Z = rng.uniform(-0.5, 0.5, (M, D))
    zi = indices(M, P, "sorted")
    Z[:, col] = zi
    g = 1
    for p in range(P):
        mp_ = int(np.sum(zi == p))
        Zp, gp = GS.grid_Z(mp_, len(sp), sp, rng)
        Z[zi == p, :col] = Zp - 0.5
        g = max(g, gp)

    def st(kind, ard, var, term):
        v = np.array([0.75 / g * rng.uniform(0.9, 1.1) for q in sp])
        return (kind, int(ard), [var] + list(v if ard else v[:1]), sp, term)
    allq = list(range(D))
    if kern == "icm_rbf":
        specs = [st("rbf", 1, 1.3, 1), coreg(P, col, 1, 1, rng)]
    elif kern == "icm_matern32":
        specs = [st("matern32", 0, 1.1, 1), coreg(P, col, 1, 1, rng)]
    elif kern == "lcm2":
        specs = [st("rbf", 1, 1.3, 1), coreg(P, col, 1, 1, rng), st("matern32", 0, 0.7, 2), coreg(P, col, 1, 2, rng)]
    elif kern == "icm+bias":
        specs = [st("rbf", 1, 1.3, 1), coreg(P, col, 1, 1, rng), ("bias", 0, [0.2], allq, 0)]
    elif kern == "coreg*bias":                     # no stationary factor: Kmm is 0.7 B for one inducing input per output
        specs = [coreg(P, col, 1, 1, rng), ("bias", 0, [0.7], allq, 1)]
    else:
        assert kern == "icm_rbf_rank2"
        specs = [st("rbf", 1, 1.3, 1), coreg(P, col, 2, 1, rng)]
    idx = X[:, col].astype(int)
    w = rng.uniform(1.0, 3.0, (len(sp), 1))
    Y = np.sin(2.0 * np.pi * X[:, :col] @ w / len(sp) + 0.7 * idx[:, None]) + 0.2 * rng.standard_normal((N, 1))
    Xs = rng.uniform(-0.5, 0.5, (7, D))
    Xs[:, col] = rng.integers(0, P, 7)
    noise_out = 0.03 + 0.02 * np.arange(P)
    return specs, X, Y, Z, Xs, noise_out, col


def save(ns, name, specs, arrays, **meta):
    k, _ = GS.assemble(ns, specs)
    Z = meta["Z"]
    kappa = float(np.linalg.cond(np.asarray(k.K(Z)) + 1e-8 * np.eye(Z.shape[0])))
    assert kappa <= COND_CAP, "%s refused: cond2(Kmm + 1e-8 I) = %.3g exceeds %g" % (name, kappa, COND_CAP)
    spec_json = json.dumps([[s[0], int(s[1]), [float(v) for v in s[2]], [int(d) for d in s[3]], int(s[4])] for s in specs])
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, specs=spec_json, cond_Kmm=kappa, **dict(arrays, **meta))
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, "%s: %d bytes is past the cap for a committed file" % (name, size)
    print("%-44s cond(Kmm + 1e-8 I) %.1f  %d bytes" % (name, kappa, size))


def main():
    ns = ref_loader.load_sum_kernels(ref_loader.load())
    ns.Linear = importlib.import_module("GPy.kern.src.linear").Linear
    ns.Coregionalize = importlib.import_module("GPy.kern.src.coregionalize").Coregionalize
    mod = importlib.import_module("GPy.inference.latent_function_inference.var_dtc")
    ns.VarDTC = mod.VarDTC
    mod.jitchol = GL.strict_jitchol                # a run that would have added jitter raises instead
    os.makedirs(OUT, exist_ok=True)
    for name, kern, N, M, D, P, order, seed in (("icm_rbf_p2_n50_m10_d2", "icm_rbf", 50, 10, 2, 2, "sorted", 1),
                                                ("icm_rbf_p3_n60_m12_d3", "icm_rbf", 60, 12, 3, 3, "sorted", 2),
                                                ("icm_matern32_p2_n56_m10_d2", "icm_matern32", 56, 10, 2, 2, "sorted", 3),
                                                ("lcm2_p2_n60_m12_d3", "lcm2", 60, 12, 3, 2, "sorted", 4),
                                                ("icm_bias_p2_n48_m10_d2", "icm+bias", 48, 10, 2, 2, "sorted", 5),
                                                ("coreg_x_bias_p3_n45_m3_d2", "coreg*bias", 45, 3, 2, 3, "sorted", 6),
                                                ("icm_rbf_rank2_p3_n60_m12_d2", "icm_rbf_rank2", 60, 12, 2, 3, "sorted", 7),
                                                ("icm_rbf_unsorted_p3_n57_m12_d3", "icm_rbf", 57, 12, 3, 3, "unsorted", 8)):
        specs, X, Y, Z, Xs, noise_out, col = inputs(N, M, D, P, kern, order, seed)
        idx = X[:, col].astype(int)
        noise = noise_out[idx]
        r = GL.vardtc(ns, specs, noise, X, Y, Z, Xs)
        dL_dR = np.asarray(r["dL_dthetaL"], float).reshape(N, -1).sum(axis=1)     # per point; MixedNoise sums them per output
        r["dL_dthetaL"] = np.array([dL_dR[idx == p].sum() for p in range(P)])
        save(ns, name, specs, r, family="vardtc", X=X, Y=Y, Z=Z, Xs=Xs, noise=noise, noise_out=noise_out, P=P, idx_col=col)


if __name__ == "__main__":
    main()
