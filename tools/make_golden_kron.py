"""Fixtures tests/golden/kron/*.npz FROM THE REFERENCE'S OWN CODE: `GaussianGridInference.inference`
(GPy/inference/latent_function_inference/gaussian_grid_inference.py) with the reference's RBF / GridRBF and Gaussian likelihood,
executed through oracle/ref_loader.py (imported, unchanged).  Only data goes into the fixtures.

`GPy.core.gp_grid` does not import under the loader, so the prediction of a fixture is composed from the reference's RBF `K`, the
reference's `kron_mvprod` (column by column, as `GpGrid.kron_mmprod` loops) and the algebra of `GpGrid._raw_predict`
(gp_grid.py:87-116), with its noise convention: the likelihood variance WITHOUT the 1e-8 that inference adds.

Coordinates are integer-valued.  A fixture is REFUSED, not written, when `list(set(X[:, d]))` is not ascending in some column (the
reference would then permute the grid), or when the reference's log marginal differs from that of its own dense
`ExactGaussianInference` on the same data by more than 1e-13 relative (the golden tolerance of the exact path).

Each fixture holds X, Y, Xs, the parameters, the reference's eigenvectors and eigenvalues as `np.linalg.eig` returned them, alpha,
V_kron, the log marginal, dL_dLen, dL_dVar, dL_dthetaL and the latent prediction at 13 new points, 4 of them on the grid.

    python tools/make_golden_kron.py
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "kron")
LML_TOL = 1e-13


def grid_of(xg):
    return np.array(np.meshgrid(*xg, indexing="ij")).reshape(len(xg), -1).T.copy()


def case(ns, name, xg, variance, ls, ARD, noise, seed):
    rng = np.random.default_rng(seed)
    xg = [np.asarray(x, float) for x in xg]
    for d, x in enumerate(xg):
        if list(set(x)) != sorted(x):
            raise RuntimeError("%s REFUSED: list(set(...)) of column %d is %r, not ascending" % (name, d, list(set(x))))
    X = grid_of(xg)
    N, D = X.shape
    Y = np.sin(X.sum(1) / (1.0 + 0.5 * D))[:, None] + 0.3 * rng.standard_normal((N, 1))
    k = ns.RBF(D, variance=variance, lengthscale=ls, ARD=ARD)
    lik = ns.Gaussian(variance=noise)
    inf = ns.GaussianGridInference()
    post, lml, gd = inf.inference(k, X, lik, Y)
    lml = float(np.real(np.asarray(lml)).item())
    _, lml_dense, _ = ns.ExactGaussianInference().inference(ns.RBF(D, variance=variance, lengthscale=ls, ARD=ARD), X,
                                                            ns.Gaussian(variance=noise), Y)
    lml_dense = float(lml_dense)
    if abs(lml - lml_dense) > LML_TOL * abs(lml_dense):
        raise RuntimeError("%s REFUSED: grid log marginal %.15e, dense %.15e, relative %.2e" % (
            name, lml, lml_dense, abs(lml - lml_dense) / abs(lml_dense)))
    Qs = [np.real(np.asarray(Q, float)) for Q in post.Qs]
    QTs = [Q.T.copy() for Q in Qs]
    V = np.real(np.asarray(post.V_kron, float)).reshape(-1)
    alpha = np.real(np.asarray(post.alpha, float)).reshape(-1, 1)
    # the eigenvalues per dimension, as np.linalg.eig gave them (V_kron is their Kronecker product)
    oneD = k.get_one_dimensional_kernel(D)
    lams = []
    for d in range(D):
        oneD.lengthscale = k.lengthscale[d]
        lams.append(np.real(np.linalg.eig(oneD.K(xg[d][:, None]))[0]).astype(float))
    Vk = np.ones(1)
    for lam in lams:
        Vk = np.kron(Vk, lam)
    assert np.array_equal(Vk, V), "np.linalg.eig is not repeatable"
    # prediction (gp_grid.py:87-116): 9 points inside the grid's box, 4 on the grid
    lo, hi = X.min(0), X.max(0)
    Xs = np.vstack([lo + (hi - lo) * rng.random((9, D)), X[rng.choice(N, 4, replace=False)]])
    Kmn = np.asarray(k.K(Xs, X), float)
    mu = np.dot(Kmn, alpha).reshape(-1, 1)
    cols = [inf.kron_mvprod(QTs, c.reshape(-1, 1)) for c in Kmn]
    A = np.column_stack(cols) / (V.reshape(-1, 1) + float(np.asarray(lik.variance).ravel()[0]))
    A = np.column_stack([inf.kron_mvprod(Qs, c.reshape(-1, 1)) for c in A.T])
    var = np.diag(np.asarray(k.K(Xs), float) - np.dot(Kmn, A)).copy().reshape(-1, 1)
    path = os.path.join(OUT, name + ".npz")
    arrays = dict(X=X, Y=Y, Xs=Xs, variance=float(variance), lengthscale=np.atleast_1d(np.asarray(ls, float)), ARD=int(ARD),
                  noise=float(noise), G=np.array([x.size for x in xg], dtype=np.int64), alpha=alpha, V_kron=V, lml=lml,
                  lml_dense=lml_dense, dL_dLen=np.asarray(gd["dL_dLen"], float).ravel(), dL_dVar=float(gd["dL_dVar"]),
                  dL_dthetaL=float(gd["dL_dthetaL"]), pred_mu=mu, pred_var=var)
    for d in range(D):
        arrays["Q%d" % d] = Qs[d]
        arrays["lam%d" % d] = lams[d]
    np.savez_compressed(path, **arrays)
    print("%-22s N %4d  lml % .12e  |grid - dense| / |dense| %.1e  %d bytes" % (
        name, N, lml, abs(lml - lml_dense) / abs(lml_dense), os.path.getsize(path)))


def main():
    ns = ref_loader.load()
    ns.GaussianGridInference = importlib.import_module(
        "GPy.inference.latent_function_inference.gaussian_grid_inference").GaussianGridInference
    os.makedirs(OUT, exist_ok=True)
    r = lambda n, start=0: np.arange(start, start + n, dtype=float)          # noqa: E731
    case(ns, "d1_g9_iso", [r(9)], 1.3, 1.7, False, 0.1, 1)
    case(ns, "d2_6x5_ard", [r(6), r(5, 2)], 1.5, [1.4, 2.1], True, 0.12, 2)
    case(ns, "d3_5x4x3_ard", [r(5), r(4), r(3)], 1.2, [1.6, 1.1, 2.0], True, 0.15, 3)
    case(ns, "d4_3x2x3x2_ard", [r(3), r(2), r(3, 1), r(2)], 0.9, [1.2, 0.9, 1.5, 1.1], True, 0.1, 4)
    case(ns, "d3_4x1x3_ard", [r(4), np.array([2.0]), r(3)], 1.1, [1.3, 1.0, 1.8], True, 0.08, 5)
    case(ns, "d2_7x3_ard_unequal", [r(7), r(3)], 2.0, [0.6, 4.0], True, 0.2, 6)


if __name__ == "__main__":
    main()
