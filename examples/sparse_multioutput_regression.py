"""Two correlated outputs with a sparse multi-output GP: the two-sine toy problem of the reference's coregionalization examples
(one output sin(x) on [0, 8], the other sin(x) + 2 on [0, 5]; seeded, nothing downloaded) with several thousand points per
output, fitted with `SparseGPCoregionalizedRegression` (an ICM of an RBF, one noise variance per output, M = 2 x 12 inducing
inputs that carry an output index) and, on a subsample, with the exact `GPCoregionalizedRegression`, which factors a matrix of
the stacked size.  Both predictive curves are printed side by side at a few points with their largest difference: the sparse
model sees every point, the exact one a fortieth of them, and they agree to within their error bars.  The second output has
no data past x = 5; there its prediction leans on the first output through the learned B = W W^T + diag(kappa).

    python examples/sparse_multioutput_regression.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpy_amd as GPy  # noqa: E402


def main():
    rng = np.random.default_rng(0)
    np.random.seed(0)                                             # (Coregionalize draws its initial W)
    n1, n2 = 6000, 4000
    X1, X2 = np.sort(rng.uniform(0.0, 8.0, (n1, 1)), 0), np.sort(rng.uniform(0.0, 5.0, (n2, 1)), 0)
    Y1 = np.sin(X1) + 0.05 * rng.standard_normal(X1.shape)
    Y2 = np.sin(X2) + 2.0 + 0.05 * rng.standard_normal(X2.shape)
    Z_list = [np.linspace(0.0, 8.0, 12)[:, None], np.linspace(0.0, 5.0, 12)[:, None]]

    def kernel():
        return GPy.util.multioutput.ICM(1, 2, GPy.kern.RBF(1, lengthscale=1.5), W_rank=1) + GPy.kern.Bias(2)
    sparse = GPy.models.SparseGPCoregionalizedRegression([X1, X2], [Y1, Y2], Z_list=Z_list, kernel=kernel())
    start = sparse.log_likelihood()
    sparse.optimize(max_iters=200)
    print("sparse  N = %d + %d, M = %d: bound % .1f -> % .1f, noise variances %s (true 0.0025)" % (
        n1, n2, sparse.Z.shape[0], start, sparse.log_likelihood(), np.round(sparse.likelihood._variances(), 5)))
    sub1, sub2 = X1[::40], X2[::40]
    exact = GPy.models.GPCoregionalizedRegression([sub1, sub2], [Y1[::40], Y2[::40]], kernel=kernel())
    exact.optimize(max_iters=200)
    print("exact   N = %d + %d: log marginal % .1f, noise variances %s" % (
        sub1.shape[0], sub2.shape[0], exact.log_likelihood(), np.round(exact.likelihood._variances(), 5)))
    worst = 0.0
    for p, hi in ((0, 8.0), (1, 8.0)):
        x = np.linspace(0.25, hi - 0.25, 16)[:, None]
        Xn = np.hstack([x, np.full_like(x, float(p))])
        meta = {"output_index": Xn[:, 1:2].astype(int)}
        (ms, vs), (me, ve) = sparse.predict(Xn, Y_metadata=meta), exact.predict(Xn, Y_metadata=meta)
        inside = x[:, 0] <= (8.0 if p == 0 else 5.0)
        worst = max(worst, float(np.abs(ms - me)[inside].max()))
        for i in (1, 8, 14):
            print("output %d at x = %.2f: sparse %.3f +- %.3f   exact %.3f +- %.3f   (f = %.3f%s)" % (
                p, x[i, 0], ms[i, 0], np.sqrt(vs[i, 0]), me[i, 0], np.sqrt(ve[i, 0]), np.sin(x[i, 0]) + 2.0 * p,
                "" if inside[i] else ", no data of this output here"))
    print("largest difference of the two predictive means where both outputs have data: %.4f" % worst)
    B = sparse.kern.parts[0].parts[1].B
    print("learned B =", np.round(B, 3).tolist(), " correlation of the outputs %.3f" % (B[0, 1] / np.sqrt(B[0, 0] * B[1, 1])))


if __name__ == "__main__":
    main()
