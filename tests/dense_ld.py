"""Judges of the fp64 tile-GEMM launchers (gpy_amd/csrc/gemm.hip) and of the dense chain potrf -> L^-1 -> A^-1 built on them,
shared by tests/test_gpu_tileops.py, tests/test_gpu_dense_ld.py (GPU) and tests/test_oracle_tileops.py (CPU: the judges accept
the numpy / LAPACK result of every case and reject a set of planted faults).

PART A -- one launcher alone.  Every case is a list of PIECES; a piece says what part of the output buffer is

    out[mask] = alpha * (A @ B) + beta * C0            A (M x K), B (K x N): dense, structural zeros written out,

on which 128-tiles (`mask`), and which k range [klo, khi) the kernel walks for each tile.  Three judgements:

  A1 exact      operands are integers in [-4, 4], alpha / beta powers of two, K <= 3072: every partial sum is an integer (or a
                half) below 2^53, so ANY accumulation order, fused or not, is exact -- and so is numpy's fp64 BLAS product of the
                same integers, which therefore IS the int64 result (test_oracle_tileops.py holds it against an int64 product).
                The device must match it under np.array_equal.  No tolerance.
  A2 rounding   operands standard normal, rows scaled by 10^U(-3, 3).  An output element is a chain of K fused multiply-adds:
                |out - exact| <= gamma_K mag, gamma_K = K u / (1 - K u), u = 2^-53, mag = |A| @ |B| (Higham, Accuracy and
                Stability, eq. 3.5; each fma rounds once).  Epilogue and partial sums: gamma_{K + S + 3} (S partial sums) on
                |alpha| mag + |beta| |C0|.  K is the length of the k range of the element's OWN tile.
                  all elements  against numpy's fp64 BLAS result at TWICE the bound (both sides carry one gamma);
                  sample        rows and columns {0, 15, 16, 63, 64, 127} of every 128-tile (first / last, the wave boundary, an
                                MFMA block boundary), full width / height, against long double at the bound itself.  mag is
                                taken in fp64 (relative error gamma_K of the bound: immaterial).
  A3 poison     tiles an operand must not be read from hold NaN (strictly above the diagonal of a triangular operand; C when
                beta == 0; an output that is overwritten starts as NaN too, so an unwritten element shows); output tiles outside
                every mask hold known values and must come back with the same BITS; no NaN inside a mask.

PART B -- the dense chain, each stage against the device's own input to it (chol_figures, inv_figures, ...): see the functions.

The long-double parts need an extended `np.longdouble` (kern_ld.HAVE_LD); everything else runs everywhere."""
import numpy as np

from kern_ld import HAVE_LD, LD

U = 2.0 ** -53
NB = 128
SAMPLE = (0, 15, 16, 63, 64, 127)
THIN = (0, 127)
LD_FLOP_BUDGET = 6.0e8          # long-double multiply-adds of one case's sample (about 2.5e8 / s here) before it is thinned to THIN


def gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1.0 - k * U)


def sample_index(n, local=SAMPLE):
    """rows (or columns) `local` of every 128-tile of a dimension n; a ragged last tile contributes what it has, and n - 1"""
    idx = sorted({t * NB + r for t in range((n + NB - 1) // NB) for r in local if t * NB + r < n} | {n - 1})
    return np.array(idx, dtype=np.intp)


# ---------------------------------------------------------------------------------------------------------------------
# operands
def draw(kind, rng, shape):
    """'int': integers uniform in [-4, 4] as doubles; 'real': standard normal with every row scaled by 10^U(-3, 3)"""
    if kind == "int":
        return rng.integers(-4, 5, size=shape).astype(np.float64)
    return rng.standard_normal(shape) * 10.0 ** rng.uniform(-3.0, 3.0, size=(shape[0],) + (1,) * (len(shape) - 1))


def lower_with_poison(kind, rng, n):
    """(X as the device gets it, X as mathematics sees it): lower triangular n x n; stored zeros above the diagonal inside the
    diagonal tiles (the kernels read whole tiles), NaN in every tile strictly above the diagonal"""
    X0 = np.tril(draw(kind, rng, (n, n)))
    X = X0.copy()
    for ti in range(n // NB):
        X[ti * NB:(ti + 1) * NB, (ti + 1) * NB:] = np.nan
    return X, X0


def tile_mask(mt, ntl, keep):
    m = np.zeros((mt * NB, ntl * NB), dtype=bool)
    for ti in range(mt):
        for tj in range(ntl):
            if keep(ti, tj):
                m[ti * NB:(ti + 1) * NB, tj * NB:(tj + 1) * NB] = True
    return m


def prefill(rng, mask, computed):
    """what an output buffer holds before the launch: `computed` (an array, or NaN) on the mask, known values elsewhere"""
    out = rng.standard_normal(mask.shape) + 3.0
    out[mask] = np.nan if computed is None else computed[mask]
    return out


class Piece:
    """out[sel][mask] = alpha * A @ B + beta * C0; tile (ti, tj) walks k in [klo[ti, tj], khi[ti, tj]); S partial sums"""

    def __init__(self, sel, A, B, alpha, beta, C0, mask, klo, khi, S=None):
        self.sel, self.A, self.B, self.alpha, self.beta, self.mask = sel, A, B, float(alpha), float(beta), mask
        self.C0 = np.zeros(mask.shape) if (C0 is None or beta == 0.0) else np.where(mask, C0, 0.0)
        mt, ntl = mask.shape[0] // NB, mask.shape[1] // NB
        self.klo = np.broadcast_to(np.asarray(klo), (mt, ntl)).copy()
        self.khi = np.broadcast_to(np.asarray(khi), (mt, ntl)).copy()
        self.S = np.zeros((mt, ntl), dtype=int) if S is None else np.broadcast_to(np.asarray(S), (mt, ntl)).copy()
        assert A.shape[0] == mask.shape[0] and B.shape[1] == mask.shape[1] and A.shape[1] == B.shape[0]
        assert not np.isnan(A).any() and not np.isnan(B).any() and not np.isnan(self.C0).any()

    def tiles(self):
        return [(ti, tj) for ti in range(self.klo.shape[0]) for tj in range(self.klo.shape[1]) if self.mask[ti * NB, tj * NB]]

    def tile(self, ti, tj, k0=None, k1=None, A=None, arows=None):
        """fp64 value of one output tile from the k range [k0, k1) (default: its own), optionally from other A rows"""
        k0 = self.klo[ti, tj] if k0 is None else k0
        k1 = self.khi[ti, tj] if k1 is None else k1
        A = self.A if A is None else A
        ar = ti if arows is None else arows
        r, c = slice(ar * NB, (ar + 1) * NB), slice(tj * NB, (tj + 1) * NB)
        return self.alpha * (A[r, k0:k1] @ self.B[k0:k1, c]) + self.beta * self.C0[ti * NB:(ti + 1) * NB, c]


class Prepared:
    """A case's references, computed once: what the judges hold an output buffer against."""

    def __init__(self, kind, out0, pieces, local=None):
        self.kind, self.out0, self.pieces = kind, out0, pieces
        self.covered = np.zeros(out0.shape, dtype=bool)
        self.refs = []
        flops = 0.0
        for p in pieces:
            self.covered[p.sel][p.mask] = True
            for ti, tj in p.tiles():
                flops += 2.0 * len(SAMPLE) * NB * (p.khi[ti, tj] - p.klo[ti, tj])
        self.local = local if local is not None else (SAMPLE if flops <= LD_FLOP_BUDGET else THIN)
        for p in pieces:
            ref = p.alpha * (p.A @ p.B) + p.beta * p.C0                       # numpy's fp64 BLAS
            tot = abs(p.alpha) * (np.abs(p.A) @ np.abs(p.B)) + abs(p.beta) * np.abs(p.C0)
            K = np.kron(p.khi - p.klo + p.S + 3, np.ones((NB, NB)))
            bound = gamma(K) * tot
            ld = self._sample(p) if (kind == "real" and HAVE_LD) else None
            self.refs.append((ref, bound, ld))

    def _sample(self, p):
        """long-double values of the sampled rows and columns, tile row by tile row over the k range that is not zero"""
        Al, Bl, Cl = p.A.astype(LD), p.B.astype(LD), p.C0.astype(LD)
        al, be = LD(p.alpha), LD(p.beta)
        rows, cols = sample_index(p.mask.shape[0], self.local), sample_index(p.mask.shape[1], self.local)
        R = np.zeros((len(rows), p.mask.shape[1]), dtype=LD)
        C = np.zeros((p.mask.shape[0], len(cols)), dtype=LD)
        for t in range(p.klo.shape[0]):
            live = np.nonzero(p.mask[t * NB, ::NB])[0]
            if live.size == 0:
                continue
            k0, k1 = p.klo[t, live].min(), p.khi[t, live].max()
            cm = p.mask[t * NB]
            rr = np.nonzero(rows // NB == t)[0]
            R[np.ix_(rr, np.nonzero(cm)[0])] = al * (Al[rows[rr], k0:k1] @ Bl[k0:k1][:, cm]) + be * Cl[rows[rr]][:, cm]
        for t in range(p.klo.shape[1]):
            live = np.nonzero(p.mask[::NB, t * NB])[0]
            if live.size == 0:
                continue
            k0, k1 = p.klo[live, t].min(), p.khi[live, t].max()
            rm = p.mask[:, t * NB]
            cc = np.nonzero(cols // NB == t)[0]
            C[np.ix_(np.nonzero(rm)[0], cc)] = al * (Al[rm][:, k0:k1] @ Bl[k0:k1][:, cols[cc]]) + be * Cl[rm][:, cols[cc]]
        return rows, cols, R, C

    def verdict(self, out):
        """dict: untouched / no_nan (bool), exact (bool, integer cases), fp64 / ld (worst err / bound, real cases; the fp64 figure
        is against TWICE the bound).  `accepts` says whether all of it holds."""
        v = {"untouched": bool(np.array_equal(out[~self.covered].view(np.int64), self.out0[~self.covered].view(np.int64))),
             "no_nan": True, "exact": None, "fp64": None, "ld": None}
        f64 = ldf = 0.0
        exact = True
        for p, (ref, bound, ld) in zip(self.pieces, self.refs):
            o = out[p.sel]
            v["no_nan"] = v["no_nan"] and not np.isnan(o[p.mask]).any()
            if self.kind == "int":
                exact = exact and bool(np.array_equal(o[p.mask], ref[p.mask]))
                continue
            with np.errstate(invalid="ignore", divide="ignore"):
                err = np.abs(o - ref)[p.mask]
                b = bound[p.mask]
                ratio = np.where(err == 0.0, 0.0, err / (2.0 * b))
                f64 = max(f64, float(np.nan_to_num(ratio, nan=np.inf).max()))
                if ld is not None:
                    rows, cols, R, C = ld
                    for got, want, bd, mk in ((o[rows], R, bound[rows], p.mask[rows]), (o[:, cols], C, bound[:, cols], p.mask[:, cols])):
                        e = np.abs(got.astype(LD) - want)[mk]
                        r = np.where(e == 0, LD(0), e / bd[mk].astype(LD))
                        ldf = max(ldf, float(np.nan_to_num(r.astype(np.float64), nan=np.inf).max()))
        if self.kind == "int":
            v["exact"] = exact
        else:
            v["fp64"] = f64
            v["ld"] = ldf if (HAVE_LD and self.refs[0][2] is not None) else None
        return v

    def numpy_result(self):
        """the output buffer as numpy's fp64 BLAS leaves it: the reference on every mask, out0 elsewhere"""
        out = self.out0.copy()
        for p, (ref, _, _) in zip(self.pieces, self.refs):
            out[p.sel][p.mask] = ref[p.mask]
        return out


def accepts(v):
    return bool(v["untouched"] and v["no_nan"] and v["exact"] is not False and (v["fp64"] is None or v["fp64"] <= 1.0)
                and (v["ld"] is None or v["ld"] <= 1.0))


# ---------------------------------------------------------------------------------------------------------------------
# the cases: Case(id, family, make) with make(kind, rng) -> (out0, pieces, run), run(L) -> the device's output buffer
class Case:
    def __init__(self, cid, family, make, kinds=("int", "real"), local=None):
        self.id, self.family, self.make, self.kinds, self.local = cid, family, make, kinds, local

    def prepare(self, kind):
        seed = int.from_bytes(self.id.encode(), "little") % (2 ** 31) + (kind == "real")
        out0, pieces, run = self.make(kind, np.random.default_rng(seed))
        return Prepared(kind, out0, pieces, self.local), run


def _gemm_case(a_m, b_n, M, N, K, alpha, beta):
    def make(kind, rng):
        A = draw(kind, rng, (K, M) if a_m else (M, K))
        B = draw(kind, rng, (K, N) if b_n else (N, K))
        mask = np.ones((M, N), dtype=bool)
        C0 = None if beta == 0.0 else draw(kind, rng, (M, N))
        out0 = prefill(rng, mask, C0)
        p = Piece(np.s_[:, :], A.T if a_m else A, B if b_n else B.T, alpha, beta, C0, mask, 0, K)
        return out0, [p], lambda L: L.dbg_gemm(A, B, out0, a_m, b_n, alpha, beta)[0]
    return make


def _trmm_case(op, mode, nt, nto, alpha):
    """op 'trmm_lower' (mode 0), 'trmm_lower_T' (mode 1) or 'trmm64' (mode 0..3)"""
    def make(kind, rng):
        n, m = nt * NB, nto * NB
        X, X0 = lower_with_poison(kind, rng, n)
        left = mode < 2                                           # X on the left: B, Out are n x m
        B = draw(kind, rng, (n, m) if left else (m, n))
        mask = np.ones(B.shape, dtype=bool)
        out0 = prefill(rng, mask, None)
        ti, tj = np.meshgrid(np.arange(mask.shape[0] // NB), np.arange(mask.shape[1] // NB), indexing="ij")
        if mode == 0:
            p = Piece(np.s_[:, :], X0, B, alpha, 0.0, None, mask, 0, (ti + 1) * NB)
        elif mode == 1:
            p = Piece(np.s_[:, :], X0.T, B, alpha, 0.0, None, mask, ti * NB, n)
        elif mode == 2:
            p = Piece(np.s_[:, :], B, X0.T, alpha, 0.0, None, mask, 0, (tj + 1) * NB)
        else:
            p = Piece(np.s_[:, :], B, X0, alpha, 0.0, None, mask, tj * NB, n)
        dims = (nt, nto, mode) if op == "trmm64" else (nt, nto)
        return out0, [p], lambda L: L.dbg_tileop(op, dims, X, B, out0, alpha)
    return make


def _gram_case(mp, rows, S, accumulate):
    def make(kind, rng):
        P = draw(kind, rng, (rows, mp))
        nt = mp // NB
        mask = tile_mask(nt, nt, lambda ti, tj: tj <= ti)
        rs = rows // S
        out0 = np.empty((S, mp, mp))
        pieces = []
        for s in range(S):
            C0 = draw(kind, rng, (mp, mp)) if accumulate else None
            out0[s] = prefill(rng, mask, C0)
            Ps = P[s * rs:(s + 1) * rs]
            pieces.append(Piece(np.s_[s], Ps.T, Ps, 1.0, 1.0 if accumulate else 0.0, C0, mask, 0, rs))
        return out0, pieces, lambda L: L.dbg_tileop("gram_splitk", (rows, mp, S, accumulate), P, None, out0)
    return make


def _update_case(K, ntr, ntc, row0t, col0t):
    def make(kind, rng):
        n = K + NB * max(row0t + ntr, col0t + ntc)
        M = draw(kind, rng, (n, n))
        r0, c0 = K + row0t * NB, K + col0t * NB
        sel = np.s_[r0:r0 + ntr * NB, c0:c0 + ntc * NB]
        mask = tile_mask(ntr, ntc, lambda ti, tj: col0t + tj <= row0t + ti)
        p = Piece(sel, M[r0:r0 + ntr * NB, :K].copy(), M[c0:c0 + ntc * NB, :K].T.copy(), -1.0, 1.0, M[sel].copy(), mask, 0, K)
        return M, [p], lambda L: L.dbg_tileop("update_nt", (K, ntr, ntc, row0t, col0t), None, None, M)
    return make


def lauum_partial_sums(nt, plan):
    """S per tile of X^T X as `lauum_device` launches it: 0 up to nt = 8 (k_lauum64), else the chunks of the split work list
    (`plan`: the rows (ti, tj, q, k0, klen, part) of gpy_amd._lib.lauum_plan)"""
    S = np.zeros((nt, nt), dtype=int)
    if nt * NB > 1024:
        q0 = plan[:, 2].min()
        for ti, tj, q, _, _, _ in plan:
            if q == q0:
                S[ti, tj] += 1
    return S


def _lauum_case(nt):
    def make(kind, rng):
        n = nt * NB
        X, X0 = lower_with_poison(kind, rng, n)
        mask = tile_mask(nt, nt, lambda ti, tj: tj <= ti)
        out0 = prefill(rng, mask, None)
        ti = np.arange(nt)[:, None]
        from gpy_amd import _lib
        S = lauum_partial_sums(nt, _lib.lauum_plan(nt)[0])
        p = Piece(np.s_[:, :], X0.T.copy(), X0, 1.0, 0.0, None, mask, ti * NB, n, S)
        return out0, [p], lambda L: L.dbg_lauum(X, 2, W0=out0)[0]
    return make


def cases():
    out = []
    for a_m in (0, 1):
        for b_n in (0, 1):
            for M, N in ((128, 128), (256, 384)):
                for K in (16, 32, 48, 128, 400):
                    for alpha, beta in ((1.0, 0.0), (0.5, -2.0), (0.7, -1.3)):
                        kinds = ("real",) if alpha == 0.7 else ("int", "real")
                        out.append(Case("gemm-a%d-b%d-%dx%dx%d-%g-%g" % (a_m, b_n, M, N, K, alpha, beta), "gemm",
                                        _gemm_case(a_m, b_n, M, N, K, alpha, beta), kinds))
    for nt in (1, 2, 3, 5):
        for nto in (1, 3):
            out.append(Case("trmm_lower-%d-%d" % (nt, nto), "trmm_lower", _trmm_case("trmm_lower", 0, nt, nto, 1.0)))
            out.append(Case("trmm_lower_T-%d-%d" % (nt, nto), "trmm_lower_T", _trmm_case("trmm_lower_T", 1, nt, nto, 1.0)))
            for mode in range(4):
                for alpha in (1.0, -0.5):
                    out.append(Case("trmm64-m%d-%d-%d-%g" % (mode, nt, nto, alpha), "trmm64 mode %d" % mode,
                                    _trmm_case("trmm64", mode, nt, nto, alpha)))
    for mp in (128, 384):
        for rows in (32, 96, 768):
            for S in (1, 2, 3):
                if rows % (16 * S) == 0:
                    for acc in (0, 1):
                        out.append(Case("gram-%d-%d-S%d-acc%d" % (mp, rows, S, acc), "gram_splitk", _gram_case(mp, rows, S, acc)))
    for K in (128, 512, 1024):
        for nt in (1, 3, 15, 16):
            out.append(Case("update-tri-K%d-%d" % (K, nt), "update_nt " + ("64" if nt <= 15 else "128"), _update_case(K, nt, nt, 0, 0)))
        for ntr, ntc, r0, c0 in ((3, 2, 2, 0), (2, 3, 1, 1), (12, 12, 3, 0)):
            out.append(Case("update-rect-K%d-%d-%d-%d-%d" % (K, ntr, ntc, r0, c0), "update_nt " + ("64" if ntr < 12 else "128"),
                            _update_case(K, ntr, ntc, r0, c0)))
    for nt in (1, 2, 3, 8, 9, 10, 17, 24):
        fam = "lauum k_lauum64" if nt <= 8 else ("lauum split 64" if nt < 24 else "lauum split 128")
        out.append(Case("lauum-%d" % nt, fam, _lauum_case(nt), local=THIN if nt == 24 else None))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# planted faults (test_oracle_tileops.py): each takes the Prepared case and a correct output buffer, returns a faulty copy or
# None where the case has no place for this fault (said there)
def _pick_tile(prep):
    """(piece, ti, tj) of the LAST computed tile of the last piece: the one with the neighbours before it"""
    p = prep.pieces[-1]
    ti, tj = p.tiles()[-1]
    return p, ti, tj


def fault_missing_slab(prep, out):
    p, ti, tj = _pick_tile(prep)
    k0 = p.klo[ti, tj] + 16 * ((p.khi[ti, tj] - p.klo[ti, tj]) // 32)              # a slab in the middle of the range
    bad = out.copy()
    r, c = slice(ti * NB, (ti + 1) * NB), slice(tj * NB, (tj + 1) * NB)
    bad[p.sel][r, c] -= p.alpha * (p.A[r, k0:k0 + 16] @ p.B[k0:k0 + 16, c])
    return bad


def fault_neighbour_range(prep, out):
    """a tile computed with the SHORTER k range of a tile next to it (a longer one would only add the structural zeros of the
    triangular operand -- on the device, its NaN tiles: the poison's business); where every tile walks the same range (GEMM,
    update, Gram), with the neighbouring tile's rows of A or columns of B: the wrong tile map.  None for a one-tile output."""
    p = prep.pieces[-1]
    bad = out.copy()
    for ti, tj in reversed(p.tiles()):
        r, c = slice(ti * NB, (ti + 1) * NB), slice(tj * NB, (tj + 1) * NB)
        for ni, nj in ((ti - 1, tj), (ti, tj - 1), (ti + 1, tj), (ti, tj + 1)):
            if not (0 <= ni < p.klo.shape[0] and 0 <= nj < p.klo.shape[1] and p.mask[ni * NB, nj * NB]):
                continue
            if p.klo[ni, nj] >= p.klo[ti, tj] and p.khi[ni, nj] <= p.khi[ti, tj] and \
                    p.khi[ni, nj] - p.klo[ni, nj] < p.khi[ti, tj] - p.klo[ti, tj]:
                bad[p.sel][r, c] = p.tile(ti, tj, p.klo[ni, nj], p.khi[ni, nj])
                return bad
    p, ti, tj = _pick_tile(prep)
    r, c = slice(ti * NB, (ti + 1) * NB), slice(tj * NB, (tj + 1) * NB)
    if ti >= 1:
        bad[p.sel][r, c] = p.tile(ti, tj, arows=ti - 1)
        return bad
    if tj >= 1:
        bad[p.sel][r, c] = p.tile(ti, tj - 1) - p.beta * (p.C0[r, (tj - 1) * NB:tj * NB] - p.C0[r, c])    # the neighbour's columns of B
        return bad
    return None


def fault_fp32_operand(prep, out):
    """real cases only: integers in [-4, 4] pass through fp32 unchanged"""
    if prep.kind == "int":
        return None
    p, ti, tj = _pick_tile(prep)
    bad = out.copy()
    bad[p.sel][ti * NB:(ti + 1) * NB, tj * NB:(tj + 1) * NB] = p.tile(ti, tj, A=p.A.astype(np.float32).astype(np.float64))
    return bad


def fault_four_gamma(prep, out):
    """one element (a sampled one: local row 15, column 64 of the tile) moved by 4 times its own bound"""
    if prep.kind == "int":
        return None
    p, ti, tj = _pick_tile(prep)
    bad = out.copy()
    i, j = ti * NB + 15, tj * NB + 64
    bad[p.sel][i, j] += 4.0 * prep.refs[-1][1][i, j]
    return bad


def fault_nan(prep, out):
    p, ti, tj = _pick_tile(prep)
    bad = out.copy()
    bad[p.sel][ti * NB + 77, tj * NB + 3] = np.nan
    return bad


def fault_sentinel(prep, out):
    free = np.argwhere(~prep.covered)
    if free.size == 0:
        return None
    bad = out.copy()
    idx = tuple(free[len(free) // 2])
    bad[idx] = np.nextafter(bad[idx], np.inf)                  # one bit
    return bad


FAULTS = {"missing 16-term k-slab": fault_missing_slab, "neighbour's k range": fault_neighbour_range,
          "operand through fp32": fault_fp32_operand, "element moved by 4 gamma mag": fault_four_gamma, "one NaN": fault_nan,
          "changed sentinel": fault_sentinel}


# ---------------------------------------------------------------------------------------------------------------------
# PART B: the dense chain.  All figures are max over the lower triangle of err / bound; `rows` = None: every element in long
# double (n <= FULL_LD_MAX), else the rows and columns of sample_index in long double -- and EVERY element in fp64 BLAS at
# twice the bound (returned separately).
FULL_LD_MAX = 640
DENSE_SIZES = (1, 2, 64, 127, 128, 129, 255, 257, 511, 513, 640, 1025, 1153)
DENSE_CASES = [(n, 0.5) for n in DENSE_SIZES] + [(640, 1e-6), (1025, 1e-6)]


def _ld_lower(P, Q, struct, idx=None):
    """Long-double P @ Q on the lower triangle only, walking only the k range where both factors are not structurally zero (a dense
    long-double product of n = 640 takes a second; this takes a sixth).  struct: 'll' P, Q lower triangular (k in [j, i]); 'lu' P
    lower, Q upper (k <= j: L L^T); 'ul' P upper, Q lower (k >= i: X^T X).  idx None: the n x n product (blocks above the diagonal
    left zero); else (rows idx of it, columns idx of it)."""
    n = P.shape[0]
    Pl, Ql = P.astype(LD if HAVE_LD else np.float64), Q.astype(LD if HAVE_LD else np.float64)
    nt = (n + NB - 1) // NB
    if idx is None:
        out = np.zeros((n, n), dtype=Pl.dtype)
        for bi in range(nt):
            r = slice(bi * NB, min((bi + 1) * NB, n))
            for bj in range(bi + 1):
                c = slice(bj * NB, min((bj + 1) * NB, n))
                k = {"ll": slice(c.start, r.stop), "lu": slice(0, c.stop), "ul": slice(r.start, n)}[struct]
                out[r, c] = Pl[r, k] @ Ql[k, c]
        return out
    R = np.zeros((len(idx), n), dtype=Pl.dtype)
    C = np.zeros((n, len(idx)), dtype=Pl.dtype)
    for t in range(nt):
        s, e = t * NB, min((t + 1) * NB, n)
        w = np.nonzero(idx // NB == t)[0]
        if w.size == 0:
            continue
        k = slice(s, n) if struct == "ul" else slice(0, e)
        R[w, :e] = Pl[idx[w], k] @ Ql[k, :e]
        k = slice(0, e) if struct == "lu" else slice(s, n)
        C[s:, w] = Pl[s:, k] @ Ql[k][:, idx[w]]
    return R, C


def _ld_parts(P, Q, struct, target):
    """[(|target - P Q| in long double, index into the matrix)] over what is judged in long double: every element up to
    n = FULL_LD_MAX, the sampled rows and columns above"""
    n = P.shape[0]
    dt = LD if HAVE_LD else np.float64
    T = target.astype(dt)
    if n <= FULL_LD_MAX:
        return [(np.abs(T - _ld_lower(P, Q, struct)), np.s_[:, :])]
    idx = sample_index(n)
    R, C = _ld_lower(P, Q, struct, idx)
    return [(np.abs(T[idx] - R), np.s_[idx, :]), (np.abs(T[:, idx] - C), np.s_[:, idx])]


def _worst(err, bound, low):
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0, 0 * err, err / bound.astype(err.dtype))[low]
    return float(np.nan_to_num(r.astype(np.float64), nan=np.inf).max())


def _product_figures(P, Q, struct, target, bound_k):
    """worst |target - P @ Q| / (gamma_k |P| |Q|) over the lower triangle: (fp64 BLAS figure over EVERY element, against twice the
    bound; long-double figure over every element if n <= FULL_LD_MAX else over the sampled rows and columns, or None)"""
    n = target.shape[0]
    low = np.tril(np.ones((n, n), dtype=bool))
    bound = gamma(bound_k) * (np.abs(P) @ np.abs(Q))
    f64 = _worst(np.abs(target - P @ Q), 2.0 * bound, low)
    if not HAVE_LD:
        return f64, None
    return f64, max(_worst(e, bound[ix], low[ix]) for e, ix in _ld_parts(P, Q, struct, target))


def chol_figures(A, L):
    """|A - L L^T| <= gamma_{n+1} |L| |L^T| elementwise (Higham, Theorem 10.3: any ordering of a Cholesky factorisation built from
    conventional products)"""
    return _product_figures(L, L.T, "lu", A, A.shape[0] + 1)


def ainv_figures(Ai, Li):
    """|Ai - Li^T Li| <= gamma_{n+35} |Li|^T |Li|: a product of at most n terms, cut into at most 32 partial sums, 3 for the epilogue"""
    return _product_figures(Li.T, Li, "ul", Ai, Ai.shape[0] + 35)


def inv_figures(L, Li):
    """(max |Li L - I| / (n u |Li| |L|), the same for L Li) over the lower triangle, in long double (every element up to
    n = FULL_LD_MAX, the sampled rows and columns above); fp64 where there is no extended type"""
    n = L.shape[0]
    low = np.tril(np.ones((n, n), dtype=bool))
    I = np.eye(n)
    out = []
    for P, Q in ((Li, L), (L, Li)):
        den = n * U * (np.abs(P) @ np.abs(Q))
        out.append(max(_worst(e, den[ix], low[ix]) for e, ix in _ld_parts(P, Q, "ll", I)))
    return tuple(out)


def logdet_figure(logdet, L):
    """|logdet - 2 sum log L_ii| / (2 gamma_{n+4} sum |log L_ii|), the sum in long double (1 where the bound is zero and met)"""
    dt = LD if HAVE_LD else np.float64
    lg = np.log(np.diag(L).astype(dt))
    ref, mag = 2 * lg.sum(), 2 * np.abs(lg).sum()
    err = abs(dt(logdet) - ref)
    bound = float(gamma(L.shape[0] + 4)) * mag
    return 0.0 if err == 0 else float(err / bound) if bound > 0 else float("inf")


def trtri_blocked(L):
    """fp64 numpy transcription of the device's triangular inverse: the 128 x 128 diagonal blocks inverted on their own, then
    bottom-up levels that merge neighbouring blocks of 2^s tiles pairwise, X21 = -X22 (L21 X11), stage by stage as gemm.hip does"""
    from scipy.linalg import solve_triangular
    n = L.shape[0]
    nt = (n + NB - 1) // NB
    X = np.zeros_like(L)
    for t in range(nt):
        s = slice(t * NB, min((t + 1) * NB, n))
        X[s, s] = solve_triangular(L[s, s], np.eye(s.stop - s.start), lower=True)
    nbt = 1
    while nbt < nt:
        for left0 in range(0, nt, 2 * nbt):
            right0 = left0 + nbt
            if right0 >= nt:
                continue
            a, b, c = left0 * NB, right0 * NB, min((right0 + nbt) * NB, n)
            T = L[b:c, a:b] @ X[a:b, a:b]
            X[b:c, a:b] = -(X[b:c, b:c] @ T)
        nbt *= 2
    return X


def trtri_lapack(L):
    from scipy.linalg.lapack import dtrtri
    X, info = dtrtri(L, lower=1)
    assert info == 0
    return np.tril(X)


def dense_report(A, Ai, L, Li, logdet, base=None):
    """every figure of one pdinv_full result, each stage against its own input; inv_ref: the reference algorithms (LAPACK's dtrtri,
    the transcription) on the SAME L.  base: an earlier report; a stage whose inputs are the very same arrays is taken from it."""
    same = (lambda *names: base is not None and all(base["_in"][k] is v for k, v in names))
    r = {"n": A.shape[0], "_in": {"A": A, "Ai": Ai, "L": L, "Li": Li, "logdet": logdet}}
    r["chol"] = base["chol"] if same(("A", A), ("L", L)) else chol_figures(A, L)
    r["ainv"] = base["ainv"] if same(("Ai", Ai), ("Li", Li)) else ainv_figures(Ai, Li)
    r["inv"] = base["inv"] if same(("L", L), ("Li", Li)) else inv_figures(L, Li)
    r["inv_ref"] = base["inv_ref"] if same(("L", L)) else (inv_figures(L, trtri_lapack(L)), inv_figures(L, trtri_blocked(L)))
    r["logdet"] = base["logdet"] if same(("L", L), ("logdet", logdet)) else logdet_figure(logdet, L)
    r["L_upper_zero"] = bool(np.all(np.triu(L, 1) == 0.0))
    r["Ai_symmetric"] = bool(np.array_equal(Ai.view(np.int64), Ai.T.view(np.int64)))
    return r


def potrf_accepts(A, L):
    f64, ld = chol_figures(A, L)
    return bool(np.all(np.triu(L, 1) == 0.0) and f64 <= 1.0 and (ld is None or ld <= 1.0)), (f64, ld)


def report_line(r):
    return "n=%d chol %.3f/%s ainv %.3f/%s logdet %.3f inv (Li L, L Li) %.4f %.4f dtrtri %.4f %.4f transcription %.4f %.4f" % (
        (r["n"], r["chol"][0], r["chol"][1], r["ainv"][0], r["ainv"][1], r["logdet"]) + r["inv"] + r["inv_ref"][0] + r["inv_ref"][1])


def dense_accepts(r, inv_factor=8.0):
    """the four checks: bounds at 1 (fp64 all-element figures are already against twice the bound), Li at most inv_factor times
    the larger reference figure, side by side"""
    ok = r["L_upper_zero"] and r["Ai_symmetric"] and r["logdet"] <= 1.0
    for key in ("chol", "ainv"):
        f64, ld = r[key]
        ok = ok and f64 <= 1.0 and (ld is None or ld <= 1.0)
    for side in (0, 1):
        ok = ok and r["inv"][side] <= inv_factor * max(r["inv_ref"][0][side], r["inv_ref"][1][side])
    return bool(ok)
