// parts.h -- the host-side model of one kernel part (mi355gp_part) shared by the exact, sparse and grid paths: which kinds
// an entry point takes, theta validation, active dimensions, input scaling, term grouping, Kdiag of a sum of products and
// the post-scaling of the reduction records into gradients in theta order.  Host code only.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/mi355gp.h"
#include "internal.h"

#define COREG_REC 256          // doubles of one Coregionalize part's S (P x P, P <= 16)

// the sums of dimension q in the records of one part (one GP_STRIDE record per group of 32 dimensions)
static inline double rec_at(const double* rec, int q) { return rec[(q / 32) * GP_STRIDE + 2 + (q % 32)]; }

typedef unsigned KindSet;      // bit k: kind k is accepted
enum : KindSet {
    KS_STATIONARY = 1u << MI355GP_RBF | 1u << MI355GP_MATERN52 | 1u << MI355GP_MATERN32 | 1u << MI355GP_EXPONENTIAL,
    KS_STATIC = 1u << MI355GP_WHITE | 1u << MI355GP_BIAS,
    KS_EXT = 1u << MI355GP_RATQUAD | 1u << MI355GP_STDPERIODIC,     // two reduction records per part (k_grad_ext)
    KS_COREG = 1u << MI355GP_COREGIONALIZE,
    KS_LINEAR = 1u << MI355GP_LINEAR,                               // exact path only; Kdiag depends on the point
    KS_DOT = 1u << MI355GP_MLP | 1u << MI355GP_POLY,                // likewise: functions of x.x', x.x and x'.x' (k_kbuild_dot)
    // exact path only: the oscillating functions of r, in RatQuad's kernels (k_kbuild_ext / k_grad_ext)
    KS_OSC = 1u << MI355GP_COSINE | 1u << MI355GP_SINC | 1u << MI355GP_EXPQUADCOSINE,
};
static inline bool kind_in(int kind, KindSet s) { return kind >= 0 && kind < 32 && ((s >> kind) & 1u); }
static inline const char* kind_name(int kind) {
    static const char* const names[] = {"RBF", "Matern52", "Matern32", "Exponential", "White", "Bias", "RatQuad",
                                        "StdPeriodic", "Coregionalize", "Linear", "MLP", "Poly", "Cosine", "Sinc",
                                        "ExpQuadCosine"};
    return kind_in(kind, KS_STATIONARY | KS_STATIC | KS_EXT | KS_COREG | KS_LINEAR | KS_DOT | KS_OSC) ? names[kind] : "unknown";
}

#define PART_FAIL(...)                    \
    do {                                  \
        mi355gp_set_error(__VA_ARGS__);   \
        return -1;                        \
    } while (0)

static inline int check_kind(int kind, KindSet accepted, const char* where) {
    if (!kind_in(kind, accepted)) PART_FAIL("%s: covariance kind %d (%s) is not supported here", where, kind, kind_name(kind));
    return 0;
}

// Coregionalize (kind 8, coregionalize.py:82-157): `ard` = the number of outputs P, theta = B (P x P).  Output indices are
// values of one input column; each must be an integer in [0, P) -- checked on the host, before any launch reads one.
static inline int coreg_check_P(int P) {
    if (P < 1 || P > 16)
        PART_FAIL("Coregionalize (kind 8): the number of outputs (ard) must be between 1 and 16, got %d", P);
    return 0;
}
static inline int coreg_check_index(const double* x, long n, long stride, int P, const char* what) {
    for (long i = 0; i < n; ++i) {
        const double v = x[i * stride];
        if (!(v >= 0.0 && v < (double)P && v == std::floor(v)))
            PART_FAIL("Coregionalize (kind 8): %s output index %.17g (row %ld) is not an integer in [0, %d)", what, v, i, P);
    }
    return 0;
}

// Everything the host derives from one mi355gp_part; no device pointers (kp.pw stays NULL: the owner points it at its own
// device copy of pw).
struct PartSpec {
    KernParams kp = {0, 0, 0, 1.0};
    int ard_in = 0;                 // the `ard` of the C-ABI part (StdPeriodic: the ARD1 | ARD2 bitmask; Coregionalize: P)
    std::vector<int> dims;          // active input dimensions (kern.py:49-53), indices into the D columns of X
    std::vector<double> theta;      // exactly the kind's parameters, in theta order
    std::vector<double> inv_ls;     // length D: 1/l on active dimensions, 0 elsewhere (= the slicing of kern.py:112-117)
                                    // (StdPeriodic: 1 on active dimensions, Coregionalize: 1 on the index column -- unscaled;
                                    // Linear: sqrt(variance_q), so that K = sum_q x~_iq x~_jq; MLP: sqrt(weight_variance_q),
                                    // Poly: sqrt(scale) -- the tile kernels see plain dot products)
    std::vector<double> pw;         // StdPeriodic: [pi / T_q (D) | 1 / l_q (D)]; Coregionalize: B (P x P); empty otherwise
    int term = 0;                   // term id of the C-ABI part: parts with the same non-zero id are multiplied (prod.py)
    int tix = 0;                    // index of its summand in the terms of group_terms
    bool stationary() const { return kind_in(kp.kind, KS_STATIONARY); }
    bool is_static() const { return kind_in(kp.kind, KS_STATIC); }
    // a second reduction record (ExpQuadCosine: its [0] = the period sum, as RatQuad's power; Cosine and Sinc have none)
    bool ext() const { return kind_in(kp.kind, KS_EXT | 1u << MI355GP_EXPQUADCOSINE); }
    bool coreg() const { return kp.kind == MI355GP_COREGIONALIZE; }
    bool linear() const { return kp.kind == MI355GP_LINEAR; }
    bool mlp() const { return kp.kind == MI355GP_MLP; }
    bool poly() const { return kp.kind == MI355GP_POLY; }
    // Kdiag depends on the point: kp.variance is NOT the diagonal
    bool diag_by_point() const { return coreg() || linear() || mlp() || poly(); }
};

// A part with its parameters on the device as well: inv_ls (D) and pw, uploaded together once per call by upload() (kp.pw ->
// dPw).  Any point set is then scaled for the part with one launch_scale_inputs.  Owners: the exact context, the sparse
// context and the stateless entry points.
struct DevicePart : PartSpec {
    DevBuf dIl, dPw;
    int upload(hipStream_t st) {
        if (!dIl) HIP_CHECK(dIl.alloc(inv_ls.size()));
        HIP_CHECK(hipMemcpyAsync(dIl, inv_ls.data(), sizeof(double) * inv_ls.size(), hipMemcpyHostToDevice, st));
        if (!pw.empty()) {
            if (!dPw) HIP_CHECK(dPw.alloc(std::max(2 * inv_ls.size(), (size_t)COREG_REC)));   // (B of a Coregionalize part)
            HIP_CHECK(hipMemcpyAsync(dPw, pw.data(), sizeof(double) * pw.size(), hipMemcpyHostToDevice, st));
            kp.pw = dPw;
        }
        return 0;
    }
};

// The one validator of a kernel part over D input columns (n_active = 0: all of them).  `accepted`: the kinds the entry point
// takes; `where`: the entry point or path, named in every error.  Coregionalize output indices are checked where the data are.
static inline int parse_part(const mi355gp_part& in, int D, KindSet accepted, const char* where, PartSpec* p) {
    const int kind = in.kind, ard = in.ard;
    if (int rc = check_kind(kind, accepted, where)) return rc;
    if (!in.theta) PART_FAIL("%s: theta of a %s (kind %d) part is NULL", where, kind_name(kind), kind);
    const double* th = in.theta;
    p->dims.clear();
    p->pw.clear();
    p->inv_ls.assign((size_t)D, 0.0);
    p->ard_in = ard;
    p->term = in.term;
    if (kind == MI355GP_COREGIONALIZE) {
        if (!(in.n_active == 1 && in.active_dims && in.active_dims[0] >= 0 && in.active_dims[0] < D))
            PART_FAIL("%s: Coregionalize (kind 8): n_active must be 1 (the input column of the output index), got %d", where,
                      in.n_active);
        if (int rc = coreg_check_P(ard)) return rc;
        for (int k = 0; k < ard * ard; ++k)
            if (!std::isfinite(th[k])) PART_FAIL("%s: Coregionalize (kind 8): B[%d] = %g is not finite", where, k, th[k]);
        const int col = in.active_dims[0];
        p->dims.assign(1, col);
        p->theta.assign(th, th + ard * ard);
        p->pw = p->theta;
        p->inv_ls[(size_t)col] = 1.0;                 // the index column stays unscaled
        p->kp = KernParams{kind, ard, D, th[0]};
        p->kp.col = col;
        return 0;
    }
    if (!(th[0] > 0.0)) PART_FAIL("%s: the variance of a %s (kind %d) part must be positive, got %g", where, kind_name(kind), kind, th[0]);
    if (in.active_dims && in.n_active > 0) {
        for (int a = 0; a < in.n_active; ++a) {
            const int q = in.active_dims[a];
            if (q < 0 || q >= D)
                PART_FAIL("%s: active dimension %d of a %s (kind %d) part is out of range [0, %d)", where, q, kind_name(kind), kind, D);
            p->dims.push_back(q);
        }
    } else {
        for (int q = 0; q < D; ++q) p->dims.push_back(q);
    }
    const int na = (int)p->dims.size();
    auto positive = [&](double v, const char* what) {
        if (v > 0.0) return 0;
        mi355gp_set_error("%s: %s %g of a %s (kind %d) part must be positive", where, what, v, kind_name(kind), kind);
        return -1;
    };
    int nt = 1;                                        // static kinds: [variance]
    p->kp = KernParams{kind, 0, D, th[0]};
    if (kind == MI355GP_STDPERIODIC) {                 // [variance, period (1 or n_active), lengthscale (1 or n_active)]
        if (ard < 0 || ard > 3)
            PART_FAIL("%s: StdPeriodic (kind 7): ard %d is not a bitmask (1 = one period, 2 = one lengthscale per dimension)",
                      where, ard);
        const int nper = (ard & 1) ? na : 1, nl = (ard & 2) ? na : 1;
        p->pw.assign(2 * (size_t)D, 0.0);
        for (int a = 0; a < na; ++a) {
            const double T = th[1 + ((ard & 1) ? a : 0)], l = th[1 + nper + ((ard & 2) ? a : 0)];
            if (int rc = positive(T, "period")) return rc;
            if (int rc = positive(l, "lengthscale")) return rc;
            const int q = p->dims[a];
            p->inv_ls[(size_t)q] = 1.0;                // unscaled inputs: Delta from the raw coordinates
            p->pw[(size_t)q] = M_PI / T;
            p->pw[(size_t)(D + q)] = 1.0 / l;
        }
        p->kp.ard = 1;                                 // per-dimension reductions
        nt = 1 + nper + nl;
    } else if (kind == MI355GP_LINEAR) {               // [variance (1 or n_active)] (linear.py:34-51)
        nt = ard ? na : 1;
        for (int a = 0; a < na; ++a) {
            const double v = th[ard ? a : 0];
            if (int rc = positive(v, "variance")) return rc;
            p->inv_ls[(size_t)p->dims[a]] = std::sqrt(v);
        }
        p->kp.ard = ard ? 1 : 0;                       // per-dimension reductions
    } else if (kind == MI355GP_MLP) {                  // [variance, weight_variance (1 or n_active), bias_variance] (mlp.py:36-45)
        const int nw = ard ? na : 1;
        for (int a = 0; a < na; ++a) {
            const double w = th[1 + (ard ? a : 0)];
            if (int rc = positive(w, "weight_variance")) return rc;
            p->inv_ls[(size_t)p->dims[a]] = std::sqrt(w);
        }
        p->kp.ard = ard ? 1 : 0;                       // per-dimension reductions
        p->kp.bias = th[1 + nw];
        if (int rc = positive(p->kp.bias, "bias_variance")) return rc;
        nt = 2 + nw;
    } else if (kind == MI355GP_POLY) {                 // [variance, scale, bias, order] (poly.py:15-23)
        if (int rc = positive(th[1], "scale")) return rc;
        if (int rc = positive(th[2], "bias")) return rc;
        if (!(th[3] >= 1.0 && std::isfinite(th[3])))
            PART_FAIL("%s: order %g of a Poly (kind %d) part must be at least 1 (poly.py:22)", where, th[3], kind);
        for (int a = 0; a < na; ++a) p->inv_ls[(size_t)p->dims[a]] = std::sqrt(th[1]);
        p->kp.bias = th[2];
        p->kp.power = th[3];
        nt = 4;
    } else if (!p->is_static()) {                      // stationary, Cosine, Sinc: [variance, lengthscale (1 or n_active)];
                                                       // RatQuad: (, power); ExpQuadCosine: (, period), carried in kp.power
        const int nl = ard ? na : 1;
        for (int a = 0; a < na; ++a) {
            const double l = th[1 + (ard ? a : 0)];
            if (int rc = positive(l, "lengthscale")) return rc;
            p->inv_ls[(size_t)p->dims[a]] = 1.0 / l;
        }
        p->kp.ard = ard ? 1 : 0;
        nt = 1 + nl;
        if (kind == MI355GP_RATQUAD) {
            p->kp.power = th[nt++];
            if (int rc = positive(p->kp.power, "power")) return rc;
        } else if (kind == MI355GP_EXPQUADCOSINE) {    // (link order stationary.py:692-695)
            p->kp.power = th[nt++];
            if (int rc = positive(p->kp.power, "period")) return rc;
            if (!std::isfinite(p->kp.power)) PART_FAIL("%s: period %g of an ExpQuadCosine (kind %d) part is not finite", where, p->kp.power, kind);
        }
    }
    p->theta.assign(th, th + nt);
    return 0;
}

// Gradient of one part in theta order from its reduction records (rec: the kind's first record, groups * GP_STRIDE;
// rec2: the second record of RatQuad / StdPeriodic / ExpQuadCosine; Coregionalize: rec = S, P x P).  Returns the number written.
// stationary.py:199,210-213 (x already divided by l inside the kernels), 790-798; standard_periodic.py:501-526
static inline int part_dtheta(const PartSpec& p, const double* rec, const double* rec2, double* o) {
    const double* th = p.theta.data();
    const int na = (int)p.dims.size(), ard = p.ard_in;
    if (p.coreg()) {                                   // S in theta (= B) order
        for (int k = 0; k < ard * ard; ++k) o[k] = rec[k];
        return ard * ard;
    }
    int k = 0;
    if (p.linear()) {                                  // linear.py:87-98: sum g K / variance, or per dimension sum g x~_iq x~_jq / variance_q
        if (!p.kp.ard) o[k++] = rec[0] / th[0];
        else
            for (int a = 0; a < na; ++a) o[k++] = rec_at(rec, p.dims[a]) / th[a];
        return k;
    }
    if (p.mlp()) {                                     // mlp.py:98-123 from the record of k_grad_dot: [0] sum g K, [1] db,
        o[k++] = rec[0] / th[0];                       // [2 + q] w_q dw_q (ARD) or [2] w dw
        if (!p.kp.ard) o[k++] = rec[2] / th[1];
        else
            for (int a = 0; a < na; ++a) o[k++] = rec_at(rec, p.dims[a]) / th[1 + a];
        o[k++] = rec[1];
        return k;
    }
    if (p.poly()) {                                    // poly.py:36-42: [0] sum g K, [1] sum h, [2] scale sum h x.x'; order: no parameter
        o[0] = rec[0] / th[0];
        o[1] = rec[2] / th[1];
        o[2] = rec[1];
        o[3] = 0.0;
        return 4;
    }
    o[k++] = rec[0] / p.kp.variance;                   // sum g K / variance
    if (p.is_static()) return k;
    if (p.kp.kind == MI355GP_STDPERIODIC) {
        const int nper = (ard & 1) ? na : 1;
        double sT = 0.0, sL = 0.0;
        for (int a = 0; a < na; ++a) {
            const double T = th[1 + ((ard & 1) ? a : 0)], l = th[1 + nper + ((ard & 2) ? a : 0)];
            const double gT = rec_at(rec, p.dims[a]) / (T * l * l), gL = rec_at(rec2, p.dims[a]) / (l * l * l);
            if (ard & 1) o[k + a] = gT;
            else sT += gT;
            if (ard & 2) o[k + nper + a] = gL;
            else sL += gL;
        }
        if (!(ard & 1)) o[k] = sT;
        k += nper;
        if (!(ard & 2)) o[k] = sL;
        return k + ((ard & 2) ? na : 1);
    }
    if (!p.kp.ard) o[k++] = -rec[1] / th[1];           // dl = -S / l
    else
        for (int a = 0; a < na; ++a) o[k++] = -rec_at(rec, p.dims[a]) / th[1 + a];
    if (p.kp.kind == MI355GP_RATQUAD || p.kp.kind == MI355GP_EXPQUADCOSINE) o[k++] = rec2[0];   // power / period (:703-709)
    return k;
}

// ---- the expression: a sum over terms of the element-wise product of the term's parts (add.py:58-72, prod.py:58-65) -----
typedef std::vector<std::vector<int>> Terms;

// term id 0 = a summand of its own; parts sharing a non-zero id are the factors of one summand.  Returns the part indices per
// summand in order of first appearance and sets every part's tix.
template <class Part>
static Terms group_terms(std::vector<Part>& parts) {
    Terms terms;
    std::vector<int> ids;
    for (size_t i = 0; i < parts.size(); ++i) {
        const int id = parts[i].term;
        size_t t = ids.size();
        if (id != 0)
            for (t = 0; t < ids.size() && ids[t] != id; ++t) {}
        if (t == ids.size()) {
            ids.push_back(id);
            terms.emplace_back();
        }
        terms[t].push_back((int)i);
        parts[i].tix = (int)t;
    }
    return terms;
}

static inline bool has_product(const Terms& terms) {
    for (const auto& t : terms)
        if (t.size() > 1) return true;
    return false;
}

// Kdiag of the expression: sum over terms of the product of the factors' variances (add.py:74-79, prod.py:67-71).  Only for
// expressions without a diag_by_point() part (the sparse path's kinds; the exact path asks expression_kdiag_points).
template <class Part>
static double expression_kdiag(const std::vector<Part>& parts, const Terms& terms) {
    double s = 0.0;
    for (const auto& t : terms) {
        double v = 1.0;
        for (int f : t) v *= parts[(size_t)f].kp.variance;
        s += v;
    }
    return s;
}

// out (+)= the expression: emit(part, dst, mul, accumulate, first_into_out) launches one factor, dst (+)= K_part * mul.  The
// leading factors of a multi-factor term are multiplied up in `scratch` (same shape as `out`), the last one lands in `out`.
// skip(term): terms left out (e.g. White in a cross-covariance).  Returns false if nothing was emitted.
template <class Skip, class Emit>
static bool emit_expression(const Terms& terms, double* out, double* scratch, bool out_holds_data, Skip skip, Emit emit) {
    bool first = !out_holds_data, any = false;
    for (const auto& t : terms) {
        if (skip(t)) continue;
        const size_t k = t.size();
        for (size_t f = 0; f + 1 < k; ++f) emit(t[f], scratch, f > 0 ? scratch : nullptr, 0, false);
        emit(t[k - 1], out, k > 1 ? scratch : nullptr, first ? 0 : 1, first);
        first = false;
        any = true;
    }
    return any;
}
template <class Emit>
static bool emit_expression(const Terms& terms, double* out, double* scratch, bool out_holds_data, Emit emit) {
    return emit_expression(terms, out, scratch, out_holds_data, [](const std::vector<int>&) { return false; }, emit);
}

// dst = the product of the OTHER factors of part p's term (index tix), emit(part, dst, mul, accumulate, first) launching one
// factor at a time; false: p stands alone
template <class Emit>
static bool emit_other_factors(const Terms& terms, int tix, size_t p, double* dst, Emit emit) {
    const auto& t = terms[(size_t)tix];
    if (t.size() < 2) return false;
    bool first = true;
    for (int f : t) {
        if ((size_t)f == p) continue;
        emit(f, dst, first ? nullptr : dst, 0, first);
        first = false;
    }
    return true;
}

// ---- point sets and cross-covariances ---------------------------------------------------------------------------------
// n host points (row-major n x D) uploaded once; points(part) scales them for that part into the ONE dimension-major buffer t
// (D x ld), overwriting the previous part's scaling.
struct PointSet {
    DevBuf raw, t;
    long n = 0, ld = 0;
    int D = 0;
    int load(hipStream_t st, const double* X, long rows, int dims) {
        n = rows;
        D = dims;
        ld = round_up(rows, 64);
        HIP_CHECK(raw.alloc(n * D));
        HIP_CHECK(t.alloc(D * ld));
        HIP_CHECK(hipMemcpyAsync(raw, X, sizeof(double) * n * D, hipMemcpyHostToDevice, st));
        return 0;
    }
    template <class Part>
    const double* points(hipStream_t st, const Part& p) const {
        launch_scale_inputs(st, raw, n, D, p.dIl, /*per-dimension vector*/ 1, t, ld);
        return t;
    }
};
// the resident, already scaled copy that every part keeps of a point set (member xt: D x ld, n points)
template <class Part>
struct Resident {
    DevBuf Part::*xt;
    long ld, n;
    const double* points(hipStream_t, const Part& p) const { return p.*xt; }
};

// out (+)= K_expr(A, B) (out: ld ldo), one launch_kbuild_cross per factor through emit_expression.  A side is a Resident or a
// PointSet; a point set is scaled for every factor, once if both sides are the same set.  Returns false if nothing was emitted.
template <class Parts, class SideA, class SideB, class Skip>
static bool emit_cross(hipStream_t st, const Parts& parts, const Terms& terms, const SideA& a, const SideB& b, double* out,
                       long ldo, double* scratch, bool out_holds_data, int diag_same, Skip skip) {
    const bool same = (const void*)&a == (const void*)&b;
    return emit_expression(terms, out, scratch, out_holds_data, skip, [&](int p, double* dst, const double* mul, int acc, bool) {
        const auto& pt = parts[(size_t)p];
        const double* xa = a.points(st, pt);
        const double* xb = same ? xa : b.points(st, pt);
        launch_kbuild_cross(st, pt.kp, xa, a.ld, a.n, xb, b.ld, b.n, dst, ldo, acc, diag_same, mul);
    });
}
template <class Parts, class SideA, class SideB>
static bool emit_cross(hipStream_t st, const Parts& parts, const Terms& terms, const SideA& a, const SideB& b, double* out,
                       long ldo, double* scratch, bool out_holds_data, int diag_same) {
    return emit_cross(st, parts, terms, a, b, out, ldo, scratch, out_holds_data, diag_same,
                      [](const std::vector<int>&) { return false; });
}

// ---- dK/dX of one part from its device reductions (gradients_X, predictive_gradients) ----------------------------------
// stationary (stationary.py:330-358): HX = H^T [x2~ | 1] (rows x (D + 1)), x the unscaled host points (rows x D):
//   put(i, q, (x_iq il_q HX[i][D] - HX[i][q]) il_q)
template <class Put>
static void gradx_stationary(const double* x, long rows, int D, const std::vector<double>& il, const double* HX, Put put) {
    for (long i = 0; i < rows; ++i)
        for (int q = 0; q < D; ++q)
            put(i, q, (x[i * D + q] * il[(size_t)q] * HX[i * (D + 1) + D] - HX[i * (D + 1) + q]) * il[(size_t)q]);
}
// StdPeriodic (standard_periodic.py:574-580): HX = the row reduction of launch_periodic_gradx (rows x D):
//   put(i, q, -pi / (2 T_q l_q^2) HX[i][q])
template <class Put>
static void gradx_periodic(const std::vector<double>& pw, long rows, int D, const double* HX, Put put) {
    for (long i = 0; i < rows; ++i)
        for (int q = 0; q < D; ++q)
            put(i, q, -0.5 * pw[(size_t)q] * pw[(size_t)(D + q)] * pw[(size_t)(D + q)] * HX[i * D + q]);
}
// Linear (linear.py:108-114): HX = H^T x2~ (rows x D, x2~ scaled by sqrt(variance_q) = il_q):
//   put(i, q, il_q HX[i][q]) = variance_q sum_j H_ij x2_jq
template <class Put>
static void gradx_linear(const std::vector<double>& il, long rows, int D, const double* HX, Put put) {
    for (long i = 0; i < rows; ++i)
        for (int q = 0; q < D; ++q) put(i, q, il[(size_t)q] * HX[i * D + q]);
}
// MLP (mlp.py:124-130): HX = H^T [x2~ | 1] (rows x (D + 1)) with H = c, x the unscaled host points (rows x D), il_q =
// sqrt(weight_variance_q), b = bias_variance.  The second weight sum_j c_ij s_ij / (p_i + 1) needs no pass of its own:
// s_ij = x~_i . x2~_j + b is linear in x2~_j, so sum_j c_ij s_ij = x~_i . HX[i][0..D) + b HX[i][D].
//   put(i, q, il_q HX[i][q] - il_q^2 x_iq (x~_i . HX_i + b HX[i][D]) / (p_i + 1))
template <class Put>
static void gradx_mlp(const double* x, long rows, int D, const std::vector<double>& il, double b, const double* HX, Put put) {
    for (long i = 0; i < rows; ++i) {
        const double* h = HX + i * (D + 1);
        double p = b, cs = b * h[D];
        for (int q = 0; q < D; ++q) {
            const double xs = x[i * D + q] * il[(size_t)q];
            p += xs * xs;
            cs += xs * h[q];
        }
        const double r = cs / (p + 1.0);
        for (int q = 0; q < D; ++q) put(i, q, il[(size_t)q] * (h[q] - il[(size_t)q] * x[i * D + q] * r));
    }
}
// The device reductions of one part's dK/dX and their host finish.  W (ld ldw): the weights, rows = the nr points xr that are
// summed over, columns = the n points xc the gradient is taken at (both scaled for the part, dimension-major; Linear does not
// read xc); StdPeriodic alone reads W transposed unless s.wt.  x_host: the unscaled points of xc (n x D).  put(row, q, g)
// receives every element.  Synchronises st.
struct GradXScratch {
    double* H;                         // H = W * (dK/dr)/r (may be W itself), ld ldh
    long ldh;
    double *part, *col, *hx;           // theta partials (unused here), column partials 64 x n x (D + 1), their sum n x (D + 1)
    double* host;                      // n x (D + 1) on the host
    int wt;                            // StdPeriodic: W is indexed [xr point][xc point] like the other kinds' weights
};
template <class Part, class Put>
static int part_gradients_X(hipStream_t st, const Part& pt, const double* W, long ldw, const double* xr, long ldr, long nr,
                            const double* xc, long ldc, long n, const double* x_host, int D, const GradXScratch& s, Put put) {
    auto fetch = [&](long cnt) -> int {
        HIP_CHECK(hipMemcpyAsync(s.host, s.hx, sizeof(double) * cnt, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        return 0;
    };
    if (pt.linear()) {
        // dK(x_i, x2_j)/dx_iq = variance_q x2_jq (linear.py:108-114): the column reduction W^T x2~ of the weights themselves
        const int ns = launch_colreduce_multi(st, W, ldw, nr, n, xr, 1, ldr, D, 0, s.col);
        launch_sum_splits(st, s.col, n * D, ns, 0, s.hx);
        if (int rc = fetch(n * D)) return rc;
        gradx_linear(pt.inv_ls, n, D, s.host, put);
    } else if (pt.kp.kind == MI355GP_STDPERIODIC) {             // not a function of r: the row reduction instead of H
        launch_periodic_gradx(st, pt.kp, xc, ldc, n, xr, ldr, nr, W, ldw, s.wt, s.hx);
        if (int rc = fetch(n * D)) return rc;
        gradx_periodic(pt.pw, n, D, s.host, put);
    } else {
        launch_grad_generic(st, pt.kp, xr, ldr, nr, xc, ldc, n, 0, W, ldw, s.part, s.H, s.ldh);
        const int ns = launch_colreduce_multi(st, s.H, s.ldh, nr, n, xr, 1, ldr, D, 1, s.col);
        launch_sum_splits(st, s.col, n * (D + 1), ns, 0, s.hx);
        if (int rc = fetch(n * (D + 1))) return rc;
        // MLP: H = c of the weights (k_grad_dot); dK/dx from H^T [x2~ | 1] (mlp.py:124-130)
        if (pt.mlp()) gradx_mlp(x_host, n, D, pt.inv_ls, pt.kp.bias, s.host, put);
        else gradx_stationary(x_host, n, D, pt.inv_ls, s.host, put);       // (il = 0 outside active_dims)
    }
    return 0;
}
// Kdiag of an MLP part at one point and its derivative factor (mlp.py:61-64,133-147): p = sum_q w_q x_q^2 + b over the active
// columns; Kdiag = var (2/pi) asin(p / (p + 1)), dKdiag/dx_q = 2 cd w_q x_q with cd = var (2/pi) / (sqrt(1 - (p/(p+1))^2) (p+1)^2)
static inline double mlp_point_p(const PartSpec& p, const double* x) {
    double s = p.kp.bias;
    for (size_t a = 0; a < p.dims.size(); ++a) s += p.theta[1 + (p.kp.ard ? a : 0)] * x[p.dims[a]] * x[p.dims[a]];
    return s;
}
static inline double mlp_kdiag(const PartSpec& p, const double* x) {
    const double s = mlp_point_p(p, x);
    return p.kp.variance * M_2_PI * std::asin(s / (s + 1.0));
}
static inline double mlp_dkdiag_factor(const PartSpec& p, const double* x) {
    const double s = mlp_point_p(p, x), t = s / (s + 1.0);
    return p.kp.variance * M_2_PI / (std::sqrt(1.0 - t * t) * (s + 1.0) * (s + 1.0));
}
// Kdiag of a Poly part at one point (poly.py:33-34: the diagonal of K): var (scale |x|^2 + bias)^order
static inline double poly_kdiag(const PartSpec& p, const double* x) {
    double d = 0.0;
    for (size_t a = 0; a < p.dims.size(); ++a) d += x[p.dims[a]] * x[p.dims[a]];
    return p.kp.variance * std::pow(p.theta[1] * d + p.kp.bias, p.kp.power);
}
