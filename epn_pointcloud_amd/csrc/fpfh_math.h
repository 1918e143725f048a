// The arithmetic of csrc/fpfh.hip that needs no device: the three pair features of two oriented points, their bins, and the
// fixed-point weighting that turns the neighbours' simplified histograms into the FPFH row.  Plain C++ on doubles, compiled into
// the kernels by hipcc and into a host program by any C++ compiler (tools/fpfh_host.cpp, which tests/test_fpfh_host.py builds
// with the address and undefined-behaviour sanitizers and compares with the numpy restatement, tests/fpfh_ref.py).
// Specification: include/epn_so3conv.h (epn_point_fpfh_f32) and DESIGN.md 3.1n.  The steps are those of open3d's
// ComputePairFeatures / ComputeSPFHFeature / ComputeFPFHFeature, argued from open3d's algorithm, not run against it.
// Every function keeps its products and sums apart (no fma contraction), so the host and the device build round alike; what
// may still differ between two builds is atan2, by an ulp or two: the bin of f1 is the same unless 11 (f1 + pi) / (2 pi) lies
// within that of an integer (the "edge pairs" of tests/fpfh_ref.py).
//
// One deviation from open3d, stated: the roles of the two points are swapped when |a1| < |a2|, where open3d compares
// acos(|a1|) > acos(|a2|).  acos is strictly decreasing on [0, 1], so the two agree except where acos rounds two different
// arguments to one value (open3d then does not swap), and for |a| > 1 (normals that are not unit vectors), where acos is NaN
// and open3d never swaps.
// Range of the fixed point: a term is rint(w s 2^40) with w = d2min / d2_k <= 1 and s = c / used <= 1, so 0 <= term <= 2^40;
// the eleven s of a group add up to 1, so one neighbour's eleven terms of a group add up to at most 2^40 + 11; a point has fewer
// than 2^22 neighbours (n <= 2^22), so every bin's sum A and every group's sum G stays below 2^63.
#pragma once
#include <cmath>

#include "rotation_math.h"

#if defined(__clang__)
#define EPN_FPFH_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define EPN_FPFH_NO_CONTRACT
#endif

namespace epn_fpfh {

constexpr int BINS = 11, WIDTH = 33;     // three groups of eleven bins
constexpr double FIX = 0x1p40;           // the weighted sums' fixed point: units of 2^-40
constexpr double PI = 3.14159265358979323846;
constexpr int FLAG_ALONE = 1, FLAG_INPUT = 2;

EPN_ROT_FN double dot3(const double a[3], const double b[3]) {
    EPN_FPFH_NO_CONTRACT
    const double p0 = a[0] * b[0], p1 = a[1] * b[1], p2 = a[2] * b[2];
    const double s = p0 + p1;
    return s + p2;
}

// a x b = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0), every product rounded before its difference
EPN_ROT_FN void cross3(const double a[3], const double b[3], double o[3]) {
    EPN_FPFH_NO_CONTRACT
    const double x0 = a[1] * b[2], x1 = a[2] * b[1], y0 = a[2] * b[0], y1 = a[0] * b[2], z0 = a[0] * b[1], z1 = a[1] * b[0];
    o[0] = x0 - x1;
    o[1] = y0 - y1;
    o[2] = z0 - z1;
}

EPN_ROT_FN bool finite3(const float v[3]) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

// f = (f1, f2, f3) of the pair (query i, neighbour k): open3d's (phi, alpha, theta) order is f[0] = atan2(w . n2, n1 . n2),
// f[1] = v . n2, f[2] = the cosine between the source normal and d.  (0, 0, 0) for coinciding points, for d parallel to the
// source normal, and for a normal with a non-finite component (which open3d does not consider; a query with such a normal gets
// a zero row altogether, so this only settles what it adds to its neighbours' histograms).  Finite fp32 inputs cannot overflow
// fp64 here: the largest intermediate is |d x n1|^2 < 2^520.
EPN_ROT_FN void pair_features(const float pi[3], const float ni[3], const float pk[3], const float nk[3], double f[3]) {
    EPN_FPFH_NO_CONTRACT
    f[0] = f[1] = f[2] = 0.0;
    if (!finite3(ni) || !finite3(nk)) return;
    double d[3] = {(double)pk[0] - (double)pi[0], (double)pk[1] - (double)pi[1], (double)pk[2] - (double)pi[2]};
    const double len = sqrt(dot3(d, d));
    if (len == 0.0) return;
    const double a[3] = {(double)ni[0], (double)ni[1], (double)ni[2]}, b[3] = {(double)nk[0], (double)nk[1], (double)nk[2]};
    const double a1 = dot3(a, d) / len, a2 = dot3(b, d) / len;
    const bool swap = fabs(a1) < fabs(a2);
    const double *n1 = swap ? b : a, *n2 = swap ? a : b;
    double f3 = a1;
    if (swap) {
        d[0] = -d[0]; d[1] = -d[1]; d[2] = -d[2];
        f3 = -a2;
    }
    double v[3], w[3];
    cross3(d, n1, v);
    const double vn = sqrt(dot3(v, v));
    if (vn == 0.0) return;
    v[0] = v[0] / vn; v[1] = v[1] / vn; v[2] = v[2] / vn;
    cross3(n1, v, w);
    double y = dot3(w, n2);
    if (y == 0.0) y = 0.0;                                  // -0 counts as +0: atan2(-0, x < 0) would be -pi, the other end
    f[0] = atan2(y, dot3(n1, n2));
    f[1] = dot3(v, n2);
    f[2] = f3;
}

// The values whose floors are the bins: t1 = (11 (f1 + pi)) / (2 pi), t2 = (11 (f2 + 1)) 0.5, t3 = (11 (f3 + 1)) 0.5
EPN_ROT_FN void bin_values(const double f[3], double t[3]) {
    EPN_FPFH_NO_CONTRACT
    t[0] = (11.0 * (f[0] + PI)) / (2.0 * PI);
    t[1] = (11.0 * (f[1] + 1.0)) * 0.5;
    t[2] = (11.0 * (f[2] + 1.0)) * 0.5;
}

// floor, clamped to 0..10 while still a double (f3 of a non-unit normal may be far outside [-1, 1])
EPN_ROT_FN int bin_of(double t) {
    const double h = floor(t);
    return h < 0.0 ? 0 : (h > 10.0 ? 10 : (int)h);
}

// One neighbour's share of bin j of the weighted sum: rint(((d2min / d2_k) (c_k(j) / used_k)) 2^40), the two quotients and the
// product rounded once each, the scaling exact.  d2_k > 0, used_k >= 1 (the query is a neighbour of its neighbour).
EPN_ROT_FN long long weighted_term(float d2min, float d2k, int c, int used) {
    EPN_FPFH_NO_CONTRACT
    const double w = (double)d2min / (double)d2k;
    const double s = (double)c / (double)used;
    const double ws = w * s;
    return llrint(ws * FIX);
}

// fpfh(j) = (float)((100 A(j)) / G(g) + (100 c_i(j)) / used_i), the first quotient 0 when G == 0; used >= 1
EPN_ROT_FN float fpfh_value(long long A, long long G, int c, int used) {
    EPN_FPFH_NO_CONTRACT
    const double own = (100.0 * (double)c) / (double)used;
    double nb = 0.0;
    if (G != 0) nb = (100.0 * (double)A) / (double)G;
    return (float)(nb + own);
}

}  // namespace epn_fpfh
