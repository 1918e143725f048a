// The least-squares rigid fit of csrc/ransac_register.hip (Horn 1987): given correspondences (x_m, y_m), the rotation R and
// translation t that minimise sum_m |x_m - (R y_m + t)|^2, so that (R, t) takes y's frame into x's.  Centroids, the
// cross-covariance C = sum_m (x_m - xbar)(y_m - ybar)^T, the projection of rotation_math.h (R maximises tr(R^T C); margin =
// (s2 + d s3) / s1 of C's singular values) and t = xbar - R ybar.  Plain C++ on doubles, compiled into the kernels by hipcc
// and into a host program by any C++ compiler (tools/rigid_fit_host.cpp, which tests/test_ransac_host.py builds with the
// address and undefined-behaviour sanitizers and compares with numpy's SVD).  Sums run in ascending m.
#pragma once
#include "rotation_math.h"

namespace epn_fit {

// C += (x - xbar)(y - ybar)^T, row-major
EPN_ROT_FN void cov_add(double C[9], const double x[3], const double xbar[3], const double y[3], const double ybar[3]) {
    const double dx[3] = {x[0] - xbar[0], x[1] - xbar[1], x[2] - xbar[2]};
    const double dy[3] = {y[0] - ybar[0], y[1] - ybar[1], y[2] - ybar[2]};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[3 * i + j] += dx[i] * dy[j];
}

// (centroids, C) -> R (row-major), t, margin
EPN_ROT_FN void fit_finish(const double xbar[3], const double ybar[3], const double C[9], double R[9], double t[3],
                           double &margin) {
    epn_rot::so3_project(C, R, margin);
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = xbar[i] - (R[3 * i] * ybar[0] + R[3 * i + 1] * ybar[1] + R[3 * i + 2] * ybar[2]);
}

// |x - (R y + t)|^2 with every product-sum an explicit fma: the same bits in every kernel and on the host, whatever the
// compiler's contraction setting, so a correspondence is an inlier of (R, t) or not wherever that is asked
EPN_ROT_FN double sq_residual(const double R[9], const double t[3], const double x[3], const double y[3]) {
    double d2 = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double d = x[i] - fma(R[3 * i], y[0], fma(R[3 * i + 1], y[1], fma(R[3 * i + 2], y[2], t[i])));
        d2 = fma(d, d, d2);
    }
    return d2;
}

// The fit of n >= 1 correspondences held as x[3 m + i], y[3 m + i].  n = 1, coincident or collinear points: C has rank < 2,
// margin = 0 (or next to it) and R is one of the maximisers; it is still a rotation.
EPN_ROT_FN void rigid_fit(const double *x, const double *y, int n, double R[9], double t[3], double &margin) {
    double xbar[3] = {0.0, 0.0, 0.0}, ybar[3] = {0.0, 0.0, 0.0}, C[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int m = 0; m < n; ++m)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            xbar[i] += x[3 * m + i];
            ybar[i] += y[3 * m + i];
        }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        xbar[i] /= (double)n;
        ybar[i] /= (double)n;
    }
    for (int m = 0; m < n; ++m) cov_add(C, x + 3 * m, xbar, y + 3 * m, ybar);
    fit_finish(xbar, ybar, C, R, t, margin);
}

}  // namespace epn_fit
