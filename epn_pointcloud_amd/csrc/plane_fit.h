// The arithmetic of csrc/point_normals.hip that needs no device: from the fixed-point moments of a neighbourhood to its plane
// (covariance, the eigen-solve of the symmetric 3 x 3, the sign of the normal), and the frame of a patch from its normal.  Plain
// C++ on doubles, compiled into the kernels by hipcc and into a host program by any C++ compiler (tools/plane_fit_host.cpp, which
// tests/test_plane_fit_host.py builds with the address and undefined-behaviour sanitizers and compares with numpy's eigh).
// Specification: include/epn_so3conv.h (epn_point_normals_f32, epn_orient_patches_f32) and DESIGN.md 3.1k.
// Every function keeps its products and sums apart (no fma contraction), so the host and the device build round alike.
#pragma once
#include <cmath>

#include "rotation_math.h"

#if defined(__clang__)
#define EPN_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define EPN_NO_CONTRACT
#endif

namespace epn_plane {

constexpr int JACOBI_SWEEPS = 10;        // 3 x 3 symmetric, fp64: converged after 4-5; the rest are no-ops
constexpr double FIX = 0x1p40;           // the moments' fixed point: units of 2^-40
constexpr double GAP_MIN = 0x1p-40;      // flag bit 2: lambda1 - lambda0 at or below it, in the units of C
constexpr int FLAG_FEW = 1, FLAG_QUERY = 2, FLAG_GAP = 4;

// t = ((double)p - (double)q) / radius on one axis: two fp64 operations, each rounded once
EPN_ROT_FN double scaled_offset(float p, float q, double radius) {
    EPN_NO_CONTRACT
    const double d = (double)p - (double)q;
    return d / radius;
}

// One neighbour's contribution to {S_x, S_y, S_z, M_xx, M_xy, M_xz, M_yy, M_yz, M_zz}: rint(t_i 2^40) and rint((t_i t_j) 2^40),
// the product rounded once before the (exact) scaling.  |t| < 1 + 2^-20, so every term is below 2^41.
EPN_ROT_FN void moments_add(long long mom[9], double tx, double ty, double tz) {
    EPN_NO_CONTRACT
    const double xx = tx * tx, xy = tx * ty, xz = tx * tz, yy = ty * ty, yz = ty * tz, zz = tz * tz;
    mom[0] += llrint(tx * FIX); mom[1] += llrint(ty * FIX); mom[2] += llrint(tz * FIX);
    mom[3] += llrint(xx * FIX); mom[4] += llrint(xy * FIX); mom[5] += llrint(xz * FIX);
    mom[6] += llrint(yy * FIX); mom[7] += llrint(yz * FIX); mom[8] += llrint(zz * FIX);
}

// mean_i = (S_i / 2^40) / used, C_ij = (M_ij / 2^40) / used - mean_i mean_j; C = {xx, xy, xz, yy, yz, zz}
EPN_ROT_FN void covariance(const long long mom[9], int used, double C[6]) {
    EPN_NO_CONTRACT
    const double k = (double)used;
    const double mx = ((double)mom[0] / FIX) / k, my = ((double)mom[1] / FIX) / k, mz = ((double)mom[2] / FIX) / k;
    const double mxx = mx * mx, mxy = mx * my, mxz = mx * mz, myy = my * my, myz = my * mz, mzz = mz * mz;
    C[0] = ((double)mom[3] / FIX) / k - mxx;
    C[1] = ((double)mom[4] / FIX) / k - mxy;
    C[2] = ((double)mom[5] / FIX) / k - mxz;
    C[3] = ((double)mom[6] / FIX) / k - myy;
    C[4] = ((double)mom[7] / FIX) / k - myz;
    C[5] = ((double)mom[8] / FIX) / k - mzz;
}

// Eigenvalues (ascending, the lowest index first on a tie) and the unit eigenvector of lam[0], by the cyclic Jacobi of
// rotation_math.h's so3_project on a 3 x 3.  A sweep that finds all three off-diagonal entries zero would change nothing (t = 0,
// c = 1, s = 0), so the loop ends there: the result is that of the full count.
EPN_ROT_FN void eigen_sym3(const double C[6], double lam[3], double nrm[3]) {
    EPN_NO_CONTRACT
    double K[3][3] = {{C[0], C[1], C[2]}, {C[1], C[3], C[4]}, {C[2], C[4], C[5]}};
    double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
        if (K[0][1] == 0.0 && K[0][2] == 0.0 && K[1][2] == 0.0) break;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
#pragma unroll
            for (int q = p + 1; q < 3; ++q) {
                const double apq = K[p][q];
                // the rotation that zeroes K[p][q]: t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)), |t| <= 1
                const double theta = (K[q][q] - K[p][p]) / (2.0 * apq);
                double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
                if (!(fabs(theta) < 1e150)) t = 0.5 / theta;          // theta^2 would overflow; inf (apq == 0) gives t = 0
                if (apq == 0.0) t = 0.0;
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int k = 0; k < 3; ++k) {                          // K <- K J
                    const double kp = K[k][p], kq = K[k][q];
                    K[k][p] = c * kp - s * kq;
                    K[k][q] = s * kp + c * kq;
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) {                          // K <- J^T K,  V <- V J
                    const double kp = K[p][k], kq = K[q][k];
                    K[p][k] = c * kp - s * kq;
                    K[q][k] = s * kp + c * kq;
                    const double vp = V[k][p], vq = V[k][q];
                    V[k][p] = c * vp - s * vq;
                    V[k][q] = s * vp + c * vq;
                }
            }
        }
    }
    // ascending diagonal, the lowest index first among equals (a stable three-element sort)
    const double d0 = K[0][0], d1 = K[1][1], d2 = K[2][2];
    int i0 = 0, i1 = 1, i2 = 2;
    double a = d0, b = d1, c2 = d2;
    if (b < a) { const double t = a; a = b; b = t; const int i = i0; i0 = i1; i1 = i; }
    if (c2 < b) { const double t = b; b = c2; c2 = t; const int i = i1; i1 = i2; i2 = i; }
    if (b < a) { const double t = a; a = b; b = t; const int i = i0; i0 = i1; i1 = i; }
    lam[0] = a; lam[1] = b; lam[2] = c2;
    double v[3] = {i0 == 0 ? V[0][0] : (i0 == 1 ? V[0][1] : V[0][2]), i0 == 0 ? V[1][0] : (i0 == 1 ? V[1][1] : V[1][2]),
                   i0 == 0 ? V[2][0] : (i0 == 1 ? V[2][1] : V[2][2])};
    double n2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    if (!(n2 > 0.25 && n2 < 4.0)) {                                    // only with non-finite input: keep the normal finite
        v[0] = 0.0; v[1] = 0.0; v[2] = 1.0;
        n2 = 1.0;
    }
    const double norm = sqrt(n2);
    nrm[0] = v[0] / norm; nrm[1] = v[1] / norm; nrm[2] = v[2] / norm;
}

// The sign of a normal.  With a viewpoint (has_view; view is not read without): n . (view - q) >= 0.  Without: the component of
// largest magnitude is positive, the lowest axis on a tie.
EPN_ROT_FN void orient(double n[3], const double q[3], bool has_view, const double view[3]) {
    EPN_NO_CONTRACT
    bool flip;
    if (has_view) {
        const double d = (n[0] * (view[0] - q[0]) + n[1] * (view[1] - q[1])) + n[2] * (view[2] - q[2]);
        flip = d < 0.0;
    } else {
        int top = 0;
        if (fabs(n[1]) > fabs(n[top])) top = 1;
        if (fabs(n[2]) > fabs(n[top])) top = 2;
        flip = (top == 0 ? n[0] : (top == 1 ? n[1] : n[2])) < 0.0;
    }
    if (flip) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
}

// moments of `used` neighbours of the query q -> the normal and the eigenvalues in fp64 (lam in the units of C); returns the
// flag bits 0 (used < 3: the normal is (0, 0, 1), whatever the viewpoint, and lam is zero) and 2 (lam[1] - lam[0] <= 2^-40).
EPN_ROT_FN int plane_fit_f64(const long long mom[9], int used, const double q[3], bool has_view, const double view[3],
                             double n[3], double lam[3]) {
    if (used < 3) {
        n[0] = 0.0; n[1] = 0.0; n[2] = 1.0;
        lam[0] = lam[1] = lam[2] = 0.0;
        return FLAG_FEW;
    }
    double C[6];
    covariance(mom, used, C);
    eigen_sym3(C, lam, n);
    orient(n, q, has_view, view);
    return lam[1] - lam[0] <= GAP_MIN ? FLAG_GAP : 0;
}

// the same, rounded once to what the entry point writes: normal f32[3], eig = lam * radius^2 f32[3]
EPN_ROT_FN int plane_fit(const long long mom[9], int used, double radius, const double q[3], bool has_view, const double view[3],
                         float normal[3], float eig[3]) {
    EPN_NO_CONTRACT
    double n[3], lam[3];
    const int flags = plane_fit_f64(mom, used, q, has_view, view, n, lam);
    const double r2 = radius * radius;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        normal[e] = (float)n[e];
        eig[e] = (float)(lam[e] * r2);
    }
    return flags;
}

// The frame of a patch from its normal, the reference's transform_with_normals (SPConvNets/datasets/match_3dmatch.py:141-152)
// restated: u(v) = v / (|v| + 1e-5) with |v| = sqrt((v0 v0 + v1 v1) + v2 v2); z = u(n), x = u(up cross z) with up = (0, -1, 0),
// y = u(z cross x); axis (row-major 3 x 3) has x, y, z as its columns, rounded once to fp32.
EPN_ROT_FN void unit_eps(const double v[3], double o[3]) {
    EPN_NO_CONTRACT
    const double s = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    const double d = sqrt(s) + 1e-5;
    o[0] = v[0] / d; o[1] = v[1] / d; o[2] = v[2] / d;
}

EPN_ROT_FN void cross3(const double u[3], const double v[3], double o[3]) {
    EPN_NO_CONTRACT
    const double a0 = u[1] * v[2], b0 = u[2] * v[1], a1 = u[2] * v[0], b1 = u[0] * v[2], a2 = u[0] * v[1], b2 = u[1] * v[0];
    o[0] = a0 - b0;
    o[1] = a1 - b1;
    o[2] = a2 - b2;
}

EPN_ROT_FN void patch_frame(const float normal[3], float axis[9]) {
    const double n[3] = {(double)normal[0], (double)normal[1], (double)normal[2]}, up[3] = {0.0, -1.0, 0.0};
    double x[3], y[3], z[3], c[3];
    unit_eps(n, z);
    cross3(up, z, c);
    unit_eps(c, x);
    cross3(z, x, c);
    unit_eps(c, y);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        axis[3 * i] = (float)x[i];
        axis[3 * i + 1] = (float)y[i];
        axis[3 * i + 2] = (float)z[i];
    }
}

// one row of patch @ axis: component j = ((p0 a0j + p1 a1j) + p2 a2j) in fp64 (the products of fp32 values are exact there)
EPN_ROT_FN void rotate_row(const float p[3], const float axis[9], float o[3]) {
    EPN_NO_CONTRACT
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double a = (double)p[0] * (double)axis[j], b = (double)p[1] * (double)axis[3 + j], c = (double)p[2] * (double)axis[6 + j];
        const double ab = a + b;
        o[j] = (float)(ab + c);
    }
}

}  // namespace epn_plane
