// The arithmetic of csrc/rotation_decode.hip and csrc/rotation_loss.hip that needs no device: the quaternion's rotation matrix,
// the two rotation maps of the head's output, the projection of a 3 x 3 matrix onto SO(3) with its conditioning margin, and
// acos_safe.  Plain C++ on doubles, compiled into the kernels by hipcc and
// into a host program by any C++ compiler (tools/so3_project_host.cpp, which tests/test_rotation_host.py builds with the
// address and undefined-behaviour sanitizers and compares with numpy's SVD at every conditioning).
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define EPN_ROT_FN __device__ __forceinline__
#else
#define EPN_ROT_FN static inline
#endif

namespace epn_rot {

constexpr int JACOBI_SWEEPS = 12;        // 4 x 4 symmetric, fp64: converged after 5-6; the rest are no-ops

// rotation matrix (row-major) of a quaternion (w, x, y, z) taken as it is: rotation.py:400-415
EPN_ROT_FN void quat_matrix(const double q[4], double R[9]) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, xw = x * w, yw = y * w, zw = z * w;
    R[0] = 1.0 - 2.0 * yy - 2.0 * zz; R[1] = 2.0 * xy - 2.0 * zw;       R[2] = 2.0 * xz + 2.0 * yw;
    R[3] = 2.0 * xy + 2.0 * zw;       R[4] = 1.0 - 2.0 * xx - 2.0 * zz; R[5] = 2.0 * yz - 2.0 * xw;
    R[6] = 2.0 * xz - 2.0 * yw;       R[7] = 2.0 * yz + 2.0 * xw;       R[8] = 1.0 - 2.0 * xx - 2.0 * yy;
}

// v / max(|v|, 1e-8) in place: normalize_vector of rotation.py:381-390.  -> |v| as it was, before the clamp
EPN_ROT_FN double normalize(double *v, int n) {
    double s = 0.0;
    for (int e = 0; e < n; ++e) s += v[e] * v[e];
    const double norm = sqrt(s), mag = fmax(norm, 1e-8);
    for (int e = 0; e < n; ++e) v[e] /= mag;
    return norm;
}

EPN_ROT_FN void cross(const double u[3], const double v[3], double o[3]) {
    o[0] = u[1] * v[2] - u[2] * v[1];
    o[1] = u[2] * v[0] - u[0] * v[2];
    o[2] = u[0] * v[1] - u[1] * v[0];
}

// The two rotation maps of the head's y entries (rotation.py:379-417 and :443-478), shared by the decode and the loss.
// NR = 4: v <- q / max(|q|, 1e-8), R = quat_matrix(v), norms[0] = norms[1] = |q|.  NR = 6: x = n(v[0:3]), z = n(x cross v[3:6]),
// y = z cross x, n(u) = u / max(|u|, 1e-8); R's columns are (x, y, z), norms = (|v[0:3]|, |x cross v[3:6]|) and v[0:3] <- x
// (v[3:6] stays as it was): what a backward through the map needs besides R.
template <int NR>
EPN_ROT_FN void rotation_map(double v[NR], double R[9], double norms[2]) {
    if (NR == 4) {
        norms[0] = norms[1] = normalize(v, 4);
        quat_matrix(v, R);
    } else {
        double x[3] = {v[0], v[1], v[2]}, yr[3] = {v[NR - 3], v[NR - 2], v[NR - 1]}, z[3], yy[3];
        norms[0] = normalize(x, 3);
        cross(x, yr, z);
        norms[1] = normalize(z, 3);
        cross(z, x, yy);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            R[3 * i] = x[i];
            R[3 * i + 1] = yy[i];
            R[3 * i + 2] = z[i];
            v[i] = x[i];
        }
    }
}

// The rotation R maximising tr(R^T Ce) and margin = (s2 + det(U V^T) s3) / s1 of Ce's singular values.
// sum_ij R(q)_ij Ce_ij = q^T K q with K below (q = (w, x, y, z)); K's eigenvalues are s1+s2+d s3 >= s1-s2-d s3 >=
// -s1+s2-d s3 >= -s1-s2+d s3, so the top eigenvector is q, l1 + l2 = 2 s1 and l1 - l2 = 2 (s2 + d s3).
EPN_ROT_FN void so3_project(const double C[9], double R[9], double &margin) {
    double K[4][4], V[4][4];
    K[0][0] = C[0] + C[4] + C[8];
    K[1][1] = C[0] - C[4] - C[8];
    K[2][2] = -C[0] + C[4] - C[8];
    K[3][3] = -C[0] - C[4] + C[8];
    K[0][1] = K[1][0] = C[7] - C[5];
    K[0][2] = K[2][0] = C[2] - C[6];
    K[0][3] = K[3][0] = C[3] - C[1];
    K[1][2] = K[2][1] = C[1] + C[3];
    K[1][3] = K[3][1] = C[2] + C[6];
    K[2][3] = K[3][2] = C[5] + C[7];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double apq = K[p][q];
                // the rotation that zeroes K[p][q]: t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)), |t| <= 1
                const double theta = (K[q][q] - K[p][p]) / (2.0 * apq);
                double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
                if (!(fabs(theta) < 1e150)) t = 0.5 / theta;          // theta^2 would overflow; inf (apq == 0) gives t = 0
                if (apq == 0.0) t = 0.0;
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int k = 0; k < 4; ++k) {                          // K <- K J
                    const double kp = K[k][p], kq = K[k][q];
                    K[k][p] = c * kp - s * kq;
                    K[k][q] = s * kp + c * kq;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {                          // K <- J^T K,  V <- V J
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
    // largest and second-largest diagonal entry, the lowest index on a tie
    int top = 0;
    double l1 = K[0][0], l2 = -INFINITY;
    double q[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (K[i][i] > l1) {
            top = i;
            l1 = K[i][i];
            q[0] = V[0][i]; q[1] = V[1][i]; q[2] = V[2][i]; q[3] = V[3][i];
        }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i != top && K[i][i] > l2) l2 = K[i][i];
    double n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    if (!(n2 > 0.25 && n2 < 4.0)) {                                    // only with non-finite input: keep R a finite matrix
        q[0] = 1.0; q[1] = q[2] = q[3] = 0.0;
        n2 = 1.0;
    }
    const double inv = 1.0 / sqrt(n2);
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] *= inv;
    quat_matrix(q, R);
    const double s1x2 = l1 + l2;                                       // 2 s1
    margin = s1x2 > 0.0 ? (l1 - l2) / s1x2 : 0.0;
}

// acos_safe of vgtk/vgtk/spconv/functional.py:138-143, eps = 1e-4
EPN_ROT_FN double acos_safe(double x) {
    const double eps = 1e-4;
    if (fabs(x) <= 1.0 - eps) return acos(x);
    const double sign = x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0);
    const double slope = acos(1.0 - eps) / eps;
    return acos(sign * (1.0 - eps)) - slope * sign * (fabs(x) - 1.0 + eps);
}

}  // namespace epn_rot
