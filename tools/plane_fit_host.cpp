// Host program around csrc/plane_fit.h: the plane fit that the normals kernel runs on a neighbourhood's fixed-point moments,
// and the frame of a patch, compiled for the CPU.  Reads records from standard input, or runs three built-in ones without
// arguments' worth of input (an empty input prints them):
//   "fit used radius q0 q1 q2 has_view v0 v1 v2 m0 .. m8"   the nine int64 moments of `used` neighbours of the query q
//        -> flags, the fp64 normal (3), the fp64 eigenvalues in the units of C (3), the fp32 normal (3) and eig (3) as written
//   "frame n0 n1 n2 p0 p1 p2"                               a normal and one patch row
//        -> the nine entries of axis (row-major, fp32) and the rotated row (3)
// 17 significant digits for fp64, 9 for fp32.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined tools/plane_fit_host.cpp -o plane_fit_host
// tests/test_plane_fit_host.py builds it like that and compares with numpy's eigh.
#include <cstdio>
#include <cstring>

#include "../epn_pointcloud_amd/csrc/plane_fit.h"

static void fit(int used, double radius, const double q[3], int has_view, const double v[3], const long long mom[9]) {
    double n[3], lam[3];
    float nf[3], ef[3];
    const int flags = epn_plane::plane_fit_f64(mom, used, q, has_view != 0, v, n, lam);
    const int again = epn_plane::plane_fit(mom, used, radius, q, has_view != 0, v, nf, ef);
    printf("%d %.17g %.17g %.17g %.17g %.17g %.17g %.9g %.9g %.9g %.9g %.9g %.9g\n", flags | again, n[0], n[1], n[2], lam[0], lam[1],
           lam[2], nf[0], nf[1], nf[2], ef[0], ef[1], ef[2]);
}

static void builtin() {
    const double q[3] = {0.0, 0.0, 0.0}, v[3] = {0.0, 0.0, -1.0};
    // the four corners (+-1/2, +-1/2, 0) of a square in z = 0, radius 1: S = 0, M_xx = M_yy = 4 * 2^38 = 2^40
    const long long square[9] = {0, 0, 0, 1LL << 40, 0, 0, 1LL << 40, 0, 0};
    fit(4, 1.0, q, 0, v, square);
    fit(4, 1.0, q, 1, v, square);
    fit(2, 1.0, q, 0, v, square);
}

int main() {
    char kind[16];
    int records = 0;
    while (scanf("%15s", kind) == 1) {
        ++records;
        if (!strcmp(kind, "fit")) {
            int used, has_view;
            double radius, q[3], v[3];
            long long mom[9];
            if (scanf("%d %lf %lf %lf %lf %d %lf %lf %lf", &used, &radius, &q[0], &q[1], &q[2], &has_view, &v[0], &v[1], &v[2]) != 9)
                return 3;
            for (int e = 0; e < 9; ++e)
                if (scanf("%lld", &mom[e]) != 1) return 3;
            if (used < 0 || used > (1 << 22)) return 2;
            fit(used, radius, q, has_view, v, mom);
        } else if (!strcmp(kind, "frame")) {
            double d[6];
            for (int e = 0; e < 6; ++e)
                if (scanf("%lf", &d[e]) != 1) return 3;
            const float nrm[3] = {(float)d[0], (float)d[1], (float)d[2]}, p[3] = {(float)d[3], (float)d[4], (float)d[5]};
            float axis[9], o[3];
            epn_plane::patch_frame(nrm, axis);
            epn_plane::rotate_row(p, axis, o);
            for (int e = 0; e < 9; ++e) printf("%.9g ", axis[e]);
            printf("%.9g %.9g %.9g\n", o[0], o[1], o[2]);
        } else {
            return 2;
        }
    }
    if (!records) builtin();
    return 0;
}
