// Host program around csrc/tsdf_math.h: the per-sample arithmetic of the TSDF fusion kernels (depth value, back-projection, unit
// index, projection and update, crossing), compiled for the CPU.  Reads records from standard input, or, on an empty input, runs
// every function over a built-in table of edge values (zeros, signed tiny and huge values, infinities, NaN) and prints "edges N":
//   "depth raw scale trunc"                                     -> d
//   "sample u v raw scale trunc fx fy cx cy sdf_trunc unit_length T0 .. T11"
//        -> d, the base-frame point (3), then lo and hi unit index per axis (6)
//   "voxel ux uy uz ix iy iz voxel_length fx fy cx cy W H T0 .. T11"   (T = base2cam's three rows)
//        -> the centre (3), the camera point (3), visible (0/1), pu, pv
//   "observe raw scale trunc z pu pv fx fy cx cy sdf_trunc tsdf w" -> observed (0/1), t, the updated tsdf and w
//   "cross f0 w0 f1 w1 p0 voxel_length"                         -> part0, part1, crosses, the coordinate
// 17 significant digits for fp64, 9 for fp32.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined tools/tsdf_host.cpp -o tsdf_host
// tests/test_tsdf_host.py builds it like that and compares with the numpy restatement (tests/tsdf_ref.py).
#include <cstdio>
#include <cstring>
#include <limits>

#include "../epn_pointcloud_amd/csrc/tsdf_math.h"

using namespace epn_tsdf;

static bool doubles(double *v, int n) {
    for (int e = 0; e < n; ++e)
        if (scanf("%lf", &v[e]) != 1) return false;
    return true;
}

static int edges() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double vals[] = {0.0, -0.0, 1.0, -1.0, 0.5, 5e-324, -5e-324, 1e-300, 0.09375, -0.09375, 3.0, 1e9, -1e9, 1e300, -1e300,
                           2147483647.0, 2147483648.0, -2147483649.0, inf, -inf, nan};
    const int n = (int)(sizeof(vals) / sizeof(vals[0]));
    const Camera cam = {585.0, 585.0, 320.0, 240.0};
    const double I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    int calls = 0;
    double sink = 0.0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const double a = vals[i], b = vals[j];
            double lo, hi, c[3] = {a, b, a}, q[3];
            int rel = 0, pu = 0, pv = 0;
            unit_span(a, 0.04, 0.09375, lo, hi);
            sink += box_offset(lo, -3, 7, rel) + box_offset(b, 0, 1 << 24, rel) + rel;
            transform(I, c, q);
            c[2] = b;
            if (project(c, cam, 640, 480, pu, pv)) sink += pu + pv;
            const Camera odd = {b > 0.0 && b < 1e300 ? b : 1.0, 585.0, a == a && a > -1e300 && a < 1e300 ? a : 0.0, 240.0};
            if (project(q, odd, 640, 480, pu, pv)) sink += pu + pv;
            float t = 0.0f, f = (float)a;
            int w = j;
            if (observe((float)a, b, i, j, cam, 0.04, t)) update(f, w, t);
            sink += takes_part((float)a, j) + crosses((float)a, (float)b) + (f == f);
            const float x = crossing((float)a, (float)b, 1.0, 3.0 / 512);
            sink += x == x;
            sink += depth_value((unsigned)(i * 3277), (float)(b > 0.0 ? b : 1000.0), a) + voxel_centre(i - 10, j % 16, 3.0 / 512);
            back_project(i, j, (float)(a > 0.0 && a < 100.0 ? a : 0.0), cam, q);
            calls += 12;
        }
    printf("edges %d %d\n", calls, sink == sink ? 1 : 0);
    return 0;
}

int main() {
    char kind[16];
    int records = 0;
    while (scanf("%15s", kind) == 1) {
        ++records;
        double v[32];
        if (!strcmp(kind, "depth")) {
            if (!doubles(v, 3) || v[0] < 0 || v[0] > 65535) return 3;
            printf("%.9g\n", depth_value((unsigned)v[0], (float)v[1], v[2]));
        } else if (!strcmp(kind, "sample")) {
            if (!doubles(v, 23) || v[2] < 0 || v[2] > 65535) return 3;
            const Camera cam = {v[5], v[6], v[7], v[8]};
            const float d = depth_value((unsigned)v[2], (float)v[3], v[4]);
            double c[3], p[3], lo[3], hi[3];
            back_project((int)v[0], (int)v[1], d, cam, c);
            transform(v + 11, c, p);
            for (int a = 0; a < 3; ++a) unit_span(p[a], v[9], v[10], lo[a], hi[a]);
            printf("%.9g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", d, p[0], p[1], p[2], lo[0], hi[0], lo[1], hi[1], lo[2],
                   hi[2]);
        } else if (!strcmp(kind, "voxel")) {
            if (!doubles(v, 25)) return 3;
            const Camera cam = {v[7], v[8], v[9], v[10]};
            double p[3], c[3];
            for (int a = 0; a < 3; ++a) p[a] = voxel_centre((int)v[a], (int)v[3 + a], v[6]);
            transform(v + 13, p, c);
            int pu = -1, pv = -1;
            const bool vis = project(c, cam, (int)v[11], (int)v[12], pu, pv);
            printf("%.17g %.17g %.17g %.17g %.17g %.17g %d %d %d\n", p[0], p[1], p[2], c[0], c[1], c[2], (int)vis, vis ? pu : -1,
                   vis ? pv : -1);
        } else if (!strcmp(kind, "observe")) {
            if (!doubles(v, 13) || v[0] < 0 || v[0] > 65535) return 3;
            const Camera cam = {v[6], v[7], v[8], v[9]};
            const float d = depth_value((unsigned)v[0], (float)v[1], v[2]);
            float t = 0.0f, f = (float)v[11];
            int w = (int)v[12];
            const bool seen = observe(d, v[3], (int)v[4], (int)v[5], cam, v[10], t);
            if (seen) update(f, w, t);
            printf("%d %.9g %.9g %d\n", (int)seen, t, f, w);
        } else if (!strcmp(kind, "cross")) {
            if (!doubles(v, 6)) return 3;
            const float f0 = (float)v[0], f1 = (float)v[2];
            const bool c = crosses(f0, f1);
            printf("%d %d %d %.9g\n", (int)takes_part(f0, (int)v[1]), (int)takes_part(f1, (int)v[3]), (int)c,
                   c ? crossing(f0, f1, v[4], v[5]) : 0.0f);
        } else {
            return 2;
        }
    }
    if (!records) return edges();
    return 0;
}
