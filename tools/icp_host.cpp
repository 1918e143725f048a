// Host program around csrc/icp_math.h: the arithmetic of the ICP stage (csrc/icp_refine.hip), compiled for the CPU.
// Reads commands from standard input, one per line, and answers each with one line of 17-significant-digit numbers:
//   step <plane 0|1> <m> <iter> <rel_fitness> <rel_rmse> <prev_fitness> <prev_rmse> <T: 16 doubles> <S: 32 integers>
//        -> flags prev_fitness prev_rmse rec[20]                               (epn_icp::step)
//   cayley <w0> <w1> <w2>                      -> R[9]                          (epn_icp::cayley)
//   terms <plane 0|1> <p: 3> <q: 3> <n: 3>     -> bad, then the 32 terms of the pair as integers (p2p_values / plane_values,
//                                                 term_of, term); the values are read as doubles and narrowed to fp32
//   transform <T: 12 doubles> <s: 3>           -> q[3]                          (epn_icp::transform_point)
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined tools/icp_host.cpp -o icp_host
// tests/test_icp_host.py builds it like that and compares with tests/icp_ref.py.
#include <cstdio>
#include <cstring>

#include "../epn_pointcloud_amd/csrc/icp_math.h"

using namespace epn_icp;

static bool read_doubles(double *v, int n) {
    for (int i = 0; i < n; ++i)
        if (scanf("%lf", &v[i]) != 1) return false;
    return true;
}

int main() {
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        if (!strcmp(cmd, "step")) {
            int plane, iter;
            long long m, S[NS];
            double h[4], T[16], rec[REC];
            if (scanf("%d %lld %d", &plane, &m, &iter) != 3 || !read_doubles(h, 4) || !read_doubles(T, 16)) return 3;
            for (int e = 0; e < NS; ++e)
                if (scanf("%lld", &S[e]) != 1) return 3;
            if (m < 1) return 2;
            double pf = h[2], pr = h[3];
            const int flags = step(plane != 0, S, m, iter, h[0], h[1], pf, pr, T, rec);
            printf("%d %.17g %.17g", flags, pf, pr);
            for (int e = 0; e < REC; ++e) printf(" %.17g", rec[e]);
            printf("\n");
        } else if (!strcmp(cmd, "cayley")) {
            double w[3], R[9];
            if (!read_doubles(w, 3)) return 3;
            cayley(w, R);
            for (int e = 0; e < 9; ++e) printf("%.17g ", R[e]);
            printf("\n");
        } else if (!strcmp(cmd, "terms")) {
            int plane;
            double v[9];
            if (scanf("%d", &plane) != 1 || !read_doubles(v, 9)) return 3;
            const float p[3] = {(float)v[0], (float)v[1], (float)v[2]}, q[3] = {(float)v[3], (float)v[4], (float)v[5]};
            const float n[3] = {(float)v[6], (float)v[7], (float)v[8]};
            const Values V = plane ? plane_values(p, q, n) : p2p_values(p, q);
            const bool bad = V.bad;
            printf("%d", (int)bad);
            for (int e = 0; e < NS; ++e) {
                int ia, ib;
                double scale;
                term_of(plane != 0, e, ia, ib, scale);
                printf(" %lld", bad ? 0ll : term(value_at(V, ia), value_at(V, ib), scale));
            }
            printf("\n");
        } else if (!strcmp(cmd, "transform")) {
            double T[12], s[3];
            if (!read_doubles(T, 12) || !read_doubles(s, 3)) return 3;
            const float sf[3] = {(float)s[0], (float)s[1], (float)s[2]};
            float q[3];
            transform_point(T, sf, q);
            printf("%.9g %.9g %.9g\n", q[0], q[1], q[2]);
        } else {
            return 4;
        }
    }
    return 0;
}
