// Host program around csrc/fpfh_math.h: the pair features, the bins and the fixed-point weighting that the FPFH kernels run,
// compiled for the CPU.  Reads records from standard input, or runs three built-in ones when the input is empty:
//   "pair p_i(3) n_i(3) p_k(3) n_k(3)"   two oriented points (fp32 values)
//        -> the three bins, then the three values whose floors they are
//   "term d2min d2k c used"              one neighbour's share of one bin of the weighted sum -> the int64 term
//   "value A G c used"                   -> the fp32 entry (100 A) / G + (100 c) / used
// 17 significant digits for fp64, 9 for fp32.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined tools/fpfh_host.cpp -o fpfh_host
// tests/test_fpfh_host.py builds it like that and compares with the numpy restatement (tests/fpfh_ref.py).
#include <cstdio>
#include <cstring>

#include "../epn_pointcloud_amd/csrc/fpfh_math.h"

static void pair(const double in[12]) {
    float a[12];
    for (int e = 0; e < 12; ++e) a[e] = (float)in[e];
    double f[3], t[3];
    epn_fpfh::pair_features(a, a + 3, a + 6, a + 9, f);
    epn_fpfh::bin_values(f, t);
    printf("%d %d %d %.17g %.17g %.17g\n", epn_fpfh::bin_of(t[0]), epn_fpfh::bin_of(t[1]), epn_fpfh::bin_of(t[2]), t[0], t[1], t[2]);
}

static void builtin() {
    // the neighbour along x, both normals +z: f = (0, 0, 0) -> the middle bins; then coinciding points; then d parallel to n
    const double along[12] = {0, 0, 0, 0, 0, 1, 0.25, 0, 0, 0, 0, 1};
    const double same[12] = {0.5, 0.5, 0.5, 0, 0, 1, 0.5, 0.5, 0.5, 1, 0, 0};
    const double up[12] = {0, 0, 0, 0, 0, 1, 0, 0, 0.25, 0, 1, 0};
    pair(along);
    pair(same);
    pair(up);
}

int main() {
    char kind[16];
    int records = 0;
    while (scanf("%15s", kind) == 1) {
        ++records;
        if (!strcmp(kind, "pair")) {
            double in[12];
            for (int e = 0; e < 12; ++e)
                if (scanf("%lf", &in[e]) != 1) return 3;
            pair(in);
        } else if (!strcmp(kind, "term")) {
            double d2min, d2k;
            int c, used;
            if (scanf("%lf %lf %d %d", &d2min, &d2k, &c, &used) != 4) return 3;
            if (!(d2k > 0.0) || used < 1 || c < 0 || c > used) return 2;
            printf("%lld\n", epn_fpfh::weighted_term((float)d2min, (float)d2k, c, used));
        } else if (!strcmp(kind, "value")) {
            long long A, G;
            int c, used;
            if (scanf("%lld %lld %d %d", &A, &G, &c, &used) != 4) return 3;
            if (used < 1) return 2;
            printf("%.9g\n", epn_fpfh::fpfh_value(A, G, c, used));
        } else {
            return 2;
        }
    }
    if (!records) builtin();
    return 0;
}
