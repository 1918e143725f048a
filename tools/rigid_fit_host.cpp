// Host program around csrc/rigid_fit.h: the least-squares rigid fit that the registration kernels run, compiled for the CPU.
// Reads sets of correspondences from standard input -- a count n >= 1, then n lines "x0 x1 x2 y0 y1 y2" -- and prints, per set,
// the nine entries of R, the three of t, the margin and the sum of the squared residuals |x - (R y + t)|^2, 17 significant
// digits.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined tools/rigid_fit_host.cpp -o rigid_fit_host
// tests/test_ransac_host.py builds it like that and compares with numpy's SVD.
#include <cstdio>
#include <vector>

#include "../epn_pointcloud_amd/csrc/rigid_fit.h"

int main() {
    int n;
    while (scanf("%d", &n) == 1) {
        if (n < 1 || n > (1 << 20)) return 2;
        std::vector<double> x(3 * (size_t)n), y(3 * (size_t)n);
        for (int m = 0; m < n; ++m)
            if (scanf("%lf %lf %lf %lf %lf %lf", &x[3 * m], &x[3 * m + 1], &x[3 * m + 2], &y[3 * m], &y[3 * m + 1], &y[3 * m + 2]) != 6)
                return 3;
        double R[9], t[3], margin, sq = 0.0;
        epn_fit::rigid_fit(x.data(), y.data(), n, R, t, margin);
        for (int m = 0; m < n; ++m) sq += epn_fit::sq_residual(R, t, &x[3 * m], &y[3 * m]);
        for (int e = 0; e < 9; ++e) printf("%.17g ", R[e]);
        printf("%.17g %.17g %.17g %.17g %.17g\n", t[0], t[1], t[2], margin, sq);
    }
    return 0;
}
