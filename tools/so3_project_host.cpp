// Host program around csrc/rotation_math.h: the projection onto SO(3) that the rotation kernels run, compiled for the CPU.
// Reads 3 x 3 matrices (nine numbers each, row-major) from standard input and prints, per matrix, the nine entries of the
// rotation and the margin, 17 significant digits; then acos_safe of every number after a line "acos".
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined tools/so3_project_host.cpp -o so3_project_host
// tests/test_rotation_host.py builds it like that and compares with numpy's SVD.
#include <cstdio>
#include <cstring>

#include "../epn_pointcloud_amd/csrc/rotation_math.h"

int main() {
    double C[9], R[9], margin, x;
    char word[16];
    while (scanf("%lf %lf %lf %lf %lf %lf %lf %lf %lf", C, C + 1, C + 2, C + 3, C + 4, C + 5, C + 6, C + 7, C + 8) == 9) {
        epn_rot::so3_project(C, R, margin);
        for (int e = 0; e < 9; ++e) printf("%.17g ", R[e]);
        printf("%.17g\n", margin);
    }
    if (scanf("%15s", word) == 1 && strcmp(word, "acos") == 0)
        while (scanf("%lf", &x) == 1) printf("%.17g\n", epn_rot::acos_safe(x));
    return 0;
}
