// The per-sample arithmetic of csrc/tsdf_fusion.hip: a depth value, its back-projection, the unit index, a voxel's projection
// into a frame and the update of its (tsdf, weight), and the surface crossing between two voxels.  Plain C++ on doubles and
// floats, compiled into the kernels by hipcc and into a host program by any C++ compiler (tools/tsdf_host.cpp, which
// tests/test_tsdf_host.py builds with the address and undefined-behaviour sanitizers).
// Specification: include/epn_so3conv.h (epn_tsdf_fuse_f32, epn_tsdf_extract_f32) and DESIGN.md 3.1l.
// Every function keeps its products and sums apart (no fma contraction), so the host and the device build round alike.  The two
// fp32 quotients (the depth, the running mean) are taken as (float)((double)a / (double)b): for fp32 operands that IS the
// correctly rounded fp32 quotient (53 >= 2 * 24 + 2 bits: the second rounding cannot move it), whatever the compiler's fp32
// division does.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define EPN_TSDF_FN __host__ __device__ __forceinline__
#else
#define EPN_TSDF_FN static inline
#endif
#if defined(__clang__)
#define EPN_TSDF_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define EPN_TSDF_NO_CONTRACT
#endif

namespace epn_tsdf {

constexpr int UNIT = 16;                         // voxels per unit and axis (open3d's volume_unit_resolution)
constexpr int UNIT_VOX = UNIT * UNIT * UNIT;
constexpr int MAX_FRAMES = 64;                   // one bit of a unit's mask per frame
constexpr int MAX_IMAGE = 16384;                 // H, W
constexpr int MAX_UNIT_LO = 1 << 24;             // |unit_lo|: 16 * (unit_lo + dim) stays an int
constexpr long long MAX_DIRECTORY = 1ll << 24;
constexpr int MAX_BLOCKS = 1 << 17;              // 2^17 * 3 * 4096 points < 2^31
constexpr int FLAG_OUTSIDE = 1, FLAG_BLOCKS = 2; // epn_tsdf_fuse_f32's status[1]
constexpr int FLAG_POINTS = 1;                   // epn_tsdf_extract_f32's status[1]
constexpr float SURFACE_BAND = 0.98f;            // a voxel takes part in the extract when -0.98f <= tsdf < 0.98f

struct Camera {
    double fx, fy, cx, cy;
};

// d = (float)raw / (float)depth_scale in fp32; 0 ("no measurement") for raw == 0 and for d > depth_trunc (compared in fp64)
EPN_TSDF_FN float depth_value(unsigned raw, float depth_scale, double depth_trunc) {
    const float d = (float)((double)(float)raw / (double)depth_scale);
    return (raw == 0u || (double)d > depth_trunc) ? 0.0f : d;
}

// pixel (u, v) at depth d -> ((u - cx) d / fx, (v - cy) d / fy, d) in the camera's frame
EPN_TSDF_FN void back_project(int u, int v, float d, const Camera &cam, double p[3]) {
    EPN_TSDF_NO_CONTRACT
    const double z = (double)d;
    const double a = ((double)u - cam.cx) * z, b = ((double)v - cam.cy) * z;
    p[0] = a / cam.fx;
    p[1] = b / cam.fy;
    p[2] = z;
}

// q = R p + t from the first three rows of a row-major 4 x 4: ((T0 p0 + T1 p1) + T2 p2) + T3 per row
EPN_TSDF_FN void transform(const double *T, const double p[3], double q[3]) {
    EPN_TSDF_NO_CONTRACT
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int r = 0; r < 3; ++r) {
        const double a = T[4 * r] * p[0], b = T[4 * r + 1] * p[1], c = T[4 * r + 2] * p[2];
        const double ab = a + b;
        const double abc = ab + c;
        q[r] = abc + T[4 * r + 3];
    }
}

// floor(x / unit_length): floor, not truncation
EPN_TSDF_FN double unit_index(double x, double unit_length) {
    return floor(x / unit_length);
}

// the two unit indices a sample at x touches on one axis: those of x - sdf_trunc and x + sdf_trunc
EPN_TSDF_FN void unit_span(double x, double sdf_trunc, double unit_length, double &lo, double &hi) {
    EPN_TSDF_NO_CONTRACT
    const double a = x - sdf_trunc, b = x + sdf_trunc;
    lo = unit_index(a, unit_length);
    hi = unit_index(b, unit_length);
}

// unit index (a double: NaN and huge values fail) -> its offset in the box [lo, lo + dim); false outside
EPN_TSDF_FN bool box_offset(double unit, int lo, int dim, int &rel) {
    const double r = unit - (double)lo;
    if (!(r >= 0.0 && r < (double)dim)) return false;
    rel = (int)r;
    return true;
}

// centre of voxel idx (0..15) of a unit on one axis: ((16 unit + idx) + 0.5) voxel_length
EPN_TSDF_FN double voxel_centre(int unit, int idx, double voxel_length) {
    EPN_TSDF_NO_CONTRACT
    const double k = (double)(UNIT * unit + idx) + 0.5;
    return k * voxel_length;
}

// a point of the camera's frame -> its pixel; false for z <= 0 (NaN included) and outside 0 <= u_f < W, 0 <= v_f < H
EPN_TSDF_FN bool project(const double c[3], const Camera &cam, int W, int H, int &pu, int &pv) {
    EPN_TSDF_NO_CONTRACT
    if (!(c[2] > 0.0)) return false;
    const double xf = c[0] * cam.fx, yf = c[1] * cam.fy;
    const double xq = xf / c[2], yq = yf / c[2];
    const double xc = xq + cam.cx, yc = yq + cam.cy;
    const double uf = xc + 0.5, vf = yc + 0.5;
    if (!(uf >= 0.0 && uf < (double)W && vf >= 0.0 && vf < (double)H)) return false;
    pu = (int)uf;
    pv = (int)vf;
    return true;
}

// the observation of a voxel at camera depth z by pixel (pu, pv) with depth d: t = min(1, sdf / sdf_trunc) as fp32; false
// for d == 0 and unless sdf > -sdf_trunc
EPN_TSDF_FN bool observe(float d, double z, int pu, int pv, const Camera &cam, double sdf_trunc, float &t) {
    EPN_TSDF_NO_CONTRACT
    if (d == 0.0f) return false;
    const double a = ((double)pu - cam.cx) / cam.fx, b = ((double)pv - cam.cy) / cam.fy;
    const double aa = a * a, bb = b * b;
    const double s = aa + bb;
    const double m = sqrt(s + 1.0);
    const double diff = (double)d - z;
    const double sdf = diff * m;
    if (!(sdf > -sdf_trunc)) return false;
    const double q = sdf / sdf_trunc;
    t = (float)(q < 1.0 ? q : 1.0);
    return true;
}

// tsdf = (tsdf * w + t) / (w + 1) in fp32, every operation rounded on its own; w += 1
EPN_TSDF_FN void update(float &tsdf, int &w, float t) {
    EPN_TSDF_NO_CONTRACT
    const float fw = (float)w;
    const float prod = tsdf * fw;
    const float num = prod + t;
    const float den = fw + 1.0f;
    tsdf = (float)((double)num / (double)den);
    w += 1;
}

EPN_TSDF_FN bool takes_part(float f, int w) {
    return w != 0 && f >= -SURFACE_BAND && f < SURFACE_BAND;
}

// f0 f1 < 0, the product taken in fp64 (exact for two floats: no underflow to zero)
EPN_TSDF_FN bool crosses(float f0, float f1) {
    EPN_TSDF_NO_CONTRACT
    return (double)f0 * (double)f1 < 0.0;
}

// the crossing's coordinate between voxel centres p0 and p0 + voxel_length: (p0 r1 + p1 r0) / (r0 + r1), r = |f|
EPN_TSDF_FN float crossing(float f0, float f1, double p0, double voxel_length) {
    EPN_TSDF_NO_CONTRACT
    const double r0 = fabs((double)f0), r1 = fabs((double)f1);
    const double p1 = p0 + voxel_length;
    const double a = p0 * r1, b = p1 * r0;
    const double num = a + b, den = r0 + r1;
    return (float)(num / den);
}

}  // namespace epn_tsdf
