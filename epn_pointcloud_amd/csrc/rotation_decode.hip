// Rotation estimation for gfx950: the stage after RegSO3ConvModel's head.  Anchor labels for a training step
// (label_relative_rotation_np, vgtk/vgtk/functional/rotation.py:521-526), the chordal L2 mean of rotations (so3_mean,
// rotation.py:481-518) and the decode of the head's (confidence, y) into one rotation per pair with its angular error (the
// alignment branch of MultiTaskDetectionLoss.forward, vgtk/vgtk/loss.py:140-172 and :210-218).  Specification:
// include/epn_so3conv.h (epn_rotation_labels_f32, epn_so3_mean_f32, epn_rotation_decode_f32) and DESIGN.md 3.1b.
//
// One launch per call, one 64-thread workgroup (one wave) per pair, lane a = source anchor a (lanes >= A contribute zeros).
//   labels  lane a keeps P = T^T A_a in registers; tr(A_a^T T A_i) = <P, A_i> for i = 0..A-1, arg max on a strict >, then
//           R_target = P^T A_label
//   mean    lane l adds w_n Rs_n for n = l, l + 64, ... in ascending order; xor tree over the wave; projection (below)
//   decode  lane a: arg max over the target anchors of its column of wts (coalesced: consecutive lanes read consecutive
//           floats), rotation map of its y entries, A_a R_a A_p^T; xor tree for sum c and for sum conf_a pred_Rs_a; projection
// The xor tree (x += shfl_xor(x, s), s = 32..1) adds the same two values in lane i and lane i ^ s, and fp addition commutes, so
// every lane ends with the same bits: all lanes run the projection redundantly and lane 0 writes it.
// Projection of Ce onto SO(3) (rotation_math.h, shared with a host program): the unit quaternion q that maximises q^T K q, K
// Horn's symmetric 4 x 4 matrix of Ce, by a cyclic Jacobi eigensolver with a FIXED number of sweeps (no convergence test, nothing data-dependent in the control flow
// except skipping an off-diagonal entry that is exactly zero).  R(q) is a rotation for every unit q, whatever the gap.
// fp64 throughout on the fp32 inputs; every output is rounded once.  Every index is below b * A (or b * N) rows: preds comes
// from a loop counter, so it lies in 0..A-1 for any wts, NaN included.
#include <cmath>

#include "epn_reduce.h"
#include "rotation_math.h"

namespace {

using epn_rot::acos_safe;
using epn_rot::rotation_map;
using epn_rot::so3_project;

constexpr int RW = 64;                   // threads per workgroup = one wave = the most anchors

__device__ __forceinline__ void load9(const float *__restrict__ p, double m[9]) {
#pragma unroll
    for (int e = 0; e < 9; ++e) m[e] = (double)p[e];
}

__global__ __launch_bounds__(RW) void rotation_labels_kernel(const float *__restrict__ anchors, const float *__restrict__ T, int A,
                                                             float *__restrict__ R_target, int32_t *__restrict__ label) {
    const int a = threadIdx.x;
    if (a >= A) return;
    const size_t pair = blockIdx.x;
    double Tm[9], Aa[9], P[9];
    load9(T + 9 * pair, Tm);
    load9(anchors + 9 * a, Aa);
#pragma unroll
    for (int j = 0; j < 3; ++j)                                        // P = T^T A_a
#pragma unroll
        for (int c = 0; c < 3; ++c) P[3 * j + c] = Tm[j] * Aa[c] + Tm[3 + j] * Aa[3 + c] + Tm[6 + j] * Aa[6 + c];
    int best = 0;
    double best_tr = 0.0;
    for (int i = 0; i < A; ++i) {
        const float *Ai = anchors + 9 * i;
        double tr = 0.0;
#pragma unroll
        for (int e = 0; e < 9; ++e) tr += P[e] * (double)Ai[e];
        if (i == 0 || tr > best_tr) {
            best = i;
            best_tr = tr;
        }
    }
    double Al[9];
    load9(anchors + 9 * best, Al);
    float *out = R_target + 9 * (pair * A + a);
#pragma unroll
    for (int c = 0; c < 3; ++c)                                        // P^T A_label
#pragma unroll
        for (int k = 0; k < 3; ++k) out[3 * c + k] = (float)(P[c] * Al[k] + P[3 + c] * Al[3 + k] + P[6 + c] * Al[6 + k]);
    label[pair * A + a] = best;
}

__global__ __launch_bounds__(RW) void so3_mean_kernel(const float *__restrict__ Rs, const float *__restrict__ weights, int N,
                                                      float *__restrict__ R, float *__restrict__ margin) {
    const int lane = threadIdx.x;
    const size_t pair = blockIdx.x;
    double C[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int n = lane; n < N; n += RW) {
        const double w = weights ? (double)weights[pair * N + n] : 1.0;
        const float *m = Rs + 9 * (pair * N + n);
#pragma unroll
        for (int e = 0; e < 9; ++e) C[e] += w * (double)m[e];
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) C[e] = epn_wave_sum(C[e]);
    double Rm[9], mg;
    so3_project(C, Rm, mg);
    if (lane == 0) {
#pragma unroll
        for (int e = 0; e < 9; ++e) R[9 * pair + e] = (float)Rm[e];
        margin[pair] = (float)mg;
    }
}

template <int NR>
__global__ __launch_bounds__(RW) void rotation_decode_kernel(const float *__restrict__ wts, const float *__restrict__ y,
                                                             const float *__restrict__ anchors, const int32_t *__restrict__ label,
                                                             const float *__restrict__ gt_T, int A, float *__restrict__ pred_R,
                                                             int32_t *__restrict__ preds, float *__restrict__ conf,
                                                             float *__restrict__ margin, float *__restrict__ pred_Rs,
                                                             int32_t *__restrict__ hits, float *__restrict__ err) {
    const int a = threadIdx.x;
    const bool live = a < A;
    const size_t pair = blockIdx.x, AA = (size_t)A * A;
    int p = 0;
    double c = 0.0;
    double Rp[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (live) {
        const float *w = wts + pair * AA + a;
        float best = w[0];
        for (int t = 1; t < A; ++t) {
            const float v = w[(size_t)t * A];
            if (v > best) {
                best = v;
                p = t;
            }
        }
        c = (double)best;
        const float *yp = y + pair * NR * AA + (size_t)p * A + a;
        double v[NR];
#pragma unroll
        for (int e = 0; e < NR; ++e) v[e] = (double)yp[e * AA];
        double Ra[9], norms[2];
        rotation_map<NR>(v, Ra, norms);
        double Aa[9], Ap[9], M[9];
        load9(anchors + 9 * a, Aa);
        load9(anchors + 9 * p, Ap);
#pragma unroll
        for (int i = 0; i < 3; ++i)                                    // M = A_a R_a
#pragma unroll
            for (int k = 0; k < 3; ++k) M[3 * i + k] = Aa[3 * i] * Ra[k] + Aa[3 * i + 1] * Ra[3 + k] + Aa[3 * i + 2] * Ra[6 + k];
#pragma unroll
        for (int i = 0; i < 3; ++i)                                    // pred_Rs = M A_p^T
#pragma unroll
            for (int l = 0; l < 3; ++l) Rp[3 * i + l] = M[3 * i] * Ap[3 * l] + M[3 * i + 1] * Ap[3 * l + 1] + M[3 * i + 2] * Ap[3 * l + 2];
    }
    const double cf = c / (1e-6 + epn_wave_sum(c));
    double C[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) C[e] = epn_wave_sum(live ? cf * Rp[e] : 0.0);
    const unsigned long long hit = __ballot(live && label && label[pair * A + a] == p);
    double Rm[9], mg;
    so3_project(C, Rm, mg);
    if (live) {
        preds[pair * A + a] = p;
        conf[pair * A + a] = (float)cf;
        if (pred_Rs) {
            float *out = pred_Rs + 9 * (pair * A + a);
#pragma unroll
            for (int e = 0; e < 9; ++e) out[e] = (float)Rp[e];
        }
    }
    if (a == 0) {
#pragma unroll
        for (int e = 0; e < 9; ++e) pred_R[9 * pair + e] = (float)Rm[e];
        margin[pair] = (float)mg;
        if (label) hits[pair] = __popcll(hit);
        if (gt_T) {
            double tr = 0.0;
#pragma unroll
            for (int e = 0; e < 9; ++e) tr += Rm[e] * (double)gt_T[9 * pair + e];
            err[pair] = (float)acos_safe(0.5 * (tr - 1.0));
        }
    }
}

}  // namespace

extern "C" int epn_rotation_labels_f32(const float *anchors, const float *T, int b, int A, float *R_target, int32_t *label,
                                       epn_stream_t stream) {
    // every argument is checked before the first HIP runtime call
    if (b < 0 || A < 1 || A > RW) return EPN_EINVAL;
    if (b == 0) return 0;
    if (!anchors || !T || !R_target || !label) return EPN_ENULL;
    EPN_LAUNCH(rotation_labels_kernel, dim3((unsigned)b), dim3(RW), 0, epn_stream(stream), anchors, T, A, R_target, label);
    EPN_CHECK_LAUNCH();
    return 0;
}

extern "C" int epn_so3_mean_f32(const float *Rs, const float *weights, int b, int N, float *R, float *margin,
                                epn_stream_t stream) {
    if (b < 0 || N < 1) return EPN_EINVAL;
    if (b == 0) return 0;
    if (!Rs || !R || !margin) return EPN_ENULL;
    EPN_LAUNCH(so3_mean_kernel, dim3((unsigned)b), dim3(RW), 0, epn_stream(stream), Rs, weights, N, R, margin);
    EPN_CHECK_LAUNCH();
    return 0;
}

extern "C" int epn_rotation_decode_f32(const float *wts, const float *y, const float *anchors, const int32_t *label,
                                       const float *gt_T, int b, int A, int nr, float *pred_R, int32_t *preds, float *conf,
                                       float *margin, float *pred_Rs, int32_t *hits, float *err, epn_stream_t stream) {
    if (b < 0 || A < 1 || A > RW || (nr != 4 && nr != 6)) return EPN_EINVAL;
    if (b == 0) return 0;
    if (!wts || !y || !anchors || !pred_R || !preds || !conf || !margin || (label && !hits) || (gt_T && !err)) return EPN_ENULL;
    const dim3 grid((unsigned)b), block(RW);
    hipStream_t st = epn_stream(stream);
    if (nr == 4)
        EPN_LAUNCH(rotation_decode_kernel<4>, grid, block, 0, st, wts, y, anchors, label, gt_T, A, pred_R, preds, conf, margin,
                   pred_Rs, hits, err);
    else
        EPN_LAUNCH(rotation_decode_kernel<6>, grid, block, 0, st, wts, y, anchors, label, gt_T, A, pred_R, preds, conf, margin,
                   pred_Rs, hits, err);
    EPN_CHECK_LAUNCH();
    return 0;
}
