// The rotation network's training loss for gfx950: the alignment branch of MultiTaskDetectionLoss.forward (vgtk/vgtk/loss.py:140-181
// with CrossEntropyLoss :18-30 and batched_select_anchor :77-92): a softmax cross-entropy over the target-anchor axis of the
// head's confidence, the rotation map of the y entries at the labelled target anchor, and the L2 distance of that matrix to the
// relative rotation it should regress.  Specification: include/epn_so3conv.h (epn_rotation_loss_f32, epn_rotation_loss_bwd_f32),
// DESIGN.md 3.1e.
//
// fp64 throughout on the fp32 inputs, every output rounded once; no atomics, no workspace, no host synchronisation; every sum
// runs in a fixed order, so two runs are bitwise equal.
//   rows    one 64-thread workgroup (one wave) per pair, lane a = source anchor a, as in rotation_decode.hip: for every target
//           anchor t the lanes read consecutive floats of wts[p,t,:].  Two passes over the column: the maximum with its
//           arg max (fp32, strict >: the decode's rule), then the sum of exp(. - max) in ascending t.
//   finish  one workgroup: thread i adds rows i, i + 256, ... ascending, then a fixed tree in LDS.
//   bwd     one 256-thread workgroup per pair: each of its four waves repeats the row arithmetic of its pair (the same
//           operations on the same values: the same bits) and wave w writes the target anchors t = w, w + 4, ...: every element
//           of dwts[p,t,:] and dy[p,:,t,:], zeros included.
// The label is the only value read from memory that becomes an address; it is range-checked on the device first, in both
// directions, and a row whose label lies outside 0..A-1 reads nothing through it.
#include <cmath>

#include "epn_reduce.h"
#include "rotation_math.h"

namespace {

using epn_rot::cross;
using epn_rot::rotation_map;

constexpr int RW = 64;                   // lanes of a wave = the most anchors
constexpr int FT = 256;                  // threads of the finish and of the backward
constexpr int BWAVES = FT / RW;          // waves per pair in the backward
constexpr double CLAMP = 1e-8;           // normalize_vector's clamp

enum { FLAG_BAD_LABEL = 1, FLAG_NORM_CLAMPED = 2 };

// the softmax pieces of column a of wts[p]: the maximum (by the decode's rule, with its arg max) and sum_t exp(w_t - max)
__device__ __forceinline__ void column_softmax(const float *__restrict__ w, int A, int &pred, double &m, double &s) {
    float best = w[0];
    pred = 0;
    for (int t = 1; t < A; ++t) {
        const float v = w[(size_t)t * A];
        if (v > best) {
            best = v;
            pred = t;
        }
    }
    m = (double)best;
    s = 0.0;
    for (int t = 0; t < A; ++t) s += exp((double)w[(size_t)t * A] - m);
}

template <int NR>
__global__ __launch_bounds__(RW) void rotation_loss_rows_kernel(const float *__restrict__ wts, const float *__restrict__ y,
                                                                const int32_t *__restrict__ label, const float *__restrict__ R_target,
                                                                int A, float *__restrict__ row_ce, float *__restrict__ row_l2,
                                                                int32_t *__restrict__ preds, int32_t *__restrict__ row_flags,
                                                                float *__restrict__ sel_R) {
    const int a = threadIdx.x;
    if (a >= A) return;
    const size_t pair = blockIdx.x, AA = (size_t)A * A, row = pair * A + a;
    const float *w = wts + pair * AA + a;
    int pred;
    double m, s;
    column_softmax(w, A, pred, m, s);
    const int L = label[row];
    double ce = 0.0, l2 = 0.0;
    double R[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int flags = FLAG_BAD_LABEL;
    if (L >= 0 && L < A) {
        ce = m + log(s) - (double)w[(size_t)L * A];
        const float *yp = y + pair * NR * AA + (size_t)L * A + a;
        double v[NR], norms[2];
#pragma unroll
        for (int e = 0; e < NR; ++e) v[e] = (double)yp[e * AA];
        rotation_map<NR>(v, R, norms);
        flags = (norms[0] < CLAMP || norms[1] < CLAMP) ? FLAG_NORM_CLAMPED : 0;
        const float *Rt = R_target + 9 * row;
#pragma unroll
        for (int e = 0; e < 9; ++e) {
            const double d = (double)Rt[e] - R[e];
            l2 += d * d;
        }
    }
    row_ce[row] = (float)ce;
    row_l2[row] = (float)l2;
    preds[row] = pred;
    row_flags[row] = flags;
#pragma unroll
    for (int e = 0; e < 9; ++e) sel_R[9 * row + e] = (float)R[e];
}

__global__ __launch_bounds__(FT) void rotation_loss_finish_kernel(const float *__restrict__ row_ce, const float *__restrict__ row_l2,
                                                                  const int32_t *__restrict__ preds, const int32_t *__restrict__ label,
                                                                  long long rows, double w, float *__restrict__ scalars) {
    __shared__ double buf[FT];
    double sc = 0.0, sl = 0.0, hit = 0.0;
    for (long long i = threadIdx.x; i < rows; i += FT) {
        sc += (double)row_ce[i];
        sl += (double)row_l2[i];
        hit += preds[i] == label[i] ? 1.0 : 0.0;
    }
    sc = epn_block_sum<FT>(sc, buf);
    sl = epn_block_sum<FT>(sl, buf);
    hit = epn_block_sum<FT>(hit, buf);
    if (threadIdx.x == 0) {
        const double cls = sc / (double)rows, reg = w * sl / (9.0 * (double)rows);
        scalars[0] = (float)(cls + reg);
        scalars[1] = (float)cls;
        scalars[2] = (float)reg;
        scalars[3] = (float)(hit / (double)rows);
    }
}

// gradient through u = v / max(|v|, 1e-8), given u, |v| and the gradient gu of u, in place: (I - u u^T) gu / |v|, or gu / 1e-8
// where the clamp was active (what autograd makes of torch.max(norm, 1e-8))
template <int N>
__device__ __forceinline__ void normalize_bwd(const double u[N], double norm, double g[N]) {
    if (norm < CLAMP) {
#pragma unroll
        for (int e = 0; e < N; ++e) g[e] /= CLAMP;
        return;
    }
    double dot = 0.0;
#pragma unroll
    for (int e = 0; e < N; ++e) dot += u[e] * g[e];
#pragma unroll
    for (int e = 0; e < N; ++e) g[e] = (g[e] - u[e] * dot) / norm;
}

// J^T G of the rotation map at the raw entries v0 (v: what rotation_map left of them, R and norms its other outputs) -> dv
template <int NR>
__device__ __forceinline__ void rotation_map_bwd(const double v0[NR], const double v[NR], const double R[9], const double norms[2],
                                                 const double G[9], double dv[NR]) {
    if (NR == 4) {
        const double w = v[0], x = v[1], yq = v[2], z = v[3];
        dv[0] = 2.0 * (-z * G[1] + yq * G[2] + z * G[3] - x * G[5] - yq * G[6] + x * G[7]);
        dv[1] = 2.0 * (yq * G[1] + z * G[2] + yq * G[3] - 2.0 * x * G[4] - w * G[5] + z * G[6] + w * G[7] - 2.0 * x * G[8]);
        dv[2] = 2.0 * (-2.0 * yq * G[0] + x * G[1] + w * G[2] + x * G[3] + z * G[5] - w * G[6] + z * G[7] - 2.0 * yq * G[8]);
        dv[3] = 2.0 * (-2.0 * z * G[0] - w * G[1] + x * G[2] + w * G[3] - 2.0 * z * G[4] + yq * G[5] + x * G[6] + yq * G[7]);
        normalize_bwd<4>(v, norms[0], dv);
    } else {
        const double x[3] = {R[0], R[3], R[6]}, z[3] = {R[2], R[5], R[8]}, yr[3] = {v0[NR - 3], v0[NR - 2], v0[NR - 1]};
        double gx[3] = {G[0], G[3], G[6]}, gy[3] = {G[1], G[4], G[7]}, gz[3] = {G[2], G[5], G[8]}, t[3];
        cross(x, gy, t);                                               // y = z cross x: gz += x cross gy, gx += gy cross z
#pragma unroll
        for (int i = 0; i < 3; ++i) gz[i] += t[i];
        cross(gy, z, t);
#pragma unroll
        for (int i = 0; i < 3; ++i) gx[i] += t[i];
        normalize_bwd<3>(z, norms[1], gz);                             // z = n(c): gz is now the gradient of c = x cross yr
        cross(yr, gz, t);                                              // gx += yr cross gc, gyr = gc cross x
#pragma unroll
        for (int i = 0; i < 3; ++i) gx[i] += t[i];
        cross(gz, x, t);
        normalize_bwd<3>(x, norms[0], gx);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            dv[i] = gx[i];
            dv[NR - 3 + i] = t[i];
        }
    }
}

template <int NR>
__global__ __launch_bounds__(FT) void rotation_loss_bwd_kernel(const float *__restrict__ upstream, const float *__restrict__ wts,
                                                               const float *__restrict__ y, const int32_t *__restrict__ label,
                                                               const float *__restrict__ R_target, const int32_t *__restrict__ row_flags,
                                                               int A, double c_ce, double c_l2, float *__restrict__ dwts,
                                                               float *__restrict__ dy) {
    const int a = threadIdx.x & (RW - 1), wave = threadIdx.x / RW;
    if (a >= A) return;
    const size_t pair = blockIdx.x, AA = (size_t)A * A, row = pair * A + a;
    const double g = (double)upstream[0];
    const float *w = wts + pair * AA + a;
    int pred, L = label[row];
    const bool live = !(row_flags[row] & FLAG_BAD_LABEL) && L >= 0 && L < A;
    double m = 0.0, s = 1.0, dv[NR];
#pragma unroll
    for (int e = 0; e < NR; ++e) dv[e] = 0.0;
    if (live) {
        column_softmax(w, A, pred, m, s);
        const float *yp = y + pair * NR * AA + (size_t)L * A + a;
        double v0[NR], v[NR], R[9], G[9], norms[2];
#pragma unroll
        for (int e = 0; e < NR; ++e) v[e] = v0[e] = (double)yp[e * AA];
        rotation_map<NR>(v, R, norms);
        const float *Rt = R_target + 9 * row;
        const double cg = g * c_l2;
#pragma unroll
        for (int e = 0; e < 9; ++e) G[e] = cg * (R[e] - (double)Rt[e]);
        rotation_map_bwd<NR>(v0, v, R, norms, G, dv);
    } else {
        L = -1;
    }
    const double cw = g * c_ce;
    for (int t = wave; t < A; t += BWAVES) {
        const size_t at = pair * AA + (size_t)t * A + a;
        dwts[at] = live ? (float)(cw * (exp((double)w[(size_t)t * A] - m) / s - (t == L ? 1.0 : 0.0))) : 0.0f;
        float *dyp = dy + pair * NR * AA + (size_t)t * A + a;
#pragma unroll
        for (int e = 0; e < NR; ++e) dyp[e * AA] = t == L ? (float)dv[e] : 0.0f;
    }
}

bool loss_shape_ok(int b, int A, int nr, double w) { return b >= 0 && A >= 1 && A <= RW && (nr == 4 || nr == 6) && std::isfinite(w); }

}  // namespace

extern "C" int epn_rotation_loss_f32(const float *wts, const float *y, const int32_t *label, const float *R_target, int b, int A,
                                     int nr, double w, float *row_ce, float *row_l2, int32_t *preds, int32_t *row_flags,
                                     float *sel_R, float *scalars, epn_stream_t stream) {
    // every argument is checked before the first HIP runtime call
    if (!loss_shape_ok(b, A, nr, w)) return EPN_EINVAL;
    if (b == 0) return 0;
    if (!wts || !y || !label || !R_target || !row_ce || !row_l2 || !preds || !row_flags || !sel_R || !scalars) return EPN_ENULL;
    const dim3 grid((unsigned)b), block(RW);
    hipStream_t st = epn_stream(stream);
    if (nr == 4)
        EPN_LAUNCH(rotation_loss_rows_kernel<4>, grid, block, 0, st, wts, y, label, R_target, A, row_ce, row_l2, preds, row_flags, sel_R);
    else
        EPN_LAUNCH(rotation_loss_rows_kernel<6>, grid, block, 0, st, wts, y, label, R_target, A, row_ce, row_l2, preds, row_flags, sel_R);
    EPN_CHECK_LAUNCH();
    EPN_LAUNCH_AUX(rotation_loss_finish_kernel, dim3(1), dim3(FT), 0, st, row_ce, row_l2, preds, label, (long long)b * A, w, scalars);
    EPN_CHECK_LAUNCH();
    return 0;
}

extern "C" int epn_rotation_loss_bwd_f32(const float *upstream, const float *wts, const float *y, const int32_t *label,
                                         const float *R_target, const int32_t *row_flags, int b, int A, int nr, double w,
                                         float *dwts, float *dy, epn_stream_t stream) {
    if (!loss_shape_ok(b, A, nr, w)) return EPN_EINVAL;
    if (b == 0) return 0;
    if (!upstream || !wts || !y || !label || !R_target || !row_flags || !dwts || !dy) return EPN_ENULL;
    const dim3 grid((unsigned)b), block(FT);
    hipStream_t st = epn_stream(stream);
    const double rows = (double)b * A, c_ce = 1.0 / rows, c_l2 = 2.0 * w / (9.0 * rows);
    if (nr == 4)
        EPN_LAUNCH(rotation_loss_bwd_kernel<4>, grid, block, 0, st, upstream, wts, y, label, R_target, row_flags, A, c_ce, c_l2, dwts, dy);
    else
        EPN_LAUNCH(rotation_loss_bwd_kernel<6>, grid, block, 0, st, upstream, wts, y, label, R_target, row_flags, A, c_ce, c_l2, dwts, dy);
    EPN_CHECK_LAUNCH();
    return 0;
}
