// 3DMatch training batches for gfx950: a batch of fragment pairs with their keypoint correspondences -> the two
// [B, npt, n_sample, 3] patch tensors, the pair's relative rotation and the augmentation that was applied.  Replaces the host
// path of the reference's FragmentLoader.__getitem__ (SPConvNets/datasets/match_3dmatch.py:301-354), which per pair, in a
// DataLoader worker, draws npt correspondences (np.random.choice), cuts a radius patch around each keypoint in both fragments
// (scipy KDTree), resamples every patch to input_num points (pctk.uniform_resample_np), draws one Euler rotation per side
// (pctk.rotate_point_cloud(None, max_degree=30), vgtk/vgtk/pc/augmentation.py:16-33 and :58-89), rotates the patches and returns
// T = R_A^T R_B.  Its draws are numpy's and cannot be reproduced on a GPU; the library defines its own deterministic form of the
// same semantics (include/epn_so3conv.h epn_fragment_pair_batch_f32).  For sample b with identity
// id = ids ? ids[b] : b, side s (0 source, 1 target) and keypoint slot j, the stream is Q' = (id * 2 + s) * npt + j:
//
//   choice     choice[j] = word0(Philox4x32-10(ctr_lo = 2^32, ctr_hi = Q'(0, j), key = seed)) mod P_b: both sides take the same
//              correspondence; the keypoint of side s is corr[choice[j], s]
//   patch      the rule of epn_radius_patches_f32 on the rows of the side's fragment with global row Q' (patch_sweep.h, shared
//              with patch_extract.hip)
//   rotation   w = Philox4x32-10(ctr_lo = 2^32 + 1, ctr_hi = Q'(s, 0), key = seed), d_k = w[k] mod max_degree degrees,
//              R = Rz(d_2) Ry(d_1) Rx(d_0) in fp64, rounded once to fp32; max_degree = 0: R = I
//   values     R (p - center * q): the subtraction rounded in fp32, the product ((r0 x + r1 y) + r2 z) in fp64 FROM THE ROUNDED R,
//              rounded once
//   T, T_aug   T = R_A^T R_B from the poses in fp64, rounded once; T_aug = (R_aug_src T) R_aug_tgt^T from the three rounded
//              matrices in fp64, rounded once
//   status     8 a pairs entry outside [0, F) or offsets / corr_offsets descending or out of range; else 1 no correspondences;
//              else 4 a non-finite pose entry or chosen keypoint coordinate.  Such a sample reads nothing out of range.
//
// Geometry: ONE launch of B * 2 * npt workgroups of 256 threads, workgroup ((b * 2 + s) * npt + j) doing what a radius_patches
// workgroup does.  Every workgroup decides its sample's status itself (a handful of table reads, npt draws spread over the
// threads, one block-wide OR) and thread 0 computes its side's R into LDS: nothing is handed from one workgroup to another.  The
// workgroups with j == 0 write R_aug[b, s]; the one with s == 0 also writes T, T_aug and status.  No workspace, no global
// atomics, every loop bounded by the fragment's rows, n_sample or npt: bitwise repeatable.
#include <cmath>

#include "epn_common.h"
#include "patch_sweep.h"

namespace {

using namespace epn_keysel;

struct PairShared {
    Shared sel;
    float R[9];                    // the side's rounded rotation
};

// Rz(d2) Ry(d1) Rx(d0) of R_from_euler_np, in fp64, rounded once; Qs0 = Q'(s, 0)
__device__ void euler_rotation(unsigned long long Qs0, unsigned long long seed, int max_degree, float Rf[9]) {
    double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    if (max_degree > 0) {
        const epn::philox::u32x4 w = epn::philox::philox4x32_10((1ull << 32) + 1ull, Qs0, seed);
        const double pi = 3.14159265358979323846264338327950288;
        const double ax = ((double)(w.w[0] % (unsigned)max_degree) * pi) / 180.0,
                     ay = ((double)(w.w[1] % (unsigned)max_degree) * pi) / 180.0,
                     az = ((double)(w.w[2] % (unsigned)max_degree) * pi) / 180.0;
        const double cx = cos(ax), sx = sin(ax), cy = cos(ay), sy = sin(ay), cz = cos(az), sz = sin(az);
        const double m01 = sy * sx, m02 = sy * cx, m21 = cy * sx, m22 = cy * cx;       // Ry Rx = [cy m01 m02; 0 cx -sx; -sy m21 m22]
        R[0] = cz * cy; R[1] = cz * m01 - sz * cx; R[2] = cz * m02 + sz * sx;
        R[3] = sz * cy; R[4] = sz * m01 + cz * cx; R[5] = sz * m02 - cz * sx;
        R[6] = -sy;     R[7] = m21;                R[8] = m22;
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) Rf[e] = (float)R[e];
}

__global__ __launch_bounds__(PT) void fragment_pair_batch_kernel(
    const float *__restrict__ points, int m, const int32_t *__restrict__ offsets, int F, const int32_t *__restrict__ pairs,
    const float *__restrict__ corr, int C, const int32_t *__restrict__ corr_offsets, const double *__restrict__ poses,
    const int64_t *__restrict__ ids, int n_sample, int npt, float radius, unsigned long long seed, int key_bits, int max_degree,
    int center, float *src, float *tgt, int32_t *idx, int32_t *__restrict__ counts, int32_t *__restrict__ choice,
    float *__restrict__ T, float *__restrict__ R_aug, float *__restrict__ T_aug, int32_t *__restrict__ status) {
    __shared__ PairShared sh;
    const int tid = threadIdx.x;
    const unsigned unpt = (unsigned)npt, j = blockIdx.x % unpt, bs = blockIdx.x / unpt, s = bs & 1u;
    const size_t b = bs >> 1;
    const unsigned long long id = ids ? (unsigned long long)ids[b] : (unsigned long long)b;
    const unsigned long long Q0 = id * 2ull * unpt, Qs0 = (id * 2ull + s) * unpt;

    // ---- the sample's status: the same in every workgroup of the sample, uniform over the workgroup
    int st = 0, f[2], o0[2] = {0, 0}, o1[2] = {0, 0};
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        f[e] = pairs[2 * b + e];
        if (f[e] < 0 || f[e] >= F) {
            st = 8;
        } else {
            o0[e] = offsets[f[e]];
            o1[e] = offsets[f[e] + 1];
            if (o0[e] < 0 || o1[e] > m || o1[e] < o0[e]) st = 8;
        }
    }
    const int c0 = corr_offsets[b], c1 = corr_offsets[b + 1];
    if (c0 < 0 || c1 > C || c1 < c0) st = 8;
    if (st == 0 && c1 == c0) st = 1;
    const unsigned P = st ? 1u : (unsigned)(c1 - c0);
    if (st == 0) {                                     // uniform: the barrier inside is safe
        int bad = 0;
        if (tid < 32) bad = !std::isfinite(poses[(size_t)16 * (tid < 16 ? f[0] : f[1]) + (tid & 15)]);
        for (unsigned t = tid; t < unpt; t += PT) {
            const unsigned ch = epn::philox::philox4x32_10(1ull << 32, Q0 + t, seed).w[0] % P;
            const float *k = corr + (size_t)6 * ((size_t)c0 + ch);
#pragma unroll
            for (int e = 0; e < 6; ++e) bad |= !std::isfinite(k[e]);
        }
        if (__syncthreads_or(bad)) st = 4;
    }

    // ---- the side's rotation; the per-sample outputs from the workgroups with j == 0
    if (tid == 0) {
        float Rs[9];
        euler_rotation(Qs0, seed, max_degree, Rs);
#pragma unroll
        for (int e = 0; e < 9; ++e) sh.R[e] = Rs[e];
        if (j == 0u) {
#pragma unroll
            for (int e = 0; e < 9; ++e) R_aug[(b * 2 + s) * 9 + e] = Rs[e];
        }
        if (j == 0u && s == 0u) {
            float Rt[9], Tf[9];
            euler_rotation(Qs0 + unpt, seed, max_degree, Rt);
            const double *A = poses + (size_t)16 * (st ? 0 : f[0]), *Bm = poses + (size_t)16 * (st ? 0 : f[1]);
#pragma unroll
            for (int r = 0; r < 3; ++r)                // R_A^T R_B
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    Tf[3 * r + c] = st ? 0.0f : (float)((A[r] * Bm[c] + A[4 + r] * Bm[4 + c]) + A[8 + r] * Bm[8 + c]);
            double U[9];
#pragma unroll
            for (int r = 0; r < 3; ++r)                // R_aug_src T
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    U[3 * r + c] = ((double)Rs[3 * r] * (double)Tf[c] + (double)Rs[3 * r + 1] * (double)Tf[3 + c]) +
                                   (double)Rs[3 * r + 2] * (double)Tf[6 + c];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) {          // (R_aug_src T) R_aug_tgt^T
                    T[b * 9 + 3 * r + c] = Tf[3 * r + c];
                    T_aug[b * 9 + 3 * r + c] =
                        st ? 0.0f
                           : (float)((U[3 * r] * (double)Rt[3 * c] + U[3 * r + 1] * (double)Rt[3 * c + 1]) +
                                     U[3 * r + 2] * (double)Rt[3 * c + 2]);
                }
            status[b] = st;
        }
    }

    const size_t row = b * unpt + j;                   // the patch row inside its side's tensor
    int32_t *irow = idx + ((b * 2 + s) * unpt + j) * (size_t)n_sample;
    float *prow = (s ? tgt : src) + row * (size_t)n_sample * 3;
    if (st) {
        for (int t = tid; t < n_sample; t += PT) {
            irow[t] = -1;
            prow[3 * t] = 0.0f; prow[3 * t + 1] = 0.0f; prow[3 * t + 2] = 0.0f;
        }
        if (tid == 0) {
            counts[(b * 2 + s) * unpt + j] = 0;
            if (s == 0u) choice[row] = -1;
        }
        return;
    }
    __syncthreads();                                   // sh.R is written

    const unsigned ch = epn::philox::philox4x32_10(1ull << 32, Q0 + j, seed).w[0] % P;
    const float *kp = corr + (size_t)6 * ((size_t)c0 + ch) + 3 * s;
    const float qx = kp[0], qy = kp[1], qz = kp[2];
    const float cx = center ? qx : 0.0f, cy = center ? qy : 0.0f, cz = center ? qz : 0.0f;
    double Rd[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) Rd[e] = (double)sh.R[e];
    const unsigned count = radius_patch_row(
        sh.sel, points + (size_t)3 * (size_t)(s ? o0[1] : o0[0]), (unsigned)(s ? o1[1] - o0[1] : o1[0] - o0[0]), qx, qy, qz, radius, n_sample, Qs0 + j, seed, key_bits,
        irow, prow, [=](float px, float py, float pz, float *out) {
            const double x = (double)__fsub_rn(px, cx), y = (double)__fsub_rn(py, cy), z = (double)__fsub_rn(pz, cz);
            out[0] = (float)((Rd[0] * x + Rd[1] * y) + Rd[2] * z);
            out[1] = (float)((Rd[3] * x + Rd[4] * y) + Rd[5] * z);
            out[2] = (float)((Rd[6] * x + Rd[7] * y) + Rd[8] * z);
        });
    if (tid == 0) {
        counts[(b * 2 + s) * unpt + j] = (int32_t)count;
        if (s == 0u) choice[row] = (int32_t)ch;
    }
}

}  // namespace

// Sizes and scalars first, then B == 0, then pointers -- all before the first HIP runtime call.  The grid is B * 2 * npt
// workgroups in x.
extern "C" int epn_fragment_pair_batch_f32(const float *points, int m, const int32_t *offsets, int F, const int32_t *pairs, int B,
                                           const float *corr, int C, const int32_t *corr_offsets, const double *poses,
                                           const int64_t *ids, int n_sample, int npt, float radius, uint64_t seed, int key_bits,
                                           int max_degree, int center, float *src, float *tgt, int32_t *idx, int32_t *counts,
                                           int32_t *choice, float *T, float *R_aug, float *T_aug, int32_t *status,
                                           epn_stream_t stream) {
    if (B < 0 || F < 0 || m < 0 || C < 0 || n_sample < 1 || n_sample > 8192 || npt < 1 || npt > 4096) return EPN_EINVAL;
    if (key_bits < 1 || key_bits > 32 || max_degree < 0 || max_degree > 360) return EPN_EINVAL;
    if (!std::isfinite(radius) || !(radius > 0.0f) || (center != 0 && center != 1)) return EPN_EINVAL;
    if ((long long)B * 2 * npt > 2147483647LL) return EPN_EINVAL;
    if (B == 0) return 0;
    if (!offsets || !pairs || !corr_offsets || (m > 0 && !points) || (C > 0 && !corr) || (F > 0 && !poses)) return EPN_EINVAL;
    if (!src || !tgt || !idx || !counts || !choice || !T || !R_aug || !T_aug || !status) return EPN_EINVAL;
    EPN_LAUNCH(fragment_pair_batch_kernel, dim3((unsigned)B * 2u * (unsigned)npt), dim3(PT), 0, epn_stream(stream), points, m,
               offsets, F, pairs, corr, C, corr_offsets, poses, ids, n_sample, npt, radius, (unsigned long long)seed, key_bits,
               max_degree, center, src, tgt, idx, counts, choice, T, R_aug, T_aug, status);
    EPN_CHECK_LAUNCH();
    return 0;
}
