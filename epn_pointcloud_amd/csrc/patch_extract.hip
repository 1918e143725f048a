// Patch extraction for gfx950: every point of a fragment within `radius` of a keypoint, resampled to n_sample points.
// Replaces the host path of the reference's 3DMatch loader (SPConvNets/datasets/match_3dmatch.py:154-177: scipy KDTree +
// query_ball_point per keypoint; vgtk/vgtk/pc/sample.py:16-36: np.random.choice to input_num points), whose selection is
// random and unordered and cannot be reproduced on a GPU.  The library defines its own deterministic form of the same
// semantics (include/epn_so3conv.h epn_radius_patches_f32); for keypoint row q, Q = kpt_row0 + q:
//
//   S       = { i : d2(i) <= r2 },  d2 = (dx*dx + dy*dy) + dz*dz,  dx = p.x - q.x ..., r2 = radius*radius, every operation an
//             individually rounded fp32 one (__fsub_rn / __fmul_rn / __fadd_rn: no fma contraction), comparison inclusive
//   key(i)  = word0(Philox4x32-10(ctr_lo = i, ctr_hi = Q, key = seed)) >> (32 - key_bits)
//   count <= 1            idx row -1, patch row 0
//   count >= n_sample     the n_sample members of S smallest in (key, i), written in ascending i
//   1 < count < n_sample  slots 0..count-1 = S in ascending i; slot j >= count repeats slot
//                         word1(Philox4x32-10(ctr_lo = j, ctr_hi = Q, key = seed)) mod count
//   patches = (pc[idx] - center * kpt) * scale: the subtraction rounded, then the multiply
//
// Geometry: ONE 256-thread workgroup per keypoint sweeps the fragment in chunks of 256 consecutive points (a 262 144-point
// fragment is 3 MB: the sweeps after the first are served by the XCD's L2 / the Infinity Cache).
//   pass 1     count, and an LDS histogram (integer LDS atomics) of the top 11 key bits of the in-radius points
//   pass 2, 3  only when count > n_sample: histograms of the next 11 and the last 10 key bits inside the boundary bucket ->
//              the exact threshold key T and the number t of key == T members to take (the lowest i win)
//   emit       compaction in ascending index: 64-bit ballot + popcount inside a wave, one LDS exchange (one barrier, two slot
//              sets) across the four waves, a running base across chunks; key == T members are admitted while their rank
//              among the ties is below t  (the search and this step: key_select.h, shared with modelnet_batch.hip)
//   upsample   slots >= count copy slots < count of the same row back after a workgroup barrier
// Distances and keys are recomputed in every pass (Philox only for in-radius lanes): no [k, n] workspace.  Every loop is
// bounded by n or n_sample; no workgroup talks to another, no global atomics, no spin: the result is bitwise repeatable.
// The sweep body itself is radius_patch_row in patch_sweep.h, shared with pair_batch.hip (3DMatch training batches).
#include <cmath>

#include "epn_common.h"
#include "patch_sweep.h"

namespace {

using namespace epn_keysel;        // PT, Shared, radius_patch_row: the sweep shared with pair_batch.hip (patch_sweep.h)

__global__ __launch_bounds__(PT) void radius_patches_kernel(const float *__restrict__ pc, int n, const float *__restrict__ kpts,
                                                            unsigned long long kpt_row0, float radius, int n_sample,
                                                            unsigned long long seed, int key_bits, int center, float scale,
                                                            int32_t *idx, int32_t *__restrict__ counts, float *patches) {
    __shared__ Shared sh;
    const unsigned q = blockIdx.x;
    const float qx = kpts[(size_t)3 * q], qy = kpts[(size_t)3 * q + 1], qz = kpts[(size_t)3 * q + 2];
    const float cx = center ? qx : 0.0f, cy = center ? qy : 0.0f, cz = center ? qz : 0.0f;
    const unsigned count = radius_patch_row(
        sh, pc, (unsigned)n, qx, qy, qz, radius, n_sample, kpt_row0 + q, seed, key_bits, idx + (size_t)q * n_sample,
        patches + (size_t)q * n_sample * 3, [=](float px, float py, float pz, float *out) {
            out[0] = __fmul_rn(__fsub_rn(px, cx), scale);
            out[1] = __fmul_rn(__fsub_rn(py, cy), scale);
            out[2] = __fmul_rn(__fsub_rn(pz, cz), scale);
        });
    if (threadIdx.x == 0) counts[q] = (int32_t)count;
}

}  // namespace

extern "C" int epn_radius_patches_f32(const float *pc, int n, const float *kpts, int k, int64_t kpt_row0, float radius,
                                      int n_sample, uint64_t seed, int key_bits, int center, float scale, int32_t *idx,
                                      int32_t *counts, float *patches, epn_stream_t stream) {
    // every argument is checked before the first HIP runtime call
    if (n < 1 || k < 0 || n_sample < 1 || n_sample > 8192 || key_bits < 1 || key_bits > 32) return EPN_EINVAL;
    if (!std::isfinite(radius) || !(radius > 0.0f) || (center != 0 && center != 1)) return EPN_EINVAL;
    if (k == 0) return 0;
    if (!pc || !kpts || !idx || !counts || !patches) return EPN_EINVAL;
    EPN_LAUNCH(radius_patches_kernel, dim3((unsigned)k), dim3(PT), 0, epn_stream(stream), pc, n, kpts,
               (unsigned long long)kpt_row0, radius, n_sample, (unsigned long long)seed, key_bits, center, scale, idx, counts,
               patches);
    EPN_CHECK_LAUNCH();
    return 0;
}
