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
#include <cmath>

#include "epn_common.h"
#include "key_select.h"

namespace {

using namespace epn_keysel;        // PT, search_hist, emit_step: the selection shared with modelnet_batch.hip
using PatchShared = Shared;

__device__ __forceinline__ bool in_radius(const float *__restrict__ pc, unsigned i, float qx, float qy, float qz, float r2,
                                          float &px, float &py, float &pz) {
    px = pc[(size_t)3 * i]; py = pc[(size_t)3 * i + 1]; pz = pc[(size_t)3 * i + 2];
    const float dx = __fsub_rn(px, qx), dy = __fsub_rn(py, qy), dz = __fsub_rn(pz, qz);
    const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
    return d2 <= r2;
}

__device__ __forceinline__ unsigned patch_key(unsigned i, unsigned long long Q, unsigned long long seed, int key_bits) {
    return key_of(i, Q, seed, key_bits);
}

__global__ __launch_bounds__(PT) void radius_patches_kernel(const float *__restrict__ pc, int n, const float *__restrict__ kpts,
                                                            unsigned long long kpt_row0, float radius, int n_sample,
                                                            unsigned long long seed, int key_bits, int center, float scale,
                                                            int32_t *idx, int32_t *__restrict__ counts, float *patches) {
    __shared__ PatchShared sh;
    const int tid = threadIdx.x;
    const unsigned q = blockIdx.x, un = (unsigned)n;
    const unsigned long long Q = kpt_row0 + q;
    const float qx = kpts[(size_t)3 * q], qy = kpts[(size_t)3 * q + 1], qz = kpts[(size_t)3 * q + 2];
    const float r2 = __fmul_rn(radius, radius);
    int32_t *irow = idx + (size_t)q * n_sample;
    float *prow = patches + (size_t)q * n_sample * 3;
    float px, py, pz;

    // ---- pass 1: count + histogram of key bits 31..21
    clear_hist(sh);
    __syncthreads();
    for (unsigned base = 0; base < un; base += PT) {
        const unsigned i = base + tid;
        if (i < un && in_radius(pc, i, qx, qy, qz, r2, px, py, pz))
            atomicAdd(&sh.hist[patch_key(i, Q, seed, key_bits) >> 21], 1u);
    }
    unsigned b1 = 0u, b2 = 0u, b3 = 0u, take = 0u;
    const unsigned count = search_hist(sh, (unsigned)n_sample, b1, take);
    if (tid == 0) counts[q] = (int32_t)count;

    if (count <= 1u) {
        for (int j = tid; j < n_sample; j += PT) {
            irow[j] = -1;
            prow[3 * j] = 0.0f; prow[3 * j + 1] = 0.0f; prow[3 * j + 2] = 0.0f;
        }
        return;
    }

    // ---- passes 2, 3: the threshold key T = b1:b2:b3 and the number `take` of key == T members (count > n_sample only)
    const bool all = count <= (unsigned)n_sample;
    unsigned T = 0xFFFFFFFFu;
    if (!all) {
        clear_hist(sh);
        __syncthreads();
        for (unsigned base = 0; base < un; base += PT) {
            const unsigned i = base + tid;
            if (i < un && in_radius(pc, i, qx, qy, qz, r2, px, py, pz)) {
                const unsigned key = patch_key(i, Q, seed, key_bits);
                if ((key >> 21) == b1) atomicAdd(&sh.hist[(key >> 10) & 0x7FFu], 1u);
            }
        }
        search_hist(sh, take, b2, take);
        clear_hist(sh);
        __syncthreads();
        const unsigned hi22 = (b1 << 11) | b2;
        for (unsigned base = 0; base < un; base += PT) {
            const unsigned i = base + tid;
            if (i < un && in_radius(pc, i, qx, qy, qz, r2, px, py, pz)) {
                const unsigned key = patch_key(i, Q, seed, key_bits);
                if ((key >> 10) == hi22) atomicAdd(&sh.hist[key & 0x3FFu], 1u);
            }
        }
        search_hist(sh, take, b3, take);
        T = (hi22 << 10) | b3;
    }

    // ---- emit: ascending index; `less` lanes always, `tie` lanes while their rank among the ties is below `take`
    const float cx = center ? qx : 0.0f, cy = center ? qy : 0.0f, cz = center ? qz : 0.0f;
    Emit em;
    for (unsigned base = 0; base < un; base += PT) {
        const unsigned i = base + tid;
        bool less = false, tie = false;
        if (i < un && in_radius(pc, i, qx, qy, qz, r2, px, py, pz)) {
            if (all) {
                less = true;
            } else {
                const unsigned key = patch_key(i, Q, seed, key_bits);
                less = key < T;
                tie = key == T;
            }
        }
        unsigned pos;
        if (emit_step(sh, em, less, tie, take, pos) && pos < (unsigned)n_sample) {
            irow[pos] = (int32_t)i;
            prow[3 * (size_t)pos] = __fmul_rn(__fsub_rn(px, cx), scale);
            prow[3 * (size_t)pos + 1] = __fmul_rn(__fsub_rn(py, cy), scale);
            prow[3 * (size_t)pos + 2] = __fmul_rn(__fsub_rn(pz, cz), scale);
        }
    }

    // ---- upsample (1 < count < n_sample): draw with replacement from the row's first `count` slots
    if (count < (unsigned)n_sample) {
        __threadfence_block();
        __syncthreads();                               // the row's first `count` slots are written and visible to the workgroup
        for (unsigned j = count + tid; j < (unsigned)n_sample; j += PT) {
            const unsigned src = epn::philox::philox4x32_10((unsigned long long)j, Q, seed).w[1] % count;
            irow[j] = irow[src];
            prow[3 * (size_t)j] = prow[3 * (size_t)src];
            prow[3 * (size_t)j + 1] = prow[3 * (size_t)src + 1];
            prow[3 * (size_t)j + 2] = prow[3 * (size_t)src + 2];
        }
    }
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
