// One row of the patch extraction inside ONE 256-thread workgroup: the sweep body that patch_extract.hip (one fragment, keypoints
// given as rows) and pair_batch.hip (a batch of fragment pairs, keypoints drawn from correspondences) share.  The rule is
// include/epn_so3conv.h epn_radius_patches_f32; the geometry is described at the top of patch_extract.hip.
//   in_radius         the membership test, in individually rounded fp32 (__fsub_rn / __fmul_rn / __fadd_rn: no fma contraction)
//   radius_patch_row  count -> (count > n_sample: the threshold key, three histogram levels) -> emit in ascending index ->
//                     upsample; writes the row's idx and patch slots and returns count.  What a selected point's patch slot
//                     holds is the caller's: value(px, py, pz, out) with the point's coordinates as they are in the fragment.
#pragma once
#include "epn_common.h"
#include "key_select.h"

namespace epn_keysel {

__device__ __forceinline__ bool in_radius(const float *__restrict__ pc, unsigned i, float qx, float qy, float qz, float r2,
                                          float &px, float &py, float &pz) {
    px = pc[(size_t)3 * i]; py = pc[(size_t)3 * i + 1]; pz = pc[(size_t)3 * i + 2];
    const float dx = __fsub_rn(px, qx), dy = __fsub_rn(py, qy), dz = __fsub_rn(pz, qz);
    const float d2 = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
    return d2 <= r2;
}

// pc: the fragment's un rows (un == 0 reads nothing and gives count 0); (qx, qy, qz): the keypoint; Q: its global row.
// irow / prow: the row's n_sample idx slots and 3 * n_sample patch slots in global memory.  Every thread of the workgroup calls
// it with the same arguments (barriers inside) and gets the same count.
template <class Value>
__device__ __forceinline__ unsigned radius_patch_row(Shared &sh, const float *__restrict__ pc, unsigned un, float qx, float qy,
                                                     float qz, float radius, int n_sample, unsigned long long Q,
                                                     unsigned long long seed, int key_bits, int32_t *irow, float *prow,
                                                     Value value) {
    const int tid = threadIdx.x;
    const float r2 = __fmul_rn(radius, radius);
    float px, py, pz;

    // ---- pass 1: count + histogram of key bits 31..21
    clear_hist(sh);
    __syncthreads();
    for (unsigned base = 0; base < un; base += PT) {
        const unsigned i = base + tid;
        if (i < un && in_radius(pc, i, qx, qy, qz, r2, px, py, pz))
            atomicAdd(&sh.hist[key_of(i, Q, seed, key_bits) >> 21], 1u);
    }
    unsigned b1 = 0u, b2 = 0u, b3 = 0u, take = 0u;
    const unsigned count = search_hist(sh, (unsigned)n_sample, b1, take);

    if (count <= 1u) {
        for (int j = tid; j < n_sample; j += PT) {
            irow[j] = -1;
            prow[3 * j] = 0.0f; prow[3 * j + 1] = 0.0f; prow[3 * j + 2] = 0.0f;
        }
        return count;
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
                const unsigned key = key_of(i, Q, seed, key_bits);
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
                const unsigned key = key_of(i, Q, seed, key_bits);
                if ((key >> 10) == hi22) atomicAdd(&sh.hist[key & 0x3FFu], 1u);
            }
        }
        search_hist(sh, take, b3, take);
        T = (hi22 << 10) | b3;
    }

    // ---- emit: ascending index; `less` lanes always, `tie` lanes while their rank among the ties is below `take`
    Emit em;
    for (unsigned base = 0; base < un; base += PT) {
        const unsigned i = base + tid;
        bool less = false, tie = false;
        if (i < un && in_radius(pc, i, qx, qy, qz, r2, px, py, pz)) {
            if (all) {
                less = true;
            } else {
                const unsigned key = key_of(i, Q, seed, key_bits);
                less = key < T;
                tie = key == T;
            }
        }
        unsigned pos;
        if (emit_step(sh, em, less, tie, take, pos) && pos < (unsigned)n_sample) {
            irow[pos] = (int32_t)i;
            value(px, py, pz, prow + 3 * (size_t)pos);
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
    return count;
}

}  // namespace epn_keysel
