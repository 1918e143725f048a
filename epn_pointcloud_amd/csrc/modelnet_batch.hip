// ModelNet training batches for gfx950: a ragged set of raw clouds -> the [B, n_sample, 3] tensor, the rotations and the anchor
// labels that ClsSO3ConvModel, RegSO3ConvModel and their losses take.  Replaces the host path of the reference's loaders
// (SPConvNets/datasets/modelnet40.py:50-80 and :115-160), which builds every sample in a DataLoader worker:
// pctk.uniform_resample_np (np.random.choice, vgtk/vgtk/pc/sample.py:16-36), p3dtk.normalize_np (vgtk/vgtk/point3d/normalize.py:
// 30-34), pctk.rotate_point_cloud with scipy's Rotation.random() (vgtk/vgtk/pc/augmentation.py:58-89) and rotation_distance_np
// against the anchors (vgtk/vgtk/functional/rotation.py:350-369).  Its draws are numpy's and scipy's and cannot be reproduced on
// a GPU; the library defines its own deterministic form of the same semantics (include/epn_so3conv.h epn_modelnet_batch_f32,
// DESIGN.md 3.1f).  For cloud b with n_b rows and identity Q = ids ? ids[b] : b -- every draw depends on (seed, Q) only:
//
//   selection   patch_extract.hip's rule with every point a member: key(i) = word0(Philox4x32-10(i, Q, seed)) >> (32 - key_bits);
//               n_b >= n_sample: the n_sample indices smallest in (key, i), in ascending i; n_b < n_sample: slots 0..n_b-1 are
//               0..n_b-1 and slot j >= n_b is word1(Philox4x32-10(j, Q, seed)) mod n_b
//   normalise   fp64: c = mean of the n_sample selected rows (duplicates counted), s = max |p - c| over them, p' = (p - c) / s
//   rotation    mode 1: Shoemake's quaternion from w = Philox4x32-10(2^32, Q, seed), u_k = (w[k] + 0.5) / 2^32; its matrix in
//               fp64, rounded once to fp32: that is R.  mode 0: I.  mode 2: R_in[b].
//   outputs     pc_plain = p' rounded once; pc_out = R p' in fp64 FROM THE ROUNDED R, rounded once
//   label       R_label = arg max_i tr(A_i^T R), nine fp64 products in row-major order, the lowest i on a tie;
//               R_res = A_label^T R in fp64, rounded once
//   status      8 offsets of the cloud descending or outside [0, m]; else 1 empty; else 4 a non-finite coordinate among the
//               selected rows; else 2 s == 0.  Such a cloud reads nothing out of range; pc_out, pc_plain, R_res zeros, idx -1.
//
// Geometry: ONE 256-thread workgroup per cloud, one launch per call.
//   select    n_b > n_sample only: three sweeps of the keys with a 2048-bin LDS histogram (11 + 11 + 10 bits) give the threshold
//             key T and the number of key == T members to take; a fourth sweep compacts in ascending index.  Both steps are
//             key_select.h, shared with patch_extract.hip.  idx is written to its global row and read back by the workgroup
//             after a block-scope fence and a barrier.
//   centroid  gather pass over the n_sample slots, FIXED REDUCTION ORDER in fp64: thread t adds slots t, t + 256, ... in
//             ascending order; an xor tree over the wave (epn_wave_sum, s = 32..1: fp addition commutes, so every lane
//             ends with the same bits); the four wave sums are added in wave order by every thread.  The order depends on
//             n_sample only and the geometry is fixed by the launcher: bitwise repeatable.  The same pass looks for non-finite
//             coordinates.
//   extent    gather pass for max |p - c|^2 (a maximum does not depend on its order), one sqrt
//   rotate    wave 0: every lane computes the quaternion and R (the same bits); lane a takes anchor a's trace; every lane scans
//             the traces (wave shuffles) in ascending i on a strict >; lane 0 writes R, R_label, R_res and leaves the rounded R
//             in LDS
//   write     pass over the slots: pc_plain, pc_out, and idx = -1 for a cloud with a status
// No global atomics, no workspace, no workgroup talks to another, every loop is bounded by n_b or n_sample, every point row
// read is offsets[b] + i with 0 <= i < n_b inside the checked [0, m].
#include <cmath>

#include "epn_reduce.h"
#include "key_select.h"
#include "rotation_math.h"

namespace {

using namespace epn_keysel;

struct BatchShared {
    Shared sel;
    double part[PW][3];            // per-wave partial sums / maxima
    float R[9];                    // the rounded rotation
    int flag[PW];
};

// The cloud row of slot j: below un by construction; the clamp keeps the address inside the cloud whatever the row holds.
__device__ __forceinline__ unsigned slot_row(const int32_t *irow, unsigned j, unsigned un) {
    const unsigned i = (unsigned)irow[j];
    return i < un ? i : un - 1u;
}

__global__ __launch_bounds__(PT) void modelnet_batch_kernel(const float *__restrict__ points, int m,
                                                            const int32_t *__restrict__ offsets,
                                                            const int64_t *__restrict__ ids, int n_sample, unsigned long long seed,
                                                            int key_bits, int rot_mode, const float *__restrict__ R_in,
                                                            const float *__restrict__ anchors, int A, float *__restrict__ pc_out,
                                                            float *__restrict__ pc_plain, int32_t *idx, float *__restrict__ R,
                                                            int32_t *__restrict__ R_label, float *__restrict__ R_res,
                                                            int32_t *__restrict__ status) {
    __shared__ BatchShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t cloud = blockIdx.x;
    const unsigned long long Q = ids ? (unsigned long long)ids[cloud] : (unsigned long long)cloud;
    const unsigned ns = (unsigned)n_sample;
    int32_t *irow = idx + cloud * ns;

    const int o0 = offsets[cloud], o1 = offsets[cloud + 1];
    int st = 0;
    if (o0 < 0 || o1 > m || o1 < o0) st = 8;
    else if (o1 == o0) st = 1;
    const unsigned un = st ? 0u : (unsigned)(o1 - o0);
    const float *__restrict__ prow = points + (size_t)3 * (size_t)(st ? 0 : o0);   // not read when st != 0

    double cx = 0.0, cy = 0.0, cz = 0.0, s = 0.0;
    if (st == 0) {                                     // uniform over the workgroup: barriers inside are safe
        // ---- select
        if (un > ns) {
            unsigned b1 = 0u, b2 = 0u, b3 = 0u, take = 0u;
            clear_hist(sh.sel);
            __syncthreads();
            for (unsigned base = 0; base < un; base += PT) {
                const unsigned i = base + tid;
                if (i < un) atomicAdd(&sh.sel.hist[key_of(i, Q, seed, key_bits) >> 21], 1u);
            }
            search_hist(sh.sel, ns, b1, take);
            clear_hist(sh.sel);
            __syncthreads();
            for (unsigned base = 0; base < un; base += PT) {
                const unsigned i = base + tid;
                if (i < un) {
                    const unsigned key = key_of(i, Q, seed, key_bits);
                    if ((key >> 21) == b1) atomicAdd(&sh.sel.hist[(key >> 10) & 0x7FFu], 1u);
                }
            }
            search_hist(sh.sel, take, b2, take);
            clear_hist(sh.sel);
            __syncthreads();
            const unsigned hi22 = (b1 << 11) | b2;
            for (unsigned base = 0; base < un; base += PT) {
                const unsigned i = base + tid;
                if (i < un) {
                    const unsigned key = key_of(i, Q, seed, key_bits);
                    if ((key >> 10) == hi22) atomicAdd(&sh.sel.hist[key & 0x3FFu], 1u);
                }
            }
            search_hist(sh.sel, take, b3, take);
            const unsigned T = (hi22 << 10) | b3;
            Emit em;
            for (unsigned base = 0; base < un; base += PT) {
                const unsigned i = base + tid;
                bool less = false, tie = false;
                if (i < un) {
                    const unsigned key = key_of(i, Q, seed, key_bits);
                    less = key < T;
                    tie = key == T;
                }
                unsigned pos;
                if (emit_step(sh.sel, em, less, tie, take, pos) && pos < ns) irow[pos] = (int32_t)i;
            }
        } else {
            for (unsigned j = tid; j < ns; j += PT)
                irow[j] = (int32_t)(j < un ? j : epn::philox::philox4x32_10((unsigned long long)j, Q, seed).w[1] % un);
        }
        __threadfence_block();
        __syncthreads();                               // the idx row is written and visible to the workgroup

        // ---- centroid (fixed order) and the non-finite check
        double ax = 0.0, ay = 0.0, az = 0.0;
        int bad = 0;
        for (unsigned j = tid; j < ns; j += PT) {
            const unsigned i = slot_row(irow, j, un);
            const float x = prow[(size_t)3 * i], y = prow[(size_t)3 * i + 1], z = prow[(size_t)3 * i + 2];
            bad |= !(std::isfinite(x) && std::isfinite(y) && std::isfinite(z));
            ax += (double)x; ay += (double)y; az += (double)z;
        }
        ax = epn_wave_sum(ax); ay = epn_wave_sum(ay); az = epn_wave_sum(az);
        const unsigned long long anybad = __ballot(bad != 0);
        if (lane == 0) {
            sh.part[wave][0] = ax; sh.part[wave][1] = ay; sh.part[wave][2] = az;
            sh.flag[wave] = anybad != 0ull;
        }
        __syncthreads();
        ax = 0.0; ay = 0.0; az = 0.0;
        bad = 0;
#pragma unroll
        for (int w = 0; w < PW; ++w) {
            ax += sh.part[w][0]; ay += sh.part[w][1]; az += sh.part[w][2];
            bad |= sh.flag[w];
        }
        cx = ax / (double)ns; cy = ay / (double)ns; cz = az / (double)ns;
        __syncthreads();                               // part is rewritten below

        if (bad) {
            st = 4;
        } else {
            // ---- extent
            double d2 = 0.0;
            for (unsigned j = tid; j < ns; j += PT) {
                const unsigned i = slot_row(irow, j, un);
                const double dx = (double)prow[(size_t)3 * i] - cx, dy = (double)prow[(size_t)3 * i + 1] - cy,
                             dz = (double)prow[(size_t)3 * i + 2] - cz;
                d2 = fmax(d2, dx * dx + dy * dy + dz * dz);
            }
            d2 = epn_wave_max(d2);
            if (lane == 0) sh.part[wave][0] = d2;
            __syncthreads();
            d2 = 0.0;
#pragma unroll
            for (int w = 0; w < PW; ++w) d2 = fmax(d2, sh.part[w][0]);
            s = sqrt(d2);
            if (!(s > 0.0)) st = 2;
        }
    }

    // ---- rotate: wave 0
    if (wave == 0) {
        double Rm[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
        float Rf[9];
        if (rot_mode == 1) {
            const epn::philox::u32x4 w = epn::philox::philox4x32_10(1ull << 32, Q, seed);
            const double u0 = ((double)w.w[0] + 0.5) / 4294967296.0, u1 = ((double)w.w[1] + 0.5) / 4294967296.0,
                         u2 = ((double)w.w[2] + 0.5) / 4294967296.0;
            const double two_pi = 6.283185307179586476925286766559;
            const double r1 = sqrt(1.0 - u0), r2 = sqrt(u0);
            const double q[4] = {r2 * cos(two_pi * u2), r1 * sin(two_pi * u1), r1 * cos(two_pi * u1), r2 * sin(two_pi * u2)};
            epn_rot::quat_matrix(q, Rm);               // q = (w, x, y, z)
        }
#pragma unroll
        for (int e = 0; e < 9; ++e) Rf[e] = rot_mode == 2 ? R_in[9 * cloud + e] : (float)Rm[e];
        int best = 0;
        if (anchors) {                                 // every lane scans the 64 traces in ascending i: the same label in all
            double tr = 0.0;
            if (lane < A) {
                const float *Aa = anchors + 9 * lane;
#pragma unroll
                for (int e = 0; e < 9; ++e) tr += (double)Aa[e] * (double)Rf[e];
            }
            double best_tr = __shfl(tr, 0, 64);
            for (int i = 1; i < A; ++i) {
                const double t = __shfl(tr, i, 64);
                if (t > best_tr) {
                    best = i;
                    best_tr = t;
                }
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int e = 0; e < 9; ++e) {
                R[9 * cloud + e] = Rf[e];
                sh.R[e] = Rf[e];
            }
            if (anchors) {
                R_label[cloud] = best;
                const float *Al = anchors + 9 * best;
#pragma unroll
                for (int r = 0; r < 3; ++r)            // A_label^T R
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        R_res[9 * cloud + 3 * r + c] =
                            st ? 0.0f
                               : (float)((double)Al[r] * (double)Rf[c] + (double)Al[3 + r] * (double)Rf[3 + c] +
                                         (double)Al[6 + r] * (double)Rf[6 + c]);
            }
            status[cloud] = st;
        }
    }
    __syncthreads();                                   // sh.R is written

    // ---- write
    float *orow = pc_out + cloud * ns * 3;
    float *plrow = pc_plain ? pc_plain + cloud * ns * 3 : nullptr;
    if (st) {
        for (unsigned j = tid; j < ns; j += PT) {
            irow[j] = -1;
            orow[3 * (size_t)j] = 0.0f; orow[3 * (size_t)j + 1] = 0.0f; orow[3 * (size_t)j + 2] = 0.0f;
            if (plrow) { plrow[3 * (size_t)j] = 0.0f; plrow[3 * (size_t)j + 1] = 0.0f; plrow[3 * (size_t)j + 2] = 0.0f; }
        }
        return;
    }
    double Rd[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) Rd[e] = (double)sh.R[e];
    for (unsigned j = tid; j < ns; j += PT) {
        const unsigned i = slot_row(irow, j, un);
        const double x = ((double)prow[(size_t)3 * i] - cx) / s, y = ((double)prow[(size_t)3 * i + 1] - cy) / s,
                     z = ((double)prow[(size_t)3 * i + 2] - cz) / s;
        if (plrow) { plrow[3 * (size_t)j] = (float)x; plrow[3 * (size_t)j + 1] = (float)y; plrow[3 * (size_t)j + 2] = (float)z; }
        orow[3 * (size_t)j] = (float)(Rd[0] * x + Rd[1] * y + Rd[2] * z);
        orow[3 * (size_t)j + 1] = (float)(Rd[3] * x + Rd[4] * y + Rd[5] * z);
        orow[3 * (size_t)j + 2] = (float)(Rd[6] * x + Rd[7] * y + Rd[8] * z);
    }
}

}  // namespace

extern "C" int epn_modelnet_batch_f32(const float *points, int m, const int32_t *offsets, int b, const int64_t *ids,
                                      int n_sample, uint64_t seed, int key_bits, int rot_mode, const float *R_in,
                                      const float *anchors, int A, float *pc_out, float *pc_plain, int32_t *idx, float *R,
                                      int32_t *R_label, float *R_res, int32_t *status, epn_stream_t stream) {
    // every argument is checked before the first HIP runtime call
    if (b < 0 || m < 0 || n_sample < 1 || n_sample > 8192 || key_bits < 1 || key_bits > 32) return EPN_EINVAL;
    if (rot_mode < 0 || rot_mode > 2 || (rot_mode == 2 && !R_in)) return EPN_EINVAL;
    if (anchors && (A < 1 || A > 64)) return EPN_EINVAL;
    if (b == 0) return 0;
    if (!offsets || !pc_out || !idx || !R || !status || (m > 0 && !points)) return EPN_EINVAL;
    if (anchors && (!R_label || !R_res)) return EPN_EINVAL;
    EPN_LAUNCH(modelnet_batch_kernel, dim3((unsigned)b), dim3(PT), 0, epn_stream(stream), points, m, offsets, ids, n_sample,
               (unsigned long long)seed, key_bits, rot_mode, R_in, anchors, A, pc_out, pc_plain, idx, R, R_label, R_res, status);
    EPN_CHECK_LAUNCH();
    return 0;
}
