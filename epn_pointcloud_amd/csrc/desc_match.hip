// Descriptor matching for gfx950: exact nearest neighbour in descriptor space in both directions between the keypoints of
// two fragments, the mutual check and the inlier count under a ground-truth transform, for every fragment pair of a scene in
// one launch each.  Replaces the host block of the reference's evaluation (SPConvNets/datasets/evaluation_3dmatch.py:77-100:
// two sklearn KDTrees, tgt -> src -> tgt, hom_transform, distances < tau1).  Specification: include/epn_so3conv.h
// (epn_nn_match_f32, epn_match_inliers_f64) and DESIGN.md 3.1a.
//
//   d2(i,j) = sum_c (a_ic - b_jc)^2 in fp32 from the differences; the nearest admissible (valid, finite d2) row of the other
//   fragment, ties to the lowest index; (-1, +inf) for an invalid query or one without an admissible candidate.
//
// Geometry: a 3-D grid (query tile, target segment, pair x direction).  A 256-thread workgroup owns 256 query rows, one per
// lane, held in registers (C padded with zeros to the instance's width CP, which changes no distance).  It streams its segment
// of MSEG target rows through LDS in tiles of TT rows; every lane reads the same target element (an LDS broadcast,
// ds_read_b128), does CP subtractions and CP FMAs per candidate and keeps a running best (d2, j) with a strict `<` in
// ascending j.  Invalid target rows are skipped by their mask byte, staged with the tile (a wave-uniform branch).
// Segments are combined through a packed key (bits(d2) << 32) | j and one 64-bit atomicMin per lane on a workspace that a
// memset on the call's stream sets to all-ones: for finite d2 >= 0 the float bits order as unsigned integers and the lowest j
// wins ties by construction; the minimum is associative and commutative, so the result is bitwise repeatable.  A finish kernel
// unpacks the keys.  Every loop is bounded by a row count or by CP; no workgroup waits on another and nothing spins.
//
// The mutual / inlier kernel runs one workgroup per pair over its tgt rows in fp64; the two counts are an integer reduction
// inside the workgroup (wave shuffles, then LDS), one result per pair, no atomics.
#include <cmath>

#include "epn_common.h"
#include "scene_tables.h"

namespace {

using epn::check_scene;                // grid.z = 2 P <= 65534: scene_tables.h refuses more than 32767 pairs

constexpr int MT = 256;            // threads per workgroup = query rows per tile
constexpr int MW = MT / 64;        // waves
constexpr int MSEG = 512;          // target rows per segment (grid.y)

template <int CP>
__global__ __launch_bounds__(MT) void nn_match_kernel(const float *__restrict__ feats, int C, const uint8_t *__restrict__ valid,
                                                      const int64_t *__restrict__ frag_off, const int32_t *__restrict__ pairs,
                                                      const int64_t *__restrict__ out_off, unsigned long long *best) {
    constexpr int TT = CP <= 64 ? 4096 / CP : 32;          // target rows per LDS tile: 16 KB at most
    __shared__ __attribute__((aligned(16))) float tile[TT * CP];
    __shared__ unsigned char tvalid[TT];
    const int tid = threadIdx.x;
    const int p = blockIdx.z >> 1, dir = blockIdx.z & 1;  // dir 0: src rows query the tgt fragment; 1: the reverse
    const int fs = pairs[2 * p], ft = pairs[2 * p + 1];
    const int fq = dir ? ft : fs, fc = dir ? fs : ft;
    const int64_t q0 = frag_off[fq], c0 = frag_off[fc];
    const int nq = (int)(frag_off[fq + 1] - q0), nc = (int)(frag_off[fc + 1] - c0);
    const int qbase = (int)blockIdx.x * MT, s0 = (int)blockIdx.y * MSEG;
    if (qbase >= nq || s0 >= nc) return;                   // the grid is sized for the largest fragment (whole workgroup leaves)
    const int s1 = s0 + MSEG < nc ? s0 + MSEG : nc;
    const int64_t o0 = out_off[p] + (dir ? frag_off[fs + 1] - frag_off[fs] : 0);

    const int qi = qbase + tid;
    const bool live = qi < nq && (valid == nullptr || valid[q0 + qi] != 0);
    const float *qrow = feats + (size_t)(q0 + (qi < nq ? qi : qbase)) * C;
    float q[CP];
    if ((C & 3) == 0 && (reinterpret_cast<uintptr_t>(feats) & 15u) == 0) {     // every row is 16-byte aligned
#pragma unroll
        for (int c = 0; c < CP; c += 4) {
            const f32x4 v = c < C ? *reinterpret_cast<const f32x4 *>(qrow + c) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            q[c] = v.x; q[c + 1] = v.y; q[c + 2] = v.z; q[c + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int c = 0; c < CP; ++c) q[c] = c < C ? qrow[c] : 0.0f;
    }
    for (int e = tid; e < TT * CP; e += MT) tile[e] = 0.0f;    // the padding columns stay zero
    __syncthreads();

    float bd = INFINITY;
    int bj = -1;
    for (int t0 = s0; t0 < s1; t0 += TT) {
        const int nt = s1 - t0 < TT ? s1 - t0 : TT;
        const float *src = feats + (size_t)(c0 + t0) * C;       // nt consecutive rows: one contiguous block
        for (int e = tid; e < nt * C; e += MT) {
            const int t = e / C;
            tile[t * CP + (e - t * C)] = src[e];
        }
        for (int t = tid; t < TT; t += MT) tvalid[t] = t < nt && (valid == nullptr || valid[c0 + t0 + t] != 0);
        __syncthreads();
        for (int t = 0; t < nt; ++t) {
            if (!tvalid[t]) continue;                          // the same byte for every lane
            const float *b = tile + t * CP;
            float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
#pragma unroll
            for (int c = 0; c < CP; c += 4) {
                const f32x4 v = *reinterpret_cast<const f32x4 *>(b + c);
                const float d0 = q[c] - v.x, d1 = q[c + 1] - v.y, d2 = q[c + 2] - v.z, d3 = q[c + 3] - v.w;
                a0 = __fmaf_rn(d0, d0, a0);
                a1 = __fmaf_rn(d1, d1, a1);
                a2 = __fmaf_rn(d2, d2, a2);
                a3 = __fmaf_rn(d3, d3, a3);
            }
            const float d2 = (a0 + a1) + (a2 + a3);
            if (d2 < bd) { bd = d2; bj = t0 + t; }             // +inf and NaN never pass: only finite d2 is admitted
        }
        __syncthreads();
    }
    if (live && bj >= 0)
        atomicMin(best + o0 + qi, ((unsigned long long)__float_as_uint(bd) << 32) | (unsigned long long)(unsigned)bj);
}

__global__ __launch_bounds__(MT) void nn_finish_kernel(const unsigned long long *__restrict__ best, long long n,
                                                       int32_t *__restrict__ nn_idx, float *__restrict__ nn_d2) {
    const long long e = (long long)blockIdx.x * MT + threadIdx.x;
    if (e >= n) return;
    const unsigned long long key = best[e];
    const bool none = key == ~0ull;
    nn_idx[e] = none ? -1 : (int32_t)(unsigned)(key & 0xFFFFFFFFull);
    nn_d2[e] = none ? INFINITY : __uint_as_float((unsigned)(key >> 32));
}

__global__ __launch_bounds__(MT) void match_inliers_kernel(const float *__restrict__ kp, const int64_t *__restrict__ frag_off,
                                                           const int32_t *__restrict__ pairs, const int64_t *__restrict__ out_off,
                                                           const int64_t *__restrict__ tgt_off, const int32_t *__restrict__ nn_idx,
                                                           const double *__restrict__ gt, double tau1,
                                                           int32_t *__restrict__ match_src, double *__restrict__ match_dist,
                                                           int32_t *__restrict__ n_match, int32_t *__restrict__ n_inlier) {
    __shared__ int wsum[MW][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = blockIdx.x;
    const int fs = pairs[2 * p], ft = pairs[2 * p + 1];
    const int64_t r0s = frag_off[fs], r0t = frag_off[ft];
    const int ns = (int)(frag_off[fs + 1] - r0s), nt = (int)(frag_off[ft + 1] - r0t);
    const int32_t *nn_src = nn_idx + out_off[p], *nn_tgt = nn_src + ns;
    const double *T = gt + (size_t)16 * p;
    int32_t *msrc = match_src + tgt_off[p];
    double *mdist = match_dist + tgt_off[p];
    int matches = 0, inliers = 0;
    for (int j = tid; j < nt; j += MT) {
        const int s = nn_tgt[j];
        const bool mutual = s >= 0 && s < ns && nn_src[s] == j;
        double dist = INFINITY;
        if (mutual) {
            const float *a = kp + (size_t)3 * (r0s + s), *b = kp + (size_t)3 * (r0t + j);
            const double x = b[0], y = b[1], z = b[2];
            const double dx = (double)a[0] - (T[0] * x + T[1] * y + T[2] * z + T[3]);
            const double dy = (double)a[1] - (T[4] * x + T[5] * y + T[6] * z + T[7]);
            const double dz = (double)a[2] - (T[8] * x + T[9] * y + T[10] * z + T[11]);
            dist = sqrt(dx * dx + dy * dy + dz * dz);
            matches += 1;
            inliers += dist < tau1 ? 1 : 0;
        }
        msrc[j] = mutual ? s : -1;
        mdist[j] = dist;
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        matches += __shfl_down(matches, s, 64);
        inliers += __shfl_down(inliers, s, 64);
    }
    if (lane == 0) { wsum[wave][0] = matches; wsum[wave][1] = inliers; }
    __syncthreads();
    if (tid == 0) {
        int m = 0, i = 0;
#pragma unroll
        for (int w = 0; w < MW; ++w) { m += wsum[w][0]; i += wsum[w][1]; }
        n_match[p] = m;
        n_inlier[p] = i;
    }
}

}  // namespace

extern "C" size_t epn_nn_match_workspace_bytes(int64_t out_rows) {
    return out_rows > 0 ? (size_t)out_rows * sizeof(unsigned long long) : 0;
}

extern "C" int epn_nn_match_f32(const float *feats, int64_t R, int C, const uint8_t *valid, int F, const int64_t *frag_off_host,
                                const int64_t *frag_off, int P, const int32_t *pairs_host, const int32_t *pairs,
                                const int64_t *out_off_host, const int64_t *out_off, void *workspace, size_t workspace_bytes,
                                int32_t *nn_idx, float *nn_d2, epn_stream_t stream) {
    // every argument is checked before the first HIP runtime call
    if (C < 1 || C > 128) return EPN_EINVAL;
    int64_t max_rows = 0;
    const int rc = check_scene(R, F, frag_off_host, P, pairs_host, out_off_host, nullptr, &max_rows);
    if (rc != 0) return rc;
    const int64_t n_out = out_off_host[P];
    if (n_out == 0) return 0;
    if (!feats || !frag_off || !pairs || !out_off || !nn_idx || !nn_d2) return EPN_ENULL;
    if (!workspace || workspace_bytes < epn_nn_match_workspace_bytes(n_out)) return EPN_EWORKSPACE;
    hipStream_t st = epn_stream(stream);
    unsigned long long *best = static_cast<unsigned long long *>(workspace);
    EPN_HIP(hipMemsetAsync(best, 0xFF, (size_t)n_out * sizeof(unsigned long long), st));
    if (max_rows > 0) {
        const dim3 grid((unsigned)epn_cdiv(max_rows, MT), (unsigned)epn_cdiv(max_rows, MSEG), (unsigned)(2 * P));
#define EPN_NN_INSTANCE(CP)                                                                                            \
    EPN_LAUNCH(nn_match_kernel<CP>, grid, dim3(MT), 0, st, feats, C, valid, frag_off, pairs, out_off, best)
        if (C <= 8) EPN_NN_INSTANCE(8);
        else if (C <= 32) EPN_NN_INSTANCE(32);
        else if (C <= 64) EPN_NN_INSTANCE(64);
        else if (C <= 96) EPN_NN_INSTANCE(96);
        else EPN_NN_INSTANCE(128);
#undef EPN_NN_INSTANCE
        EPN_CHECK_LAUNCH();
    }
    EPN_LAUNCH_AUX(nn_finish_kernel, dim3((unsigned)epn_cdiv(n_out, MT)), dim3(MT), 0, st, best, (long long)n_out, nn_idx, nn_d2);
    EPN_CHECK_LAUNCH();
    return 0;
}

extern "C" int epn_match_inliers_f64(const float *kp_xyz, int64_t R, int F, const int64_t *frag_off_host, const int64_t *frag_off,
                                     int P, const int32_t *pairs_host, const int32_t *pairs, const int64_t *out_off_host,
                                     const int64_t *out_off, const int64_t *tgt_off_host, const int64_t *tgt_off,
                                     const int32_t *nn_idx, const double *gt, double tau1, int32_t *match_src,
                                     double *match_dist, int32_t *n_match, int32_t *n_inlier, epn_stream_t stream) {
    if (std::isnan(tau1)) return EPN_EINVAL;
    if (!tgt_off_host) return EPN_ENULL;
    int64_t max_rows = 0;
    const int rc = check_scene(R, F, frag_off_host, P, pairs_host, out_off_host, tgt_off_host, &max_rows);
    if (rc != 0) return rc;
    if (P == 0) return 0;
    if (!frag_off || !pairs || !out_off || !tgt_off || !gt || !n_match || !n_inlier) return EPN_ENULL;
    if (out_off_host[P] > 0 && (!kp_xyz || !nn_idx)) return EPN_ENULL;
    if (tgt_off_host[P] > 0 && (!match_src || !match_dist)) return EPN_ENULL;
    EPN_LAUNCH(match_inliers_kernel, dim3((unsigned)P), dim3(MT), 0, epn_stream(stream), kp_xyz, frag_off, pairs, out_off, tgt_off,
               nn_idx, gt, tau1, match_src, match_dist, n_match, n_inlier);
    EPN_CHECK_LAUNCH();
    return 0;
}
