// Pairwise registration for gfx950: the rigid transform between the two fragments of every pair of a scene from its mutual
// matches alone, by hypothesise-and-verify (RANSAC) over three-point samples and one least-squares refit.  The stage after
// epn_match_inliers_f64 for a caller without ground truth; the host tool usually run for it is open3d's
// registration_ransac_based_on_feature_matching.  Specification: include/epn_so3conv.h (epn_ransac_register_f64) and
// DESIGN.md 3.1c.
//
// Three launches on the call's stream, 256-thread workgroups:
//   compact  one workgroup per pair walks the pair's tgt rows 256 at a time; a row j with 0 <= s = match_src[j] < n_src is a
//            correspondence.  Its rank among the pair's correspondences = the count so far + the waves before it (LDS) + the
//            lanes before it (ballot, popcount): ascending j, no atomics.  Writes (kp_src[s], kp_tgt[j]) as six floats to the
//            workspace and the pair's count M.  s is used as an index only after the range check.
//   score    grid ceil(H / 256) x P, lane = hypothesis h.  The lane draws i_k = word_k(Philox(h, pair0 + p, seed)) mod M, fits
//            the three correspondences (rigid_fit.h) and keeps R, t in registers; the workgroup then streams the pair's
//            correspondences through LDS in tiles of 256 (6 KB), every lane reading the same one (a broadcast), widening it to
//            fp64 and counting |x - (R y + t)|^2 < tau^2 in a register.  Writes hyp_count (-1: rejected).
//   finish   one workgroup per pair: integer arg-max of hyp_count through the key (count + 1) << 32 | ~h (largest count, lowest
//            h); every thread re-derives the winner's R, t (the same instructions on the same values); three passes over the
//            correspondences -- centroids of the inliers, their cross-covariance about the centroids, the residuals under the
//            refit -- in each of which thread i adds m = i, i + 256, ... in ascending order, followed by a fixed tree (xor
//            shuffles inside a wave, then (w0 + w1) + (w2 + w3) through LDS).  Thread 0 writes the pair's outputs.
// Every loop is bounded by a row count, M, H or the sweep count of the projection; the only data-dependent indices are s
// (checked) and i_k (a remainder below M); no workgroup waits on another; no atomics: two runs are bitwise equal.
#include <cmath>

#include "epn_reduce.h"
#include "philox.h"
#include "rigid_fit.h"
#include "scene_tables.h"

namespace {

constexpr int RT = 256;                  // threads per workgroup
constexpr int RWV = RT / 64;             // waves
constexpr int TILE = 256;                // correspondences per LDS tile: 6 KB
constexpr int MAX_HYP = 65536;

inline size_t corr_bytes(int64_t tgt_rows) { return ((size_t)tgt_rows * 6 * sizeof(float) + 7) & ~(size_t)7; }

__global__ __launch_bounds__(RT) void ransac_compact_kernel(const float *__restrict__ kp, const int64_t *__restrict__ frag_off,
                                                            const int32_t *__restrict__ pairs, const int64_t *__restrict__ tgt_off,
                                                            const int32_t *__restrict__ match_src, float *__restrict__ corr,
                                                            int32_t *__restrict__ count) {
    __shared__ int wcnt[RWV];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = blockIdx.x;
    const int fs = pairs[2 * p], ft = pairs[2 * p + 1];
    const int64_t r0s = frag_off[fs], r0t = frag_off[ft];
    const int ns = (int)(frag_off[fs + 1] - r0s), nt = (int)(frag_off[ft + 1] - r0t);
    const int32_t *msrc = match_src + tgt_off[p];
    float *out = corr + (size_t)6 * tgt_off[p];
    int base = 0;                                                      // correspondences before this chunk: <= j0
    for (int64_t j0 = 0; j0 < nt; j0 += RT) {
        const int64_t j = j0 + tid;
        const int s = j < nt ? msrc[j] : -1;
        const bool keep = s >= 0 && s < ns;                            // an out-of-range entry is dropped, never an index
        const unsigned long long b = __ballot(keep);
        if (lane == 0) wcnt[wave] = __popcll(b);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < RWV; ++w) {
            before += w < wave ? wcnt[w] : 0;
            total += wcnt[w];
        }
        if (keep) {
            const int rank = base + before + __popcll(b & ((1ull << lane) - 1ull));   // <= j < nt
            const float *x = kp + (size_t)3 * (r0s + s), *y = kp + (size_t)3 * (r0t + j);
            float *o = out + (size_t)6 * rank;
            o[0] = x[0]; o[1] = x[1]; o[2] = x[2];
            o[3] = y[0]; o[4] = y[1]; o[5] = y[2];
        }
        base += total;
        __syncthreads();                                               // wcnt is rewritten by the next chunk
    }
    if (tid == 0) count[p] = base;
}

__device__ __forceinline__ void load_corr(const float *__restrict__ c, double x[3], double y[3]) {
    x[0] = (double)c[0]; x[1] = (double)c[1]; x[2] = (double)c[2];
    y[0] = (double)c[3]; y[1] = (double)c[4]; y[2] = (double)c[5];
}

// Hypothesis h of the pair with counter word `pair`: the draw and the three-point fit.  false: rejected (R, t then unset).
__device__ __forceinline__ bool draw_and_fit(const float *__restrict__ cp, int M, unsigned long long h, unsigned long long pair,
                                             unsigned long long seed, double min_margin, double R[9], double t[3]) {
    if (M < 3) return false;
    const epn::philox::u32x4 w = epn::philox::philox4x32_10(h, pair, seed);
    const unsigned i0 = w.w[0] % (unsigned)M, i1 = w.w[1] % (unsigned)M, i2 = w.w[2] % (unsigned)M;   // bias about M / 2^32
    if (i0 == i1 || i0 == i2 || i1 == i2) return false;
    double x[9], y[9], margin;
    load_corr(cp + (size_t)6 * i0, x, y);
    load_corr(cp + (size_t)6 * i1, x + 3, y + 3);
    load_corr(cp + (size_t)6 * i2, x + 6, y + 6);
    epn_fit::rigid_fit(x, y, 3, R, t, margin);
    return !(margin < min_margin);
}

__global__ __launch_bounds__(RT) void ransac_score_kernel(const float *__restrict__ corr, const int32_t *__restrict__ count,
                                                          const int64_t *__restrict__ tgt_off, int H, unsigned long long pair0,
                                                          unsigned long long seed, double min_margin, double tau2,
                                                          int32_t *__restrict__ hyp_count) {
    __shared__ __attribute__((aligned(16))) float tile[TILE * 6];
    const int tid = threadIdx.x;
    const int p = blockIdx.y, h = (int)blockIdx.x * RT + tid;
    const int M = count[p];
    const float *cp = corr + (size_t)6 * tgt_off[p];
    double R[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, t[3] = {0.0, 0.0, 0.0};
    const bool ok = h < H && draw_and_fit(cp, M, (unsigned long long)h, pair0 + (unsigned long long)p, seed, min_margin, R, t);
    int cnt = 0;
    for (int64_t m0 = 0; M >= 3 && m0 < M; m0 += TILE) {               // M is the same for the whole workgroup
        const int n = M - m0 < TILE ? (int)(M - m0) : TILE;
        const float *src = cp + (size_t)6 * m0;                        // n consecutive correspondences: one contiguous block
        for (int e = tid; e < 6 * n; e += RT) tile[e] = src[e];
        __syncthreads();
        for (int m = 0; m < n; ++m) {
            double x[3], y[3];
            load_corr(tile + 6 * m, x, y);                             // the same address in every lane
            cnt += epn_fit::sq_residual(R, t, x, y) < tau2 ? 1 : 0;
        }
        __syncthreads();
    }
    if (h < H) hyp_count[(size_t)p * H + h] = ok ? cnt : -1;
}

// an order of its own (not epn_block_sum's tree): the wave butterfly, then the four wave sums paired as written
__device__ __forceinline__ double block_sum(double v, double *red) {
    v = epn_wave_sum(v);
    __syncthreads();                                                   // the previous sum has been read
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(RT) void ransac_finish_kernel(const float *__restrict__ corr, const int32_t *__restrict__ count,
                                                           const int64_t *__restrict__ tgt_off,
                                                           const int32_t *__restrict__ hyp_count, int H, unsigned long long pair0,
                                                           unsigned long long seed, double min_margin, double tau2,
                                                           double *__restrict__ T, int32_t *__restrict__ best_h,
                                                           int32_t *__restrict__ n_inlier, double *__restrict__ rmse,
                                                           double *__restrict__ margin) {
    static_assert(RWV == 4, "block_sum and the arg-max below combine four waves");
    __shared__ double red[RWV];
    __shared__ long long kred[RWV];
    const int tid = threadIdx.x;
    const int p = blockIdx.x;
    const int M = count[p];
    const float *cp = corr + (size_t)6 * tgt_off[p];

    // arg-max: the largest count, the lowest h among equals
    long long key = -1;
    for (int h = tid; h < H; h += RT) {
        const long long k = ((long long)(hyp_count[(size_t)p * H + h] + 1) << 32) | (long long)(0xFFFFFFFFu - (unsigned)h);
        key = k > key ? k : key;
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const long long o = __shfl_xor(key, s, 64);
        key = o > key ? o : key;
    }
    if ((tid & 63) == 0) kred[tid >> 6] = key;
    __syncthreads();
    key = kred[0];
#pragma unroll
    for (int w = 1; w < RWV; ++w) key = kred[w] > key ? kred[w] : key;
    const int bcount = (int)(key >> 32) - 1;
    const int bh = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFll));

    double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0}, mg = 0.0, err = INFINITY;
    int hbest = -1, ninl = 0;
    if (bcount >= 3) {                                                 // the same value in every thread
        double R0[9], t0[3];
        draw_and_fit(cp, M, (unsigned long long)bh, pair0 + (unsigned long long)p, seed, min_margin, R0, t0);
        // centroids of the winner's inlier set
        double s[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int64_t m = tid; m < M; m += RT) {
            double x[3], y[3];
            load_corr(cp + (size_t)6 * m, x, y);
            if (epn_fit::sq_residual(R0, t0, x, y) < tau2) {
                s[0] += x[0]; s[1] += x[1]; s[2] += x[2];
                s[3] += y[0]; s[4] += y[1]; s[5] += y[2];
                s[6] += 1.0;
            }
        }
#pragma unroll
        for (int e = 0; e < 7; ++e) s[e] = block_sum(s[e], red);
        if (s[6] >= 1.0) {                                             // count[best_h] >= 3 says so; kept for defined outputs
            const double xbar[3] = {s[0] / s[6], s[1] / s[6], s[2] / s[6]}, ybar[3] = {s[3] / s[6], s[4] / s[6], s[5] / s[6]};
            double C[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            for (int64_t m = tid; m < M; m += RT) {
                double x[3], y[3];
                load_corr(cp + (size_t)6 * m, x, y);
                if (epn_fit::sq_residual(R0, t0, x, y) < tau2) epn_fit::cov_add(C, x, xbar, y, ybar);
            }
#pragma unroll
            for (int e = 0; e < 9; ++e) C[e] = block_sum(C[e], red);
            epn_fit::fit_finish(xbar, ybar, C, R, t, mg);
            // the inliers of the refit and their residuals
            double n = 0.0, sq = 0.0;
            for (int64_t m = tid; m < M; m += RT) {
                double x[3], y[3];
                load_corr(cp + (size_t)6 * m, x, y);
                const double d2 = epn_fit::sq_residual(R, t, x, y);
                if (d2 < tau2) {
                    n += 1.0;
                    sq += d2;
                }
            }
            n = block_sum(n, red);
            sq = block_sum(sq, red);
            hbest = bh;
            ninl = (int)n;
            err = n >= 1.0 ? sqrt(sq / n) : INFINITY;
        }
    }
    if (tid == 0) {
        double *o = T + (size_t)16 * p;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            o[4 * i] = R[3 * i]; o[4 * i + 1] = R[3 * i + 1]; o[4 * i + 2] = R[3 * i + 2]; o[4 * i + 3] = t[i];
        }
        o[12] = 0.0; o[13] = 0.0; o[14] = 0.0; o[15] = 1.0;
        best_h[p] = hbest;
        n_inlier[p] = ninl;
        rmse[p] = err;
        margin[p] = mg;
    }
}

}  // namespace

extern "C" size_t epn_ransac_register_workspace_bytes(int64_t tgt_rows) {
    return tgt_rows >= 0 ? corr_bytes(tgt_rows) + (size_t)(epn::SCENE_MAX_PAIRS + 1) * sizeof(int32_t) : 0;
}

extern "C" int epn_ransac_register_f64(const float *kp_xyz, int64_t R, int F, const int64_t *frag_off_host, const int64_t *frag_off,
                                       int P, const int32_t *pairs_host, const int32_t *pairs, const int64_t *tgt_off_host,
                                       const int64_t *tgt_off, const int32_t *match_src, double tau, int H, uint64_t seed,
                                       int64_t pair0, double min_margin, void *workspace, size_t workspace_bytes, double *T,
                                       int32_t *best_h, int32_t *hyp_count, int32_t *n_inlier, double *rmse, double *margin,
                                       epn_stream_t stream) {
    // every argument is checked before the first HIP runtime call
    if (H < 1 || H > MAX_HYP || !std::isfinite(tau) || !(tau > 0.0) || !(min_margin >= 0.0 && min_margin < 1.0) || pair0 < 0)
        return EPN_EINVAL;
    if (!tgt_off_host) return EPN_ENULL;
    int64_t max_rows = 0;
    const int rc = epn::check_scene(R, F, frag_off_host, P, pairs_host, nullptr, tgt_off_host, &max_rows, false);
    if (rc != 0) return rc;
    if (P == 0) return 0;
    if (!frag_off || !pairs || !tgt_off || !T || !best_h || !hyp_count || !n_inlier || !rmse || !margin) return EPN_ENULL;
    const int64_t tgt_rows = tgt_off_host[P];
    if (tgt_rows > 0 && (!kp_xyz || !match_src)) return EPN_ENULL;
    if (!workspace || workspace_bytes < epn_ransac_register_workspace_bytes(tgt_rows)) return EPN_EWORKSPACE;
    hipStream_t st = epn_stream(stream);
    float *corr = static_cast<float *>(workspace);
    int32_t *count = reinterpret_cast<int32_t *>(static_cast<char *>(workspace) + corr_bytes(tgt_rows));
    const unsigned long long ctr = (unsigned long long)pair0, sd = (unsigned long long)seed;
    const double tau2 = tau * tau;
    EPN_LAUNCH_AUX(ransac_compact_kernel, dim3((unsigned)P), dim3(RT), 0, st, kp_xyz, frag_off, pairs, tgt_off, match_src, corr, count);
    EPN_CHECK_LAUNCH();
    EPN_LAUNCH(ransac_score_kernel, dim3((unsigned)epn_cdiv(H, RT), (unsigned)P), dim3(RT), 0, st, corr, count, tgt_off, H, ctr, sd,
               min_margin, tau2, hyp_count);
    EPN_CHECK_LAUNCH();
    EPN_LAUNCH_AUX(ransac_finish_kernel, dim3((unsigned)P), dim3(RT), 0, st, corr, count, tgt_off, hyp_count, H, ctr, sd, min_margin,
                   tau2, T, best_h, n_inlier, rmse, margin);
    EPN_CHECK_LAUNCH();
    return 0;
}
