// The descriptor network's training loss for gfx950: batch-hard triplet mining over the N x N distances of two descriptor sets
// (TripletBatchLoss._forward_invariance with pairwise_distance_matrix and batch_hard_negative_mining, vgtk/vgtk/loss.py:220-235
// and :280-318) and the anchor interpolation of its equivariance term (_interpolate / _rotation_distance, loss.py:400-445, with
// the per-sample gather the commented-out line :427 intends).  Specification: include/epn_so3conv.h
// (epn_triplet_batch_hard_f32, epn_triplet_batch_hard_bwd_f32, epn_anchor_interp_f32, epn_anchor_interp_bwd_f32), DESIGN.md 3.1d.
//
// fp64 throughout on the fp32 inputs, every output rounded once; no atomics, no workspace, no host synchronisation; every sum
// runs in a fixed order, so two runs are bitwise equal.  The N x N matrix is never written.
//   rows     256 threads = 4 waves, wave w of workgroup g owns source row i = 4 g + w.  The tgt rows go through LDS in tiles
//            of 64 rows x 64 columns (row stride 65 floats: lane l reads bank (65 l + c) % 32, no conflict); lane l of every
//            wave owns tgt row j = 64 t + l of tile t and adds its (s - t)^2 terms in ascending column order.  Tiles ascend, so
//            a strict < keeps the lowest j per lane; the xor tree across lanes takes the smaller distance, the lower j on a tie.
//   finish   one workgroup: thread t adds rows t, t + 256, ... ascending, then a fixed tree in LDS.
//   bwd      workgroup j writes dsrc[j,:] and dtgt[j,:].  The rows i with neg_idx[i] == j are found by ballots over neg_idx
//            (one 64-bit mask per 64 rows, kept in LDS), ranked by the set bits in front of them and written with their
//            coefficients, once, into a list in LDS that every column then walks in ascending i: a gather, nothing is
//            scattered.  The list holds 1024 rows; more than that sharing one hardest negative are taken in rounds.
//   interp   workgroup b: thread n < A ranks the A traces of anchor n (three strict > insertions over ascending m: lowest m on a
//            tie), writes idx and w and leaves them in LDS; then all threads blend the [C, A] features.
//   interp bwd  workgroup b: thread (c, m) scans the 3 A saved entries in index order.
// Limits: 2 <= N <= 65536 (the LDS masks of the backward: N / 64 words; every grid is N or N / 4 workgroups), D >= 1 with
// N * D < 2^31, A in {12, 60}, nb * C * A < 2^31.  Every index read back from memory (neg_idx in the backward, idx in the
// interpolation backward) is range-checked on the device before it is used as an address.
#include <cmath>

#include "epn_reduce.h"

namespace {

constexpr int TT = 256;                  // threads per workgroup
constexpr int TW = TT / 64;              // waves per workgroup = source rows per workgroup
constexpr int TJ = 64;                   // tgt rows per tile = lanes
constexpr int TD = 64;                   // columns per tile
constexpr int MAXN = 65536;
constexpr int MAXA = 60;
constexpr int HITS = 1024;                // rows per round of the backward's hit list

enum { FLAG_POS_CLAMPED = 1, FLAG_NEG_CLAMPED = 2, FLAG_HINGE_ACTIVE = 4 };

// (distance, index) minimum of two lanes: the smaller distance, the lower index on a tie; the same bits in both lanes
__device__ __forceinline__ void wave_argmin(double &d, int &j) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const double od = __shfl_xor(d, s, 64);
        const int oj = __shfl_xor(j, s, 64);
        if (od < d || (od == d && oj < j)) {
            d = od;
            j = oj;
        }
    }
}

__global__ __launch_bounds__(TT) void triplet_rows_kernel(const float *__restrict__ src, const float *__restrict__ tgt, int N, int D,
                                                          int mode, double margin, double eps, float *__restrict__ d_pos,
                                                          float *__restrict__ d_neg, float *__restrict__ row_loss,
                                                          int32_t *__restrict__ neg_idx, int32_t *__restrict__ nn_idx,
                                                          int32_t *__restrict__ row_flags) {
    __shared__ float tile[TJ * (TD + 1)];
    __shared__ float rows[TW * TD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x * TW + wave;                   // may be >= N in the last workgroup: computes, writes nothing
    const int is = i < N ? i : N - 1;
    double best_neg = INFINITY, best_all = INFINITY, dpos = 0.0;
    int jn = is == 0 ? 1 : 0, ja = 0;                       // in range whatever the data (NaN rows never win a <)
    bool pos_clamped = false, neg_clamped = false;
    for (int j0 = 0; j0 < N; j0 += TJ) {
        const int j = j0 + lane;
        double d2 = 0.0;
        for (int c0 = 0; c0 < D; c0 += TD) {
            const int nc = D - c0 < TD ? D - c0 : TD;
            __syncthreads();
            for (int e = tid; e < TJ * TD; e += TT) {
                const int r = e / TD, c = e % TD;
                tile[r * (TD + 1) + c] = (j0 + r < N && c < nc) ? tgt[(size_t)(j0 + r) * D + c0 + c] : 0.0f;
            }
            {
                const int r = tid / TD, c = tid % TD;       // TW * TD == TT
                const int ir = blockIdx.x * TW + r;
                rows[tid] = (ir < N && c < nc) ? src[(size_t)ir * D + c0 + c] : 0.0f;
            }
            __syncthreads();
            const float *tr = tile + lane * (TD + 1), *sr = rows + wave * TD;
            for (int c = 0; c < nc; ++c) {
                const double diff = (double)sr[c] - (double)tr[c];
                d2 = fma(diff, diff, d2);
            }
        }
        if (j < N) {
            const bool clamped = d2 < eps;
            const double dist = sqrt(clamped ? eps : d2);   // torch.clamp(min = eps) passes a NaN on; so does this
            if (j == is) {
                dpos = dist;
                pos_clamped = clamped;
            } else if (dist < best_neg) {
                best_neg = dist;
                jn = j;
                neg_clamped = clamped;
            }
            if (dist < best_all) {
                best_all = dist;
                ja = j;
            }
        }
    }
    dpos = __shfl(dpos, is & 63, 64);
    const unsigned long long pc = __ballot(pos_clamped && lane == (is & 63));
    wave_argmin(best_all, ja);
    const int my_jn = jn;
    wave_argmin(best_neg, jn);
    const unsigned long long ncl = __ballot(neg_clamped && my_jn == jn);
    if (lane != 0 || i >= N) return;
    const double x = dpos - best_neg;
    double loss;
    bool active = true;
    if (mode == EPN_TRIPLET_HARD) {
        active = x + margin > 0.0;
        loss = active ? x + margin : 0.0;
    } else if (mode == EPN_TRIPLET_SOFT) {
        loss = margin * x > 20.0 ? x : log1p(exp(margin * x)) / margin;
    } else {
        active = margin - best_neg > 0.0;
        loss = dpos + (active ? margin - best_neg : 0.0);
    }
    d_pos[i] = (float)dpos;
    d_neg[i] = (float)best_neg;
    row_loss[i] = (float)loss;
    neg_idx[i] = jn;
    nn_idx[i] = ja;
    row_flags[i] = (pc ? FLAG_POS_CLAMPED : 0) | (ncl ? FLAG_NEG_CLAMPED : 0) | (active ? FLAG_HINGE_ACTIVE : 0);
}

__global__ __launch_bounds__(TT) void triplet_finish_kernel(const float *__restrict__ d_pos, const float *__restrict__ d_neg,
                                                            const float *__restrict__ row_loss, const int32_t *__restrict__ nn_idx,
                                                            int N, float *__restrict__ scalars) {
    __shared__ double buf[TT];
    double sl = 0.0, sp = 0.0, sn = 0.0, hit = 0.0;
    for (int i = threadIdx.x; i < N; i += TT) {
        sl += (double)row_loss[i];
        sp += (double)d_pos[i];
        sn += (double)d_neg[i];
        hit += nn_idx[i] == i ? 1.0 : 0.0;
    }
    sl = epn_block_sum<TT>(sl, buf);
    sp = epn_block_sum<TT>(sp, buf);
    sn = epn_block_sum<TT>(sn, buf);
    hit = epn_block_sum<TT>(hit, buf);
    if (threadIdx.x == 0) {
        scalars[0] = (float)(sl / N);
        scalars[1] = (float)(hit / N);
        scalars[2] = (float)(sp / N);
        scalars[3] = (float)(sn / N);
    }
}

// d row_loss / d d_pos and - d row_loss / d d_neg of row i, each already divided by its distance and multiplied by upstream / N;
// zero for a clamped distance and for an inactive hinge
__device__ __forceinline__ void row_coefficients(int i, int mode, double margin, double scale, const float *__restrict__ d_pos,
                                                 const float *__restrict__ d_neg, const int32_t *__restrict__ row_flags, double &cp,
                                                 double &cn) {
    const int f = row_flags[i];
    const double dp = (double)d_pos[i], dn = (double)d_neg[i];
    double gp, gn;
    if (mode == EPN_TRIPLET_HARD) {
        gp = gn = (f & FLAG_HINGE_ACTIVE) ? 1.0 : 0.0;
    } else if (mode == EPN_TRIPLET_SOFT) {
        const double bx = margin * (dp - dn);
        gp = gn = bx > 20.0 ? 1.0 : 1.0 / (1.0 + exp(-bx));
    } else {
        gp = 1.0;
        gn = (f & FLAG_HINGE_ACTIVE) ? 1.0 : 0.0;
    }
    cp = (f & FLAG_POS_CLAMPED) ? 0.0 : scale * gp / dp;
    cn = (f & FLAG_NEG_CLAMPED) ? 0.0 : scale * gn / dn;
}

__global__ __launch_bounds__(TT) void triplet_bwd_kernel(const float *__restrict__ upstream, const float *__restrict__ src,
                                                         const float *__restrict__ tgt, const float *__restrict__ d_pos,
                                                         const float *__restrict__ d_neg, const int32_t *__restrict__ neg_idx,
                                                         const int32_t *__restrict__ row_flags, int N, int D, int mode, double margin,
                                                         float *__restrict__ dsrc, float *__restrict__ dtgt) {
    __shared__ unsigned long long mask[MAXN / 64];          // bit b of word g: neg_idx[64 g + b] == j
    __shared__ int before[MAXN / 64 + 1];                   // set bits in front of word g; [groups] = all of them
    __shared__ int hit_row[HITS];                           // one round of the rows found, ascending, and their coefficients
    __shared__ double hit_cn[HITS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = blockIdx.x;
    const int groups = (N + 63) / 64;
    for (int g = wave; g < groups; g += TW) {
        const int i = g * 64 + lane;
        const unsigned long long m = __ballot(i < N && neg_idx[i] == j);
        if (lane == 0) mask[g] = m;
    }
    __syncthreads();
    if (tid == 0) {
        int n = 0;
        for (int g = 0; g < groups; ++g) {
            before[g] = n;
            n += __popcll(mask[g]);
        }
        before[groups] = n;
    }
    __syncthreads();
    const int hits = before[groups];
    const int rounds = (hits + HITS - 1) / HITS;            // 1 unless more than HITS rows share this hardest negative
    const double scale = (double)upstream[0] / N;
    double cp, cn;
    row_coefficients(j, mode, margin, scale, d_pos, d_neg, row_flags, cp, cn);
    int jn = neg_idx[j];
    if (jn < 0 || jn >= N) {                                // never an address: a row that is not the forward's contributes zero
        jn = j;
        cn = 0.0;
    }
    const float *sj = src + (size_t)j * D, *tj = tgt + (size_t)j * D, *tn = tgt + (size_t)jn * D;
    for (int d0 = 0; d0 < D; d0 += TT) {                    // the same trip count in every thread: there are barriers inside
        const int d = d0 + tid;
        const bool live = d < D;
        double t = 0.0, acc = 0.0;
        if (live) {
            const double s = (double)sj[d];
            t = (double)tj[d];
            const double pos = cp * (s - t);
            dsrc[(size_t)j * D + d] = (float)(pos - cn * (s - (double)tn[d]));
            acc = -pos;
        }
        for (int r = 0; r < rounds; ++r) {
            if (rounds > 1 || d0 == 0) {                    // one round: the list is built once and serves every d0
                __syncthreads();
                for (int i = tid; i < N; i += TT) {
                    const unsigned long long m = mask[i >> 6], bit = 1ull << (i & 63);
                    if (!(m & bit)) continue;
                    const int k = before[i >> 6] + __popcll(m & (bit - 1)) - r * HITS;      // rank in ascending i
                    if (k < 0 || k >= HITS) continue;
                    double cpi, cni;
                    row_coefficients(i, mode, margin, scale, d_pos, d_neg, row_flags, cpi, cni);
                    hit_row[k] = i;
                    hit_cn[k] = cni;
                }
                __syncthreads();
            }
            const int cnt = hits - r * HITS < HITS ? hits - r * HITS : HITS;
            if (live)
                for (int k = 0; k < cnt; ++k) acc += hit_cn[k] * ((double)src[(size_t)hit_row[k] * D + d] - t);
        }
        if (live) dtgt[(size_t)j * D + d] = (float)acc;
    }
}

__global__ __launch_bounds__(TT) void anchor_interp_kernel(const float *__restrict__ feature, const float *__restrict__ T,
                                                           const float *__restrict__ anchors, int C, int A, double sigma,
                                                           float *__restrict__ out, int32_t *__restrict__ idx, float *__restrict__ w) {
    __shared__ float an[MAXA * 9];
    __shared__ int sidx[MAXA * 3];
    __shared__ double sw[MAXA * 3];
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    for (int e = tid; e < A * 9; e += TT) an[e] = anchors[e];
    __syncthreads();
    if (tid < A) {
        const int n = tid;
        double R[9], P[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) R[e] = (double)T[9 * b + e];
#pragma unroll
        for (int r = 0; r < 3; ++r)                                    // P = R^T A_n; tr(R^T A_n A_m^T) = <P, A_m>
#pragma unroll
            for (int c = 0; c < 3; ++c)
                P[3 * r + c] = R[r] * (double)an[9 * n + c] + R[3 + r] * (double)an[9 * n + 3 + c] + R[6 + r] * (double)an[9 * n + 6 + c];
        double v0 = -INFINITY, v1 = -INFINITY, v2 = -INFINITY;
        int m0 = 0, m1 = 1, m2 = 2;                                    // in range whatever the data
        for (int m = 0; m < A; ++m) {
            double tr = 0.0;
#pragma unroll
            for (int e = 0; e < 9; ++e) tr += P[e] * (double)an[9 * m + e];
            if (tr > v0) {
                v2 = v1, m2 = m1;
                v1 = v0, m1 = m0;
                v0 = tr, m0 = m;
            } else if (tr > v1) {
                v2 = v1, m2 = m1;
                v1 = tr, m1 = m;
            } else if (tr > v2) {
                v2 = tr, m2 = m;
            }
        }
        const double e1 = exp((v1 - v0) / sigma), e2 = exp((v2 - v0) / sigma);   // softmax with the maximum taken out
        const double den = 1.0 + e1 + e2;
        const double ws[3] = {1.0 / den, e1 / den, e2 / den};
        const int ms[3] = {m0, m1, m2};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            sidx[3 * n + k] = ms[k];
            sw[3 * n + k] = ws[k];
            idx[(b * A + n) * 3 + k] = ms[k];
            w[(b * A + n) * 3 + k] = (float)ws[k];
        }
    }
    __syncthreads();
    const float *f = feature + b * C * A;
    for (int e = tid; e < C * A; e += TT) {
        const int c = e / A, n = e % A;
        const float *fc = f + (size_t)c * A;
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) acc += sw[3 * n + k] * (double)fc[sidx[3 * n + k]];
        out[b * C * A + e] = (float)acc;
    }
}

__global__ __launch_bounds__(TT) void anchor_interp_bwd_kernel(const float *__restrict__ dout, const int32_t *__restrict__ idx,
                                                               const float *__restrict__ w, int C, int A, float *__restrict__ dfeature) {
    __shared__ int sidx[MAXA * 3];
    __shared__ float sw[MAXA * 3];
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    for (int e = tid; e < 3 * A; e += TT) {
        sidx[e] = idx[b * 3 * A + e];                                  // only compared with m below, never an address
        sw[e] = w[b * 3 * A + e];
    }
    __syncthreads();
    const float *g = dout + b * C * A;
    for (int e = tid; e < C * A; e += TT) {
        const int c = e / A, m = e % A;
        const float *gc = g + (size_t)c * A;
        double acc = 0.0;
        for (int n = 0; n < A; ++n)
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if (sidx[3 * n + k] == m) acc += (double)sw[3 * n + k] * (double)gc[n];
        dfeature[b * C * A + e] = (float)acc;
    }
}

bool triplet_shape_ok(int N, int D, int mode) {
    return N >= 2 && N <= MAXN && D >= 1 && (long long)N * D < (1ll << 31) &&
           (mode == EPN_TRIPLET_HARD || mode == EPN_TRIPLET_SOFT || mode == EPN_TRIPLET_CONTRASTIVE);
}

bool interp_shape_ok(int nb, int C, int A, int knn) {
    return nb >= 0 && C >= 1 && (A == 12 || A == 60) && knn == 3 && (long long)nb * C * A < (1ll << 31);
}

}  // namespace

extern "C" int epn_triplet_batch_hard_f32(const float *src, const float *tgt, int N, int D, int mode, double margin, double eps,
                                          float *d_pos, float *d_neg, float *row_loss, int32_t *neg_idx, int32_t *nn_idx,
                                          int32_t *row_flags, float *scalars, epn_stream_t stream) {
    // every argument is checked before the first HIP runtime call
    if (!triplet_shape_ok(N, D, mode) || !(eps > 0.0) || !std::isfinite(margin)) return EPN_EINVAL;
    if (mode == EPN_TRIPLET_SOFT && !(margin > 0.0)) return EPN_EINVAL;
    if (!src || !tgt || !d_pos || !d_neg || !row_loss || !neg_idx || !nn_idx || !row_flags || !scalars) return EPN_ENULL;
    hipStream_t st = epn_stream(stream);
    EPN_LAUNCH(triplet_rows_kernel, dim3((unsigned)epn_cdiv(N, TW)), dim3(TT), 0, st, src, tgt, N, D, mode, margin, eps, d_pos, d_neg,
               row_loss, neg_idx, nn_idx, row_flags);
    EPN_CHECK_LAUNCH();
    EPN_LAUNCH_AUX(triplet_finish_kernel, dim3(1), dim3(TT), 0, st, d_pos, d_neg, row_loss, nn_idx, N, scalars);
    EPN_CHECK_LAUNCH();
    return 0;
}

extern "C" int epn_triplet_batch_hard_bwd_f32(const float *upstream, const float *src, const float *tgt, const float *d_pos,
                                              const float *d_neg, const int32_t *neg_idx, const int32_t *row_flags, int N, int D,
                                              int mode, double margin, float *dsrc, float *dtgt, epn_stream_t stream) {
    if (!triplet_shape_ok(N, D, mode) || !std::isfinite(margin)) return EPN_EINVAL;
    if (!upstream || !src || !tgt || !d_pos || !d_neg || !neg_idx || !row_flags || !dsrc || !dtgt) return EPN_ENULL;
    EPN_LAUNCH(triplet_bwd_kernel, dim3((unsigned)N), dim3(TT), 0, epn_stream(stream), upstream, src, tgt, d_pos, d_neg, neg_idx,
               row_flags, N, D, mode, margin, dsrc, dtgt);
    EPN_CHECK_LAUNCH();
    return 0;
}

extern "C" int epn_anchor_interp_f32(const float *feature, const float *T, const float *anchors, int nb, int C, int A, int knn,
                                     double sigma, float *out, int32_t *idx, float *w, epn_stream_t stream) {
    if (!interp_shape_ok(nb, C, A, knn) || !(sigma > 0.0) || !std::isfinite(sigma)) return EPN_EINVAL;
    if (nb == 0) return 0;
    if (!feature || !T || !anchors || !out || !idx || !w) return EPN_ENULL;
    EPN_LAUNCH(anchor_interp_kernel, dim3((unsigned)nb), dim3(TT), 0, epn_stream(stream), feature, T, anchors, C, A, sigma, out, idx, w);
    EPN_CHECK_LAUNCH();
    return 0;
}

extern "C" int epn_anchor_interp_bwd_f32(const float *dout, const int32_t *idx, const float *w, int nb, int C, int A, int knn,
                                         float *dfeature, epn_stream_t stream) {
    if (!interp_shape_ok(nb, C, A, knn)) return EPN_EINVAL;
    if (nb == 0) return 0;
    if (!dout || !idx || !w || !dfeature) return EPN_ENULL;
    EPN_LAUNCH(anchor_interp_bwd_kernel, dim3((unsigned)nb), dim3(TT), 0, epn_stream(stream), dout, idx, w, C, A, dfeature);
    EPN_CHECK_LAUNCH();
    return 0;
}
