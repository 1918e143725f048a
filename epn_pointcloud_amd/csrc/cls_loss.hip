// The classification network's training loss and evaluation tallies for gfx950: CrossEntropyLoss and AttentionCrossEntropyLoss
// (vgtk/vgtk/loss.py:18-75) and the counting of SPConvNets/trainer_modelnet.py:138-210.  Specification: include/epn_so3conv.h
// (epn_cls_loss_f32, epn_cls_loss_bwd_f32, epn_cls_tally_i32), DESIGN.md 3.1g.
//
// The class term and the attention term are one problem twice: rows of n contiguous fp32 logits with one int32 label each.  A
// launch takes a descriptor of the two row sets (the second may be empty) and serves both.
//   rows    one wave per row, four rows per 256-thread workgroup; lane l reads elements l, l + 64, ...  Two passes over the row:
//           the maximum with its arg max (fp32 comparison, the lowest index on a tie, xor tree over the lanes) and whether every
//           element is finite; then the sum of exp(. - max) in fp64, each lane ascending, then a fixed xor tree on the fp64
//           partials.  A row of at most 4096 floats stays in the cache between the passes.
//   finish  one workgroup: thread i adds rows i, i + 256, ... ascending, then a fixed tree in LDS; reads coef on the device.
//   bwd     the row arithmetic again (the same operations on the same values: the same bits), then every element of the row.
//   tally   one thread per row; integer vector atomics into the caller's tables (integer addition does not depend on the order),
//           the four totals added once per wave.
// fp64 throughout on the fp32 inputs, every output rounded once; no float atomics, no workspace, no host synchronisation, no
// globals; every float sum runs in a fixed order, so two runs are bitwise equal.  A label is compared, or becomes an address
// only after its range was checked on the device; the tally checks the predictions it is handed in the same way.
#include <climits>
#include <cmath>

#include "epn_reduce.h"

namespace {

constexpr int RW = EPN_WAVE;             // lanes of a wave: one row each
constexpr int FT = 256;                  // threads of every workgroup here
constexpr int RPB = FT / RW;             // rows per workgroup

enum { FLAG_BAD_LABEL = 1, FLAG_NONFINITE = 2 };

// one set of rows: x f32[rows][n], label i32[rows]; the per-row outputs of the forward (flags is an input of the backward)
struct RowSet {
    const float *x;
    const int32_t *label;
    float *row_ce;
    int32_t *pred;
    int32_t *flags;
    float *dx;
    int rows, n;
};

// what a launch reads: the class rows, the attention rows, and where the second set's workgroups begin
struct RowSets {
    RowSet set[2];
    int blocks0;
};

// the softmax pieces of one row, the same bits in every lane: the maximum m with its arg max (the lowest index on a tie),
// s = sum_j exp(x_j - m), and whether every element is finite
__device__ __forceinline__ void row_softmax(const float *__restrict__ x, int n, int lane, int &pred, double &m, double &s, bool &finite) {
    float best = -INFINITY;
    int at = INT_MAX;
    bool bad = false;
    for (int j = lane; j < n; j += RW) {
        const float v = x[j];
        bad |= !isfinite(v);
        if (v > best) {
            best = v;
            at = j;
        }
    }
#pragma unroll
    for (int off = RW / 2; off > 0; off >>= 1) {
        const float ov = __shfl_xor(best, off);
        const int oa = __shfl_xor(at, off);
        if (ov > best || (ov == best && oa < at)) {
            best = ov;
            at = oa;
        }
    }
    finite = !__any(bad);
    pred = at;
    m = (double)best;
    double part = 0.0;
    if (finite)
        for (int j = lane; j < n; j += RW) part += exp((double)x[j] - m);
#pragma unroll
    for (int off = RW / 2; off > 0; off >>= 1) part += __shfl_xor(part, off);
    s = part;
}

__global__ __launch_bounds__(FT) void cls_loss_rows_kernel(const RowSets d) {
    const int which = (int)blockIdx.x >= d.blocks0;
    const RowSet &rs = d.set[which];
    const int lane = threadIdx.x & (RW - 1);
    const int row = ((int)blockIdx.x - (which ? d.blocks0 : 0)) * RPB + (int)(threadIdx.x / RW);
    if (row >= rs.rows) return;
    const float *x = rs.x + (size_t)row * rs.n;
    int pred;
    double m, s;
    bool finite;
    row_softmax(x, rs.n, lane, pred, m, s, finite);
    if (lane != 0) return;
    const int L = rs.label[row];
    const bool in_range = L >= 0 && L < rs.n;
    float ce = 0.0f;
    if (in_range) ce = finite ? (float)((m - (double)x[L]) + log(s)) : NAN;
    rs.row_ce[row] = ce;
    rs.pred[row] = finite ? pred : -1;
    rs.flags[row] = (in_range ? 0 : FLAG_BAD_LABEL) | (finite ? 0 : FLAG_NONFINITE);
}

__global__ __launch_bounds__(FT) void cls_loss_finish_kernel(const RowSets d, const float *__restrict__ coef,
                                                             float *__restrict__ scalars) {
    __shared__ double buf[FT];
    double mean[2] = {0.0, 0.0}, acc[2] = {0.0, 0.0};
    for (int w = 0; w < 2; ++w) {
        const RowSet &rs = d.set[w];
        if (rs.rows == 0) continue;
        double sc = 0.0, hit = 0.0;
        for (int i = threadIdx.x; i < rs.rows; i += FT) {
            sc += (double)rs.row_ce[i];
            const int p = rs.pred[i];
            hit += (p >= 0 && p == rs.label[i]) ? 1.0 : 0.0;
        }
        mean[w] = epn_block_sum<FT>(sc, buf) / (double)rs.rows;
        acc[w] = epn_block_sum<FT>(hit, buf) / (double)rs.rows;
    }
    if (threadIdx.x == 0) {
        double loss = (double)coef[0] * mean[0];
        if (d.set[1].rows > 0) loss += (double)coef[1] * mean[1];
        scalars[0] = (float)loss;
        scalars[1] = (float)mean[0];
        scalars[2] = (float)mean[1];
        scalars[3] = (float)acc[0];
        scalars[4] = (float)acc[1];
    }
}

__global__ __launch_bounds__(FT) void cls_loss_bwd_kernel(const RowSets d, const float *__restrict__ upstream,
                                                          const float *__restrict__ coef) {
    const int which = (int)blockIdx.x >= d.blocks0;
    const RowSet &rs = d.set[which];
    const int lane = threadIdx.x & (RW - 1);
    const int row = ((int)blockIdx.x - (which ? d.blocks0 : 0)) * RPB + (int)(threadIdx.x / RW);
    if (row >= rs.rows) return;
    const int n = rs.n;
    const float *x = rs.x + (size_t)row * n;
    float *dx = rs.dx + (size_t)row * n;
    const int L = rs.label[row], fl = rs.flags[row];
    if ((fl & FLAG_BAD_LABEL) || L < 0 || L >= n) {
        for (int j = lane; j < n; j += RW) dx[j] = 0.0f;
        return;
    }
    int pred;
    double m, s;
    bool finite;
    row_softmax(x, n, lane, pred, m, s, finite);
    if ((fl & FLAG_NONFINITE) || !finite) {
        for (int j = lane; j < n; j += RW) dx[j] = NAN;
        return;
    }
    const double c = (double)upstream[0] * (double)coef[which] / (double)rs.rows;
    for (int j = lane; j < n; j += RW) dx[j] = (float)(c * (exp((double)x[j] - m) / s - (j == L ? 1.0 : 0.0)));
}

__global__ __launch_bounds__(FT) void cls_tally_kernel(const int32_t *__restrict__ pred, const int32_t *__restrict__ label,
                                                       const int32_t *__restrict__ flags, const int32_t *__restrict__ att_pred,
                                                       const int32_t *__restrict__ att_label, const int32_t *__restrict__ att_flags,
                                                       int B, int k, int A, int32_t *__restrict__ confusion,
                                                       int32_t *__restrict__ anchor_table, int32_t *__restrict__ totals) {
    const int i = (int)(blockIdx.x * FT + threadIdx.x);
    bool seen = false, skipped = false, hit = false, att_hit = false;
    if (i < B) {
        const int L = label[i], P = pred[i];
        int fl = flags[i] | (L < 0 || L >= k || P < 0 || P >= k ? FLAG_BAD_LABEL : 0);
        int AP = -1;
        if (att_pred) {
            AP = att_pred[i];
            fl |= att_flags[i] | (AP < 0 || AP >= A ? FLAG_BAD_LABEL : 0);
        }
        skipped = fl != 0;
        seen = !skipped;
        if (seen) {
            hit = P == L;
            atomicAdd(&confusion[(size_t)L * k + P], 1);
            if (att_pred) {
                atomicAdd(&anchor_table[(size_t)L * A + AP], 1);
                att_hit = att_label && AP == att_label[i];
            }
        }
    }
    const int n_seen = __popcll(__ballot(seen)), n_hit = __popcll(__ballot(hit));
    const int n_att = __popcll(__ballot(att_hit)), n_skip = __popcll(__ballot(skipped));
    if ((threadIdx.x & (RW - 1)) == 0) {
        if (n_seen) atomicAdd(&totals[0], n_seen);
        if (n_hit) atomicAdd(&totals[1], n_hit);
        if (n_att) atomicAdd(&totals[2], n_att);
        if (n_skip) atomicAdd(&totals[3], n_skip);
    }
}

RowSets row_sets(const float *logits, const int32_t *label, int B, int k, const float *att, const int32_t *att_label, int R, int A,
                 float *row_ce, int32_t *pred, int32_t *flags, float *dlogits, float *att_row_ce, int32_t *att_pred,
                 int32_t *att_flags, float *datt) {
    RowSets d;
    d.set[0] = RowSet{logits, label, row_ce, pred, flags, dlogits, B, k};
    d.set[1] = RowSet{att, att_label, att_row_ce, att_pred, att_flags, datt, R, R > 0 ? A : 0};
    d.blocks0 = epn_cdiv(B, RPB);
    return d;
}

bool cls_rows_ok(int rows, int n) { return rows >= 1 && rows <= 65536 && n >= 1 && n <= 4096 && (long long)rows * n < (1LL << 31); }

}  // namespace

// Every argument is checked before the first HIP runtime call.  Sizes first (EPN_EINVAL), then pointers (EPN_ENULL); the
// attention set is absent as a whole (R == 0: its pointers are not looked at)
extern "C" int epn_cls_loss_f32(const float *logits, const int32_t *label, int B, int k, const float *att,
                                const int32_t *att_label, int R, int A, const float *coef, float *row_ce, int32_t *pred,
                                int32_t *flags, float *att_row_ce, int32_t *att_pred, int32_t *att_flags, float *scalars,
                                epn_stream_t stream) {
    if (!cls_rows_ok(B, k) || (R != 0 && !cls_rows_ok(R, A))) return EPN_EINVAL;
    if (!logits || !label || !coef || !row_ce || !pred || !flags || !scalars) return EPN_ENULL;
    if (R != 0 && (!att || !att_label || !att_row_ce || !att_pred || !att_flags)) return EPN_ENULL;
    hipStream_t st = epn_stream(stream);
    const RowSets d = row_sets(logits, label, B, k, att, att_label, R, A, row_ce, pred, flags, nullptr, att_row_ce, att_pred,
                               att_flags, nullptr);
    const dim3 grid((unsigned)(d.blocks0 + epn_cdiv(R, RPB))), block(FT);
    EPN_LAUNCH(cls_loss_rows_kernel, grid, block, 0, st, d);
    EPN_CHECK_LAUNCH();
    EPN_LAUNCH_AUX(cls_loss_finish_kernel, dim3(1), block, 0, st, d, coef, scalars);
    EPN_CHECK_LAUNCH();
    return 0;
}

extern "C" int epn_cls_loss_bwd_f32(const float *upstream, const float *logits, const int32_t *label, const int32_t *flags, int B,
                                    int k, const float *att, const int32_t *att_label, const int32_t *att_flags, int R, int A,
                                    const float *coef, float *dlogits, float *datt, epn_stream_t stream) {
    if (!cls_rows_ok(B, k) || (R != 0 && !cls_rows_ok(R, A))) return EPN_EINVAL;
    if (!upstream || !logits || !label || !flags || !coef || !dlogits) return EPN_ENULL;
    if (R != 0 && (!att || !att_label || !att_flags || !datt)) return EPN_ENULL;
    const RowSets d = row_sets(logits, label, B, k, att, att_label, R, A, nullptr, nullptr, const_cast<int32_t *>(flags), dlogits,
                               nullptr, nullptr, const_cast<int32_t *>(att_flags), datt);
    const dim3 grid((unsigned)(d.blocks0 + epn_cdiv(R, RPB))), block(FT);
    EPN_LAUNCH(cls_loss_bwd_kernel, grid, block, 0, epn_stream(stream), d, upstream, coef);
    EPN_CHECK_LAUNCH();
    return 0;
}

extern "C" int epn_cls_tally_i32(const int32_t *pred, const int32_t *label, const int32_t *flags, const int32_t *att_pred,
                                 const int32_t *att_label, const int32_t *att_flags, int B, int k, int A, int32_t *confusion,
                                 int32_t *anchor_table, int32_t *totals, epn_stream_t stream) {
    if (B < 1 || B > 65536 || k < 1 || k > 4096) return EPN_EINVAL;
    if (att_pred && (A < 1 || A > 4096)) return EPN_EINVAL;
    if (!pred || !label || !flags || !confusion || !totals) return EPN_ENULL;
    if (att_pred && (!att_flags || !anchor_table)) return EPN_ENULL;
    EPN_LAUNCH(cls_tally_kernel, dim3((unsigned)epn_cdiv(B, FT)), dim3(FT), 0, epn_stream(stream), pred, label, flags, att_pred,
               att_pred ? att_label : nullptr, att_flags, B, k, A, confusion, anchor_table, totals);
    EPN_CHECK_LAUNCH();
    return 0;
}
