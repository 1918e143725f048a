// Surface normals of a cloud from its point grid, and the normal frame of a patch, for gfx950.  It replaces what the reference
// does on the host with open3d (SPConvNets/datasets/preprocess/run_fusion.py:48, pc.estimate_normals(): a KD-tree and an
// eigen-solve per point) and with numpy per patch (transform_with_normals, SPConvNets/datasets/match_3dmatch.py:141-152).
// Specification: include/epn_so3conv.h (epn_point_normals_f32, epn_orient_patches_f32) and DESIGN.md 3.1k; the grid, its cell
// walk and the fp32 distance rule are point_grid.h's, the plane fit and the frame are plane_fit.h's.
//
// Normals: one launch, one WAVE per query, four per workgroup, the skeleton of the grid's nearest-point query.  A wave sweeps
// its candidates (the records of the 27 cells around the query, 64 per pass) up to three times:
//   count    the members (d2 <= r2), and the smallest and largest member key d2 bits << 32 | row
//   cut      only when max_nn > 0 and count > max_nn: a bisection on the 64-bit key between those two for the threshold T with
//            exactly max_nn member keys <= T (the keys are distinct: a row occurs once).  One sweep per step, at most 64 steps,
//            no storage.
//   moments  every lane adds the nine int64 terms of its members with key <= T; the wave sum is the integer xor tree
// and, when the caller wants the rows, a rank pass: a member's slot is the number of neighbourhood keys below its own, counted by
// passing every candidate key round the wave.  Then lane 0 of each wave leaves its sums in LDS and, after one barrier, threads
// 0..3 of the workgroup each finish one query (covariance, Jacobi, sign: fp64 on one lane each), so that the eigen-solve is
// issued once per four queries and not once per query.
// Frames: one launch, one workgroup per patch; every thread derives the frame from the patch's normal (the same few fp64
// operations in every lane) and rotates rows tid, tid + 256, ..: a row is read and written by the same thread, so `out` may be
// `patches`.
// Every record index is below n (record_of), every output index is below its row's length; nothing waits on another workgroup,
// there are no floating-point atomics and no scratch.
#include "epn_reduce.h"
#include "plane_fit.h"
#include "point_grid.h"

namespace {

using namespace epn_grid;

constexpr int MAX_NN = 1024;
constexpr int MAX_SAMPLE = 8192;
constexpr int PT = 256;                  // threads per workgroup of the frame kernel

// The key of candidate t of the wave's query when it is a member of the in-radius set, NONE otherwise; p = its record.  Every
// lane of the wave calls it.
__device__ __forceinline__ unsigned long long candidate_key(const Cells &cells, const int4 *__restrict__ records, int n, int t,
                                                            float qx, float qy, float qz, float r2, int4 &p) {
    const int at = record_of(cells, t, n);
    if (at < 0) return NONE;
    p = records[at];
    const float d2 = dist2(__int_as_float(p.x), __int_as_float(p.y), __int_as_float(p.z), qx, qy, qz);
    return d2 <= r2 ? member_key(d2, p.w) : NONE;
}

// n == 0 (an empty grid) reads nothing of head, slots and records.
__global__ __launch_bounds__(QW * 64) void point_normals_kernel(const Head *__restrict__ head, const Slot *__restrict__ slots,
                                                                const int4 *__restrict__ records, int n, int log2cap, double edge,
                                                                const float *__restrict__ qry, int m, float r2, double radius,
                                                                int max_nn, const float *__restrict__ view,
                                                                float *__restrict__ normals, float *__restrict__ eig,
                                                                int32_t *__restrict__ count, int32_t *__restrict__ flags,
                                                                long long *__restrict__ moments, int32_t *__restrict__ nbr_idx) {
    __shared__ long long wmom[QW][9];
    __shared__ int wcount[QW], wused[QW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = (int)blockIdx.x * QW + wave;             // the same in every lane of the wave
    long long mom[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int cnt = 0, used = 0;
    if (q < m) {
        const float qx = qry[3 * (size_t)q], qy = qry[3 * (size_t)q + 1], qz = qry[3 * (size_t)q + 2];
        if (n > 0 && isfinite(qx) && isfinite(qy) && isfinite(qz)) {
            const Cells cells = find_cells(head, slots, n, log2cap, edge, qx, qy, qz, lane);
            int4 p = make_int4(0, 0, 0, 0);
            unsigned long long lo = NONE, hi = 0;
            for (int base = 0; base < cells.total; base += 64) {   // every lane runs every pass: the shuffles read all of them
                const unsigned long long k = candidate_key(cells, records, n, base + lane, qx, qy, qz, r2, p);
                if (k != NONE) {
                    ++cnt;
                    lo = k < lo ? k : lo;
                    hi = k > hi ? k : hi;
                }
            }
            cnt = epn_wave_isum(cnt);
            lo = epn_wave_imin(lo);
            hi = epn_wave_imax(hi);
            used = cnt;
            // the threshold: every member key is <= hi < NONE, so "k <= T" also leaves the non-members out
            if (max_nn > 0 && cnt > max_nn) {
                used = max_nn;
                // max_nn keys are <= hi and fewer are <= lo - 1; halve until lo == hi (at most 64 steps)
                for (int step = 0; step < 64 && lo < hi; ++step) {
                    const unsigned long long mid = lo + ((hi - lo) >> 1);
                    int below = 0;
                    for (int base = 0; base < cells.total; base += 64)
                        below += candidate_key(cells, records, n, base + lane, qx, qy, qz, r2, p) <= mid;
                    below = epn_wave_isum(below);
                    if (below >= max_nn) hi = mid;
                    else lo = mid + 1;
                }
            }
            const unsigned long long T = hi;
            for (int base = 0; base < cells.total; base += 64) {
                if (candidate_key(cells, records, n, base + lane, qx, qy, qz, r2, p) <= T)
                    epn_plane::moments_add(mom, epn_plane::scaled_offset(__int_as_float(p.x), qx, radius),
                                           epn_plane::scaled_offset(__int_as_float(p.y), qy, radius),
                                           epn_plane::scaled_offset(__int_as_float(p.z), qz, radius));
            }
#pragma unroll
            for (int e = 0; e < 9; ++e) mom[e] = epn_wave_isum(mom[e]);
            if (nbr_idx) {                                 // the same in every thread; max_nn >= 1 with it
                int32_t *__restrict__ mine = nbr_idx + (size_t)q * max_nn;
                for (int base = 0; base < cells.total; base += 64) {
                    unsigned long long k = candidate_key(cells, records, n, base + lane, qx, qy, qz, r2, p);
                    if (k > T) k = NONE;
                    const int row = p.w;
                    int rank = 0;                          // the neighbourhood keys below k
                    for (int other = 0; other < cells.total; other += 64) {
                        int4 po;
                        unsigned long long ko = candidate_key(cells, records, n, other + lane, qx, qy, qz, r2, po);
                        if (ko > T) ko = NONE;
                        for (int l = 0; l < 64; ++l) rank += __shfl(ko, l, 64) < k;
                    }
                    if (k != NONE && rank < max_nn) mine[rank] = row;
                }
            }
        }
        if (nbr_idx)
            for (int j = used + lane; j < max_nn; j += 64) nbr_idx[(size_t)q * max_nn + j] = -1;
    }
    if (lane == 0) {
#pragma unroll
        for (int e = 0; e < 9; ++e) wmom[wave][e] = mom[e];
        wcount[wave] = cnt;
        wused[wave] = used;
    }
    __syncthreads();
    const int f = (int)blockIdx.x * QW + (int)threadIdx.x; // the query thread 0..3 finishes
    if (threadIdx.x < QW && f < m) {
        const float qf[3] = {qry[3 * (size_t)f], qry[3 * (size_t)f + 1], qry[3 * (size_t)f + 2]};
        const double qd[3] = {(double)qf[0], (double)qf[1], (double)qf[2]};
        const double vd[3] = {view ? (double)view[0] : 0.0, view ? (double)view[1] : 0.0, view ? (double)view[2] : 0.0};
        long long s[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) s[e] = wmom[threadIdx.x][e];
        float nf[3], ef[3];
        int fl = epn_plane::plane_fit(s, wused[threadIdx.x], radius, qd, view != nullptr, vd, nf, ef);
        if (!(isfinite(qf[0]) && isfinite(qf[1]) && isfinite(qf[2]))) fl |= epn_plane::FLAG_QUERY;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            normals[3 * (size_t)f + e] = nf[e];
            eig[3 * (size_t)f + e] = ef[e];
        }
        count[f] = wcount[threadIdx.x];
        flags[f] = fl;
        if (moments) {
#pragma unroll
            for (int e = 0; e < 9; ++e) moments[9 * (size_t)f + e] = s[e];
        }
    }
}

__global__ __launch_bounds__(PT) void orient_patches_kernel(const float *patches, const float *__restrict__ normals, int n_sample,
                                                            float *__restrict__ axis, float *out) {
    const size_t k = blockIdx.x;
    const float nrm[3] = {normals[3 * k], normals[3 * k + 1], normals[3 * k + 2]};
    float a[9];
    epn_plane::patch_frame(nrm, a);                        // the same in every thread
    if (threadIdx.x < 9) axis[9 * k + threadIdx.x] = a[threadIdx.x];
    for (int r = threadIdx.x; r < n_sample; r += PT) {
        const size_t at = 3 * (k * (size_t)n_sample + (size_t)r);
        const float p[3] = {patches[at], patches[at + 1], patches[at + 2]};
        float o[3];
        epn_plane::rotate_row(p, a, o);
        out[at] = o[0];
        out[at + 1] = o[1];
        out[at + 2] = o[2];
    }
}

}  // namespace

extern "C" int epn_point_normals_f32(const void *workspace, int64_t n, const float *qry, int64_t m, double radius, int max_nn,
                                     int self_rows, const float *view, float *normals, float *eig, int32_t *count, int32_t *flags,
                                     int64_t *moments, int32_t *nbr_idx, epn_stream_t stream) {
    // every argument is checked before the first HIP runtime call
    if (n < 0 || n > MAX_N || m < 0 || m > MAX_N || !std::isfinite(radius) || !(radius > 0.0)) return EPN_EINVAL;
    if (max_nn < 0 || max_nn > MAX_NN || (nbr_idx && max_nn == 0)) return EPN_EINVAL;
    if (self_rows != 0 && self_rows != 1) return EPN_EINVAL;
    if (self_rows && m != n) return EPN_EINVAL;
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15u) != 0) return EPN_EINVAL;
    Built b;
    if (!recall(workspace, b) || b.n != n || radius > b.max_radius) return EPN_EINVAL;
    if (m > 0 && (!qry || !normals || !eig || !count || !flags)) return EPN_EINVAL;
    if (m == 0) return 0;
    const Layout L = layout(n);
    const char *ws = static_cast<const char *>(workspace);
    EPN_LAUNCH(point_normals_kernel, dim3((unsigned)epn_cdiv(m, QW)), dim3(QW * 64), 0, epn_stream(stream),
               reinterpret_cast<const Head *>(ws), reinterpret_cast<const Slot *>(ws + L.slots),
               reinterpret_cast<const int4 *>(ws + L.records), (int)n, L.log2cap, cell_edge(b.max_radius), qry, (int)m,
               (float)(radius * radius), radius, max_nn, view, normals, eig, count, flags, reinterpret_cast<long long *>(moments),
               nbr_idx);
    EPN_CHECK_LAUNCH();
    return 0;
}

extern "C" int epn_orient_patches_f32(const float *patches, const float *normals, int64_t k, int n_sample, float *axis, float *out,
                                      epn_stream_t stream) {
    // every argument is checked before the first HIP runtime call
    if (k < 0 || k > MAX_N || n_sample < 1 || n_sample > MAX_SAMPLE) return EPN_EINVAL;
    if (k > 0 && (!patches || !normals || !axis || !out)) return EPN_EINVAL;
    if (k == 0) return 0;
    EPN_LAUNCH(orient_patches_kernel, dim3((unsigned)k), dim3(PT), 0, epn_stream(stream), patches, normals, n_sample, axis, out);
    EPN_CHECK_LAUNCH();
    return 0;
}
