// FPFH descriptors of a cloud from its point grid and its normals, for gfx950.  It replaces what the reference does on the host
// with open3d (compute_fpfh_feature, SPConvNets/datasets/preprocess/run_keypoint.py:40-50: a KD-tree radius search and
// ComputeFPFHFeature).  Specification: include/epn_so3conv.h (epn_point_fpfh_f32) and DESIGN.md 3.1n; the grid, its cell walk
// and the fp32 distance rule are point_grid.h's, the pair features, the bins and the fixed-point weighting are fpfh_math.h's.
//
// Two launches, both with the skeleton of the grid's nearest-point query: one WAVE per point, four per workgroup; lanes 0..26
// look up the 27 cells around the point and the wave strides over their records, 64 per pass.
//   spfh   every lane computes the three pair features of its candidate in fp64 (the neighbour's normal is a 12-byte gather by
//          row) and adds 1 to three of the 33 integer bins its wave keeps in LDS (integer ds_add: order-free).  Lanes 0..32 then
//          write the counts; lane 0 the size of the neighbourhood, the smallest non-zero d2 in it, and the flags.
//   fpfh   needs every neighbour's finished counts, hence the second launch.  The wave finds its neighbours again; per pass the
//          ballot of the members with d2 > 0 is walked bit by bit (the same in every lane: the neighbour's row and d2 come out
//          of a uniform-lane shuffle), and lane j < 33 reads count j of that neighbour's row -- one coalesced 132-byte read --
//          and adds the fixed-point term to the ONE int64 it keeps for bin j.  No cross-lane sum but the eleven-bin group totals
//          (shuffles), no LDS, no compaction buffer.
// Every record index is below n (record_of), a record's row is used only when it is in [0, n), every output index is below its
// row's length; nothing waits on another workgroup, there are no floating-point atomics and no scratch.
#include "epn_reduce.h"
#include "fpfh_math.h"
#include "point_grid.h"

namespace {

using namespace epn_grid;
using epn_fpfh::WIDTH;

constexpr unsigned NO_D2 = 0x7f800000u;  // +inf: no neighbour at a non-zero distance

struct Scratch {                          // the caller's workspace: counts i32[n,33], then d2min f32[n] (as its bits)
    size_t d2min, bytes;
};

inline Scratch scratch(int64_t n) {
    Scratch s;
    s.d2min = (size_t)n * WIDTH * sizeof(int32_t);
    s.bytes = (s.d2min + (size_t)n * sizeof(unsigned) + 15) & ~(size_t)15;
    return s;
}

// The member of the wave's query q among the grid's in-radius set that candidate t is, or none: its row (-1), d2 and record.
__device__ __forceinline__ int member_row(const Cells &cells, const int4 *__restrict__ records, int n, int t, int q, float qx,
                                          float qy, float qz, float r2, float &d2, int4 &p) {
    const int at = record_of(cells, t, n);
    if (at < 0) return -1;
    p = records[at];
    d2 = dist2(__int_as_float(p.x), __int_as_float(p.y), __int_as_float(p.z), qx, qy, qz);
    return d2 <= r2 && p.w != q && (unsigned)p.w < (unsigned)n ? p.w : -1;
}

// n > 0.  A point the grid left out (pslot < 0: a non-finite coordinate, a zero `valid` byte) reads no cell.
__global__ __launch_bounds__(QW * 64) void spfh_kernel(const Head *__restrict__ head, const Slot *__restrict__ slots,
                                                       const int4 *__restrict__ records, const int *__restrict__ pslot, int n,
                                                       int log2cap, double edge, const float *__restrict__ points,
                                                       const float *__restrict__ normals, float r2,
                                                       int32_t *__restrict__ counts, unsigned *__restrict__ d2min_out,
                                                       int32_t *__restrict__ count, int32_t *__restrict__ flags,
                                                       int32_t *__restrict__ spfh) {
    __shared__ int hist[QW][WIDTH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = (int)blockIdx.x * QW + wave;             // the same in every lane of the wave
    if (lane < WIDTH) hist[wave][lane] = 0;
    __syncthreads();
    int used = 0, fl = 0;
    unsigned d2min = NO_D2;
    if (q < n) {
        const float qp[3] = {points[3 * (size_t)q], points[3 * (size_t)q + 1], points[3 * (size_t)q + 2]};
        const float qn[3] = {normals[3 * (size_t)q], normals[3 * (size_t)q + 1], normals[3 * (size_t)q + 2]};
        const bool in_grid = pslot[q] >= 0 && epn_fpfh::finite3(qp);
        const bool whole = in_grid && epn_fpfh::finite3(qn);
        if (!whole) fl |= epn_fpfh::FLAG_INPUT;
        if (in_grid) {
            const Cells cells = find_cells(head, slots, n, log2cap, edge, qp[0], qp[1], qp[2], lane);
            for (int base = 0; base < cells.total; base += 64) {   // every lane runs every pass: the shuffles read all of them
                int4 p = make_int4(0, 0, 0, 0);
                float d2 = 0.0f;
                const int row = member_row(cells, records, n, base + lane, q, qp[0], qp[1], qp[2], r2, d2, p);
                if (row >= 0) {
                    ++used;
                    if (d2 > 0.0f) d2min = min(d2min, __float_as_uint(d2));
                    if (whole) {
                        const float kp[3] = {__int_as_float(p.x), __int_as_float(p.y), __int_as_float(p.z)};
                        const float kn[3] = {normals[3 * (size_t)row], normals[3 * (size_t)row + 1], normals[3 * (size_t)row + 2]};
                        double f[3], t[3];
                        epn_fpfh::pair_features(qp, qn, kp, kn, f);
                        epn_fpfh::bin_values(f, t);
                        atomicAdd(&hist[wave][epn_fpfh::bin_of(t[0])], 1);
                        atomicAdd(&hist[wave][epn_fpfh::BINS + epn_fpfh::bin_of(t[1])], 1);
                        atomicAdd(&hist[wave][2 * epn_fpfh::BINS + epn_fpfh::bin_of(t[2])], 1);
                    }
                }
            }
            used = epn_wave_isum(used);
            d2min = epn_wave_imin(d2min);
        }
        if (used == 0) fl |= epn_fpfh::FLAG_ALONE;
    }
    __syncthreads();
    if (q < n) {
        if (lane < WIDTH) {
            const int c = hist[wave][lane];
            counts[(size_t)q * WIDTH + lane] = c;
            if (spfh) spfh[(size_t)q * WIDTH + lane] = c;
        }
        if (lane == 0) {
            d2min_out[q] = d2min;
            count[q] = used;
            flags[q] = fl;
        }
    }
}

__global__ __launch_bounds__(QW * 64) void fpfh_kernel(const Head *__restrict__ head, const Slot *__restrict__ slots,
                                                       const int4 *__restrict__ records, int n, int log2cap, double edge,
                                                       const float *__restrict__ points, float r2,
                                                       const int32_t *__restrict__ counts, const unsigned *__restrict__ d2min_in,
                                                       const int32_t *__restrict__ count, const int32_t *__restrict__ flags,
                                                       float *__restrict__ fpfh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = (int)blockIdx.x * QW + wave;             // the same in every lane of the wave
    if (q >= n) return;
    const int bin = lane < WIDTH ? lane : WIDTH - 1;       // lanes 33..63 shadow bin 32 and write nothing
    const int used = count[q];
    float out = 0.0f;
    if (flags[q] == 0) {                                   // in the grid, a finite normal, at least one neighbour
        const float qx = points[3 * (size_t)q], qy = points[3 * (size_t)q + 1], qz = points[3 * (size_t)q + 2];
        const float d2min = __uint_as_float(d2min_in[q]);
        const Cells cells = find_cells(head, slots, n, log2cap, edge, qx, qy, qz, lane);
        long long A = 0;
        for (int base = 0; base < cells.total; base += 64) {       // every lane runs every pass: the shuffles read all of them
            int4 p = make_int4(0, 0, 0, 0);
            float d2 = 0.0f;
            const int row = member_row(cells, records, n, base + lane, q, qx, qy, qz, r2, d2, p);
            unsigned long long todo = __ballot(row >= 0 && d2 > 0.0f);
            while (todo) {                                 // the same in every lane
                const int l = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const int k = __shfl(row, l, 64);
                const float d2k = __shfl(d2, l, 64);
                const int uk = count[k];
                if (uk > 0) A += epn_fpfh::weighted_term(d2min, d2k, counts[(size_t)k * WIDTH + bin], uk);
            }
        }
        long long G = 0;
        const int group = bin / epn_fpfh::BINS;
#pragma unroll
        for (int e = 0; e < epn_fpfh::BINS; ++e) G += __shfl(A, group * epn_fpfh::BINS + e, 64);
        out = epn_fpfh::fpfh_value(A, G, counts[(size_t)q * WIDTH + bin], used);
    }
    if (lane < WIDTH) fpfh[(size_t)q * WIDTH + lane] = out;
}

}  // namespace

extern "C" size_t epn_point_fpfh_workspace_bytes(int64_t n) {
    return n >= 0 && n <= MAX_N ? scratch(n).bytes : 0;
}

extern "C" int epn_point_fpfh_f32(const void *grid_workspace, int64_t n, const float *points, const float *normals, double radius,
                                  float *fpfh, int32_t *count, int32_t *flags, int32_t *spfh, void *workspace,
                                  size_t workspace_bytes, epn_stream_t stream) {
    // every argument is checked before the first HIP runtime call
    if (n < 0 || n > MAX_N || !std::isfinite(radius) || !(radius > 0.0)) return EPN_EINVAL;
    if (!grid_workspace || (reinterpret_cast<uintptr_t>(grid_workspace) & 15u) != 0) return EPN_EINVAL;
    Built b;
    if (!recall(grid_workspace, b) || b.n != n || radius > b.max_radius) return EPN_EINVAL;
    const Scratch S = scratch(n);
    if (n > 0 && (!points || !normals || !fpfh || !count || !flags)) return EPN_EINVAL;
    if (n > 0 && (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15u) != 0 || workspace_bytes < S.bytes)) return EPN_EINVAL;
    if (n == 0) return 0;
    const Layout L = layout(n);
    const char *ws = static_cast<const char *>(grid_workspace);
    const Head *head = reinterpret_cast<const Head *>(ws);
    const Slot *slots = reinterpret_cast<const Slot *>(ws + L.slots);
    const int4 *records = reinterpret_cast<const int4 *>(ws + L.records);
    const int *pslot = reinterpret_cast<const int *>(ws + L.pslot);
    int32_t *counts = static_cast<int32_t *>(workspace);
    unsigned *d2min = reinterpret_cast<unsigned *>(static_cast<char *>(workspace) + S.d2min);
    const dim3 grid((unsigned)epn_cdiv(n, QW)), block(QW * 64);
    const double edge = cell_edge(b.max_radius);
    const float r2 = (float)(radius * radius);
    hipStream_t st = epn_stream(stream);
    EPN_LAUNCH(spfh_kernel, grid, block, 0, st, head, slots, records, pslot, (int)n, L.log2cap, edge, points, normals, r2,
                   counts, d2min, count, flags, spfh);
    EPN_LAUNCH(fpfh_kernel, grid, block, 0, st, head, slots, records, (int)n, L.log2cap, edge, points, r2, counts, d2min, count,
               flags, fpfh);
    EPN_CHECK_LAUNCH();
    return 0;
}
