// Voxel-grid downsampling for gfx950: one centroid per occupied voxel of a fragment, the stage the reference runs on the host
// before it searches a fragment (SPConvNets/datasets/match_3dmatch.py:107-139: open3d's pcd.voxel_down_sample, then the
// KD-tree over the centroids).  Specification: include/epn_so3conv.h (epn_voxel_downsample_f32) and DESIGN.md 3.1.
//
// Seven launches on the call's stream, every one a grid of 256-thread workgroups over points or over table slots:
//   init    the table (empty keys, zero sums, first = INT_MAX) and the header (minima +inf, flags 0): one kernel, no memsets
//   bounds  per-axis fp32 minimum of the kept points: wave shuffles, LDS across the four waves, one integer atomicMin per
//           workgroup and axis on the order-preserving image of the float; flag bit 0 for |coordinate| > 256
//   insert  voxel index in fp64, key = ix << 42 | iy << 21 | iz, home slot (key * 0x9E3779B97F4A7C15) >> (64 - log2 cap), linear
//           probing with wrap-around; a slot is claimed by one 64-bit atomicCAS on its key (a relaxed load first: a key, once
//           set, never changes, so a non-empty value read is final); then three 64-bit integer atomicAdds (fixed-point
//           coordinates), one on the count, one atomicMin on the first index.  The point remembers its slot.
//   count   flag(i) = point i is its voxel's first; per-workgroup sum of the flags (ballot + popcount)
//   scan    ONE workgroup turns the per-workgroup sums into exclusive offsets, 256 at a time with a running carry; it also
//           writes status = {M, flags}
//   write   rank(i) = offset of i's workgroup + flags below i inside it; the first point of a voxel writes the voxel's row
//           (centroid, count, first index) at its rank and leaves the rank in the slot
//   rows    point_voxel[i] = rank stored in i's slot, -1 for a dropped point
// The sums are integers and the minimum is a minimum: nothing depends on arrival order, so the result is bitwise repeatable.
// Every probe loop is bounded by the capacity (the load factor is at most 1/2, so a free slot exists); no workgroup waits on
// another, nothing spins, no floating-point atomics.  Every table index is masked by capacity - 1, every point index is below n
// and every rank below M <= n (the caller allocates n rows).  The cell rule, the hash probing, the bounds reduction and the
// workgroup scans live in cell_hash.h, which point_grid.hip shares.
#include "cell_hash.h"

namespace {

using namespace epn_cells;               // the cell rule, the hash table and the workgroup scans: shared with point_grid.hip

constexpr int64_t VOX_MAX_N = MAX_N;

struct Slot {                            // 48 bytes: one voxel
    unsigned long long key;
    unsigned long long sum[3];           // two's complement sums of llrint(coordinate * 2^32)
    int count, first, row, pad;
};

struct Layout {
    int log2cap;
    size_t cap, slots, pslot, bcnt, bytes;   // byte offsets of the table, the points' slots and the scan's sums
};

Layout layout(int64_t n) {
    Layout L;
    L.log2cap = log2_capacity(n);
    L.cap = (size_t)1 << L.log2cap;
    L.slots = sizeof(Head);
    L.pslot = L.slots + L.cap * sizeof(Slot);
    L.bcnt = L.pslot + (size_t)n * sizeof(int);
    L.bytes = L.bcnt + (size_t)epn_cdiv(n, VT) * sizeof(int);
    return L;
}

__global__ __launch_bounds__(VT) void voxel_init_kernel(Head *head, Slot *slots, unsigned cap) {
    const unsigned e = blockIdx.x * VT + threadIdx.x;
    if (e == 0) init_head(head);
    if (e >= cap) return;
    Slot s;
    s.key = EMPTY;
    s.sum[0] = s.sum[1] = s.sum[2] = 0ull;
    s.count = 0;
    s.first = INT_MAX;
    s.row = -1;
    s.pad = 0;
    slots[e] = s;
}

__global__ __launch_bounds__(VT) void voxel_bounds_kernel(const float *__restrict__ pc, int n, Head *head) {
    const int i = (int)blockIdx.x * VT + (int)threadIdx.x;
    float x = INFINITY, y = INFINITY, z = INFINITY;
    int far = 0;
    if (i < n) {
        float px, py, pz;
        if (load_point(pc, i, px, py, pz)) {
            x = px; y = py; z = pz;
            far = too_far(px, py, pz);
        }
    }
    bounds_body(x, y, z, far, head);
}

__global__ __launch_bounds__(VT) void voxel_insert_kernel(const float *__restrict__ pc, int n, double voxel_size, int log2cap,
                                                          Head *head, Slot *slots, int *__restrict__ pslot) {
    const int i = (int)blockIdx.x * VT + (int)threadIdx.x;
    if (i >= n) return;
    float x, y, z;
    int mine = -1;
    if (load_point(pc, i, x, y, z) && !too_far(x, y, z)) {
        const double ix = cell_axis(x, head->lo[0], voxel_size);
        const double iy = cell_axis(y, head->lo[1], voxel_size);
        const double iz = cell_axis(z, head->lo[2], voxel_size);
        if (!(ix < INDEX_END && iy < INDEX_END && iz < INDEX_END)) {
            atomicOr(&head->flags, FLAG_INDEX);
        } else {
            mine = claim_slot(slots, cell_key(ix, iy, iz), log2cap);
            if (mine < 0) {
                atomicOr(&head->flags, FLAG_TABLE);        // cannot happen at a load factor <= 1/2; loud if it ever does
            } else {
                Slot *v = slots + mine;
                atomicAdd(&v->sum[0], (unsigned long long)llrint((double)x * 4294967296.0));
                atomicAdd(&v->sum[1], (unsigned long long)llrint((double)y * 4294967296.0));
                atomicAdd(&v->sum[2], (unsigned long long)llrint((double)z * 4294967296.0));
                atomicAdd(&v->count, 1);
                atomicMin(&v->first, i);
            }
        }
    }
    pslot[i] = mine;
}

// is point i (a thread of this workgroup; i >= n: no) the first of its voxel?
__device__ __forceinline__ bool is_first(const int *__restrict__ pslot, const Slot *__restrict__ slots, int i, int n, int &s) {
    s = i < n ? pslot[i] : -1;
    return s >= 0 && slots[s].first == i;
}

__global__ __launch_bounds__(VT) void voxel_count_kernel(const int *__restrict__ pslot, const Slot *__restrict__ slots, int n,
                                                         int *__restrict__ bcnt) {
    __shared__ int wsum[VW];
    const int tid = threadIdx.x;
    int s;
    const unsigned long long m = __ballot(is_first(pslot, slots, (int)blockIdx.x * VT + tid, n, s));
    if ((tid & 63) == 0) wsum[tid >> 6] = __popcll(m);
    __syncthreads();
    if (tid == 0) {
        int t = 0;
#pragma unroll
        for (int w = 0; w < VW; ++w) t += wsum[w];
        bcnt[blockIdx.x] = t;
    }
}

// one workgroup: bcnt[0..nb) -> exclusive prefix sums in place, VT entries per pass with a running carry
__global__ __launch_bounds__(VT) void voxel_scan_kernel(int *bcnt, int nb, const Head *head, int32_t *__restrict__ status) {
    const int total = scan_sums(bcnt, nb);
    if (threadIdx.x == 0) {
        status[0] = total;
        status[1] = (int32_t)head->flags;
    }
}

__global__ __launch_bounds__(VT) void voxel_write_kernel(const int *__restrict__ pslot, Slot *slots, int n,
                                                         const int *__restrict__ bcnt, float *__restrict__ centroids,
                                                         int32_t *__restrict__ counts, int32_t *__restrict__ first_idx) {
    __shared__ int wsum[VW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = (int)blockIdx.x * VT + tid;
    int s;
    const bool first = is_first(pslot, slots, i, n, s);
    const unsigned long long m = __ballot(first);
    if (lane == 0) wsum[wave] = __popcll(m);
    __syncthreads();
    if (!first) return;
    int row = bcnt[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
#pragma unroll
    for (int w = 0; w < VW; ++w) row += w < wave ? wsum[w] : 0;
    Slot *v = slots + s;                                   // only this thread touches the slot in this kernel
    const int count = v->count;
    const double scale = (double)count * 4294967296.0;
    centroids[3 * (size_t)row] = (float)((double)(long long)v->sum[0] / scale);
    centroids[3 * (size_t)row + 1] = (float)((double)(long long)v->sum[1] / scale);
    centroids[3 * (size_t)row + 2] = (float)((double)(long long)v->sum[2] / scale);
    counts[row] = count;
    first_idx[row] = i;
    v->row = row;
}

__global__ __launch_bounds__(VT) void voxel_rows_kernel(const int *__restrict__ pslot, const Slot *__restrict__ slots, int n,
                                                        int32_t *__restrict__ point_voxel) {
    const int i = (int)blockIdx.x * VT + (int)threadIdx.x;
    if (i >= n) return;
    const int s = pslot[i];
    point_voxel[i] = s >= 0 ? slots[s].row : -1;
}

}  // namespace

extern "C" size_t epn_voxel_downsample_workspace_bytes(int64_t n) {
    return n > 0 && n <= VOX_MAX_N ? layout(n).bytes : 0;
}

extern "C" int epn_voxel_downsample_f32(const float *pc, int64_t n, double voxel_size, float *centroids, int32_t *counts,
                                        int32_t *first_idx, int32_t *point_voxel, int32_t *status, void *workspace,
                                        size_t workspace_bytes, epn_stream_t stream) {
    // every argument is checked before the first HIP runtime call
    if (n < 0 || n > VOX_MAX_N || !std::isfinite(voxel_size) || !(voxel_size > 0.0)) return EPN_EINVAL;
    if (n == 0) return 0;
    if (!pc || !centroids || !counts || !first_idx || !point_voxel || !status) return EPN_EINVAL;
    const Layout L = layout(n);
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7u) != 0 || workspace_bytes < L.bytes) return EPN_EINVAL;
    hipStream_t st = epn_stream(stream);
    char *ws = static_cast<char *>(workspace);
    Head *head = reinterpret_cast<Head *>(ws);
    Slot *slots = reinterpret_cast<Slot *>(ws + L.slots);
    int *pslot = reinterpret_cast<int *>(ws + L.pslot), *bcnt = reinterpret_cast<int *>(ws + L.bcnt);
    const int ni = (int)n, nb = epn_cdiv(n, VT);
    const dim3 points((unsigned)nb), block(VT);
    EPN_LAUNCH_AUX(voxel_init_kernel, dim3((unsigned)epn_cdiv((long long)L.cap, VT)), block, 0, st, head, slots, (unsigned)L.cap);
    EPN_LAUNCH_AUX(voxel_bounds_kernel, points, block, 0, st, pc, ni, head);
    EPN_LAUNCH(voxel_insert_kernel, points, block, 0, st, pc, ni, voxel_size, L.log2cap, head, slots, pslot);
    EPN_LAUNCH_AUX(voxel_count_kernel, points, block, 0, st, pslot, slots, ni, bcnt);
    EPN_LAUNCH_AUX(voxel_scan_kernel, dim3(1), block, 0, st, bcnt, nb, head, status);
    EPN_LAUNCH_AUX(voxel_write_kernel, points, block, 0, st, pslot, slots, ni, bcnt, centroids, counts, first_idx);
    EPN_LAUNCH_AUX(voxel_rows_kernel, points, block, 0, st, pslot, slots, ni, point_voxel);
    EPN_CHECK_LAUNCH();
    return 0;
}
