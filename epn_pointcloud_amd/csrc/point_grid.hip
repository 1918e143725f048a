// Nearest 3-D point within a bound, for gfx950: a hashed grid over ONE cloud with its points sorted by cell, and the query that
// walks the 27 cells around a point.  It replaces the host trees of the reference's keypoint stage
// (SPConvNets/datasets/preprocess/run_keypoint.py: sklearn's NearestNeighbors at :30-37, :98-112 and :131-138, open3d's radius
// search behind compute_fpfh_feature at :47-48).  Specification: include/epn_so3conv.h (epn_point_grid_build_f32,
// epn_point_grid_nn_f32) and DESIGN.md 3.1j; the cell rule and the hash table are voxel_grid.hip's (cell_hash.h).
//
// Build: seven launches on the call's stream, every one a grid of 256-thread workgroups over points or over table slots:
//   init     the table (empty keys, zero counts) and the header (minima +inf, flags 0): one kernel, no memsets
//   bounds   per-axis fp32 minimum of the participating points; flag bit 0 for |coordinate| > 256
//   count    cell of every participating point (edge = max_radius * (1 + 2^-10)); the slot is claimed as in the voxel kernel,
//            one integer atomicAdd on its count.  The point remembers its slot.
//   tiles    per-workgroup sum of the counts of 256 slots
//   scan     ONE workgroup turns the per-tile sums into exclusive offsets; it also writes status = {kept, flags}
//   offsets  cursor(slot) = offset of its tile + counts below it inside the tile: where the cell's run of records starts
//   scatter  record {x, y, z, row} of point i at atomicAdd(cursor of its slot, 1): afterwards cursor = the END of the run and
//            the run is [cursor - count, cursor).  The order inside a run depends on arrival; no output depends on it.
// Query: one launch, one WAVE per query, four per workgroup (plus a one-wave launch that zeroes `hits` when it is asked for: the
// query's workgroups add to it and none may wait for another, so the zero has to be there before the first of them starts).
//   Lanes 0..26 each look up one of the 27 cells around the query's (find_slot: reads only) and keep (start, count) of its run.
//   A prefix sum of the 27 counts across the wave numbers the candidates 0..total-1; lane l takes candidates l, l + 64, ...: it
//   finds the candidate's cell by a five-step search of the prefix sums (shuffles) and loads the 16-byte record, so consecutive
//   lanes read consecutive records of a run.  The running best is one 64-bit key, d2 bits << 32 | row (d2 >= 0, so its bits
//   order like its value); a minimum over the wave by shuffles gives the smallest distance and, on a tie, the lowest row.
//   No LDS but four ints for `hits`, no floating-point atomics, no scratch.
// Every probe loop is bounded by the capacity, every slot index is masked by capacity - 1, every record index is below n (the
// run ends are clamped to [0, n] on reading, so even a workspace that was overwritten cannot send a load out of it); nothing
// waits on another workgroup.
#include <mutex>
#include <unordered_map>

#include "point_grid.h"

namespace epn_grid {

// What the query's argument checks need of the build, kept on the host per workspace address (the workspace itself is device
// memory, and a refusal is decided before any HIP runtime call).  A build replaces its address' entry.  The table is emptied
// when it reaches MAX_GRIDS addresses: queries on the grids built before that are then refused until they are built again.
namespace {
constexpr size_t MAX_GRIDS = 1 << 16;
std::mutex g_mutex;
std::unordered_map<const void *, Built> g_built;

void remember(const void *workspace, int64_t n, double max_radius) {
    std::lock_guard<std::mutex> lock(g_mutex);
    if (g_built.size() >= MAX_GRIDS && !g_built.count(workspace)) g_built.clear();
    g_built[workspace] = Built{n, max_radius};
}
}  // namespace

bool recall(const void *workspace, Built &b) {
    std::lock_guard<std::mutex> lock(g_mutex);
    const auto it = g_built.find(workspace);
    if (it == g_built.end()) return false;
    b = it->second;
    return true;
}

}  // namespace epn_grid

namespace {

using namespace epn_grid;

constexpr double MIN_RADIUS = 0x1p-60;   // below it the fp32 products of admissible differences underflow (the header's argument)

__device__ __forceinline__ bool takes_part(const float *__restrict__ ref, const uint8_t *__restrict__ valid, int i, float &x,
                                           float &y, float &z) {
    return load_point(ref, i, x, y, z) && (!valid || valid[i] != 0);
}

__global__ __launch_bounds__(VT) void grid_init_kernel(Head *head, Slot *slots, unsigned cap) {
    const unsigned e = blockIdx.x * VT + threadIdx.x;
    if (e == 0) init_head(head);
    if (e >= cap) return;
    Slot s;
    s.key = EMPTY;
    s.count = 0;
    s.cursor = 0;
    slots[e] = s;
}

__global__ __launch_bounds__(VT) void grid_bounds_kernel(const float *__restrict__ ref, const uint8_t *__restrict__ valid, int n,
                                                         Head *head) {
    const int i = (int)blockIdx.x * VT + (int)threadIdx.x;
    float x = INFINITY, y = INFINITY, z = INFINITY;
    int far = 0;
    if (i < n) {
        float px, py, pz;
        if (takes_part(ref, valid, i, px, py, pz)) {
            x = px; y = py; z = pz;
            far = too_far(px, py, pz);
        }
    }
    bounds_body(x, y, z, far, head);
}

__global__ __launch_bounds__(VT) void grid_count_kernel(const float *__restrict__ ref, const uint8_t *__restrict__ valid, int n,
                                                        double edge, int log2cap, Head *head, Slot *slots,
                                                        int *__restrict__ pslot) {
    const int i = (int)blockIdx.x * VT + (int)threadIdx.x;
    if (i >= n) return;
    float x, y, z;
    int mine = -1;
    if (takes_part(ref, valid, i, x, y, z) && !too_far(x, y, z)) {
        const double ix = cell_axis(x, head->lo[0], edge);
        const double iy = cell_axis(y, head->lo[1], edge);
        const double iz = cell_axis(z, head->lo[2], edge);
        if (!(ix < INDEX_END && iy < INDEX_END && iz < INDEX_END)) {
            atomicOr(&head->flags, FLAG_INDEX);
        } else {
            mine = claim_slot(slots, cell_key(ix, iy, iz), log2cap);
            if (mine < 0) atomicOr(&head->flags, FLAG_TABLE);  // cannot happen at a load factor <= 1/2; loud if it ever does
            else atomicAdd(&slots[mine].count, 1);
        }
    }
    pslot[i] = mine;
}

__global__ __launch_bounds__(VT) void grid_tiles_kernel(const Slot *__restrict__ slots, unsigned cap, int *__restrict__ tsum) {
    __shared__ int wsum[VW];
    const unsigned e = blockIdx.x * VT + threadIdx.x;
    int total;
    tile_scan(e < cap ? slots[e].count : 0, wsum, total);
    if (threadIdx.x == 0) tsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(VT) void grid_scan_kernel(int *tsum, int nt, const Head *head, int32_t *__restrict__ status) {
    const int total = scan_sums(tsum, nt);
    if (threadIdx.x == 0) {
        status[0] = total;
        status[1] = (int32_t)head->flags;
    }
}

__global__ __launch_bounds__(VT) void grid_offsets_kernel(Slot *slots, unsigned cap, const int *__restrict__ tsum) {
    __shared__ int wsum[VW];
    const unsigned e = blockIdx.x * VT + threadIdx.x;
    int total;
    const int below = tile_scan(e < cap ? slots[e].count : 0, wsum, total);
    if (e < cap) slots[e].cursor = tsum[blockIdx.x] + below;
}

__global__ __launch_bounds__(VT) void grid_scatter_kernel(const float *__restrict__ ref, int n, const int *__restrict__ pslot,
                                                          Slot *slots, int4 *__restrict__ records) {
    const int i = (int)blockIdx.x * VT + (int)threadIdx.x;
    if (i >= n) return;
    const int s = pslot[i];
    if (s < 0) return;
    const int at = atomicAdd(&slots[s].cursor, 1);
    if (at < 0 || at >= n) return;                         // the counts sum to at most n: cannot happen
    records[at] = make_int4(__float_as_int(ref[3 * (size_t)i]), __float_as_int(ref[3 * (size_t)i + 1]),
                          __float_as_int(ref[3 * (size_t)i + 2]), i);
}

__global__ void grid_zero_hits_kernel(int32_t *hits) {
    if (threadIdx.x == 0) *hits = 0;
}

// n == 0 (an empty grid) reads nothing of head, slots and records.
__global__ __launch_bounds__(QW * 64) void grid_nn_kernel(const Head *__restrict__ head, const Slot *__restrict__ slots,
                                                          const int4 *__restrict__ records, int n, int log2cap, double edge,
                                                          const float *__restrict__ qry, int m, float r2, int exclude_row,
                                                          int32_t *__restrict__ nn_idx, float *__restrict__ nn_d2,
                                                          int32_t *__restrict__ hits) {
    __shared__ int whit[QW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = (int)blockIdx.x * QW + wave;             // the same in every lane of the wave
    unsigned long long best = NONE;
    if (q < m && n > 0) {
        const float qx = qry[3 * (size_t)q], qy = qry[3 * (size_t)q + 1], qz = qry[3 * (size_t)q + 2];
        best = nearest_member(head, slots, records, n, log2cap, edge, qx, qy, qz, r2, exclude_row, q, lane).key;
    }
    if (q < m && lane == 0) {
        nn_idx[q] = best == NONE ? -1 : (int32_t)(unsigned)(best & 0xFFFFFFFFull);
        nn_d2[q] = best == NONE ? INFINITY : __uint_as_float((unsigned)(best >> 32));
    }
    if (hits) {                                            // the same in every thread
        if (lane == 0) whit[wave] = best != NONE;
        __syncthreads();
        if (threadIdx.x == 0) {
            int t = 0;
#pragma unroll
            for (int w = 0; w < QW; ++w) t += whit[w];
            if (t) atomicAdd(hits, t);
        }
    }
}

}  // namespace

extern "C" size_t epn_point_grid_workspace_bytes(int64_t n) {
    return n >= 0 && n <= MAX_N ? layout(n).bytes : 0;
}

extern "C" int epn_point_grid_build_f32(const float *ref, int64_t n, const uint8_t *ref_valid, double max_radius, void *workspace,
                                        size_t workspace_bytes, int32_t *status, epn_stream_t stream) {
    // every argument is checked before the first HIP runtime call
    if (n < 0 || n > MAX_N || !std::isfinite(max_radius) || !(max_radius >= MIN_RADIUS)) return EPN_EINVAL;
    const Layout L = layout(n);
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15u) != 0 || workspace_bytes < L.bytes) return EPN_EINVAL;
    if (n > 0 && (!ref || !status)) return EPN_EINVAL;
    remember(workspace, n, max_radius);
    if (n == 0) return 0;                                  // an empty grid: the queries read nothing of the workspace
    hipStream_t st = epn_stream(stream);
    char *ws = static_cast<char *>(workspace);
    Head *head = reinterpret_cast<Head *>(ws);
    int4 *records = reinterpret_cast<int4 *>(ws + L.records);
    Slot *slots = reinterpret_cast<Slot *>(ws + L.slots);
    int *pslot = reinterpret_cast<int *>(ws + L.pslot), *tsum = reinterpret_cast<int *>(ws + L.tsum);
    const int ni = (int)n, nt = epn_cdiv((long long)L.cap, VT);
    const dim3 points((unsigned)epn_cdiv(n, VT)), tiles((unsigned)nt), block(VT);
    const double edge = cell_edge(max_radius);
    EPN_LAUNCH_AUX(grid_init_kernel, tiles, block, 0, st, head, slots, (unsigned)L.cap);
    EPN_LAUNCH_AUX(grid_bounds_kernel, points, block, 0, st, ref, ref_valid, ni, head);
    EPN_LAUNCH_AUX(grid_count_kernel, points, block, 0, st, ref, ref_valid, ni, edge, L.log2cap, head, slots, pslot);
    EPN_LAUNCH_AUX(grid_tiles_kernel, tiles, block, 0, st, slots, (unsigned)L.cap, tsum);
    EPN_LAUNCH_AUX(grid_scan_kernel, dim3(1), block, 0, st, tsum, nt, head, status);
    EPN_LAUNCH_AUX(grid_offsets_kernel, tiles, block, 0, st, slots, (unsigned)L.cap, tsum);
    EPN_LAUNCH(grid_scatter_kernel, points, block, 0, st, ref, ni, pslot, slots, records);
    EPN_CHECK_LAUNCH();
    return 0;
}

extern "C" int epn_point_grid_nn_f32(const void *workspace, int64_t n, const float *qry, int64_t m, double radius, int exclude_row,
                                     int32_t *nn_idx, float *nn_d2, int32_t *hits, epn_stream_t stream) {
    // every argument is checked before the first HIP runtime call
    if (n < 0 || n > MAX_N || m < 0 || m > MAX_N || !std::isfinite(radius) || !(radius > 0.0)) return EPN_EINVAL;
    if (exclude_row != 0 && exclude_row != 1) return EPN_EINVAL;
    if (exclude_row && m != n) return EPN_EINVAL;
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15u) != 0) return EPN_EINVAL;
    Built b;
    if (!recall(workspace, b) || b.n != n || radius > b.max_radius) return EPN_EINVAL;
    if (m > 0 && (!qry || !nn_idx || !nn_d2)) return EPN_EINVAL;
    hipStream_t st = epn_stream(stream);
    if (hits) EPN_LAUNCH_AUX(grid_zero_hits_kernel, dim3(1), dim3(64), 0, st, hits);
    if (m > 0) {
        const Layout L = layout(n);
        const char *ws = static_cast<const char *>(workspace);
        EPN_LAUNCH(grid_nn_kernel, dim3((unsigned)epn_cdiv(m, QW)), dim3(QW * 64), 0, st, reinterpret_cast<const Head *>(ws),
                   reinterpret_cast<const Slot *>(ws + L.slots), reinterpret_cast<const int4 *>(ws + L.records), (int)n,
                   L.log2cap, cell_edge(b.max_radius), qry, (int)m, (float)(radius * radius), exclude_row, nn_idx, nn_d2, hits);
    }
    if (hits || m > 0) EPN_CHECK_LAUNCH();
    return 0;
}
