// Cells of a regular grid over ONE cloud, hashed: what voxel_grid.hip (one centroid per cell) and point_grid.hip (the points
// sorted by cell, for nearest-neighbour queries) share, so that both derive the same cell from the same point, bit for bit.
// The rules are include/epn_so3conv.h's (epn_voxel_downsample_f32: voxel index, range errors, hash table).
//   cell_axis     fp64 index on one axis from the fp32 minimum of that axis: floor((x - (lo - edge / 2)) / edge)
//   cell_key      ix << 42 | iy << 21 | iz, 21 bits per axis; no valid key has bit 63 set, so all-ones marks an empty slot
//   home_slot     (key * 0x9E3779B97F4A7C15) >> (64 - log2(capacity)), 64-bit wrapping arithmetic
//   claim_slot    linear probing with wrap-around; a slot is claimed by one 64-bit atomicCAS on its key (a relaxed load first: a
//                 key, once set, never changes, so a non-empty value read is final).  At most capacity probes.
//   find_slot     the same walk, reading only: stops at the key or at the first empty slot.  At most capacity probes.
//   bounds_body   per-axis fp32 minimum over a workgroup's points: wave shuffles, LDS across the four waves, one integer atomicMin
//                 per workgroup and axis on the order-preserving image of the float; flag bit 0 for |coordinate| > 256
//   tile_scan     exclusive prefix sum of one int per thread across a 256-thread workgroup, and the workgroup's total
// Every table index is masked by capacity - 1.
#pragma once
#include <climits>
#include <cmath>

#include "epn_common.h"

namespace epn_cells {

constexpr int VT = 256;                  // threads per workgroup = entries per scan tile
constexpr int VW = VT / 64;              // waves
constexpr int64_t MAX_N = 1 << 22;
constexpr double INDEX_END = 2097152.0;  // 2^21: indices are 0 .. 2^21 - 1
constexpr unsigned long long EMPTY = ~0ull;
constexpr unsigned long long HASH = 0x9E3779B97F4A7C15ull;
constexpr unsigned FLAG_COORD = 1u, FLAG_INDEX = 2u, FLAG_TABLE = 4u;

struct Head {                            // the workspace's first 64 bytes
    unsigned lo[3];                      // order-preserving image of the fp32 minima
    unsigned flags;
    unsigned pad[12];
};

// capacity = the smallest power of two >= max(2n, 128)
inline int log2_capacity(int64_t n) {
    int l = 7;
    while (((int64_t)1 << l) < 2 * n) ++l;
    return l;
}

// floats order like these unsigned integers (-0 below +0, which changes no cell index)
__device__ __forceinline__ unsigned ordered(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unordered(unsigned u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}

// a point's coordinates, and whether it is kept (all three finite)
__device__ __forceinline__ bool load_point(const float *__restrict__ pc, int i, float &x, float &y, float &z) {
    x = pc[3 * (size_t)i];
    y = pc[3 * (size_t)i + 1];
    z = pc[3 * (size_t)i + 2];
    return isfinite(x) && isfinite(y) && isfinite(z);
}

__device__ __forceinline__ bool too_far(float x, float y, float z) {
    return fmaxf(fmaxf(fabsf(x), fabsf(y)), fabsf(z)) > 256.0f;
}

__device__ __forceinline__ void init_head(Head *head) {
    head->lo[0] = head->lo[1] = head->lo[2] = ordered(INFINITY);
    head->flags = 0u;
}

__device__ __forceinline__ double cell_axis(float x, unsigned lo, double edge) {
    return floor(((double)x - ((double)unordered(lo) - 0.5 * edge)) / edge);
}

__device__ __forceinline__ unsigned long long cell_key(double ix, double iy, double iz) {
    return ((unsigned long long)ix << 42) | ((unsigned long long)iy << 21) | (unsigned long long)iz;
}

__device__ __forceinline__ unsigned home_slot(unsigned long long key, int log2cap) {
    return (unsigned)((key * HASH) >> (64 - log2cap));
}

// Slot: any struct whose member `key` is an unsigned long long.  -1: the table is full (a load factor <= 1/2 excludes it).
template <class Slot>
__device__ __forceinline__ int claim_slot(Slot *slots, unsigned long long key, int log2cap) {
    const unsigned mask = (1u << log2cap) - 1u;
    unsigned s = home_slot(key, log2cap);
    for (unsigned probe = 0; probe <= mask; ++probe, s = (s + 1u) & mask) {
        unsigned long long k = __hip_atomic_load(&slots[s].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == EMPTY) k = atomicCAS(&slots[s].key, EMPTY, key);
        if (k == EMPTY || k == key) return (int)s;
    }
    return -1;
}

// the finished table, read only.  -1: no slot holds the key.
template <class Slot>
__device__ __forceinline__ int find_slot(const Slot *__restrict__ slots, unsigned long long key, int log2cap) {
    const unsigned mask = (1u << log2cap) - 1u;
    unsigned s = home_slot(key, log2cap);
    for (unsigned probe = 0; probe <= mask; ++probe, s = (s + 1u) & mask) {
        const unsigned long long k = slots[s].key;
        if (k == key) return (int)s;
        if (k == EMPTY) return -1;
    }
    return -1;
}

// Every thread of a VT-thread workgroup calls it: (x, y, z) = its kept point, +inf without one; far = that point is too_far.
__device__ __forceinline__ void bounds_body(float x, float y, float z, int far, Head *head) {
    __shared__ float wmin[VW][3];
    __shared__ int wfar[VW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        x = fminf(x, __shfl_xor(x, s, 64));
        y = fminf(y, __shfl_xor(y, s, 64));
        z = fminf(z, __shfl_xor(z, s, 64));
        far |= __shfl_xor(far, s, 64);
    }
    if (lane == 0) { wmin[wave][0] = x; wmin[wave][1] = y; wmin[wave][2] = z; wfar[wave] = far; }
    __syncthreads();
    if (tid < 3) {
        float m = wmin[0][tid];
#pragma unroll
        for (int w = 1; w < VW; ++w) m = fminf(m, wmin[w][tid]);
        if (m < INFINITY) atomicMin(&head->lo[tid], ordered(m));
    }
    if (tid == 3) {
        int f = 0;
#pragma unroll
        for (int w = 0; w < VW; ++w) f |= wfar[w];
        if (f) atomicOr(&head->flags, FLAG_COORD);
    }
}

// Every thread of a VT-thread workgroup calls it with its v; returns the sum of the v of the threads below it, total = the
// workgroup's sum.  wsum: VW ints of LDS, free to be rewritten once every thread has returned AND passed a barrier.
__device__ __forceinline__ int tile_scan(int v, int *wsum, int &total) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int incl = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const int up = __shfl_up(incl, s, 64);
        if (lane >= s) incl += up;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < VW; ++w) {
        before += w < wave ? wsum[w] : 0;
        total += wsum[w];
    }
    return before + incl - v;
}

// ONE workgroup: sums[0..nb) -> exclusive prefix sums in place, VT entries per pass with a running carry; returns the total
// (the same value in every thread).
__device__ __forceinline__ int scan_sums(int *sums, int nb) {
    __shared__ int wsum[VW];
    const int tid = threadIdx.x;
    int carry = 0;
    for (int base = 0; base < nb; base += VT) {
        const int e = base + tid;
        int total;
        const int excl = tile_scan(e < nb ? sums[e] : 0, wsum, total);
        if (e < nb) sums[e] = carry + excl;
        carry += total;
        __syncthreads();                                   // wsum is rewritten by the next pass
    }
    return carry;
}

}  // namespace epn_cells
