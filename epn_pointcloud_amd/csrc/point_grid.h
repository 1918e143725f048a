// What the kernels that QUERY a point grid share (point_grid.hip: the nearest point; point_normals.hip: the neighbourhood of a
// plane fit): the workspace's layout, the host's memory of the builds, the fp32 distance rule and the walk over the 27 cells
// around a query.  The build itself is point_grid.hip's; the cell rule and the hash table are cell_hash.h's.
#pragma once
#include "cell_hash.h"

namespace epn_grid {

using namespace epn_cells;

constexpr int QW = 4;                    // queries (waves) per workgroup
constexpr unsigned long long NONE = ~0ull;

struct Slot {                            // 16 bytes: one cell
    unsigned long long key;
    int count;                           // its points
    int cursor;                          // offsets: the start of its run; after scatter: the end
};

struct Layout {
    int log2cap;
    size_t cap, records, slots, pslot, tsum, bytes;   // byte offsets of the records, the table, the points' slots, the tile sums
};

inline Layout layout(int64_t n) {
    Layout L;
    L.log2cap = log2_capacity(n);
    L.cap = (size_t)1 << L.log2cap;
    L.records = sizeof(Head);
    L.slots = L.records + (size_t)n * sizeof(int4);
    L.pslot = L.slots + L.cap * sizeof(Slot);
    L.tsum = L.pslot + (size_t)n * sizeof(int);
    L.bytes = L.tsum + (size_t)epn_cdiv((long long)L.cap, VT) * sizeof(int);
    return L;
}

inline double cell_edge(double max_radius) { return max_radius * (1.0 + 0x1p-10); }

// What a query's argument checks need of the build, kept on the host per workspace address (point_grid.hip).
struct Built {
    int64_t n;
    double max_radius;
};
bool recall(const void *workspace, Built &b);

// (dx*dx + dy*dy) + dz*dz, every operation rounded on its own.  Plain operators under "fp contract(off)": the pragma governs the
// operations written in its scope, and the __f*_rn intrinsics are inline functions of the HIP headers, compiled outside it, whose
// products this compiler fuses into fma.
__device__ __forceinline__ float dist2(float px, float py, float pz, float qx, float qy, float qz) {
#pragma clang fp contract(off)
    const float dx = px - qx, dy = py - qy, dz = pz - qz;
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const float xy = xx + yy;
    return xy + zz;
}

// The candidates of one query, numbered 0..total-1 across the wave: lane l < 27 holds the run (start, count) of the cell moved by
// (l % 3 - 1, l / 3 % 3 - 1, l / 9 - 1) from the query's and the number `first` of its first candidate.
struct Cells {
    int start, count, first, total;
};

// Every lane of the wave calls it, with a finite query and n > 0.  An index outside [0, 2^21) on an axis (far queries included: the
// comparison is made in fp64, before any conversion) holds no point.  The run ends are clamped to [0, n] on reading.
__device__ __forceinline__ Cells find_cells(const Head *__restrict__ head, const Slot *__restrict__ slots, int n, int log2cap,
                                            double edge, float qx, float qy, float qz, int lane) {
    const int c = lane < 27 ? lane : 13;
    const double ix = cell_axis(qx, head->lo[0], edge) + (double)(c % 3 - 1);
    const double iy = cell_axis(qy, head->lo[1], edge) + (double)(c / 3 % 3 - 1);
    const double iz = cell_axis(qz, head->lo[2], edge) + (double)(c / 9 - 1);
    Cells r;
    r.start = 0;
    r.count = 0;
    if (lane < 27 && ix >= 0.0 && ix < INDEX_END && iy >= 0.0 && iy < INDEX_END && iz >= 0.0 && iz < INDEX_END) {
        const int s = find_slot(slots, cell_key(ix, iy, iz), log2cap);
        if (s >= 0) {
            const int end = min(max(slots[s].cursor, 0), n);
            r.count = min(max(slots[s].count, 0), end);
            r.start = end - r.count;
        }
    }
    int incl = r.count;                                    // lanes 27..63 add nothing: five steps cover lanes 0..31
#pragma unroll
    for (int s = 1; s < 32; s <<= 1) {
        const int up = __shfl_up(incl, s, 64);
        if (lane >= s) incl += up;
    }
    r.first = incl - r.count;
    r.total = __shfl(incl, 31, 64);
    return r;
}

// Every lane of the wave calls it (the shuffles read all of them): the record index of candidate t, -1 when t >= total or the
// index is outside [0, n).  A five-step search of the prefix sums finds the last cell whose first candidate is <= t.
__device__ __forceinline__ int record_of(const Cells &c, int t, int n) {
    int cell = 0;
#pragma unroll
    for (int step = 16; step > 0; step >>= 1) {
        const int f = __shfl(c.first, cell + step, 64);
        if (cell + step < 27 && f <= t) cell += step;
    }
    const int at = __shfl(c.start, cell, 64) + (t - __shfl(c.first, cell, 64));
    return t < c.total && at >= 0 && at < n ? at : -1;
}

// d2 bits << 32 | row: d2 >= 0, so its bits order like its value; the lowest row wins a tie
__device__ __forceinline__ unsigned long long member_key(float d2, int row) {
    return ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)row;
}

// The answer of epn_point_grid_nn_f32 for the wave's query (qx, qy, qz), the same in every lane: key = the smallest member key
// among the grid's points with d2 <= r2 (NONE without one, and for a non-finite query or n == 0, which read nothing of the
// grid), and the winner's coordinates as its record holds them.  exclude_row skips the candidate whose row is q.  Every lane of
// the wave calls it.  A kernel that does not use the coordinates pays nothing for them.
struct Nearest {
    unsigned long long key;
    float x, y, z;
};

__device__ __forceinline__ Nearest nearest_member(const Head *__restrict__ head, const Slot *__restrict__ slots,
                                                  const int4 *__restrict__ records, int n, int log2cap, double edge, float qx,
                                                  float qy, float qz, float r2, int exclude_row, int q, int lane) {
    Nearest best;
    best.key = NONE;
    best.x = best.y = best.z = 0.0f;
    if (n > 0 && isfinite(qx) && isfinite(qy) && isfinite(qz)) {
        const Cells cells = find_cells(head, slots, n, log2cap, edge, qx, qy, qz, lane);
        for (int base = 0; base < cells.total; base += 64) {   // every lane runs every pass: the shuffles read all of them
            const int at = record_of(cells, base + lane, n);
            if (at >= 0) {
                const int4 p = records[at];
                const int row = p.w;
                const float px = __int_as_float(p.x), py = __int_as_float(p.y), pz = __int_as_float(p.z);
                const float d2 = dist2(px, py, pz, qx, qy, qz);
                if (d2 <= r2 && !(exclude_row && row == q)) {
                    const unsigned long long k = member_key(d2, row);
                    if (k < best.key) {
                        best.key = k;
                        best.x = px; best.y = py; best.z = pz;
                    }
                }
            }
        }
        unsigned long long low = best.key;
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            const unsigned long long o = __shfl_xor(low, s, 64);
            low = o < low ? o : low;
        }
        // a row occurs once in the grid, so one lane holds the winning key: the lowest such lane hands its coordinates out
        const unsigned long long holders = __ballot(best.key == low && low != NONE);
        const int owner = holders ? __ffsll((long long)holders) - 1 : 0;
        best.key = low;
        best.x = __shfl(best.x, owner, 64);
        best.y = __shfl(best.y, owner, 64);
        best.z = __shfl(best.z, owner, 64);
    }
    return best;
}

}  // namespace epn_grid
