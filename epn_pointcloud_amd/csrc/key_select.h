// "The n_sample members smallest in (key, i), written in ascending i" inside ONE 256-thread workgroup: the parts that
// patch_extract.hip (members = the points within a radius) and modelnet_batch.hip (members = every point of a cloud) share.
//   key_of       key(i) = word0(Philox4x32-10(ctr_lo = i, ctr_hi = Q, key = seed)) >> (32 - key_bits)
//   search_hist  the bucket of a 2048-bin LDS histogram that holds the `need`-th smallest member: three levels of it (11 + 11 + 10
//                key bits) give the exact threshold key T and the number of key == T members to take (the lowest i win)
//   emit_step    one chunk of 256 consecutive indices of the ordered compaction: 64-bit ballot + popcount inside a wave, one LDS
//                exchange (one barrier, two slot sets) across the four waves, a running base across chunks; key == T members
//                are admitted while their rank among the ties is below `take`
// The callers keep their own sweeps (what a member is, and what is written for a selected one, differs between them); the
// radius sweep has two callers of its own and lives in patch_sweep.h (patch_extract.hip, pair_batch.hip).
#pragma once
#include "epn_common.h"
#include "philox.h"

namespace epn_keysel {

constexpr int PT = 256;            // threads per workgroup
constexpr int PW = PT / 64;        // waves
constexpr int PBINS = 2048;        // histogram bins: 11 + 11 + 10 key bits over the three levels
constexpr int PBT = PBINS / PT;    // bins a thread owns in the search

struct Shared {
    unsigned hist[PBINS];
    unsigned wsum[PW];
    unsigned found[2];             // (bucket, members still to take inside it)
    unsigned slots[2][PW][2];      // emit: (selected below T, ties) per wave, two sets -> one barrier per chunk
};

__device__ __forceinline__ unsigned key_of(unsigned i, unsigned long long Q, unsigned long long seed, int key_bits) {
    return epn::philox::philox4x32_10((unsigned long long)i, Q, seed).w[0] >> (32 - key_bits);
}

__device__ __forceinline__ void clear_hist(Shared &sh) {
    for (int b = threadIdx.x; b < PBINS; b += PT) sh.hist[b] = 0u;
}

// The histogram's total and, when 1 <= need <= total, the bucket B with below(B) < need <= below(B) + hist[B] and
// need - below(B).  Every thread calls it (barriers inside) and gets the same three values.
__device__ __forceinline__ unsigned search_hist(Shared &sh, unsigned need, unsigned &bucket, unsigned &rest) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __syncthreads();                                   // the pass's LDS atomics are done
    unsigned h[PBT], own = 0u;
#pragma unroll
    for (int b = 0; b < PBT; ++b) { h[b] = sh.hist[PBT * tid + b]; own += h[b]; }
    unsigned incl = own;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const unsigned o = __shfl_up(incl, s, 64);
        incl += lane >= s ? o : 0u;
    }
    if (lane == 63) sh.wsum[wave] = incl;
    if (tid == 0) { sh.found[0] = 0u; sh.found[1] = 0u; }
    __syncthreads();
    unsigned below = incl - own, total = 0u;
#pragma unroll
    for (int w = 0; w < PW; ++w) {
        below += w < wave ? sh.wsum[w] : 0u;
        total += sh.wsum[w];
    }
    if (below < need && need <= below + own) {         // exactly one thread when 1 <= need <= total
#pragma unroll
        for (int b = 0; b < PBT; ++b) {
            if (below < need && need <= below + h[b]) { sh.found[0] = (unsigned)(PBT * tid + b); sh.found[1] = need - below; }
            below += h[b];
        }
    }
    __syncthreads();
    bucket = sh.found[0];
    rest = sh.found[1];
    __syncthreads();                                   // found / wsum / hist may be rewritten by the caller
    return total;
}

// The running state of the ordered compaction across a sweep's chunks.
struct Emit {
    unsigned out_base = 0u, tie_base = 0u;             // members written / ties seen in the chunks so far
    int set = 0;
};

// One chunk: this lane's index has key < T (`less`) or key == T (`tie`), or is no member (neither).  Every thread of the
// workgroup calls it once per chunk (one barrier inside).  -> whether the lane's index is selected, and its output slot `pos`
// (the caller still checks pos < n_sample).
__device__ __forceinline__ bool emit_step(Shared &sh, Emit &e, bool less, bool tie, unsigned take, unsigned &pos) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below_lane = (1ull << lane) - 1ull;
    const unsigned long long mless = __ballot(less), mtie = __ballot(tie);
    if (lane == 0) { sh.slots[e.set][wave][0] = (unsigned)__popcll(mless); sh.slots[e.set][wave][1] = (unsigned)__popcll(mtie); }
    __syncthreads();
    unsigned less_before = 0u, ties_before = 0u, less_all = 0u, ties_all = 0u;
#pragma unroll
    for (int w = 0; w < PW; ++w) {
        const unsigned a = sh.slots[e.set][w][0], b = sh.slots[e.set][w][1];
        less_before += w < wave ? a : 0u;
        ties_before += w < wave ? b : 0u;
        less_all += a;
        ties_all += b;
    }
    // ties admitted so far (earlier chunks: tie_base of them, capped by take) and in this chunk's earlier waves
    const unsigned room = take > e.tie_base ? take - e.tie_base : 0u;            // ties this chunk may still admit
    const unsigned adm_before = ties_before < room ? ties_before : room;
    const unsigned rank = ties_before + (unsigned)__popcll(mtie & below_lane);   // among this chunk's ties
    const bool sel = less || (tie && rank < room);
    const unsigned long long msel = __ballot(sel);
    pos = e.out_base + less_before + adm_before + (unsigned)__popcll(msel & below_lane);
    e.out_base += less_all + (ties_all < room ? ties_all : room);
    e.tie_base += ties_all;
    e.set ^= 1;
    return sel;
}

}  // namespace epn_keysel
