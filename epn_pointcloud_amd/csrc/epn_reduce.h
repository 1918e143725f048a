// Fixed-order reductions shared by the stage kernels.  The stages promise bitwise repeatable results because their sums run in
// one order; that order is stated here, once, and is the contract of these functions.
#pragma once
#include "epn_common.h"

// Sum over the 64 lanes of a wave by an xor butterfly: step s = 32, 16, .. 1 adds the value of lane ^ s.  Lanes i and i ^ s add
// the same two values and fp addition commutes, so every lane ends with the same bits.
__device__ __forceinline__ double epn_wave_sum(double x) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) x += __shfl_xor(x, s, 64);
    return x;
}

// The same butterfly with fmax: the maximum over the wave in every lane.
__device__ __forceinline__ double epn_wave_max(double x) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) x = fmax(x, __shfl_xor(x, s, 64));
    return x;
}

// The same butterfly on integers (int, long long, their unsigned forms): sum, minimum and maximum over the wave in every lane.
// Integer addition is exact, so these do not depend on the order at all.
template <typename I>
__device__ __forceinline__ I epn_wave_isum(I x) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) x += __shfl_xor(x, s, 64);
    return x;
}
template <typename I>
__device__ __forceinline__ I epn_wave_imin(I x) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const I o = __shfl_xor(x, s, 64);
        x = o < x ? o : x;
    }
    return x;
}
template <typename I>
__device__ __forceinline__ I epn_wave_imax(I x) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const I o = __shfl_xor(x, s, 64);
        x = o > x ? o : x;
    }
    return x;
}

// Sum over a workgroup of T threads (one dimension, T a power of two) through buf[T] in LDS: every thread stores its value, then
// level s = T / 2, T / 4, .. 1 adds buf[tid + s] into buf[tid] for tid < s, with a barrier per level; the result is buf[0], the
// same bits in every thread.  The barrier in front of the store lets the same buf serve one sum after another.
template <int T, typename V>
__device__ __forceinline__ V epn_block_sum(V x, V *buf) {
    static_assert(T > 0 && (T & (T - 1)) == 0, "the halving tree needs a power-of-two workgroup");
    const int tid = threadIdx.x;
    __syncthreads();
    buf[tid] = x;
    __syncthreads();
    for (int s = T / 2; s > 0; s >>= 1) {
        if (tid < s) buf[tid] += buf[tid + s];
        __syncthreads();
    }
    return buf[0];
}
