// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants), the
// library's one counter-based generator: the dropout masks of the block glue (glue.hip) and the sampling keys of the patch
// extraction (patch_extract.hip).  tests/philox_ref.py restates it in numpy.
#pragma once
#include <hip/hip_runtime.h>

namespace epn {
namespace philox {

struct u32x4 { unsigned w[4]; };
__device__ __forceinline__ u32x4 philox4x32_10(unsigned long long ctr_lo, unsigned long long ctr_hi, unsigned long long key) {
    unsigned c0 = (unsigned)ctr_lo, c1 = (unsigned)(ctr_lo >> 32), c2 = (unsigned)ctr_hi, c3 = (unsigned)(ctr_hi >> 32);
    unsigned k0 = (unsigned)key, k1 = (unsigned)(key >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const unsigned h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1;
        c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return u32x4{{c0, c1, c2, c3}};
}

}  // namespace philox
}  // namespace epn
