// Weight gradients of BasicSO3Conv as hand-written MFMA GEMMs for gfx950 (the TN half of what gemm.hip's header describes):
//
//   TN   C[N1][N2] = X[R][N1]^T . Y[R][N2]     dW = dOut^T G (contraction over the R = b*p*a columns)
//
// Four kernel families, every instance of which is named ONCE in the EPN_TN_*_INSTANCES tables below: fp32 operands (native
// fp32 MFMA or split in the kernel into three bf16 / two fp16 pieces), fp32 operands with X pre-split into planes, bf16
// operands (two LDS stages), bf16 operands (ring of stages).  A launch writes split partial slabs that a fixed-order
// reduction sums.  tn_plan() chooses family, tile and splits for the launcher AND the workspace query.
#include "conv_internal.h"
#include "gemm.h"

namespace epn {
namespace {
EPN_F2_SENTINEL_DECL

// ------------------------------------------------------------------------------------------------ TN (fp32)
// C[N1][N2] (+ split partials) = sum_r X[r][n1] Y[r][n2].  Block tile BN1 x BN2 = (WGM*TM*32) x (WGN*TN*32); stage =
// BR rows of both operands, row-contiguous in LDS.  MFMA tile tm of a wave covers rows n1 = base + TM*i + tm (i = MFMA
// row) so that ONE ds_read of TM floats at [r][base + TM*i] serves all TM tiles (likewise columns): output rows are a
// permutation the epilogue undoes.
// Split form (X3, see gemm_x3.hip): fp32 operands split without loss into three bf16 pieces in registers, six
// v_mfma_f32_32x32x16_bf16 per 32x32x16 block instead of eight v_mfma_f32_32x32x2_f32 -- fp32 accuracy at 2.7x the rate.

// X3: both operands split in registers (the narrow / grouped problems, where a separate splitting pass over X would cost
// as much as the GEMM); the wide weight gradients run on gemm_tn_x3_kernel below.
#ifndef EPN_TN_GROUP_TARGET_BF16
#define EPN_TN_GROUP_TARGET_BF16 768
#endif
#ifndef EPN_TN_GROUP_TARGET_F32
#define EPN_TN_GROUP_TARGET_F32 1024
#endif
#ifndef EPN_TN_SINGLE_TARGET_BF16
#define EPN_TN_SINGLE_TARGET_BF16 512
#endif
// Image of the staged rows of the bf16 weight-gradient kernels (round 6).  A 16-lane group of `ds_read_b64_tr_b16` reads four
// consecutive rows of a 16-column tile (32 bytes each); the instruction is serviced in two 32-lane groups, i.e. eight rows
// ({r .. r+3} of two lane groups 8 rows apart) at once, and the bank of a byte is (a / 4) mod 64.  In the linear image of
// the 128 x 256 tile a row is 768 bytes = 3 x 256: all eight rows start on bank 0 and the 64 chunks of a wave queue on 8
// banks -- SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE 0.75-0.88 in rounds 3-5's PMC files (review, round 5).  1: the 16-byte
// slots of row r are XOR-ed with 2 rho(r), rho = (r & 3) | ((r >> 3) & 1) << 2 -- applied to the SOURCE address of the
// direct-to-LDS loads (their LDS side is lane-linear), so the eight rows of a group land on eight different 32-byte windows
// of the 256-byte bank row.  Needs operand regions that are multiples of 16 slots (128 columns): the 128 x 256 tiles;
// narrower tiles keep the linear image (tools/lds_tr_probe.hip measures the candidates).
#ifndef EPN_TN_SWZ
#define EPN_TN_SWZ 1
#endif
__device__ __forceinline__ int tn_row_swz(int r) { return 2 * ((r & 3) | (((r >> 3) & 1) << 2)); }
// column (bf16 index inside the staged row) where the swizzled image keeps logical column `col` of row r; rows r and r + 4
// share the mask (bit 2 of r is not used), so the second read of a fragment keeps its fixed row offset
template <bool SWZ>
__device__ __forceinline__ int tn_swz_col(int col, int r) {
    if constexpr (!SWZ) return col;
    return (((col >> 3) ^ tn_row_swz(r)) << 3) | (col & 7);
}
#ifndef EPN_TN_WIDE_NSTG
#define EPN_TN_WIDE_NSTG 3
#endif
#ifndef EPN_TN_NARROW_NSTG
#define EPN_TN_NARROW_NSTG 4
#endif
#ifndef EPN_TN_NARROW_STAGE_KB  // stage size aimed at (a stage = a power-of-two number of 32-row contraction steps)
#define EPN_TN_NARROW_STAGE_KB 32
#endif
constexpr int tn_ring_kr(int wgm, int wgn, int tm, int tn) {
    const int step_b = 32 * 2 * 16 * (wgm * tm + wgn * tn);      // bytes of one 32-row step of [BN1 + BN2] bf16
    int kr = 1;
    while (2 * kr * step_b <= EPN_TN_NARROW_STAGE_KB * 1024 && 2 * kr * step_b * EPN_TN_NARROW_NSTG <= 160 * 1024) kr *= 2;
    return kr;
}
#ifndef EPN_TN_NARROW_WGS       // resident workgroups per CU the split count aims at
#define EPN_TN_NARROW_WGS 1
#endif
// Workgroup -> (tile, split) of a TN problem.  Launch order is split-major (all tiles of one K range, then the next
// range); every tile row streams the whole Y panel and every tile column the whole X panel, so the tiles of ONE K range
// running on ONE XCD read each operand row once from HBM and again from that XCD's L2.  Workgroup b runs on XCD b % 8:
// the bijective remap of epn_common.h hands every XCD a contiguous run of that order (a problem's first workgroup is a
// multiple of 8, tn_plan).  Placement only: the partial slabs and their fixed-order reduction are unchanged.
__device__ __forceinline__ unsigned tn_tile_of(unsigned lb, unsigned ntiles, unsigned nsplit) {
    return epn_xcd_tile(lb, (ntiles * nsplit + 7u) & ~7u);
}

// Fragment reads: W = 1 / 2 / 4 consecutive floats of a staged row in ONE LDS read (the W MFMA tiles of a wave interleave
// their rows / columns: one read serves them all), into column k of v[W][K] or into v[W]
template <int W, int K>
__device__ __forceinline__ void tn_frag_k(const char *p, float (&v)[W][K], int k) {
    static_assert(W == 1 || W == 2 || W == 4, "fragment width");
    if constexpr (W == 4) {
        const f32x4 q = *reinterpret_cast<const f32x4 *>(p);
        v[0][k] = q[0]; v[1][k] = q[1]; v[2][k] = q[2]; v[3][k] = q[3];
    } else if constexpr (W == 2) {
        const f32x2 q = *reinterpret_cast<const f32x2 *>(p);
        v[0][k] = q[0]; v[1][k] = q[1];
    } else {
        v[0][k] = *reinterpret_cast<const float *>(p);
    }
}
template <int W>
__device__ __forceinline__ void tn_frag(const char *p, float (&v)[W]) {
    static_assert(W == 1 || W == 2 || W == 4, "fragment width");
    if constexpr (W == 4) {
        const f32x4 q = *reinterpret_cast<const f32x4 *>(p);
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
    } else if constexpr (W == 2) {
        const f32x2 q = *reinterpret_cast<const f32x2 *>(p);
        v[0] = q[0]; v[1] = q[1];
    } else {
        v[0] = *reinterpret_cast<const float *>(p);
    }
}

template <int WGM, int WGN, int TM, int TN, int BR, int X3 = 0>     // X3: 0 = fp32 MFMA, 3 = three bf16 pieces, 2 = two fp16 pieces
__global__ __launch_bounds__(64 * WGM * WGN) void gemm_tn_f32_kernel(GemmTnBatch B) {
    constexpr int NW = WGM * WGN;
    constexpr int BN1 = WGM * TM * 32, BN2 = WGN * TN * 32;
    constexpr int ROWF = BN1 + BN2;                 // floats per staged row (X part, then Y part)
    constexpr int STAGE_B = BR * ROWF * 4;
    constexpr int NI = STAGE_B / 1024;              // wave-level 1 KiB load instructions per stage
    constexpr int IPW = (NI + NW - 1) / NW;
    static_assert(STAGE_B % 1024 == 0, "stage must be a whole number of 1 KiB pieces");
    __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE_B];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int pi = 0;
#pragma unroll
    for (int i = 1; i < GEMM_MAX_PROB; ++i)
        if (i < B.nprob && blockIdx.x >= B.p[i].block0) pi = i;
    const GemmTnArgs &G = B.p[pi];
    const unsigned tile = tn_tile_of(blockIdx.x - G.block0, G.ntiles, (unsigned)G.nsplit) % G.ntiles;
    const unsigned split = tn_tile_of(blockIdx.x - G.block0, G.ntiles, (unsigned)G.nsplit) / G.ntiles;
    if (split >= (unsigned)G.nsplit) return;           // padding workgroup of a grouped launch (uniform per workgroup)
    const int n1_0 = (int)(tile / G.tiles_n2) * BN1, n2_0 = (int)(tile % G.tiles_n2) * BN2;
    const long long nchunk = G.R / BR;
    const long long c0 = nchunk * split / G.nsplit, c1 = nchunk * (split + 1) / G.nsplit;
    const int nk = (int)(c1 - c0);
    const float *__restrict__ X = static_cast<const float *>(G.X);
    const float *__restrict__ Y = static_cast<const float *>(G.Y);

    // piece q (1 KiB = 256 floats) of a stage: float offset 256 q + 4 lane -> (row, col) of the [BR][ROWF] image
    const float *src[IPW];
    long long sstep[IPW];
#pragma unroll
    for (int i = 0; i < IPW; ++i) {
        const int q = wave + i * NW;
        const int fo = 256 * q + 4 * lane;
        const int r = fo / ROWF, c = fo % ROWF;
        if (c < BN1) {
            int n = n1_0 + c;
            n = n < G.N1 - 4 ? n : G.N1 - 4;
            src[i] = X + (c0 * BR + r) * G.ldx + n;
            sstep[i] = (long long)BR * G.ldx;
        } else {
            int n = n2_0 + (c - BN1);
            n = n < G.N2 - 4 ? n : G.N2 - 4;
            src[i] = Y + (c0 * BR + r) * G.ldy + n;
            sstep[i] = (long long)BR * G.ldy;
        }
    }
    auto stage_one = [&](int buf, int i) {
        const int q = wave + i * NW;
        if (NI % NW == 0 || q < NI) {
            glds16(src[i], smem + buf * STAGE_B + q * 1024);
            src[i] += sstep[i];
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int i = 0; i < IPW; ++i) stage_one(buf, i);
    };
    const int wpar = NW == 8 ? __builtin_amdgcn_readfirstlane(wave >> 2) : 0;   // SIMD partner parity (gemm_nt_kernel)

    const int wm = wave / WGN, wn = wave % WGN;
    const int li = lane & 31, lj = lane >> 5;
    const int xo = (wm * TM * 32 + TM * li) * 4;                 // byte offset inside a staged row
    const int yo = (BN1 + wn * TN * 32 + TN * li) * 4;
    float x_scale = 1.0f, y_scale = 1.0f;                        // two-piece form: powers of two from the device maxima
    if constexpr (X3 == 2) { x_scale = f2_scale_of(*G.x_amax); y_scale = f2_scale_of(*G.y_amax); }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    if (nk > 0) stage(0);
    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();
        const char *base = smem + (kt & 1) * STAGE_B;
        const bool more = kt + 1 < nk;
        if constexpr (X3 != 0) {
            if (more) stage((kt + 1) & 1);
#pragma unroll
            for (int s = 0; s < BR / 16; ++s) {     // 16 rows per fragment step: lane group lj holds rows 8 lj .. 8 lj + 7
                float xa[TM][8], yb[TN][8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const char *row = base + (16 * s + 8 * lj + k) * (ROWF * 4);
                    tn_frag_k<TM>(row + xo, xa, k);
                    tn_frag_k<TN>(row + yo, yb, k);
                }
                if constexpr (X3 == 3) {
                bf16x8 ah[TM], am[TM], al[TM], bh[TN], bm[TN], bl[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) split3(xa[i], ah[i], am[i], al[i]);
#pragma unroll
                for (int j = 0; j < TN; ++j) split3(yb[j], bh[j], bm[j], bl[j]);
                x3_terms(acc, ah, am, al, bh, bm, bl);
                } else {
                gemm_f16x8 ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) f2_split8(xa[i], x_scale, ah[i], al[i]);
#pragma unroll
                for (int j = 0; j < TN; ++j) f2_split8(yb[j], y_scale, bh[j], bl[j]);
                f2_terms(acc, ah, al, bh, bl);
                }
            }
            continue;
        }
        // fragments of k-pair s+1 are read while the MFMAs of pair s issue (two register sets, static indices)
        float a[2][TM], b[2][TN];
        auto rd = [&](int s, int set) {
            const char *row = base + (2 * s + lj) * (ROWF * 4);
            tn_frag<TM>(row + xo, a[set]);
            tn_frag<TN>(row + yo, b[set]);
        };
        rd(0, 0);
#pragma unroll
        for (int s = 0; s < BR / 2; ++s) {
            if (s + 1 < BR / 2) rd(s + 1, (s + 1) & 1);
            __builtin_amdgcn_sched_barrier(0);
            if (more) {                         // next stage's loads spread over the step (see gemm_nt_kernel)
                constexpr int NGRP = BR / 2;
#pragma unroll
                for (int i = 0; i < IPW; ++i) {
                    const int g0 = (i * (NGRP - 1)) / IPW;
                    const int g1 = g0 + 1 < NGRP ? g0 + 1 : NGRP - 1;
                    if ((g0 == s && wpar == 0) || (g1 == s && wpar != 0)) stage_one((kt + 1) & 1, i);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s & 1][i], b[s & 1][j], acc[i][j], 0, 0, 0);
        }
    }

    // ---- epilogue: MFMA row ri of tile tm = output row base1 + TM*ri + tm; column li of tile tn = base2 + TN*li + tn
    if constexpr (X3 == 2) {
        const float ux = f2_inverse(x_scale), uy = f2_inverse(y_scale);
        EPN_F2_CHECK(f2_unscale(acc, ux, uy));
    }
    float *__restrict__ C = G.nsplit > 1 ? static_cast<float *>(G.part) + (size_t)split * G.N1 * G.N2
                                         : static_cast<float *>(G.C);
    const long long ldc = G.nsplit > 1 ? G.N2 : G.ldc;
    if (n1_0 + BN1 <= G.N1 && n2_0 + BN2 <= G.N2 && (long long)BN1 * ldc < (1LL << 30)) {
        // interior tile: wave-uniform base + 32-bit lane offset (see gemm_nt_kernel's epilogue)
        float *__restrict__ cw = C + (size_t)(n1_0 + wm * TM * 32) * ldc + (n2_0 + wn * TN * 32);
        const unsigned ld = (unsigned)ldc;
        const unsigned lane_off = (unsigned)(TM * 4 * lj) * ld + TN * li;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const unsigned o = lane_off + (unsigned)(TM * ((r & 3) + 8 * (r >> 2)) + i) * ld;
#pragma unroll
                for (int j = 0; j < TN; ++j) cw[o + j] = acc[i][j][r];
            }
        return;
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ri = (r & 3) + 8 * (r >> 2) + 4 * lj;
            const int n1 = n1_0 + wm * TM * 32 + TM * ri + i;
            const int n2 = n2_0 + wn * TN * 32 + TN * li;
            if (n1 < G.N1) {
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    if (n2 + j < G.N2) C[(long long)n1 * ldc + n2 + j] = acc[i][j][r];
            }
        }
}

// ------------------------------------------------------------------------------------------------ TN (fp32, split form)
// Split form with the NARROW operand X (the output gradient: N1 = cout columns, a few % of the bytes of Y) split ahead of
// the GEMM by split_octets_kernel into three bf16 planes laid out [plane][R/8][N1][8]: the eight contraction values a
// lane needs for one output row are one 16-byte chunk, so an X fragment is ONE ds_read_b128 per plane and costs no VALU
// work; only Y (the grouped features, streamed once) is split in registers -- 36 VALU instructions per Y fragment,
// 1.5 per MFMA for a 128 x 64 wave tile instead of 4.5-6 when both operands are split in the kernel (the VALU/issue
// slots beside a 32-cycle MFMA are what bounded that form at 150 TFLOP/s).  MFMA tile i of a wave covers output rows
// base + 32 i + (MFMA row) here (contiguous chunks: conflict-free b128 reads), columns as in gemm_tn_f32_kernel.
__global__ void split_octets_kernel(const float *__restrict__ X, long long ldx, long long R, int N1, u32x4 *__restrict__ planes) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long n = (R >> 3) * N1;
    if (i >= n) return;
    const long long o = i / N1;
    const int c = (int)(i - o * N1);
    float x[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = X[(8 * o + k) * ldx + c];
    bf16x8 h, m, l;
    split3(x, h, m, l);
    planes[i] = __builtin_bit_cast(u32x4, h);
    planes[n + i] = __builtin_bit_cast(u32x4, m);
    planes[2 * n + i] = __builtin_bit_cast(u32x4, l);
}

// two-piece fp16 form: planes [2][R/8][N1][8], scaled by the power of two of max|X| (device scalar)
__global__ void split_octets2_kernel(const float *__restrict__ X, long long ldx, long long R, int N1, u32x4 *__restrict__ planes,
                                     const float *__restrict__ amax) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long n = (R >> 3) * N1;
    if (i >= n) return;
    const long long o = i / N1;
    const int c = (int)(i - o * N1);
    float x[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = X[(8 * o + k) * ldx + c];
    gemm_f16x8 h, l;
    f2_split8(x, f2_scale_of(*amax), h, l);
    planes[i] = __builtin_bit_cast(u32x4, h);
    planes[n + i] = __builtin_bit_cast(u32x4, l);
}

template <int WGM, int WGN, int TM, int TN, int BR, int NPL = 3>
__global__ __launch_bounds__(64 * WGM * WGN) void gemm_tn_x3_kernel(GemmTnBatch B) {
    constexpr int NW = WGM * WGN;
    constexpr int BN1 = WGM * TM * 32, BN2 = WGN * TN * 32;
    constexpr int OCT = BR / 8;                     // row octets per stage
    constexpr int XB = NPL * OCT * BN1 * 16;        // X planes of a stage: [plane][octet][n1] 16-byte chunks
    constexpr int YB = BR * BN2 * 4;                // Y rows (fp32)
    constexpr int STAGE_B = XB + YB;
    constexpr int NIX = XB / 1024, NI = STAGE_B / 1024;
    constexpr int IPW = (NI + NW - 1) / NW;
    static_assert(XB % 1024 == 0 && YB % 1024 == 0 && 2 * STAGE_B <= 160 * 1024, "stage");
    __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE_B];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int pi = 0;
#pragma unroll
    for (int i = 1; i < GEMM_MAX_PROB; ++i)
        if (i < B.nprob && blockIdx.x >= B.p[i].block0) pi = i;
    const GemmTnArgs &G = B.p[pi];
    const unsigned tile = tn_tile_of(blockIdx.x - G.block0, G.ntiles, (unsigned)G.nsplit) % G.ntiles;
    const unsigned split = tn_tile_of(blockIdx.x - G.block0, G.ntiles, (unsigned)G.nsplit) / G.ntiles;
    if (split >= (unsigned)G.nsplit) return;           // padding workgroup of a grouped launch (uniform per workgroup)
    const int n1_0 = (int)(tile / G.tiles_n2) * BN1, n2_0 = (int)(tile % G.tiles_n2) * BN2;
    const long long nchunk = G.R / BR;
    const long long c0 = nchunk * split / G.nsplit, c1 = nchunk * (split + 1) / G.nsplit;
    const int nk = (int)(c1 - c0);

    const char *src[IPW];
    long long sstep[IPW];
#pragma unroll
    for (int i = 0; i < IPW; ++i) {
        const int q = wave + i * NW;
        if (q < NIX) {
            const int ci = 64 * q + lane;            // chunk of the [plane][octet][n1] image
            const int c = ci % BN1, po = ci / BN1;
            const int oct = po % OCT, pl = po / OCT;
            int n = n1_0 + c;
            n = n < G.N1 ? n : G.N1 - 1;
            src[i] = static_cast<const char *>(G.Xp) + (((size_t)pl * (G.R >> 3) + (c0 * OCT + oct)) * G.N1 + n) * 16;
            sstep[i] = (long long)OCT * G.N1 * 16;
        } else {
            const int fo = 256 * (q - NIX) + 4 * lane;
            const int r = fo / BN2, c = fo % BN2;
            int n = n2_0 + c;
            n = n < G.N2 - 4 ? n : G.N2 - 4;
            src[i] = reinterpret_cast<const char *>(static_cast<const float *>(G.Y) + (c0 * BR + r) * G.ldy + n);
            sstep[i] = (long long)BR * G.ldy * 4;
        }
    }
    auto stage = [&](int buf) {
#pragma unroll
        for (int i = 0; i < IPW; ++i) {
            const int q = wave + i * NW;
            if (NI % NW == 0 || q < NI) {
                glds16(src[i], smem + buf * STAGE_B + q * 1024);
                src[i] += sstep[i];
            }
        }
    };

    const int wm = wave / WGN, wn = wave % WGN;
    const int li = lane & 31, lj = lane >> 5;
    const int xo = (wm * TM * 32 + li) * 16;                      // chunk of MFMA tile 0 inside an [octet] row of a plane
    const int yo = XB + (wn * TN * 32 + TN * li) * 4;
    float y_scale = 1.0f;
    if constexpr (NPL == 2) y_scale = f2_scale_of(*G.y_amax);

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    if (nk > 0) stage(0);
    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();
        const char *base = smem + (kt & 1) * STAGE_B;
        if (kt + 1 < nk) stage((kt + 1) & 1);
#pragma unroll
        for (int s = 0; s < BR / 16; ++s) {         // 16 rows per fragment step: lane group lj holds octet 2 s + lj
            float yb[TN][8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const char *row = base + (16 * s + 8 * lj + k) * (BN2 * 4);
                tn_frag_k<TN>(row + yo, yb, k);
            }
            if constexpr (NPL == 3) {
            bf16x8 ah[TM], am[TM], al[TM], bh[TN], bm[TN], bl[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const char *xp = base + (2 * s + lj) * (BN1 * 16) + xo + i * 512;
                ah[i] = *reinterpret_cast<const bf16x8 *>(xp);
                am[i] = *reinterpret_cast<const bf16x8 *>(xp + OCT * BN1 * 16);
                al[i] = *reinterpret_cast<const bf16x8 *>(xp + 2 * OCT * BN1 * 16);
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) split3(yb[j], bh[j], bm[j], bl[j]);
            mfma_term(acc, ah, bl);                 // small terms first (x3_terms written out: as one call it moved the
            mfma_term(acc, al, bh);                 // register allocation of the <1, 8, 2, 2, 16, 3> instance)
            mfma_term(acc, am, bm);
            mfma_term(acc, ah, bm);
            mfma_term(acc, am, bh);
            mfma_term(acc, ah, bh);
            } else {
            gemm_f16x8 ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const char *xp = base + (2 * s + lj) * (BN1 * 16) + xo + i * 512;
                ah[i] = *reinterpret_cast<const gemm_f16x8 *>(xp);
                al[i] = *reinterpret_cast<const gemm_f16x8 *>(xp + OCT * BN1 * 16);
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) f2_split8(yb[j], y_scale, bh[j], bl[j]);
            f2_terms(acc, ah, al, bh, bl);
            }
        }
    }

    if constexpr (NPL == 2) {
        const float ux = f2_inverse(f2_scale_of(*G.x_amax)), uy = f2_inverse(y_scale);
        EPN_F2_CHECK(f2_unscale(acc, ux, uy));
    }
    // ---- epilogue: MFMA row ri of tile i = output row base1 + 32 i + ri; column li of tile j = base2 + TN*li + j
    float *__restrict__ C = G.nsplit > 1 ? static_cast<float *>(G.part) + (size_t)split * G.N1 * G.N2
                                         : static_cast<float *>(G.C);
    const long long ldc = G.nsplit > 1 ? G.N2 : G.ldc;
    if (n1_0 + BN1 <= G.N1 && n2_0 + BN2 <= G.N2 && (long long)BN1 * ldc < (1LL << 30)) {
        float *__restrict__ cw = C + (size_t)(n1_0 + wm * TM * 32) * ldc + (n2_0 + wn * TN * 32);
        const unsigned ld = (unsigned)ldc;
        const unsigned lane_off = (unsigned)(4 * lj) * ld + TN * li;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const unsigned o = lane_off + (unsigned)(32 * i + (r & 3) + 8 * (r >> 2)) * ld;
#pragma unroll
                for (int j = 0; j < TN; ++j) cw[o + j] = acc[i][j][r];
            }
        return;
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int n1 = n1_0 + wm * TM * 32 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lj;
            const int n2 = n2_0 + wn * TN * 32 + TN * li;
            if (n1 < G.N1) {
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    if (n2 + j < G.N2) C[(long long)n1 * ldc + n2 + j] = acc[i][j][r];
            }
        }
}

// ------------------------------------------------------------------------------------------------ TN (bf16)
// Same problem with bf16 operands, fp32 result: v_mfma_f32_16x16x32_bf16, both fragments by ds_read_b64_tr_b16 (a
// 16-lane group reads a [4 rows][16 columns] block and receives it column-per-lane: lane i gets rows 0..3 of column i).
// Wave tile = (TM*16) x (TN*16); stage = 32 rows (= one MFMA contraction step) of [BN1 + BN2] bf16.
template <int WGM, int WGN, int TM, int TN>
__global__ __launch_bounds__(64 * WGM * WGN) void gemm_tn_bf16_kernel(GemmTnBatch B) {
    constexpr int NW = WGM * WGN;
    constexpr int BR = 32;
    constexpr int BN1 = WGM * TM * 16, BN2 = WGN * TN * 16;
    constexpr int ROWE = BN1 + BN2;                 // bf16 per staged row
    constexpr int STAGE_B = BR * ROWE * 2;
    constexpr int NI = STAGE_B / 1024;
    constexpr int IPW = (NI + NW - 1) / NW;
    static_assert(STAGE_B % 1024 == 0, "stage must be a whole number of 1 KiB pieces");
    __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE_B];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int pi = 0;
#pragma unroll
    for (int i = 1; i < GEMM_MAX_PROB; ++i)
        if (i < B.nprob && blockIdx.x >= B.p[i].block0) pi = i;
    const GemmTnArgs &G = B.p[pi];
    const unsigned tile = tn_tile_of(blockIdx.x - G.block0, G.ntiles, (unsigned)G.nsplit) % G.ntiles;
    const unsigned split = tn_tile_of(blockIdx.x - G.block0, G.ntiles, (unsigned)G.nsplit) / G.ntiles;
    if (split >= (unsigned)G.nsplit) return;           // padding workgroup of a grouped launch (uniform per workgroup)
    const int n1_0 = (int)(tile / G.tiles_n2) * BN1, n2_0 = (int)(tile % G.tiles_n2) * BN2;
    const long long nchunk = G.R / BR;
    const long long c0 = nchunk * split / G.nsplit, c1 = nchunk * (split + 1) / G.nsplit;
    const int nk = (int)(c1 - c0);
    const __bf16 *__restrict__ X = static_cast<const __bf16 *>(G.X);
    const __bf16 *__restrict__ Y = static_cast<const __bf16 *>(G.Y);

    constexpr bool SWZ = EPN_TN_SWZ && BN1 % 128 == 0 && BN2 % 128 == 0;   // (see EPN_TN_SWZ)
    const __bf16 *src[IPW];
    long long sstep[IPW];
#pragma unroll
    for (int i = 0; i < IPW; ++i) {
        const int q = wave + i * NW;
        const int eo = 512 * q + 8 * lane;            // bf16 offset inside the [BR][ROWE] image
        const int r = eo / ROWE;
        int c = eo % ROWE;
        if constexpr (SWZ) c = 8 * ((c >> 3) ^ tn_row_swz(r));      // this LDS slot holds the row's slot (s ^ swz): an involution
        if (c < BN1) {
            int n = n1_0 + c;
            n = n < G.N1 - 8 ? n : G.N1 - 8;
            src[i] = X + (c0 * BR + r) * G.ldx + n;
            sstep[i] = (long long)BR * G.ldx;
        } else {
            int n = n2_0 + (c - BN1);
            n = n < G.N2 - 8 ? n : G.N2 - 8;
            src[i] = Y + (c0 * BR + r) * G.ldy + n;
            sstep[i] = (long long)BR * G.ldy;
        }
    }
    auto stage = [&](int buf) {
#pragma unroll
        for (int i = 0; i < IPW; ++i) {
            const int q = wave + i * NW;
            if (NI % NW == 0 || q < NI) {
                glds16(src[i], smem + buf * STAGE_B + q * 1024);
                src[i] += sstep[i];
            }
        }
    };

    const int wm = wave / WGN, wn = wave % WGN;
    const int li = lane & 15, lg = lane >> 4;
    // transposed read: lane i of a 16-lane group supplies the address of chunk i of the [4][16] block:
    // row i/4, columns 4 (i%4) .. +3; the group g handles contraction rows 8g .. 8g+7 (two reads of 4 rows)
    const int tr_row = 8 * lg + (li >> 2), tr_col = 4 * (li & 3);

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    if (nk > 0) stage(0);
    for (int kt = 0; kt < nk; ++kt) {
        __syncthreads();
        const char *base = smem + (kt & 1) * STAGE_B;
        bf16x8 a[TM], b[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int col = tn_swz_col<SWZ>((wm * TM + i) * 16 + tr_col, tr_row);
            const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                (__attribute__((address_space(3))) s16x4 *)(base + ((tr_row)*ROWE + col) * 2));
            const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                (__attribute__((address_space(3))) s16x4 *)(base + ((tr_row + 4) * ROWE + col) * 2));
            typedef short s16x8 __attribute__((ext_vector_type(8)));
            const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            a[i] = __builtin_bit_cast(bf16x8, v);
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int col = tn_swz_col<SWZ>(BN1 + (wn * TN + j) * 16 + tr_col, tr_row);
            const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                (__attribute__((address_space(3))) s16x4 *)(base + ((tr_row)*ROWE + col) * 2));
            const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                (__attribute__((address_space(3))) s16x4 *)(base + ((tr_row + 4) * ROWE + col) * 2));
            typedef short s16x8 __attribute__((ext_vector_type(8)));
            const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            b[j] = __builtin_bit_cast(bf16x8, v);
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
                if (i == 0 && j == 0) {
                    __builtin_amdgcn_sched_barrier(0);
                    if (kt + 1 < nk) stage((kt + 1) & 1);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
    }

    // D[row = 4 lg + r][col = li]
    float *__restrict__ C = G.nsplit > 1 ? static_cast<float *>(G.part) + (size_t)split * G.N1 * G.N2
                                         : static_cast<float *>(G.C);
    const long long ldc = G.nsplit > 1 ? G.N2 : G.ldc;
    if (n1_0 + BN1 <= G.N1 && n2_0 + BN2 <= G.N2 && (long long)BN1 * ldc < (1LL << 30)) {
        float *__restrict__ cw = C + (size_t)(n1_0 + wm * TM * 16) * ldc + (n2_0 + wn * TN * 16);
        const unsigned ld = (unsigned)ldc;
        const unsigned lane_off = (unsigned)(4 * lg) * ld + li;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const unsigned o = lane_off + (unsigned)(i * 16 + r) * ld;
#pragma unroll
                for (int j = 0; j < TN; ++j) cw[o + j * 16] = acc[i][j][r];
            }
        return;
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n1 = n1_0 + (wm * TM + i) * 16 + 4 * lg + r;
                const int n2 = n2_0 + (wn * TN + j) * 16 + li;
                if (n1 < G.N1 && n2 < G.N2) C[(long long)n1 * ldc + n2] = acc[i][j][r];
            }
}

// ------------------------------------------------------------------------------------------------ TN (bf16), ring form
// The streaming weight gradients (1x1 convolutions: N1, N2 <= 256 outputs over 10^5..10^6 rows) -- same fragments and
// MFMA as gemm_tn_bf16_kernel, but (a) the tile IS the output (no columns of loads wasted on a 256-wide tile), (b) a
// stage holds KR contraction steps and NSTG stages form a ring with NSTG - 1 requested ahead: the wait in front of the
// barrier counts the younger stages' loads instead of draining them, (c) the transposed LDS reads are inline assembly --
// behind the builtin the compiler puts `s_waitcnt vmcnt(0)` in front of the first read of every step (it cannot tell the
// stage being read from the stages the LDS-direct loads are still writing), which empties the ring -- and are waited for
// by hand (the empty asm statements tie each fragment register to that wait).  Few, long workgroups: measured cold
// (tools/tn_probe.py), 256 workgroups stream faster than 512 or 1024 (fewer concurrent DRAM streams).
template <int WGM, int WGN, int TM, int TN, int NSTG, int KR>
__global__ __launch_bounds__(64 * WGM * WGN) void gemm_tn_bf16_ring_kernel(GemmTnBatch B) {
    constexpr int NW = WGM * WGN;
    constexpr int BN1 = WGM * TM * 16, BN2 = WGN * TN * 16;
    constexpr int ROWE = BN1 + BN2;                 // bf16 per staged row
    constexpr int BR = 32 * KR;                     // rows per stage
    constexpr int STAGE_B = BR * ROWE * 2;
    constexpr int NI = STAGE_B / 1024;
    constexpr int IPW = (NI + NW - 1) / NW;
    static_assert(STAGE_B % 1024 == 0, "stage must be a whole number of 1 KiB pieces");
    static_assert(NSTG >= 3 && NSTG <= 4 && NSTG * STAGE_B <= 160 * 1024, "ring of 3 or 4 stages in LDS");
    static_assert(IPW * (NSTG - 2) <= 63, "vmcnt range");
    __shared__ __attribute__((aligned(1024))) char smem[NSTG * STAGE_B];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int pi = 0;
#pragma unroll
    for (int i = 1; i < GEMM_MAX_PROB; ++i)
        if (i < B.nprob && blockIdx.x >= B.p[i].block0) pi = i;
    const GemmTnArgs &G = B.p[pi];
    const unsigned tile = tn_tile_of(blockIdx.x - G.block0, G.ntiles, (unsigned)G.nsplit) % G.ntiles;
    const unsigned split = tn_tile_of(blockIdx.x - G.block0, G.ntiles, (unsigned)G.nsplit) / G.ntiles;
    if (split >= (unsigned)G.nsplit) return;           // padding workgroup of a grouped launch (uniform per workgroup)
    const int n1_0 = (int)(tile / G.tiles_n2) * BN1, n2_0 = (int)(tile % G.tiles_n2) * BN2;
    const long long nchunk = G.R / 32;
    const long long c0 = nchunk * split / G.nsplit, c1 = nchunk * (split + 1) / G.nsplit;
    const int nk = (int)(c1 - c0);
    const int nst = (nk + KR - 1) / KR;             // stages (the last one may be partly used)
    const __bf16 *__restrict__ X = static_cast<const __bf16 *>(G.X);
    const __bf16 *__restrict__ Y = static_cast<const __bf16 *>(G.Y);

    // every wave issues IPW loads per stage so that one vmcnt value holds for all (a wave past the last piece requests
    // piece q - NI again: same bytes to the same place); rows past the end of the operands (last stage of the last
    // split) are clamped to the last row -- loaded, never multiplied
    constexpr bool SWZ = EPN_TN_SWZ && BN1 % 128 == 0 && BN2 % 128 == 0;   // (see EPN_TN_SWZ)
    const __bf16 *src[IPW], *lim[IPW];
    long long sstep[IPW];
#pragma unroll
    for (int i = 0; i < IPW; ++i) {
        const int q = (wave + i * NW) % NI;
        const int eo = 512 * q + 8 * lane;            // bf16 offset inside the [BR][ROWE] image
        const int r = eo / ROWE;
        int c = eo % ROWE;
        if constexpr (SWZ) c = 8 * ((c >> 3) ^ tn_row_swz(r));
        if (c < BN1) {
            int n = n1_0 + c;
            n = n < G.N1 - 8 ? n : G.N1 - 8;
            src[i] = X + (c0 * 32 + r) * G.ldx + n;
            lim[i] = X + (G.R - 1) * G.ldx + n;
            sstep[i] = (long long)BR * G.ldx;
        } else {
            int n = n2_0 + (c - BN1);
            n = n < G.N2 - 8 ? n : G.N2 - 8;
            src[i] = Y + (c0 * 32 + r) * G.ldy + n;
            lim[i] = Y + (G.R - 1) * G.ldy + n;
            sstep[i] = (long long)BR * G.ldy;
        }
    }
    auto stage = [&](int buf) {
#pragma unroll
        for (int i = 0; i < IPW; ++i) {
            const int q = (wave + i * NW) % NI;
            glds16(KR > 1 && src[i] > lim[i] ? lim[i] : src[i], smem + buf * STAGE_B + q * 1024);
            src[i] += sstep[i];
        }
    };

    const int wm = wave / WGN, wn = wave % WGN;
    const int li = lane & 15, lg = lane >> 4;
    const int tr_row = 8 * lg + (li >> 2), tr_col = 4 * (li & 3);      // see gemm_tn_bf16_kernel

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
    for (int s = 0; s < NSTG - 1; ++s)
        if (s < nst) stage(s);
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    for (int kt = 0; kt < nst; ++kt) {
        // stage kt has landed; up to NSTG - 2 younger stages (IPW loads each, this wave's) may still be on their way
        const int ahead = nst - 1 - kt;
        if (NSTG == 4 && ahead >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * IPW) : "memory");
        else if (ahead >= 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(IPW) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const char *sbase = smem + (kt % NSTG) * STAGE_B;
#pragma unroll
        for (int ks = 0; ks < KR; ++ks) {
            if (KR > 1 && kt * KR + ks >= nk) break;
            const char *base = sbase + ks * (32 * ROWE * 2);
            // Y fragments first, then X's: row i of MFMAs starts when its X fragment (and all of Y) has arrived
            s16x4 lo[TM + TN], hi[TM + TN];
#pragma unroll
            for (int f = 0; f < TM + TN; ++f) {
                const int col = tn_swz_col<SWZ>(f < TN ? BN1 + (wn * TN + f) * 16 + tr_col : (wm * TM + (f - TN)) * 16 + tr_col, tr_row);
                const unsigned ad =
                    (unsigned)(uintptr_t)(__attribute__((address_space(3))) char *)(base + (tr_row * ROWE + col) * 2);
                asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(lo[f]) : "v"(ad));
                asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(hi[f]) : "v"(ad), "n"(4 * ROWE * 2));
            }
            bf16x8 b[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                // reads return in order: all but the 2 (TM - 1 - i) youngest have landed
                asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(2 * (TM - 1 - i)) : "memory");
                if (i == 0) {
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        asm volatile("" : "+v"(lo[j]), "+v"(hi[j]));
                        const s16x8 v = {lo[j][0], lo[j][1], lo[j][2], lo[j][3], hi[j][0], hi[j][1], hi[j][2], hi[j][3]};
                        b[j] = __builtin_bit_cast(bf16x8, v);
                    }
                }
                asm volatile("" : "+v"(lo[TN + i]), "+v"(hi[TN + i]));
                const s16x8 va = {lo[TN + i][0], lo[TN + i][1], lo[TN + i][2], lo[TN + i][3],
                                  hi[TN + i][0], hi[TN + i][1], hi[TN + i][2], hi[TN + i][3]};
                const bf16x8 a = __builtin_bit_cast(bf16x8, va);
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[j], acc[i][j], 0, 0, 0);
                    if (ks == 0 && i == 0 && j == 0) {
                        __builtin_amdgcn_sched_barrier(0);
                        if (kt + NSTG - 1 < nst) stage((kt + NSTG - 1) % NSTG);   // the buffer of stage kt - 1 (all waves past it)
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
        }
    }

    // D[row = 4 lg + r][col = li]
    float *__restrict__ C = G.nsplit > 1 ? static_cast<float *>(G.part) + (size_t)split * G.N1 * G.N2
                                         : static_cast<float *>(G.C);
    const long long ldc = G.nsplit > 1 ? G.N2 : G.ldc;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n1 = n1_0 + (wm * TM + i) * 16 + 4 * lg + r;
                const int n2 = n2_0 + (wn * TN + j) * 16 + li;
                if (n1 < G.N1 && n2 < G.N2) C[(long long)n1 * ldc + n2] = acc[i][j][r];
            }
}

// sum the split partials in a fixed order (deterministic): C[i] = sum_s part[s][i].  Streaming: 16-byte loads, eight
// splits in flight per thread (a scalar loop over the splits ran at a third of the HBM rate).
__global__ __launch_bounds__(256) void gemm_tn_reduce_kernel(GemmTnBatch B) {      // blockIdx.y = problem
    const GemmTnArgs &G = B.p[blockIdx.y];
    if (G.nsplit <= 1) return;
    const float *__restrict__ part = static_cast<const float *>(G.part);
    float *__restrict__ C = static_cast<float *>(G.C);
    const size_t n = (size_t)G.N1 * G.N2;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    if ((G.N2 & 3) == 0 && (G.ldc & 3) == 0 && !((uintptr_t)C & 15)) {
        const size_t n4 = n >> 2;
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
            const f32x4 *p = reinterpret_cast<const f32x4 *>(part) + i;
            f32x4 a[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) a[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            int k = 0;
            for (; k + 8 <= G.nsplit; k += 8)
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const f32x4 v = p[(size_t)(k + u) * n4];
                    a[u][0] += v[0]; a[u][1] += v[1]; a[u][2] += v[2]; a[u][3] += v[3];
                }
            for (; k < G.nsplit; ++k) {
                const f32x4 v = p[(size_t)k * n4];
                a[0][0] += v[0]; a[0][1] += v[1]; a[0][2] += v[2]; a[0][3] += v[3];
            }
            f32x4 r;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                r[e] = ((a[0][e] + a[1][e]) + (a[2][e] + a[3][e])) + ((a[4][e] + a[5][e]) + (a[6][e] + a[7][e]));
            const size_t e0 = i << 2;
            *reinterpret_cast<f32x4 *>(C + (e0 / G.N2) * G.ldc + (e0 % G.N2)) = r;
        }
        return;
    }
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        float s = 0.f;
        for (int k = 0; k < G.nsplit; ++k) s += part[(size_t)k * n + i];
        C[(i / G.N2) * G.ldc + (i % G.N2)] = s;
    }
}

// The same sum for SMALL outputs with MANY partials (the narrow weight gradients: 32 x 32 .. 256 x 128 outputs, 256
// partial slabs): one thread per output quad walks all the slabs in rounds of eight dependent-latency loads -- 32 rounds,
// ~40 us, as long as the GEMM itself.  Here SP threads share a quad: thread g of them sums slabs g, g + SP, g + 2 SP, ...
// (four in flight), the SP partial sums are added in the order g = 0 .. SP-1 through LDS.  Fixed order: deterministic.
template <int SP>
__global__ __launch_bounds__(256) void gemm_tn_reduce_sp_kernel(GemmTnBatch B) {      // blockIdx.y = problem
    constexpr int QB = 256 / SP;                   // output quads per workgroup
    __shared__ f32x4 red[SP][QB];
    const GemmTnArgs &G = B.p[blockIdx.y];
    if (G.nsplit <= 1) return;
    const f32x4 *__restrict__ part = static_cast<const f32x4 *>(G.part);
    float *__restrict__ C = static_cast<float *>(G.C);
    const size_t n4 = ((size_t)G.N1 * G.N2) >> 2;
    const int ql = threadIdx.x % QB, g = threadIdx.x / QB;
    for (size_t q0 = (size_t)blockIdx.x * QB; q0 < n4; q0 += (size_t)gridDim.x * QB) {      // uniform per workgroup
        const size_t q = q0 + ql;
        f32x4 a[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (q < n4) {
            int k = g;
            for (; k + 3 * SP < G.nsplit; k += 4 * SP)
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const f32x4 v = part[(size_t)(k + u * SP) * n4 + q];
                    a[u][0] += v[0]; a[u][1] += v[1]; a[u][2] += v[2]; a[u][3] += v[3];
                }
            for (; k < G.nsplit; k += SP) {
                const f32x4 v = part[(size_t)k * n4 + q];
                a[0][0] += v[0]; a[0][1] += v[1]; a[0][2] += v[2]; a[0][3] += v[3];
            }
        }
        f32x4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = (a[0][e] + a[1][e]) + (a[2][e] + a[3][e]);
        red[g][ql] = r;
        __syncthreads();
        if (g == 0 && q < n4) {
            for (int j = 1; j < SP; ++j) {
                const f32x4 v = red[j][ql];
                r[0] += v[0]; r[1] += v[1]; r[2] += v[2]; r[3] += v[3];
            }
            const size_t e0 = q << 2;
            *reinterpret_cast<f32x4 *>(C + (e0 / G.N2) * G.ldc + (e0 % G.N2)) = r;
        }
        __syncthreads();
    }
}

// generic fallback (any shape, VALU): one thread per output element
template <typename T>
__global__ void gemm_tn_generic_kernel(const T *__restrict__ X, const T *__restrict__ Y, float *__restrict__ C,
                                       long long R, int N1, int N2, long long ldx, long long ldy, long long ldc) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)N1 * N2) return;
    const int n1 = (int)(i / N2), n2 = (int)(i % N2);
    float s = 0.f;
    for (long long r = 0; r < R; ++r) s = fmaf((float)X[r * ldx + n1], (float)Y[r * ldy + n2], s);
    C[(long long)n1 * ldc + n2] = s;
}

// ------------------------------------------------------------------------------------------------ the kernel instances
// Every TN kernel instance the library launches is named ONCE, here: X(...) = its template arguments, from which the block
// tile BN1 x BN2 follows.  tn_plan() chooses (family, BN1, BN2); the launcher looks the instance up and fails with EPN_EINVAL
// when there is none -- no catch-all that would run a kernel of another tile size.
enum TnFamily { TN_F32, TN_PLANES, TN_BF16, TN_RING };
// gemm_tn_f32_kernel<WGM, WGN, TM, TN, BR, X3>, X3 = 0 / 3 / 2 by mode; tile (WGM*TM*32) x (WGN*TN*32)
#define EPN_TN_F32_INSTANCES(X)                                                                                      \
    X(1, 8, 1, 2, 32) /*  32 x 512 */                                                                                \
    X(2, 2, 1, 1, 32) /*  64 x  64 */                                                                                \
    X(2, 2, 1, 2, 32) /*  64 x 128 */                                                                                \
    X(1, 8, 2, 1, 32) /*  64 x 256 */                                                                                \
    X(1, 4, 2, 4, 16) /*  64 x 512 */                                                                                \
    X(2, 2, 2, 1, 32) /* 128 x  64 */                                                                                \
    X(2, 2, 2, 2, 32) /* 128 x 128 */                                                                                \
    X(2, 4, 2, 2, 32) /* 128 x 256 */                                                                                \
    X(1, 8, 4, 2, 32) /* 128 x 512 */
// gemm_tn_x3_kernel<WGM, WGN, TM, TN, BR, NPL>, NPL = 3 / 2 by mode; same tile formula
#define EPN_TN_PLANES_INSTANCES(X)                                                                                   \
    X(1, 8, 1, 2, 32) /*  32 x 512 */                                                                                \
    X(1, 8, 2, 2, 16) /*  64 x 512 */                                                                                \
    X(2, 4, 2, 2, 32) /* 128 x 256: grouped spectral weight gradients (c >= 128) */                                  \
    X(1, 8, 4, 2, 16) /* 128 x 512 */                                                                                \
    X(2, 4, 4, 2, 16) /* 256 x 256 */
// gemm_tn_bf16_kernel<WGM, WGN, TM, TN>; tile (WGM*TM*16) x (WGN*TN*16).  4 waves: fewer, larger wave tiles.  The 128 x 256
// tile on FOUR waves (64 x 128 per wave: 32 MFMAs per 12 transposed LDS reads): the 8-wave form (16 MFMAs per 16 reads) was
// LDS-bandwidth bound -- 3 workgroups x 64 KB of fragment reads per 1024 cycles > 128 B/clk: 245760 x 256 x 6144: 1.63 -> 1.23 ms
// (630 TFLOP/s)
#define EPN_TN_BF16_INSTANCES(X)                                                                                     \
    X(1, 4, 2, 4) /*  32 x 256 */                                                                                    \
    X(1, 4, 4, 4) /*  64 x 256 */                                                                                    \
    X(2, 2, 4, 8) /* 128 x 256 */
// gemm_tn_bf16_ring_kernel<WGM, WGN, TM, TN, NSTG, KR>; same tile formula.  Narrow single problems (gemm_tn_tile): 2 x 2 waves,
// the tile IS the output; and the 128 x 256 tile of the grouped launches (single problems of that tile stay on the two-stage
// kernel: the ring measured no gain there, CHANGELOG round 6)
#define EPN_TN_RING_NARROW(X, TM, TN) X(2, 2, TM, TN, EPN_TN_NARROW_NSTG, tn_ring_kr(2, 2, TM, TN))
#define EPN_TN_RING_INSTANCES(X)                                                                                     \
    EPN_TN_RING_NARROW(X, 1, 1) /*  32 x  32 */                                                                      \
    EPN_TN_RING_NARROW(X, 2, 1) /*  64 x  32 */                                                                      \
    EPN_TN_RING_NARROW(X, 1, 2) /*  32 x  64 */                                                                      \
    EPN_TN_RING_NARROW(X, 2, 2) /*  64 x  64 */                                                                      \
    EPN_TN_RING_NARROW(X, 4, 2) /* 128 x  64 */                                                                      \
    EPN_TN_RING_NARROW(X, 8, 2) /* 256 x  64 */                                                                      \
    EPN_TN_RING_NARROW(X, 1, 4) /*  32 x 128 */                                                                      \
    EPN_TN_RING_NARROW(X, 2, 4) /*  64 x 128 */                                                                      \
    EPN_TN_RING_NARROW(X, 4, 4) /* 128 x 128 */                                                                      \
    EPN_TN_RING_NARROW(X, 8, 4) /* 256 x 128 */                                                                      \
    X(2, 2, 4, 8, EPN_TN_WIDE_NSTG, 1) /* 128 x 256 */

struct TnChoice {          // what tn_plan decided: the workspace query and the launcher both go by it
    TnFamily family;
    int bn1, bn2;          // block tile = the instance inside the family
    bool planes;           // X pre-split into planes (family TN_PLANES; the planes are carved from the workspace)
    size_t ws_bytes;       // workspace the launch needs
    size_t amax_off;       // two-piece form: offset of the [max|X_i|, max|Y_i|] slots inside the workspace
};

inline bool tn_has_instance(TnFamily f, int bn1, int bn2) {
#define EPN_TN_IS32(WGM, WGN, TM, TN, ...) || (bn1 == WGM * TM * 32 && bn2 == WGN * TN * 32)
#define EPN_TN_IS16(WGM, WGN, TM, TN, ...) || (bn1 == WGM * TM * 16 && bn2 == WGN * TN * 16)
    switch (f) {
        case TN_F32: return false EPN_TN_F32_INSTANCES(EPN_TN_IS32);
        case TN_PLANES: return false EPN_TN_PLANES_INSTANCES(EPN_TN_IS32);
        case TN_BF16: return false EPN_TN_BF16_INSTANCES(EPN_TN_IS16);
        case TN_RING: return false EPN_TN_RING_INSTANCES(EPN_TN_IS16);
    }
#undef EPN_TN_IS32
#undef EPN_TN_IS16
    return false;
}

// launches the instance `ch` names; EPN_EINVAL when the tables above have none
template <typename T>
int launch_tn_instance(const TnChoice &ch, const GemmTnBatch &B, hipStream_t st, int x3) {
    const dim3 grid(B.nblocks);
#define EPN_TN_F32(WGM, WGN, TM, TN, BR)                                                                                       \
    if (ch.bn1 == WGM * TM * 32 && ch.bn2 == WGN * TN * 32) {                                                                  \
        if (x3 == 3) EPN_LAUNCH((gemm_tn_f32_kernel<WGM, WGN, TM, TN, BR, 3>), grid, dim3(64 * WGM * WGN), 0, st, B);          \
        else if (x3 == 2) EPN_LAUNCH((gemm_tn_f32_kernel<WGM, WGN, TM, TN, BR, 2>), grid, dim3(64 * WGM * WGN), 0, st, B);     \
        else EPN_LAUNCH((gemm_tn_f32_kernel<WGM, WGN, TM, TN, BR, 0>), grid, dim3(64 * WGM * WGN), 0, st, B);                  \
        return 0;                                                                                                              \
    }
#define EPN_TN_PLANES(WGM, WGN, TM, TN, BR)                                                                                    \
    if (ch.bn1 == WGM * TM * 32 && ch.bn2 == WGN * TN * 32) {                                                                  \
        if (x3 == 3) EPN_LAUNCH((gemm_tn_x3_kernel<WGM, WGN, TM, TN, BR, 3>), grid, dim3(64 * WGM * WGN), 0, st, B);           \
        else EPN_LAUNCH((gemm_tn_x3_kernel<WGM, WGN, TM, TN, BR, 2>), grid, dim3(64 * WGM * WGN), 0, st, B);                   \
        return 0;                                                                                                              \
    }
#define EPN_TN_BF16(WGM, WGN, TM, TN)                                                                                          \
    if (ch.bn1 == WGM * TM * 16 && ch.bn2 == WGN * TN * 16) {                                                                  \
        EPN_LAUNCH((gemm_tn_bf16_kernel<WGM, WGN, TM, TN>), grid, dim3(64 * WGM * WGN), 0, st, B);                             \
        return 0;                                                                                                              \
    }
#define EPN_TN_RING(WGM, WGN, TM, TN, NSTG, KR)                                                                                \
    if (ch.bn1 == WGM * TM * 16 && ch.bn2 == WGN * TN * 16) {                                                                  \
        EPN_LAUNCH((gemm_tn_bf16_ring_kernel<WGM, WGN, TM, TN, NSTG, KR>), grid, dim3(64 * WGM * WGN), 0, st, B);              \
        return 0;                                                                                                              \
    }
    if constexpr (sizeof(T) == 4) {
        if (ch.family == TN_F32) { EPN_TN_F32_INSTANCES(EPN_TN_F32) }
        if (ch.family == TN_PLANES) { EPN_TN_PLANES_INSTANCES(EPN_TN_PLANES) }
    } else {
        if (ch.family == TN_BF16) { EPN_TN_BF16_INSTANCES(EPN_TN_BF16) }
        if (ch.family == TN_RING) { EPN_TN_RING_INSTANCES(EPN_TN_RING) }
    }
#undef EPN_TN_F32
#undef EPN_TN_PLANES
#undef EPN_TN_BF16
#undef EPN_TN_RING
    return EPN_EINVAL;
}

// split form: single wide weight gradients take the pre-split planes kernel, narrow / grouped ones split in the kernel
// (N2 = the narrowest output; groups of c = 128 blocks measured slower with the extra pass over X: 1.43 vs 1.34 ms,
// c = 256 ones too once timed cold -- X is as large as Y in a spectral block, so the pre-split is a full extra pass)
#ifndef EPN_TN_GROUP_PLANES     // narrowest output from which a GROUP takes the pre-split planes kernel (256 x 256 tiles)
#define EPN_TN_GROUP_PLANES 512  // (three-piece form; the two-piece form: 256, see below) cold, tools/tn_probe.py, three-piece bf16 form: c = 256 groups 1.05 ms in-kernel split vs 1.14 planes; c = 512: 2.40 vs 1.48.
                                 // Two-piece fp16 form (round 5: the planes are 4 bytes per value, the MFMA half is twice as fast, so the in-kernel split of BOTH
                                 // operands weighs more; tools/spectral_dw_probe.py, maxima supplied): c = 256, 4096 points 0.751 -> 0.632 ms, 2048 points 0.368 -> 0.361;
                                 // c = 128 0.420 -> 0.441, c = 64 0.296 -> 0.346 (stay on the in-kernel split)
#endif
inline int tn_group_planes(int x3) { return x3 == 2 ? EPN_TN_GROUP_PLANES / 2 : EPN_TN_GROUP_PLANES; }
inline bool tn_planes_form(int nprob, int N2, int x3) { return N2 >= (nprob == 1 ? 512 : tn_group_planes(x3)); }

template <typename T>
bool tn_fast_ok(const GemmTnArgs &G) {
    constexpr int E16 = ElemOf<T>::PER16;
    return G.R > 0 && G.R % 32 == 0 && G.N1 >= E16 && G.N2 >= E16 && G.ldx % E16 == 0 && G.ldy % E16 == 0 &&
           !((uintptr_t)G.X & 15) && !((uintptr_t)G.Y & 15) && G.N1 % E16 == 0 && G.N2 % E16 == 0;
}

// Plan of a (grouped) TN launch: one block tile for all problems; splits so that every workgroup runs about the same
// number of K steps and the launch has ~2048 workgroups (single problem) / ~1024 (group); partial slabs carved from `ws`.
template <typename T>
TnChoice tn_plan(GemmTnBatch &B, void *ws, int x3 = 0) {
    // x3: 0 = operands as they are, 3 = fp32 operands in three bf16 pieces, 2 = in two fp16 pieces (same tiles and splits)
    const int bf = sizeof(T) == 2 ? 1 : (x3 ? 2 : 0);
    int max1 = 0, min2 = 1 << 30;
    for (int i = 0; i < B.nprob; ++i) {
        max1 = B.p[i].N1 > max1 ? B.p[i].N1 : max1;
        min2 = B.p[i].N2 < min2 ? B.p[i].N2 : min2;
    }
    int bn1, bn2;
    gemm_tn_tile(B.nprob > 1 && bf == 2 ? 0 : bf, max1, B.nprob > 1 && min2 < 256 ? 256 : min2, &bn1, &bn2);   // groups: the wide tiles
    if (B.nprob > 1 && bf == 2 && min2 >= tn_group_planes(x3)) {       // wide spectral groups (c >= 512), split form: 256 x 256 tiles
        int min1 = 1 << 30;                             // halve the re-reads of X and Y (every tile row / column streams
        for (int i = 0; i < B.nprob; ++i) min1 = B.p[i].N1 < min1 ? B.p[i].N1 : min1;   // the other operand again)
        if (min1 >= 256) { bn1 = 256; bn2 = 256; }
    }
    // narrow spectral groups (c < 256) in the two-piece form: 128 x 128 tiles -- 64 KB of stages, two workgroups per CU, and the
    // ragged widths (c, 3c, 3c, 4c, 5c) pad less: c = 64 0.302 -> 0.279 ms, c = 128 0.422 -> 0.348 (tools/spectral_dw_probe.py)
    if (B.nprob > 1 && x3 == 2 && min2 < 256) { bn1 = 128; bn2 = 128; }
    long long tiles[GEMM_MAX_PROB], chunks[GEMM_MAX_PROB];
    for (int i = 0; i < B.nprob; ++i) {
        GemmTnArgs &G = B.p[i];
        G.tiles_n2 = (G.N2 + bn2 - 1) / bn2;
        G.ntiles = (unsigned)((G.N1 + bn1 - 1) / bn1) * G.tiles_n2;
        tiles[i] = G.ntiles;
        chunks[i] = G.R / 32;
    }
    if (B.nprob == 1) {
        B.p[0].nsplit = gemm_tn_splits(bf, B.p[0].R, B.p[0].N1, B.p[0].N2);
    } else {
        // smallest steps-per-workgroup S (>= 8) whose launch fits `target` workgroups; every problem gets ceil(chunks / S)
        // splits.  The five problems of a group are ragged (d = 1, 3, 3, 4, 5 times the rows AND the width): with ONE round
        // of 256 workgroups the launch ends when its longest ones do (76 % of the CU-time used, SQ_BUSY / GRBM 3.1 against
        // 3.85 for the single-problem kernels); several rounds of shorter workgroups fill in behind each other.  fp32 groups,
        // cold (tools/tn_probe.py), 256 / 384 / 512 / 768 / 1024 / 1536 / 2048 workgroups: c = 64: 0.64 / 0.49 / 0.52 / 0.42 /
        // 0.43 / 0.45 / 0.48 ms, c = 128: 0.84 / 0.67 / 0.71 / 0.60 / 0.61 / 0.64 / 0.67, c = 256: 0.98 / 1.03 / 0.91 / 0.97 /
        // 0.94 / 0.97 / 1.00.  (Round 2 measured the opposite, 6.2 / 6.7 / 7.4 / 7.9 ms per step for 256 / 512 / 1024 / 2048:
        // that was the cost of its slab reduction, one thread per output quad walking every slab -- gemm_tn_reduce_sp_kernel.)
        const long long target = bf == 1 ? EPN_TN_GROUP_TARGET_BF16 : EPN_TN_GROUP_TARGET_F32;
        long long S = 8;
        for (long long cand = 8; cand <= 8192; ++cand) {
            long long blocks = 0;
            for (int i = 0; i < B.nprob; ++i) blocks += tiles[i] * ((chunks[i] + cand - 1) / cand);
            S = cand;
            if (blocks <= target) break;
        }
        for (int i = 0; i < B.nprob; ++i) {
            long long sp = (chunks[i] + S - 1) / S;
            sp = sp < 1 ? 1 : (sp > 512 ? 512 : sp);
            B.p[i].nsplit = (int)sp;
        }
    }
    size_t off = 0;
    unsigned blk = 0;
    for (int i = 0; i < B.nprob; ++i) {
        GemmTnArgs &G = B.p[i];
        G.block0 = blk;
        blk += (G.ntiles * (unsigned)G.nsplit + 7u) & ~7u;      // whole octets: workgroup % 8 (= XCD) holds per problem
        G.part = nullptr; G.part_bytes = 0;
        if (G.nsplit > 1) {
            const size_t nb = (size_t)G.nsplit * G.N1 * G.N2 * sizeof(float);
            if (ws) G.part = static_cast<char *>(ws) + off;
            G.part_bytes = nb;
            off += (nb + 255) & ~(size_t)255;
        }
    }
    B.nblocks = blk;
    for (int i = 0; i < B.nprob; ++i) B.p[i].Xp = nullptr;
    const bool planes = x3 && tn_has_instance(TN_PLANES, bn1, bn2) && tn_planes_form(B.nprob, min2, x3);
    if (planes)                                 // bf16 planes of X: 6 bytes per value (fp16 planes: 4)
        for (int i = 0; i < B.nprob; ++i) {
            GemmTnArgs &G = B.p[i];
            // (a null workspace = size query: a non-null marker keeps the two passes on the same path)
            G.Xp = ws ? static_cast<char *>(ws) + off : reinterpret_cast<const void *>(1);
            off += ((size_t)2 * x3 * G.R * G.N1 + 255) & ~(size_t)255;
        }
    size_t amax_off = 0;
    if (x3 == 2) {                              // two-piece form: [max|X_i|, max|Y_i|] per problem when the caller has none
        amax_off = off;
        off += 256;
    }
    TnFamily family = planes ? TN_PLANES : TN_F32;
    // bf16: the narrow single problems (gemm_tn_tile) and the 128 x 256 tile of a GROUP stream through the ring kernel
    if constexpr (sizeof(T) == 2) family = (B.nprob == 1 ? bn2 <= 128 : bn1 == 128) ? TN_RING : TN_BF16;
    return TnChoice{family, bn1, bn2, planes, off, amax_off};
}

template <typename T>
int launch_tn_typed(GemmTnBatch &B, void *ws, size_t ws_bytes, hipStream_t st, int x3 = 0) {
    bool fast = true;
    for (int i = 0; i < B.nprob; ++i) {
        const GemmTnArgs &G = B.p[i];
        if (G.R < 0 || G.N1 < 1 || G.N2 < 1) return EPN_EINVAL;
        if (!G.C) return EPN_ENULL;
        if (G.R > 0 && (!G.X || !G.Y)) return EPN_ENULL;
        fast = fast && tn_fast_ok<T>(G);
    }
    if (!fast) {
        for (int i = 0; i < B.nprob; ++i) {
            const GemmTnArgs &G = B.p[i];
            const long long n = (long long)G.N1 * G.N2;
            EPN_LAUNCH((gemm_tn_generic_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                               static_cast<const T *>(G.X), static_cast<const T *>(G.Y), static_cast<float *>(G.C), G.R,
                               G.N1, G.N2, G.ldx, G.ldy, G.ldc);
            EPN_CHECK_LAUNCH();
        }
        return 0;
    }
    const TnChoice ch = tn_plan<T>(B, ws, x3);
    if (ch.ws_bytes > 0 && (!ws || ws_bytes < ch.ws_bytes)) return EPN_EWORKSPACE;
    if (!tn_has_instance(ch.family, ch.bn1, ch.bn2)) return EPN_EINVAL;      // (before the helper launches below)
    if constexpr (sizeof(T) == 4) {
        if (x3 == 2) {                                  // maxima nobody supplied: one pass over the operand each
            float *slots = reinterpret_cast<float *>(static_cast<char *>(ws) + ch.amax_off);
            for (int i = 0; i < B.nprob; ++i) {
                GemmTnArgs &G = B.p[i];
                if (!G.x_amax) {
                    int rc = launch_absmax(static_cast<const float *>(G.X), G.ldx, G.R, G.N1, slots + 2 * i, st);
                    if (rc) return rc;
                    G.x_amax = slots + 2 * i;
                }
                if (!G.y_amax) {
                    int rc = launch_absmax(static_cast<const float *>(G.Y), G.ldy, G.R, G.N2, slots + 2 * i + 1, st);
                    if (rc) return rc;
                    G.y_amax = slots + 2 * i + 1;
                }
            }
        }
        if (ch.planes) {
            for (int i = 0; i < B.nprob; ++i) {         // X's planes (workspace, after the slabs)
                const GemmTnArgs &G = B.p[i];
                const long long n = (G.R >> 3) * G.N1;
                if (x3 == 3)
                    EPN_LAUNCH_AUX(split_octets_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                                   static_cast<const float *>(G.X), G.ldx, G.R, G.N1, static_cast<u32x4 *>(const_cast<void *>(G.Xp)));
                else
                    EPN_LAUNCH_AUX(split_octets2_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                                   static_cast<const float *>(G.X), G.ldx, G.R, G.N1, static_cast<u32x4 *>(const_cast<void *>(G.Xp)), G.x_amax);
                EPN_CHECK_LAUNCH();
            }
        }
    }
    const int rc = launch_tn_instance<T>(ch, B, st, x3);
    if (rc) return rc;
    EPN_CHECK_LAUNCH();
    bool any_split = false;
    size_t nmax = 0;
    for (int i = 0; i < B.nprob; ++i) {
        any_split = any_split || B.p[i].nsplit > 1;
        const size_t n = (size_t)B.p[i].N1 * B.p[i].N2;
        nmax = n > nmax ? n : nmax;
    }
    if (any_split) {
        const size_t nv = (nmax + 3) / 4;               // one thread per four outputs
        bool quads = true;                              // (the shared-quad form needs the 16-byte path of every problem)
        int smax = 1;
        for (int i = 0; i < B.nprob; ++i) {
            const GemmTnArgs &G = B.p[i];
            quads = quads && (G.N2 & 3) == 0 && (G.ldc & 3) == 0 && !((uintptr_t)G.C & 15);
            smax = G.nsplit > smax ? G.nsplit : smax;
        }
        // many partials: SP threads per quad so that a thread walks its slabs in at most ~4 rounds of four loads (while
        // the launch stays under a million threads)
        int sp = 1;
        while (quads && sp < 64 && smax > 16 * sp && nv * B.nprob * sp * 4 <= (1u << 20)) sp *= 4;
        if (sp > 1) {
            const size_t qb = 256 / sp;
            const unsigned gx = (unsigned)((nv + qb - 1) / qb < 2048 ? (nv + qb - 1) / qb : 2048);
            if (sp == 4) EPN_LAUNCH_AUX(gemm_tn_reduce_sp_kernel<4>, dim3(gx, B.nprob), dim3(256), 0, st, B);
            else if (sp == 16) EPN_LAUNCH_AUX(gemm_tn_reduce_sp_kernel<16>, dim3(gx, B.nprob), dim3(256), 0, st, B);
            else EPN_LAUNCH_AUX(gemm_tn_reduce_sp_kernel<64>, dim3(gx, B.nprob), dim3(256), 0, st, B);
        } else {
            const unsigned gx = (unsigned)((nv + 255) / 256 < 2048 ? (nv + 255) / 256 : 2048);
            EPN_LAUNCH_AUX(gemm_tn_reduce_kernel, dim3(gx, B.nprob), dim3(256), 0, st, B);
        }
        EPN_CHECK_LAUNCH();
    }
    return 0;
}

}  // namespace

EPN_F2_SENTINEL_TAKE(f2_nonfinite_take_gemm)

// block tile of the TN kernels for an output of N1 x N2 (shared with the workspace query)
void gemm_tn_tile(int dtype, int N1, int N2, int *bn1, int *bn2) {   // dtype: 0 fp32, 1 bf16, 2 fp32 split form
    if (dtype == 1) {
        if (N2 <= 128) {        // 1x1 convolutions: the tile IS the output, ring form (gemm_tn_bf16_ring_kernel)
            *bn2 = N2 <= 32 ? 32 : (N2 <= 64 ? 64 : 128);
            *bn1 = N1 <= 32 ? 32 : (N1 <= 64 ? 64 : (N1 <= 128 ? 128 : 256));
            if (*bn2 == 32 && *bn1 > 64) *bn1 = 64;
            return;
        }
        if (N1 <= 32) { *bn1 = 32; *bn2 = 256; }
        else if (N1 <= 64) { *bn1 = 64; *bn2 = 256; }
        else { *bn1 = 128; *bn2 = 256; }
    } else {
        // wide outputs (dW of the inter convolutions: N2 = cin*ks): 512-column tiles, 8 MFMAs per pair of LDS reads;
        // narrow ones (spectral blocks, 1x1 convolutions): 256-column tiles
        // narrow single problems (dW of the 1x1 convolutions: N2 = cin <= 128): 64- / 128-column tiles, 4 waves
        if (dtype == 2 && N2 >= 512) {   // split form, wide outputs (gemm_tn_x3_kernel): X planes + Y rows, two stages in LDS
            if (N1 <= 32) { *bn1 = 32; *bn2 = 512; }
            else if (N1 <= 64) { *bn1 = 64; *bn2 = 512; }
            else if (N1 >= 256) { *bn1 = 256; *bn2 = 256; }     // X covered by one tile row: Y is streamed once
            else { *bn1 = 128; *bn2 = 512; }
            return;
        }
        if (N1 <= 32 && N2 > 128) { *bn1 = 32; *bn2 = 512; }      // (narrow N2: the 64-row tiles below, not a 512-column tile)
        else if (N1 <= 64) { *bn1 = 64; *bn2 = N2 >= 512 ? 512 : (N2 > 128 ? 256 : (N2 > 64 ? 128 : 64)); }
        else { *bn1 = 128; *bn2 = N2 >= 512 ? 512 : (N2 > 128 ? 256 : (N2 > 64 ? 128 : 64)); }
    }
}

int gemm_tn_splits(int dtype, long long R, int N1, int N2) {
    int bn1, bn2;
    gemm_tn_tile(dtype, N1, N2, &bn1, &bn2);
    const long long tiles = (long long)((N1 + bn1 - 1) / bn1) * ((N2 + bn2 - 1) / bn2);
    const long long chunks = R / 32;
    const int pol = kernel_policy();
    const long long target = (pol & ~0xff) == 0x200 ? 256LL * (pol & 0xff) : (dtype == 1 ? EPN_TN_SINGLE_TARGET_BF16 : 512);    // 0x200 | v: tuning override
    // two rounds of the 256 CUs.  With the split count rounded down (below) 512 / 1024 / 1536 / 2048 workgroups run the dW
    // shapes of the ModelNet schedule within 1.5 % of each other (18.7 / 18.8 / 18.9 / 19.0 ms summed, fp32 partial slabs and
    // their fixed-order reduction included); fewer workgroups = fewer partial slabs
    // rounded DOWN: the wide tiles take a whole CU's LDS, so 2048 workgroups are exactly 8 rounds of the 256 CUs and one
    // workgroup more is a ninth round that runs 16 workgroups wide (24 tiles x 86 splits = 2064: measured 118 -> 129 TFLOP/s)
    if (dtype == 1 && N2 <= 128 && (pol & ~0xff) != 0x200) {
        // ring form: EPN_TN_NARROW_WGS workgroups per CU, all resident; >= 16 steps per split
        long long sn = 256LL * EPN_TN_NARROW_WGS / tiles;
        const long long cap = chunks / 16 > 1 ? chunks / 16 : 1;
        sn = sn > cap ? cap : sn;
        return (int)(sn < 1 ? 1 : sn);
    }
    long long s = target / tiles;
    // at least 32 K steps per split: a split ends in an N1 x N2 fp32 slab write (+ its share of the reduction), which
    // for the short-and-wide problems (spectral blocks: R = pts*d rows, up to 1280 x 1280 outputs) outweighs 8 steps of loads
    const long long smax = chunks / 32 > 1 ? chunks / 32 : 1;
    if (s > smax) s = smax;
    if (s > 512) s = 512;
    return (int)(s < 1 ? 1 : s);
}

int launch_gemm_tn_batch(GemmTnBatch &B, int dtype, void *ws, size_t ws_bytes, hipStream_t st) {
    if (B.nprob < 1 || B.nprob > GEMM_MAX_PROB) return EPN_EINVAL;
    if (dtype == 2) return launch_tn_typed<float>(B, ws, ws_bytes, st, 3);    // fp32 operands, three bf16 pieces
    if (dtype == 3) return launch_tn_typed<float>(B, ws, ws_bytes, st, 2);    // fp32 operands, two fp16 pieces
    return dtype == 0 ? launch_tn_typed<float>(B, ws, ws_bytes, st) : launch_tn_typed<__bf16>(B, ws, ws_bytes, st);
}

size_t gemm_tn_batch_workspace(GemmTnBatch &B, int dtype) {
    for (int i = 0; i < B.nprob; ++i)
        if (B.p[i].R < 32 || B.p[i].N1 < 1 || B.p[i].N2 < 1) return 0;
    return dtype != 1 ? tn_plan<float>(B, nullptr, dtype == 2 ? 3 : (dtype == 3 ? 2 : 0)).ws_bytes
                      : tn_plan<__bf16>(B, nullptr).ws_bytes;
}

int launch_gemm_tn(GemmTnArgs &G, int dtype, hipStream_t st) {
    GemmTnBatch B;
    B.nprob = 1; B.nblocks = 0; B.p[0] = G;
    return launch_gemm_tn_batch(B, dtype, G.part, G.part_bytes, st);
}

}  // namespace epn

using namespace epn;

extern "C" size_t epn_gemm_tn_workspace_bytes(int bf16, long long R, int N1, int N2) {
    if (R < 1 || N1 < 1 || N2 < 1) return 0;
    const int mode = bf16 == 3 ? 2 : bf16;            // 3 = two-piece fp16 form: the tiles and splits of the three-piece form
    const int s = gemm_tn_splits(mode, R, N1, N2);
    const size_t planes = mode == 2 && N2 >= 512 ? (((size_t)(bf16 == 3 ? 4 : 6) * R * N1 + 255) & ~(size_t)255) : 0;   // X's planes
    return (s > 1 ? (((size_t)s * N1 * N2 * sizeof(float) + 255) & ~(size_t)255) : 0) + planes + (bf16 == 3 ? 256 : 0);
}

static int tn_entry(const void *X, long long ldx, const void *Y, long long ldy, float *C, long long ldc, long long R, int N1,
                    int N2, void *ws, size_t ws_bytes, int dtype, epn_stream_t stream) {
    GemmTnArgs G;
    G.X = X; G.Y = Y; G.C = C; G.part = ws; G.part_bytes = ws_bytes; G.R = R; G.N1 = N1; G.N2 = N2;
    G.ldx = ldx; G.ldy = ldy; G.ldc = ldc; G.ntiles = 0; G.tiles_n2 = 0; G.nsplit = 1; G.block0 = 0; G.Xp = nullptr; G.x_amax = G.y_amax = nullptr;
    return launch_gemm_tn(G, dtype, epn_stream(stream));
}
extern "C" int epn_gemm_tn_f32(const float *X, long long ldx, const float *Y, long long ldy, float *C, long long ldc,
                               long long R, int N1, int N2, void *workspace, size_t workspace_bytes, epn_stream_t stream) {
    return tn_entry(X, ldx, Y, ldy, C, ldc, R, N1, N2, workspace, workspace_bytes, 0, stream);
}
extern "C" int epn_gemm_tn_split_f32(const float *X, long long ldx, const float *Y, long long ldy, float *C, long long ldc,
                                     long long R, int N1, int N2, void *workspace, size_t workspace_bytes, epn_stream_t stream) {
    return tn_entry(X, ldx, Y, ldy, C, ldc, R, N1, N2, workspace, workspace_bytes, 2, stream);
}
extern "C" int epn_gemm_tn_bf16(const void *X, long long ldx, const void *Y, long long ldy, float *C, long long ldc,
                                long long R, int N1, int N2, void *workspace, size_t workspace_bytes, epn_stream_t stream) {
    return tn_entry(X, ldx, Y, ldy, C, ldc, R, N1, N2, workspace, workspace_bytes, 1, stream);
}
extern "C" int epn_gemm_tn_f16x2_f32(const float *X, long long ldx, const float *Y, long long ldy, float *C, long long ldc,
                                     long long R, int N1, int N2, const float *x_amax, const float *y_amax, void *workspace,
                                     size_t workspace_bytes, epn_stream_t stream) {
    GemmTnArgs G;
    G.X = X; G.Y = Y; G.C = C; G.part = workspace; G.part_bytes = workspace_bytes; G.R = R; G.N1 = N1; G.N2 = N2;
    G.ldx = ldx; G.ldy = ldy; G.ldc = ldc; G.ntiles = 0; G.tiles_n2 = 0; G.nsplit = 1; G.block0 = 0; G.Xp = nullptr;
    G.x_amax = x_amax; G.y_amax = y_amax;
    return launch_gemm_tn(G, 3, epn_stream(stream));
}

static void tn_fill(GemmTnBatch &B, int nprob, const epn_gemm_tn_problem *probs) {
    B.nprob = nprob; B.nblocks = 0;
    for (int i = 0; i < nprob; ++i) {
        GemmTnArgs &G = B.p[i];
        const epn_gemm_tn_problem &q = probs[i];
        G.X = q.X; G.Y = q.Y; G.C = q.C; G.part = nullptr; G.part_bytes = 0; G.R = q.R; G.N1 = q.N1; G.N2 = q.N2;
        G.ldx = q.ldx; G.ldy = q.ldy; G.ldc = q.ldc; G.ntiles = 0; G.tiles_n2 = 0; G.nsplit = 1; G.block0 = 0; G.Xp = nullptr; G.x_amax = G.y_amax = nullptr;
    }
}
extern "C" size_t epn_gemm_tn_grouped_workspace_bytes(int bf16, int nprob, const epn_gemm_tn_problem *probs) {
    if (!probs || nprob < 1 || nprob > GEMM_MAX_PROB) return 0;
    GemmTnBatch B;
    tn_fill(B, nprob, probs);
    return gemm_tn_batch_workspace(B, bf16);
}
extern "C" int epn_gemm_tn_grouped(int bf16, int nprob, const epn_gemm_tn_problem *probs, void *workspace,
                                   size_t workspace_bytes, epn_stream_t stream) {
    if (!probs) return EPN_ENULL;
    if (nprob < 1 || nprob > GEMM_MAX_PROB) return EPN_EINVAL;
    GemmTnBatch B;
    tn_fill(B, nprob, probs);
    return launch_gemm_tn_batch(B, bf16 == 2 ? 2 : (bf16 ? 1 : 0), workspace, workspace_bytes, epn_stream(stream));
}
extern "C" int epn_gemm_tn_grouped_f16x2(int nprob, const epn_gemm_tn_problem *probs, const float *const *x_amax,
                                         const float *const *y_amax, void *workspace, size_t workspace_bytes, epn_stream_t stream) {
    if (!probs) return EPN_ENULL;
    if (nprob < 1 || nprob > GEMM_MAX_PROB) return EPN_EINVAL;
    GemmTnBatch B;
    tn_fill(B, nprob, probs);
    for (int i = 0; i < nprob; ++i) {
        B.p[i].x_amax = x_amax ? x_amax[i] : nullptr;
        B.p[i].y_amax = y_amax ? y_amax[i] : nullptr;
    }
    return launch_gemm_tn_batch(B, 3, workspace, workspace_bytes, epn_stream(stream));
}
