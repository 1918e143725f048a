// Weight contractions of BasicSO3Conv (vgtk/vgtk/so3conv/modules.py:48-55: `W @ feats.view(b, c*ks, p*a)`) and of its
// autograd transposes, as hand-written MFMA GEMMs for gfx950 -- round 1 handed these to the BLAS library.
//
//   NT   C[M][N]   = A[M][K] . Bt[N][K]^T      activation x weight: out = G W^T, dG = dOut (W^T)^T, the spectral blocks
//   TN   C[N1][N2] = X[R][N1]^T . Y[R][N2]     weight gradients: dW = dOut^T G (contraction over the R = b*p*a columns)
//
// This file holds the NT kernel, its instance table (EPN_NT_INSTANCES) with the selection rule (nt_choose), the generic
// fallbacks and the cast / transpose kernels; the TN family is gemm_tn.hip, the tile planner and the marshalling of the entry
// points' problems are in gemm.h (nt_plan_tiles, nt_marshal / nt_for_chunks).  Both stream 128-byte row segments through a double-buffered LDS ring with direct-to-LDS loads
// (global_load_lds_dwordx4, one 1 KiB wave instruction = 8 row segments), one barrier per K step.  The NT image is
// XOR-swizzled on the SOURCE address (16-byte slot ^ ((row >> 1) & 7)) so that the ds_read_b128 fragment reads are
// bank-conflict free (cdna_hip_programming.md T2 / rule 21); the TN image is read along its rows and needs none.
// fp32 uses v_mfma_f32_32x32x2_f32 (exact f32, 64 FLOP/clk/SIMD): one ds_read_b128 per operand tile feeds FOUR MFMAs
// because the contraction index may be visited in any order as long as both operands agree (lane group j of a step
// holds k = 8s + 4j .. +3).  bf16 uses v_mfma_f32_32x32x16_bf16 (NT, one b128 = one operand) and
// v_mfma_f32_16x16x32_bf16 fed by ds_read_b64_tr_b16 transposed reads (TN), fp32 accumulation throughout.
#include "conv_internal.h"
#include "gemm.h"

namespace epn {
namespace {
__device__ __forceinline__ void store_out(float *p, float v) { *p = v; }
__device__ __forceinline__ void store_out(__bf16 *p, float v) { *p = (__bf16)v; }

// ------------------------------------------------------------------------------------------------ NT
// Block tile BM x BN = (WGM*TM*32) x (WGN*TN*32), WGM*WGN waves, each wave TM x TN MFMA tiles of 32x32.
// K step = KS 16-byte slots of a row: KS = 8 (128 bytes: 32 floats / 64 bf16) or, for contraction lengths that are
// only a multiple of half that (the 32-channel layers in bf16), KS = 4.
template <typename T, typename TO, int WGM, int WGN, int TM, int TN, int KS = 8, int NSTG = 2>
__global__ __launch_bounds__(64 * WGM * WGN) void gemm_nt_kernel(GemmNtBatch B) {
    constexpr int NW = WGM * WGN;
    constexpr int BM = WGM * TM * 32, BN = WGN * TN * 32;
    constexpr int ROWS = BM + BN;                  // LDS rows per stage (A rows, then Bt rows)
    constexpr int ROWB = KS * 16;                  // bytes per LDS row
    constexpr int RPG = 64 / KS;                   // rows per wave-level load instruction (1 KiB)
    constexpr int NG = ROWS / RPG;                 // wave-level load instructions per stage
    constexpr int GPW = (NG + NW - 1) / NW;        // ... per wave
    constexpr int E16 = ElemOf<T>::PER16;          // elements per 16-byte slot
    constexpr int BKE = KS * E16;                  // elements per K step
    constexpr int NS = KS / 2;                     // fragment steps per K step (two slots each: lane groups j = 0, 1)
    __shared__ __attribute__((aligned(1024))) char smem[NSTG * ROWS * ROWB];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    EPN_NT_DECODE(B)                               // ---- which problem / tile: P, m0, n0 (gemm.h, with the plan it reads)
    const T *__restrict__ A = static_cast<const T *>(P.A);
    const T *__restrict__ Bt = static_cast<const T *>(P.Bt);
    const int nk = P.K / BKE;

    // ---- staging pointers: group g covers LDS rows 8g .. 8g+7; lane -> (row 8g + lane/8, physical slot lane%8)
    const T *src[GPW];
#pragma unroll
    for (int i = 0; i < GPW; ++i) {
        const int g = wave + i * NW;
        const int r = RPG * g + lane / KS;                     // LDS row
        // logical 16-byte slot stored at physical slot lane % KS (conflict-free ds_read_b128 of 32 consecutive rows)
        const int slot = (lane % KS) ^ (KS == 8 ? (r >> 1) & 7 : (r >> 2) & 3);
        if (r < BM) {
            long long gr = m0 + r;
            gr = gr < P.M ? gr : P.M - 1;
            src[i] = A + gr * P.lda + slot * E16;
        } else {
            int gn = n0 + (r - BM);
            gn = gn < P.N ? gn : P.N - 1;
            src[i] = Bt + (long long)gn * P.ldb + slot * E16;
        }
    }
    auto stage_one = [&](int buf, int i) {
        const int g = wave + i * NW;
        if (NG % NW == 0 || g < NG) {
            glds16(src[i], smem + buf * (ROWS * ROWB) + g * 1024);
            src[i] += BKE;
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int i = 0; i < GPW; ++i) stage_one(buf, i);
    };
    // waves w and w + 4 of an 8-wave workgroup share a SIMD: their loads go to alternating MFMA groups (below)
    const int wpar = NW == 8 ? __builtin_amdgcn_readfirstlane(wave >> 2) : 0;

    const int wm = wave / WGN, wn = wave % WGN;
    const int li = lane & 31, lj = lane >> 5;
    const int fsw = KS == 8 ? (li >> 1) & 7 : (li >> 2) & 3;
    // byte offsets of this lane's fragment rows inside a stage
    int aoff[TM], boff[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) aoff[i] = ((wm * TM + i) * 32 + li) * ROWB;
#pragma unroll
    for (int i = 0; i < TN; ++i) boff[i] = (BM + (wn * TN + i) * 32 + li) * ROWB;

    f32x16 acc[TM][TN];
    EPN_NT_ZERO_ACC(acc)

    // One barrier per K step.  A direct-to-LDS load costs its wave ~60-180 cycles of issue during which it feeds no MFMA,
    // and the two waves of a SIMD leave the barrier together: issued as one burst (wherever in the step) both waves
    // stall at once and the matrix pipe idles ~7 % (measured, tools/gemm_lab).  So the next stage's loads are spread
    // one per MFMA group over the step, the partner waves on alternating groups (sched_barrier pins the placement; left
    // alone the compiler hoists all of them in front of the first ds_read).  fp32: +3 % over the burst; bf16 is
    // HBM-bound on these shapes and keeps the burst.
    constexpr int NGRP = 4 * NS;               // fp32: MFMA groups per K step (NS fragment steps x 4 contraction pairs)
    constexpr bool BURST = sizeof(T) != 4 || BN <= 64;   // HBM-bound shapes: the whole next stage is requested at once
    static_assert(NSTG == 2 || (NSTG == 3 && BURST && NG % NW == 0), "the 3-stage ring is for the burst (HBM-bound) configurations");
    stage(0);
    if constexpr (NSTG == 3) {
        if (nk > 1) stage(1);
    }
    for (int kt = 0; kt < nk; ++kt) {
        const bool more = kt + 1 < nk;
        if constexpr (NSTG == 3) {
            // Two stages in flight (HBM-bound operands: one stage of bytes per CU does not cover the loaded latency):
            // stage kt must have landed, stage kt+1 (this wave's GPW youngest loads) may still be on its way.
            if (more) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(GPW) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
        } else {
            __syncthreads();                   // stage kt has landed (vmcnt(0) rides on the barrier); buffer (kt+1)&1 is free
        }
        const char *base = smem + (kt % NSTG) * (ROWS * ROWB);
        if constexpr (BURST) {
            if constexpr (NSTG == 3) {
                if (kt + 2 < nk) stage((kt + 2) % 3);      // buffer of step kt-1: every wave is past it (barrier above)
            } else {
                if (more) stage((kt + 1) & 1);
            }
        }
        if constexpr (sizeof(T) == 4) {
            // fragments of step s+1 are read while the MFMAs of step s issue (two register sets, static indices)
            f32x4 a[2][TM], b[2][TN];
            auto rd = [&](int s, int set) {
                const int so = ((2 * s + lj) ^ fsw) * 16;
#pragma unroll
                for (int i = 0; i < TM; ++i) a[set][i] = *reinterpret_cast<const f32x4 *>(base + aoff[i] + so);
#pragma unroll
                for (int i = 0; i < TN; ++i) b[set][i] = *reinterpret_cast<const f32x4 *>(base + boff[i] + so);
            };
            rd(0, 0);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                if (s + 1 < NS) rd(s + 1, (s + 1) & 1);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    __builtin_amdgcn_sched_barrier(0);
                    if (more && !BURST) {
                        const int grp = 4 * s + e;
#pragma unroll
                        for (int i = 0; i < GPW; ++i) {
                            const int g0 = 1 + (i * (NGRP - 2)) / GPW;             // group of load i, first wave of a SIMD
                            const int g1 = g0 + 1 < NGRP ? g0 + 1 : NGRP - 1;      // ... its partner, one group later
                            if ((g0 == grp && wpar == 0) || (g1 == grp && wpar != 0)) stage_one((kt + 1) & 1, i);
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s & 1][i][e], b[s & 1][j][e], acc[i][j], 0, 0, 0);
                }
            }
        } else {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int so = ((2 * s + lj) ^ fsw) * 16;
                bf16x8 a[TM], b[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) a[i] = *reinterpret_cast<const bf16x8 *>(base + aoff[i] + so);
#pragma unroll
                for (int i = 0; i < TN; ++i) b[i] = *reinterpret_cast<const bf16x8 *>(base + boff[i] + so);
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
            }
        }
    }

    // ---- epilogue: D[row = (r&3) + 8 (r>>2) + 4 lj][col = li]
    TO *__restrict__ C = static_cast<TO *>(P.C);
    if (P.stats) nt_col_stats<TM, TN, TO>(acc, P.stats, P.M, P.N, m0 + wm * TM * 32, n0 + wn * TN * 32, li, lj);
    if (P.c_amax) nt_c_amax<TM, TN, TO>(acc, P.c_amax);
    if (m0 + BM <= P.M && n0 + BN <= P.N && (long long)BM * P.ldc < (1LL << 30)) {
        // interior tile: wave-uniform base + 32-bit lane offset; one scalar multiply and one vector add per output row.
        // (The checked form below costs ~15 VALU instructions per element -- 128 elements per lane: measured as a fixed
        // ~8 us per 256 x 256 tile, a third of the run time of the short-K data-gradient GEMMs.)
        TO *__restrict__ cw = C + (size_t)(m0 + wm * TM * 32) * P.ldc + (n0 + wn * TN * 32);
        const unsigned ldc = (unsigned)P.ldc;
        const unsigned lane_off = 4u * lj * ldc + li;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const unsigned o = lane_off + (unsigned)(i * 32 + (r & 3) + 8 * (r >> 2)) * ldc;
#pragma unroll
                for (int j = 0; j < TN; ++j) store_out(cw + o + j * 32, acc[i][j][r]);
            }
        return;
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + (wn * TN + j) * 32 + li;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long long m = m0 + (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lj;
                if (m < P.M && n < P.N) store_out(C + m * P.ldc + n, acc[i][j][r]);
            }
        }
}


// ------------------------------------------------------------------------------------------------ small helpers
// dst[c][r] = (TO) src[r][c]   (weights only: a few MB at most)
template <typename TI, typename TO>
__global__ void transpose_cast_kernel(const TI *__restrict__ src, TO *__restrict__ dst, int rows, int cols) {
    __shared__ float tile[32][33];
    const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
    for (int i = threadIdx.y; i < 32; i += blockDim.y) {
        const int r = by + i, c = bx + threadIdx.x;
        tile[i][threadIdx.x] = (r < rows && c < cols) ? (float)src[(size_t)r * cols + c] : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.y; i < 32; i += blockDim.y) {
        const int c = bx + i, r = by + threadIdx.x;
        if (r < rows && c < cols) dst[(size_t)c * rows + r] = (TO)tile[threadIdx.x][i];
    }
}

template <typename TI, typename TO>
__global__ void cast_scalar_kernel(const TI *__restrict__ src, TO *__restrict__ dst, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        dst[i] = (TO)(float)src[i];
}

// four elements per thread and step (16 / 8-byte accesses; both pointers 16-byte aligned: launcher), scalar tail.
// ADD: dst = (TO)(src + (float)add[i]) -- the fp32 scatter target of a bf16 network's data gradient converted and added to the
// gradient that reached the same tensor by the other branch, in one pass
template <typename TI, typename TO, bool ADD = false>
__global__ void cast_kernel(const TI *__restrict__ src, TO *__restrict__ dst, size_t n, const TO *__restrict__ add = nullptr) {
    typedef TI vin __attribute__((ext_vector_type(4)));
    typedef TO vout __attribute__((ext_vector_type(4)));
    const size_t n4 = n >> 2, stride = (size_t)gridDim.x * blockDim.x, t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (size_t i = t0; i < n4; i += stride) {
        const vin v = reinterpret_cast<const vin *>(src)[i];
        float f[4] = {(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
        if constexpr (ADD) {
            const vout a = reinterpret_cast<const vout *>(add)[i];
#pragma unroll
            for (int q = 0; q < 4; ++q) f[q] += (float)a[q];
        }
        reinterpret_cast<vout *>(dst)[i] = vout{(TO)f[0], (TO)f[1], (TO)f[2], (TO)f[3]};
    }
    for (size_t i = 4 * n4 + t0; i < n; i += stride) {
        float f = (float)src[i];
        if constexpr (ADD) f += (float)add[i];
        dst[i] = (TO)f;
    }
}

// column statistics of the generic path: one thread per (32-row block, column) reads C back
template <typename TO>
__global__ void nt_stats_from_c_kernel(const TO *__restrict__ C, long long M, int N, long long ldc, float *__restrict__ part) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (M >> 5) * N) return;
    const long long rb = i / N;
    const int n = (int)(i % N);
    float s1 = 0.f, s2 = 0.f;
    for (int r = 0; r < 32; ++r) {
        const float v = (float)C[(rb * 32 + r) * ldc + n];
        s1 += v;
        s2 = fmaf(v, v, s2);
    }
    part[i * 2] = s1;
    part[i * 2 + 1] = s2;
}

// generic fallbacks (any shape, VALU): one thread per output element
template <typename T, typename TO>
__global__ void gemm_nt_generic_kernel(const T *__restrict__ A, const T *__restrict__ Bt, TO *__restrict__ C, long long M,
                                       int N, int K, long long lda, long long ldb, long long ldc) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * N) return;
    const long long m = i / N;
    const int n = (int)(i % N);
    float s = 0.f;
    for (int k = 0; k < K; ++k) s = fmaf((float)A[m * lda + k], (float)Bt[(long long)n * ldb + k], s);
    store_out(C + m * ldc + n, s);
}
// generic path: max|C| by a pass over C (the MFMA kernels take it from their accumulators, gemm.h nt_c_amax)
template <typename TO>
__global__ __launch_bounds__(256) void nt_amax_from_c_kernel(const TO *__restrict__ C, long long M, int N, long long ldc, unsigned *__restrict__ out) {
    unsigned m = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < M * N; i += (long long)gridDim.x * 256) {
        const unsigned a = __builtin_bit_cast(unsigned, (float)C[(i / N) * ldc + i % N]) & 0x7fffffffu;
        m = (a > m && a < 0x7f800000u) ? a : m;
    }
    EPN_WAVE_UMAX(m)
    if ((threadIdx.x & 63) == 0 && m > __atomic_load_n(out, __ATOMIC_RELAXED)) atomicMax(out, m);
}
template <typename T, typename TO, int WGM, int WGN, int TM, int TN, int KS = 8, int NSTG = 2>
int launch_nt_cfg(GemmNtBatch &B, hipStream_t st) {
    const unsigned total = nt_plan_tiles(B, WGM * TM * 32, WGN * TN * 32);
    if (total == 0) return 0;
    EPN_LAUNCH((gemm_nt_kernel<T, TO, WGM, WGN, TM, TN, KS, NSTG>), dim3(total), dim3(64 * WGM * WGN), 0, st, B);
    EPN_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------------------------ the kernel instances
// Every gemm_nt_kernel<T, TO, ...> instance the library contains is named ONCE, here, for every operand / output type pair:
// X(code, WGM, WGN, TM, TN, KS, NSTG); block tile (WGM*TM*32) x (WGN*TN*32); code = policy code of the tuning override
// (tools/gemm_bench.py --cfg), 0 = none.  nt_choose() names a tuple; launch_nt_instance() looks it up and fails with EPN_EINVAL
// when there is none.  "override only": instantiated, but no rule of nt_choose reaches it for any type (kept: the code object
// stays what it was).  256 x 64 and 128 x 128 are rule tiles of fp32 only, 256 x 128 (two stages) too: under bf16 operands
// only the override reaches them.
#ifdef EPN_TUNING
// short-K (data-gradient) shapes: four-wave workgroups with 128 accumulators per wave and a half-width K step, so that TWO
// fit a CU and one's store epilogue overlaps the other's loads (round 6 sweep, tools/r06_dg_sweep.sh ->
// profiles/r06_bf16_dg_tile_sweep.txt).  MEASURED 25-30 % SLOWER than the 256 x 256 tile on every bf16 data-gradient
// shape (245760 x 3072 x 256: 0.76-0.79 vs 0.60 ms; hipBLASLt through torch.mm: 0.60-0.62): kept for the record only
#define EPN_NT_TUNING_INSTANCES(X)                                                                                   \
    X(7, 2, 2, 2, 4, 4, 2)  /* 128 x 256, 4 waves, K step 32 (bf16) / 16 (fp32), 48 KB */                            \
    X(8, 2, 2, 4, 2, 4, 2)  /* 256 x 128, 4 waves, same */                                                           \
    X(10, 2, 2, 2, 4, 8, 2) /* 128 x 256, 4 waves, full K step (96 KB: one workgroup per CU) */
#else
#define EPN_NT_TUNING_INSTANCES(X)
#endif
#define EPN_NT_INSTANCES(X)                                                                                          \
    X(0, 8, 1, 2, 1, 4, 2)  /* 512 x  32, half K step */                                                             \
    X(0, 8, 1, 2, 2, 4, 2)  /* 512 x  64, half K step */                                                             \
    X(0, 4, 2, 2, 2, 4, 2)  /* 256 x 128, half K step */                                                             \
    X(0, 8, 1, 2, 1, 8, 2)  /* 512 x  32 */                                                                          \
    X(0, 8, 1, 2, 2, 8, 2)  /* 512 x  64 */                                                                          \
    X(1, 4, 2, 2, 2, 8, 2)  /* 256 x 128, 8 waves */                                                                 \
    X(2, 4, 2, 2, 4, 8, 2)  /* 256 x 256, 8 waves */                                                                 \
    X(3, 2, 2, 2, 2, 8, 2)  /* 128 x 128, 4 waves (2 workgroups / CU) */                                             \
    X(4, 2, 4, 2, 2, 8, 2)  /* 128 x 256, 8 waves: override only */                                                  \
    X(5, 4, 1, 2, 2, 8, 2)  /* 256 x  64, 4 waves */                                                                 \
    X(6, 2, 2, 4, 2, 8, 2)  /* 256 x 128, 4 waves, 128 x 64 per wave: override only */                               \
    EPN_NT_TUNING_INSTANCES(X)
// bf16 operands only (the kernel's static_assert rejects a three-stage ring for fp32 tiles wider than 64)
#define EPN_NT_BF16_INSTANCES(X) X(0, 4, 2, 2, 2, 8, 3) /* 256 x 128, three stages */

struct NtTile { int wgm, wgn, tm, tn, ks, nstg; };

// The selection rule of the MFMA path.  half_k: some K is a multiple of 4 slots only; M0: rows of problem 0; policy: kernel_policy()
inline NtTile nt_choose(bool is_fp32, int nprob, int maxn, int minn, bool half_k, long long M0, int policy) {
    if (half_k) {
        if (maxn <= 32) return {8, 1, 2, 1, 4, 2};
        if (maxn <= 64) return {8, 1, 2, 2, 4, 2};
        return {4, 2, 2, 2, 4, 2};
    }
    if ((policy & ~0xff) == 0x100) {           // tuning override (tools/gemm_bench.py --cfg); a code without entry: the rules
#define EPN_NT_CODE(CODE, ...) if (CODE != 0 && (policy & 0xff) == CODE) return {__VA_ARGS__};
        EPN_NT_INSTANCES(EPN_NT_CODE)
#undef EPN_NT_CODE
    }
    if (is_fp32 && nprob == 1 && maxn >= 128 && maxn <= 256 && maxn % 128 == 0 && (M0 / 128) * (maxn / 128) >= 3840)
        // many-tile problems: 128 x 128 tiles, 4 waves, two workgroups per CU (measured on 491520 x 128 and 245760 x 256:
        // 130-140 TFLOP/s against 124-136 for the 256-row tiles; below ~3840 tiles the big tiles win)
        return {2, 2, 2, 2, 8, 2};
    if (is_fp32 && nprob > 1) {
        // grouped spectral blocks (widths d*c, d = 1, 3, 3, 4, 5): narrow tiles waste less of the ragged widths
        // (c = 64: 256 x 64 tiles 0.40 ms vs 0.45; c = 128 / 256: 128 x 128 tiles 0.65 / 1.22 vs 0.69 / 1.25, measured)
        if (maxn <= 320 && minn <= 64) return {4, 1, 2, 2, 8, 2};
        return {2, 2, 2, 2, 8, 2};
    }
    if (maxn <= 32) return {8, 1, 2, 1, 8, 2};      // 512 x 32
    if (maxn <= 64) return {8, 1, 2, 2, 8, 2};      // 512 x 64
    // 256 x 256 (fewer LDS fragment reads per MFMA: 6 per 8 instead of 4 per 4).  bf16 too: 11-12 % faster
    // than the 3-stage 256 x 128 instance on the N >= 256 shapes (245760 x 256 x 6144: 0.92 -> 0.82 ms)
    if (minn >= 256) return {4, 2, 2, 4, 8, 2};   // (fp32 groups were routed above)
    // 256 x 128.  bf16 is HBM-bound on these shapes (it streams G or dG): a THREE-stage LDS ring keeps two stages of loads
    // in flight (144 KB of LDS; the wait before the barrier is vmcnt(loads of one stage), not 0): 10-16 % faster on the
    // schedule's shapes (245760 x 256 x 6144: 1.07 -> 0.93 ms).  Narrow tiles and fp32 (MFMA-bound) measured no gain.
    if (!is_fp32) return {4, 2, 2, 2, 8, 3};
    return {4, 2, 2, 2, 8, 2};
}

// launches the instance `c` names; EPN_EINVAL when the tables above have none for this type pair
template <typename T, typename TO>
int launch_nt_instance(const NtTile &c, GemmNtBatch &B, hipStream_t st) {
#define EPN_NT_TRY(CODE, WGM, WGN, TM, TN, KS, NSTG)                                                                 \
    if (c.wgm == WGM && c.wgn == WGN && c.tm == TM && c.tn == TN && c.ks == KS && c.nstg == NSTG)                    \
        return launch_nt_cfg<T, TO, WGM, WGN, TM, TN, KS, NSTG>(B, st);
    EPN_NT_INSTANCES(EPN_NT_TRY)
    if constexpr (sizeof(T) == 2) { EPN_NT_BF16_INSTANCES(EPN_NT_TRY) }
#undef EPN_NT_TRY
    return EPN_EINVAL;
}

template <typename T, typename TO>
int launch_nt_typed(GemmNtBatch &B, hipStream_t st) {
    constexpr int E16 = ElemOf<T>::PER16;
    bool fast = true, half_k = false;
    int maxn = 0, minn = 1 << 30;
    for (int i = 0; i < B.nprob; ++i) {
        const GemmNtProb &p = B.p[i];
        if (p.M < 0 || p.N < 1 || p.K < 1 || (p.stats && p.M % 32)) return EPN_EINVAL;
        if (!p.Bt || (p.M > 0 && (!p.A || !p.C))) return EPN_ENULL;     // (an empty problem has nothing to point at)
        if (p.K % (4 * E16) || p.lda % E16 || p.ldb % E16 || ((uintptr_t)p.A & 15) || ((uintptr_t)p.Bt & 15)) fast = false;
        if (p.K % (8 * E16)) half_k = true;      // K a multiple of 4 slots only: the short-K-step kernels
        maxn = p.N > maxn ? p.N : maxn;
        minn = p.N < minn ? p.N : minn;
    }
    if (!fast) {
        for (int i = 0; i < B.nprob; ++i) {
            const GemmNtProb &p = B.p[i];
            if (p.M == 0) continue;
            const long long n = p.M * p.N;
            EPN_LAUNCH((gemm_nt_generic_kernel<T, TO>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                               static_cast<const T *>(p.A), static_cast<const T *>(p.Bt), static_cast<TO *>(p.C), p.M,
                               p.N, p.K, p.lda, p.ldb, p.ldc);
            EPN_CHECK_LAUNCH();
            if (p.c_amax) {
                EPN_LAUNCH_AUX((nt_amax_from_c_kernel<TO>), dim3((unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096)), dim3(256), 0, st,
                               static_cast<const TO *>(p.C), p.M, p.N, p.ldc, p.c_amax);
                EPN_CHECK_LAUNCH();
            }
            if (p.stats) {
                const long long ns = (p.M >> 5) * p.N;
                EPN_LAUNCH_AUX((nt_stats_from_c_kernel<TO>), dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, st,
                               static_cast<const TO *>(p.C), p.M, p.N, p.ldc, p.stats);
                EPN_CHECK_LAUNCH();
            }
        }
        return 0;
    }
    return launch_nt_instance<T, TO>(nt_choose(sizeof(T) == 4, B.nprob, maxn, minn, half_k, B.p[0].M, kernel_policy()), B, st);
}

}  // namespace

int launch_gemm_nt(GemmNtBatch &B, int dtype, int out_dtype, hipStream_t st) {
    if (B.nprob < 1 || B.nprob > GEMM_MAX_PROB) return EPN_EINVAL;
    if (dtype == 0 && out_dtype == 0) return launch_nt_typed<float, float>(B, st);
    if (dtype == 1 && out_dtype == 1) return launch_nt_typed<__bf16, __bf16>(B, st);
    if (dtype == 1 && out_dtype == 0) return launch_nt_typed<__bf16, float>(B, st);
    return EPN_EINVAL;
}

int launch_transpose_cast(const void *src, void *dst, int rows, int cols, int src_bf16, int dst_bf16, hipStream_t st) {
    if (rows < 1 || cols < 1) return EPN_EINVAL;
    if (!src || !dst) return EPN_ENULL;
    const dim3 grid((cols + 31) / 32, (rows + 31) / 32), blk(32, 8);
    if (!src_bf16 && !dst_bf16)
        EPN_LAUNCH((transpose_cast_kernel<float, float>), grid, blk, 0, st, (const float *)src, (float *)dst, rows, cols);
    else if (!src_bf16 && dst_bf16)
        EPN_LAUNCH((transpose_cast_kernel<float, __bf16>), grid, blk, 0, st, (const float *)src, (__bf16 *)dst, rows, cols);
    else if (src_bf16 && !dst_bf16)
        EPN_LAUNCH((transpose_cast_kernel<__bf16, float>), grid, blk, 0, st, (const __bf16 *)src, (float *)dst, rows, cols);
    else
        EPN_LAUNCH((transpose_cast_kernel<__bf16, __bf16>), grid, blk, 0, st, (const __bf16 *)src, (__bf16 *)dst, rows, cols);
    EPN_CHECK_LAUNCH();
    return 0;
}

int launch_cast(const void *src, void *dst, size_t n, int src_bf16, int dst_bf16, hipStream_t st) {
    if (n == 0) return 0;
    if (!src || !dst) return EPN_ENULL;
    // vector accesses need 16-byte aligned pointers; anything else runs the scalar tail loop over everything
    const bool al = !(((uintptr_t)src | (uintptr_t)dst) & 15);
    const size_t nv = al ? n : 0, work = al ? (n + 3) / 4 : n;
    const dim3 grid((unsigned)((work + 255) / 256 < 8192 ? (work + 255) / 256 : 8192)), blk(256);
    if (!src_bf16 && dst_bf16) {
        if (al) EPN_LAUNCH((cast_kernel<float, __bf16>), grid, blk, 0, st, (const float *)src, (__bf16 *)dst, nv, nullptr);
        else EPN_LAUNCH((cast_scalar_kernel<float, __bf16>), grid, blk, 0, st, (const float *)src, (__bf16 *)dst, n);
    } else if (src_bf16 && !dst_bf16) {
        if (al) EPN_LAUNCH((cast_kernel<__bf16, float>), grid, blk, 0, st, (const __bf16 *)src, (float *)dst, nv, nullptr);
        else EPN_LAUNCH((cast_scalar_kernel<__bf16, float>), grid, blk, 0, st, (const __bf16 *)src, (float *)dst, n);
    } else return EPN_EINVAL;
    EPN_CHECK_LAUNCH();
    return 0;
}

int launch_cast_add(const float *src, const void *add_bf16, void *dst_bf16, size_t n, hipStream_t st) {
    if (n == 0) return 0;
    if (!src || !add_bf16 || !dst_bf16) return EPN_ENULL;
    if (((uintptr_t)src | (uintptr_t)add_bf16 | (uintptr_t)dst_bf16) & 15) return EPN_EINVAL;
    const size_t work = (n + 3) / 4;
    const dim3 grid((unsigned)((work + 255) / 256 < 8192 ? (work + 255) / 256 : 8192)), blk(256);
    EPN_LAUNCH((cast_kernel<float, __bf16, true>), grid, blk, 0, st, src, (__bf16 *)dst_bf16, n, (const __bf16 *)add_bf16);
    EPN_CHECK_LAUNCH();
    return 0;
}

}  // namespace epn

using namespace epn;

static int nt_entry(int nprob, const epn_gemm_nt_problem *probs, int dtype, int out_dtype, epn_stream_t stream) {
    return nt_for_chunks(nprob, probs, nullptr,
                         [&](GemmNtBatch &B) { return launch_gemm_nt(B, dtype, out_dtype, epn_stream(stream)); });
}

extern "C" int epn_gemm_nt_f32(int nprob, const epn_gemm_nt_problem *probs, epn_stream_t stream) {
    return nt_entry(nprob, probs, 0, 0, stream);
}
extern "C" int epn_gemm_nt_bf16(int nprob, const epn_gemm_nt_problem *probs, int out_f32, epn_stream_t stream) {
    return nt_entry(nprob, probs, 1, out_f32 ? 0 : 1, stream);
}

extern "C" int epn_transpose_cast(const void *src, void *dst, int rows, int cols, int src_bf16, int dst_bf16,
                                  epn_stream_t stream) {
    return launch_transpose_cast(src, dst, rows, cols, src_bf16, dst_bf16, epn_stream(stream));
}
extern "C" int epn_cast(const void *src, void *dst, size_t n, int src_bf16, int dst_bf16, epn_stream_t stream) {
    return launch_cast(src, dst, n, src_bf16, dst_bf16, epn_stream(stream));
}
extern "C" int epn_cast_add_bf16(const float *src, const void *add, void *dst, size_t n, epn_stream_t stream) {
    return launch_cast_add(src, add, dst, n, epn_stream(stream));
}
