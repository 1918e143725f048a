// Adam over every parameter of a model in two launches for gfx950: the optimiser of the three trainers
// (vgtk/vgtk/app/trainer.py:162-168, optim.Adam driven by vgtk.LearningRateScheduler).  Specification: include/epn_so3conv.h
// (epn_adam_step_f32), DESIGN.md 3.1i.
//
// The flat index space 0..n-1 is cut into chunks of ADAM_SPAN = 1024 elements; workgroup b owns the contiguous chunks
// [b K, (b + 1) K) with K = ceil(chunks / min(chunks, 2048)), so the partition depends on n alone.  Thread t of a chunk owns the
// four consecutive elements at 4 t (a "quad").
//   norm    pass A: every thread adds (s g)^2 of its quads in fp64, ascending, and counts the non-finite g; a fixed LDS tree per
//           workgroup; one fp64 partial and one count per workgroup into the workspace.  Thread 0 of workgroup 0 copies
//           counters[0] into the workspace: pass B reads the step count from there and never from the word it writes.
//   update  pass B: every workgroup adds the partials (thread i takes i, i + 256, ... ascending, then the same tree): the same
//           bits everywhere.  It forms norm, skip, c, t and the bias corrections; workgroup 0 writes info and the counters.
//           A skipped step returns here.  Otherwise each thread finds the segment of its quad (one 256-ary search per workgroup
//           for its first element, then a walk forward: a thread's quads ascend) and updates it.
// Wide and narrow accesses: a quad that lies inside one segment and inside n reads grad, exp_avg and exp_avg_sq as one 16-byte
// load each when the three flat buffers are 16-byte aligned, and the parameter as one 16-byte access when its address is; every
// other quad (a segment boundary inside it, the tail of n, a parameter off the 16-byte grid) goes element by element.  The
// arithmetic is the same on either path.  Plain stores: the lines are read again by the next step's forward pass.
// fp64 throughout on the fp32 inputs, no contraction into fused multiply-adds (the restatement in tests/adam_ref.py has none),
// one rounding per stored value; no float atomics, no ticket, no grid barrier, no allocation, no host synchronisation.
#include <cmath>

#include "epn_reduce.h"

#pragma clang fp contract(off)

namespace {

constexpr int FT = 256;                       // threads of every workgroup here
constexpr int QUAD = 4;                       // elements per thread and chunk
constexpr int SPAN = FT * QUAD;               // elements per chunk: EPN_ADAM_SPAN
constexpr int MAX_GRID = 2048;                // workgroups at most; the partials one workgroup of pass B adds
static_assert(SPAN == EPN_ADAM_SPAN, "the header states the chunk length");

// the workspace: a header, then one partial sum and one count per workgroup of pass A
struct Header {
    int32_t steps_applied;                    // counters[0] as pass A found it
    int32_t pad[15];
};
constexpr size_t WS_BYTES = sizeof(Header) + MAX_GRID * (sizeof(double) + sizeof(unsigned long long));

struct Plan {
    long long n, chunks;
    int per_block, grid;                      // K and the workgroups that own at least one chunk
};

Plan make_plan(long long n) {
    Plan p;
    p.n = n;
    p.chunks = (n + SPAN - 1) / SPAN;
    const long long g = p.chunks < MAX_GRID ? p.chunks : MAX_GRID;
    const long long k = (p.chunks + g - 1) / g;
    p.per_block = (int)k;                     // n < 2^40: at most 2^19
    p.grid = (int)((p.chunks + k - 1) / k);
    return p;
}

__global__ __launch_bounds__(FT) void adam_norm_kernel(const float *__restrict__ grad, long long n, int per_block, int wide,
                                                       double s, const int32_t *__restrict__ counters, Header *__restrict__ hdr,
                                                       double *__restrict__ partial, unsigned long long *__restrict__ bad) {
    __shared__ double buf[FT];
    __shared__ unsigned long long cbuf[FT];
    const long long c0 = (long long)blockIdx.x * per_block;
    double acc = 0.0;
    unsigned long long nbad = 0;
#pragma unroll 4
    for (int k = 0; k < per_block; ++k) {
        const long long i0 = (c0 + k) * SPAN + (long long)threadIdx.x * QUAD;
        if (i0 >= n) break;
        float g[QUAD];
        const int cnt = n - i0 < QUAD ? (int)(n - i0) : QUAD;
        if (wide && cnt == QUAD) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(grad + i0);
            g[0] = v.x, g[1] = v.y, g[2] = v.z, g[3] = v.w;
        } else {
            for (int j = 0; j < QUAD; ++j) g[j] = j < cnt ? grad[i0 + j] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < QUAD; ++j) {
            const double sg = s * (double)g[j];
            acc += sg * sg;
            nbad += isfinite(g[j]) ? 0 : 1;
        }
    }
    const double sum = epn_block_sum<FT>(acc, buf);
    const unsigned long long cnt = epn_block_sum<FT>(nbad, cbuf);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = sum;
        bad[blockIdx.x] = cnt;
        if (blockIdx.x == 0) hdr->steps_applied = counters[0];
    }
}

struct Hyper {
    double beta1, beta2, eps, weight_decay, grad_scale, max_norm;
};

// the segment of flat index i, walking forward from s: seg_off[s] <= i is known.  The walk never leaves the table, whatever
// the table holds
__device__ __forceinline__ int walk(const long long *__restrict__ seg_off, int nseg, int s, long long i, long long &start,
                                    long long &end) {
    while (i >= end && s + 1 < nseg) {
        ++s;
        start = end;
        end = seg_off[s + 1];
    }
    return s;
}

__global__ __launch_bounds__(FT) void adam_update_kernel(const unsigned long long *__restrict__ seg_param,
                                                         const long long *__restrict__ seg_off, int nseg, long long n,
                                                         int per_block, int nparts, int wide, const float *__restrict__ grad,
                                                         float *__restrict__ exp_avg, float *__restrict__ exp_avg_sq,
                                                         const float *__restrict__ lr_dev, Hyper h, int32_t *__restrict__ counters,
                                                         float *__restrict__ info, const Header *__restrict__ hdr,
                                                         const double *__restrict__ partial,
                                                         const unsigned long long *__restrict__ bad) {
    __shared__ double buf[FT];
    __shared__ unsigned long long cbuf[FT];
    const int tid = threadIdx.x;
    double part = 0.0;
    unsigned long long nb = 0;
    for (int j = tid; j < nparts; j += FT) {
        part += partial[j];
        nb += bad[j];
    }
    const double sumsq = epn_block_sum<FT>(part, buf);
    const unsigned long long nbad = epn_block_sum<FT>(nb, cbuf);
    const double norm = sqrt(sumsq);
    const bool skip = nbad > 0 || !isfinite(norm);
    double c = 1.0;
    if (h.max_norm > 0.0 && h.max_norm < INFINITY) {
        const double q = h.max_norm / (norm + 1e-6);
        if (q < 1.0) c = q;                                  // a NaN quotient compares false: c stays 1
    }
    const float lr32 = lr_dev[0];
    const int t0 = hdr->steps_applied;
    if (blockIdx.x == 0 && tid == 0) {
        info[0] = (float)norm;
        info[1] = (float)c;
        info[2] = lr32;
        info[3] = skip ? 1.0f : 0.0f;
        if (skip)
            counters[1] += 1;                                // read and written by this thread alone
        else
            counters[0] = t0 + 1;                            // every workgroup reads the copy in the workspace instead
    }
    if (skip) return;

    const double t = (double)t0 + 1.0;
    const double bias1 = 1.0 - pow(h.beta1, t), bias2 = 1.0 - pow(h.beta2, t);
    const double step_size = (double)lr32 / bias1, root2 = sqrt(bias2);
    const double sc = h.grad_scale * c, omb1 = 1.0 - h.beta1, omb2 = 1.0 - h.beta2;

    const long long c0 = (long long)blockIdx.x * per_block;
    const long long first = c0 * SPAN;
    if (first >= n) return;
    // the segment of the workgroup's first element: the largest s with seg_off[s] <= first, 256 probes per round
    int lo = 0, hi = nseg;
    while (hi - lo > 1) {
        const int step = (hi - lo + FT - 1) / FT;
        const long long idx = (long long)lo + (long long)tid * step;
        const int below = idx < hi && seg_off[idx] <= first;
        const int cnt = __syncthreads_count(below);          // seg_off[lo] <= first: at least one
        lo += (cnt - 1) * step;
        hi = lo + step < hi ? lo + step : hi;
    }
    int s = lo;
    long long start = seg_off[s], end = seg_off[s + 1];

    for (int k = 0; k < per_block; ++k) {
        const long long i0 = (c0 + k) * SPAN + (long long)tid * QUAD;
        if (i0 >= n) break;
        const int cnt = n - i0 < QUAD ? (int)(n - i0) : QUAD;
        s = walk(seg_off, nseg, s, i0, start, end);
        const bool whole = cnt == QUAD && i0 + QUAD <= end;   // inside n and inside one segment
        float g[QUAD], m[QUAD], v[QUAD], p[QUAD];
        float *pp[QUAD];
        if (wide && cnt == QUAD) {
            const f32x4 a = *reinterpret_cast<const f32x4 *>(grad + i0);
            const f32x4 b = *reinterpret_cast<const f32x4 *>(exp_avg + i0);
            const f32x4 d = *reinterpret_cast<const f32x4 *>(exp_avg_sq + i0);
            g[0] = a.x, g[1] = a.y, g[2] = a.z, g[3] = a.w;
            m[0] = b.x, m[1] = b.y, m[2] = b.z, m[3] = b.w;
            v[0] = d.x, v[1] = d.y, v[2] = d.z, v[3] = d.w;
        } else {
            for (int j = 0; j < QUAD; ++j) {
                g[j] = j < cnt ? grad[i0 + j] : 0.0f;
                m[j] = j < cnt ? exp_avg[i0 + j] : 0.0f;
                v[j] = j < cnt ? exp_avg_sq[i0 + j] : 0.0f;
            }
        }
        float *base = reinterpret_cast<float *>(seg_param[s]) + (i0 - start);
        const bool pwide = whole && (reinterpret_cast<uintptr_t>(base) & 15) == 0;
        if (pwide) {
            const f32x4 a = *reinterpret_cast<const f32x4 *>(base);
            p[0] = a.x, p[1] = a.y, p[2] = a.z, p[3] = a.w;
        } else if (whole) {
            for (int j = 0; j < QUAD; ++j) {
                pp[j] = base + j;
                p[j] = base[j];
            }
        } else {
            int sj = s;
            long long sa = start, se = end;
            for (int j = 0; j < QUAD; ++j) {
                pp[j] = nullptr;
                p[j] = 0.0f;
                if (j < cnt) {
                    sj = walk(seg_off, nseg, sj, i0 + j, sa, se);
                    pp[j] = reinterpret_cast<float *>(seg_param[sj]) + (i0 + j - sa);
                    p[j] = *pp[j];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < QUAD; ++j) {
            const double gd = sc * (double)g[j] + h.weight_decay * (double)p[j];
            m[j] = (float)(h.beta1 * (double)m[j] + omb1 * gd);
            v[j] = (float)(h.beta2 * (double)v[j] + omb2 * (gd * gd));
            const double den = sqrt((double)v[j]) / root2 + h.eps;
            p[j] = (float)((double)p[j] - step_size * (double)m[j] / den);
        }
        if (wide && cnt == QUAD) {
            *reinterpret_cast<f32x4 *>(exp_avg + i0) = f32x4{m[0], m[1], m[2], m[3]};
            *reinterpret_cast<f32x4 *>(exp_avg_sq + i0) = f32x4{v[0], v[1], v[2], v[3]};
        } else {
            for (int j = 0; j < cnt; ++j) {
                exp_avg[i0 + j] = m[j];
                exp_avg_sq[i0 + j] = v[j];
            }
        }
        if (pwide) {
            *reinterpret_cast<f32x4 *>(base) = f32x4{p[0], p[1], p[2], p[3]};
        } else {
            for (int j = 0; j < cnt; ++j) *pp[j] = p[j];
        }
    }
}

size_t adam_workspace_bytes(long long n) {
    (void)n;                                  // the partials are bounded by the grid, not by n
    return WS_BYTES;
}

bool adam_sizes_ok(int nseg, long long n) { return nseg >= 1 && nseg <= 65536 && n >= 1 && n < (1LL << 40) && nseg <= n; }

}  // namespace

extern "C" size_t epn_adam_workspace_bytes(long long n) { return adam_workspace_bytes(n); }

extern "C" int epn_adam_check_plan(const unsigned long long *seg_param, const long long *seg_off, int nseg, long long n) {
    if (!(nseg >= 1 && nseg <= 65536 && n >= 1 && n < (1LL << 40))) return EPN_EINVAL;
    if (!seg_param || !seg_off) return EPN_ENULL;
    if (seg_off[0] != 0 || seg_off[nseg] != n) return EPN_EINVAL;
    for (int s = 0; s < nseg; ++s)
        if (seg_off[s + 1] <= seg_off[s] || seg_param[s] == 0 || (seg_param[s] & 3) != 0) return EPN_EINVAL;
    return 0;
}

// Every refusal is decided before the first HIP runtime call.  Sizes and hyper-parameters first (EPN_EINVAL; the comparisons
// are written so that a NaN fails them), then pointers (EPN_ENULL), then the workspace
extern "C" int epn_adam_step_f32(const unsigned long long *seg_param, const long long *seg_off, int nseg, long long n,
                                 const float *grad, float *exp_avg, float *exp_avg_sq, const float *lr, double beta1,
                                 double beta2, double eps, double weight_decay, double grad_scale, double max_norm,
                                 int32_t *counters, float *info, void *workspace, size_t workspace_bytes, epn_stream_t stream) {
    if (!adam_sizes_ok(nseg, n)) return EPN_EINVAL;
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return EPN_EINVAL;
    if (!(eps > 0.0 && eps < INFINITY) || !(weight_decay >= 0.0 && weight_decay < INFINITY)) return EPN_EINVAL;
    if (!(grad_scale >= 0.0 && grad_scale < INFINITY) || max_norm != max_norm) return EPN_EINVAL;
    if (!seg_param || !seg_off || !grad || !exp_avg || !exp_avg_sq || !lr || !counters || !info) return EPN_ENULL;
    if (!workspace || workspace_bytes < adam_workspace_bytes(n) || (reinterpret_cast<uintptr_t>(workspace) & 7) != 0)
        return EPN_EWORKSPACE;
    hipStream_t st = epn_stream(stream);
    const Plan p = make_plan(n);
    Header *hdr = static_cast<Header *>(workspace);
    double *partial = reinterpret_cast<double *>(hdr + 1);
    unsigned long long *bad = reinterpret_cast<unsigned long long *>(partial + MAX_GRID);
    const auto aligned = [](const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    const int wide_g = aligned(grad), wide = wide_g && aligned(exp_avg) && aligned(exp_avg_sq);
    const dim3 grid((unsigned)p.grid), block(FT);
    EPN_LAUNCH_AUX(adam_norm_kernel, grid, block, 0, st, grad, n, p.per_block, wide_g, grad_scale, counters, hdr, partial, bad);
    EPN_CHECK_LAUNCH();
    const Hyper h{beta1, beta2, eps, weight_decay, grad_scale, max_norm};
    EPN_LAUNCH(adam_update_kernel, grid, block, 0, st, seg_param, seg_off, nseg, n, p.per_block, p.grid, wide, grad, exp_avg,
               exp_avg_sq, lr, h, counters, info, hdr, partial, bad);
    EPN_CHECK_LAUNCH();
    return 0;
}
