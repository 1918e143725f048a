// ICP refinement of a rigid transform on the dense clouds, for gfx950: the stage after the RANSAC registration
// (ransac_register.hip).  This is open3d's registration_icp (TransformationEstimationPointToPoint / PointToPlane with
// ICPConvergenceCriteria) made deterministic; it is argued from open3d's algorithm and has not been run against open3d.
// Specification: include/epn_so3conv.h (epn_icp_refine_f32) and DESIGN.md 3.1m; the grid, its cell walk and the nearest-point
// rule are point_grid.h's (nearest_member, shared with epn_point_grid_nn_f32), the arithmetic is icp_math.h's.
//
// Two launches per iteration on the call's stream, 2 * max_iter in all, and nothing else: no memset, no host synchronisation,
// no atomics.  The loop's state (T, the previous fitness and rmse, the stop flag) lives in the caller's workspace and is
// written by icp_solve only; iteration 0 reads T_init instead, so nothing has to be initialised.
//   icp_accumulate  one WAVE per source point, four per workgroup, at most ACC_GROUPS workgroups that stride over the points.
//                   A wave transforms its point (an explicit fma chain, the same in every lane), finds its nearest grid point as
//                   epn_point_grid_nn_f32 does, and lane e < 32 adds the pair's term of sum e to ONE int64 register it keeps
//                   across the wave's points: the term is a product of two of nine wave-uniform values, picked by lane once.
//                   In point-to-plane mode lanes 0..2 gather the winner's normal: one 12-byte load per wave.  At the end the
//                   four waves meet in LDS and the workgroup writes one row of 32 sums.  A launch that finds the stop flag set
//                   returns at once.
//   icp_solve       one workgroup: adds the rows (integers: any order), then one lane runs epn_icp::step and writes the state,
//                   T, the trace record, iterations and status.  A launch that finds the stop flag set repeats the last record.
// Every index is bounded: a source row is below m, a record index below n (record_of), a winner's row is checked against n
// before it indexes the normals, a partial row is the workgroup's own.  Nothing waits on another workgroup.
#include <algorithm>

#include "point_grid.h"
#include "icp_math.h"

namespace {

using namespace epn_grid;
using namespace epn_icp;

constexpr int ACC_GROUPS = 1024;         // workgroups of icp_accumulate, at most: the result does not depend on it
constexpr int ST = 256;                  // threads of icp_solve
constexpr size_t STATE_BYTES = 256;

struct State {                           // the workspace's first 256 bytes
    double T[16];
    double prev_fitness, prev_rmse;
    int stop, iterations, status, pad;
};
static_assert(sizeof(State) <= STATE_BYTES, "the partial rows start behind the state");

int groups_of(int64_t m) { return (int)std::min<int64_t>(std::max<int64_t>(epn_cdiv(m, QW), 1), ACC_GROUPS); }

template <bool PLANE>
__global__ __launch_bounds__(QW * 64) void icp_accumulate_kernel(const Head *__restrict__ head, const Slot *__restrict__ slots,
                                                                 const int4 *__restrict__ records, int n, int log2cap, double edge,
                                                                 const float *__restrict__ normals, const float *__restrict__ src,
                                                                 int m, float r2, const double *__restrict__ T,
                                                                 const int *__restrict__ stop, long long *__restrict__ partial,
                                                                 int32_t *__restrict__ nn_idx) {
    __shared__ long long wsum[QW][NS];
    if (stop && *stop) return;                             // the same in every thread of the launch
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int ia, ib;
    double scale;
    term_of(PLANE, lane, ia, ib, scale);
    double Tm[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) Tm[e] = T[e];             // wave-uniform
    long long acc = 0;
    for (int q = (int)blockIdx.x * QW + wave; q < m; q += (int)gridDim.x * QW) {   // q is the same in every lane of the wave
        const float sv = lane < 3 ? src[3 * (size_t)q + lane] : 0.0f;
        const float s[3] = {__shfl(sv, 0, 64), __shfl(sv, 1, 64), __shfl(sv, 2, 64)};
        float qf[3];
        transform_point(Tm, s, qf);
        const Nearest nb = nearest_member(head, slots, records, n, log2cap, edge, qf[0], qf[1], qf[2], r2, 0, q, lane);
        int row = nb.key == NONE ? -1 : (int)(unsigned)(nb.key & 0xFFFFFFFFull);
        if ((unsigned)row >= (unsigned)n) row = -1;
        if (nn_idx && lane == 0) nn_idx[q] = row;
        if (row >= 0) {
            const float p[3] = {nb.x, nb.y, nb.z};
            Values V;
            if (PLANE) {
                const float nv = lane < 3 ? normals[3 * (size_t)row + lane] : 0.0f;
                const float nrm[3] = {__shfl(nv, 0, 64), __shfl(nv, 1, 64), __shfl(nv, 2, 64)};
                V = plane_values(p, qf, nrm);
            } else {
                V = p2p_values(p, qf);
            }
            if (lane == S_RANGE) acc += V.bad ? 1 : 0;
            else if (!V.bad && scale != 0.0) acc += term(value_at(V, ia), value_at(V, ib), scale);   // scale 0: the lane holds no sum
        }
    }
    if (lane < NS) wsum[wave][lane] = acc;
    __syncthreads();
    if (threadIdx.x < NS) {
        long long t = 0;
#pragma unroll
        for (int w = 0; w < QW; ++w) t += wsum[w][threadIdx.x];
        partial[(size_t)blockIdx.x * NS + threadIdx.x] = t;
    }
}

template <bool PLANE>
__global__ __launch_bounds__(ST) void icp_solve_kernel(const long long *__restrict__ partial, int groups, int m, int iter,
                                                       double rel_fitness, double rel_rmse, const double *T_init, State *state,
                                                       double *T_out, double *trace, int32_t *__restrict__ iterations,
                                                       int32_t *__restrict__ status, long long *__restrict__ sums) {
    __shared__ long long red[ST / NS][NS];
    __shared__ long long tot[NS];
    const int tid = threadIdx.x, e = tid & (NS - 1), g0 = tid / NS;
    if (iter > 0 && state->stop) {                         // the same in every thread
        if (tid < REC) trace[(size_t)iter * REC + tid] = trace[(size_t)(iter - 1) * REC + tid];
        return;
    }
    long long s = 0;
    for (int g = g0; g < groups; g += ST / NS) s += partial[(size_t)g * NS + e];
    red[g0][e] = s;
    __syncthreads();
    if (tid < NS) {
        long long t = 0;
#pragma unroll
        for (int g = 0; g < ST / NS; ++g) t += red[g][tid];
        tot[tid] = t;
        if (sums) sums[tid] = t;
    }
    __syncthreads();
    if (tid != 0) return;
    long long S[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) S[k] = tot[k];
    double T[16], rec[REC];
#pragma unroll
    for (int k = 0; k < 16; ++k) T[k] = iter == 0 ? T_init[k] : state->T[k];
    double prev_fitness = iter == 0 ? 0.0 : state->prev_fitness, prev_rmse = iter == 0 ? 0.0 : state->prev_rmse;
    const int done = iter == 0 ? 0 : state->iterations, before = iter == 0 ? 0 : state->status;
    const int flags = step(PLANE, S, m, iter, rel_fitness, rel_rmse, prev_fitness, prev_rmse, T, rec);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        state->T[k] = T[k];
        T_out[k] = T[k];
    }
#pragma unroll
    for (int k = 0; k < REC; ++k) trace[(size_t)iter * REC + k] = rec[k];
    state->prev_fitness = prev_fitness;
    state->prev_rmse = prev_rmse;
    state->stop = flags != 0;
    state->iterations = done + (flags == 0);
    state->status = before | flags;
    *iterations = done + (flags == 0);
    *status = before | flags;
}

// m == 0 or max_iter == 0: T = T_init (bottom row 0 0 0 1), every trace record {T, 0, 0, 0, 0}, no correspondences
__global__ __launch_bounds__(ST) void icp_idle_kernel(const double *T_init, double *T_out, double *trace, int max_iter,
                                                      int32_t *__restrict__ iterations, int32_t *__restrict__ status,
                                                      long long *__restrict__ sums, int32_t *__restrict__ nn_idx, int m) {
    const int tid = threadIdx.x;
    double v = 0.0;
    if (tid < 12) v = T_init[tid];
    if (tid == 15) v = 1.0;
    __syncthreads();                                       // T_out may be T_init: every read is made before the first write
    if (tid < 16) T_out[tid] = v;
    for (int k = 0; k < max_iter; ++k)
        if (tid < REC) trace[(size_t)k * REC + tid] = v;   // threads 16..19 hold 0
    if (tid == 0) {
        *iterations = 0;
        *status = 0;
    }
    if (sums && tid < NS) sums[tid] = 0;
    if (nn_idx)
        for (int q = tid; q < m; q += ST) nn_idx[q] = -1;
}

}  // namespace

extern "C" size_t epn_icp_workspace_bytes(int64_t m) {
    return m >= 0 && m <= MAX_M ? STATE_BYTES + (size_t)groups_of(m) * NS * sizeof(long long) : 0;
}

extern "C" int epn_icp_refine_f32(const void *grid_workspace, int64_t n, const float *tgt_normals, const float *src, int64_t m,
                                  const double *T_init, double max_dist, int max_iter, double rel_fitness, double rel_rmse,
                                  void *workspace, size_t workspace_bytes, double *T, double *trace, int32_t *iterations,
                                  int32_t *status, int64_t *sums, int32_t *nn_idx, epn_stream_t stream) {
    // every argument is checked before the first HIP runtime call
    if (n < 0 || n > MAX_N || m < 0 || m > MAX_M || !std::isfinite(max_dist) || !(max_dist > 0.0)) return EPN_EINVAL;
    if (max_iter < 0 || max_iter > MAX_ITER) return EPN_EINVAL;
    if (!(rel_fitness >= 0.0) || !(rel_rmse >= 0.0) || !std::isfinite(rel_fitness) || !std::isfinite(rel_rmse)) return EPN_EINVAL;
    if (!grid_workspace || (reinterpret_cast<uintptr_t>(grid_workspace) & 15u) != 0) return EPN_EINVAL;
    Built b;
    if (!recall(grid_workspace, b) || b.n != n || max_dist > b.max_radius) return EPN_EINVAL;
    if (!T_init || !T || !iterations || !status || (m > 0 && !src) || (max_iter > 0 && !trace)) return EPN_ENULL;
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15u) != 0 || workspace_bytes < epn_icp_workspace_bytes(m))
        return EPN_EWORKSPACE;
    hipStream_t st = epn_stream(stream);
    long long *out_sums = reinterpret_cast<long long *>(sums);
    if (m == 0 || max_iter == 0) {
        EPN_LAUNCH(icp_idle_kernel, dim3(1), dim3(ST), 0, st, T_init, T, trace, max_iter, iterations, status, out_sums, nn_idx,
                   (int)m);
        EPN_CHECK_LAUNCH();
        return 0;
    }
    const Layout L = layout(n);
    const char *gw = static_cast<const char *>(grid_workspace);
    const Head *head = reinterpret_cast<const Head *>(gw);
    const Slot *slots = reinterpret_cast<const Slot *>(gw + L.slots);
    const int4 *records = reinterpret_cast<const int4 *>(gw + L.records);
    State *state = static_cast<State *>(workspace);
    long long *partial = reinterpret_cast<long long *>(static_cast<char *>(workspace) + STATE_BYTES);
    const int groups = groups_of(m);
    const double edge = cell_edge(b.max_radius);
    const float r2 = (float)(max_dist * max_dist);
    for (int iter = 0; iter < max_iter; ++iter) {
        const double *Tk = iter == 0 ? T_init : state->T;
        const int *stop = iter == 0 ? nullptr : &state->stop;
        if (tgt_normals) {
            EPN_LAUNCH(icp_accumulate_kernel<true>, dim3((unsigned)groups), dim3(QW * 64), 0, st, head, slots, records, (int)n,
                       L.log2cap, edge, tgt_normals, src, (int)m, r2, Tk, stop, partial, nn_idx);
            EPN_LAUNCH_AUX(icp_solve_kernel<true>, dim3(1), dim3(ST), 0, st, partial, groups, (int)m, iter, rel_fitness, rel_rmse,
                           T_init, state, T, trace, iterations, status, out_sums);
        } else {
            EPN_LAUNCH(icp_accumulate_kernel<false>, dim3((unsigned)groups), dim3(QW * 64), 0, st, head, slots, records, (int)n,
                       L.log2cap, edge, tgt_normals, src, (int)m, r2, Tk, stop, partial, nn_idx);
            EPN_LAUNCH_AUX(icp_solve_kernel<false>, dim3(1), dim3(ST), 0, st, partial, groups, (int)m, iter, rel_fitness, rel_rmse,
                           T_init, state, T, trace, iterations, status, out_sums);
        }
    }
    EPN_CHECK_LAUNCH();
    return 0;
}
