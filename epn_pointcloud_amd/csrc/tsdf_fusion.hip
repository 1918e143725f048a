// TSDF fusion for gfx950: a window of depth frames -> the (tsdf, weight) blocks of a fragment -> its surface points, the stage
// the reference runs on the host with open3d (SPConvNets/datasets/preprocess/run_fusion.py:20-49: ScalableTSDFVolume.integrate
// per frame, extract_point_cloud).  Specification: include/epn_so3conv.h (epn_tsdf_fuse_f32, epn_tsdf_extract_f32) and DESIGN.md
// 3.1l; the per-sample arithmetic is tsdf_math.h's, which tools/tsdf_host.cpp runs on the host.
//
// epn_tsdf_fuse_f32, six launches on the call's stream:
//   init       the directory's masks to zero (one kernel, no memset)
//   touch      one thread per sampled pixel of a frame: depth, back-projection, pose, then bit f into the (at most 2 x 2 x 2) units
//              of point +- sdf_trunc with a 64-bit atomicOr -- the only atomic of the file.  A sample with a unit outside the
//              box is counted per workgroup (ballot + popcount) into the workspace; no atomic counter.
//   count      allocated entries per tile of 256 directory entries
//   scan       ONE workgroup: the tile sums -> exclusive offsets (scan_sums), the outside counts summed in a fixed order, status
//   rank       rank(e) = offset of e's tile + allocated entries below e in it (tile_scan); block_unit / block_mask rows and the
//              directory's rank array, -1 for an entry without a block
//   integrate  THE HOT PATH, one workgroup of 256 threads per block.  Thread (x = tid & 15, y = tid >> 4) owns the 16 voxels of
//              one z column.  In the fragment's frame (the first camera's) the image's u runs along x and v along y, while z is
//              the viewing direction, along which a column projects to nearly one pixel: so the 64 lanes of a wave are a 16 x 4
//              patch in x, y at one z, their pixels fall into four short runs of four image rows (at 2 m one voxel is about 1.7
//              pixels: 16 voxels are ~54 bytes of a u16 row, one or two cache lines), and the 16 steps of a thread along z
//              hit the same lines again while they are in the L1.  Per voxel the frames of the block's mask run in ascending
//              order with (tsdf, w) in two registers; the per-frame pose rows and the intrinsics are read with uniform
//              (scalar) loads.  A finished voxel goes to a 32 KiB LDS image of the block, which is stored once with 16-byte
//              row-contiguous stores (the thread-to-voxel map that suits the depth reads would store 4 bytes at a 64-byte
//              stride).  The kernel takes 42 VGPRs and no scratch, so the 32 KiB LDS image sets the occupancy: 5 workgroups =
//              20 waves per CU, 5 per SIMD, enough to cover the depth reads of a kernel whose time goes to fp64 division and
//              square root (six and one per voxel-frame update), not to memory.  Launch bounds 256.
// epn_tsdf_extract_f32, three launches: count (crossings per block), scan (one workgroup, scan_sums over the blocks), write.
//   Count and write are one kernel template: a block's voxels, reduced to "its tsdf, or NaN when it takes no part", and its three
//   +faces (looked up through the directory's rank array) go to LDS; then 16 passes of 256 voxels, each voxel testing its three
//   +neighbours, ranked inside the block by tile_scan.
// The grids of integrate, count and write are max_blocks workgroups; one beyond min(n_blocks, max_blocks) returns at once (the
// count writes its 0).  Every loop is bounded by an argument (F, the tile counts, 16); every directory index passes box_offset,
// every rank is checked against min(n_blocks, max_blocks), every pixel against W and H, every output row against its limit.
// Nothing waits on another workgroup; no floating-point atomics; two runs are bitwise equal.
#include "cell_hash.h"
#include "tsdf_math.h"

namespace {

using namespace epn_cells;               // VT, VW, tile_scan, scan_sums
using namespace epn_tsdf;

struct TsdfHead {                        // the workspace's first 64 bytes
    int n_blocks, flags, n_outside, pad[13];
};

struct Box {
    int lo[3], dim[3];
};

struct Layout {
    long long D;                         // directory entries
    int nt, ntouch, tiles_per_frame, ws, hs;
    size_t masks, rank, bcount, tsum, wgout, bytes;
};

bool box_ok(const Box &b) {
    long long D = 1;
    for (int a = 0; a < 3; ++a) {
        if (b.dim[a] < 1 || b.lo[a] < -MAX_UNIT_LO || b.lo[a] > MAX_UNIT_LO) return false;
        D *= b.dim[a];
        if (D > MAX_DIRECTORY) return false;
    }
    return true;
}

// callers have checked box_ok, 1 <= max_blocks <= MAX_BLOCKS; F, H, W, stride are used only by the fuse
Layout layout(const Box &b, int max_blocks, int F, int H, int W, int stride) {
    Layout L;
    L.D = (long long)b.dim[0] * b.dim[1] * b.dim[2];
    L.nt = epn_cdiv(L.D, VT);
    L.ws = (W + stride - 1) / stride;
    L.hs = (H + stride - 1) / stride;
    L.tiles_per_frame = epn_cdiv((long long)L.ws * L.hs, VT);
    L.ntouch = F * L.tiles_per_frame;
    L.masks = sizeof(TsdfHead);
    L.rank = L.masks + (size_t)L.D * 8;
    L.bcount = L.rank + (size_t)L.D * 4;
    L.tsum = L.bcount + (size_t)max_blocks * 4;
    L.wgout = L.tsum + (size_t)L.nt * 4;
    L.bytes = (L.wgout + (size_t)L.ntouch * 4 + 7) & ~(size_t)7;
    return L;
}

__device__ __forceinline__ long long dir_index(const Box &b, int rx, int ry, int rz) {
    return ((long long)rx * b.dim[1] + ry) * b.dim[2] + rz;
}

__global__ __launch_bounds__(VT) void tsdf_init_kernel(unsigned long long *__restrict__ masks, long long D) {
    const long long e = (long long)blockIdx.x * VT + threadIdx.x;
    if (e < D) masks[e] = 0ull;
}

__global__ __launch_bounds__(VT) void tsdf_touch_kernel(const uint16_t *__restrict__ depth, int H, int W, int ws, int hs, int stride,
                                                        const double *__restrict__ cam2base, Camera cam, float depth_scale,
                                                        double depth_trunc, double unit_length, double sdf_trunc, Box box,
                                                        unsigned long long *masks, int *__restrict__ wgout) {
    __shared__ int wcnt[VW];
    const int tid = threadIdx.x, f = blockIdx.y;
    const int s = (int)blockIdx.x * VT + tid;
    bool outside = false;
    if (s < ws * hs) {
        const int u = (s % ws) * stride, v = (s / ws) * stride;        // u < W and v < H: s % ws < ws = ceil(W / stride)
        const float d = depth_value(depth[((size_t)f * H + v) * W + u], depth_scale, depth_trunc);
        if (d != 0.0f) {
            double c[3], p[3], lo[3], hi[3];
            back_project(u, v, d, cam, c);
            transform(cam2base + 16 * (size_t)f, c, p);
#pragma unroll
            for (int a = 0; a < 3; ++a) unit_span(p[a], sdf_trunc, unit_length, lo[a], hi[a]);
            const unsigned long long bit = 1ull << f;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const bool kx = k & 4, ky = k & 2, kz = k & 1;
                if ((kx && hi[0] == lo[0]) || (ky && hi[1] == lo[1]) || (kz && hi[2] == lo[2])) continue;   // the same unit again
                int rx, ry, rz;
                if (box_offset(kx ? hi[0] : lo[0], box.lo[0], box.dim[0], rx) && box_offset(ky ? hi[1] : lo[1], box.lo[1], box.dim[1], ry) &&
                    box_offset(kz ? hi[2] : lo[2], box.lo[2], box.dim[2], rz))
                    atomicOr(&masks[dir_index(box, rx, ry, rz)], bit);
                else
                    outside = true;
            }
        }
    }
    const unsigned long long m = __ballot(outside);
    if ((tid & 63) == 0) wcnt[tid >> 6] = __popcll(m);
    __syncthreads();
    if (tid == 0) {
        int t = 0;
#pragma unroll
        for (int w = 0; w < VW; ++w) t += wcnt[w];
        wgout[(size_t)f * gridDim.x + blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(VT) void tsdf_count_kernel(const unsigned long long *__restrict__ masks, long long D,
                                                        int *__restrict__ tsum) {
    __shared__ int wcnt[VW];
    const int tid = threadIdx.x;
    const long long e = (long long)blockIdx.x * VT + tid;
    const unsigned long long m = __ballot(e < D && masks[e] != 0ull);
    if ((tid & 63) == 0) wcnt[tid >> 6] = __popcll(m);
    __syncthreads();
    if (tid == 0) {
        int t = 0;
#pragma unroll
        for (int w = 0; w < VW; ++w) t += wcnt[w];
        tsum[blockIdx.x] = t;
    }
}

// one workgroup
__global__ __launch_bounds__(VT) void tsdf_scan_kernel(int *tsum, int nt, const int *__restrict__ wgout, int ntouch, int max_blocks,
                                                       TsdfHead *head, int32_t *__restrict__ status) {
    __shared__ int wsum[VW];
    const int n_blocks = scan_sums(tsum, nt);
    int mine = 0;
    for (int e = threadIdx.x; e < ntouch; e += VT) mine += wgout[e];
    int n_outside;
    tile_scan(mine, wsum, n_outside);
    if (threadIdx.x == 0) {
        const int flags = (n_outside ? FLAG_OUTSIDE : 0) | (n_blocks > max_blocks ? FLAG_BLOCKS : 0);
        head->n_blocks = n_blocks;
        head->flags = flags;
        head->n_outside = n_outside;
        status[0] = n_blocks;
        status[1] = flags;
        status[2] = n_outside;
        status[3] = 0;
    }
}

__global__ __launch_bounds__(VT) void tsdf_rank_kernel(const unsigned long long *__restrict__ masks, long long D,
                                                       const int *__restrict__ tsum, Box box, int max_blocks,
                                                       int32_t *__restrict__ rank, int32_t *__restrict__ block_unit,
                                                       unsigned long long *__restrict__ block_mask) {
    __shared__ int wsum[VW];
    const long long e = (long long)blockIdx.x * VT + threadIdx.x;
    const unsigned long long m = e < D ? masks[e] : 0ull;
    int total;
    const int r = tsum[blockIdx.x] + tile_scan(m != 0ull, wsum, total);
    if (e >= D) return;
    const bool mine = m != 0ull && r < max_blocks;
    rank[e] = mine ? r : -1;
    if (mine) {
        const int rz = (int)(e % box.dim[2]), ry = (int)((e / box.dim[2]) % box.dim[1]);
        const int rx = (int)(e / ((long long)box.dim[2] * box.dim[1]));
        block_unit[3 * (size_t)r] = box.lo[0] + rx;
        block_unit[3 * (size_t)r + 1] = box.lo[1] + ry;
        block_unit[3 * (size_t)r + 2] = box.lo[2] + rz;
        block_mask[r] = m;
    }
}

__global__ __launch_bounds__(VT) void tsdf_integrate_kernel(const uint16_t *__restrict__ depth, int F, int H, int W,
                                                            const double *__restrict__ base2cam, Camera cam, float depth_scale,
                                                            double depth_trunc, double voxel_length, double sdf_trunc,
                                                            const TsdfHead *__restrict__ head, int max_blocks,
                                                            const int32_t *__restrict__ block_unit,
                                                            const unsigned long long *__restrict__ block_mask,
                                                            float *__restrict__ tsdf, int32_t *__restrict__ weight) {
    __shared__ __attribute__((aligned(16))) float s_tsdf[UNIT_VOX];
    __shared__ __attribute__((aligned(16))) int s_w[UNIT_VOX];
    const int b = blockIdx.x;
    const int nb = min(max(head->n_blocks, 0), max_blocks);
    if (b >= nb) return;                                            // uniform: the whole workgroup leaves
    const int tid = threadIdx.x, x = tid & 15, y = tid >> 4;
    const int ux = block_unit[3 * (size_t)b], uy = block_unit[3 * (size_t)b + 1], uz = block_unit[3 * (size_t)b + 2];
    const unsigned long long mask = block_mask[b];
    double p[3];
    p[0] = voxel_centre(ux, x, voxel_length);
    p[1] = voxel_centre(uy, y, voxel_length);
    for (int z = 0; z < UNIT; ++z) {
        p[2] = voxel_centre(uz, z, voxel_length);
        float val = 0.0f;
        int w = 0;
        for (int f = 0; f < F; ++f) {
            if (!((mask >> f) & 1ull)) continue;                    // uniform
            double c[3];
            transform(base2cam + 16 * (size_t)f, p, c);
            int pu, pv;
            if (!project(c, cam, W, H, pu, pv)) continue;
            const float d = depth_value(depth[((size_t)f * H + pv) * W + pu], depth_scale, depth_trunc);
            float t;
            if (observe(d, c[2], pu, pv, cam, sdf_trunc, t)) update(val, w, t);
        }
        const int i = (x * UNIT + y) * UNIT + z;
        s_tsdf[i] = val;
        s_w[i] = w;
    }
    __syncthreads();
    float4 *gt = reinterpret_cast<float4 *>(tsdf + (size_t)b * UNIT_VOX);
    int4 *gw = reinterpret_cast<int4 *>(weight + (size_t)b * UNIT_VOX);
#pragma unroll
    for (int k = 0; k < UNIT_VOX / 4 / VT; ++k) {
        const int q = k * VT + tid;
        gt[q] = reinterpret_cast<const float4 *>(s_tsdf)[q];
        gw[q] = reinterpret_cast<const int4 *>(s_w)[q];
    }
}

// rank of the block of unit (ux, uy, uz), -1 when it is outside the box, absent or beyond the pool
__device__ __forceinline__ int block_of(const int32_t *__restrict__ rank, const Box &box, double ux, double uy, double uz, int nb) {
    int rx, ry, rz;
    if (!(box_offset(ux, box.lo[0], box.dim[0], rx) && box_offset(uy, box.lo[1], box.dim[1], ry) &&
          box_offset(uz, box.lo[2], box.dim[2], rz)))
        return -1;
    const int r = rank[dir_index(box, rx, ry, rz)];
    return r >= 0 && r < nb ? r : -1;
}

template <bool WRITE>
__global__ __launch_bounds__(VT) void tsdf_extract_kernel(const float *__restrict__ tsdf, const int32_t *__restrict__ weight,
                                                          const int32_t *__restrict__ block_unit, const TsdfHead *__restrict__ head,
                                                          int max_blocks, const int32_t *__restrict__ rank, Box box,
                                                          double voxel_length, int *__restrict__ bcount,
                                                          float *__restrict__ points, int max_points) {
    __shared__ float val[UNIT_VOX];                                 // a voxel's tsdf, NaN when it takes no part
    __shared__ float face[3][UNIT * UNIT];                          // voxel 0 of the +neighbour unit on each axis
    __shared__ int nbr[3];
    __shared__ int wsum[VW];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int nb = min(max(head->n_blocks, 0), max_blocks);
    if (b >= nb) {                                                  // uniform
        if (!WRITE && tid == 0) bcount[b] = 0;
        return;
    }
    const int unit[3] = {block_unit[3 * (size_t)b], block_unit[3 * (size_t)b + 1], block_unit[3 * (size_t)b + 2]};
    if (tid < 3)
        nbr[tid] = block_of(rank, box, (double)unit[0] + (tid == 0), (double)unit[1] + (tid == 1), (double)unit[2] + (tid == 2), nb);
    for (int i = tid; i < UNIT_VOX; i += VT) {
        const float f = tsdf[(size_t)b * UNIT_VOX + i];
        val[i] = takes_part(f, weight[(size_t)b * UNIT_VOX + i]) ? f : NAN;
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int r = nbr[a], p = tid >> 4, q = tid & 15;          // the face's two free coordinates, in x, y, z order
        const int i = a == 0 ? p * UNIT + q : a == 1 ? p * UNIT * UNIT + q : (p * UNIT + q) * UNIT;
        float f = NAN;
        if (r >= 0) {
            const float g = tsdf[(size_t)r * UNIT_VOX + i];
            if (takes_part(g, weight[(size_t)r * UNIT_VOX + i])) f = g;
        }
        face[a][tid] = f;
    }
    __syncthreads();
    int base = WRITE ? bcount[b] : 0;                              // WRITE: the exclusive offset the scan left there
    for (int pass = 0; pass < UNIT_VOX / VT; ++pass) {
        const int i = pass * VT + tid;
        const int x = i >> 8, y = (i >> 4) & 15, z = i & 15;
        const float f0 = val[i];
        float f1[3];
        f1[0] = x < 15 ? val[i + 256] : face[0][y * UNIT + z];
        f1[1] = y < 15 ? val[i + 16] : face[1][x * UNIT + z];
        f1[2] = z < 15 ? val[i + 1] : face[2][x * UNIT + y];
        bool hit[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) hit[a] = !isnan(f0) && !isnan(f1[a]) && crosses(f0, f1[a]);
        const int n = (int)hit[0] + (int)hit[1] + (int)hit[2];
        int total;
        int row = base + tile_scan(n, wsum, total);
        base += total;
        if (WRITE && n) {
            const int idx[3] = {x, y, z};
            double c[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) c[a] = voxel_centre(unit[a], idx[a], voxel_length);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (!hit[a]) continue;
                if (row < max_points) {
                    float o[3] = {(float)c[0], (float)c[1], (float)c[2]};
                    o[a] = crossing(f0, f1[a], c[a], voxel_length);
                    points[3 * (size_t)row] = o[0];
                    points[3 * (size_t)row + 1] = o[1];
                    points[3 * (size_t)row + 2] = o[2];
                }
                ++row;
            }
        }
        __syncthreads();                                            // wsum is rewritten by the next pass
    }
    if (!WRITE && tid == 0) bcount[b] = base;
}

// one workgroup
__global__ __launch_bounds__(VT) void tsdf_extract_scan_kernel(int *bcount, int max_blocks, int max_points, int32_t *__restrict__ status) {
    const int total = scan_sums(bcount, max_blocks);
    if (threadIdx.x == 0) {
        status[0] = total;
        status[1] = total > max_points ? FLAG_POINTS : 0;
    }
}

bool positive(double v) { return std::isfinite(v) && v > 0.0; }

}  // namespace

extern "C" size_t epn_tsdf_fuse_workspace_bytes(int F, int H, int W, int stride, int dim_x, int dim_y, int dim_z, int max_blocks) {
    const Box box = {{0, 0, 0}, {dim_x, dim_y, dim_z}};
    if (F < 1 || F > MAX_FRAMES || H < 1 || H > MAX_IMAGE || W < 1 || W > MAX_IMAGE || stride < 1 || !box_ok(box) ||
        max_blocks < 1 || max_blocks > MAX_BLOCKS)
        return 0;
    return layout(box, max_blocks, F, H, W, stride).bytes;
}

extern "C" int epn_tsdf_fuse_f32(const uint16_t *depth, int F, int H, int W, const double *cam2base, const double *base2cam,
                                 double fx, double fy, double cx, double cy, double depth_scale, double depth_trunc,
                                 double voxel_length, double sdf_trunc, int stride, int lo_x, int lo_y, int lo_z, int dim_x, int dim_y,
                                 int dim_z, int max_blocks, int32_t *block_unit, uint64_t *block_mask, float *tsdf,
                                 int32_t *weight, int32_t *status, void *workspace, size_t workspace_bytes, epn_stream_t stream) {
    // every argument is checked before the first HIP runtime call
    const Box box = {{lo_x, lo_y, lo_z}, {dim_x, dim_y, dim_z}};
    if (F < 1 || F > MAX_FRAMES || H < 1 || H > MAX_IMAGE || W < 1 || W > MAX_IMAGE || stride < 1) return EPN_EINVAL;
    if (!positive(fx) || !positive(fy) || !std::isfinite(cx) || !std::isfinite(cy)) return EPN_EINVAL;
    if (!positive(depth_scale) || !positive((double)(float)depth_scale) || !std::isfinite((double)(float)depth_scale)) return EPN_EINVAL;
    if (!positive(depth_trunc) || !positive(voxel_length) || !positive(sdf_trunc)) return EPN_EINVAL;
    if (!(sdf_trunc <= 8.0 * voxel_length) || !positive(16.0 * voxel_length)) return EPN_EINVAL;
    if (!box_ok(box) || max_blocks < 1 || max_blocks > MAX_BLOCKS) return EPN_EINVAL;
    if (!depth || !cam2base || !base2cam || !block_unit || !block_mask || !tsdf || !weight || !status) return EPN_ENULL;
    const Layout L = layout(box, max_blocks, F, H, W, stride);
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7u) != 0 || workspace_bytes < L.bytes) return EPN_EWORKSPACE;
    if ((reinterpret_cast<uintptr_t>(tsdf) & 15u) != 0 || (reinterpret_cast<uintptr_t>(weight) & 15u) != 0) return EPN_EINVAL;
    hipStream_t st = epn_stream(stream);
    char *ws = static_cast<char *>(workspace);
    TsdfHead *head = reinterpret_cast<TsdfHead *>(ws);
    unsigned long long *masks = reinterpret_cast<unsigned long long *>(ws + L.masks);
    int32_t *rank = reinterpret_cast<int32_t *>(ws + L.rank);
    int *tsum = reinterpret_cast<int *>(ws + L.tsum), *wgout = reinterpret_cast<int *>(ws + L.wgout);
    const Camera cam = {fx, fy, cx, cy};
    const double unit_length = 16.0 * voxel_length;
    const dim3 block(VT), tiles((unsigned)L.nt);
    EPN_LAUNCH_AUX(tsdf_init_kernel, tiles, block, 0, st, masks, L.D);
    EPN_LAUNCH_AUX(tsdf_touch_kernel, dim3((unsigned)L.tiles_per_frame, (unsigned)F), block, 0, st, depth, H, W, L.ws, L.hs, stride,
                   cam2base, cam, (float)depth_scale, depth_trunc, unit_length, sdf_trunc, box, masks, wgout);
    EPN_LAUNCH_AUX(tsdf_count_kernel, tiles, block, 0, st, masks, L.D, tsum);
    EPN_LAUNCH_AUX(tsdf_scan_kernel, dim3(1), block, 0, st, tsum, L.nt, wgout, L.ntouch, max_blocks, head, status);
    EPN_LAUNCH_AUX(tsdf_rank_kernel, tiles, block, 0, st, masks, L.D, tsum, box, max_blocks, rank, block_unit,
                   reinterpret_cast<unsigned long long *>(block_mask));
    EPN_LAUNCH(tsdf_integrate_kernel, dim3((unsigned)max_blocks), block, 0, st, depth, F, H, W, base2cam, cam, (float)depth_scale,
               depth_trunc, voxel_length, sdf_trunc, head, max_blocks, block_unit,
               reinterpret_cast<const unsigned long long *>(block_mask), tsdf, weight);
    EPN_CHECK_LAUNCH();
    return 0;
}

extern "C" int epn_tsdf_extract_f32(const float *tsdf, const int32_t *weight, const int32_t *block_unit, int max_blocks, int lo_x,
                                    int lo_y, int lo_z, int dim_x, int dim_y, int dim_z, double voxel_length, float *points,
                                    int max_points, int32_t *status, void *workspace, size_t workspace_bytes, epn_stream_t stream) {
    const Box box = {{lo_x, lo_y, lo_z}, {dim_x, dim_y, dim_z}};
    if (!positive(voxel_length) || !box_ok(box) || max_blocks < 1 || max_blocks > MAX_BLOCKS || max_points < 0) return EPN_EINVAL;
    if (!tsdf || !weight || !block_unit || !status || (max_points > 0 && !points)) return EPN_ENULL;
    const Layout L = layout(box, max_blocks, 1, 1, 1, 1);           // the offsets the extract uses do not depend on the frames
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7u) != 0 || workspace_bytes < L.tsum) return EPN_EWORKSPACE;
    hipStream_t st = epn_stream(stream);
    char *ws = static_cast<char *>(workspace);
    const TsdfHead *head = reinterpret_cast<const TsdfHead *>(ws);
    const int32_t *rank = reinterpret_cast<const int32_t *>(ws + L.rank);
    int *bcount = reinterpret_cast<int *>(ws + L.bcount);
    const dim3 block(VT), blocks((unsigned)max_blocks);
    EPN_LAUNCH_AUX(tsdf_extract_kernel<false>, blocks, block, 0, st, tsdf, weight, block_unit, head, max_blocks, rank, box,
                   voxel_length, bcount, points, max_points);
    EPN_LAUNCH_AUX(tsdf_extract_scan_kernel, dim3(1), block, 0, st, bcount, max_blocks, max_points, status);
    EPN_LAUNCH(tsdf_extract_kernel<true>, blocks, block, 0, st, tsdf, weight, block_unit, head, max_blocks, rank, box, voxel_length,
               bcount, points, max_points);
    EPN_CHECK_LAUNCH();
    return 0;
}
