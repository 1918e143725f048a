"""TSDF fusion (vgtk.pc.fuse_fragment, csrc/tsdf_fusion.hip) priced on one fragment of the reference's size: 50 frames of 640 x 480
(SPConvNets/datasets/preprocess/tool.py:17-27), rendered analytically from the inside of a 4 x 3 x 5 m room (a box, in numpy), the
reference's settings (voxel_length 3 / 512, sdf_trunc 0.04, depth scale 1000, depth_trunc 6, stride 4).

Timed with HIP events on preallocated buffers, median of --runs after warm-up: the fuse call (six launches), the same call with
a pool of ONE block (its five other launches, and an integrate kernel that leaves at once: their difference is the integrate
kernel on the pool), and the extract call (three launches).  The integrate kernel's rate is set against the two bounds that can
be derived:
  * fp64 arithmetic: voxel-frame updates (4096 x the bits of every block's mask) x 40 fp64 operations per update (18 for the pose,
    8 for the projection, 1 for the depth, 13 for the observation; six of them divisions and one a square root, each counted as
    one) against the fp64 vector peak, half the fp32 vector peak of 157.3 TFLOP/s;
  * memory: the pool's bytes, written once (8 bytes per voxel), against the 6.29 TB/s a float4 copy reaches.
Next to it the stages that follow on the same fragment: voxel_down_sample at 0.03 and estimate_normals (radius 0.1, 30 neighbours).

    python tools/tsdf_bench.py [--frames 50] [--runs 10] [--out profiles/tsdf_fusion.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP64_PEAK = 157.3e12 / 2
HBM_COPY = 6.29e12
OPS_PER_UPDATE = 40
ROOM_LO, ROOM_HI = np.array([-2.0, -1.5, -2.5]), np.array([2.0, 1.5, 2.5])


def event_ms(fn, runs, warmup=2):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return times


def pose(k, n):
    """a camera inside the room, turning about the vertical axis while it drifts"""
    a = -0.35 + 0.7 * k / max(n - 1, 1)
    c, s = np.cos(a), np.sin(a)
    T = np.eye(4)
    T[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    T[:3, 3] = (-0.4 + 0.8 * k / max(n - 1, 1), 0.1 * np.sin(0.3 * k), -1.0 + 0.01 * k)
    return T


def render_room(T, H, W, K):
    """u16 [H,W]: the z-depth, in millimetres, at which every pixel's ray leaves the room"""
    fx, fy, cx, cy = K
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ray = np.stack(((u - cx) / fx, (v - cy) / fy, np.ones_like(u)), axis=-1) @ T[:3, :3].T
    o = T[:3, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(ray > 0, (ROOM_HI - o) / ray, np.where(ray < 0, (ROOM_LO - o) / ray, np.inf)).min(axis=-1)
    return np.clip(np.rint(1000.0 * t), 0, 65535).astype(np.uint16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "tsdf_fusion.txt"))
    a = ap.parse_args()
    from epn_pointcloud_amd import fusion
    from epn_pointcloud_amd.vgtk import pc as pctk
    dev = torch.device("cuda:0")
    H, W, K = 480, 640, (585.0, 585.0, 320.0, 240.0)
    vl, st, stride, dtr = 3.0 / 512, 0.04, 4, 6.0
    poses = np.stack([pose(k, a.frames) for k in range(a.frames)])
    depth_np = np.stack([render_room(T, H, W, K) for T in poses])
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"tsdf_bench: {a.frames} frames of {W} x {H} from inside a 4 x 3 x 5 m room, voxel_length 3/512, sdf_trunc {st}, stride {stride}, "
        f"depth_trunc {dtr}; median of {a.runs} runs, device = {torch.cuda.get_device_name(0)}")
    depth = torch.from_numpy(depth_np.view(np.int16)).to(dev)
    whole = event_ms(lambda: pctk.fuse_fragment(depth, poses, K), max(3, a.runs // 2), warmup=1)
    frag = pctk.fuse_fragment(depth, poses, K, return_volume=True)
    vol = frag.volume
    n_blocks, M = frag.n_blocks, frag.points.shape[0]
    cam2base, base2cam, _ = fusion.relative_poses(poses)
    c2b, b2c = torch.from_numpy(cam2base).to(dev), torch.from_numpy(base2cam).to(dev)
    kw = dict(depth_scale=1000.0, depth_trunc=dtr, voxel_length=vl, sdf_trunc=st, stride=stride)
    D = vol.unit_dims[0] * vol.unit_dims[1] * vol.unit_dims[2]
    updates = 4096 * sum(bin(m & (2 ** 64 - 1)).count("1") for m in vol.block_mask.tolist())
    pool_bytes = n_blocks * 4096 * 8

    out = fusion.tsdf_fuse(depth, c2b, b2c, K, vol.unit_lo, vol.unit_dims, n_blocks, **kw)
    outs, ws = out[:4], out[5]
    fuse = event_ms(lambda: fusion.tsdf_fuse(depth, c2b, b2c, K, vol.unit_lo, vol.unit_dims, n_blocks, out=outs, **kw), a.runs)
    one = fusion.tsdf_fuse(depth, c2b, b2c, K, vol.unit_lo, vol.unit_dims, 1, **kw)[:4]
    rest = event_ms(lambda: fusion.tsdf_fuse(depth, c2b, b2c, K, vol.unit_lo, vol.unit_dims, 1, out=one, **kw), a.runs)
    out = fusion.tsdf_fuse(depth, c2b, b2c, K, vol.unit_lo, vol.unit_dims, n_blocks, out=outs, **kw)       # the workspace of the full pool
    ws = out[5]
    points = torch.empty((M, 3), dtype=torch.float32, device=dev)
    extract = event_ms(lambda: fusion.tsdf_extract(outs[2], outs[3], outs[0], ws, vol.unit_lo, vol.unit_dims, vl, M, points=points), a.runs)
    f, r, x, w = (statistics.median(t) for t in (fuse, rest, extract, whole))
    integrate = max(f - r, 1e-6)
    say(f"unit box {vol.unit_dims} = {D} directory entries ({12 * D / 2 ** 20:.1f} MiB of workspace), {n_blocks} blocks "
        f"({pool_bytes / 2 ** 20:.0f} MiB of tsdf + weight), {M} points, {updates / 1e6:.1f} M voxel-frame updates")
    say(f"fuse_fragment, whole (allocations, box, two status read-backs, counting and writing extract): {w:.2f} ms "
        f"(min {min(whole):.2f}, max {max(whole):.2f})")
    say(f"fuse call, six launches: {f:.3f} ms (min {min(fuse):.3f}, max {max(fuse):.3f}); with a pool of one block: {r:.3f} ms "
        f"(min {min(rest):.3f}, max {max(rest):.3f}); integrate kernel = the difference: {integrate:.3f} ms")
    say(f"integrate: {updates / integrate / 1e6:.2f} G voxel-frame updates/s = {OPS_PER_UPDATE * updates / integrate / 1e9:.2f} TFLOP/s fp64 at "
        f"{OPS_PER_UPDATE} operations per update = {100 * OPS_PER_UPDATE * updates / (integrate * 1e-3) / FP64_PEAK:.1f} % of the fp64 vector peak "
        f"({FP64_PEAK / 1e12:.1f} TFLOP/s: the arithmetic bound is {1e3 * OPS_PER_UPDATE * updates / FP64_PEAK:.3f} ms); the pool written once at "
        f"{HBM_COPY / 1e12:.2f} TB/s is {1e3 * pool_bytes / HBM_COPY:.3f} ms = {100 * 1e3 * pool_bytes / HBM_COPY / integrate:.1f} % of the kernel")
    say(f"extract call, three launches: {x:.3f} ms (min {min(extract):.3f}, max {max(extract):.3f})")
    down = event_ms(lambda: pctk.voxel_down_sample(frag.points, 0.03), a.runs)
    normals = event_ms(lambda: pctk.estimate_normals(frag.points, 0.1, max_nn=30, view=(0.0, 0.0, 0.0)), max(3, a.runs // 2))
    dn, nm = statistics.median(down), statistics.median(normals)
    say(f"the same fragment's next stages: voxel_down_sample(0.03) {dn:.3f} ms, estimate_normals(radius 0.1, 30 neighbours, grid build "
        f"included) {nm:.3f} ms; fuse + extract calls = {100 * (f + x) / (dn + nm):.0f} % of the two")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
