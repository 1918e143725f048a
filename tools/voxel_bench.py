"""Voxel-grid downsampling (vgtk.pc.voxel_down_sample, csrc/voxel_grid.hip) in front of the patch extraction.

Workload: one fragment of n = 262 144 points, the reference's two voxel sizes (0.03 below 1024 input points, 0.015 from there):
  * "box": uniform in a 3 x 3 x 3 box -- almost every point is its own voxel: the most slots claimed, the least contention;
  * "planes": a floor and two walls of a 3 x 3 x 3 room with 5 mm of noise -- the dense case of a real fragment: several points
    per voxel, so the atomics of a voxel's points meet on one slot.
Timed with HIP events, median of --runs after warm-up: the whole call as describe() makes it (allocations, the seven launches,
the one read-back of the status word), and the launches alone on preallocated buffers.  Next to it the host form on this
machine's CPU: the same keys in numpy, np.unique with inverse and counts, fp64 means by np.bincount.
The yardstick: the patch extraction that follows takes 6.42 ms for 5000 keypoints (profiles/patch_extract.txt).

    python tools/voxel_bench.py [--n 262144] [--runs 20]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PATCH_EXTRACT_MS = 6.42


def event_ms(fn, runs, warmup=3):
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


def clouds(n, rng):
    box = rng.uniform(0.0, 3.0, (n, 3)).astype(np.float32)
    planes = rng.uniform(0.0, 3.0, (n, 3))
    flat = rng.integers(0, 3, n)                                   # the coordinate that is pressed onto its plane
    planes[np.arange(n), flat] = rng.normal(0.0, 0.005, n)
    return {"box": box, "planes": planes.astype(np.float32)}


def launches_only(lib, _lib, cloud, voxel_size):
    """The C call on buffers allocated once: no allocation and no read-back inside the timed region."""
    n = cloud.shape[0]
    i32 = dict(dtype=torch.int32, device=cloud.device)
    cen = torch.empty((n, 3), dtype=torch.float32, device=cloud.device)
    cnt, first, pv, status = torch.empty(n, **i32), torch.empty(n, **i32), torch.empty(n, **i32), torch.empty(2, **i32)
    ws_bytes = int(lib.epn_voxel_downsample_workspace_bytes(n))
    ws = torch.empty(((ws_bytes + 7) // 8,), dtype=torch.int64, device=cloud.device)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())

    def call():
        _lib.check(lib.epn_voxel_downsample_f32(ptr(cloud), n, voxel_size, ptr(cen), ptr(cnt), ptr(first), ptr(pv), ptr(status),
                                                ptr(ws), ws.numel() * 8, _lib.stream_of(cloud)), "voxel_downsample")
    return call, ws_bytes


def host_unique_ms(pc, voxel_size):
    t0 = time.perf_counter()
    p = pc.astype(np.float64)
    idx = np.floor((p - (pc.min(axis=0).astype(np.float64) - 0.5 * voxel_size)) / voxel_size).astype(np.int64)
    key = (idx[:, 0] << 42) | (idx[:, 1] << 21) | idx[:, 2]
    _, inverse, counts = np.unique(key, return_inverse=True, return_counts=True)
    np.stack([np.bincount(inverse, weights=p[:, c]) for c in range(3)], axis=1) / counts[:, None]
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--runs", type=int, default=20)
    a = ap.parse_args()
    from epn_pointcloud_amd import _lib
    from epn_pointcloud_amd.vgtk import pc as pctk
    lib = _lib.get_lib()
    dev = torch.device("cuda:0")
    print(f"voxel_bench: n = {a.n}, median of {a.runs} runs, device = {torch.cuda.get_device_name(0)}; yardstick: patch extraction "
          f"{PATCH_EXTRACT_MS} ms for 5000 keypoints (profiles/patch_extract.txt)")
    for name, pc in clouds(a.n, np.random.default_rng(2913)).items():
        cloud = torch.from_numpy(pc).to(dev)
        for vs in (0.03, 0.015):
            m = pctk.voxel_down_sample(cloud, vs)[0].shape[0]
            whole = event_ms(lambda: pctk.voxel_down_sample(cloud, vs), a.runs)
            call, ws_bytes = launches_only(lib, _lib, cloud, vs)
            alone = event_ms(call, a.runs)
            host = statistics.median(host_unique_ms(pc, vs) for _ in range(3))
            w, k = statistics.median(whole), statistics.median(alone)
            print(f"{name:6s} voxel_size {vs}: {m} voxels ({a.n / m:.2f} points per voxel), workspace {ws_bytes / 2 ** 20:.1f} MiB; "
                  f"call {w:.3f} ms (min {min(whole):.3f}, max {max(whole):.3f}) = {100 * w / PATCH_EXTRACT_MS:.1f} % of the patch "
                  f"extraction; launches alone {k:.3f} ms (min {min(alone):.3f}, max {max(alone):.3f}); host np.unique form "
                  f"{host:.1f} ms = {host / w:.0f}x the call")


if __name__ == "__main__":
    main()
