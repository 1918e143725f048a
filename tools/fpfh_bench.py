"""Price of the FPFH stage (csrc/fpfh.hip) on the keypoint stage's shapes, against the normals stage on the same cloud and the
numpy restatement:  python tools/fpfh_bench.py [--reps 7] > profiles/fpfh.txt   (needs the GPU).

The synthetic room corner of tools/grid_nn_bench.py.  Two shapes: its 0.05 m voxel centroids (about 9 500) at radius 0.15, the
reference's call (run_keypoint.py:40-50), and the raw cloud (about 366 000 points at the density of an 8 mm lattice) at the
radius that gives a comparable neighbour count, 0.15 * 0.008 / 0.05 = 0.024.

All device forms run in one process, alternating rep by rep, timed with HIP events on the current stream; the table gives the
median and the minimum.  The two launches of a call are priced apart from a torch.profiler run of the same calls (kernel
averages by name) where the profiler reports device kernels.  The numpy restatement (tests/fpfh_ref.py: brute force over all
pairs) is one run on one process, wall clock, on the centroid shape only; the all-pairs sweep is out of reach on the raw cloud.
A restatement spread over 16 processes is not built."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from epn_pointcloud_amd import correspondence as C          # noqa: E402
from epn_pointcloud_amd.vgtk import pc as pctk              # noqa: E402
from grid_nn_bench import room_corner                       # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-numpy", action="store_true", help="skip the host restatement")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    raw_h = room_corner(np.random.default_rng(0))
    raw = torch.from_numpy(raw_h).to(dev)
    cen = pctk.voxel_down_sample(raw, 0.05)[0]
    view = [1.5, 1.2, 1.5]
    print(f"# tools/fpfh_bench.py --reps {args.reps} on {torch.cuda.get_device_name(0)}; HIP events, ms; forms alternate rep by rep")
    shapes = (("centroids", cen, 0.15), ("raw", raw, 0.024))
    forms, notes = {}, []
    for name, pts, r in shapes:
        grid = C.PointGrid(pts, r)
        normals = grid.normals(None, r, max_nn=30, view=view).normals
        out = grid.fpfh(normals, r)
        cnt = out.count.float()
        notes.append(f"# {name}: n = {pts.shape[0]}, radius {r}: neighbours median {int(cnt.median())}, mean {float(cnt.mean()):.1f}, "
                     f"max {int(cnt.max())}; {int((out.flags != 0).sum())} flagged rows")
        forms[f"{name:<10} grid build"] = lambda pts=pts, r=r: C.PointGrid(pts, r)
        forms[f"{name:<10} estimate_normals (max_nn = 30, view)"] = lambda g=grid, r=r: g.normals(None, r, max_nn=30, view=view)
        forms[f"{name:<10} fpfh, both launches"] = lambda g=grid, nr=normals, r=r: g.fpfh(nr, r)
    for fn in forms.values():
        fn()
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(args.reps):
        for k, fn in forms.items():
            times[k].append(timed(fn))
    print("\n".join(notes))
    print(f"{'form':<72} {'median':>9} {'min':>9} {'reps':>5}")
    for k, v in times.items():
        print(f"{k:<72} {statistics.median(v):9.3f} {min(v):9.3f} {len(v):5d}")

    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(args.reps):
                for k, fn in forms.items():
                    if "fpfh" in k:
                        fn()
            torch.cuda.synchronize()
        rows = [e for e in prof.key_averages() if "fpfh_kernel" in e.key or "spfh_kernel" in e.key]
        if not rows:
            print("# torch.profiler reported no device kernels: the two launches are not priced apart")
        for e in rows:
            total = getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0)
            print(f"# profiler: {e.key[:60]:<60} calls {e.count:4d}  mean over both shapes {total / max(e.count, 1) / 1e3:9.3f} ms")
    except Exception as exc:                                        # the profiler is optional equipment
        print(f"# torch.profiler did not run ({type(exc).__name__}): the two launches are not priced apart")

    if not args.no_numpy:
        import fpfh_ref as F
        pts, r = cen.cpu().numpy(), 0.15
        nr = C.PointGrid(cen, r).normals(None, r, max_nn=30, view=view).normals.cpu().numpy()
        t0 = time.perf_counter()
        F.point_fpfh(pts, nr, r)
        print(f"{'centroids  numpy restatement, all pairs, one process, wall clock, one run':<72} {(time.perf_counter() - t0) * 1e3:9.1f}")


if __name__ == "__main__":
    main()
