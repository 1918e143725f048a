"""Price of the normals stage (csrc/point_normals.hip) on a fragment-sized cloud, against a host form and against the patch
extraction that follows it:  python tools/normals_bench.py [--reps 7] > profiles/normals.txt   (needs the GPU).

The cloud is tools/grid_nn_bench.py's room corner: the floor and two walls sampled uniformly at random at the density of an 8 mm
lattice (about 366 000 points).  radius = 2.5 lattice pitches = 0.02 m, max_nn = 30: open3d's KDTreeSearchParamHybrid at the
scale the reference's fused fragments are estimated at.

All device forms run in one process, alternating rep by rep after a warm-up of every form, timed with HIP events on the current
stream; the table gives the median and the minimum in ms.  Forms: the grid's build; the normals of every point with the cut
(max_nn = 30), without it (max_nn = 0) and with the moments and neighbour rows written out; the patch stage of one fragment
(voxel_down_sample at 0.015, radius_patches of 2048 keypoints at 0.3 m to 1024 points) and orient_patches on its result.  Host
form, wall clock, one run: scipy's cKDTree (query of the 30 nearest within the radius, workers = 16) and a batched
numpy.linalg.eigh of the covariances, if scipy imports; otherwise the numpy restatement of tests/normals_ref.py on a subsample,
scaled to the cloud -- the output says which."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from epn_pointcloud_amd import correspondence as C          # noqa: E402
from epn_pointcloud_amd.vgtk import pc as pctk              # noqa: E402
from grid_nn_bench import room_corner                       # noqa: E402


def host_scipy(pts, radius, max_nn):
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    tree = cKDTree(pts)
    t1 = time.perf_counter()
    dist, idx = tree.query(pts, k=max_nn, distance_upper_bound=radius, workers=16)
    t2 = time.perf_counter()
    ok = np.isfinite(dist)
    nb = pts[np.where(ok, idx, 0)].astype(np.float64) - pts[:, None, :].astype(np.float64)
    nb[~ok] = 0.0
    k = ok.sum(axis=1)[:, None]
    mean = nb.sum(axis=1) / k
    cov = np.einsum("nki,nkj->nij", nb, nb) / k[:, :, None] - mean[:, :, None] * mean[:, None, :]
    np.linalg.eigh(cov)
    t3 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3


def host_numpy(pts, radius, max_nn, sample=200):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import normals_ref
    t0 = time.perf_counter()
    normals_ref.point_normals(pts, pts[:sample], radius, max_nn=max_nn)
    return (time.perf_counter() - t0) * 1e3 * pts.shape[0] / sample


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    pts_h = room_corner(rng)
    pts = torch.from_numpy(pts_h).to(dev)
    radius, max_nn = 0.02, 30
    grid = C.PointGrid(pts, radius)
    view = torch.tensor([1.5, 1.5, 1.2], device=dev)
    down = pctk.voxel_down_sample(pts, 0.015)[0]
    kpts = pts[torch.from_numpy(rng.choice(pts.shape[0], 2048, replace=False)).to(dev)].contiguous()
    patches = pctk.radius_patches(down, kpts, 0.3, 1024)[0]
    kp_normals = grid.normals(kpts, radius, max_nn=max_nn, view=view).normals

    forms = {
        f"build    grid, n = {pts.shape[0]}, max_radius {radius}": lambda: C.PointGrid(pts, radius),
        f"normals  every point, r = {radius}, max_nn = {max_nn}, view": lambda: grid.normals(None, radius, max_nn=max_nn, view=view),
        f"normals  every point, r = {radius}, max_nn = 0 (no cut)": lambda: grid.normals(None, radius, max_nn=0),
        f"normals  every point, max_nn = {max_nn}, moments and neighbour rows written":
            lambda: grid.normals(None, radius, max_nn=max_nn, return_moments=True, return_neighbors=True),
        f"normals  {kpts.shape[0]} keypoints only, max_nn = {max_nn}": lambda: grid.normals(kpts, radius, max_nn=max_nn, view=view),
        f"patches  voxel_down_sample at 0.015 ({down.shape[0]} centroids)": lambda: pctk.voxel_down_sample(pts, 0.015),
        f"patches  radius_patches, {kpts.shape[0]} keypoints, r = 0.3, 1024 points": lambda: pctk.radius_patches(down, kpts, 0.3, 1024),
        f"patches  orient_patches, {kpts.shape[0]} x 1024": lambda: pctk.orient_patches(patches, kp_normals),
    }

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    times = {k: [] for k in forms}
    for _ in range(2):
        for fn in forms.values():
            fn()                                                   # warm-up
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for k, fn in forms.items():
            times[k].append(timed(fn))
    fit = grid.normals(None, radius, max_nn=max_nn, view=view)
    cut = (fit.count > max_nn).float().mean().item()

    print(f"# tools/normals_bench.py --reps {args.reps} on {torch.cuda.get_device_name(0)}; HIP events, ms; forms alternate rep by rep")
    print(f"# {pts.shape[0]} points; in-radius count: median {int(fit.count.median())}, max {int(fit.count.max())}; "
          f"{cut:.1%} of the queries take the max_nn cut; flags: {int((fit.flags & 1 != 0).sum())} with fewer than 3 "
          f"neighbours, {int((fit.flags & 4 != 0).sum())} undetermined")
    print("# the build and voxel_down_sample include their status read-backs (host synchronisations)")
    print(f"{'form':<88} {'median':>9} {'min':>9} {'reps':>5}")
    for k, v in times.items():
        print(f"{k:<88} {statistics.median(v):9.3f} {min(v):9.3f} {len(v):5d}")
    try:
        build, query, solve = host_scipy(pts_h, radius, max_nn)
        print(f"{'host     scipy cKDTree build / query (k = 30 within r, 16 workers) / covariance + eigh; wall clock, one run':<88} "
              f"{build:9.1f} {query:9.1f} {solve:9.1f}")
    except ImportError:
        print(f"{'host     numpy restatement on 200 queries, scaled to the cloud (scipy does not import); wall clock':<88} "
              f"{host_numpy(pts_h, radius, max_nn):9.1f}")


if __name__ == "__main__":
    main()
