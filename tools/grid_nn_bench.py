"""Price of the point grid (csrc/point_grid.hip) on the keypoint stage's shapes, against an all-pairs sweep on the device and a
host tree:  python tools/grid_nn_bench.py [--reps 7] > profiles/grid_nn.txt   (needs the GPU).

Synthetic fragments the size of the reference's: the floor (3 m x 3 m) and two walls (3 m x 2.4 m) of a room corner, sampled
uniformly at random at the density of an 8 mm lattice (about 366 000 points); the target is a second, independent sample of the
same surfaces moved 0.3 m along x.  Their 0.05 m voxel centroids (about 10 000) are the sparse clouds.

All forms run in one process, alternating rep by rep, timed with HIP events on the current stream; the table gives the median
and the minimum.  Forms: the grid's build and queries at the four radii of one keypoint_pairs call and of fragment_overlap;
torch.cdist + argmin in row chunks on the device for the same two searches (raw overlap, centroid cross match); and, where it
imports, sklearn.neighbors.NearestNeighbors (kd_tree, n_jobs = 16) on the host, wall clock, tree build and query separately."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from epn_pointcloud_amd import correspondence as C          # noqa: E402
from epn_pointcloud_amd.vgtk import pc as pctk              # noqa: E402


def room_corner(rng, pitch=0.008):
    def plane(a, b, fixed_axis):
        n = int(a * b / pitch ** 2)
        uv = rng.uniform(0, 1, (n, 2)) * [a, b]
        return np.insert(uv, fixed_axis, 0.0, axis=1)
    return np.vstack((plane(3, 3, 2), plane(3, 2.4, 1), plane(3, 2.4, 0))).astype(np.float32)


def cdist_nn(qry, ref, chunk):
    idx = torch.empty(qry.shape[0], dtype=torch.int64, device=qry.device)
    d = torch.empty(qry.shape[0], dtype=torch.float32, device=qry.device)
    for a in range(0, qry.shape[0], chunk):
        d[a:a + chunk], idx[a:a + chunk] = torch.cdist(qry[a:a + chunk], ref).min(dim=1)
    return idx, d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--slow-reps", type=int, default=2, help="reps of the all-pairs sweep over the raw clouds")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    src_h = room_corner(rng)
    tgt_h = room_corner(rng) + np.float32([0.3, 0, 0])
    src, tgt = torch.from_numpy(src_h).to(dev), torch.from_numpy(tgt_h).to(dev)
    voxel, iso, match, margin = 0.05, 0.15, 0.03, 0.075
    R = C.raw_radius(voxel)
    cs, ct = pctk.voxel_down_sample(src, voxel)[0], pctk.voxel_down_sample(tgt, voxel)[0]
    g_raw_t, g_raw_s = C.PointGrid(tgt, max(R, margin)), C.PointGrid(src, max(R, margin))
    g_iso = C.PointGrid(cs, iso)
    keep_t = C.PointGrid(ct, iso).nearest(ct, iso, exclude_self=True)[0] >= 0
    g_match = C.PointGrid(ct, match, valid=keep_t)
    sel = torch.nonzero(g_match.nearest(cs, match)[0] >= 0).reshape(-1)
    kept = cs[sel]

    forms = {
        f"build   raw grid, n = {tgt.shape[0]}, max_radius {max(R, margin):.4f}": lambda: C.PointGrid(tgt, max(R, margin)),
        f"build   centroid grid, n = {ct.shape[0]}, max_radius {iso}": lambda: C.PointGrid(ct, iso),
        f"query   isolation: {cs.shape[0]} centroids in their own grid, r = {iso}": lambda: g_iso.nearest(cs, iso, exclude_self=True),
        f"query   cross match: {cs.shape[0]} centroids in the kept target centroids, r = {match}": lambda: g_match.nearest(cs, match),
        f"query   map back: {kept.shape[0]} centroids in the raw source, r = {R:.4f}": lambda: g_raw_s.nearest(kept, R),
        f"query   fragment_overlap: {src.shape[0]} raw points in the raw target grid, r = {margin}":
            lambda: C.fragment_overlap(src, g_raw_t, margin),
        f"whole   keypoint_pairs with prebuilt raw grids": lambda: C.keypoint_pairs(g_raw_s, g_raw_t),
        f"cdist   cross match: {cs.shape[0]} x {ct.shape[0]}, one chunk": lambda: cdist_nn(cs, ct, 16384),
    }
    slow = {f"cdist   fragment_overlap: {src.shape[0]} x {tgt.shape[0]}, chunks of 2048 rows": lambda: cdist_nn(src, tgt, 2048)}

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    times = {k: [] for k in list(forms) + list(slow)}
    for fn in forms.values():
        fn()                                                       # warm-up
    torch.cuda.synchronize()
    for rep in range(args.reps):
        for k, fn in forms.items():
            times[k].append(timed(fn))
        if rep < args.slow_reps:
            for k, fn in slow.items():
                times[k].append(timed(fn))

    print(f"# tools/grid_nn_bench.py --reps {args.reps} on {torch.cuda.get_device_name(0)}; HIP events, ms; forms alternate rep by rep")
    print(f"# src {src.shape[0]} / tgt {tgt.shape[0]} raw points, {cs.shape[0]} / {ct.shape[0]} centroids at {voxel}; "
          f"{int(keep_t.sum())} target centroids kept, {kept.shape[0]} matched")
    print(f"# the builds and fragment_overlap / keypoint_pairs include their status read-backs (host synchronisations)")
    print(f"{'form':<96} {'median':>9} {'min':>9} {'reps':>5}")
    for k, v in times.items():
        print(f"{k:<96} {statistics.median(v):9.3f} {min(v):9.3f} {len(v):5d}")

    try:
        from sklearn.neighbors import NearestNeighbors
    except ImportError:
        print("# sklearn does not import on this machine: no host tree measured")
        return
    os.environ.setdefault("OMP_NUM_THREADS", "16")
    for name, ref, qry in (("fragment_overlap (raw in raw)", tgt_h, src_h), ("cross match (centroids)", ct.cpu().numpy(), cs.cpu().numpy())):
        t0 = time.perf_counter()
        nn = NearestNeighbors(n_neighbors=1, algorithm="kd_tree", n_jobs=16).fit(ref)
        t1 = time.perf_counter()
        nn.kneighbors(qry)
        t2 = time.perf_counter()
        print(f"{'sklearn ' + name + ': kd_tree fit / query, 16 threads, wall clock, one run':<96} {(t1 - t0) * 1e3:9.1f} {(t2 - t1) * 1e3:9.1f}")


if __name__ == "__main__":
    main()
