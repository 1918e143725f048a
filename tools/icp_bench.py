"""Price of the ICP stage (csrc/icp_refine.hip) on a fragment pair, beside the stages around it and a torch formulation:
python tools/icp_bench.py [--reps 7] > profiles/icp_refine.txt   (needs the GPU).

The workload is tools/grid_nn_bench.py's synthetic room corner (floor and two walls, about 366 000 points at the density of
an 8 mm lattice): the target is one sample of it, the source a second, independent sample moved by 2 degrees and (3, -2, 1) cm, 3.7 cm in all; the
stage starts from the identity.  Both variants run with open3d's default criteria; point-to-plane takes the target's normals
from PointGrid.normals.  Beside them: the grid build the stage needs, the RANSAC stage on 5 000 planted keypoint matches (the
stage in front of this one), and ONE iteration of ICP written in torch (cdist in row chunks + argmin, then the Horn fit through
torch.linalg.svd) on --torch-points of the source rows.  The table also gives that row scaled to the whole source and to the
updates the device's point-to-point run made plus its stopping iteration: an estimate, marked as one, not a measurement.

All forms run in one process, alternating rep by rep, timed with HIP events on the current stream after a warm-up; the table
gives the median and the minimum."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from epn_pointcloud_amd import correspondence as C          # noqa: E402
from epn_pointcloud_amd import matching as M                # noqa: E402
from epn_pointcloud_amd.vgtk.cuda import grouping           # noqa: E402
from tools.grid_nn_bench import room_corner                 # noqa: E402


def rigid(deg, t):
    a = np.radians(deg)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    T[:3, 3] = t
    return T


def torch_iteration(src, tgt, T, max_dist, chunk=2048):
    """One point-to-point iteration in torch, fp32 search and fp64 fit."""
    q = (src.double() @ T[:3, :3].T + T[:3, 3]).float()
    idx = torch.empty(q.shape[0], dtype=torch.int64, device=q.device)
    d = torch.empty(q.shape[0], dtype=torch.float32, device=q.device)
    for a in range(0, q.shape[0], chunk):
        d[a:a + chunk], idx[a:a + chunk] = torch.cdist(q[a:a + chunk], tgt).min(dim=1)
    keep = d <= max_dist
    p, qq = tgt[idx[keep]].double(), q[keep].double()
    pb, qb = p.mean(0), qq.mean(0)
    U, _, Vt = torch.linalg.svd((p - pb).T @ (qq - qb))
    D = torch.diag(torch.tensor([1.0, 1.0, float(torch.sign(torch.det(U @ Vt)))], dtype=torch.float64, device=q.device))
    R = U @ D @ Vt
    out = torch.eye(4, dtype=torch.float64, device=q.device)
    out[:3, :3], out[:3, 3] = R @ T[:3, :3], R @ T[:3, 3] + (pb - R @ qb)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--torch-points", type=int, default=32768, help="source rows of the torch formulation (scaled up in the table)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    tgt_h, fresh = room_corner(rng), room_corner(rng)
    inv = np.linalg.inv(rigid(2.0, [0.03, -0.02, 0.01]))
    src_h = (fresh.astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    src, tgt = torch.from_numpy(src_h).to(dev), torch.from_numpy(tgt_h).to(dev)
    max_dist, radius = 0.1, 0.1
    grid = C.PointGrid(tgt, max(max_dist, radius))
    normals = grid.normals(radius=radius, max_nn=30, view=[1.5, 1.5, 1.2]).normals
    T0 = torch.eye(4, dtype=torch.float64, device=dev)

    K = 5000
    kp_t = tgt[torch.randperm(tgt.shape[0], device=dev)[:K]]
    truth = torch.as_tensor(rigid(2.0, [0.03, -0.02, 0.01]), device=dev)
    kp_s = (kp_t.double() @ truth[:3, :3].T + truth[:3, 3]).float()
    feats = torch.randn(K, 32, device=dev)

    results = {}

    def icp(n):
        def run():
            results[n is not None] = grouping.icp_refine(grid._workspace, grid.n, src, T0, max_dist, tgt_normals=n)
        return run

    sub = src[:args.torch_points]
    forms = {
        f"build   target grid, n = {tgt.shape[0]}, max_radius {max(max_dist, radius)}": lambda: C.PointGrid(tgt, max(max_dist, radius)),
        f"normals of the target, radius {radius}, max_nn 30": lambda: grid.normals(radius=radius, max_nn=30),
        f"ransac  register_scene, {K} planted matches, 4096 hypotheses": lambda: M.register_scene([kp_s, kp_t], [feats, feats], None, [[0, 1]]),
        f"icp     point-to-point, m = {src.shape[0]}, max_iter 30 (whole call, no read-back)": icp(None),
        f"icp     point-to-plane, m = {src.shape[0]}, max_iter 30 (whole call, no read-back)": icp(normals),
        f"torch   ONE point-to-point iteration, {sub.shape[0]} of the source rows (cdist chunks + svd)":
            lambda: torch_iteration(sub, tgt, T0, max_dist),
    }

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    times = {k: [] for k in forms}
    for fn in forms.values():
        fn()                                                       # warm-up
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for k, fn in forms.items():
            times[k].append(timed(fn))

    print(f"# tools/icp_bench.py --reps {args.reps} on {torch.cuda.get_device_name(0)}; HIP events, ms; forms alternate rep by rep")
    print(f"# src {src.shape[0]} / tgt {tgt.shape[0]} points; max_dist {max_dist}; the source is off by 2 degrees and 3.7 cm")
    for plane, out in sorted(results.items()):
        T, trace, iterations, status = (t.cpu().numpy() for t in out[:4])
        rre, rte = M.registration_errors(T, truth.cpu().numpy())
        print(f"# {'point-to-plane' if plane else 'point-to-point'}: {int(iterations[0])} updates, status {int(status[0])}, "
              f"rre {rre[0]:.4f} deg, rte {rte[0]:.5f} m")
    print("# the torch row is ONE iteration on a part of the source; scale it by the rows and by the updates above to compare")
    print(f"{'form':<96} {'median':>9} {'min':>9} {'reps':>5}")
    for k, v in times.items():
        print(f"{k:<96} {statistics.median(v):9.3f} {min(v):9.3f} {len(v):5d}")
    torch_key = [k for k in times if k.startswith("torch")][0]
    searches = int(results[False][2].cpu()[0]) + (1 if int(results[False][3].cpu()[0]) else 0)
    factor = src.shape[0] / sub.shape[0] * searches
    print(f"# estimate, not measured: the torch iteration x {src.shape[0] / sub.shape[0]:.2f} (rows) x {searches} (searches of the "
          f"point-to-point run) = {statistics.median(times[torch_key]) * factor:.0f} ms for the same work")


if __name__ == "__main__":
    main()
