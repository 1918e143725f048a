"""Patch extraction (vgtk.pc.radius_patches, csrc/patch_extract.hip) next to the network that consumes the patches.

Workload: one fragment of n = 262 144 points uniform in a 3 x 3 x 3 box, k = 5000 keypoints drawn from them, radius 0.4,
n_sample = 2048 -- the shape of a 3DMatch fragment in front of the default build_inv network.  Timed with HIP events:
  * the extraction, median of 20 runs after warm-up; the same with n_sample = 8192, where every ball holds fewer points than
    samples and the kernel makes two sweeps of the fragment (count, emit) instead of four (count, two threshold passes, emit):
    the difference prices the threshold passes;
  * in the same process, the default build_inv network's forward over the 5000 patches (batches of 64, eval mode), fp32
    features and bf16 features;
  * the host form the reference uses (scipy KDTree + query_ball_point + np.random.choice), only if scipy is importable.
The claim to check: extraction < 10 % of the network's time on the same patches.

    python tools/patch_bench.py [--n 262144] [--k 5000] [--radius 0.4] [--n-sample 2048] [--runs 20] [--no-network]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def event_ms(fn, runs, warmup):
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


def network_ms(model, patches, batch):
    k = patches.shape[0]

    def sweep():
        for r0 in range(0, k, batch):
            x = patches[r0:r0 + batch]
            if x.shape[0] < batch:
                x = torch.cat((x, x.new_zeros(batch - x.shape[0], *x.shape[1:])))
            model(x)

    with torch.no_grad():
        model(patches[:batch])                        # warm-up: tables, workspaces
        return event_ms(sweep, 1, 0)[0]


def host_reference_s(pc, rows, radius, n_sample):
    from scipy.spatial import KDTree
    rng = np.random.default_rng(0)
    t0 = time.perf_counter()
    found = KDTree(pc).query_ball_point(pc[rows], radius)
    t1 = time.perf_counter()
    out = np.zeros((len(rows), n_sample, 3), dtype=np.float32)
    for q, members in enumerate(found):
        if len(members) > 1:
            m = np.asarray(members)
            pick = (rng.choice(m.size, n_sample, replace=False) if m.size >= n_sample
                    else np.concatenate((np.arange(m.size), rng.choice(m.size, n_sample - m.size, replace=True))))
            out[q] = pc[m[pick]]
    return t1 - t0, time.perf_counter() - t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--k", type=int, default=5000)
    ap.add_argument("--radius", type=float, default=0.4)
    ap.add_argument("--n-sample", type=int, default=2048)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--no-network", action="store_true")
    a = ap.parse_args()
    from epn_pointcloud_amd import _lib, models as M, schedule as S
    from epn_pointcloud_amd.vgtk import pc as pctk
    _lib.get_lib()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(2913)
    pc = rng.uniform(0.0, 3.0, (a.n, 3)).astype(np.float32)
    rows = rng.choice(a.n, a.k, replace=False)
    cloud, kp = torch.from_numpy(pc).to(dev), torch.from_numpy(rows).to(dev)
    print(f"patch_bench: n = {a.n}, k = {a.k}, radius = {a.radius}, n_sample = {a.n_sample}, device = {torch.cuda.get_device_name(0)}")

    t = event_ms(lambda: pctk.radius_patches(cloud, kp, a.radius, a.n_sample), a.runs, 3)
    extract = statistics.median(t)
    patches, _, counts = pctk.radius_patches(cloud, kp, a.radius, a.n_sample)
    c = counts.float()
    print(f"in-radius points per keypoint: min {int(c.min())}, mean {c.mean().item():.0f}, max {int(c.max())}; "
          f"{int((counts > a.n_sample).sum())} of {a.k} balls hold more than n_sample")
    print(f"extraction: median {extract:.3f} ms of {a.runs} runs (min {min(t):.3f}, max {max(t):.3f})")
    two = statistics.median(event_ms(lambda: pctk.radius_patches(cloud, kp, a.radius, 8192), a.runs, 3))
    print(f"extraction with n_sample = 8192 (count and emit sweeps only, 4x the output): median {two:.3f} ms "
          f"-> the two threshold sweeps of n_sample = {a.n_sample} cost at most {max(extract - two, 0.0):.3f} ms")

    if not a.no_network:
        model = M.build_inv(input_num=a.n_sample, search_radius=a.radius).to(dev).eval()
        for name, dt in (("fp32", None), ("bf16", torch.bfloat16)):
            if dt is not None:
                S.set_feature_dtype(model, dt)
            net = network_ms(model, patches, a.batch)
            print(f"network forward ({name} features) over the {a.k} patches, batches of {a.batch}: {net:.1f} ms "
                  f"({a.k / net * 1e3:.0f} clouds/s); extraction / network = {100.0 * extract / net:.2f} % "
                  f"(claim: < 10 %: {'holds' if extract < 0.1 * net else 'FAILS'})")

    try:
        import scipy  # noqa: F401
    except ImportError:
        print("host reference form (scipy KDTree + query_ball_point + np.random.choice): NOT TIMED, scipy is not installed")
        return
    search, resample = host_reference_s(pc, rows, a.radius, a.n_sample)
    print(f"host reference form on this machine's CPU, one process (scipy KDTree over the whole fragment + query_ball_point: "
          f"{search * 1e3:.0f} ms; np.random.choice resampling: {resample * 1e3:.0f} ms): {1e3 * (search + resample):.0f} ms "
          f"= {1e3 * (search + resample) / extract:.0f}x the extraction kernel")


if __name__ == "__main__":
    main()
