"""Descriptor matching (epn_pointcloud_amd.matching, csrc/desc_match.hip) next to what a user would write instead.

Workload: one scene of 60 fragments x 5000 keypoints x 64-d unit descriptors (in every fragment after the first, two rows of
three are noisy copies of rows of fragment 0), 200 fragment pairs, random rigid ground-truth transforms.  Timed with HIP
events after warm-up, median of --runs:
  * the two library calls of evaluate_scene (nn_match: memset + sweep + finish; match_inliers) for the whole scene, and the
    wall time of evaluate_scene itself (tables, copies back and the per-pair compaction on the host included);
  * the same scene pair by pair (evaluate_fragment_pair, wall time);
  * torch.cdist + argmin in both directions for every pair, on the GPU (no masks, no tie rule, expanded-form distances);
  * sklearn KDTree build + query in both directions on --host-threads processes for --host-pairs pairs, scaled to 200;
  * describe() on ONE 262 144-point fragment with 5000 keypoints (default build_inv network), scaled to the 60 fragments: the
    matching's share of producing the descriptors it consumes (skipped with --no-describe).
The sweep does 2 C lane-operations (a subtraction and an FMA) per (query, target) pair: the tool prints the achieved rate
next to the chip's fp32 vector rate (256 CUs x 128 lanes x 2.4 GHz; MI355X_MICROARCH figures).

    python tools/match_bench.py [--frags 60] [--k 5000] [--c 64] [--pairs 200] [--runs 10] [--host-pairs 4] [--no-describe]
"""
import argparse
import multiprocessing
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


def wall_ms(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return times


def make_scene(frags, k, c, pairs, seed):
    rng = np.random.default_rng(seed)
    unit = lambda x: x / np.linalg.norm(x, axis=1, keepdims=True)
    base = unit(rng.standard_normal((k, c)))
    feats = [base]
    for _ in range(frags - 1):
        x = unit(rng.standard_normal((k, c)))
        copy = rng.random(k) < 2.0 / 3.0
        x[copy] = unit(base[rng.integers(0, k, int(copy.sum()))] + 0.05 * rng.standard_normal((int(copy.sum()), c)))
        feats.append(x)
    kps = [rng.uniform(0, 3, (k, 3)) for _ in range(frags)]
    pr = np.stack([rng.choice(frags, 2, replace=False) for _ in range(pairs)]).astype(np.int32)
    gts = np.tile(np.eye(4), (pairs, 1, 1))
    for g in gts:
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        g[:3, :3], g[:3, 3] = q * np.sign(np.linalg.det(q)), rng.uniform(-1, 1, 3)
    return [f.astype(np.float32) for f in feats], [x.astype(np.float32) for x in kps], pr, gts


def _kdtree_pair(args):
    from sklearn.neighbors import KDTree
    a, b = args
    KDTree(b).query(a, k=1)
    KDTree(a).query(b, k=1)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frags", type=int, default=60)
    ap.add_argument("--k", type=int, default=5000)
    ap.add_argument("--c", type=int, default=64)
    ap.add_argument("--pairs", type=int, default=200)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--host-pairs", type=int, default=4)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--no-describe", action="store_true")
    a = ap.parse_args()
    from epn_pointcloud_amd import _lib, matching, models as M
    from epn_pointcloud_amd.vgtk.cuda import grouping
    _lib.get_lib()
    dev = torch.device("cuda:0")
    feats, kps, pairs, gts = make_scene(a.frags, a.k, a.c, a.pairs, 2913)
    dfeats, dkps = [torch.from_numpy(f).to(dev) for f in feats], [torch.from_numpy(x).to(dev) for x in kps]
    print(f"match_bench: {a.frags} fragments x {a.k} keypoints x {a.c}-d, {a.pairs} pairs, device = {torch.cuda.get_device_name(0)}")

    all_feats, all_kps = torch.cat(dfeats), torch.cat(dkps)
    frag_off = np.arange(a.frags + 1, dtype=np.int64) * a.k
    nn = statistics.median(event_ms(lambda: grouping.nn_match(all_feats, frag_off, pairs), a.runs, 2))
    nn_idx = grouping.nn_match(all_feats, frag_off, pairs)[0]
    inl = statistics.median(event_ms(lambda: grouping.match_inliers(all_kps, frag_off, pairs, nn_idx, gts, 0.1), a.runs, 2))
    lane_ops = 2.0 * a.c * 2 * a.pairs * a.k * a.k
    peak = 256 * 128 * 2.4e9
    print(f"nn_match, whole scene in one launch: median {nn:.2f} ms of {a.runs} runs = {lane_ops / nn / 1e9:.1f} T lane-ops/s "
          f"({100 * lane_ops / (nn * 1e-3) / peak:.0f} % of the {peak / 1e12:.1f} T/s fp32 vector rate); match_inliers: {inl:.3f} ms")
    scene = lambda: matching.evaluate_scene(dkps, dfeats, None, pairs, gts, tau1=0.1)
    whole = statistics.median(wall_ms(scene, a.runs, 1))
    r = scene()
    print(f"evaluate_scene (wall, host tables / copies / compaction included): median {whole:.1f} ms; "
          f"mean matches per pair {r.n_match.mean():.0f}, recall {r.recall}")

    def per_pair():
        for p, (s, t) in enumerate(pairs):
            matching.evaluate_fragment_pair(dkps[s], dkps[t], dfeats[s], dfeats[t], gts[p], tau1=0.1)
    single = statistics.median(wall_ms(per_pair, max(1, a.runs // 3), 1))
    print(f"the same scene pair by pair (evaluate_fragment_pair x {a.pairs}, wall): median {single:.1f} ms = {single / whole:.2f}x the one-launch form")

    def cdist_scene():
        for s, t in pairs:
            d = torch.cdist(dfeats[s], dfeats[t])
            d.argmin(dim=1), d.argmin(dim=0)
    cd = statistics.median(event_ms(cdist_scene, a.runs, 1))
    print(f"torch.cdist + argmin (both directions from one matrix, {a.pairs} pairs, no masks / tie rule): median {cd:.2f} ms "
          f"= {cd / nn:.2f}x nn_match")

    try:
        import sklearn  # noqa: F401
    except ImportError:
        print("host form (sklearn KDTree, both directions): NOT TIMED, sklearn is not installed")
    else:
        jobs = [(feats[s], feats[t]) for s, t in pairs[:a.host_pairs * a.host_threads]]
        t0 = time.perf_counter()
        with multiprocessing.get_context("spawn").Pool(a.host_threads) as pool:
            pool.map(_kdtree_pair, jobs)
        host = (time.perf_counter() - t0) * a.pairs / len(jobs)
        print(f"host form (sklearn KDTree build + query, both directions, {a.host_threads} processes, {len(jobs)} pairs scaled to "
              f"{a.pairs}, pool start-up included): {host:.1f} s = {1e3 * host / nn:.0f}x nn_match")

    if not a.no_describe:
        rng = np.random.default_rng(1)
        pc = torch.from_numpy(rng.uniform(0.0, 3.0, (262144, 3)).astype(np.float32)).to(dev)
        rows = torch.from_numpy(rng.choice(262144, a.k, replace=False)).to(dev)
        model = M.build_inv(input_num=2048, search_radius=0.4).to(dev).eval()
        model.describe(pc, rows[:64])
        d = wall_ms(lambda: model.describe(pc, rows), 1, 0)[0]
        print(f"describe() of one 262 144-point fragment, {a.k} keypoints (fp32 features): {d:.0f} ms -> {a.frags} fragments: "
              f"{d * a.frags / 1e3:.1f} s; evaluate_scene / describe = {100 * whole / (d * a.frags):.3f} %")


if __name__ == "__main__":
    main()
