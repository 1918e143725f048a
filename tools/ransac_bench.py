"""Pairwise registration (epn_pointcloud_amd.matching.register_scene, csrc/ransac_register.hip) next to what precedes it and
what a user would run instead.  Writes its report to --out (default profiles/ransac_register.txt) and prints it.

Workload: one scene of 60 fragments x 5000 keypoints x 64-d unit descriptors, 200 fragment pairs, H = 4096 hypotheses per
pair.  Fragment f is a rigid motion T_f of a base cloud: in every fragment after the first, two rows of three are noisy
copies of rows of fragment 0 (descriptor noise 0.05 per component, keypoint noise 0.005 per coordinate after the motion),
the rest are random; so a pair (s, t) has the transform T_s T_t^-1 and a share of its mutual matches follows it.
Timed with HIP events after warm-up, median / min / max of --runs:
  * the registration call (grouping.ransac_register: allocations + compact, score, finish) for the whole scene;
  * the nearest-neighbour call that precedes it (grouping.nn_match) and the mutual check (grouping.match_inliers);
  * the numpy restatement (tests/ransac_ref.py: philox draws, batched SVD fits, chunked scoring) on --host-threads processes
    for --host-pairs x --host-threads pairs, scaled to the scene (pool start-up included).
It also checks the result: registration recall against the planted transforms (RRE < 15 degrees, RTE < 0.3) and best_h /
n_inlier against the restatement on the host-timed pairs.  The scoring does 15 fp64 lane-operations per (hypothesis,
correspondence): the tool prints the achieved rate.

    python tools/ransac_bench.py [--frags 60] [--k 5000] [--c 64] [--pairs 200] [--hyp 4096] [--runs 10] [--host-pairs 1]
"""
import argparse
import multiprocessing
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TAU, MIN_MARGIN, SEED = 0.05, 1e-2, 7


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


def fmt(times):
    return f"median {statistics.median(times):.3f} ms (min {min(times):.3f}, max {max(times):.3f}, {len(times)} runs)"


def make_scene(frags, k, c, pairs, seed):
    import ransac_ref as R
    rng = np.random.default_rng(seed)
    unit = lambda x: x / np.linalg.norm(x, axis=1, keepdims=True)
    base_f, base_x = unit(rng.standard_normal((k, c))), rng.uniform(-1.5, 1.5, (k, 3))
    motions = [np.eye(4)] + [R.random_rigid(rng) for _ in range(frags - 1)]
    feats, kps = [base_f], [base_x]
    for f in range(1, frags):
        x, xyz = unit(rng.standard_normal((k, c))), rng.uniform(-2.5, 2.5, (k, 3))
        copy = np.flatnonzero(rng.random(k) < 2.0 / 3.0)
        rows = rng.integers(0, k, copy.size)
        x[copy] = unit(base_f[rows] + 0.05 * rng.standard_normal((copy.size, c)))
        xyz[copy] = base_x[rows] @ motions[f][:3, :3].T + motions[f][:3, 3] + 0.005 * rng.standard_normal((copy.size, 3))
        feats.append(x)
        kps.append(xyz)
    pr = np.stack([rng.choice(frags, 2, replace=False) for _ in range(pairs)]).astype(np.int32)
    gts = np.stack([motions[s] @ np.linalg.inv(motions[t]) for s, t in pr])
    return [f.astype(np.float32) for f in feats], [x.astype(np.float32) for x in kps], pr, gts


def _host_pair(args):
    import ransac_ref as R
    x, y, p, hyp = args
    r = R.register_pair(x, y, TAU, hyp, SEED, p, MIN_MARGIN)
    return r["best_h"], r["n_inlier"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frags", type=int, default=60)
    ap.add_argument("--k", type=int, default=5000)
    ap.add_argument("--c", type=int, default=64)
    ap.add_argument("--pairs", type=int, default=200)
    ap.add_argument("--hyp", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--host-pairs", type=int, default=1)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ransac_register.txt"))
    a = ap.parse_args()
    import ransac_ref as R
    from epn_pointcloud_amd import _lib, matching
    from epn_pointcloud_amd.vgtk.cuda import grouping
    _lib.get_lib()
    dev = torch.device("cuda:0")
    feats, kps, pairs, gts = make_scene(a.frags, a.k, a.c, a.pairs, 2913)
    dfeats, dkps = [torch.from_numpy(f).to(dev) for f in feats], [torch.from_numpy(x).to(dev) for x in kps]
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"ransac_bench: {a.frags} fragments x {a.k} keypoints x {a.c}-d, {a.pairs} pairs, H = {a.hyp}, tau = {TAU}, "
        f"device = {torch.cuda.get_device_name(0)}")
    all_feats, all_kps = torch.cat(dfeats), torch.cat(dkps)
    frag_off = np.arange(a.frags + 1, dtype=np.int64) * a.k
    eye = np.tile(np.eye(4), (a.pairs, 1, 1))
    nn = event_ms(lambda: grouping.nn_match(all_feats, frag_off, pairs), a.runs, 2)
    nn_idx = grouping.nn_match(all_feats, frag_off, pairs)[0]
    mi = event_ms(lambda: grouping.match_inliers(all_kps, frag_off, pairs, nn_idx, eye, 0.0), a.runs, 2)
    match_src, _, n_match, _, tgt_off = grouping.match_inliers(all_kps, frag_off, pairs, nn_idx, eye, 0.0)
    reg = event_ms(lambda: grouping.ransac_register(all_kps, frag_off, pairs, match_src, tgt_off, TAU, a.hyp, SEED, MIN_MARGIN),
                   a.runs, 2)
    T, best_h, hyp_count, n_inlier, rmse, margin = (v.cpu().numpy() for v in grouping.ransac_register(
        all_kps, frag_off, pairs, match_src, tgt_off, TAU, a.hyp, SEED, MIN_MARGIN))
    M = n_match.cpu().numpy().astype(np.int64)
    ops = 15.0 * a.hyp * float(M.sum())
    med = statistics.median(reg)
    say(f"ransac_register, whole scene (allocations + compact, score, finish): {fmt(reg)}")
    say(f"  mutual matches per pair: mean {M.mean():.0f}, min {M.min()}, max {M.max()}; scoring = {ops / 1e9:.1f} G fp64 lane-ops "
        f"-> {ops / med / 1e9:.2f} T lane-ops/s over the whole call")
    say(f"nn_match, whole scene: {fmt(nn)}")
    say(f"match_inliers (the mutual check, identity transforms, tau1 = 0): {fmt(mi)}")
    stage = statistics.median(nn) + statistics.median(mi)
    say(f"registration / (nn_match + match_inliers) = {100 * med / stage:.2f} %; registration / nn_match = "
        f"{100 * med / statistics.median(nn):.2f} %")
    rre, rte = matching.registration_errors(T, gts)
    say(f"result: {int((best_h >= 0).sum())} of {a.pairs} pairs registered, registration recall (15 deg, 0.3) = "
        f"{matching.registration_recall(T, gts):.3f}, median RRE {np.median(rre):.4f} deg, median RTE {np.median(rte):.5f}, "
        f"mean inliers {n_inlier.mean():.0f}, least refit margin {margin[best_h >= 0].min() if (best_h >= 0).any() else 0:.3f}")

    ms, off, kp_host = match_src.cpu().numpy(), tgt_off.numpy(), np.concatenate(kps)
    jobs = []
    for p in range(min(a.pairs, a.host_pairs * a.host_threads)):
        s, t = pairs[p]
        x, y, _ = R.correspondences(kp_host[frag_off[s]:frag_off[s + 1]], kp_host[frag_off[t]:frag_off[t + 1]], ms[off[p]:off[p + 1]])
        jobs.append((x, y, p, a.hyp))
    t0 = time.perf_counter()
    with multiprocessing.get_context("spawn").Pool(a.host_threads) as pool:
        ref = pool.map(_host_pair, jobs)
    host = (time.perf_counter() - t0) * a.pairs / len(jobs)
    same = sum(int(best_h[p] == r[0] and n_inlier[p] == r[1]) for p, r in enumerate(ref))
    say(f"numpy restatement (tests/ransac_ref.py, {a.host_threads} processes, {len(jobs)} pairs scaled to {a.pairs}, pool start-up "
        f"included): {host:.1f} s = {1e3 * host / med:.0f}x the registration call; best_h and n_inlier equal on {same} of {len(jobs)}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
