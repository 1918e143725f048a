"""ModelNet training batches (vgtk.pc.modelnet_batch, csrc/modelnet_batch.hip) next to the host loader they replace and to the
training step they feed.

Workload: B = 32 raw clouds of 2048 points and of 10 000 points (uniform in a box, off-centre), n_sample = 1024, A = 60 anchors
-- a ModelNet40 classification batch.  Timed:
  * the device call (one launch), HIP events, median of --runs after warm-up, for both cloud sizes;
  * a numpy restatement of the reference's per-sample loader (SPConvNets/datasets/modelnet40.py:50-80: np.random.choice,
    centre and scale, a random rotation, the anchor arg max) over the same batch on --procs worker processes (what its
    DataLoader does), wall clock, median of --host-runs batches, plus the host-to-device copy of the [B, n_sample, 3] batch it
    produces.  The workers are started before the device is touched and never open it.
Reported: both, and the device call's share of the training step (--step-ms, default 59.93: the headline ModelNet40
configuration).  No ratio is claimed beforehand; the file records what was measured, on which commit, and how many repetitions.

    python tools/modelnet_batch_bench.py [--runs 50] [--host-runs 10] [--procs 16] [--commit ID] [--out profiles/modelnet_batch.txt]
"""
import argparse
import multiprocessing
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, N_SAMPLE = 32, 1024


def raw_clouds(n, seed):
    rng = np.random.default_rng(seed)
    return [(rng.uniform(-1.0, 1.0, (n, 3)) * rng.uniform(0.5, 2.0) + rng.uniform(-3.0, 3.0, 3)).astype(np.float32) for _ in range(B)]


def host_sample(args):
    """One __getitem__ of the reference's loader, restated in numpy (its scipy rotation replaced by Shoemake's, three uniforms)."""
    pc, anchors, seed = args
    rng = np.random.default_rng(seed)
    pc = pc[rng.choice(pc.shape[0], N_SAMPLE, replace=pc.shape[0] < N_SAMPLE)].astype(np.float64)
    pc = pc - pc.mean(axis=0, keepdims=True)
    pc = pc / np.sqrt((pc ** 2).sum(axis=1)).max()
    u0, u1, u2 = rng.random(3)
    x, y = np.sqrt(1 - u0) * np.sin(2 * np.pi * u1), np.sqrt(1 - u0) * np.cos(2 * np.pi * u1)
    z, w = np.sqrt(u0) * np.sin(2 * np.pi * u2), np.sqrt(u0) * np.cos(2 * np.pi * u2)
    R = np.array([[1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * z * w, 2 * x * z + 2 * y * w],
                  [2 * x * y + 2 * z * w, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * x * w],
                  [2 * x * z - 2 * y * w, 2 * y * z + 2 * x * w, 1 - 2 * x * x - 2 * y * y]])
    pc = (R @ pc.T).T
    diff_r = np.matmul(np.transpose(anchors, (0, 2, 1)), R)
    label = int(np.argmax(np.einsum('bii->b', diff_r)))
    return pc.astype(np.float32), R.astype(np.float32), label


def host_batches_ms(pool, clouds, anchors, runs):
    times = []
    for r in range(runs + 1):                                   # the first batch warms the workers up
        t0 = time.perf_counter()
        out = pool.map(host_sample, [(c, anchors, 1000 * r + i) for i, c in enumerate(clouds)])
        batch = np.stack([o[0] for o in out])
        times.append((time.perf_counter() - t0) * 1e3)
    return times[1:], batch


def event_ms(fn, runs, warmup):
    import torch
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


def commit_id():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--host-runs", type=int, default=10)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--step-ms", type=float, default=59.93)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "modelnet_batch.txt"))
    a = ap.parse_args()
    anchors = np.load(os.path.join(ROOT, "epn_pointcloud_amd", "vgtk", "data", "so3_anchors60.npy")).astype(np.float32)
    sets = {n: raw_clouds(n, n) for n in (2048, 10000)}

    host = {}
    with multiprocessing.get_context("spawn").Pool(a.procs) as pool:            # before the device is touched
        for n, clouds in sets.items():
            host[n] = host_batches_ms(pool, clouds, anchors.astype(np.float64), a.host_runs)

    import torch
    from epn_pointcloud_amd import _lib, data
    _lib.get_lib()
    dev = torch.device("cuda:0")
    an = torch.from_numpy(anchors).to(dev)
    ids = torch.arange(B, device=dev, dtype=torch.int64)
    lines = [f"modelnet_batch_bench: commit {a.commit or commit_id()}, device {torch.cuda.get_device_name(0)}",
             f"B = {B}, n_sample = {N_SAMPLE}, A = {an.shape[0]}; device call: median of {a.runs} runs after 5 warm-up (HIP events); "
             f"host loader: median of {a.host_runs} batches after 1 warm-up on {a.procs} processes (wall clock); "
             f"step = {a.step_ms} ms"]
    for n, clouds in sets.items():
        points, offsets = data.pack_clouds(clouds, dev)
        t = event_ms(lambda: data.modelnet_batch(points, offsets, N_SAMPLE, seed=1, ids=ids, anchors=an), a.runs, 5)
        out = data.modelnet_batch(points, offsets, N_SAMPLE, seed=1, ids=ids, anchors=an)
        assert int(out.status.abs().sum()) == 0
        pack = event_ms(lambda: data.pack_clouds(clouds, dev), a.runs, 3)
        call = statistics.median(t)
        times, batch = host[n]
        pinned = torch.from_numpy(batch).pin_memory()
        h2d = statistics.median(event_ms(lambda: pinned.to(dev, non_blocking=True), a.runs, 3))
        hostm = statistics.median(times)
        lines += [f"raw clouds of {n} points:",
                  f"  device call            median {call:.4f} ms (min {min(t):.4f}, max {max(t):.4f}) = {100.0 * call / a.step_ms:.3f} % "
                  f"of the step",
                  f"  pack_clouds (host concatenation + one copy of the RAW clouds, {points.numel() * 4 / 1e6:.2f} MB): median "
                  f"{statistics.median(pack):.4f} ms",
                  f"  host loader            median {hostm:.2f} ms per batch (min {min(times):.2f}, max {max(times):.2f}) + "
                  f"host-to-device copy of its batch {h2d:.4f} ms",
                  f"  host loader + copy / device call = {(hostm + h2d) / call:.0f}x"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
