"""3DMatch training batches (vgtk.pc.fragment_pair_batch, csrc/pair_batch.hip) next to the composition that was available before
it: vgtk.cuda.grouping.radius_patches once per fragment side plus torch glue for the draws, the rotation and T.

Workload: the trainer's defaults (SPConvNets/options.py: batch 8, npt 24, input_num 1024) on synthetic fragments -- 16 fragments
of --points points uniform in a --box m cube, 8 pairs, 200 correspondences per pair inside the cube, radius --radius.  Timed, in
one process, the two forms alternating round by round (HIP events around --inner calls, median over --rounds after warm-up):
  * fused         one call of fragment_pair_batch
  * composition   torch.randint for the keypoints and the degrees, the Euler matrices and T in torch fp64, radius_patches per
                  fragment side with center, one batched matmul per side for the rotation
Before timing, the composition is run once on the fused call's own choices and rotations: idx and counts must be equal and the
patches agree to 1e-5 (the composition rotates in fp32).  Device kernels per call are counted with torch's profiler in a run of
their own ("not measured" if the profiler gives none).  No ratio is claimed beforehand; the file records what was measured.

    python tools/pair_batch_bench.py [--rounds 20] [--inner 10] [--commit ID] [--out profiles/pair_batch.txt]
"""
import argparse
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, NPT, N_SAMPLE, P = 8, 24, 1024, 200


def commit_id():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


def euler(deg):
    """torch f64 [n,3] degrees -> [n,3,3]: Rz Ry Rx."""
    import torch
    a = deg * (np.pi / 180.0)
    c, s = torch.cos(a), torch.sin(a)
    one, zero = torch.ones_like(c[:, 0]), torch.zeros_like(c[:, 0])
    Rx = torch.stack((one, zero, zero, zero, c[:, 0], -s[:, 0], zero, s[:, 0], c[:, 0]), 1).view(-1, 3, 3)
    Ry = torch.stack((c[:, 1], zero, s[:, 1], zero, one, zero, -s[:, 1], zero, c[:, 1]), 1).view(-1, 3, 3)
    Rz = torch.stack((c[:, 2], -s[:, 2], zero, s[:, 2], c[:, 2], zero, zero, zero, one), 1).view(-1, 3, 3)
    return Rz @ Ry @ Rx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--points", type=int, default=30000)
    ap.add_argument("--box", type=float, default=2.5)
    ap.add_argument("--radius", type=float, default=0.55)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_batch.txt"))
    a = ap.parse_args()

    import torch
    from epn_pointcloud_amd import _lib, data
    from epn_pointcloud_amd.vgtk.cuda import grouping
    _lib.get_lib()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(8)
    frags = [(rng.random((a.points, 3)) * a.box).astype(np.float32) for _ in range(2 * B)]
    corrs = [(rng.random((P, 1, 3)) * a.box).astype(np.float32).repeat(2, axis=1) for _ in range(B)]
    points, offsets = data.pack_clouds(frags, dev)
    corr, corr_offsets = data.pack_correspondences(corrs, dev)
    pairs = torch.arange(2 * B, device=dev, dtype=torch.int32).view(B, 2)
    poses = torch.eye(4, device=dev, dtype=torch.float64).repeat(2 * B, 1, 1)
    ids = torch.arange(B, device=dev, dtype=torch.int64)
    dfrags = [points[offsets[f]:offsets[f + 1]] for f in range(2 * B)]
    corr_b = corr.view(B, P, 2, 3)

    def fused():
        return data.fragment_pair_batch(points, offsets, pairs, corr, corr_offsets, poses, N_SAMPLE, NPT, a.radius, seed=1, ids=ids,
                                        center=True)

    def composition(choice=None, R=None):
        if choice is None:
            choice = torch.randint(0, P, (B, NPT), device=dev)
            R = euler(torch.randint(0, 30, (2 * B, 3), device=dev).double()).float().view(B, 2, 3, 3)
        kp = torch.gather(corr_b, 1, choice.long().view(B, NPT, 1, 1).expand(B, NPT, 2, 3))        # [B,npt,2,3]
        Rp = poses[:, :3, :3]
        T = (Rp[pairs[:, 0].long()].transpose(1, 2) @ Rp[pairs[:, 1].long()]).float()
        out, idx, counts = [], [], []
        for s in (0, 1):
            rows = []
            for b in range(B):
                i, c, p = grouping.radius_patches(dfrags[2 * b + s], kp[b, :, s].contiguous(), a.radius, N_SAMPLE, seed=1,
                                                  kpt_row0=(b * 2 + s) * NPT, center=True)
                rows.append(p)
                idx.append(i)
                counts.append(c)
            pat = torch.stack(rows)                                                              # [B,npt,n,3]
            out.append((pat.view(B, -1, 3) @ R[:, s].transpose(1, 2)).view(B, NPT, N_SAMPLE, 3))
        T_aug = R[:, 0] @ T @ R[:, 1].transpose(1, 2)
        return out[0], out[1], idx, counts, T, T_aug

    # ---- the two forms compute the same thing
    f = fused()
    assert int(f.status.abs().sum()) == 0
    src, tgt, idx, counts, T, T_aug = composition(f.choice, f.R_aug)
    same_idx = all(torch.equal(idx[s * B + b], f.idx[b, s]) and torch.equal(counts[s * B + b], f.counts[b, s])
                   for s in (0, 1) for b in range(B))
    err = max(float((src - f.src).abs().max()), float((tgt - f.tgt).abs().max()), float((T_aug - f.T_aug).abs().max()))
    assert same_idx and err < 1e-5, (same_idx, err)
    cmin, cmean, cmax = int(f.counts.min()), float(f.counts.float().mean()), int(f.counts.max())

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.inner

    for _ in range(3):
        window(fused)
        window(composition)
    tf, tc = [], []
    for _ in range(a.rounds):                                    # alternating: both see the same neighbours on the machine
        tf.append(window(fused))
        tc.append(window(composition))

    def kernels(fn):
        try:
            from torch.profiler import profile, ProfilerActivity
            fn()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
            return str(n) if n else "not measured"
        except Exception as exc:                                 # a profiler that is not there is no reason to lose the timings
            return f"not measured ({type(exc).__name__})"

    mf, mc = statistics.median(tf), statistics.median(tc)
    lines = [f"pair_batch_bench: commit {a.commit or commit_id()}, device {torch.cuda.get_device_name(0)}",
             f"B = {B}, npt = {NPT}, n_sample = {N_SAMPLE}: {2 * B * NPT} patches per call; {2 * B} fragments of {a.points} points in a "
             f"{a.box} m cube, radius {a.radius}; in-radius counts min {cmin}, mean {cmean:.0f}, max {cmax}",
             f"HIP events around {a.inner} calls, median of {a.rounds} alternating rounds after 3 warm-up rounds; per call:",
             f"  fused (fragment_pair_batch, 1 library launch)                  median {mf:.4f} ms (min {min(tf):.4f}, max {max(tf):.4f})",
             f"  composition (radius_patches x {2 * B} + torch draws / rotation)   median {mc:.4f} ms (min {min(tc):.4f}, max {max(tc):.4f})",
             f"  composition / fused = {mc / mf:.2f}x",
             f"device kernels per call (torch profiler, a run of its own): fused {kernels(fused)}, composition {kernels(composition)}",
             f"same results: idx and counts equal, max |patch, T_aug difference| = {err:.2e} (the composition rotates in fp32)"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
