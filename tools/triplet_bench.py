"""Batch-hard triplet loss (epn_pointcloud_amd.losses.batch_hard_triplet, csrc/triplet_loss.hip) next to what it replaces and to
the network in front of it.

Workload: forward + backward of the loss on seeded unit-norm descriptors, tgt a perturbed src, hard mode, the margin chosen per
shape so that half of the rows have an active hinge (half_active_margin), at
  N = 192, D = 32       the reference trainer's default: 8 x 24 patches, 32-dimensional output
  N = 192, D = 64
  N = 192, D = 60 * 64  the equivariance term's width (after the interpolation)
Timed with HIP events around one forward + backward, median of --runs after warm-up, eager mode:
  fused       batch_hard_triplet(...).loss.backward(): allocations + two launches forward, one backward
  torch form  the operations of the reference's formulation in torch on the same device (vgtk/vgtk/loss.py:220-235, :280-318:
              an expansion-form distance matrix, a boolean-mask index of its off-diagonal entries, which synchronises with
              the host, min, relu, mean, topk) and autograd's backward through them
  network     one forward + backward of build_inv() (train mode, plain fp32) on N patches of 1024 points with
              feats.square().mean() as the loss: what the loss follows in a step.
              Priced at N = 192 only if --network is given; it takes most of the run's time.
One process, no retries; run each shape under its own time limit:

    timeout -k 10 300 python tools/triplet_bench.py --shape 192x32 [--runs 50] [--network] [--out profiles/triplet_loss.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_POINTS = 1024


def event_ms(fn, runs, warmup=5):
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


def descriptors(N, D, dev, seed=2913):
    g = torch.Generator().manual_seed(seed)
    x = torch.nn.functional.normalize(torch.randn(N, D, generator=g, dtype=torch.float64), dim=1)
    noise = torch.nn.functional.normalize(torch.randn(N, D, generator=g, dtype=torch.float64), dim=1)
    y = torch.nn.functional.normalize(x + noise * (0.05 + 1.15 * torch.rand(N, 1, generator=g, dtype=torch.float64)), dim=1)
    return x.float().to(dev).requires_grad_(), y.float().to(dev).requires_grad_()


def torch_form(src, tgt, margin, eps=1e-6):
    """The operations of the reference's formulation, written in torch on their own (no library call): a distance matrix from
    the expansion of the square, a boolean-mask selection of the off-diagonal entries (which synchronises with the host), the
    row minimum, the hinge, the mean, and a top-1 search for the accuracy."""
    n = src.shape[0]
    inner = src @ tgt.T
    d2 = src.square().sum(1)[:, None] + tgt.square().sum(1)[None, :] - (inner + inner)
    dist = d2.clamp_min(eps).sqrt()
    pos = dist.diagonal()
    off_diagonal = ~torch.eye(n, dtype=torch.bool, device=dist.device)
    neg = dist[off_diagonal].view(n, n - 1).amin(dim=1)
    loss = (pos - neg + margin).relu().mean()
    nearest = dist.topk(1, dim=1, largest=False).indices.squeeze(1)
    acc = (nearest == torch.arange(n, device=dist.device)).float().mean()
    return loss, acc, pos.mean(), neg.mean()


def half_active_margin(src, tgt):
    """The margin at which half of the rows have an active hinge: minus the midpoint of the two middle values of d_pos - d_neg
    (from the library's own per-row outputs; the midpoint keeps every row off the hinge's kink), so that the priced backward
    has work at every width."""
    from epn_pointcloud_amd import losses
    with torch.no_grad():
        _, rows = losses.batch_hard_rows(src, tgt, "hard", 0.0)
    x = (rows["d_pos"].double() - rows["d_neg"].double()).sort().values
    return -float(0.5 * (x[x.numel() // 2 - 1] + x[x.numel() // 2]).item())


def line(name, times):
    return f"{name}: median {statistics.median(times):.4f} ms (min {min(times):.4f}, max {max(times):.4f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="192x32", help="NxD")
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--network", action="store_true")
    ap.add_argument("--out", default=None, help="appended to, one block per shape")
    a = ap.parse_args()
    N, D = (int(v) for v in a.shape.lower().split("x"))
    from epn_pointcloud_amd import _lib, losses
    _lib.get_lib()
    dev = torch.device("cuda:0")
    src, tgt = descriptors(N, D, dev)
    MARGIN = half_active_margin(src, tgt)
    lines = [f"triplet_bench: N = {N}, D = {D}, hard, margin {MARGIN:.6f} (half of the rows active), forward + backward, eager, median of {a.runs} runs after 5 "
             f"warm-up runs, HIP events, device = {torch.cuda.get_device_name(0)}"]

    def fused():
        src.grad = tgt.grad = None
        losses.batch_hard_triplet(src, tgt, "hard", MARGIN).loss.backward()

    def form():
        src.grad = tgt.grad = None
        torch_form(src, tgt, MARGIN)[0].backward()

    fused()
    got = (losses.batch_hard_triplet(src, tgt, "hard", MARGIN), src.grad.clone(), tgt.grad.clone())
    form()
    ref = (torch_form(src, tgt, MARGIN), src.grad.clone(), tgt.grad.clone())
    torch.cuda.synchronize()
    t_form, t_fused = event_ms(form, a.runs), event_ms(fused, a.runs)          # alternated once more below: the spread
    t_form2, t_fused2 = event_ms(form, a.runs), event_ms(fused, a.runs)
    lines.append(line("batch_hard_triplet forward + backward (fp64 inside, 3 launches)", t_fused))
    lines.append(line("  the same, second window", t_fused2))
    lines.append(line("torch formulation of the reference, forward + backward", t_form))
    lines.append(line("  the same, second window", t_form2))
    r = statistics.median(t_form + t_form2) / statistics.median(t_fused + t_fused2)
    lines.append(f"torch formulation / fused = {r:.2f} x" + ("" if r >= 1 else "  (the fp64 form is SLOWER here)"))
    lines.append(f"agreement: loss {got[0].loss.item():.7f} vs {ref[0][0].item():.7f}, accuracy {got[0].accuracy.item():.4f} vs "
                 f"{ref[0][1].item():.4f}, max |dsrc difference| {(got[1] - ref[1]).abs().max().item():.2e}, max |dtgt difference| "
                 f"{(got[2] - ref[2]).abs().max().item():.2e}")

    if a.network:
        from epn_pointcloud_amd import models
        model = models.build_inv(input_num=N_POINTS).to(dev).train()
        rng = np.random.default_rng(2913)
        g = rng.standard_normal((N, N_POINTS, 3))
        pts = torch.from_numpy((g / np.linalg.norm(g, axis=2, keepdims=True) * rng.random((N, N_POINTS, 1)) ** (1 / 3)).astype(np.float32)).to(dev)

        def step():
            model.zero_grad(set_to_none=True)
            feats, _ = model(pts)
            feats.square().mean().backward()
        t_net = event_ms(step, max(3, a.runs // 10), warmup=2)
        lines.append(line(f"build_inv forward + backward, {N} patches of {N_POINTS} points (train, fp32, eager)", t_net) +
                     f"; the fused loss = {100 * statistics.median(t_fused + t_fused2) / statistics.median(t_net):.3f} % of it, the torch "
                     f"formulation {100 * statistics.median(t_form + t_form2) / statistics.median(t_net):.3f} %")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n\n")


if __name__ == "__main__":
    main()
