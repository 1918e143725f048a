"""The classification network's training loss (epn_pointcloud_amd.losses.classification_loss, csrc/cls_loss.hip) next to what it
replaces.

Workload: forward + backward of the loss at the classification trainer's shape, k = 40 classes, A = 60 anchors, B = 32 (the
trainer's batch) and B = 256, blend weights (1, 0.5), on seeded Gaussian logits with labels in range.
Timed with HIP events around one forward + backward, median of --runs after warm-up, eager mode, the two forms alternated in two
windows each (the spread between the windows is printed):
  fused       classification_loss(...).loss.backward(): allocations + two launches forward, one backward
  torch form  the operations of the reference's formulation in torch on the same device (vgtk/vgtk/loss.py:18-75: two
              cross_entropy calls, two max / compare / sum chains, the scalar blend) and autograd's backward through them
Launch counts of both forms come from torch.profiler over one un-timed forward + backward each (device kernels and memsets).
One process, no retries:

    timeout -k 10 300 python tools/cls_loss_bench.py [--runs 50] [--out profiles/cls_loss.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K, A, COEF = 40, 60, (1.0, 0.5)


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


def torch_form(pred, label, wts, rlabel, coef):
    """CrossEntropyLoss twice and the blend, written in torch on their own (no library call)."""
    def metric(x, y):
        hit = (x.max(1)[1].reshape(-1) == y.reshape(-1)).sum().float() / float(y.numel())
        return torch.nn.functional.cross_entropy(x, y), hit
    cls_loss, acc = metric(pred, label)
    r_loss, racc = metric(wts, rlabel)
    return coef[0] * cls_loss + coef[1] * r_loss, cls_loss, r_loss, acc, racc


def launches(fn):
    """Device kernels and memsets of one call of fn, from torch.profiler; None with the reason if the profiler cannot say."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return (n, None) if n > 0 else (None, "the profiler recorded no device activity")
    except Exception as e:                                  # a count is a diagnostic; the times below do not depend on it
        return None, f"{type(e).__name__}: {e}"


def line(name, times):
    return f"{name}: median {statistics.median(times):.4f} ms (min {min(times):.4f}, max {max(times):.4f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--out", default=None, help="appended to, one block per batch size")
    a = ap.parse_args()
    from epn_pointcloud_amd import _lib, losses
    _lib.get_lib()
    assert torch.cuda.is_available(), "cls_loss_bench needs a GPU"
    dev = torch.device("cuda:0")
    blocks = []
    for B in (32, 256):
        rng = np.random.default_rng(2913 + B)
        pred = torch.from_numpy((2 * rng.standard_normal((B, K))).astype(np.float32)).to(dev).requires_grad_()
        wts = torch.from_numpy((2 * rng.standard_normal((B, A))).astype(np.float32)).to(dev).requires_grad_()
        label = torch.from_numpy(rng.integers(0, K, B)).to(dev)
        rlabel = torch.from_numpy(rng.integers(0, A, B)).to(dev)
        label32, rlabel32 = label.int(), rlabel.int()
        coef = torch.tensor(COEF, dtype=torch.float32, device=dev)
        lines = [f"cls_loss_bench: B = {B}, k = {K}, A = {A}, coef = {COEF}, forward + backward, eager, median of {a.runs} runs after 5 "
                 f"warm-up runs, HIP events, device = {torch.cuda.get_device_name(0)}"]

        def fused():
            pred.grad = wts.grad = None
            losses.classification_loss(pred, label32, wts, rlabel32, coef).loss.backward()

        def form():
            pred.grad = wts.grad = None
            torch_form(pred, label, wts, rlabel, COEF)[0].backward()

        fused()
        got = (losses.classification_loss(pred, label32, wts, rlabel32, coef), pred.grad.clone(), wts.grad.clone())
        form()
        ref = (torch_form(pred, label, wts, rlabel, COEF), pred.grad.clone(), wts.grad.clone())
        torch.cuda.synchronize()
        t_form, t_fused = event_ms(form, a.runs), event_ms(fused, a.runs)      # alternated once more below: the spread
        t_form2, t_fused2 = event_ms(form, a.runs), event_ms(fused, a.runs)
        m_fused, m_form = statistics.median(t_fused + t_fused2), statistics.median(t_form + t_form2)
        lines.append(line("classification_loss forward + backward (fp64 inside)", t_fused))
        lines.append(line("  the same, second window", t_fused2))
        lines.append(line("torch formulation of the reference, forward + backward", t_form))
        lines.append(line("  the same, second window", t_form2))
        r = m_form / m_fused
        lines.append(f"torch formulation / fused = {r:.2f} x" + ("" if r >= 1 else "  (the fused form is SLOWER here)"))
        for name, fn in (("fused", fused), ("torch formulation", form)):
            n, why = launches(fn)
            lines.append(f"device launches of one forward + backward, {name}: " + (str(n) if n is not None else f"not measured ({why})"))
        lines.append(f"agreement: loss {got[0].loss.item():.7f} vs {ref[0][0].item():.7f}, acc {got[0].acc.item():.4f} vs "
                     f"{ref[0][3].item():.4f}, att_acc {got[0].att_acc.item():.4f} vs {ref[0][4].item():.4f}, max |dpred difference| "
                     f"{(got[1] - ref[1]).abs().max().item():.2e}, max |dwts difference| {(got[2] - ref[2]).abs().max().item():.2e}")
        blocks.append("\n".join(lines))
    text = "\n\n".join(blocks)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n\n")


if __name__ == "__main__":
    main()
