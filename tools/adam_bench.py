"""One optimiser step of optim.FlatAdam (csrc/adam_step.hip) next to torch.optim.Adam in its three forms, at the parameter shapes of
the full-width cls, reg and inv networks.

No forward pass: the parameters get their shapes from the public builders (built on the host), values and gradients are seeded
Gaussians.  Four optimisers over four copies of the parameters in one process:
  FlatAdam             two launches, rate / step count / skip on the device, clipping and 1/world folded in
  torch default        torch.optim.Adam(params)            (the multi-tensor form on a device)
  torch fused          torch.optim.Adam(params, fused=True)
  torch capturable     torch.optim.Adam(params, capturable=True)
Timed with HIP events around one step(), eager mode, the four forms ALTERNATED step by step (so that clock and cache state drift
over all of them alike), median of --runs steps after --warmup.  Launches per step come from a torch.profiler run of its own, after
the timed runs (device kernels and memsets of one step).  Bandwidth: FlatAdam moves 32 bytes per element (grad twice, exp_avg,
exp_avg_sq and the parameter read and written); the torch forms are charged the 28 bytes of one pass, whatever they really move.
The yardstick is the 6.29 TB/s of a float4 copy on this part.  One process, no retries:

    timeout -k 10 600 python tools/adam_bench.py [--runs 50] [--out profiles/adam_step.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_RATE = 6.29e12


def shapes_of(name):
    from epn_pointcloud_amd import models
    return [tuple(p.shape) for p in getattr(models, "build_" + name)().parameters() if p.requires_grad]


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
    except Exception as e:                                  # a count is a diagnostic; the times do not depend on it
        return None, f"{type(e).__name__}: {e}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None, help="appended to, one block per network")
    a = ap.parse_args()
    from epn_pointcloud_amd import _lib, optim
    _lib.get_lib()
    assert torch.cuda.is_available(), "adam_bench needs a GPU"
    dev = torch.device("cuda:0")
    blocks = []
    for net in ("cls", "reg", "inv"):
        shapes = shapes_of(net)
        gen = torch.Generator(device="cpu").manual_seed(len(shapes))
        start = [torch.randn(*s, generator=gen) for s in shapes]
        grads = [0.01 * torch.randn(*s, generator=gen) for s in shapes]
        n = sum(t.numel() for t in start)

        def copies():
            return [torch.nn.Parameter(t.to(dev)) for t in start]

        forms = {}
        ps = copies()
        flat = optim.FlatAdam(ps, lr=1e-3)
        for v, g in zip(flat.grad_buckets.views, grads):
            v.copy_(g)
        forms["FlatAdam"] = (flat.step, 32)
        for label, kw in (("torch default", {}), ("torch fused", dict(fused=True)), ("torch capturable", dict(capturable=True))):
            qs = copies()
            for q, g in zip(qs, grads):
                q.grad = g.to(dev)
            forms[label] = (torch.optim.Adam(qs, lr=1e-3, **kw).step, 28)
        times = {k: [] for k in forms}
        for it in range(a.warmup + a.runs):
            for k, (fn, _) in forms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if it >= a.warmup:
                    times[k].append(e0.elapsed_time(e1))
        lines = [f"adam_bench: {net} network, {len(shapes)} parameter tensors, {n} elements, one optimiser step, eager, the four forms "
                 f"alternated, median of {a.runs} steps after {a.warmup} warm-up steps, HIP events, device = {torch.cuda.get_device_name(0)}"]
        med = {k: statistics.median(v) for k, v in times.items()}
        for k, (fn, nbytes) in forms.items():
            rate = nbytes * n / (med[k] * 1e-3)
            cnt, why = launches(fn)
            lines.append(f"{k:17s}: median {med[k]:.4f} ms (min {min(times[k]):.4f}, max {max(times[k]):.4f}); {nbytes} B/element -> "
                         f"{rate / 1e12:.3f} TB/s = {100 * rate / COPY_RATE:.1f} % of the 6.29 TB/s copy rate; device launches per step: "
                         + (str(cnt) if cnt is not None else f"not measured ({why})"))
        best = min((k for k in forms if k != "FlatAdam"), key=lambda k: med[k])
        r = med[best] / med["FlatAdam"]
        lines.append(f"fastest torch form ({best}) / FlatAdam = {r:.2f} x" + ("" if r >= 1 else "  (FlatAdam is SLOWER here)"))
        lines.append(f"FlatAdam after the runs: counters {flat.counters.tolist()}, info {[round(x, 6) for x in flat.last_info().tolist()]}")
        blocks.append("\n".join(lines))
        del forms, flat, ps
        torch.cuda.empty_cache()
    text = "\n\n".join(blocks)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n\n")


if __name__ == "__main__":
    main()
