"""The rotation network's training loss (epn_pointcloud_amd.losses.rotation_loss, csrc/rotation_loss.hip) next to what it replaces
and to the training step in front of it.

Workload: forward + backward of the loss at the rotation trainer's shape, b = 64 pairs, A = 60 anchors, nr = 4 (quaternion) and
nr = 6 (two columns), w = 10, on seeded inputs: the confidence a softmax over random logits peaked at the label for half of the
pairs, y Gaussian, labels and R_target from label_relative_rotation of random rotations.
Timed with HIP events around one forward + backward, median of --runs after warm-up, eager mode, the two forms alternated in two
windows each (the spread between the windows is printed):
  fused       rotation_loss(...).loss.backward(): allocations + two launches forward, one backward
  torch form  the operations of the reference's formulation in torch on the same device (vgtk/vgtk/loss.py:140-181: cross-entropy
              over dim 1, max, two transposes with a gather, the rotation map with torch.max(norm, 1e-8), the mean of squares)
              and autograd's backward through them
Launch counts of both forms come from torch.profiler over one un-timed forward + backward each (device kernels and memsets).
Share of the step: --bench-json names a file holding bench.py's result line; its configs.reg_bf16.ms_per_step (forward +
backward of the network with feats.square().mean() in place of a loss, b = 64 pairs of 1024 points, bf16, graph replay) is
what both times are divided by.  Without it the share is reported as not measured.
One process, no retries:

    timeout -k 10 300 python tools/rotation_loss_bench.py [--runs 50] [--bench-json FILE] [--out profiles/rotation_loss.txt]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, A, W = 64, 60, 10.0


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


def _normalize(v):
    mag = torch.max(torch.sqrt(v.pow(2).sum(1)), torch.tensor([1e-8], dtype=v.dtype, device=v.device))
    return v / mag[:, None]


def quaternion_map(q):
    q = _normalize(q)
    w, x, y, z = (q[:, i:i + 1] for i in range(4))
    xx, yy, zz, xy, xz, yz, xw, yw, zw = x * x, y * y, z * z, x * y, x * z, y * z, x * w, y * w, z * w
    row0 = torch.cat((1 - 2 * yy - 2 * zz, 2 * xy - 2 * zw, 2 * xz + 2 * yw), 1)
    row1 = torch.cat((2 * xy + 2 * zw, 1 - 2 * xx - 2 * zz, 2 * yz - 2 * xw), 1)
    row2 = torch.cat((2 * xz - 2 * yw, 2 * yz + 2 * xw, 1 - 2 * xx - 2 * yy), 1)
    return torch.stack((row0, row1, row2), 1)


def ortho6d_map(v):
    x = _normalize(v[:, 0:3])
    z = _normalize(torch.cross(x, v[:, 3:6], dim=1))
    y = torch.cross(z, x, dim=1)
    return torch.stack((x, y, z), 2)


def torch_form(wts, label, y, gt_R, w):
    """The loss terms of the reference's alignment branch, written in torch on their own (no library call)."""
    b, nr, na = y.shape[0], y.shape[1], y.shape[2]
    cls_loss = torch.nn.functional.cross_entropy(wts, label)
    preds = wts.max(1)[1]
    r_acc = (preds.reshape(-1) == label.reshape(-1)).sum().float() / float(label.numel())
    y_rs = y.transpose(1, 3).contiguous().view(b * na, na, nr)
    y_select = torch.gather(y_rs, 1, label.view(-1, 1, 1).expand(-1, 1, nr)).view(b * na, nr)
    select_R = (quaternion_map if nr == 4 else ortho6d_map)(y_select).view(b, na, 3, 3)
    l2_loss = torch.pow(gt_R - select_R, 2).mean()
    return cls_loss + w * l2_loss, cls_loss, w * l2_loss, r_acc


def inputs(nr, dev, seed=2913):
    import epn_pointcloud_amd
    import epn_pointcloud_amd.vgtk.functional as F
    epn_pointcloud_amd.install_vgtk_alias()
    import vgtk.so3conv.functional as L
    rng = np.random.default_rng(seed + nr)
    anchors = torch.from_numpy(np.ascontiguousarray(np.asarray(L.get_anchors(A), dtype=np.float32))).to(dev)
    q, r = np.linalg.qr(rng.standard_normal((B, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[:, :, 0] *= np.sign(np.linalg.det(q))[:, None]
    R_target, label = F.label_relative_rotation(anchors, torch.from_numpy(np.ascontiguousarray(q.astype(np.float32))).to(dev))
    logits = torch.from_numpy(rng.standard_normal((B, A, A)).astype(np.float32)).to(dev)
    hot = torch.nn.functional.one_hot(label.long(), A).transpose(1, 2).float()
    logits[::2] += 3.0 * hot[::2]
    wts = torch.softmax(3.0 * logits, dim=1).contiguous().requires_grad_()
    y = torch.from_numpy(rng.standard_normal((B, nr, A, A)).astype(np.float32)).to(dev).requires_grad_()
    return wts, y, label, R_target


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
    ap.add_argument("--bench-json", default=None, help="file with bench.py's result line: configs.reg_bf16.ms_per_step is the step")
    ap.add_argument("--out", default=None, help="appended to, one block per nr")
    a = ap.parse_args()
    from epn_pointcloud_amd import _lib, losses
    _lib.get_lib()
    assert torch.cuda.is_available(), "rotation_loss_bench needs a GPU"
    dev = torch.device("cuda:0")
    step_ms = None
    if a.bench_json:
        for ln in open(a.bench_json):
            ln = ln.strip()
            if not ln.startswith("{"):
                continue
            o = json.loads(ln)
            if "reg_bf16" in o.get("configs", {}):           # a --full run of the default workload
                step_ms = o["configs"]["reg_bf16"]["ms_per_step"]
            elif o.get("dtype") == "bf16" and "ms_per_step" in o:      # bench.py --model reg: the reg_bf16 config itself
                step_ms = o["ms_per_step"]
        if step_ms is None:
            raise SystemExit(f"{a.bench_json} holds no reg_bf16 step time")
    blocks = []
    for nr in (4, 6):
        wts, y, label, R_target = inputs(nr, dev)
        label64 = label.long()
        lines = [f"rotation_loss_bench: b = {B}, A = {A}, nr = {nr}, w = {W}, forward + backward, eager, median of {a.runs} runs after 5 "
                 f"warm-up runs, HIP events, device = {torch.cuda.get_device_name(0)}"]

        def fused():
            wts.grad = y.grad = None
            losses.rotation_loss(wts, y, label, R_target, W).loss.backward()

        def form():
            wts.grad = y.grad = None
            torch_form(wts, label64, y, R_target, W)[0].backward()

        fused()
        got = (losses.rotation_loss(wts, y, label, R_target, W), wts.grad.clone(), y.grad.clone())
        form()
        ref = (torch_form(wts, label64, y, R_target, W), wts.grad.clone(), y.grad.clone())
        torch.cuda.synchronize()
        t_form, t_fused = event_ms(form, a.runs), event_ms(fused, a.runs)      # alternated once more below: the spread
        t_form2, t_fused2 = event_ms(form, a.runs), event_ms(fused, a.runs)
        m_fused, m_form = statistics.median(t_fused + t_fused2), statistics.median(t_form + t_form2)
        lines.append(line("rotation_loss forward + backward (fp64 inside)", t_fused))
        lines.append(line("  the same, second window", t_fused2))
        lines.append(line("torch formulation of the reference, forward + backward", t_form))
        lines.append(line("  the same, second window", t_form2))
        r = m_form / m_fused
        lines.append(f"torch formulation / fused = {r:.2f} x" + ("" if r >= 1 else "  (the fp64 form is SLOWER here)"))
        for name, fn in (("fused", fused), ("torch formulation", form)):
            n, why = launches(fn)
            lines.append(f"device launches of one forward + backward, {name}: " + (str(n) if n is not None else f"not measured ({why})"))
        if step_ms is None:
            lines.append("share of the configs.reg_bf16 step: not measured (no --bench-json)")
        else:
            lines.append(f"configs.reg_bf16 step (bench.py, this run's --bench-json): {step_ms:.3f} ms; the fused loss = "
                         f"{100 * m_fused / step_ms:.3f} % of it, the torch formulation {100 * m_form / step_ms:.3f} %")
        lines.append(f"agreement: loss {got[0].loss.item():.7f} vs {ref[0][0].item():.7f}, r_acc {got[0].r_acc.item():.4f} vs "
                     f"{ref[0][3].item():.4f}, max |dwts difference| {(got[1] - ref[1]).abs().max().item():.2e}, max |dy difference| "
                     f"{(got[2] - ref[2]).abs().max().item():.2e}")
        blocks.append("\n".join(lines))
    text = "\n\n".join(blocks)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n\n")


if __name__ == "__main__":
    main()
