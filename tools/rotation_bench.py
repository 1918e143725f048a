"""Rotation decode (epn_pointcloud_amd.alignment.decode_rotation, csrc/rotation_decode.hip) next to what it replaces and to
the network in front of it.

Workload: b = 64 pairs, A = 60 anchors, quaternion head (nr = 4): a seeded head-like output (confidence a softmax over the
target anchors peaked near the label, y near the label's relative rotation plus noise), labels and ground truth given, so the
call also counts hits and computes the angular error.  Timed with HIP events, median of --runs after warm-up:
  decode      the call as estimate_rotation() makes it (output allocations + one launch), and the launch alone on preallocated
              buffers
  torch form  the same decode written in torch operations on the device, the reference's formulation (vgtk/vgtk/loss.py:140-172,
              :210-218: max over the target anchors, index_select, the quaternion map, the three-matrix einsum, so3_mean with
              torch.linalg.svd and torch.det, acos_safe).  If torch.linalg.svd cannot run on the machine that is recorded and
              only the other two are priced.
  forward     build_reg()'s forward (eval mode, no_grad, fp32 input, 1024 points per cloud) on the same number of pairs: what
              the decode follows in estimate_rotation()
One process, no retries; run it under a time limit:

    timeout -k 10 600 python tools/rotation_bench.py [--runs 20] [--out profiles/rotation_decode.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, A, NR, N_POINTS = 64, 60, 4, 1024


def event_ms(fn, runs, warmup=3):
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


def head_like(anchors, dev, seed=2913):
    """-> (wts [B,A,A], y [B,4,A,A], label int32 [B,A], T [B,3,3]) on the device, labels from the library itself."""
    import epn_pointcloud_amd.vgtk.functional as F
    g = torch.Generator().manual_seed(seed)
    q, r = torch.linalg.qr(torch.randn(B, 3, 3, generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r, dim1=1, dim2=2))[:, None, :]
    q[:, :, 0] *= torch.sign(torch.linalg.det(q))[:, None]
    T = q.float().to(dev).contiguous()
    R_target, label = F.label_relative_rotation(anchors, T)
    logits = torch.randn(B, A, A, generator=g).to(dev)
    logits.scatter_add_(1, label.long()[:, None, :], torch.full((B, 1, A), 3.0, device=dev))
    wts = torch.softmax(3.0 * logits, dim=1).contiguous()
    # quaternion of R_target[b, a] (the larger of the w- and x-pivot forms is enough for a benchmark input), on every target row
    Rt = R_target.double()
    w = 0.5 * torch.sqrt(torch.clamp(1 + Rt[..., 0, 0] + Rt[..., 1, 1] + Rt[..., 2, 2], min=1e-12))
    quat = torch.stack((w, (Rt[..., 2, 1] - Rt[..., 1, 2]) / (4 * w), (Rt[..., 0, 2] - Rt[..., 2, 0]) / (4 * w),
                        (Rt[..., 1, 0] - Rt[..., 0, 1]) / (4 * w)), dim=1)                     # [B, 4, A]
    y = (quat[:, :, None, :].float() + 0.2 * torch.randn(B, NR, A, A, generator=g).to(dev)).contiguous()
    return wts, y, label, T


def torch_decode(wts, y, anchors, label, T):
    """The reference's formulation in torch operations (no library call)."""
    b, na = wts.shape[0], wts.shape[1]
    confidence, preds = wts.max(1)
    y_rs = y.transpose(1, 3).contiguous().view(b * na, na, -1)
    sel = preds.reshape(-1)[:, None, None].expand(-1, 1, y_rs.shape[2])
    quat = torch.gather(y_rs, 1, sel).view(b * na, -1)
    quat = quat / torch.clamp(torch.sqrt(quat.pow(2).sum(1, keepdim=True)), min=1e-8)
    qw, qx, qy, qz = quat[:, 0:1], quat[:, 1:2], quat[:, 2:3], quat[:, 3:4]
    xx, yy, zz, xy, xz, yz, xw, yw, zw = qx * qx, qy * qy, qz * qz, qx * qy, qx * qz, qy * qz, qx * qw, qy * qw, qz * qw
    rows = torch.cat((1 - 2 * yy - 2 * zz, 2 * xy - 2 * zw, 2 * xz + 2 * yw, 2 * xy + 2 * zw, 1 - 2 * xx - 2 * zz, 2 * yz - 2 * xw,
                      2 * xz - 2 * yw, 2 * yz + 2 * xw, 1 - 2 * xx - 2 * yy), 1)
    pred_RAnchor = rows.view(b, na, 3, 3)
    confidence = confidence / (1e-6 + confidence.sum(1, keepdim=True))
    pred_Rs = torch.einsum('baij,bajk,balk->bail', anchors[None].expand(b, -1, -1, -1), pred_RAnchor, anchors[preds])
    Ce = torch.sum(confidence[:, :, None, None] * pred_Rs, dim=1)
    cu, _, cvT = torch.linalg.svd(Ce)
    dets = torch.det(torch.matmul(cu, cvT))
    Dm = torch.diag_embed(torch.stack((torch.ones_like(dets), torch.ones_like(dets), dets), dim=1))
    pred_R = cu @ Dm @ cvT
    hits = (preds == label).sum(1)
    x = 0.5 * (torch.einsum('bij,bij->b', pred_R, T) - 1)
    eps = 1e-4
    slope = float(np.arccos(1 - eps) / eps)
    sign = torch.sign(x)
    err = torch.where(x.abs() <= 1 - eps, torch.acos(x.clamp(-1, 1)),
                      torch.acos(sign * (1 - eps)) - slope * sign * (x.abs() - 1 + eps))
    return pred_R, preds, confidence, hits, err


def launch_only(lib, _lib, wts, y, anchors, label, T):
    dev = wts.device
    f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
    out = [torch.empty(B * 9, **f32), torch.empty(B * A, **i32), torch.empty(B * A, **f32), torch.empty(B, **f32),
           torch.empty(B * A * 9, **f32), torch.empty(B, **i32), torch.empty(B, **f32)]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())

    def call():
        _lib.check(lib.epn_rotation_decode_f32(ptr(wts), ptr(y), ptr(anchors), ptr(label), ptr(T), B, A, NR, *(ptr(o) for o in out),
                                               _lib.stream_of(wts)), "rotation_decode")
    return call


def line(name, times):
    return f"{name}: median {statistics.median(times):.4f} ms (min {min(times):.4f}, max {max(times):.4f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from epn_pointcloud_amd import _lib, alignment, models
    lib = _lib.get_lib()
    dev = torch.device("cuda:0")
    model = models.build_reg(input_num=N_POINTS).to(dev).eval()
    anchors = model.get_anchor().detach().float().contiguous()
    wts, y, label, T = head_like(anchors, dev)
    lines = [f"rotation_bench: b = {B} pairs, A = {A}, nr = {NR}, median of {a.runs} runs after 3 warm-up runs, HIP events, device = "
             f"{torch.cuda.get_device_name(0)}"]

    got = alignment.decode_rotation(wts, y, anchors, label, T)
    whole = event_ms(lambda: alignment.decode_rotation(wts, y, anchors, label, T), a.runs)
    alone = event_ms(launch_only(lib, _lib, wts, y, anchors, label, T), a.runs)
    lines.append(line("decode_rotation (allocations + one launch)", whole))
    lines.append(line("epn_rotation_decode_f32 alone (preallocated outputs)", alone))

    try:
        ref = torch_decode(wts, y, anchors, label, T)
        torch.cuda.synchronize()
        form = event_ms(lambda: torch_decode(wts, y, anchors, label, T), a.runs)
        lines.append(line("torch formulation with torch.linalg.svd", form) +
                     f" = {statistics.median(form) / statistics.median(whole):.1f} x decode_rotation")
        lines.append(f"agreement with the torch formulation: preds equal {bool(torch.equal(ref[1].int(), got.preds))}, max |pred_R "
                     f"difference| {(ref[0] - got.pred_R).abs().max().item():.2e}, max |err difference| "
                     f"{(ref[4] - got.err).abs().max().item():.2e}, hits equal {bool(torch.equal(ref[3].int(), got.hits))}")
    except (NotImplementedError, RuntimeError) as e:                   # recorded, not retried
        # only "torch.linalg.svd has no backend here" is a result; anything else (a HIP runtime error above all) ends the run
        text = str(e).lower()
        missing = isinstance(e, (NotImplementedError, torch.linalg.LinAlgError)) or any(
            w in text for w in ("not implemented", "not compiled", "no backend", "hipsolver", "rocsolver", "magma", "lapack"))
        if not missing:
            raise
        lines.append(f"torch formulation: torch.linalg.svd cannot run on this machine ({type(e).__name__}: "
                     f"{str(e).splitlines()[0][:160]}); not priced")

    rng = np.random.default_rng(2913)
    g = rng.standard_normal((B, 2, N_POINTS, 3))
    pts = g / np.linalg.norm(g, axis=3, keepdims=True) * rng.random((B, 2, N_POINTS, 1)) ** (1 / 3)
    x = torch.from_numpy(pts.astype(np.float32)).to(dev)
    with torch.no_grad():
        fwd = event_ms(lambda: model(x), a.runs)
    lines.append(line(f"build_reg forward, {B} pairs of {N_POINTS} points (eval, no_grad, fp32)", fwd) +
                 f"; decode_rotation = {100 * statistics.median(whole) / statistics.median(fwd):.2f} % of it")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
