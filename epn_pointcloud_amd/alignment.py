"""Rotation estimation on the GPU after RegSO3ConvModel's head: the step after `forward()` (confidence, y), the counterpart of
matching.py for the rotation network.

In-memory counterpart of the alignment branch of the reference's MultiTaskDetectionLoss.forward without the loss terms
(vgtk/vgtk/loss.py:140-172, :210-218): per source anchor the most confident target anchor, the regressed relative rotation of
that anchor pair mapped to a matrix and carried back through the two anchors, the confidence-weighted chordal mean of the A
candidates, the number of anchors classified like the label and the angular error against the ground truth -- the number
SPConvNets/trainer_modelnetRotation.py:166 logs as its median.  Specification: include/epn_so3conv.h
(epn_rotation_decode_f32) and DESIGN.md 3.1b; kernel: csrc/rotation_decode.hip, one launch per call.

All tensors are device tensors; nothing here synchronises except evaluate_alignment's final copy of the per-pair results.
"""
import collections

import numpy as np
import torch

from . import _lib
from .vgtk.functional import rotation as _rot

RotationDecode = collections.namedtuple("RotationDecode", "pred_R preds conf margin pred_Rs hits err")
RotationDecode.__doc__ = """decode_rotation's result: pred_R f32 [b,3,3] (the estimate), preds int32 [b,A] (the chosen target anchor
of every source anchor), conf f32 [b,A] (its normalised confidence), margin f32 [b] (conditioning of the mean: so3_mean),
pred_Rs f32 [b,A,3,3] (the A candidates), hits int32 [b] (anchors with preds == label; None without label) and err f32 [b]
(angular error in radians against gt; None without gt)."""

AlignmentResult = collections.namedtuple("AlignmentResult", "errors accuracy median_deg pred_R margin")
AlignmentResult.__doc__ = """evaluate_alignment's result: errors float32 numpy [k] (radians), accuracy (share of the k * A source
anchors whose chosen target anchor is the label), median_deg (median error in degrees; nan for k = 0), pred_R f32 [k,3,3] and
margin f32 [k] (device tensors)."""


def _check_head(confidence, y, anchors, label, gt):
    """Everything decode_rotation refuses, decided on the host from shapes and dtypes alone."""
    for name, t in (("confidence", confidence), ("y", y)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch tensor, got {type(t).__name__}")
        if not t.is_floating_point():
            raise TypeError(f"{name} must be a floating-point tensor, got {t.dtype}")
        if not t.is_cuda:
            raise RuntimeError(f"{name} must be a CUDA tensor")
    anchors = _rot.check_anchors(anchors)
    A = anchors.shape[0]
    if confidence.dim() != 3 or tuple(confidence.shape[1:]) != (A, A):
        raise ValueError(f"confidence must be [b, {A}, {A}] (target anchor, source anchor), got {tuple(confidence.shape)}")
    b = confidence.shape[0]
    if y.dim() != 4 or y.shape[0] != b or y.shape[1] not in (4, 6) or tuple(y.shape[2:]) != (A, A):
        raise ValueError(f"y must be [{b}, 4 | 6, {A}, {A}], got {tuple(y.shape)}")
    if label is not None:
        if not isinstance(label, torch.Tensor) or tuple(label.shape) != (b, A) or label.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"label must be an int32 / int64 tensor of shape {(b, A)}")
        # a host label (a loader's) is range-checked here and uploaded by the caller below; a device label is only ever
        # compared with preds, never used as an index, so a value outside 0..A-1 there is a miss and nothing else
        if not label.is_cuda and label.numel() and not (0 <= int(label.min()) and int(label.max()) < A):
            raise ValueError(f"label must lie in 0..{A - 1}")
    if gt is not None:
        gt = _rot._mat33(gt, "gt", 1)
        if gt.shape[0] != b:
            raise ValueError(f"gt must be [{b}, 3, 3], got {tuple(gt.shape)}")
    return anchors, gt


def decode_rotation(confidence, y, anchors, label=None, gt=None):
    """(confidence [b,A,A], y [b,4|6,A,A]: RegSO3ConvModel.forward's outputs; anchors f32 [A,3,3], A <= 64; label int [b,A] and
    gt f32 [b,3,3]: optional, label_relative_rotation's labels (a device tensor, or a host tensor with values in 0..A-1) and
    the ground-truth rotation) -> RotationDecode.  Label range: a HOST label is checked against 0..A-1 here and uploaded; a DEVICE
    label is NOT range-checked (that would cost a synchronisation) -- the kernel only compares it with preds and never indexes
    with it, so a value outside 0..A-1 is a miss in `hits` and nothing else.  One launch;
    floating-point inputs of another dtype or memory format are converted to contiguous fp32 first (the head hands out
    channels-last y)."""
    anchors, gt = _check_head(confidence, y, anchors, label, gt)
    b, A, nr = confidence.shape[0], anchors.shape[0], y.shape[1]
    wts, y = confidence.detach().float().contiguous(), y.detach().float().contiguous()
    if label is not None:
        label = label.to(device=wts.device, dtype=torch.int32).contiguous()
    _lib.same_device(wts, y, anchors, label, gt)
    dev = wts.device
    f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
    out = RotationDecode(torch.empty((b, 3, 3), **f32), torch.empty((b, A), **i32), torch.empty((b, A), **f32),
                         torch.empty((b,), **f32), torch.empty((b, A, 3, 3), **f32),
                         None if label is None else torch.empty((b,), **i32), None if gt is None else torch.empty((b,), **f32))
    if b > 0:
        p = _lib.dev_ptr
        _lib.check(_lib.get_lib().epn_rotation_decode_f32(
            p(wts, "confidence"), p(y, "y"), p(anchors, "anchors"), p(label, "label", torch.int32), p(gt, "gt"), b, A, nr,
            p(out.pred_R, "pred_R"), p(out.preds, "preds", torch.int32), p(out.conf, "conf"), p(out.margin, "margin"),
            p(out.pred_Rs, "pred_Rs"), p(out.hits, "hits", torch.int32), p(out.err, "err"), _lib.stream_of(wts)),
            "rotation_decode")
    return out


def check_pairs(src, tgt, batch):
    """What estimate_rotation and evaluate_alignment refuse about their clouds, on the host: src, tgt float [k,n,3] of one
    shape on one device, batch >= 1.  -> int(batch)."""
    for name, t in (("src", src), ("tgt", tgt)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch tensor, got {type(t).__name__}")
        if t.dim() != 3 or t.shape[2] != 3:
            raise ValueError(f"{name} must be [k, n, 3], got {tuple(t.shape)}")
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be torch.float32, got {t.dtype}")
    if src.shape != tgt.shape:
        raise ValueError(f"src {tuple(src.shape)} and tgt {tuple(tgt.shape)} differ in shape")
    if src.device != tgt.device:
        raise RuntimeError(f"src is on {src.device}, tgt on {tgt.device}")
    if int(batch) != batch or int(batch) < 1:
        raise ValueError(f"batch must be an integer >= 1, got {batch}")
    return int(batch)


def batched_decode(model, src, tgt, batch, label=None, gt=None):
    """forward() over the pairs in batches of `batch` (the last one padded with zero clouds whose rows are dropped), each
    decoded with the model's anchors -> RotationDecode over all k pairs (k >= 1).  The caller holds torch.no_grad()."""
    anchors = model.get_anchor().detach().float().contiguous()
    k = src.shape[0]
    parts = []
    for r0 in range(0, k, batch):
        x = torch.stack((src[r0:r0 + batch], tgt[r0:r0 + batch]), dim=1)
        rows = x.shape[0]
        if rows < batch:
            x = torch.cat((x, x.new_zeros(batch - rows, *x.shape[1:])))
        confidence, y = model.forward(x)
        parts.append(decode_rotation(confidence[:rows], y[:rows], anchors, None if label is None else label[r0:r0 + rows],
                                     None if gt is None else gt[r0:r0 + rows]))
    return RotationDecode(*(None if f[0] is None else torch.cat(f) for f in zip(*parts)))


def evaluate_alignment(model, src, tgt, T, batch=32):
    """(model: a RegSO3ConvModel in eval() mode; src, tgt f32 [k,n,3]: the pairs, src = T applied to the shape of tgt as in
    the reference's loader (SPConvNets/datasets/modelnet40.py:129-155); T f32 [k,3,3]: the ground-truth rotations) ->
    AlignmentResult: per-pair angular errors in radians, the anchor-classification accuracy against
    label_relative_rotation(anchors, T) and the median error in degrees (trainer_modelnetRotation.py:166)."""
    if model.training:
        raise RuntimeError("evaluate_alignment() needs the model in eval() mode: call model.eval() first")
    batch = check_pairs(src, tgt, batch)
    k = src.shape[0]
    if not isinstance(T, torch.Tensor) or tuple(T.shape) != (k, 3, 3) or T.dtype != torch.float32:
        raise ValueError(f"T must be a float32 tensor of shape {(k, 3, 3)}")
    if T.device != src.device:
        raise RuntimeError(f"T is on {T.device}, the clouds on {src.device}")
    anchors = model.get_anchor()
    if not 1 <= anchors.shape[0] <= _rot.MAX_ANCHORS:
        raise ValueError(f"the rotation kernels take 1..{_rot.MAX_ANCHORS} anchors, the model has {anchors.shape[0]}")
    if k == 0:
        return AlignmentResult(np.zeros(0, np.float32), float("nan"), float("nan"), src.new_zeros((0, 3, 3)), src.new_zeros((0,)))
    with torch.no_grad():
        T = T.contiguous()
        _, label = _rot.label_relative_rotation(anchors.detach().float().contiguous(), T)
        d = batched_decode(model, src, tgt, batch, label, T)
    errors = d.err.cpu().numpy()
    accuracy = float(d.hits.sum().item()) / (k * anchors.shape[0])
    return AlignmentResult(errors, accuracy, float(np.median(errors) * 180.0 / np.pi), d.pred_R, d.margin)
