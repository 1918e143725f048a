"""Mirror of the rotation utilities of vgtk/vgtk/functional/rotation.py and vgtk/vgtk/loss.py that the rotation network needs
after its head, on the device: label_relative_rotation (rotation.py:521-526, the reference's _np function per sample on the
host), so3_mean (rotation.py:481-518, torch.svd in the reference) and mean_angular_error (loss.py:212-218).

The first two are one launch each of csrc/rotation_decode.hip through the C ABI (epn_rotation_labels_f32, epn_so3_mean_f32:
include/epn_so3conv.h); the whole decode of a head output is epn_pointcloud_amd.alignment.decode_rotation.
Inputs are device tensors; a host tensor raises like every other wrapper of the library (no CPU fallback)."""
import numpy as np
import torch

from ... import _lib

MAX_ANCHORS = 64            # one wave per pair, one lane per source anchor


# Order of the checks in every wrapper of this file and of alignment.py: type, shape, dtype, device -- all decided on the host
# from the tensors' metadata -- and only then the first call that touches device memory (.contiguous() of a strided tensor,
# an allocation, the launch).  tests/test_rotation_spec.py reaches the shape and dtype refusals without a device through a
# host tensor that claims is_cuda; keep the metadata checks in front of anything that would dereference it.
def _mat33(t, name, lead):
    """t must be float32 [*lead-many dims*, 3, 3] on the device; returns it contiguous."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch tensor, got {type(t).__name__}")
    if t.dim() != lead + 2 or tuple(t.shape[-2:]) != (3, 3):
        raise ValueError(f"{name} must have {lead} leading dimension(s) and end in [3, 3], got {tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be torch.float32, got {t.dtype}")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")
    return t.contiguous()


def check_anchors(anchors):
    """anchors f32 [A,3,3] on the device, 1 <= A <= 64 -> the contiguous tensor."""
    anchors = _mat33(anchors, "anchors", 1)
    if not 1 <= anchors.shape[0] <= MAX_ANCHORS:
        raise ValueError(f"the rotation kernels take 1..{MAX_ANCHORS} anchors, got {anchors.shape[0]}")
    return anchors


def label_relative_rotation(anchors, T):
    """(anchors f32 [A,3,3], T f32 [b,3,3] or [3,3]) -> (R_target f32 [b,A,3,3], label int32 [b,A]) (without the leading b for a
    single T, as the reference's label_relative_rotation_np returns them): for every source anchor a the target anchor i with
    the largest tr(A_a^T T A_i), the lowest i on a tie, and that relative rotation A_a^T T A_label."""
    anchors = check_anchors(anchors)
    single = isinstance(T, torch.Tensor) and T.dim() == 2
    T = _mat33(T[None] if single else T, "T", 1)
    _lib.same_device(anchors, T)
    b, A = T.shape[0], anchors.shape[0]
    R_target = torch.empty((b, A, 3, 3), dtype=torch.float32, device=T.device)
    label = torch.empty((b, A), dtype=torch.int32, device=T.device)
    if b > 0:
        _lib.check(_lib.get_lib().epn_rotation_labels_f32(_lib.dev_ptr(anchors, "anchors"), _lib.dev_ptr(T, "T"), b, A,
                                                          _lib.dev_ptr(R_target, "R_target"),
                                                          _lib.dev_ptr(label, "label", torch.int32), _lib.stream_of(T)),
                   "rotation_labels")
    return (R_target[0], label[0]) if single else (R_target, label)


def so3_mean(Rs, weights=None, return_margin=False):
    """(Rs f32 [b,N,3,3], weights f32 [b,N] or None) -> R f32 [b,3,3]: the chordal L2 mean, the rotation closest to
    sum_n w_n Rs_n.  return_margin=True -> (R, margin f32 [b]); margin = (s2 + det(U V^T) s3) / s1 of that sum's singular values
    says how well the mean is determined (0: not unique, e.g. two opposed rotations; 2: all rotations equal)."""
    Rs = _mat33(Rs, "Rs", 2)
    b, N = Rs.shape[0], Rs.shape[1]
    if N < 1:
        raise ValueError("so3_mean needs at least one rotation per row")
    if weights is not None:
        if not isinstance(weights, torch.Tensor) or tuple(weights.shape) != (b, N):
            raise ValueError(f"weights must be a tensor of shape {(b, N)}")
        if weights.dtype != torch.float32:
            raise TypeError(f"weights must be torch.float32, got {weights.dtype}")
        if not weights.is_cuda:
            raise RuntimeError("weights must be a CUDA tensor")
        weights = weights.contiguous()
        _lib.same_device(Rs, weights)
    R = torch.empty((b, 3, 3), dtype=torch.float32, device=Rs.device)
    margin = torch.empty((b,), dtype=torch.float32, device=Rs.device)
    if b > 0:
        _lib.check(_lib.get_lib().epn_so3_mean_f32(_lib.dev_ptr(Rs, "Rs"), _lib.dev_ptr(weights, "weights"), b, N,
                                                   _lib.dev_ptr(R, "R"), _lib.dev_ptr(margin, "margin"), _lib.stream_of(Rs)),
                   "so3_mean")
    return (R, margin) if return_margin else R


_ACOS_EPS = 1e-4            # acos_safe, vgtk/vgtk/spconv/functional.py:138-143


def mean_angular_error(pred_R, gt_R):
    """(pred_R f32 [b,3,3], gt_R f32 [b,3,3]) -> angles f32 [b] in radians: acos_safe(0.5 (tr(pred_R gt_R^T) - 1)), per pair
    like the reference's (its name notwithstanding).  A handful of element-wise torch operations in fp64 on [b] values; the
    decode entry computes the same from its unrounded pred_R when it is given the ground truth."""
    pred_R, gt_R = _mat33(pred_R, "pred_R", 1), _mat33(gt_R, "gt_R", 1)
    _lib.same_device(pred_R, gt_R)
    if pred_R.shape != gt_R.shape:
        raise ValueError(f"pred_R {tuple(pred_R.shape)} and gt_R {tuple(gt_R.shape)} differ in shape")
    x = 0.5 * ((pred_R.double() * gt_R.double()).sum(dim=(1, 2)) - 1.0)
    lim = 1.0 - _ACOS_EPS
    slope = float(np.arccos(lim) / _ACOS_EPS)
    sign = torch.sign(x)
    far = torch.acos(sign * lim) - slope * sign * (x.abs() - lim)
    return torch.where(x.abs() <= lim, torch.acos(x.clamp(-1.0, 1.0)), far).float()
