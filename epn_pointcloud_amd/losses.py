"""The descriptor network's training loss on the GPU: batch-hard triplet mining over two descriptor sets and the anchor
interpolation of the equivariance term, the two pieces of the reference's TripletBatchLoss (vgtk/vgtk/loss.py:220-235, :280-318,
:400-445) -- the only loss SPConvNets/trainer_3dmatch.py uses.  The mirror of that class is epn_pointcloud_amd.vgtk.loss.

Specification: include/epn_so3conv.h (epn_triplet_batch_hard_f32 and its backward, epn_anchor_interp_f32 and its backward) and
DESIGN.md 3.1d; kernels: csrc/triplet_loss.hip.  Forward two launches (one for the interpolation), backward one; nothing
synchronises with the host and nothing indexes with a boolean mask, so a step that ends in this loss can be captured into a
HIP graph -- the reference's dist_mat[is_neg] (loss.py:234) cannot.

And the rotation network's: rotation_loss, the alignment branch of the reference's MultiTaskDetectionLoss (loss.py:140-181) --
anchor cross-entropy plus the L2 distance of the regressed relative rotations -- the loss SPConvNets/trainer_modelnetRotation.py
trains with.  Specification: epn_rotation_loss_f32 and its backward; kernels: csrc/rotation_loss.hip.  Forward
two launches, backward one, under the same rules.

And the classification network's: classification_loss, the reference's CrossEntropyLoss and AttentionCrossEntropyLoss
(loss.py:18-75) -- class cross-entropy blended with the cross-entropy of the anchor attention -- the loss
SPConvNets/trainer_modelnet.py trains with, and classification_tally, the counting of its evaluation loop.  Specification:
epn_cls_loss_f32, its backward and epn_cls_tally_i32; kernels: csrc/cls_loss.hip.  Forward two launches, backward
one, tally one; the blend weights are read on the device.

Shapes and dtypes are checked on the host before the device is touched: type, shape, dtype, then device."""
import collections

import torch

from . import _lib

MODES = {"hard": 0, "soft": 1, "contrastive": 2}        # the mode numbers of include/epn_so3conv.h
EPS = 1e-6                                              # pairwise_distance_matrix's clamp, loss.py:220
MAX_ROWS = 65536
ANCHOR_COUNTS = (12, 60)
KNN = 3

TripletResult = collections.namedtuple("TripletResult", "loss accuracy pos neg neg_idx nn_idx")
TripletResult.__doc__ = """batch_hard_triplet's result: loss (f32 scalar, the mean row loss; the only differentiable field),
accuracy (share of rows whose nearest tgt row is their own), pos and neg (mean positive and mean hardest-negative distance) --
the four values TripletBatchLoss._forward_invariance returns -- and neg_idx, nn_idx int32 [N]: the hardest negative and the
nearest tgt row of every src row (the lowest index on a tie)."""


def _check_pair(src, tgt, mode, margin):
    """Everything batch_hard_triplet refuses, decided on the host from metadata alone -> (N, D, mode number)."""
    for name, t in (("src", src), ("tgt", tgt)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch tensor, got {type(t).__name__}")
        if t.dim() != 2:
            raise ValueError(f"{name} must be [N, D], got {tuple(t.shape)}")
    if src.shape != tgt.shape:
        raise ValueError(f"src {tuple(src.shape)} and tgt {tuple(tgt.shape)} differ in shape: row i of tgt is the positive of row i of src")
    N, D = src.shape
    if N < 2:
        raise ValueError(f"batch-hard mining needs N >= 2 rows, got {N}: with one row there is no negative to mine (the reference "
                         "fails on it too)")
    if N > MAX_ROWS:
        raise ValueError(f"N = {N} is beyond the {MAX_ROWS} rows one call takes")
    if D < 1 or N * D >= 2 ** 31:
        raise ValueError(f"D must be >= 1 with N * D < 2^31, got N = {N}, D = {D}")
    for name, t in (("src", src), ("tgt", tgt)):
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be torch.float32, got {t.dtype}")
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)}, got {mode!r}")
    margin = float(margin)
    if margin != margin or margin in (float("inf"), float("-inf")) or (mode == "soft" and margin <= 0.0):
        raise ValueError(f"margin must be finite (and > 0 in soft mode, where it is softplus's beta), got {margin}")
    for name, t in (("src", src), ("tgt", tgt)):
        if not t.is_cuda:
            raise RuntimeError(f"{name} must be a CUDA tensor")
    _lib.same_device(src, tgt)
    return N, D, MODES[mode]


class _BatchHard(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, tgt, mode, margin):
        N, D = src.shape
        src, tgt = src.contiguous(), tgt.contiguous()
        f32, i32 = dict(dtype=torch.float32, device=src.device), dict(dtype=torch.int32, device=src.device)
        d_pos, d_neg, row_loss = torch.empty(N, **f32), torch.empty(N, **f32), torch.empty(N, **f32)
        neg_idx, nn_idx, row_flags = torch.empty(N, **i32), torch.empty(N, **i32), torch.empty(N, **i32)
        scalars = torch.empty(4, **f32)
        p = _lib.dev_ptr
        _lib.check(_lib.get_lib().epn_triplet_batch_hard_f32(
            p(src, "src"), p(tgt, "tgt"), N, D, mode, margin, EPS, p(d_pos, "d_pos"), p(d_neg, "d_neg"), p(row_loss, "row_loss"),
            p(neg_idx, "neg_idx", torch.int32), p(nn_idx, "nn_idx", torch.int32), p(row_flags, "row_flags", torch.int32),
            p(scalars, "scalars"), _lib.stream_of(src)), "triplet_batch_hard")
        ctx.save_for_backward(src, tgt, d_pos, d_neg, neg_idx, row_flags)
        ctx.mode, ctx.margin = mode, margin
        ctx.set_materialize_grads(False)                    # no zero fills for the outputs nobody differentiates
        loss, accuracy, pos, neg = scalars.unbind(0)
        ctx.mark_non_differentiable(accuracy, pos, neg, d_pos, d_neg, row_loss, neg_idx, nn_idx, row_flags)
        return loss, accuracy, pos, neg, d_pos, d_neg, row_loss, neg_idx, nn_idx, row_flags

    @staticmethod
    def backward(ctx, g_loss, *unused):
        if g_loss is None:
            return None, None, None, None
        src, tgt, d_pos, d_neg, neg_idx, row_flags = ctx.saved_tensors
        N, D = src.shape
        upstream = g_loss.reshape(1).to(torch.float32).contiguous()
        dsrc, dtgt = torch.empty_like(src), torch.empty_like(tgt)
        p = _lib.dev_ptr
        _lib.check(_lib.get_lib().epn_triplet_batch_hard_bwd_f32(
            p(upstream, "upstream"), p(src, "src"), p(tgt, "tgt"), p(d_pos, "d_pos"), p(d_neg, "d_neg"),
            p(neg_idx, "neg_idx", torch.int32), p(row_flags, "row_flags", torch.int32), N, D, ctx.mode, ctx.margin,
            p(dsrc, "dsrc"), p(dtgt, "dtgt"), _lib.stream_of(src)), "triplet_batch_hard_bwd")
        return dsrc, dtgt, None, None


def batch_hard_rows(src, tgt, mode="hard", margin=1.0):
    """batch_hard_triplet with the per-row outputs of the entry as well -> (TripletResult, rows) with rows a dict of d_pos,
    d_neg, row_loss f32 [N] and row_flags int32 [N] (include/epn_so3conv.h).  None of the per-row tensors is differentiable."""
    N, D, m = _check_pair(src, tgt, mode, margin)
    loss, accuracy, pos, neg, d_pos, d_neg, row_loss, neg_idx, nn_idx, row_flags = _BatchHard.apply(src, tgt, m, float(margin))
    return (TripletResult(loss, accuracy, pos, neg, neg_idx, nn_idx),
            dict(d_pos=d_pos, d_neg=d_neg, row_loss=row_loss, row_flags=row_flags))


def batch_hard_triplet(src, tgt, mode="hard", margin=1.0):
    """(src, tgt f32 [N,D] on the device: row i of tgt is the positive of row i of src, every other row a negative; mode "hard" |
    "soft" | "contrastive": relu(pos - neg + margin), softplus(pos - neg, beta=margin), pos + relu(margin - neg)) ->
    TripletResult.  Distances are sqrt(max(sum_d (s - t)^2, 1e-6)) from the differences in fp64; the hardest negative of a row is
    its nearest other tgt row.  loss.backward() reaches src and tgt through one launch; accuracy, pos and neg are for logging
    and carry no gradient."""
    return batch_hard_rows(src, tgt, mode, margin)[0]


RotationLossResult = collections.namedtuple("RotationLossResult", "loss cls_loss reg r_acc preds row_ce row_l2 row_flags")
RotationLossResult.__doc__ = """rotation_loss's result: loss (f32 scalar, cls_loss + reg; the only differentiable field), cls_loss
(the mean cross-entropy over the b * A rows), reg (w times the mean squared difference of the selected rotations to R_target),
r_acc (share of rows whose most confident target anchor is the label) -- the first four values MultiTaskDetectionLoss.forward
returns -- and per row [b,A]: preds int32 (the most confident target anchor, the lowest on a tie), row_ce and row_l2 f32,
row_flags int32 (bit 0: the label lies outside 0..A-1 and the row counts as zero; bit 1: a norm of the rotation map was below
1e-8 and clamped)."""

MAX_ANCHORS = 64
ROTATION_WIDTHS = (4, 6)


def _check_rotation_loss(confidence, y, label, R_target, w):
    """Everything rotation_loss refuses, decided on the host from metadata alone (a host label's values included) -> (b, A, nr)."""
    for name, t in (("confidence", confidence), ("y", y), ("label", label), ("R_target", R_target)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch tensor, got {type(t).__name__}")
    if confidence.dim() != 3 or confidence.shape[1] != confidence.shape[2] or not 1 <= confidence.shape[1] <= MAX_ANCHORS:
        raise ValueError(f"confidence must be [b, A, A] (target anchor, source anchor) with 1 <= A <= {MAX_ANCHORS}, got "
                         f"{tuple(confidence.shape)}")
    b, A = confidence.shape[0], confidence.shape[1]
    if b < 1:
        raise ValueError("the loss is a mean over b * A rows and needs b >= 1 pairs, got 0")
    if y.dim() != 4 or y.shape[0] != b or y.shape[1] not in ROTATION_WIDTHS or tuple(y.shape[2:]) != (A, A):
        raise ValueError(f"y must be [{b}, 4 | 6, {A}, {A}], got {tuple(y.shape)}")
    if tuple(label.shape) != (b, A):
        raise ValueError(f"label must be [{b}, {A}], got {tuple(label.shape)}")
    if tuple(R_target.shape) != (b, A, 3, 3):
        raise ValueError(f"R_target must be [{b}, {A}, 3, 3], got {tuple(R_target.shape)}")
    for name, t in (("confidence", confidence), ("y", y)):
        if not t.is_floating_point():
            raise TypeError(f"{name} must be a floating-point tensor, got {t.dtype}")
    if label.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"label must be torch.int32 or torch.int64, got {label.dtype}")
    if R_target.dtype != torch.float32:
        raise TypeError(f"R_target must be torch.float32, got {R_target.dtype}")
    w = float(w)
    if w != w or w in (float("inf"), float("-inf")):
        raise ValueError(f"w must be finite, got {w}")
    # a host label (a loader's) is range-checked here and uploaded by the caller; checking a device label would synchronise:
    # the kernels check it themselves and report a value outside 0..A-1 in bit 0 of row_flags
    if not label.is_cuda and not (0 <= int(label.min()) and int(label.max()) < A):
        raise ValueError(f"label must lie in 0..{A - 1}")
    for name, t in (("confidence", confidence), ("y", y), ("R_target", R_target)):
        if not t.is_cuda:
            raise RuntimeError(f"{name} must be a CUDA tensor")
    return b, A, y.shape[1]


class _RotationLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, wts, y, label, R_target, w):
        b, nr, A = y.shape[0], y.shape[1], y.shape[2]
        f32, i32 = dict(dtype=torch.float32, device=wts.device), dict(dtype=torch.int32, device=wts.device)
        row_ce, row_l2, sel_R = torch.empty((b, A), **f32), torch.empty((b, A), **f32), torch.empty((b, A, 3, 3), **f32)
        preds, row_flags = torch.empty((b, A), **i32), torch.empty((b, A), **i32)
        scalars = torch.empty(4, **f32)
        p = _lib.dev_ptr
        _lib.check(_lib.get_lib().epn_rotation_loss_f32(
            p(wts, "confidence"), p(y, "y"), p(label, "label", torch.int32), p(R_target, "R_target"), b, A, nr, w,
            p(row_ce, "row_ce"), p(row_l2, "row_l2"), p(preds, "preds", torch.int32), p(row_flags, "row_flags", torch.int32),
            p(sel_R, "sel_R"), p(scalars, "scalars"), _lib.stream_of(wts)), "rotation_loss")
        ctx.save_for_backward(wts, y, label, R_target, row_flags)
        ctx.w = w
        ctx.set_materialize_grads(False)                    # no zero fills for the outputs nobody differentiates
        loss, cls_loss, reg, r_acc = scalars.unbind(0)
        ctx.mark_non_differentiable(cls_loss, reg, r_acc, preds, row_ce, row_l2, row_flags, sel_R)
        return loss, cls_loss, reg, r_acc, preds, row_ce, row_l2, row_flags, sel_R

    @staticmethod
    def backward(ctx, g_loss, *unused):
        if g_loss is None:
            return None, None, None, None, None
        wts, y, label, R_target, row_flags = ctx.saved_tensors
        b, nr, A = y.shape[0], y.shape[1], y.shape[2]
        upstream = g_loss.reshape(1).to(torch.float32).contiguous()
        dwts, dy = torch.empty_like(wts), torch.empty_like(y)
        p = _lib.dev_ptr
        _lib.check(_lib.get_lib().epn_rotation_loss_bwd_f32(
            p(upstream, "upstream"), p(wts, "confidence"), p(y, "y"), p(label, "label", torch.int32), p(R_target, "R_target"),
            p(row_flags, "row_flags", torch.int32), b, A, nr, ctx.w, p(dwts, "dwts"), p(dy, "dy"), _lib.stream_of(wts)),
            "rotation_loss_bwd")
        return dwts, dy, None, None, None


def rotation_loss_rows(confidence, y, label, R_target, w=10.0):
    """rotation_loss with the selected rotations as well -> (RotationLossResult, sel_R f32 [b,A,3,3]: the rotation map of
    y[p,:,label[p,a],a], zero where bit 0 of row_flags is set; not differentiable)."""
    _check_rotation_loss(confidence, y, label, R_target, w)
    # the head hands out channels-last y, under autocast bf16: the conversion is torch's, and the gradient flows back through it
    wts, yc = confidence.float().contiguous(), y.float().contiguous()
    label = label.to(device=wts.device, dtype=torch.int32).contiguous()
    R_target = R_target.detach().contiguous()
    _lib.same_device(wts, yc, label, R_target)
    out = _RotationLoss.apply(wts, yc, label, R_target, float(w))
    return RotationLossResult(*out[:8]), out[8]


def rotation_loss(confidence, y, label, R_target, w=10.0):
    """(confidence [b,A,A] (target anchor, source anchor) and y [b,4|6,A,A]: RegSO3ConvModel.forward's outputs, A <= 64; label
    int32 / int64 [b,A] and R_target f32 [b,A,3,3]: label_relative_rotation's outputs; w: the weight of the L2 term) ->
    RotationLossResult.  The alignment branch of the reference's MultiTaskDetectionLoss.forward (vgtk/vgtk/loss.py:140-181):
    cross-entropy over the target-anchor axis of confidence taken as logits, plus w times the mean squared difference between
    R_target and the rotation map (quaternion for 4 rows of y, Gram-Schmidt for 6) of y at the labelled target anchor.
    Specification: include/epn_so3conv.h (epn_rotation_loss_f32 and its backward); fp64 inside, two launches
    forward, one backward, nothing synchronises.  loss.backward() reaches confidence and y; everything else is for logging.
    Label range: a HOST label is checked against 0..A-1 here and uploaded; a DEVICE label is not (that would synchronise): a value
    outside 0..A-1 there sets bit 0 of that row's row_flags, and the row counts as zero in both sums and in the gradient."""
    return rotation_loss_rows(confidence, y, label, R_target, w)[0]


ClsLossResult = collections.namedtuple(
    "ClsLossResult", "loss cls_loss att_loss acc att_acc preds att_preds row_ce att_row_ce row_flags att_row_flags")
ClsLossResult.__doc__ = """classification_loss's result: loss (f32 scalar, c_cls * cls_loss + c_att * att_loss; the only
differentiable field), cls_loss and att_loss (the mean cross-entropy over the B class rows and over the R attention rows), acc and
att_acc (share of rows whose arg max is the label) -- the five values AttentionCrossEntropyLoss.forward returns -- and per row:
preds int32 [B] and att_preds int32 [B] or [B,C] (the arg max, the lowest index on a tie, -1 for a row with a non-finite logit),
row_ce and att_row_ce f32, row_flags and att_row_flags int32 (bit 0: the label lies outside the row's classes and the row counts
as zero; bit 1: the row holds a non-finite logit).  Without attention: att_loss = att_acc = 0 and the att_* rows are None."""

MAX_CLASSES = 4096


def _check_classification_loss(logits, label, attention, attention_label, coef):
    """Everything classification_loss refuses, decided on the host from metadata alone (a host label's values included)."""
    for name, t in (("logits", logits), ("label", label)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch tensor, got {type(t).__name__}")
    if (attention is None) != (attention_label is None):
        raise TypeError("attention and attention_label come together: both tensors, or both None")
    for name, t in (("attention", attention), ("attention_label", attention_label)):
        if t is not None and not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch tensor, got {type(t).__name__}")
    if not isinstance(coef, torch.Tensor):
        if not isinstance(coef, (tuple, list)) or len(coef) != 2 or not all(isinstance(c, (int, float)) for c in coef):
            raise TypeError(f"coef must be a pair of floats or a device float32 tensor of two elements, got {coef!r}")
    if logits.dim() != 2 or not 1 <= logits.shape[0] <= MAX_ROWS or not 1 <= logits.shape[1] <= MAX_CLASSES:
        raise ValueError(f"logits must be [B, k] with 1 <= B <= {MAX_ROWS} and 1 <= k <= {MAX_CLASSES}, got {tuple(logits.shape)}")
    B, k = logits.shape
    if tuple(label.shape) != (B,):
        raise ValueError(f"label must be [{B}], got {tuple(label.shape)}")
    if attention is not None:
        if attention.dim() not in (2, 3) or attention.shape[0] != B or not 1 <= attention.shape[-1] <= MAX_CLASSES:
            raise ValueError(f"attention must be [{B}, A] or [{B}, C, A] with 1 <= A <= {MAX_CLASSES}, got {tuple(attention.shape)}")
        R = attention.numel() // attention.shape[-1]
        if not 1 <= R <= MAX_ROWS:
            raise ValueError(f"attention has {R} rows, one call takes 1..{MAX_ROWS}")
        if tuple(attention_label.shape) != tuple(attention.shape[:-1]):
            raise ValueError(f"attention_label must be {list(attention.shape[:-1])}, got {tuple(attention_label.shape)}")
    if isinstance(coef, torch.Tensor) and (tuple(coef.shape) != (2,) or not coef.is_contiguous()):
        # a strided view would have to be copied, and a captured step would then never see its later updates
        raise ValueError(f"a coef tensor must be a contiguous [2] = (c_cls, c_att), got shape {tuple(coef.shape)}, stride "
                         f"{tuple(coef.stride())}")
    for name, t in (("logits", logits), ("attention", attention)):
        if t is not None and not t.is_floating_point():
            raise TypeError(f"{name} must be a floating-point tensor, got {t.dtype}")
    for name, t in (("label", label), ("attention_label", attention_label)):
        if t is not None and t.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"{name} must be torch.int32 or torch.int64, got {t.dtype}")
    if isinstance(coef, torch.Tensor):
        if coef.dtype != torch.float32:
            raise TypeError(f"a coef tensor must be torch.float32, got {coef.dtype}")
    elif not all(c == c and c not in (float("inf"), float("-inf")) for c in map(float, coef)):
        raise ValueError(f"coef must be finite, got {coef!r}")
    # a host label (a loader's) is range-checked here and uploaded by the caller; checking a device label would synchronise:
    # the kernels check it themselves and report a value outside the row's classes in bit 0 of the row's flags
    for name, t, n in (("label", label, k), ("attention_label", attention_label, attention.shape[-1] if attention is not None else 0)):
        if t is not None and not t.is_cuda and not (0 <= int(t.min()) and int(t.max()) < n):
            raise ValueError(f"{name} must lie in 0..{n - 1}")
    for name, t in (("logits", logits), ("attention", attention), ("coef", coef if isinstance(coef, torch.Tensor) else None)):
        if t is not None and not t.is_cuda:
            raise RuntimeError(f"{name} must be a CUDA tensor")


class _ClsLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, label, att, att_label, coef):
        B, k = logits.shape
        R, A = (att.shape[0], att.shape[1]) if att is not None else (0, 0)
        f32, i32 = dict(dtype=torch.float32, device=logits.device), dict(dtype=torch.int32, device=logits.device)
        row_ce, preds, row_flags = torch.empty(B, **f32), torch.empty(B, **i32), torch.empty(B, **i32)
        att_row_ce = att_preds = att_row_flags = None
        if R:
            att_row_ce, att_preds, att_row_flags = torch.empty(R, **f32), torch.empty(R, **i32), torch.empty(R, **i32)
        scalars = torch.empty(5, **f32)
        p = _lib.dev_ptr
        _lib.check(_lib.get_lib().epn_cls_loss_f32(
            p(logits, "logits"), p(label, "label", torch.int32), B, k, p(att, "attention"), p(att_label, "attention_label", torch.int32),
            R, A, p(coef, "coef"), p(row_ce, "row_ce"), p(preds, "preds", torch.int32), p(row_flags, "row_flags", torch.int32),
            p(att_row_ce, "att_row_ce"), p(att_preds, "att_preds", torch.int32), p(att_row_flags, "att_row_flags", torch.int32),
            p(scalars, "scalars"), _lib.stream_of(logits)), "classification_loss")
        ctx.save_for_backward(logits, label, row_flags, att, att_label, att_row_flags, coef)
        ctx.set_materialize_grads(False)                    # no zero fills for the outputs nobody differentiates
        loss, cls_loss, att_loss, acc, att_acc = scalars.unbind(0)
        ctx.mark_non_differentiable(*(t for t in (cls_loss, att_loss, acc, att_acc, preds, att_preds, row_ce, att_row_ce, row_flags,
                                                  att_row_flags) if t is not None))
        return loss, cls_loss, att_loss, acc, att_acc, preds, att_preds, row_ce, att_row_ce, row_flags, att_row_flags

    @staticmethod
    def backward(ctx, g_loss, *unused):
        if g_loss is None:
            return None, None, None, None, None
        logits, label, row_flags, att, att_label, att_row_flags, coef = ctx.saved_tensors
        B, k = logits.shape
        R, A = (att.shape[0], att.shape[1]) if att is not None else (0, 0)
        upstream = g_loss.reshape(1).to(torch.float32).contiguous()
        dlogits = torch.empty_like(logits)
        datt = torch.empty_like(att) if R else None
        p = _lib.dev_ptr
        _lib.check(_lib.get_lib().epn_cls_loss_bwd_f32(
            p(upstream, "upstream"), p(logits, "logits"), p(label, "label", torch.int32), p(row_flags, "row_flags", torch.int32), B, k,
            p(att, "attention"), p(att_label, "attention_label", torch.int32), p(att_row_flags, "att_row_flags", torch.int32), R, A,
            p(coef, "coef"), p(dlogits, "dlogits"), p(datt, "datt"), _lib.stream_of(logits)), "classification_loss_bwd")
        return dlogits, None, datt, None, None


def classification_loss(logits, label, attention=None, attention_label=None, coef=(1.0, 1.0)):
    """(logits [B,k]: ClsSO3ConvModel.forward's first output; label int32 / int64 [B]; attention [B,A] with attention_label [B]
    -- the network's second output and the loader's R_label -- or [B,C,A] with attention_label [B,C], one row per (b, c); coef =
    (c_cls, c_att): a pair of floats, or a contiguous DEVICE float32 [2] tensor that is used in place, never copied) -> ClsLossResult.  The reference's
    CrossEntropyLoss (attention None) and AttentionCrossEntropyLoss (vgtk/vgtk/loss.py:18-75) with the blend left to coef:
    loss = c_cls * mean CE(logits, label) + c_att * mean CE(attention rows, attention_label).
    Specification: include/epn_so3conv.h (epn_cls_loss_f32 and its backward); fp64 inside, two launches forward,
    one backward, nothing synchronises.  loss.backward() reaches logits and attention; everything else is for logging.  The
    kernels read coef on the device: a captured step replays with new blend weights after coef.copy_(...); a pair of floats is
    uploaded by this call, which a capture does not allow -- pass the tensor there.
    Label range: a HOST label is checked against the row's classes here and uploaded; a DEVICE label is not (that would
    synchronise): a value outside them sets bit 0 of that row's flags, and the row counts as zero in the sums and in the gradient
    while the means still divide by B and R.  torch's cross-entropy asserts on the device there, except for ignore_index = -100,
    which it also takes out of the divisor: -100 is no exception here.  A row with a non-finite logit sets bit 1: its row_ce and
    gradient are NaN (so is the mean) and its prediction is -1."""
    _check_classification_loss(logits, label, attention, attention_label, coef)
    # non-fp32 logits (a bf16 head): the conversion is torch's, and the gradient flows back through it
    x = logits.float().contiguous()
    dev = x.device
    label = label.to(device=dev, dtype=torch.int32).contiguous()
    att = att_label = None
    if attention is not None:
        att = attention.float().contiguous().reshape(-1, attention.shape[-1])
        att_label = attention_label.to(device=dev, dtype=torch.int32).contiguous().reshape(-1)
    coef = coef.detach() if isinstance(coef, torch.Tensor) else torch.tensor([float(c) for c in coef], dtype=torch.float32,
                                                                                         device=dev)
    _lib.same_device(x, label, att, att_label, coef)
    out = list(_ClsLoss.apply(x, label, att, att_label, coef))
    if attention is not None and attention.dim() == 3:
        for i in (6, 8, 10):
            out[i] = out[i].view(attention.shape[:-1])
    return ClsLossResult(*out)


ClassificationTally = collections.namedtuple(
    "ClassificationTally", "instance_acc class_acc attention_acc confusion anchor_table rows skipped")
ClassificationTally.__doc__ = """ClassificationTables.result(): instance_acc (rows correct / rows seen), class_acc (float64 [k]:
the diagonal of confusion over its row sums, NaN for a class never seen), attention_acc (attention rows correct / rows seen; NaN
without attention labels), confusion int32 [k,k] at (label, prediction), anchor_table int32 [k,A] at (label, most attended anchor)
or None, rows (seen) and skipped (flagged rows, left out of every count) -- host values."""


class ClassificationTables:
    """The int32 tables classification_tally adds into, on `device`, zeroed here: confusion [k,k], anchor_table [k,A] (None with
    A = 0) and totals [4] = rows seen, rows correct, attention rows correct, rows skipped.  They accumulate over any number of
    calls without a host synchronisation; result() performs the one copy to the host."""

    def __init__(self, k, A=0, device="cuda"):
        k, A = int(k), int(A)
        if not 1 <= k <= MAX_CLASSES or not 0 <= A <= MAX_CLASSES:
            raise ValueError(f"the tables take 1 <= k <= {MAX_CLASSES} classes and 0 <= A <= {MAX_CLASSES} anchors, got k = {k}, A = {A}")
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("the tables live on a CUDA device")
        self.k, self.A = k, A
        self.confusion = torch.zeros((k, k), dtype=torch.int32, device=device)
        self.anchor_table = torch.zeros((k, A), dtype=torch.int32, device=device) if A else None
        self.totals = torch.zeros(4, dtype=torch.int32, device=device)
        self.attention_labelled = False

    def zero_(self):
        for t in (self.confusion, self.anchor_table, self.totals):
            if t is not None:
                t.zero_()
        self.attention_labelled = False
        return self

    def result(self):
        import numpy as np
        confusion, totals = self.confusion.cpu().numpy(), self.totals.cpu().numpy()
        anchor_table = None if self.anchor_table is None else self.anchor_table.cpu().numpy()
        seen, hit, att_hit, skipped = (int(v) for v in totals)
        per_class = confusion.sum(axis=1).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            class_acc = np.where(per_class > 0, np.diagonal(confusion) / per_class, np.nan)
        nan = float("nan")
        return ClassificationTally(hit / seen if seen else nan, class_acc,
                                   att_hit / seen if seen and self.attention_labelled else nan, confusion, anchor_table, seen, skipped)


def classification_tally(result, label, tables, attention_label=None):
    """(result: a ClsLossResult; label int32 / int64 [B] on the device: the labels it was computed with; tables: a
    ClassificationTables on the same device) -> tables, with every unflagged row of the batch added: confusion at (label,
    prediction), rows seen and correct, and -- when result carries one attention row per cloud (the [B,A] layout) and the tables
    have an anchor table -- the class x anchor table at (label, most attended anchor), upstream's commented-out lmc
    (trainer_modelnet.py:157, :179-182); with attention_label [B] also the attention rows correct.  A row with any flag bit is
    skipped and counted in totals[3].  One launch (epn_cls_tally_i32), nothing synchronises."""
    if not isinstance(result, ClsLossResult):
        raise TypeError(f"result must be a ClsLossResult, got {type(result).__name__}")
    if not isinstance(label, torch.Tensor):
        raise TypeError(f"label must be a torch tensor, got {type(label).__name__}")
    if not isinstance(tables, ClassificationTables):
        raise TypeError(f"tables must be a ClassificationTables, got {type(tables).__name__}")
    if attention_label is not None and not isinstance(attention_label, torch.Tensor):
        raise TypeError(f"attention_label must be a torch tensor, got {type(attention_label).__name__}")
    B = result.preds.shape[0]
    if tuple(label.shape) != (B,):
        raise ValueError(f"label must be [{B}], got {tuple(label.shape)}")
    with_att = tables.anchor_table is not None and result.att_preds is not None and result.att_preds.dim() == 1
    if attention_label is not None:
        if not with_att:
            raise ValueError("attention_label needs one attention row per cloud in result and an anchor table in tables")
        if tuple(attention_label.shape) != (B,):
            raise ValueError(f"attention_label must be [{B}], got {tuple(attention_label.shape)}")
    for name, t in (("label", label), ("attention_label", attention_label)):
        if t is not None and t.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"{name} must be torch.int32 or torch.int64, got {t.dtype}")
    for name, t in (("label", label), ("attention_label", attention_label)):
        if t is not None and not t.is_cuda:
            raise RuntimeError(f"{name} must be a CUDA tensor")
    label = label.to(torch.int32).contiguous()
    att_label = None if attention_label is None else attention_label.to(torch.int32).contiguous()
    _lib.same_device(result.preds, label, att_label, tables.confusion)
    p = _lib.dev_ptr
    i32 = torch.int32
    _lib.check(_lib.get_lib().epn_cls_tally_i32(
        p(result.preds, "preds", i32), p(label, "label", i32), p(result.row_flags, "row_flags", i32),
        p(result.att_preds if with_att else None, "att_preds", i32), p(att_label, "attention_label", i32),
        p(result.att_row_flags if with_att else None, "att_row_flags", i32), B, tables.k, tables.A,
        p(tables.confusion, "confusion", i32), p(tables.anchor_table, "anchor_table", i32), p(tables.totals, "totals", i32),
        _lib.stream_of(label)), "classification_tally")
    tables.attention_labelled |= att_label is not None
    return tables


def _check_interp(feature, T, anchors, sigma):
    """Everything interpolate_anchor_features refuses, on the host -> (nb, C, A)."""
    for name, t in (("feature", feature), ("T", T), ("anchors", anchors)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch tensor, got {type(t).__name__}")
    if anchors.dim() != 3 or tuple(anchors.shape[1:]) != (3, 3):
        raise ValueError(f"anchors must be [A, 3, 3], got {tuple(anchors.shape)}")
    A = anchors.shape[0]
    if A not in ANCHOR_COUNTS:
        raise ValueError(f"the anchor interpolation takes A in {ANCHOR_COUNTS} anchors (the tetrahedral and icosahedral tables), got {A}")
    if feature.dim() != 3 or feature.shape[2] != A or feature.shape[1] < 1:
        raise ValueError(f"feature must be [nb, C, {A}] with C >= 1, got {tuple(feature.shape)}")
    nb, C = feature.shape[0], feature.shape[1]
    if T.dim() != 3 or T.shape[0] != nb or tuple(T.shape[1:]) not in ((3, 3), (4, 4)):
        raise ValueError(f"T must be [{nb}, 3, 3] or [{nb}, 4, 4], got {tuple(T.shape)}")
    if nb * C * A >= 2 ** 31:
        raise ValueError(f"feature has {nb * C * A} elements, one call takes fewer than 2^31")
    for name, t in (("feature", feature), ("T", T), ("anchors", anchors)):
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be torch.float32, got {t.dtype}")
    sigma = float(sigma)
    if not 0.0 < sigma < float("inf"):
        raise ValueError(f"sigma must be finite and > 0, got {sigma}")
    for name, t in (("feature", feature), ("T", T), ("anchors", anchors)):
        if not t.is_cuda:
            raise RuntimeError(f"{name} must be a CUDA tensor")
    _lib.same_device(feature, T, anchors)
    return nb, C, A


class _AnchorInterp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feature, R, anchors, sigma):
        nb, C, A = feature.shape
        feature = feature.contiguous()
        out = torch.empty_like(feature)
        idx = torch.empty((nb, A, KNN), dtype=torch.int32, device=feature.device)
        w = torch.empty((nb, A, KNN), dtype=torch.float32, device=feature.device)
        p = _lib.dev_ptr
        if nb > 0:
            _lib.check(_lib.get_lib().epn_anchor_interp_f32(
                p(feature, "feature"), p(R, "T"), p(anchors, "anchors"), nb, C, A, KNN, sigma, p(out, "out"),
                p(idx, "idx", torch.int32), p(w, "w"), _lib.stream_of(feature)), "anchor_interp")
        ctx.save_for_backward(idx, w)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(idx, w)
        return out, idx, w

    @staticmethod
    def backward(ctx, g_out, *unused):
        if g_out is None:
            return None, None, None, None
        idx, w = ctx.saved_tensors
        g_out = g_out.to(torch.float32).contiguous()
        nb, C, A = g_out.shape
        dfeature = torch.empty_like(g_out)
        p = _lib.dev_ptr
        if nb > 0:
            _lib.check(_lib.get_lib().epn_anchor_interp_bwd_f32(
                p(g_out, "dout"), p(idx, "idx", torch.int32), p(w, "w"), nb, C, A, KNN, p(dfeature, "dfeature"),
                _lib.stream_of(g_out)), "anchor_interp_bwd")
        return dfeature, None, None, None


def interpolate_anchor_features(feature, T, anchors, sigma=0.2, return_weights=False):
    """(feature f32 [nb,C,A]: per-anchor features; T f32 [nb,3,3] or [nb,4,4]: the rigid transform of every sample, of which
    the rotation block is used; anchors f32 [A,3,3], A = 12 or 60) -> f32 [nb,C,A]: for every sample b and anchor n the blend of
    the features at the three anchors m with the largest tr(T_b^T A_n A_m^T), weighted by the softmax of those traces over
    sigma.  TripletBatchLoss._interpolate (loss.py:400-445) with the gather done PER SAMPLE -- the reference's line :424 indexes
    the anchor axis of every sample with the indices of all samples and fails for nb >= 2.  The gradient reaches feature only.
    return_weights=True -> (out, idx int32 [nb,A,3], w f32 [nb,A,3])."""
    _check_interp(feature, T, anchors, sigma)
    R = T[:, :3, :3].detach().contiguous()
    out, idx, w = _AnchorInterp.apply(feature, R, anchors.detach().contiguous(), float(sigma))
    return (out, idx, w) if return_weights else out
