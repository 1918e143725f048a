"""Evaluation of the classification network on the device: the loop of SPConvNets/trainer_modelnet.py:138-210 (network, loss,
accuracy per batch, the mean of the per-batch accuracies) without its two .item() calls per batch, and with the class x anchor
table that upstream builds on the host and has commented out (lmc, :157, :179-182).  Per chunk: forward(), the loss
(losses.classification_loss) and one tally launch (losses.classification_tally); one host synchronisation at the end.
DESIGN.md 3.1g."""
import collections

import numpy as np
import torch

from . import losses

ClassificationEval = collections.namedtuple(
    "ClassificationEval", "instance_acc batch_mean_acc loss cls_loss att_loss att_acc class_acc confusion anchor_table rows skipped "
                          "batch_acc")
ClassificationEval.__doc__ = """evaluate_classification's result, host values: instance_acc (clouds classified correctly over
clouds counted), batch_mean_acc (upstream's figure, trainer_modelnet.py:195-197: the mean of the per-batch accuracies in float32,
which weighs a short last batch like a full one), loss, cls_loss and att_loss (means of the per-batch values weighted by the
batch's size, i.e. per cloud; att_loss and att_acc are NaN without r_labels), att_acc (attention rows correct over clouds
counted), class_acc float64 [k], confusion int32 [k,k] at (label, prediction), anchor_table int32 [k,A] at (label, most attended
anchor) or None for a head without attention, rows and skipped (clouds counted; clouds left out of every count because a flag was
set: a label out of range, a non-finite logit), batch_acc float32 [chunks]."""


def check_clouds(pc, batch):
    """What classify and evaluate_classification refuse about their clouds, on the host: pc float32 [M,N,3], batch >= 1.
    -> int(batch)."""
    if not isinstance(pc, torch.Tensor):
        raise TypeError(f"pc must be a torch tensor, got {type(pc).__name__}")
    if pc.dim() != 3 or pc.shape[2] != 3:
        raise ValueError(f"pc must be [M, N, 3], got {tuple(pc.shape)}")
    if pc.dtype != torch.float32:
        raise TypeError(f"pc must be torch.float32, got {pc.dtype}")
    if int(batch) != batch or int(batch) < 1:
        raise ValueError(f"batch must be an integer >= 1, got {batch}")
    return int(batch)


def _attention_of(model, logits, feat):
    """The network's second output as [b, A] attention logits, or None for a head that pools without attention ('max',
    'mean': their second output is the pre-pointnet feature map, whatever its shape).  Decided by the head's pooling mode."""
    if not str(getattr(model.outblock, "pooling_method", "")).startswith("attention"):
        return None
    return feat.reshape(logits.shape[0], -1)                    # squeeze() upstream: [A] for a single cloud


def forward_chunk(model, pc):
    """(pc [b,N,3]) -> (logits f32 [b,k], predicted class int32 [b], most attended anchor int32 [b] or -1).  The caller holds
    torch.no_grad()."""
    logits, feat = model(pc)
    logits = logits.float()
    att = _attention_of(model, logits, feat)
    zeros = torch.zeros(logits.shape[0], dtype=torch.int32, device=logits.device)
    r = losses.classification_loss(logits, zeros, att, None if att is None else zeros)       # the labels do not enter an arg max
    return logits, r.preds, r.att_preds if att is not None else torch.full_like(r.preds, -1)


def evaluate_classification(model, clouds, labels, r_labels=None, *, batch=32, loss=None, pretrain_step=2000):
    """(model: a ClsSO3ConvModel in eval() mode; clouds f32 [M,N,3] and labels int [M] on the device; r_labels int [M]: the
    loader's R_label, or None; loss: a vgtk.AttentionCrossEntropyLoss whose blend weights the reported loss uses -- at its
    current iter_counter with the trainer's pretrain_step (what the trainer passes to the loss's forward; read by 'schedule'
    only), its counter is not advanced -- or None for cls_loss + r_loss, cls_loss alone without r_labels) -> ClassificationEval.  The device form
    of trainer_modelnet.eval(): the clouds go through forward() in chunks of `batch` under torch.no_grad(), each followed by the
    loss and the tally; nothing is read back until all chunks are queued."""
    if model.training:
        raise RuntimeError("evaluate_classification() needs the model in eval() mode: call model.eval() first")
    batch = check_clouds(clouds, batch)
    M = clouds.shape[0]
    for name, t in (("labels", labels), ("r_labels", r_labels)):
        if t is None and name == "r_labels":
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch tensor, got {type(t).__name__}")
        if tuple(t.shape) != (M,):
            raise ValueError(f"{name} must be [{M}], got {tuple(t.shape)}")
        if t.dtype not in (torch.int32, torch.int64):
            raise TypeError(f"{name} must be torch.int32 or torch.int64, got {t.dtype}")
        if t.device != clouds.device:
            raise RuntimeError(f"{name} is on {t.device}, the clouds on {clouds.device}")
    if M == 0:
        raise ValueError("evaluate_classification() needs at least one cloud")
    if not clouds.is_cuda:
        raise RuntimeError("clouds must be a CUDA tensor")
    coef = (1.0, 1.0 if r_labels is not None else 0.0)
    if loss is not None:
        coef = tuple(float(c) for c in loss.coefficients(pretrain_step))
    coef = torch.tensor(coef, dtype=torch.float32, device=clouds.device)
    tables, scalars, sizes = None, [], []
    with torch.no_grad():
        for i in range(0, M, batch):
            logits, feat = model(clouds[i:i + batch])
            lab = labels[i:i + batch]
            att = _attention_of(model, logits, feat)
            if att is None and r_labels is not None:
                raise ValueError("r_labels were given, but the model's head returns no [b, A] attention logits")
            if tables is None:
                tables = losses.ClassificationTables(logits.shape[1], 0 if att is None else att.shape[1], clouds.device)
            rl = None if r_labels is None else r_labels[i:i + batch]
            # without r_labels the attention rows still go through the kernel for their arg max (zero labels, weight zero)
            r = losses.classification_loss(logits, lab, att, None if att is None else (torch.zeros_like(lab) if rl is None else rl), coef)
            losses.classification_tally(r, lab, tables, rl)
            scalars.append(torch.stack(r[:5]))
            sizes.append(lab.shape[0])
        scalars = torch.stack(scalars).cpu().numpy()                                # the one synchronisation
        t = tables.result()
    w = np.asarray(sizes, dtype=np.float64) / M
    mean = (scalars.astype(np.float64) * w[:, None]).sum(axis=0)
    nan = float("nan")
    return ClassificationEval(t.instance_acc, float(scalars[:, 3].mean()), float(mean[0]), float(mean[1]),
                              float(mean[2]) if r_labels is not None else nan, t.attention_acc, t.class_acc, t.confusion,
                              t.anchor_table, t.rows, t.skipped, scalars[:, 3].copy())
