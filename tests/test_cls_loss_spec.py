"""The classification loss and the evaluation tallies without a GPU: the numpy fp64 restatement (tests/cls_loss_ref.py) against
torch's CPU fp64 cross_entropy and autograd, and against the reference's own classes (tests/golden/cls_loss.npz,
gen_golden_cls_loss.py); properties of the restatement; the entries at every layer; every refusal, decided on the host.

Tolerances.
  torch fp64   both sides are fp64 evaluations of the same formulas: 1e-12 relative to the largest magnitude of the compared
               array plus 1e-13 (a few thousand fp64 roundings at n = 4096).
  golden       the reference works in fp32.  The fixture stores the largest difference between its results and the restatement,
               measured when it was written (fwd_err, grad_err); the tests allow exactly that, read from the fixture, plus
               ROUNDINGS = 64 fp64 roundings of the largest compared magnitude: the restatement here may differ from the run
               that measured it by the libm and the summation order of numpy (rows of at most 60 terms)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
import cls_loss_ref as Cf

EINVAL, ENULL = -1, -3
ENTRIES = ("epn_cls_loss_f32", "epn_cls_loss_bwd_f32", "epn_cls_tally_i32")
ROUNDINGS = 64


def _slack(ref):
    return ROUNDINGS * 2.0 ** -53 * float(np.abs(ref).max())


def _close(got, ref, rel=1e-12):
    return np.abs(np.asarray(got) - np.asarray(ref)).max() <= rel * np.abs(ref).max() + 1e-13


def _against_torch(logits, label, att, att_label, coef, g=1.0):
    tl = torch.from_numpy(logits).double().requires_grad_()
    cls = torch.nn.functional.cross_entropy(tl, torch.from_numpy(label).long())
    loss, r = coef[0] * cls, torch.zeros((), dtype=torch.float64)
    ta = None
    if att is not None:
        ta = torch.from_numpy(att).double().requires_grad_()
        a2 = ta.reshape(-1, att.shape[-1])
        r = torch.nn.functional.cross_entropy(a2, torch.from_numpy(np.ascontiguousarray(att_label)).long().reshape(-1))
        loss = loss + coef[1] * r
    (g * loss).backward()
    fwd = Cf.forward(logits, label, att, att_label, coef)
    B = logits.shape[0]
    unrounded = [fwd["row_ce"].sum() / B, 0.0 if att is None else fwd["att_row_ce"].sum() / fwd["att_row_ce"].size]
    assert _close(unrounded, [cls.item(), r.item()])
    assert _close(fwd["scalars"][:3], [loss.item(), cls.item(), r.item()], rel=2.0 ** -23)         # means of ROUNDED rows
    assert fwd["scalars"][3] == (tl.detach().argmax(1).numpy() == label).mean()
    dl, da = Cf.backward(g, logits, label, att, att_label, coef)
    assert _close(dl, tl.grad.numpy()) and (att is None or _close(da, ta.grad.numpy()))


# ----------------------------------------------------------------------------------------------- restatement vs torch fp64
@pytest.mark.parametrize("case", [c for c in Cf.CASES if c[0] <= 33 and c[2] <= 33], ids=str)
def test_restatement_agrees_with_torch_autograd(case):
    _against_torch(*Cf.case(*case))


@pytest.mark.parametrize("name", ["tie", "label_edges", "big", "c_att0"])
def test_built_cases_agree_with_torch_autograd(name):
    _against_torch(*Cf.built_case(name))


@pytest.mark.parametrize("C", Cf.CHANNELS)
def test_three_dimensional_layout_agrees_with_torch_on_the_transposed_logits(C):
    """Upstream hands cross_entropy wts.transpose(1, 2) [B,A,C] with rlabel [B,C]: the same rows as [B C, A]."""
    logits, label, wts, rlabel = Cf.layout_case(C)
    lab = Cf.expand_rlabel(wts, rlabel)
    assert lab.shape == (4, C) and (C <= 60 or np.array_equal(lab[:, 60:], rlabel[:, :C - 60]))
    tw = torch.from_numpy(wts).double().requires_grad_()
    r = torch.nn.functional.cross_entropy(tw.transpose(1, 2), torch.from_numpy(np.ascontiguousarray(lab)).long())
    r.backward()
    fwd = Cf.forward(logits, label, wts, lab, (0.0, 1.0))
    assert _close(fwd["att_row_ce"].mean(), r.item()) and fwd["att_preds"].shape == (4, C)
    assert _close(Cf.backward(1.0, logits, label, wts, lab, (0.0, 1.0))[1], tw.grad.numpy())
    _against_torch(logits, label, wts, lab, (0.75, 1.25))


def test_upstream_gradient_scales_the_restatement():
    _against_torch(*Cf.case(*Cf.CASES[12]), g=-2.5)


# ----------------------------------------------------------------------------------------------- restatement vs the reference
@pytest.mark.parametrize("key", "abc")
def test_restatement_agrees_with_the_reference(key):
    g = golden("cls_loss.npz")
    pred, label, wts, rlabel = Cf.golden_inputs(key)
    for name, arr in (("pred", pred), ("label", label), ("wts", wts), ("rlabel", rlabel)):
        assert np.array_equal(g[f"{key}_{name}"], arr), name
    fwd_err, grad_err = float(g["fwd_err"]), float(g["grad_err"])
    lab2 = Cf.expand_rlabel(wts, rlabel) if wts.ndim == 3 else rlabel
    ref = Cf.forward(pred, label)
    assert abs(ref["scalars"][1] - g[f"{key}_ce"][0]) <= fwd_err + _slack(g[f"{key}_ce"][:1]) and np.float32(ref["scalars"][3]) == g[f"{key}_ce"][1]
    assert np.abs(Cf.backward(1.0, pred, label)[0] - g[f"{key}_ce_dpred"]).max() <= grad_err + _slack(g[f"{key}_ce_dpred"])
    for loss_type, m in Cf.GOLDEN_TYPES:
        for counter in Cf.GOLDEN_COUNTERS:
            tag = f"{key}_{loss_type}_{counter}"
            coef = Cf.schedule_coefficients(loss_type, m, counter)
            fwd = Cf.forward(pred, label, wts, lab2, coef)
            dpred, dwts = Cf.backward(1.0, pred, label, wts, lab2, coef)
            e_f = np.abs(fwd["scalars"][:3] - g[f"{tag}_out"][:3]).max()
            e_g = max(np.abs(dpred - g[f"{tag}_dpred"]).max(), np.abs(dwts - g[f"{tag}_dwts"]).max())
            print(f"{tag}: |scalars - golden| {e_f:.3e} (stored {fwd_err:.3e}), |grad - golden| {e_g:.3e} (stored {grad_err:.3e})")
            assert e_f <= fwd_err + _slack(g[f"{tag}_out"][:3]) and e_g <= grad_err + _slack(g[f"{tag}_dpred"])
            assert np.array_equal(fwd["scalars"][3:].astype(np.float32), g[f"{tag}_out"][3:]) and int(g[f"{tag}_counter"]) == counter + 1
    # the comparison says something: a few fp32 roundings of the largest scalar, and gradients far above the tolerance
    assert fwd_err <= 8 * 2.0 ** -24 * max(np.abs(g[f"{k}_schedule_0_out"]).max() for k in "abc")
    assert np.abs(g[f"{key}_default_0_dpred"]).max() > 1e4 * grad_err and np.abs(g[f"{key}_default_0_dwts"]).max() > 1e4 * grad_err


def test_fixture_holds_arrays_only():
    g = golden("cls_loss.npz")                                 # allow_pickle=False
    assert all(g[k].dtype.kind in "fi" for k in g.files)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "cls_loss.npz")) < 768 * 1024
    assert g["a_wts"].shape == (6, 60) and g["b_wts"].shape == (6, 40, 60) and g["c_wts"].shape == (3, 70, 12)


# ----------------------------------------------------------------------------------------------- properties of the restatement
def test_a_row_is_invariant_under_a_shift():
    logits, label, att, att_label, coef = Cf.case(5, 40, 5, 60, 7001)
    a, b = Cf.rows_forward(logits, label), Cf.rows_forward(logits.astype(np.float64) + 3.0, label)
    assert _close(a[0], b[0], rel=1e-13) and np.array_equal(a[1], b[1])
    assert _close(Cf.rows_backward(0.2, logits, label), Cf.rows_backward(0.2, logits.astype(np.float64) - 7.0, label), rel=1e-13)


@pytest.mark.parametrize("name", Cf.BUILT)
def test_gradient_rows_sum_to_zero_and_flagged_rows_count_as_zero(name):
    logits, label, att, att_label, coef = Cf.built_case(name)
    fwd = Cf.forward(logits, label, att, att_label, coef)
    for d, fl, ce in zip(Cf.backward(1.0, logits, label, att, att_label, coef), (fwd["row_flags"], fwd["att_row_flags"]),
                         (fwd["row_ce"], fwd["att_row_ce"])):
        live = fl == 0
        assert np.abs(d[live].sum(axis=1)).max() <= 1e-15
        assert not d[(fl & 1) != 0].any() and not ce[(fl & 1) != 0].any()
        assert np.isnan(d[fl == 2]).all() and np.isnan(ce[fl == 2]).all()
    if name == "bad":
        assert fwd["row_flags"].tolist() == [0, 1, 0, 1, 1, 0] and fwd["att_row_flags"].tolist() == [1, 0, 0, 0, 0, 1]
        keep = fwd["row_flags"] == 0
        assert _close(fwd["scalars"][1], Cf.rows_forward(logits[keep], label[keep])[0].astype(np.float32).astype(np.float64).sum() / 6,
                      rel=1e-15)                                 # the divisor stays B
    if name == "nonfinite":
        assert fwd["row_flags"].tolist() == [0, 0, 2, 0, 3, 0] and fwd["att_row_flags"].tolist() == [0, 0, 0, 2, 0, 2]
        assert fwd["preds"][2] == fwd["preds"][4] == -1 and fwd["row_ce"][4] == 0 and np.isnan(fwd["scalars"][:3]).all()
    if name == "tie":
        assert fwd["preds"][:3].tolist() == [0, 13, 22] and fwd["att_preds"][1:3].tolist() == [30, 0]
    if name == "big":
        assert np.isfinite(fwd["scalars"]).all() and fwd["row_ce"][0] == 0 and fwd["row_ce"][1] == 2e4
    if name == "c_att0":
        assert not Cf.backward(1.0, logits, label, att, att_label, coef)[1].any() and fwd["scalars"][0] == fwd["scalars"][1]


def test_cases_are_unambiguous():
    """What the one-ulp bound of test_gpu_cls_loss.py rests on: gaps at the maximum of at least GAP (or exact ties, built), labels
    in range, and a class probability at the label far enough from 1 for the gradient's subtraction (1 - p >= 1e-6 wherever the
    row has more than one class: fp64's 1e-16 on p is then 1e-10 relative on p - 1, against fp32's 6e-8)."""
    assert {(c[0], c[1]) for c in Cf.CASES} == {(r, n) for r in Cf.ROWS for n in Cf.WIDTHS}
    assert {c[3] for c in Cf.CASES if c[2]} == set(Cf.WIDTHS) and {c[2] for c in Cf.CASES} == set(Cf.ROWS) | {0}
    for c in Cf.CASES:
        logits, label, att, att_label, coef = Cf.case(*c)
        for x, lab in ((logits, label), (att, att_label)):
            if x is None:
                continue
            assert x.dtype == np.float32 and lab.dtype == np.int32 and (Cf.top_gap(x) >= Cf.GAP).all()
            assert (0 <= lab).all() and (lab < x.shape[1]).all()
            p = np.exp(-Cf.rows_forward(x, lab)[0])
            assert x.shape[1] == 1 or (1 - p >= 1e-6).all()


def test_tally_tables_sum_to_the_rows_seen():
    rng = np.random.default_rng(5)
    k, A, tables = 7, 12, None
    for n in (33, 9):
        preds, label = rng.integers(0, k, n).astype(np.int32), rng.integers(0, k, n).astype(np.int32)
        att_preds, att_label = rng.integers(0, A, n).astype(np.int32), rng.integers(0, A, n).astype(np.int32)
        flags, att_flags = (rng.random(n) < 0.2).astype(np.int32), 2 * (rng.random(n) < 0.1).astype(np.int32)
        preds[flags != 0] = -1
        tables = Cf.tally(preds, label, flags, k, att_preds, att_flags, att_label, A, tables)
    confusion, anchor_table, totals = tables
    assert confusion.sum() == anchor_table.sum() == totals[0] and totals[0] + totals[3] == 42 and totals[3] > 0
    assert np.trace(confusion) == totals[1] and 0 < totals[2] < totals[0]
    assert np.array_equal(confusion.sum(axis=1), anchor_table.sum(axis=1))


# ----------------------------------------------------------------------------------------------- the layers
def test_entries_are_declared_exported_and_bound(vgtk_alias):
    from epn_pointcloud_amd import _lib, classification, losses, models
    header = open(os.path.join(ROOT, "include", "epn_so3conv.h")).read()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.EXPORTS and hasattr(cdll, name) and getattr(_lib.get_lib(), name)
    par = inspect.signature(losses.classification_loss).parameters
    assert list(par) == ["logits", "label", "attention", "attention_label", "coef"]
    assert (par["attention"].default, par["attention_label"].default, par["coef"].default) == (None, None, (1.0, 1.0))
    assert losses.ClsLossResult._fields == ("loss", "cls_loss", "att_loss", "acc", "att_acc", "preds", "att_preds", "row_ce",
                                            "att_row_ce", "row_flags", "att_row_flags")
    par = inspect.signature(losses.classification_tally).parameters
    assert list(par)[:3] == ["result", "label", "tables"] and all(p.default is None for p in list(par.values())[3:])
    assert list(inspect.signature(losses.ClassificationTables.__init__).parameters) == ["self", "k", "A", "device"]
    assert losses.ClassificationTally._fields[:5] == ("instance_acc", "class_acc", "attention_acc", "confusion", "anchor_table")
    par = inspect.signature(models.ClsSO3ConvModel.classify).parameters
    assert list(par) == ["self", "pc", "batch"] and par["batch"].kind is inspect.Parameter.KEYWORD_ONLY and par["batch"].default == 32
    par = inspect.signature(classification.evaluate_classification).parameters
    assert list(par) == ["model", "clouds", "labels", "r_labels", "batch", "loss", "pretrain_step"]
    assert par["batch"].kind is par["loss"].kind is par["pretrain_step"].kind is inspect.Parameter.KEYWORD_ONLY
    assert par["r_labels"].default is None and par["pretrain_step"].default == 2000
    import epn_pointcloud_amd
    assert epn_pointcloud_amd.evaluate_classification is classification.evaluate_classification


def test_mirror_classes_signatures_counter_and_schedule(vgtk_alias):
    import vgtk
    from vgtk.loss import AttentionCrossEntropyLoss, CrossEntropyLoss
    from epn_pointcloud_amd.vgtk import loss as mirror
    assert vgtk.AttentionCrossEntropyLoss is AttentionCrossEntropyLoss is mirror.AttentionCrossEntropyLoss
    assert vgtk.CrossEntropyLoss is CrossEntropyLoss is mirror.CrossEntropyLoss
    assert list(inspect.signature(CrossEntropyLoss.__init__).parameters) == ["self"]
    assert list(inspect.signature(CrossEntropyLoss.forward).parameters) == ["self", "pred", "label"]
    assert list(inspect.signature(AttentionCrossEntropyLoss.__init__).parameters) == ["self", "loss_type", "loss_margin"]
    par = inspect.signature(AttentionCrossEntropyLoss.forward).parameters
    assert list(par) == ["self", "pred", "label", "wts", "rlabel", "pretrain_step"] and par["pretrain_step"].default == 2000
    crit = AttentionCrossEntropyLoss("schedule", 0.5)
    assert (crit.loss_type, crit.loss_margin, crit.iter_counter, crit.training) == ("schedule", 0.5, 0, True)
    for counter, want in ((0, (0.0, 1.5)), (1000, (0.5, 1.0)), (2500, (1.0, 0.5))):
        crit.iter_counter = counter
        assert crit.coefficients() == want == Cf.schedule_coefficients("schedule", 0.5, counter)
        buf = crit.update_schedule("cpu")                     # the weights are read BEFORE the counter advances
        assert buf.dtype == torch.float32 and buf.tolist() == list(want) and crit.iter_counter == counter + 1
    assert crit.update_schedule("cpu", pretrain_step=5002).tolist() == [0.5, 1.0] and crit.update_schedule("cpu") is buf
    # one buffer per device, for good, however the device is spelled; None is the buffer that exists
    assert crit.update_schedule(torch.device("cpu")) is buf and crit.update_schedule() is buf and crit.update_schedule(None, 10) is buf
    with pytest.raises(RuntimeError, match="first call"):
        AttentionCrossEntropyLoss("schedule", 0.5).update_schedule()
    assert list(inspect.signature(AttentionCrossEntropyLoss.update_schedule).parameters) == ["self", "device", "pretrain_step"]
    crit.eval()
    crit.iter_counter = 1000
    assert crit.update_schedule("cpu").tolist() == [0.5, 1.0] and crit.iter_counter == 1000      # counts training steps only
    assert AttentionCrossEntropyLoss("default", 0.25).coefficients() == (1.0, 0.25)
    assert AttentionCrossEntropyLoss("no_reg", 0.25).coefficients() == (1.0, 0.0)
    pred, label, wts, rlabel = torch.zeros(2, 40), torch.zeros(2, dtype=torch.int64), torch.zeros(2, 60), torch.zeros(2, dtype=torch.int64)
    bad = AttentionCrossEntropyLoss("no_cls", 1.0)            # constructs, as upstream; refused in forward
    with pytest.raises(NotImplementedError, match="no_cls is not Implemented"):
        bad(pred, label, wts, rlabel)
    for c in (AttentionCrossEntropyLoss("default", 1.0), CrossEntropyLoss()):
        with pytest.raises(RuntimeError, match="CUDA"):         # no CPU fallback
            c(pred, label, wts, rlabel) if isinstance(c, AttentionCrossEntropyLoss) else c(pred, label)
    assert bad.iter_counter == 0


# ----------------------------------------------------------------------------------------------- refusals of the wrappers
def test_classification_loss_refusals():
    from epn_pointcloud_amd import losses
    logits, label = torch.zeros(3, 40), torch.zeros(3, dtype=torch.int64)
    att, att_label = torch.zeros(3, 60), torch.zeros(3, dtype=torch.int64)
    good = dict(logits=logits, label=label, attention=att, attention_label=att_label)
    for key in good:
        with pytest.raises(TypeError, match=key):
            losses.classification_loss(**{**good, key: good[key].numpy()})
    for bad in (dict(attention=None), dict(attention_label=None), dict(coef=1.0), dict(coef=(1.0,)), dict(coef=("a", 1.0)),
                dict(coef=np.ones(2, np.float32))):
        with pytest.raises(TypeError):
            losses.classification_loss(**{**good, **bad})
    for bad in (dict(logits=torch.zeros(3, 40, 1)), dict(logits=torch.zeros(40)), dict(logits=torch.zeros(3, 0)), dict(logits=torch.zeros(3, 4097)),
                dict(logits=torch.zeros(0, 40), label=label[:0]), dict(label=label[:2]), dict(label=label[:, None]),
                dict(attention=torch.zeros(2, 60)), dict(attention=torch.zeros(3, 2, 3, 60)), dict(attention=torch.zeros(3, 0)),
                dict(attention=torch.zeros(3, 4097)), dict(attention_label=att_label[:2]), dict(attention_label=torch.zeros(3, 2, dtype=torch.int64)),
                dict(attention=torch.zeros(3, 5, 60)), dict(attention=torch.zeros(3, 0, 60), attention_label=torch.zeros(3, 0, dtype=torch.int64)),
                dict(coef=torch.ones(3)), dict(coef=torch.ones(2, 1)), dict(coef=torch.ones(4)[::2]), dict(coef=torch.ones(2, 2)[:, 0]), dict(coef=(float("nan"), 1.0)), dict(coef=(1.0, float("inf"))),
                dict(label=label + 40), dict(label=label - 1), dict(label=label - 100), dict(attention_label=att_label + 60),
                dict(attention_label=att_label - 1)):
        with pytest.raises(ValueError):
            losses.classification_loss(**{**good, **bad})
    with pytest.raises(ValueError, match="65536"):
        losses.classification_loss(logits, label, torch.zeros(3, 21846, 1).expand(3, 21846, 2), torch.zeros(3, 21846, dtype=torch.int64))
    for bad in (dict(logits=logits.int()), dict(attention=att.long()), dict(label=label.float()), dict(label=label.to(torch.int16)),
                dict(attention_label=att_label.bool()), dict(coef=torch.ones(2, dtype=torch.float64))):
        with pytest.raises(TypeError):
            losses.classification_loss(**{**good, **bad})
    with pytest.raises(ValueError):                             # shape comes before dtype
        losses.classification_loss(logits.int(), label[:2], att, att_label)
    with pytest.raises(TypeError):                              # dtype comes before the device
        losses.classification_loss(logits, label.float(), att, att_label)
    for kw in (good, dict(logits=logits, label=label), dict(good, label=label.int()), dict(good, coef=torch.ones(2))):
        with pytest.raises(RuntimeError, match="CUDA"):         # no CPU fallback
            losses.classification_loss(**kw)


def test_tally_tables_and_evaluation_refusals():
    from epn_pointcloud_amd import classification, losses, models
    for k, A in ((0, 0), (4097, 0), (40, -1), (40, 4097)):
        with pytest.raises(ValueError):
            losses.ClassificationTables(k, A)
    with pytest.raises(RuntimeError, match="CUDA"):
        losses.ClassificationTables(40, 60, "cpu")
    with pytest.raises(TypeError, match="ClsLossResult"):
        losses.classification_tally((1, 2), torch.zeros(2, dtype=torch.int64), None)
    r = losses.ClsLossResult(*[torch.zeros(())] * 5, torch.zeros(2, dtype=torch.int32), None, torch.zeros(2), None,
                             torch.zeros(2, dtype=torch.int32), None)
    with pytest.raises(TypeError, match="label"):
        losses.classification_tally(r, [0, 1], None)
    with pytest.raises(TypeError, match="ClassificationTables"):
        losses.classification_tally(r, torch.zeros(2, dtype=torch.int64), None)
    from test_models_cpu import product_model
    m = product_model("cls")
    assert isinstance(m, models.ClsSO3ConvModel) and m.training
    # whether the head's second output is attention is read from its pooling mode, never guessed from a shape: a 'max' head's
    # squeezed feature map of one cloud with one point left is 2-d as well
    from test_models_cpu import tiny_layers
    plain = models.ClsSO3ConvModel(tiny_layers("cls"), out_mlps=(32,), pooling="max")
    assert classification._attention_of(plain, torch.zeros(1, 40), torch.zeros(32, 60)) is None
    assert classification._attention_of(m, torch.zeros(1, 40), torch.zeros(60)).shape == (1, 60)
    assert classification._attention_of(m, torch.zeros(3, 40), torch.zeros(3, 60)).shape == (3, 60)
    pc = torch.zeros(2, 64, 3)
    with pytest.raises(RuntimeError, match="eval"):
        m.classify(pc)
    with pytest.raises(RuntimeError, match="eval"):
        classification.evaluate_classification(m, pc, torch.zeros(2, dtype=torch.int64))
    m.eval()
    for bad, err in ((pc.numpy(), TypeError), (pc[0], ValueError), (torch.zeros(2, 64, 2), ValueError), (pc.double(), TypeError)):
        with pytest.raises(err):
            m.classify(bad)
    with pytest.raises(ValueError, match="batch"):
        m.classify(pc, batch=0)
    with pytest.raises(RuntimeError, match="CUDA"):
        m.classify(pc)
    out = m.classify(pc[:0])                                  # no cloud: empty results without a launch
    assert out[0].shape == (0, 40) and out[1].shape == out[2].shape == (0,) and out[1].dtype == out[2].dtype == torch.int32
    lab = torch.zeros(2, dtype=torch.int64)
    for kw, err in ((dict(labels=lab[:1]), ValueError), (dict(labels=lab.float()), TypeError), (dict(labels=[0, 0]), TypeError),
                    (dict(r_labels=lab[:1]), ValueError), (dict(r_labels=lab.float()), TypeError)):
        with pytest.raises(err):
            classification.evaluate_classification(m, **{**dict(clouds=pc, labels=lab), **kw})
    with pytest.raises(ValueError, match="at least one"):
        classification.evaluate_classification(m, pc[:0], lab[:0])
    with pytest.raises(RuntimeError, match="CUDA"):
        classification.evaluate_classification(m, pc, lab)


# ----------------------------------------------------------------------------------------------- refusals of the C entries
def _vp(v):
    return ctypes.c_void_p(v) if v else None


_FWD = dict(logits=16, label=16, B=6, k=40, att=16, att_label=16, R=6, A=60, coef=16, row_ce=16, pred=16, flags=16, att_row_ce=16,
            att_pred=16, att_flags=16, scalars=16)
_BWD = dict(upstream=16, logits=16, label=16, flags=16, B=6, k=40, att=16, att_label=16, att_flags=16, R=6, A=60, coef=16, dlogits=16,
            datt=16)
_TALLY = dict(pred=16, label=16, flags=16, att_pred=16, att_label=16, att_flags=16, B=6, k=40, A=60, confusion=16, anchor_table=16,
              totals=16)
_INTS = ("B", "k", "R", "A")


def _call(entry, base, over):
    """Pointers: non-NULL and never dereferenced (every call is refused before the first HIP runtime call)."""
    from epn_pointcloud_amd import _lib
    a = dict(base, **over)
    return getattr(_lib.get_lib(), entry)(*[a[n] if n in _INTS else _vp(a[n]) for n in base], None)


def _fwd(**over):
    return _call("epn_cls_loss_f32", _FWD, over)


def _bwd(**over):
    return _call("epn_cls_loss_bwd_f32", _BWD, over)


def _tally(**over):
    return _call("epn_cls_tally_i32", _TALLY, over)


_ids = dict(ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))


@pytest.mark.parametrize("bad", [dict(B=0), dict(B=-1), dict(B=65537), dict(k=0), dict(k=4097), dict(k=-2), dict(R=-1), dict(R=65537),
                                 dict(A=0), dict(A=4097), dict(A=-1)], **_ids)
def test_loss_entries_refuse_sizes(bad):
    assert _fwd(**bad) == EINVAL and _bwd(**bad) == EINVAL
    assert _fwd(**bad, logits=0) == EINVAL and _bwd(**bad, upstream=0) == EINVAL              # sizes before pointers


@pytest.mark.parametrize("bad", [dict(B=0), dict(B=-1), dict(B=65537), dict(k=0), dict(k=4097), dict(A=0), dict(A=4097)], **_ids)
def test_tally_entry_refuses_sizes(bad):
    assert _tally(**bad) == EINVAL and _tally(**bad, totals=0) == EINVAL


@pytest.mark.parametrize("name", sorted(n for n in set(_FWD) | set(_BWD) | set(_TALLY) if n not in _INTS))
def test_entries_refuse_null(name):
    if name in _FWD:
        assert _fwd(**{name: 0}) == ENULL
    if name in _BWD:
        assert _bwd(**{name: 0}) == ENULL
    if name in _TALLY and name not in ("att_pred", "att_label"):
        assert _tally(**{name: 0}) == ENULL


def test_the_attention_set_is_optional_as_a_whole():
    """R = 0: the attention pointers and A are not looked at (the remaining checks hold); the tally without att_pred ignores
    A, att_label, att_flags and the anchor table.  Nothing is launched: every call here is still refused for another reason."""
    none = dict(att=0, att_label=0, att_row_ce=0, att_pred=0, att_flags=0)
    assert _fwd(R=0, A=0, scalars=0, **none) == ENULL and _fwd(R=0, A=-5, B=0, **none) == EINVAL
    assert _bwd(R=0, A=0, att=0, att_label=0, att_flags=0, datt=0, dlogits=0) == ENULL
    assert _tally(att_pred=0, att_label=0, att_flags=0, anchor_table=0, A=0, totals=0) == ENULL
    assert _tally(att_pred=0, A=-1, B=0) == EINVAL
