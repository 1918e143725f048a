"""The rotation network's training loss without a GPU: the numpy fp64 restatement (tests/rotation_loss_ref.py) against torch's CPU
fp64 autograd over a torch restatement of the reference's alignment branch (vgtk/vgtk/loss.py:140-181, written below) and
against the reference's own results (tests/golden/rotation_loss.npz, gen_golden_rotation_loss.py); the entries at every layer;
every refusal, decided on the host; the condition test_gpu_rotation_loss.py's tolerances rest on, for every case of the table.

Tolerances.
  torch fp64   both sides are fp64 evaluations of the same formulas: 1e-12 relative to the largest magnitude of the compared
               array plus 1e-13 (a few hundred fp64 roundings; the clamped Jacobians reach 1e16, hence relative).
  golden       the reference works in fp32.  The fixture stores the largest difference between its results and the restatement,
               measured when it was written (fwd_err, grad_err); the tests allow FACTOR = 2 times that, read from the fixture:
               the restatement here may differ from the run that measured it by the libm and the summation order of numpy."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, golden
import rotation_loss_ref as Lf

EINVAL, ENULL = -1, -3
ENTRIES = ("epn_rotation_loss_f32", "epn_rotation_loss_bwd_f32")
FACTOR = 2.0


# ----------------------------------------------------------------------------------------------- torch restatement of loss.py:140-181
def _normalize(v):
    mag = torch.max(torch.sqrt(v.pow(2).sum(1)), torch.tensor([1e-8], dtype=v.dtype, device=v.device))
    return v / mag[:, None]


def quaternion_map(q):
    q = _normalize(q)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return torch.stack((1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * z * w, 2 * x * z + 2 * y * w,
                        2 * x * y + 2 * z * w, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * x * w,
                        2 * x * z - 2 * y * w, 2 * y * z + 2 * x * w, 1 - 2 * x * x - 2 * y * y), 1).view(-1, 3, 3)


def ortho6d_map(v):
    x = _normalize(v[:, 0:3])
    z = _normalize(torch.cross(x, v[:, 3:6], dim=1))
    y = torch.cross(z, x, dim=1)
    return torch.stack((x, y, z), 2)


def torch_loss(wts, label, y, gt_R, w):
    """The loss terms of the alignment branch -> (loss, cls_loss, w * l2_loss, r_acc), in the dtype of the inputs."""
    b, nr, na = y.shape[0], y.shape[1], y.shape[2]
    cls_loss = torch.nn.functional.cross_entropy(wts, label.long())
    preds = wts.max(1)[1]
    r_acc = (preds.reshape(-1) == label.reshape(-1)).sum().to(wts.dtype) / float(label.numel())
    y_rs = y.transpose(1, 3).contiguous().view(b * na, na, nr)                # batched_select_anchor, loss.py:77-92
    y_select = torch.gather(y_rs, 1, label.long().view(-1, 1, 1).expand(-1, 1, nr)).view(b * na, nr)
    select_R = (quaternion_map if nr == 4 else ortho6d_map)(y_select).view(b, na, 3, 3)
    l2_loss = torch.pow(gt_R - select_R, 2).mean()
    return cls_loss + w * l2_loss, cls_loss, w * l2_loss, r_acc


def _close(got, ref, rel=1e-12):
    return np.abs(np.asarray(got) - np.asarray(ref)).max() <= rel * np.abs(ref).max() + 1e-13


def _against_torch(wts, y, label, R_target, fwd, bwd, g=Lf.UPSTREAM):
    tw = torch.from_numpy(wts).double().requires_grad_()
    ty = torch.from_numpy(y).double().requires_grad_()
    out = torch_loss(tw, torch.from_numpy(label), ty, torch.from_numpy(R_target).double(), Lf.W)
    (g * out[0]).backward()
    n = label.size
    cls, reg = fwd["row_ce"].sum() / n, Lf.W * fwd["row_l2"].sum() / (9 * n)      # the unrounded rows: what torch sums
    assert _close([cls + reg, cls, reg, fwd["scalars"][3]], [o.item() for o in out])
    assert _close(bwd[0], tw.grad.numpy()) and _close(bwd[1], ty.grad.numpy())
    assert (bwd[2] >= np.abs(bwd[0])).all() and (bwd[3] >= np.abs(bwd[1]) * (1 - 1e-9)).all()   # magnitudes bound values


@pytest.mark.parametrize("case", [c for c in Lf.CASES if c[1] <= 5], ids=str)
def test_restatement_agrees_with_torch_autograd(case):
    wts, y, label, R_target, _, _, fwd, bwd = Lf.case(*case)
    _against_torch(wts, y, label, R_target, fwd, bwd)


@pytest.mark.parametrize("name", ["tie", "clamp4", "clamp6_tiny", "clamp6_cross", "big", "huge"])
def test_built_cases_agree_with_torch_autograd(name):
    wts, y, label, R_target, fwd, bwd = Lf.built_case(name)
    _against_torch(wts, y, label, R_target, fwd, bwd)


def test_autograd_has_no_gradient_at_a_zero_norm_and_the_specification_does():
    """Row (1, 4) of "clamp6" has a zero first triple.  autograd's backward of sqrt at 0 is 0 * inf: the reference's gradient of
    that row is NaN.  The specification's clamped Jacobian is finite there; every other row agrees with autograd."""
    wts, y, label, R_target, fwd, (dwts, dy, _, _) = Lf.built_case("clamp6")
    ty = torch.from_numpy(y).double().requires_grad_()
    torch_loss(torch.from_numpy(wts).double(), torch.from_numpy(label), ty, torch.from_numpy(R_target).double(), Lf.W)[0].backward()
    got = ty.grad.numpy()
    row = (1, slice(None), label[1, 4], 4)
    assert np.isnan(got[row][:3]).all() and np.isfinite(dy).all() and np.abs(dy[row]).max() > 1e3
    got[row] = dy[row]
    assert _close(dy, got)


def test_upstream_gradient_scales_the_restatement():
    wts, y, label, R_target, _, _, fwd, _ = Lf.case(*Lf.CASES[8])
    _against_torch(wts, y, label, R_target, fwd, Lf.backward(-2.5, wts, y, label, R_target, fwd), g=-2.5)


# ----------------------------------------------------------------------------------------------- restatement vs the reference
@pytest.mark.parametrize("nr,key", [(4, "q"), (6, "o")])
def test_restatement_agrees_with_the_reference(nr, key):
    g = golden("rotation_loss.npz")
    wts, y, label, R_target, anchors, T = Lf.golden_inputs(nr)
    for name, arr in (("wts", wts), ("y", y), ("label", label), ("R_target", R_target), ("T", T)):
        assert np.array_equal(g[f"{key}_{name}"], arr), name
    assert np.array_equal(g["anchors"], anchors) and float(g["w"]) == Lf.W
    fwd, (dwts, dy, _, _) = Lf.evaluate(wts, y, label, R_target)
    fwd_err, grad_err = float(g["fwd_err"]), float(g["grad_err"])
    e_f = np.abs(fwd["scalars"][:3] - g[f"{key}_out"][:3]).max()
    e_g = max(np.abs(dwts - g[f"{key}_dwts"]).max(), np.abs(dy - g[f"{key}_dy"]).max())
    print(f"nr = {nr}: |scalars - golden| {e_f:.3e} (stored {fwd_err:.3e}), |grad - golden| {e_g:.3e} (stored {grad_err:.3e})")
    assert e_f <= FACTOR * fwd_err and e_g <= FACTOR * grad_err
    assert np.float32(fwd["scalars"][3]) == g[f"{key}_out"][3]
    # the comparison says something: one fp32 rounding of the largest scalar, and gradients far above the tolerance
    assert fwd_err <= 4 * 2.0 ** -24 * np.abs(g[f"{key}_out"]).max()
    assert np.abs(g[f"{key}_dy"]).max() > 1e5 * grad_err and np.abs(g[f"{key}_dwts"]).max() > 1e4 * grad_err


def test_fixture_holds_arrays_only():
    g = golden("rotation_loss.npz")                            # allow_pickle=False
    assert all(g[k].dtype.kind in "fi" for k in g.files)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "rotation_loss.npz")) < 512 * 1024


# ----------------------------------------------------------------------------------------------- the case tables
def test_case_table_covers_the_shapes_and_needed_no_reseeding():
    assert {c[:3] for c in Lf.CASES} == ({(A, b, nr) for A in (1, 12, 60, 64) for b in (1, 3, 65) for nr in (4, 6)} |
                                         {(60, 5, 4), (60, 5, 6)})
    assert len({c[3] for c in Lf.CASES}) == len(Lf.CASES)
    assert Lf.RESEEDED == 0 and [c[3] for c in Lf.CASES[:24]] == [500 + 20 * i + 2 * j + k for i in range(4) for j in range(3)
                                                                  for k in range(2)]


@pytest.mark.parametrize("case", Lf.CASES, ids=str)
def test_cases_have_no_tie_at_the_maximum(case):
    """The one condition the GPU tolerances rest on (case() asserts it too); and what the magnitudes assume: labels in range,
    finite values, rotation maps whose conditioning stays below 1e4, no clamped norm."""
    A, b, nr, _ = case
    wts, y, label, R_target, anchors, T, fwd, bwd = Lf.case(*case)
    assert wts.shape == (b, A, A) and y.shape == (b, nr, A, A) and R_target.shape == (b, A, 3, 3) and R_target.dtype == np.float32
    assert Lf.no_top_tie(wts)
    assert not fwd["row_flags"].any() and fwd["cond"].max() < 1e4
    assert all(np.isfinite(x).all() for x in (fwd["row_ce"], fwd["row_l2"], fwd["sel_R"]) + bwd)
    assert ((fwd["row_ce"] > 0) | (A == 1)).all() and np.abs(fwd["sel_R"]).max() <= 1 + 1e-12


def test_built_cases_are_what_they_claim():
    wts, y, label, R_target, fwd, bwd = Lf.built_case("tie")
    assert wts[1, 3, 5] == wts[1, 7, 5] == wts[1, :, 5].max() and fwd["preds"][1, 5] == 3
    wts, y, label, R_target, fwd, (dwts, dy, _, _) = Lf.built_case("bad")
    assert label[0, 2] == -1 and label[2, 11] == 12
    for p, a in ((0, 2), (2, 11)):
        assert fwd["row_flags"][p, a] == Lf.FLAG_BAD_LABEL and fwd["row_ce"][p, a] == 0 and fwd["row_l2"][p, a] == 0
        assert not fwd["sel_R"][p, a].any() and not dwts[p, :, a].any() and not dy[p, :, :, a].any()
    assert (fwd["row_flags"] != 0).sum() == 2 and np.count_nonzero(dwts) == dwts.size - 2 * 12
    for name, nr, clamped in (("clamp4", 4, (True, True)), ("clamp6", 6, (True, True)), ("clamp6_tiny", 6, (True, False)),
                              ("clamp6_cross", 6, (False, True))):
        wts, y, label, R_target, fwd, (dwts, dy, _, _) = Lf.built_case(name)
        assert y.shape[1] == nr and fwd["row_flags"][1, 4] == Lf.FLAG_NORM_CLAMPED and (fwd["row_flags"] != 0).sum() == 1
        assert tuple(fwd["norms"][1, 4] < 1e-8) == clamped and Lf.no_top_tie(wts)
        assert (name == "clamp6") == (not fwd["norms"][1, 4].any())
        assert np.isfinite(dy).all() and np.abs(dy[1, :, label[1, 4], 4]).max() > 1e3      # the clamped Jacobian is 1 / 1e-8
        assert np.abs(dy).max() < 3e38                                                  # representable in fp32
    for name, size in (("big", 80), ("huge", 100)):
        wts, y, label, R_target, fwd, bwd = Lf.built_case(name)
        assert wts.max() > size and wts.min() < 1 - size and Lf.no_top_tie(wts)
        with np.errstate(over="ignore"):
            assert np.isinf(np.exp(wts).sum(axis=1)).any() == (name == "huge")     # the naive form overflows fp32 at 100
        assert np.isfinite(fwd["row_ce"]).all() and fwd["row_ce"].max() > size and all(np.isfinite(x).all() for x in bwd)


# ----------------------------------------------------------------------------------------------- the layers
def test_entries_are_declared_exported_and_bound(vgtk_alias):
    from epn_pointcloud_amd import _lib, losses
    header = open(os.path.join(ROOT, "include", "epn_so3conv.h")).read()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.EXPORTS and hasattr(cdll, name)
    assert list(inspect.signature(losses.rotation_loss).parameters) == ["confidence", "y", "label", "R_target", "w"]
    assert inspect.signature(losses.rotation_loss).parameters["w"].default == 10.0
    assert losses.RotationLossResult._fields == ("loss", "cls_loss", "reg", "r_acc", "preds", "row_ce", "row_l2", "row_flags")


def test_mirror_class_signature_and_unsupported_branches(vgtk_alias):
    import vgtk
    from vgtk.loss import MultiTaskDetectionLoss
    from epn_pointcloud_amd.vgtk import loss as mirror
    assert vgtk.MultiTaskDetectionLoss is MultiTaskDetectionLoss is mirror.MultiTaskDetectionLoss
    par = inspect.signature(MultiTaskDetectionLoss.__init__).parameters
    assert list(par) == ["self", "anchors", "nr", "w", "threshold"]
    assert (par["nr"].default, par["w"].default, par["threshold"].default) == (4, 10, 1.0)
    par = inspect.signature(MultiTaskDetectionLoss.forward).parameters
    assert list(par) == ["self", "wts", "label", "y", "gt_R", "gt_T"] and par["gt_T"].default is None
    an = torch.eye(3).repeat(12, 1, 1)
    crit = MultiTaskDetectionLoss(an, nr=6, w=3)
    assert (crit.nr, crit.w, crit.threshold, crit.iter_counter) == (6, 3, 1.0, 0) and crit.anchors is an
    with pytest.raises(AssertionError):
        MultiTaskDetectionLoss(an, nr=5)
    wts, y = torch.zeros(2, 12, 12), torch.zeros(2, 6, 12, 12)
    label, gt_R, gt_T = torch.zeros(2, 12, dtype=torch.int64), torch.zeros(2, 12, 3, 3), torch.eye(3).repeat(2, 1, 1)
    with pytest.raises(NotImplementedError, match="single-anchor"):
        crit(torch.zeros(2, 1, 1), label[:, :1], torch.zeros(2, 6, 1, 1), gt_R[:, :1], gt_T)
    with pytest.raises(NotImplementedError, match="canonical"):
        crit(wts, label, y, gt_R)
    with pytest.raises(NotImplementedError, match="canonical"):
        crit(wts[:, :, 0], label[:, 0], y[:, :, :, 0], gt_R, gt_T)
    with pytest.raises(ValueError, match="nr = 6"):
        crit(wts, label, torch.zeros(2, 4, 12, 12), gt_R, gt_T)
    with pytest.raises(RuntimeError, match="CUDA"):             # no CPU fallback
        crit(wts, label, y, gt_R, gt_T)
    assert crit.iter_counter == 0


# ----------------------------------------------------------------------------------------------- refusals of the wrapper
def test_rotation_loss_refusals():
    from epn_pointcloud_amd import losses
    wts, y = torch.zeros(2, 12, 12), torch.zeros(2, 4, 12, 12)
    label, R = torch.zeros(2, 12, dtype=torch.int64), torch.zeros(2, 12, 3, 3)
    good = dict(confidence=wts, y=y, label=label, R_target=R)
    for key in good:
        with pytest.raises(TypeError, match=key):
            losses.rotation_loss(**{**good, key: good[key].numpy()})
    for bad in (dict(confidence=torch.zeros(2, 12, 11)), dict(confidence=torch.zeros(2, 12)), dict(confidence=torch.zeros(2, 65, 65)),
                dict(confidence=torch.zeros(2, 0, 0)), dict(confidence=torch.zeros(0, 12, 12)), dict(y=torch.zeros(2, 5, 12, 12)),
                dict(y=torch.zeros(3, 4, 12, 12)), dict(y=torch.zeros(2, 4, 12)), dict(label=label[:, :11]), dict(label=label[0]),
                dict(R_target=torch.zeros(2, 12, 3, 4)), dict(R_target=torch.zeros(2, 11, 3, 3)), dict(label=label + 12),
                dict(label=label - 1), dict(w=float("nan")), dict(w=float("inf"))):
        with pytest.raises(ValueError):
            losses.rotation_loss(**{**good, **bad})
    for bad in (dict(confidence=wts.int()), dict(y=y.long()), dict(label=label.float()), dict(label=label.to(torch.int16)),
                dict(R_target=R.double())):
        with pytest.raises(TypeError):
            losses.rotation_loss(**{**good, **bad})
    with pytest.raises(ValueError):                             # shape comes before dtype
        losses.rotation_loss(wts, torch.zeros(2, 5, 12, 12, dtype=torch.int32), label, R)
    with pytest.raises(TypeError):                              # dtype comes before device
        losses.rotation_loss(wts, y, label, R.double())
    for lab in (label, label.int()):
        with pytest.raises(RuntimeError, match="CUDA"):         # no CPU fallback
            losses.rotation_loss(wts, y, lab, R)


# ----------------------------------------------------------------------------------------------- refusals of the C entries
def _vp(v):
    return ctypes.c_void_p(v) if v else None


def _fwd(**over):
    """Pointers: non-NULL and never dereferenced (every call is refused, or b = 0)."""
    from epn_pointcloud_amd import _lib
    a = dict(wts=16, y=16, label=16, R_target=16, b=2, A=60, nr=4, w=10.0, row_ce=16, row_l2=16, preds=16, row_flags=16, sel_R=16,
             scalars=16)
    a.update(over)
    return _lib.get_lib().epn_rotation_loss_f32(
        _vp(a["wts"]), _vp(a["y"]), _vp(a["label"]), _vp(a["R_target"]), a["b"], a["A"], a["nr"], a["w"], _vp(a["row_ce"]),
        _vp(a["row_l2"]), _vp(a["preds"]), _vp(a["row_flags"]), _vp(a["sel_R"]), _vp(a["scalars"]), None)


def _bwd(**over):
    from epn_pointcloud_amd import _lib
    a = dict(upstream=16, wts=16, y=16, label=16, R_target=16, row_flags=16, b=2, A=60, nr=4, w=10.0, dwts=16, dy=16)
    a.update(over)
    return _lib.get_lib().epn_rotation_loss_bwd_f32(
        _vp(a["upstream"]), _vp(a["wts"]), _vp(a["y"]), _vp(a["label"]), _vp(a["R_target"]), _vp(a["row_flags"]), a["b"], a["A"],
        a["nr"], a["w"], _vp(a["dwts"]), _vp(a["dy"]), None)


_ids = dict(ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
_FWD_PTRS = ("wts", "y", "label", "R_target", "row_ce", "row_l2", "preds", "row_flags", "sel_R", "scalars")
_BWD_PTRS = ("upstream", "wts", "y", "label", "R_target", "row_flags", "dwts", "dy")


@pytest.mark.parametrize("bad", [dict(b=-1), dict(A=0), dict(A=65), dict(A=-3), dict(nr=3), dict(nr=5), dict(nr=0), dict(nr=9),
                                 dict(w=float("nan")), dict(w=float("inf")), dict(w=float("-inf"))], **_ids)
def test_entries_refuse_sizes(bad):
    assert _fwd(**bad) == EINVAL and _bwd(**bad) == EINVAL


@pytest.mark.parametrize("name", sorted(set(_FWD_PTRS + _BWD_PTRS)))
def test_entries_refuse_null(name):
    if name in _FWD_PTRS:
        assert _fwd(**{name: 0}) == ENULL
    if name in _BWD_PTRS:
        assert _bwd(**{name: 0}) == ENULL


def test_no_pair_is_success_and_launches_nothing():
    assert _fwd(b=0) == 0 and _bwd(b=0) == 0
    assert _fwd(b=0, **dict.fromkeys(_FWD_PTRS, 0)) == 0 and _bwd(b=0, **dict.fromkeys(_BWD_PTRS, 0)) == 0
    assert _fwd(b=0, A=65) == EINVAL and _bwd(b=0, nr=5) == EINVAL and _fwd(b=0, w=float("nan")) == EINVAL   # the other checks hold
    assert _fwd(b=-1, wts=0) == EINVAL and _bwd(A=0, dy=0) == EINVAL                                          # sizes before pointers
