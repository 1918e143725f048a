"""The training loss of the rotation network on the GPU (csrc/rotation_loss.hip behind epn_pointcloud_amd.losses.rotation_loss and
the mirror class vgtk.loss.MultiTaskDetectionLoss) against the numpy fp64 restatement of its specification
(tests/rotation_loss_ref.py).  The case table and the condition the tolerances rest on (no fp32 tie at the maximum of a column of
wts outside the tie case) are asserted on the CPU by test_rotation_loss_spec.py.

Tolerances.  The kernels compute in fp64 and round every output once, so a device value is compared with the restatement's value
ROUNDED to fp32 and may differ from it by
    one fp32 ulp of the reference value  +  k 2^-53 mag
The ulp: the two fp64 values may straddle a rounding boundary.  The second term: both sides form the value from k fp64 operations
on terms whose magnitudes add up to mag (supplied by the restatement), each operation within 2^-53 relative (exp, log, sqrt:
2^-52, counted twice); it matters only where the terms cancel.  k per output, A the number of anchors:
  integers   preds, row_flags: equal.
  row_ce     m + log(s) - w_L.  s: A exp terms (2 each) and A - 1 additions per side, relative to s, i.e. absolute in log(s):
             2 (A + 1) together with the log's own 2 roundings; two more additions.  mag = 1 + |m| + |log s| + |w_L|,
             k = 2 (A + 1) + 8 = 2 A + 10.
  sel_R      at most 24 operations between the y entries and an entry (norm: 7, division, cross products and products: 5 each),
             per side; the Gram-Schmidt form divides by |x cross y2|, which amplifies what came before by cond = 1 + |x||y2| /
             |x cross y2|.  mag = cond max(1, |R|), k = 64.
  row_l2     sum of 9 squares of d = R_target - sel_R: d inherits sel_R's error, the sum adds 9 + 9 roundings of non-negative
             terms.  mag = 2 cond max(1, |R|) sum|d| + row_l2, k = 64.
  scalars    the fp64 sum of the b A ROUNDED rows, divided, rounded once: k = b A + 4 additions on mag = sum|rows| / (b A)
             (times w / 9 for reg).  The device's rounded rows are taken to be the restatement's (a row on the neighbouring fp32
             -- possible where the two fp64 values straddle a boundary, about one row in 10^7 -- would move a scalar by
             2^-23 / (b A) relative).  r_acc is a count over b A: k = 0.
  dwts       g / (b A) (exp(w_t - m) / s - [t == L]): s as above, the subtraction cancels where the softmax is peaked at L.
             mag = |g| / (b A) (p_t + [t == L]), k = 2 A + 10.
  dy         J^T G.  G = coef (sel_R - R_target) carries sel_R's 64 cond 2^-53; J is a product of at most five small matrices
             (normalisations, cross products, the quaternion form), each entry a sum of at most 6 products.  The restatement
             forms the same products with every factor and term in absolute value (Jabs) and mag = Jabs^T coef (cond + |sel_R|
             + |R_target|); k = 256 (64 for G, under 40 per factor of J and per side, with room).
The mirror class's angular error is the decode entry's, held to test_gpu_rotation.py's bound there; here it is compared with
the restatement of the decode within 1e-5 rad and with the reference's fp32 value within 1e-3 rad (torch.svd in fp32 at a
margin near 1e-2 for the noise pair)."""
import ctypes

import numpy as np
import pytest
import torch

import rotation_loss_ref as Lf
import rotation_ref as Rf

pytestmark = pytest.mark.gpu

E53 = 2.0 ** -53


def D(gpu, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def H(t):
    return None if t is None else t.detach().cpu().numpy()


def within(got, ref, k, mag, what=""):
    """|got - fp32(ref)| <= ulp(fp32(ref)) + k 2^-53 mag, elementwise; prints the largest ratio before it decides."""
    got = H(got).astype(np.float64)
    with np.errstate(over="ignore"):
        ref32 = np.asarray(ref).astype(np.float32)
    assert np.isfinite(ref32).all(), what
    err = np.abs(got - ref32.astype(np.float64))
    tol = np.spacing(np.abs(ref32)).astype(np.float64) + k * E53 * np.broadcast_to(mag, err.shape)
    worst = np.unravel_index(np.argmax(err / tol), err.shape) if err.size else ()
    print(f"{what}: largest err / tol {float((err / tol).max()) if err.size else 0:.3f} at {worst}, exact in {float((err == 0).mean()):.4f} of "
          f"{err.size}")
    return bool((err <= tol).all())


def run(gpu, wts, y, label, R_target, w=Lf.W, upstream=None, device_label=True):
    from epn_pointcloud_amd import losses
    tw, ty = D(gpu, wts).requires_grad_(), D(gpu, y).requires_grad_()
    lab = D(gpu, label) if device_label else torch.from_numpy(label)
    r, sel_R = losses.rotation_loss_rows(tw, ty, lab, D(gpu, R_target), w)
    (r.loss if upstream is None else r.loss * upstream).backward()
    return r, sel_R, tw.grad, ty.grad


def check(got, fwd, bwd, A, n, what):
    r, sel_R, gw, gy = got
    assert r.preds.dtype == r.row_flags.dtype == torch.int32 and r.loss.dtype == gw.dtype == gy.dtype == torch.float32
    assert r.loss.dim() == 0 and r.loss.requires_grad and not any(t.requires_grad for t in r[1:]) and not sel_R.requires_grad
    assert np.array_equal(H(r.preds), fwd["preds"]) and np.array_equal(H(r.row_flags), fwd["row_flags"])
    rmax = np.maximum(np.abs(fwd["sel_R"]).max(axis=(2, 3)), 1.0)
    assert within(r.row_ce, fwd["row_ce"], 2 * A + 10, fwd["mag_ce"], what + " row_ce")
    assert within(sel_R, fwd["sel_R"], 64, (fwd["cond"] * rmax)[:, :, None, None], what + " sel_R")
    assert within(r.row_l2, fwd["row_l2"], 64, fwd["mag_l2"], what + " row_l2")
    sc = torch.stack((r.loss, r.cls_loss, r.reg, r.r_acc))
    print(what, "scalars", H(sc), "ref", fwd["scalars"])
    assert within(sc, fwd["scalars"], n + 4, fwd["mag_scalars"], what + " scalars")
    dwts, dy, mag_w, mag_y = bwd
    assert within(gw, dwts, 2 * A + 10, mag_w, what + " dwts") and within(gy, dy, 256, mag_y, what + " dy")


# ----------------------------------------------------------------------------------------------- the table and the built cases
@pytest.mark.parametrize("case", Lf.CASES, ids=str)
def test_rotation_loss(gpu, case):
    A, b, nr, _ = case
    wts, y, label, R_target, _, _, fwd, bwd = Lf.case(*case)
    check(run(gpu, wts, y, label, R_target), fwd, bwd, A, b * A, str(case))


def test_upstream_gradient_scales_the_backward(gpu):
    A, b, nr, _ = case = Lf.CASES[8]
    wts, y, label, R_target, _, _, fwd, _ = Lf.case(*case)
    bwd = Lf.backward(-2.5, wts, y, label, R_target, fwd)
    check(run(gpu, wts, y, label, R_target, upstream=-2.5), fwd, bwd, A, b * A, "upstream -2.5")


def test_ties_go_to_the_lower_target_anchor(gpu):
    wts, y, label, R_target, fwd, bwd = Lf.built_case("tie")
    got = run(gpu, wts, y, label, R_target)
    assert H(got[0].preds)[1, 5] == 3
    check(got, fwd, bwd, 12, 36, "tie")


def test_labels_out_of_range_are_flagged_and_count_as_zero(gpu):
    """label -1 and A, on the device: bit 0, zero rows, zero gradient columns -- and the host check refuses the same label."""
    from epn_pointcloud_amd import losses
    wts, y, label, R_target, fwd, bwd = Lf.built_case("bad")
    got = run(gpu, wts, y, label, R_target)
    check(got, fwd, bwd, 12, 36, "bad")
    r, sel_R, gw, gy = got
    for p, a in ((0, 2), (2, 11)):
        assert H(r.row_flags)[p, a] == Lf.FLAG_BAD_LABEL and H(r.row_ce)[p, a] == 0 and H(r.row_l2)[p, a] == 0
        assert not H(sel_R)[p, a].any() and not H(gw)[p, :, a].any() and not H(gy)[p, :, :, a].any()
    with pytest.raises(ValueError, match="0..11"):
        losses.rotation_loss(D(gpu, wts), D(gpu, y), torch.from_numpy(label), D(gpu, R_target))


@pytest.mark.parametrize("name", ["clamp4", "clamp6", "clamp6_tiny", "clamp6_cross"])
def test_clamped_norms_are_flagged_and_use_the_clamped_jacobian(gpu, name):
    wts, y, label, R_target, fwd, bwd = Lf.built_case(name)
    got = run(gpu, wts, y, label, R_target)
    assert H(got[0].row_flags)[1, 4] == Lf.FLAG_NORM_CLAMPED and torch.isfinite(got[3]).all()
    check(got, fwd, bwd, 12, 36, name)


@pytest.mark.parametrize("name", ["big", "huge"])
def test_large_logits_stay_finite(gpu, name):
    wts, y, label, R_target, fwd, bwd = Lf.built_case(name)
    got = run(gpu, wts, y, label, R_target)
    assert torch.isfinite(got[0].loss) and torch.isfinite(got[0].row_ce).all() and torch.isfinite(got[2]).all()
    check(got, fwd, bwd, 12, 36, name)


def test_host_labels_and_int64_labels_give_the_same_bits(gpu):
    wts, y, label, R_target, _, _, _, _ = Lf.case(*Lf.CASES[9])
    a = run(gpu, wts, y, label, R_target)
    b = run(gpu, wts, y, label.astype(np.int64), R_target)
    c = run(gpu, wts, y, label.astype(np.int64), R_target, device_label=False)
    for other in (b, c):
        assert torch.equal(a[0].loss, other[0].loss) and torch.equal(a[2], other[2]) and torch.equal(a[3], other[3])


def test_channels_last_and_bf16_heads_are_converted_and_get_their_gradient(gpu):
    """y in channels-last memory gives the bits of contiguous y; a bf16 head output gives what its fp32 copy gives, and the
    gradient comes back in the input's dtype and shape."""
    wts, y, label, R_target, _, _, _, _ = Lf.case(*Lf.CASES[8])
    base = run(gpu, wts, y, label, R_target)
    from epn_pointcloud_amd import losses
    ty = D(gpu, y).contiguous(memory_format=torch.channels_last).requires_grad_()
    assert not ty.is_contiguous()
    r = losses.rotation_loss(D(gpu, wts), ty, D(gpu, label), D(gpu, R_target))
    r.loss.backward()
    assert torch.equal(r.loss, base[0].loss) and torch.equal(ty.grad, base[3])
    yb = D(gpu, y).bfloat16().requires_grad_()
    wb = D(gpu, wts).bfloat16().requires_grad_()
    rb = losses.rotation_loss(wb, yb, D(gpu, label), D(gpu, R_target))
    rb.loss.backward()
    y32, w32 = yb.detach().float().requires_grad_(), wb.detach().float().requires_grad_()
    r32 = losses.rotation_loss(w32, y32, D(gpu, label), D(gpu, R_target))
    r32.loss.backward()
    assert torch.equal(rb.loss, r32.loss) and yb.grad.dtype == wb.grad.dtype == torch.bfloat16
    assert torch.equal(yb.grad, y32.grad.bfloat16()) and torch.equal(wb.grad, w32.grad.bfloat16())


# ----------------------------------------------------------------------------------------------- every element is written
def test_every_output_element_is_written_over_a_nan_prefill(gpu):
    """The raw C entries on buffers pre-filled with NaN: no NaN is left in any output, and the bits are those of the wrapper."""
    from epn_pointcloud_amd import _lib
    A, b, nr = 12, 3, 6
    wts, y, label, R_target, fwd, _ = Lf.built_case("bad")          # two rows out of range
    base = run(gpu, wts, y, label, R_target)
    tw, ty, tl, tr = D(gpu, wts), D(gpu, y), D(gpu, label), D(gpu, R_target)
    nan = float("nan")
    f = lambda *s: torch.full(s, nan, device=gpu)
    i = lambda *s: torch.full(s, -7, dtype=torch.int32, device=gpu)
    row_ce, row_l2, sel_R, scalars, preds, flags = f(b, A), f(b, A), f(b, A, 3, 3), f(4), i(b, A), i(b, A)
    dwts, dy, up = f(b, A, A), f(b, nr, A, A), torch.ones(1, device=gpu)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    lib = _lib.get_lib()
    st = _lib.stream_of(tw)
    assert lib.epn_rotation_loss_f32(vp(tw), vp(ty), vp(tl), vp(tr), b, A, nr, Lf.W, vp(row_ce), vp(row_l2), vp(preds), vp(flags),
                                     vp(sel_R), vp(scalars), st) == 0
    assert lib.epn_rotation_loss_bwd_f32(vp(up), vp(tw), vp(ty), vp(tl), vp(tr), vp(flags), b, A, nr, Lf.W, vp(dwts), vp(dy),
                                         _lib.stream_of(tw)) == 0
    torch.cuda.synchronize()
    for t in (row_ce, row_l2, sel_R, scalars, dwts, dy):
        assert not torch.isnan(t).any()
    assert (preds >= 0).all() and (preds < A).all() and (flags >= 0).all()
    r = base[0]
    assert torch.equal(row_ce, r.row_ce) and torch.equal(row_l2, r.row_l2) and torch.equal(sel_R, base[1])
    assert torch.equal(scalars, torch.stack((r.loss, r.cls_loss, r.reg, r.r_acc)).detach())
    assert torch.equal(dwts, base[2]) and torch.equal(dy, base[3])
    assert torch.count_nonzero(dy) == (b * A - 2) * nr            # one target anchor per live row, exact zeros elsewhere


def test_two_runs_are_bitwise_equal(gpu):
    for case in (Lf.CASES[17], Lf.CASES[23]):                        # A = 60, b = 65, nr = 6; A = 64, b = 65, nr = 6
        wts, y, label, R_target = Lf.case(*case)[:4]
        a, b = run(gpu, wts, y, label, R_target), run(gpu, wts, y, label, R_target)
        assert all(torch.equal(x, z) for x, z in zip(a[0], b[0])) and torch.equal(a[1], b[1])
        assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


# ----------------------------------------------------------------------------------------------- next to the decode entry
@pytest.mark.parametrize("case", [Lf.CASES[3], Lf.CASES[10], Lf.CASES[16], Lf.CASES[23]], ids=str)
def test_preds_and_accuracy_are_the_decode_entry_s(gpu, case):
    from epn_pointcloud_amd import alignment
    A, b, nr, _ = case
    wts, y, label, R_target, anchors, T = Lf.case(*case)[:6]
    r = run(gpu, wts, y, label, R_target)[0]
    d = alignment.decode_rotation(D(gpu, wts), D(gpu, y), D(gpu, anchors), D(gpu, label), D(gpu, T))
    assert torch.equal(r.preds, d.preds)
    assert round(r.r_acc.item() * b * A) == int(d.hits.sum().item())
    assert r.r_acc.item() == np.float32(int(d.hits.sum().item()) / (b * A))


def test_ties_agree_with_the_decode_entry(gpu):
    from epn_pointcloud_amd import alignment
    wts, y, label, R_target, fwd, _ = Lf.built_case("tie")
    r = run(gpu, wts, y, label, R_target)[0]
    d = alignment.decode_rotation(D(gpu, wts), D(gpu, y), D(gpu, Rf.anchors_for(12)))
    assert torch.equal(r.preds, d.preds) and H(d.preds)[1, 5] == 3


# ----------------------------------------------------------------------------------------------- the mirror class
def _criterion(gpu, anchors, nr):
    from epn_pointcloud_amd.vgtk.loss import MultiTaskDetectionLoss
    return MultiTaskDetectionLoss(D(gpu, anchors), nr=nr, w=Lf.W).to(gpu)


@pytest.mark.parametrize("nr,key", [(4, "q"), (6, "o")])
def test_mirror_class_against_the_reference(gpu, nr, key):
    """The reference's own five outputs and gradients (tests/golden/rotation_loss.npz) within FACTOR = 2 times the distance the
    fixture measured between the reference's fp32 results and the fp64 restatement, plus one fp32 ulp for the device's rounding."""
    from conftest import golden
    g = golden("rotation_loss.npz")
    crit = _criterion(gpu, g["anchors"], nr).train()
    tw, ty = D(gpu, g[f"{key}_wts"]).requires_grad_(), D(gpu, g[f"{key}_y"]).requires_grad_()
    out = crit(tw, D(gpu, g[f"{key}_label"]), ty, D(gpu, g[f"{key}_R_target"]), D(gpu, g[f"{key}_T"]))
    assert isinstance(out, tuple) and len(out) == 5 and crit.iter_counter == 1 and out[4].shape == (2,)
    out[0].backward()
    want = g[f"{key}_out"]
    fwd_err, grad_err = float(g["fwd_err"]), float(g["grad_err"])
    got = H(torch.stack(out[:4])).astype(np.float64)
    print("mirror", got, "golden", want, "err", H(out[4]), "golden", g[f"{key}_err"])
    assert (np.abs(got - want)[:3] <= 2 * fwd_err + np.spacing(want[:3])).all() and got[3] == want[3]
    assert np.abs(H(tw.grad) - g[f"{key}_dwts"]).max() <= 2 * grad_err + 2.0 ** -23 * np.abs(g[f"{key}_dwts"]).max()
    assert np.abs(H(ty.grad) - g[f"{key}_dy"]).max() <= 2 * grad_err + 2.0 ** -23 * np.abs(g[f"{key}_dy"]).max()
    ref = Rf.decode(g[f"{key}_wts"], g[f"{key}_y"], g["anchors"], None, g[f"{key}_T"])
    assert np.abs(H(out[4]) - ref["err"]).max() <= 1e-5 and np.abs(H(out[4]) - g[f"{key}_err"]).max() <= 1e-3
    assert np.array_equal(H(crit.preds), ref["preds"]) and not H(crit.row_flags).any()
    crit.eval()
    crit(tw, D(gpu, g[f"{key}_label"]), ty, D(gpu, g[f"{key}_R_target"]), D(gpu, g[f"{key}_T"]))
    assert crit.iter_counter == 1                              # counts training steps only, as upstream


def test_forward_and_backward_replay_from_a_captured_graph(gpu):
    """Forward + backward of the mirror class at A = 12, b = 3, captured once on one stream (a linear graph: no parallel
    branches) and replayed with new values copied into the static inputs: each replay equals the eager result bitwise."""
    sets = [Lf.case(12, 3, 4, seed)[:6] for seed in (Lf.CASES[8][3],)] + [Lf.built_case(n)[:4] for n in ("tie", "big")]
    anchors, T = sets[0][4], D(gpu, sets[0][5])
    crit = _criterion(gpu, anchors, 4)
    eager = []
    for s in sets:
        tw, ty = D(gpu, s[0]).requires_grad_(), D(gpu, s[1]).requires_grad_()
        out = crit(tw, D(gpu, s[2]), ty, D(gpu, s[3]), T)
        out[0].backward()
        eager.append([o.detach().clone() for o in out] + [tw.grad.clone(), ty.grad.clone()])
    tw, ty = D(gpu, sets[0][0]).requires_grad_(), D(gpu, sets[0][1]).requires_grad_()
    lab, Rt = D(gpu, sets[0][2]), D(gpu, sets[0][3])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                            # warm-up off the capture, as torch asks
        crit(tw, lab, ty, Rt, T)[0].backward()
    torch.cuda.current_stream().wait_stream(side)
    tw.grad = ty.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = crit(tw, lab, ty, Rt, T)
        out[0].backward()
    for k in (1, 2, 0):
        with torch.no_grad():
            tw.copy_(D(gpu, sets[k][0]))
            ty.copy_(D(gpu, sets[k][1]))
            lab.copy_(D(gpu, sets[k][2]))
            Rt.copy_(D(gpu, sets[k][3]))
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(o.detach(), e) for o, e in zip(out, eager[k][:5]))
        assert torch.equal(tw.grad, eager[k][5]) and torch.equal(ty.grad, eager[k][6])


# ----------------------------------------------------------------------------------------------- network level
def test_network_trains_against_the_loss(gpu):
    """The tiny RegSO3ConvModel of the model tests in training mode, two forwards on the same pairs: one followed by the mirror
    loss, one by the torch restatement of the reference's loss terms (test_rotation_loss_spec.torch_loss) in fp32; backward();
    every parameter gradient agrees under the rule of the network-level gradient tests of test_gpu_models.py (grad_close: relative
    L2 error below 3 %; exact-zero gradients and the noise-decided first skip branch as there, see below), and the losses
    within 1e-4 relative (fp32 sums over 120 rows on the torch side)."""
    import epn_pointcloud_amd.vgtk.functional as F
    from test_gpu_models import grad_close
    from test_gpu_rotation import _pairs, _tiny_reg
    from test_rotation_loss_spec import torch_loss
    m = _tiny_reg(gpu).train()
    src, tgt, T = _pairs(2, 256, 23)
    x = torch.stack((D(gpu, src), D(gpu, tgt)), dim=1)
    anchors = m.get_anchor().detach().float().contiguous()
    gt_T = D(gpu, T)
    R_target, label = F.label_relative_rotation(anchors, gt_T)
    nr = m.outblock.out_channel
    crit = _criterion(gpu, H(anchors), nr)
    grads, values = [], []
    for use_mirror in (True, False):
        m.zero_grad(set_to_none=True)
        conf, y = m(x)
        assert y.shape[1] == nr
        loss = crit(conf, label, y, R_target, gt_T)[0] if use_mirror else torch_loss(conf.float(), label, y.float(), R_target, Lf.W)[0]
        loss.backward()
        values.append(loss.item())
        grads.append({k: None if p.grad is None else p.grad.detach().clone() for k, p in m.named_parameters()})
    print("losses", values)
    assert np.isfinite(values).all() and abs(values[0] - values[1]) <= 1e-4 * abs(values[1])
    assert grads[0] and all(g is not None for g in grads[0].values()), [k for k, g in grads[0].items() if g is None]
    assert any(torch.count_nonzero(g) > 0 for g in grads[0].values())
    # As in test_gpu_models.test_full_width_cls_step_matches_oracle_loss: a parameter whose exact gradient is zero (the first
    # block's skip convolution over the constant occupancy feature, the biases a normalisation cancels) holds rounding noise
    # below 1e-3 of the largest gradient on either side, and the first block's skip-branch norm affine is decided by the sign
    # of such noise; the former are held to 2e-3 of the largest gradient, the latter left out by name.
    noise_decided = {"backbone.0.blocks.0.norm.bias", "backbone.0.blocks.0.norm.weight"}
    gmax = max(g.abs().max().item() for g in grads[1].values())
    bad, checked = [], 0
    for k, g in grads[0].items():
        assert torch.isfinite(g).all(), k
        want = grads[1][k]
        if k in noise_decided:
            continue
        if want.abs().max().item() < 1e-3 * gmax:
            assert g.abs().max().item() < 2e-3 * gmax, k
            continue
        checked += 1
        if not grad_close(g, want.cpu()):
            bad.append((k, ((g - want).norm() / want.norm()).item()))
    print("checked", checked, "of", len(grads[0]), "gmax", gmax)
    assert not bad, bad
    assert 2 * checked > len(grads[0]), checked
