"""The classification loss and the evaluation tallies on the GPU (csrc/cls_loss.hip behind losses.classification_loss,
losses.classification_tally, the mirror classes vgtk.CrossEntropyLoss / vgtk.AttentionCrossEntropyLoss, ClsSO3ConvModel.classify
and classification.evaluate_classification) against the numpy fp64 restatement of their specification (tests/cls_loss_ref.py).
The case table and what the bound rests on are asserted on the CPU by test_cls_loss_spec.py (test_cases_are_unambiguous).

Tolerance.  The kernels compute in fp64 and round every output once, so a float output is compared with the restatement's value
rounded to fp32 and may differ from it by ONE fp32 ulp of that value: the two fp64 values differ by the exp / log implementations
and the summation order, of order 1e-16 relative -- far below half an fp32 ulp, but enough to straddle a rounding boundary.
Integer outputs and flags are exact.  NaN is expected exactly where the restatement has it.

Measured on an MI355X when this file was written: every float output of the 45 table cases, the six built cases, the three
[B,C,A] layouts and the network-level tests equalled the restatement's value rounded to fp32 bit for bit (largest error 0 ulp,
exact in 100 % of the elements; each test prints both figures).  Against the reference's fp32 results the stored margins
are fwd_err 1.122e-06 and grad_err 2.325e-08."""
import ctypes

import numpy as np
import pytest
import torch

import cls_loss_ref as Cf

pytestmark = pytest.mark.gpu


def D(gpu, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def H(t):
    return None if t is None else t.detach().cpu().numpy()


def one_ulp(got, ref, what=""):
    """|got - fp32(ref)| <= ulp(fp32(ref)) elementwise, NaN exactly where ref has it; prints the largest error first."""
    got = np.asarray(H(got) if isinstance(got, torch.Tensor) else got).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        ref32 = np.asarray(ref, dtype=np.float64).astype(np.float32)
    assert got.shape == ref32.shape, (what, got.shape, ref32.shape)
    nan = np.isnan(ref32)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.isfinite(ref32[~nan]).all(), what
    err = np.abs(got[~nan] - ref32[~nan].astype(np.float64))
    ulp = np.spacing(np.abs(ref32[~nan])).astype(np.float64)
    print(f"{what}: largest err {float((err / ulp).max()) if err.size else 0:.3f} ulp, exact in "
          f"{float((err == 0).mean()) if err.size else 1:.4f} of {err.size}")
    return bool((err <= ulp).all())


def run(gpu, logits, label, att, att_label, coef, upstream=None, coef_on_device=False):
    from epn_pointcloud_amd import losses
    tl = D(gpu, logits).requires_grad_()
    ta = None if att is None else D(gpu, att).requires_grad_()
    c = D(gpu, np.asarray(coef, dtype=np.float32)) if coef_on_device else coef
    if att is None or att.shape[0] == logits.shape[0]:
        r = losses.classification_loss(tl, D(gpu, label), ta, D(gpu, att_label), c)
    else:
        # the entry takes any two row sets; the public function ties the attention rows to the batch, so the table's cases with
        # R != B go through its autograd Function directly
        r = losses.ClsLossResult(*losses._ClsLoss.apply(tl, D(gpu, label), ta, D(gpu, att_label), D(gpu, np.asarray(coef, dtype=np.float32))))
    (r.loss if upstream is None else r.loss * upstream).backward()
    return r, tl.grad, None if ta is None else ta.grad


def check(got, logits, label, att, att_label, coef, what, g=1.0):
    r, dl, da = got
    fwd = Cf.forward(logits, label, att, att_label, coef)
    rdl, rda = Cf.backward(g, logits, label, att, att_label, coef)
    assert r.loss.dim() == 0 and r.loss.requires_grad and not any(t.requires_grad for t in r[1:] if t is not None)
    assert r.preds.dtype == r.row_flags.dtype == torch.int32 and r.loss.dtype == r.row_ce.dtype == dl.dtype == torch.float32
    assert np.array_equal(H(r.preds), fwd["preds"]) and np.array_equal(H(r.row_flags), fwd["row_flags"])
    assert one_ulp(r.row_ce, fwd["row_ce"], what + " row_ce")
    sc = torch.stack(r[:5])
    print(what, "scalars", H(sc), "ref", fwd["scalars"])
    assert one_ulp(sc, fwd["scalars"], what + " scalars") and one_ulp(dl, rdl, what + " dlogits")
    if att is None:
        assert r.att_preds is None and r.att_row_ce is None and r.att_row_flags is None and da is None
        assert r.att_loss.item() == 0 and r.att_acc.item() == 0
    else:
        assert np.array_equal(H(r.att_preds), fwd["att_preds"]) and np.array_equal(H(r.att_row_flags), fwd["att_row_flags"])
        assert one_ulp(r.att_row_ce, fwd["att_row_ce"], what + " att_row_ce") and one_ulp(da, rda, what + " datt")
    return fwd


# ----------------------------------------------------------------------------------------------- the table and the built cases
@pytest.mark.parametrize("case", Cf.CASES, ids=str)
def test_classification_loss(gpu, case):
    args = Cf.case(*case)
    check(run(gpu, *args), *args, str(case))


def test_upstream_gradient_scales_the_backward(gpu):
    args = Cf.case(*Cf.CASES[13])
    check(run(gpu, *args, upstream=-2.5), *args, "upstream -2.5", g=-2.5)


@pytest.mark.nonfinite_inputs
@pytest.mark.parametrize("name", Cf.BUILT)
def test_built_cases(gpu, name):
    """Ties at the first, a middle and the last index; labels at 0 and n - 1; labels -1, n and -100; logits +-1e4; rows with NaN
    and inf; c_att = 0."""
    args = Cf.built_case(name)
    r, dl, da = got = run(gpu, *args)
    fwd = check(got, *args, name)
    if name == "tie":
        assert H(r.preds)[:3].tolist() == [0, 13, 22] and H(r.att_preds)[1:3].tolist() == [30, 0]
    if name == "bad":
        assert H(r.row_flags).tolist() == [0, 1, 0, 1, 1, 0] and not H(dl)[[1, 3, 4]].any() and not H(r.row_ce)[[1, 3, 4]].any()
        assert not H(da)[[0, 5]].any() and torch.isfinite(r.loss)
    if name == "big":
        assert torch.isfinite(torch.stack(r[:5])).all() and torch.isfinite(dl).all() and torch.isfinite(da).all()
        assert H(r.row_ce)[:2].tolist() == [0.0, 2e4]
    if name == "nonfinite":
        assert H(r.row_flags).tolist() == [0, 0, 2, 0, 3, 0] and H(r.preds)[[2, 4]].tolist() == [-1, -1]
        assert np.isnan(H(dl)[2]).all() and not H(dl)[4].any() and np.isnan(H(da)[[3, 5]]).all() and np.isfinite(H(dl)[[0, 1, 3, 5]]).all()
    if name == "c_att0":
        assert not H(da).any() and torch.equal(r.loss, r.cls_loss)
    assert fwd["scalars"].shape == (5,)


def test_host_labels_are_checked_and_give_the_same_bits(gpu):
    from epn_pointcloud_amd import losses
    logits, label, att, att_label, coef = Cf.built_case("bad")
    with pytest.raises(ValueError, match="0..39"):
        losses.classification_loss(D(gpu, logits), torch.from_numpy(label), D(gpu, att), D(gpu, att_label))
    logits, label, att, att_label, coef = Cf.case(5, 40, 5, 60, 7960)
    a = run(gpu, logits, label, att, att_label, coef)
    r = losses.classification_loss(D(gpu, logits), torch.from_numpy(label).long(), D(gpu, att), torch.from_numpy(att_label).long(), coef)
    b = run(gpu, logits, label, att, att_label, coef, coef_on_device=True)
    assert torch.equal(r.loss, a[0].loss) and torch.equal(b[0].loss, a[0].loss) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_bf16_logits_are_converted_and_get_their_gradient(gpu):
    from epn_pointcloud_amd import losses
    logits, label, att, att_label, coef = Cf.case(5, 40, 5, 60, 7960)
    lb, ab = D(gpu, logits).bfloat16().requires_grad_(), D(gpu, att).bfloat16().requires_grad_()
    losses.classification_loss(lb, D(gpu, label), ab, D(gpu, att_label), coef).loss.backward()
    l32, a32 = lb.detach().float().requires_grad_(), ab.detach().float().requires_grad_()
    losses.classification_loss(l32, D(gpu, label), a32, D(gpu, att_label), coef).loss.backward()
    assert lb.grad.dtype == ab.grad.dtype == torch.bfloat16
    assert torch.equal(lb.grad, l32.grad.bfloat16()) and torch.equal(ab.grad, a32.grad.bfloat16())


# ----------------------------------------------------------------------------------------------- the [B,C,A] layout, the mirror
@pytest.mark.parametrize("C", Cf.CHANNELS)
def test_three_dimensional_attention_through_the_mirror_class(gpu, C):
    """wts [4,C,12] with rlabel [4,60]: C = 3 and 60 cut the labels, C = 70 tiles them first; one row per (b, c)."""
    from epn_pointcloud_amd.vgtk import AttentionCrossEntropyLoss
    logits, label, wts, rlabel = Cf.layout_case(C)
    lab = Cf.expand_rlabel(wts, rlabel)
    crit = AttentionCrossEntropyLoss("default", 0.5).to(gpu)
    tl, tw = D(gpu, logits).requires_grad_(), D(gpu, wts).requires_grad_()
    out = crit(tl, D(gpu, label).long(), tw, D(gpu, rlabel).long())
    assert isinstance(out, tuple) and len(out) == 5 and crit.iter_counter == 1
    out[0].backward()
    fwd = Cf.forward(logits, label, wts, lab, (1.0, 0.5))
    rdl, rdw = Cf.backward(1.0, logits, label, wts, lab, (1.0, 0.5))
    assert one_ulp(torch.stack(out), fwd["scalars"], f"C = {C} scalars")
    assert one_ulp(tl.grad, rdl, f"C = {C} dpred") and one_ulp(tw.grad, rdw, f"C = {C} dwts")
    assert crit.att_preds.shape == (4, C) and np.array_equal(H(crit.att_preds), fwd["att_preds"])


@pytest.mark.parametrize("key", "abc")
def test_mirror_classes_against_the_reference(gpu, key):
    """The reference's own outputs and gradients (tests/golden/cls_loss.npz) within the distance the fixture
    measured between the reference's fp32 results and the fp64 restatement, plus one fp32 ulp for the device's rounding."""
    from conftest import golden
    from epn_pointcloud_amd.vgtk import AttentionCrossEntropyLoss, CrossEntropyLoss
    g = golden("cls_loss.npz")
    fwd_err, grad_err = float(g["fwd_err"]), float(g["grad_err"])
    pred, label, wts, rlabel = (g[f"{key}_{n}"] for n in ("pred", "label", "wts", "rlabel"))
    tp = D(gpu, pred).requires_grad_()
    loss, acc = CrossEntropyLoss()(tp, D(gpu, label))
    loss.backward()
    want = g[f"{key}_ce"]
    assert abs(loss.item() - want[0]) <= fwd_err + np.spacing(want[0]) and acc.item() == want[1]
    assert (np.abs(H(tp.grad) - g[f"{key}_ce_dpred"]) <= grad_err + np.spacing(np.abs(g[f"{key}_ce_dpred"]))).all()
    for loss_type, m in Cf.GOLDEN_TYPES:
        for counter in Cf.GOLDEN_COUNTERS:
            tag = f"{key}_{loss_type}_{counter}"
            crit = AttentionCrossEntropyLoss(loss_type, m).to(gpu).train()
            crit.iter_counter = counter
            tp, tw = D(gpu, pred).requires_grad_(), D(gpu, wts).requires_grad_()
            out = crit(tp, D(gpu, label), tw, D(gpu, rlabel), 2000)
            out[0].backward()
            want = g[f"{tag}_out"]
            got = H(torch.stack(out)).astype(np.float64)
            print(tag, "mirror", got, "golden", want)
            assert (np.abs(got - want)[:3] <= fwd_err + np.spacing(want[:3])).all() and np.array_equal(got[3:], want[3:])
            assert crit.iter_counter == int(g[f"{tag}_counter"])
            for grad, name in ((tp.grad, "dpred"), (tw.grad, "dwts")):
                ref = g[f"{tag}_{name}"]
                assert (np.abs(H(grad) - ref) <= grad_err + np.spacing(np.abs(ref))).all(), (tag, name)
            crit.eval()
            crit(tp, D(gpu, label), tw, D(gpu, rlabel), 2000)
            assert crit.iter_counter == counter + 1                 # counts training steps only, as upstream


# ----------------------------------------------------------------------------------------------- every element is written
@pytest.mark.nonfinite_inputs
def test_every_output_element_is_written_over_a_prefill_and_two_runs_are_bitwise_equal(gpu):
    """The raw C entries on buffers pre-filled with NaN (-7 for integers), for a case with flagged rows of both kinds and one
    from the table with 4096 columns: nothing of the prefill is left, the bits are the wrapper's, and a second call repeats
    them."""
    from epn_pointcloud_amd import _lib
    lib = _lib.get_lib()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    for args in (Cf.built_case("bad"), Cf.case(33, 4096, 257, 65, 7411), Cf.case(5, 63, 0, 0, 7412)):
        logits, label, att, att_label, coef = args
        base = run(gpu, *args, coef_on_device=True)
        B, k = logits.shape
        R, A = att.shape if att is not None else (0, 0)
        tl, tlab, tc = D(gpu, logits), D(gpu, label), D(gpu, np.asarray(coef, dtype=np.float32))
        ta, talab = (D(gpu, att), D(gpu, att_label)) if R else (torch.zeros(1, device=gpu), torch.zeros(1, dtype=torch.int32, device=gpu))
        f = lambda *s: torch.full(s, float("nan"), device=gpu)
        i = lambda *s: torch.full(s, -7, dtype=torch.int32, device=gpu)
        runs = []
        for _ in range(2):
            row_ce, pred, flags, arow, apred, aflags, scalars = f(B), i(B), i(B), f(max(R, 1)), i(max(R, 1)), i(max(R, 1)), f(5)
            dl, da, up = f(B, k), f(max(R, 1), max(A, 1)), torch.ones(1, device=gpu)
            null = ctypes.c_void_p(0)
            a5 = (vp(ta), vp(talab)) if R else (null, null)
            assert lib.epn_cls_loss_f32(vp(tl), vp(tlab), B, k, *a5, R, A, vp(tc), vp(row_ce), vp(pred), vp(flags),
                                        vp(arow) if R else null, vp(apred) if R else null, vp(aflags) if R else null, vp(scalars),
                                        _lib.stream_of(tl)) == 0
            assert lib.epn_cls_loss_bwd_f32(vp(up), vp(tl), vp(tlab), vp(flags), B, k, *a5, vp(aflags) if R else null, R, A, vp(tc),
                                            vp(dl), vp(da) if R else null, _lib.stream_of(tl)) == 0
            torch.cuda.synchronize()
            runs.append((row_ce, pred, flags, arow, apred, aflags, scalars, dl, da))
        row_ce, pred, flags, arow, apred, aflags, scalars, dl, da = runs[0]
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(*runs))        # bitwise, NaN included
        assert not torch.isnan(scalars).any() and not torch.isnan(dl).any() and (pred >= 0).all() and (flags >= 0).all()
        r = base[0]
        assert torch.equal(row_ce, r.row_ce) and torch.equal(pred, r.preds) and torch.equal(flags, r.row_flags)
        assert torch.equal(scalars, torch.stack(r[:5]).detach()) and torch.equal(dl, base[1])
        if R:
            assert torch.equal(arow, r.att_row_ce) and torch.equal(apred, r.att_preds) and torch.equal(aflags, r.att_row_flags)
            assert torch.equal(da, base[2]) and not torch.isnan(da).any()
        else:                                                       # an absent set is not touched
            assert torch.isnan(arow).all() and (apred == -7).all() and torch.isnan(da).all()
            assert scalars[2].item() == 0 and scalars[4].item() == 0


# ----------------------------------------------------------------------------------------------- capture
def test_forward_and_backward_replay_from_a_captured_graph(gpu):
    """Forward + backward at B = 6, k = 40, A = 60 captured once on one stream and replayed after logits, labels and coef were
    rewritten in place: each replay equals a fresh eager call bitwise."""
    from epn_pointcloud_amd import losses
    sets = [Cf.case(6, 40, 6, 60, 7900)] + [Cf.built_case(n) for n in ("tie", "big", "c_att0")]
    eager = []
    for s in sets:
        r, dl, da = run(gpu, *s, coef_on_device=True)
        eager.append([t.detach().clone() for t in r[:5]] + [r.preds.clone(), r.att_preds.clone(), dl.clone(), da.clone()])
    tl, ta = D(gpu, sets[0][0]).requires_grad_(), D(gpu, sets[0][2]).requires_grad_()
    lab, alab, coef = D(gpu, sets[0][1]), D(gpu, sets[0][3]), D(gpu, np.asarray(sets[0][4], dtype=np.float32))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                            # warm-up off the capture, as torch asks
        losses.classification_loss(tl, lab, ta, alab, coef).loss.backward()
    torch.cuda.current_stream().wait_stream(side)
    tl.grad = ta.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        r = losses.classification_loss(tl, lab, ta, alab, coef)
        r.loss.backward()
    for k in (1, 2, 3, 0):
        with torch.no_grad():
            tl.copy_(D(gpu, sets[k][0]))
            lab.copy_(D(gpu, sets[k][1]))
            ta.copy_(D(gpu, sets[k][2]))
            alab.copy_(D(gpu, sets[k][3]))
            coef.copy_(D(gpu, np.asarray(sets[k][4], dtype=np.float32)))
        graph.replay()
        torch.cuda.synchronize()
        got = [t.detach() for t in r[:5]] + [r.preds, r.att_preds, tl.grad, ta.grad]
        assert all(torch.equal(x, y) for x, y in zip(got, eager[k])), k


# ----------------------------------------------------------------------------------------------- tallies
@pytest.mark.nonfinite_inputs
def test_two_chunks_accumulate_into_the_restatement_s_tables(gpu):
    from epn_pointcloud_amd import losses
    k, A = 40, 60
    tables, ref = losses.ClassificationTables(k, A, gpu), None
    flagged = 0
    for B, seed in ((33, 7950), (257, 7951)):
        logits, label, att, att_label, coef = Cf.case(B, k, B, A, seed)
        label[1], att_label[2], logits[3, 5], att[4, 0] = -1, A, np.nan, np.inf
        label[5] = logits[5].argmax()
        r = losses.classification_loss(D(gpu, logits), D(gpu, label), D(gpu, att), D(gpu, att_label), coef)
        assert losses.classification_tally(r, D(gpu, label), tables, D(gpu, att_label)) is tables
        fwd = Cf.forward(logits, label, att, att_label, coef)
        ref = Cf.tally(fwd["preds"], label, fwd["row_flags"], k, fwd["att_preds"], fwd["att_row_flags"], att_label, A, ref)
        flagged += 4
    assert np.array_equal(H(tables.confusion), ref[0]) and np.array_equal(H(tables.anchor_table), ref[1])
    assert H(tables.totals).tolist() == ref[2].tolist() and ref[2][3] == flagged and ref[2][0] == 33 + 257 - flagged
    t = tables.result()
    assert t.rows == ref[2][0] and t.skipped == flagged and t.instance_acc == ref[2][1] / ref[2][0] and t.attention_acc == ref[2][2] / ref[2][0]
    assert t.confusion.sum() == t.anchor_table.sum() == t.rows
    seen = ref[0].sum(axis=1) > 0
    assert np.array_equal(t.class_acc[seen], (np.diagonal(ref[0]) / ref[0].sum(axis=1).astype(np.float64))[seen]) and np.isnan(t.class_acc[~seen]).all()
    # without attention: the confusion matrix alone
    plain = losses.ClassificationTables(k, 0, gpu)
    r = losses.classification_loss(D(gpu, logits), D(gpu, label))
    losses.classification_tally(r, D(gpu, label), plain)
    fwd = Cf.forward(logits, label)
    ref = Cf.tally(fwd["preds"], label, fwd["row_flags"], k)
    assert np.array_equal(H(plain.confusion), ref[0]) and H(plain.totals).tolist() == ref[2].tolist() and plain.anchor_table is None
    assert np.isnan(plain.result().attention_acc)


# ----------------------------------------------------------------------------------------------- network level
def _tiny_cls(gpu):
    """The public builder at a quarter of the width (16 to 64 channels: the kernel family of the full-size network), 256 points,
    filled deterministically."""
    from epn_pointcloud_amd import models
    from test_models_cpu import fill_state_dict
    return fill_state_dict(models.build_cls(input_num=256, width_div=4)).to(gpu)


def _clouds(gpu, M, seed):
    from epn_pointcloud_amd import schedule as S
    rng = np.random.default_rng(seed)
    return S.synthetic_clouds(M, 256, gpu, seed=seed), D(gpu, rng.integers(0, 40, M)), D(gpu, rng.integers(0, 60, M))


def test_network_gradients_arrive_through_the_loss(gpu):
    """The tiny ClsSO3ConvModel of the model tests in training mode, B = 4, N = 256: the gradient arriving at the retained
    logits and attention tensors is the restatement's on the device's own logits, and every parameter gets a finite gradient."""
    from epn_pointcloud_amd.vgtk import AttentionCrossEntropyLoss
    m = _tiny_cls(gpu).train()
    pc, label, rlabel = _clouds(gpu, 4, 31)
    crit = AttentionCrossEntropyLoss("default", 0.5).to(gpu)
    logits, att = m(pc)
    assert logits.shape == (4, 40) and att.shape == (4, 60)
    logits.retain_grad()
    att.retain_grad()
    out = crit(logits, label, att, rlabel)
    out[0].backward()
    args = (H(logits).astype(np.float32), H(label), H(att).astype(np.float32), H(rlabel), (1.0, 0.5))
    fwd = Cf.forward(*args)
    rdl, rda = Cf.backward(1.0, *args)
    assert one_ulp(torch.stack(out), fwd["scalars"], "network scalars")
    assert one_ulp(logits.grad, rdl, "network dlogits") and one_ulp(att.grad, rda, "network dattention")
    missing = [k for k, p in m.named_parameters() if p.grad is None or not torch.isfinite(p.grad).all()]
    assert not missing, missing
    assert any(torch.count_nonzero(p.grad) > 0 for p in m.parameters())


def test_classify_and_evaluate_classification_equal_the_per_chunk_restatement(gpu):
    """10 clouds with batch = 4 (chunks of 4, 4 and 2): the tables, the accuracies and the mean losses are the restatement's on
    each chunk's own logits; the short last chunk weighs like a full one in batch_mean_acc only."""
    from epn_pointcloud_amd import classification, losses
    m = _tiny_cls(gpu).eval()
    pc, label, rlabel = _clouds(gpu, 10, 37)
    ev = classification.evaluate_classification(m, pc, label, rlabel, batch=4)
    logits, pred, anchor = m.classify(pc, batch=4)
    assert logits.shape == (10, 40) and pred.dtype == anchor.dtype == torch.int32
    ref, scal = None, []
    with torch.no_grad():
        for i in (0, 4, 8):
            lg, at = m(pc[i:i + 4])
            assert torch.equal(lg, logits[i:i + 4])
            lab, rl = H(label[i:i + 4]), H(rlabel[i:i + 4])
            fwd = Cf.forward(H(lg), lab, H(at).reshape(len(lab), -1), rl, (1.0, 1.0))
            assert np.array_equal(H(pred[i:i + 4]), fwd["preds"]) and np.array_equal(H(anchor[i:i + 4]), fwd["att_preds"])
            ref = Cf.tally(fwd["preds"], lab, fwd["row_flags"], 40, fwd["att_preds"], fwd["att_row_flags"], rl, 60, ref)
            scal.append(fwd["scalars"].astype(np.float32))
    scal = np.stack(scal)
    assert np.array_equal(ev.confusion, ref[0]) and np.array_equal(ev.anchor_table, ref[1]) and (ev.rows, ev.skipped) == (10, 0)
    assert ev.instance_acc == ref[2][1] / 10 and ev.att_acc == ref[2][2] / 10
    assert one_ulp(ev.batch_acc, scal[:, 3], "batch acc") and ev.batch_mean_acc == float(ev.batch_acc.mean())
    w = np.array([0.4, 0.4, 0.2])
    for got, col in ((ev.loss, 0), (ev.cls_loss, 1), (ev.att_loss, 2)):
        want = float((scal[:, col].astype(np.float64) * w).sum())
        assert abs(got - want) <= 3 * np.spacing(np.float32(want)), (col, got, want)
    plain = classification.evaluate_classification(m, pc, label, batch=4)
    assert np.array_equal(plain.confusion, ref[0]) and np.array_equal(plain.anchor_table, ref[1]) and np.isnan(plain.att_loss)
    assert np.isnan(plain.att_acc) and abs(plain.loss - plain.cls_loss) <= np.spacing(np.float32(plain.loss))
    # a head that pools without attention, one cloud per chunk: its second output is a feature map, whatever its shape
    from epn_pointcloud_amd import models
    from test_models_cpu import fill_state_dict
    mm = fill_state_dict(models.build_cls(input_num=256, width_div=4, pooling="max")).to(gpu).eval()
    lg, pr, an = mm.classify(pc[:2], batch=1)
    assert lg.shape == (2, 40) and an.tolist() == [-1, -1] and torch.equal(pr.long(), lg.argmax(1))
    ev = classification.evaluate_classification(mm, pc[:2], label[:2], batch=1)
    assert ev.anchor_table is None and ev.rows == 2 and ev.confusion.sum() == 2 and np.isnan(ev.att_loss)
    with pytest.raises(ValueError, match="attention"):
        classification.evaluate_classification(mm, pc[:2], label[:2], rlabel[:2], batch=1)


def test_a_captured_training_step_with_the_schedule_loss_replays(gpu):
    """forward + vgtk.AttentionCrossEntropyLoss('schedule', 1.0) + backward of the tiny network captured once; before each
    replay the trainer calls update_schedule() in forward's place.  Each replay's five loss values are the restatement's on the
    replay's own logits with the schedule weight of that step, and the gradient at the logits follows."""
    from epn_pointcloud_amd.vgtk import AttentionCrossEntropyLoss
    m = _tiny_cls(gpu).train()
    pc, label, rlabel = _clouds(gpu, 4, 41)
    crit = AttentionCrossEntropyLoss("schedule", 1.0).to(gpu).train()
    params = [p for p in m.parameters() if p.requires_grad]
    kept = {}

    def step():
        for p in params:
            p.grad = None
        logits, att = m(pc)
        logits.retain_grad()
        out = crit(logits, label, att, rlabel, 4)
        out[0].backward()
        kept.update(logits=logits, att=att, out=out)

    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        step()
        step()
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize(gpu)
    assert crit.iter_counter == 2
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        step()
    assert crit.iter_counter == 2                                   # a capture computes nothing and counts nothing
    captured = crit._coef                                           # the buffer the graph reads
    # every spelling of the device names the same buffer: "cuda" (the current device), torch.device("cuda"), the indexed
    # device, and None (the buffer that exists); a new allocation would leave the graph reading freed memory
    for counter, dev in zip((2, 3, 4, 5), ("cuda", torch.device("cuda"), None, gpu)):
        assert crit.iter_counter == counter
        buf = crit.update_schedule(dev, 4)
        assert buf is captured and buf.data_ptr() == captured.data_ptr()
        assert buf.tolist() == [float(np.float32(c)) for c in Cf.schedule_coefficients("schedule", 1.0, counter, 4)]
        with torch.no_grad():
            label.copy_((label + 1) % 40)
        graph.replay()
        torch.cuda.synchronize(gpu)
        coef = Cf.schedule_coefficients("schedule", 1.0, counter, 4)
        args = (H(kept["logits"]), H(label), H(kept["att"]).reshape(4, -1), H(rlabel), coef)
        fwd = Cf.forward(*args)
        assert one_ulp(torch.stack(kept["out"]), fwd["scalars"], f"replay at counter {counter}")
        assert one_ulp(kept["logits"].grad, Cf.backward(1.0, *args)[0], f"replay at counter {counter} dlogits")
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in params)
