"""The training loss of the descriptor network on the GPU (csrc/triplet_loss.hip behind epn_pointcloud_amd.losses and the mirror
class vgtk.loss.TripletBatchLoss) against the numpy fp64 restatement of its specification (tests/triplet_ref.py).  The case
tables and the conditions the tolerances rest on (no near tie among the distances of a row or among the four largest traces,
hinge arguments away from their kink, no d2 near eps) are asserted on the CPU by test_triplet_spec.py.

Tolerances (u = 2^-24, the relative size of one fp32 rounding; the kernels compute in fp64 and round every output once):
  integers   equal.
  per-row    d_pos, d_neg, row_loss: the fp64 value differs from the restatement's by the order of D additions, about
             D 2^-53 relative, and is rounded once: within u |ref| + 1e-12 (the absolute term for a hinge value that is a
             difference of two distances: 1e-12 >> 3840 * 2^-53 * 2).
  scalars    the fp64 mean of the ROUNDED rows, rounded once.  The restatement rounds its own rows; a device row may round to
             the neighbouring fp32 (1 ulp = 2u relative) where the two fp64 values straddle a rounding boundary, all terms
             are >= 0, and the mean is rounded again: within 3u |ref|.  accuracy is a count / N: within u.
  gradients  the backward works on the saved fp32 d_pos, d_neg.  Given the same saved values it differs from the restatement
             by fp64 noise and one rounding: u |ref|.  If a saved distance is the neighbouring fp32 (as above), the
             coefficient g / d of that row moves by 2u relative through d, and in soft mode by another beta 2u (d_pos + d_neg)
             through g = sigmoid(beta x) (|dg / g| <= beta |dx|): within u |ref| + 2u (1 + beta (d_pos + d_neg)_max) mag, mag
             the sum of the absolute values of the terms of the element (triplet_ref.batch_hard_bwd); beta = 0 outside soft.
  interpolation  w within u; out within u |ref| + 1e-13; dfeature, from the saved fp32 w: u |ref| + 2u mag.
  mirror     total is a sum of two fp32 scalars formed in fp32: 3u (|inv| + alpha |equi|) + u |total|.  The equivariance
             term's input is the ROUNDED interpolation output, which may be the neighbouring fp32 of the restatement's: a
             distance over D' = C A entries then moves by at most 2u max|entry| sqrt(D') -- added to the per-row and scalar
             tolerances of that term -- and its gradients are compared with (s - t) perturbed likewise: an extra
             2u max|entry| |c| per element, |c| <= alpha / (N d_min)."""
import numpy as np
import pytest
import torch

import triplet_ref as Tf

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def D(gpu, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def H(t):
    return None if t is None else t.detach().cpu().numpy()


def within(got, ref, tol):
    err = np.abs(H(got).astype(np.float64) - ref)
    ok = bool((err <= tol).all())
    if not ok:
        k = np.unravel_index(np.argmax(err - tol), err.shape)
        print(f"worst at {k}: got {H(got)[k]!r}, ref {ref[k]!r}, err {err[k]:.3e}, tol {np.broadcast_to(tol, err.shape)[k]:.3e}")
    return ok


def grad_tol(ref, mag, fwd, mode, margin):
    beta = margin if mode == "soft" else 0.0
    return U * np.abs(ref) + 2 * U * (1 + beta * (fwd["d_pos"] + fwd["d_neg"]).max()) * mag + 1e-30


def run_batch_hard(gpu, src, tgt, mode, margin, upstream=None):
    from epn_pointcloud_amd import losses
    s, t = D(gpu, src).requires_grad_(), D(gpu, tgt).requires_grad_()
    r, rows = losses.batch_hard_rows(s, t, mode, margin)
    (r.loss if upstream is None else r.loss * upstream).backward()
    return r, rows, s.grad, t.grad


def check_batch_hard(got, fwd, bwd, mode, margin):
    r, rows, gs, gt = got
    assert r.neg_idx.dtype == r.nn_idx.dtype == rows["row_flags"].dtype == torch.int32
    assert r.loss.dtype == torch.float32 and r.loss.dim() == 0 and not r.accuracy.requires_grad and not r.pos.requires_grad
    assert np.array_equal(H(r.neg_idx), fwd["neg_idx"])
    assert np.array_equal(H(r.nn_idx), fwd["nn_idx"])
    assert np.array_equal(H(rows["row_flags"]), fwd["row_flags"])
    for key in ("d_pos", "d_neg", "row_loss"):
        assert within(rows[key], fwd[key], U * np.abs(fwd[key]) + 1e-12), key
    sc = torch.stack((r.loss, r.accuracy, r.pos, r.neg))
    print("scalars", H(sc), "ref", fwd["scalars"])
    assert within(sc, fwd["scalars"], np.array([3, 1, 3, 3]) * U * np.abs(fwd["scalars"]) + 1e-30)
    dsrc, dtgt, mag_s, mag_t = bwd
    assert gs.dtype == gt.dtype == torch.float32
    assert within(gs, dsrc, grad_tol(dsrc, mag_s, fwd, mode, margin)), "dsrc"
    assert within(gt, dtgt, grad_tol(dtgt, mag_t, fwd, mode, margin)), "dtgt"


# ----------------------------------------------------------------------------------------------- batch-hard
@pytest.mark.parametrize("case", Tf.BH_CASES, ids=str)
def test_batch_hard(gpu, case):
    src, tgt, margin, fwd, bwd = Tf.bh_case(*case)
    check_batch_hard(run_batch_hard(gpu, src, tgt, case[2], margin), fwd, bwd, case[2], margin)


def test_upstream_gradient_scales_the_backward(gpu):
    N, Dm, mode, seed = Tf.BH_CASES[4]
    src, tgt, margin, fwd, _ = Tf.bh_case(N, Dm, mode, seed)
    dsrc, dtgt, mag_s, mag_t = Tf.batch_hard_bwd(-2.5, src, tgt, fwd, mode, margin)
    _, _, gs, gt = run_batch_hard(gpu, src, tgt, mode, margin, upstream=-2.5)
    assert within(gs, dsrc, grad_tol(dsrc, mag_s, fwd, mode, margin))
    assert within(gt, dtgt, grad_tol(dtgt, mag_t, fwd, mode, margin))


def test_identical_tgt_rows_lower_index_wins(gpu):
    src, tgt, mode, margin, fwd, bwd = Tf.built_case("dup")
    got = run_batch_hard(gpu, src, tgt, mode, margin)
    assert H(got[0].neg_idx)[0] == 2 and H(got[0].nn_idx)[0] == 2
    check_batch_hard(got, fwd, bwd, mode, margin)


def test_exact_positive_is_clamped_and_has_no_gradient(gpu):
    src, tgt, mode, margin, fwd, bwd = Tf.built_case("zero")
    got = run_batch_hard(gpu, src, tgt, mode, margin)
    check_batch_hard(got, fwd, bwd, mode, margin)
    r, rows, gs, gt = got
    assert H(rows["d_pos"])[3] == np.float32(np.sqrt(Tf.EPS)) and H(rows["row_flags"])[3] & Tf.FLAG_POS_CLAMPED
    # row 3's positive term is zero: what is left of dsrc[3] is its negative term alone
    s, t = src.astype(np.float64), tgt.astype(np.float64)
    j = fwd["neg_idx"][3]
    active = float(bool(fwd["row_flags"][3] & Tf.FLAG_HINGE_ACTIVE))
    want = -active / 8 * (s[3] - t[j]) / np.float64(np.float32(fwd["d_neg"][3]))
    assert within(gs[3], want, 3 * U * np.abs(want) + 1e-30)
    assert torch.isfinite(gs).all() and torch.isfinite(gt).all()


def test_one_negative_shared_by_more_rows_than_a_round_of_the_list(gpu):
    """1029 rows whose hardest negative is tgt[0], D = 257: dtgt[0] is gathered in two rounds of the backward's 1024-row list,
    over two passes of columns."""
    src, tgt, mode, margin, fwd, bwd = Tf.built_case("crowd")
    check_batch_hard(run_batch_hard(gpu, src, tgt, mode, margin), fwd, bwd, mode, margin)


def test_softplus_threshold_rows(gpu):
    src, tgt, mode, margin, fwd, bwd = Tf.built_case("soft")
    check_batch_hard(run_batch_hard(gpu, src, tgt, mode, margin), fwd, bwd, mode, margin)


# ----------------------------------------------------------------------------------------------- interpolation
def run_interp(gpu, feature, T, anchors, dout):
    from epn_pointcloud_amd import losses
    f = D(gpu, feature).requires_grad_()
    out, idx, w = losses.interpolate_anchor_features(f, D(gpu, T), D(gpu, anchors), Tf.SIGMA, return_weights=True)
    out.backward(D(gpu, dout))
    return out, idx, w, f.grad


@pytest.mark.parametrize("case", Tf.INTERP_CASES, ids=str)
def test_anchor_interpolation(gpu, case):
    feature, T, anchors, dout, fwd, (df, mag) = Tf.interp_case(*case)
    out, idx, w, g = run_interp(gpu, feature, T, anchors, dout)
    assert idx.dtype == torch.int32 and out.dtype == w.dtype == g.dtype == torch.float32 and out.shape == feature.shape
    assert np.array_equal(H(idx), fwd["idx"])
    assert within(w, fwd["w"], U * fwd["w"])
    assert within(out, fwd["out"], U * np.abs(fwd["out"]) + 1e-13)
    assert within(g, df, U * np.abs(df) + 2 * U * mag + 1e-30)


@pytest.mark.parametrize("A", [12, 60])
def test_identity_transform_keeps_every_anchor_first(gpu, A):
    """T = I: anchor n is its own nearest anchor (trace 3) and the weights sum to one.  The second and third neighbours of a
    group element are tied by symmetry and are not compared."""
    import rotation_ref as Rf
    from epn_pointcloud_amd import losses
    anchors = Rf.anchors_for(A)
    f = torch.randn(2, 3, A, device=gpu, generator=torch.Generator(device=gpu).manual_seed(5))
    out, idx, w = losses.interpolate_anchor_features(f, torch.eye(3, device=gpu).repeat(2, 1, 1), D(gpu, anchors), Tf.SIGMA,
                                                     return_weights=True)
    assert np.array_equal(H(idx)[:, :, 0], np.tile(np.arange(A), (2, 1)))
    assert np.abs(H(w).astype(np.float64).sum(-1) - 1).max() <= 3 * U
    assert (H(idx) >= 0).all() and (H(idx) < A).all() and torch.isfinite(out).all()


def test_rigid_transform_gives_what_its_rotation_block_gives(gpu):
    from epn_pointcloud_amd import losses
    feature, T, anchors, dout, fwd, _ = Tf.interp_case(*Tf.INTERP_CASES[1])
    T4 = np.zeros((T.shape[0], 4, 4), np.float32)
    T4[:, :3, :3], T4[:, :3, 3], T4[:, 3, 3] = T, 7.0, 1.0
    a = losses.interpolate_anchor_features(D(gpu, feature), D(gpu, T), D(gpu, anchors), Tf.SIGMA, return_weights=True)
    b = losses.interpolate_anchor_features(D(gpu, feature), D(gpu, T4), D(gpu, anchors), Tf.SIGMA, return_weights=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ----------------------------------------------------------------------------------------------- the mirror class
def _criterion(gpu, m, alpha, mode="hard"):
    import types
    from epn_pointcloud_amd.vgtk.loss import TripletBatchLoss
    opt = types.SimpleNamespace(device=gpu, train_loss=types.SimpleNamespace(loss_type=mode, margin=m["margin"]))
    return TripletBatchLoss(opt, D(gpu, m["anchors"]), sigma=Tf.SIGMA, alpha=alpha).to(gpu)


def _mirror_inputs(gpu, m):
    return [D(gpu, m[k]).requires_grad_() for k in ("src", "tgt", "equi_src", "equi_tgt")] + [D(gpu, m["T"])]


def test_mirror_class_invariance_form(gpu):
    m = Tf.mirror_case(0.0)
    crit = _criterion(gpu, m, 0.0)
    src, tgt, es, et, T = _mirror_inputs(gpu, m)
    out = crit(src, tgt, T, es, et)                         # alpha = 0: the equivariant features are ignored, as upstream
    assert isinstance(out, tuple) and len(out) == 4
    out[0].backward()
    inv = m["inv"]
    assert within(torch.stack(out), inv["scalars"], np.array([3, 1, 3, 3]) * U * np.abs(inv["scalars"]) + 1e-30)
    assert np.array_equal(H(crit.match_idx), inv["nn_idx"][:, None])
    assert within(crit.fpos, inv["d_pos"], U * inv["d_pos"]) and within(crit.cneg, inv["d_neg"], U * inv["d_neg"])
    assert not hasattr(crit, "all_dist") and es.grad is None and et.grad is None
    assert within(src.grad, m["dsrc"], grad_tol(m["dsrc"], m["mag_src"], inv, "hard", 0))
    assert within(tgt.grad, m["dtgt"], grad_tol(m["dtgt"], m["mag_tgt"], inv, "hard", 0))


def test_mirror_class_equivariance_form(gpu):
    alpha = 0.5
    m = Tf.mirror_case(alpha)
    crit = _criterion(gpu, m, alpha)
    src, tgt, es, et, T = _mirror_inputs(gpu, m)
    total, inv_info, equi_info = crit(src, tgt, T, es, et)
    total.backward()
    inv, equi = m["inv"], m["equi"]
    N, Dm, C, A, _ = Tf.MIRROR_CASE
    assert isinstance(inv_info, list) and isinstance(equi_info, list) and len(inv_info) == len(equi_info) == 4
    assert within(torch.stack(inv_info), inv["scalars"], np.array([3, 1, 3, 3]) * U * np.abs(inv["scalars"]) + 1e-30)
    amax = max(np.abs(m["equi_src"]).max(), np.abs(m["interp"]["out"]).max())
    shift = 2 * U * amax * np.sqrt(C * A)                    # the interpolation output one fp32 off in every entry
    assert within(torch.stack(equi_info), equi["scalars"], np.array([3, 1, 3, 3]) * U * np.abs(equi["scalars"]) +
                  np.array([2, 0, 1, 1]) * shift)
    assert within(total, np.float64(m["total"]), 3 * U * (inv["scalars"][0] + alpha * equi["scalars"][0]) + U * abs(m["total"]) +
                  2 * alpha * shift)
    assert within(src.grad, m["dsrc"], grad_tol(m["dsrc"], m["mag_src"], inv, "hard", 0))
    assert within(tgt.grad, m["dtgt"], grad_tol(m["dtgt"], m["mag_tgt"], inv, "hard", 0))
    c_max = alpha / (N * min(equi["d_pos"].min(), equi["d_neg"].min()))
    extra = 2 * U * amax * c_max * (1 + shift / min(equi["d_pos"].min(), equi["d_neg"].min()) * np.sqrt(C * A))
    assert within(es.grad, m["d_equi_src"], grad_tol(m["d_equi_src"], m["mag_equi_src"], equi, "hard", 0) + 2 * extra)
    # through the interpolation's backward: its input dtgt carries the tolerance above, its weights sum to one per output
    # row but an input anchor may collect up to 3 A weights; mag_equi_tgt bounds the sum actually formed
    tol_flat = grad_tol(m["mag_flat_tgt"], m["mag_flat_tgt"], equi, "hard", 0) + 2 * N * extra
    wsum = np.abs(Tf.anchor_interp_bwd(np.ones_like(m["equi_tgt"]), m["interp"]["idx"], m["interp"]["w"])[0])
    assert within(et.grad, m["d_equi_tgt"], U * np.abs(m["d_equi_tgt"]) + 2 * U * m["mag_equi_tgt"] + wsum * tol_flat.max() + 1e-30)
    assert torch.count_nonzero(et.grad) > 0 and torch.count_nonzero(es.grad) > 0


# ----------------------------------------------------------------------------------------------- repeatability, capture, network
def _step(crit, inputs):
    for t in inputs[:4]:
        t.grad = None
    total = crit(inputs[0], inputs[1], inputs[4], inputs[2], inputs[3])[0]
    total.backward()
    return [total.detach().clone()] + [t.grad.detach().clone() for t in inputs[:4]]


def test_two_runs_are_bitwise_equal(gpu):
    m = Tf.mirror_case(0.5)
    crit = _criterion(gpu, m, 0.5)
    a, b = _step(crit, _mirror_inputs(gpu, m)), _step(crit, _mirror_inputs(gpu, m))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    src, tgt, margin, _, _ = Tf.bh_case(*Tf.BH_CASES[15])                # N = 193, D = 64
    x, y = run_batch_hard(gpu, src, tgt, "hard", margin), run_batch_hard(gpu, src, tgt, "hard", margin)
    assert torch.equal(x[2], y[2]) and torch.equal(x[3], y[3]) and torch.equal(x[0].loss, y[0].loss)


def test_forward_and_backward_replay_from_a_captured_graph(gpu):
    """Forward + backward of the mirror class at N = 8, D = 32, captured once on one stream (no parallel branches) and replayed
    twice with new values copied into the static inputs: each replay equals the eager result bitwise.  The reference's
    dist_mat[is_neg] synchronises with the host and cannot be captured."""
    N, Dm = 8, 32
    sets = [Tf.descriptors(np.random.default_rng(seed), N, Dm) for seed in (811, 812, 813)]
    m = dict(anchors=Tf.Rf.anchors_for(60), margin=0.3)
    crit = _criterion(gpu, m, 0.0, "soft")
    eager = []
    for src, tgt in sets:
        s, t = D(gpu, src).requires_grad_(), D(gpu, tgt).requires_grad_()
        loss = crit(s, t, None)[0]
        loss.backward()
        eager.append((loss.detach().clone(), s.grad.clone(), t.grad.clone()))
    s, t = D(gpu, sets[0][0]).requires_grad_(), D(gpu, sets[0][1]).requires_grad_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                            # warm-up off the capture, as torch asks
        crit(s, t, None)[0].backward()
    torch.cuda.current_stream().wait_stream(side)
    s.grad = t.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = crit(s, t, None)[0]
        loss.backward()
    for k in (1, 2):
        with torch.no_grad():
            s.copy_(D(gpu, sets[k][0]))
            t.copy_(D(gpu, sets[k][1]))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss.detach(), eager[k][0]) and torch.equal(s.grad, eager[k][1]) and torch.equal(t.grad, eager[k][2])


def test_network_descriptors_train_against_the_loss(gpu):
    """The smallest inv model of the model tests, one forward on two tiny batches of patches, the mirror class's loss,
    backward(): every parameter has a finite gradient, and every parameter the descriptors depend on a gradient that is not
    all zero.

    "Not all zero for EVERY parameter" cannot hold for this architecture under any loss: skip_conv.bias of a block is added
    directly in front of a normalisation that subtracts the per-channel mean (schedule.py: norm(skip_conv(x))), so the
    descriptors do not depend on it and its gradient is identically zero; the block glue skips the add and returns the
    gradient as an exact zero (ops.norm_act).  On an MI355X the four skip_conv.bias of the tiny model are the parameters with
    an all-zero gradient.  They are not exempted by name: for whatever parameters come back all zero, the test shows that
    there is no gradient to find -- shifting all of them by 0.5 leaves both batches of descriptors bitwise unchanged -- and
    that they are biases and fewer than the parameters that do train."""
    from conftest import golden, unit_ball_cloud
    from test_models_cpu import fill_state_dict, product_model
    n = golden("model_inv_tiny.npz")["pts"].shape[1]          # the patch size the tiny model's schedule was built for
    model = fill_state_dict(product_model("inv")).to(gpu).train()
    cloud = unit_ball_cloud(np.random.default_rng(31), 3, n).transpose(0, 2, 1)
    pts = torch.from_numpy(np.ascontiguousarray(cloud)).to(gpu)
    rng = torch.Generator(device=gpu).manual_seed(3)
    pts2 = pts + 0.01 * torch.randn(pts.shape, device=gpu, generator=rng)
    desc_src, _ = model(pts)
    desc_tgt, _ = model(pts2)
    assert desc_src.shape == desc_tgt.shape and desc_src.shape[0] == 3
    m = dict(anchors=model.get_anchor().detach().float().cpu().numpy(), margin=0.5)
    crit = _criterion(gpu, m, 0.0, "soft")
    loss, acc, pos, neg = crit(desc_src, desc_tgt, None)
    loss.backward()
    assert torch.isfinite(loss) and 0.0 <= acc.item() <= 1.0
    params = dict(model.named_parameters())
    assert params and all(p.requires_grad and p.grad is not None for p in params.values()), \
        [k for k, p in params.items() if p.grad is None]
    assert all(torch.isfinite(p.grad).all() for p in params.values())
    zero = [k for k, p in params.items() if torch.count_nonzero(p.grad) == 0]
    print("parameters with an all-zero gradient:", zero)
    assert all(k.endswith(".bias") for k in zero) and 2 * len(zero) < len(params), zero
    with torch.no_grad():
        for k in zero:
            params[k].add_(0.5)
        again_src, again_tgt = model(pts)[0], model(pts2)[0]
    assert torch.equal(again_src, desc_src) and torch.equal(again_tgt, desc_tgt), \
        f"the descriptors depend on {zero}, and the loss gave them no gradient"
