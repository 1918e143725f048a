"""Rotation estimation on the GPU (csrc/rotation_decode.hip behind vgtk.functional and epn_pointcloud_amd.alignment) against the
numpy fp64 restatement of its specification (tests/rotation_ref.py).  The case tables and the conditions the tolerances rest on
(no near tie among the label traces, margin >= 1e-3 for every compared mean) are asserted on the CPU by test_rotation_spec.py.

Tolerances: integers are equal.  Matrices are within 2^-24 absolute: the kernels compute in fp64 and round once, entries are
<= 1 in magnitude, so one fp32 rounding is <= 2^-25, and the fp64 work differs from the restatement's by < 1e-10 at margin >= 1e-3
(the projection moves by at most 2 |dCe| / (s2 +- s3), |dCe| ~ A 2^-53).  conf is within 2^-23 relative, margin within 1e-6,
err within 141.5 * 4.5 * 2^-24 + 2^-22 (slope of acos_safe, nine products halved, the rounding of a value below 4)."""
import ctypes

import numpy as np
import pytest
import torch

import rotation_ref as Rf

pytestmark = pytest.mark.gpu

TOL_R = 2.0 ** -24
TOL_CONF = 2.0 ** -23
TOL_MARGIN = 1e-6
TOL_ERR = 141.5 * 4.5 * 2.0 ** -24 + 2.0 ** -22


def D(gpu, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def H(t):
    return None if t is None else t.cpu().numpy()


def run_decode(gpu, wts, y, anchors, label=None, gt=None):
    from epn_pointcloud_amd import alignment
    return alignment.decode_rotation(D(gpu, wts), D(gpu, y), D(gpu, anchors), D(gpu, label), D(gpu, gt))


def check_decode(got, ref, with_label=True, with_gt=True):
    assert got.preds.dtype == torch.int32 and got.pred_R.dtype == got.conf.dtype == got.margin.dtype == torch.float32
    assert np.array_equal(H(got.preds), ref["preds"])
    assert (np.abs(H(got.conf) - ref["conf"]) <= TOL_CONF * np.abs(ref["conf"])).all()
    assert np.abs(H(got.pred_Rs) - ref["pred_Rs"]).max() <= TOL_R
    assert np.abs(H(got.pred_R) - ref["pred_R"]).max() <= TOL_R
    assert np.abs(H(got.margin) - ref["margin"]).max() <= TOL_MARGIN
    if with_label:
        assert got.hits.dtype == torch.int32 and np.array_equal(H(got.hits), ref["hits"])
    else:
        assert got.hits is None
    if with_gt:
        assert np.abs(H(got.err) - ref["err"]).max() <= TOL_ERR
    else:
        assert got.err is None


# ----------------------------------------------------------------------------------------------- labels
@pytest.mark.parametrize("case", Rf.LABEL_CASES, ids=str)
def test_labels(gpu, case):
    import epn_pointcloud_amd.vgtk.functional as F
    anchors, T, (R_target, label, _) = Rf.label_case(*case)
    got_R, got_label = F.label_relative_rotation(D(gpu, anchors), D(gpu, T))
    assert got_label.dtype == torch.int32 and got_R.shape == R_target.shape
    assert np.array_equal(H(got_label), label)
    assert np.abs(H(got_R) - R_target).max() <= TOL_R


@pytest.mark.parametrize("A", [12, 60])
def test_labels_known_answers(gpu, A):
    """T = I labels every anchor with itself; T = A_j A_k^T (the fp64 product of the fp32 tables, rounded to fp32) gives a
    permutation of 0..A-1 with R_target = I up to the tables' defect.  Two quantities, both computed and printed here: the
    tables' ORTHOGONALITY defect max_a |A_a^T A_a - I| (rotation_ref.orthogonality_defect: 1.4e-7 for the 12 anchors, 1.6e-7
    for the 60) and their CLOSURE defect max |A_a^T (A_j A_k^T) A_i - I| over the labelled triples, which is what R_target - I
    is made of and is the bound used (1.34e-6 and 1.30e-6: the reference's fp32 tables are each orthogonal to fp32 but form a
    group only to about 1e-6; the closure defect is at most a few times the largest rounding of a table entry and is asserted
    below 1e-5 and above the orthogonality defect).  The closure defect comes from the fp64 restatement on the same T; the
    device may add its one rounding, 2^-24.  The permutation and identity checks do not involve the restatement.  A single
    [3,3] T returns unbatched results."""
    import epn_pointcloud_amd.vgtk.functional as F
    anchors = Rf.anchors_for(A)
    an = anchors.astype(np.float64)
    R1, l1 = F.label_relative_rotation(D(gpu, anchors), torch.eye(3, device=gpu))
    assert R1.shape == (A, 3, 3) and H(l1).tolist() == list(range(A))
    pairs = [(0, 1), (A - 1, 2), (5, 5), (7, A // 2)]
    T = np.stack([an[j] @ an[k].T for j, k in pairs]).astype(np.float32)
    ref_R, ref_label, gap = Rf.label_relative_rotation(anchors, T)
    defect = np.abs(ref_R - np.eye(3)).max()
    ortho = Rf.orthogonality_defect(anchors)
    print(f"A={A}: orthogonality defect {ortho:.3e}, closure defect through A_a^T (A_j A_k^T) A_i {defect:.3e}")
    assert gap.min() > 0.1 and ortho <= defect < 1e-5
    got_R, got_label = F.label_relative_rotation(D(gpu, anchors), D(gpu, T))
    got_label = H(got_label)
    assert np.array_equal(got_label, ref_label)
    assert all(sorted(row.tolist()) == list(range(A)) for row in got_label)
    assert np.abs(H(got_R) - np.eye(3)).max() <= defect + TOL_R
    assert got_label[2].tolist() == list(range(A))               # j == k: T = A_5 A_5^T = I up to rounding


# ----------------------------------------------------------------------------------------------- mean
@pytest.mark.parametrize("case", Rf.MEAN_CASES, ids=str)
def test_so3_mean(gpu, case):
    import epn_pointcloud_amd.vgtk.functional as F
    Rs, weights, (R, margin) = Rf.mean_case(*case)
    got_R, got_margin = F.so3_mean(D(gpu, Rs), D(gpu, weights), return_margin=True)
    assert got_R.dtype == got_margin.dtype == torch.float32
    assert np.abs(H(got_R) - R).max() <= TOL_R
    assert np.abs(H(got_margin) - margin).max() <= TOL_MARGIN
    assert torch.equal(F.so3_mean(D(gpu, Rs), D(gpu, weights)), got_R)


def test_so3_mean_low_margin(gpu):
    """Two opposed rotations (R and R turned by pi about an axis) with equal weights: the mean is not unique.  What comes
    back is still a rotation and margin says so; nothing else is compared.  All-zero weights: R = I, margin = 0."""
    import epn_pointcloud_amd.vgtk.functional as F
    rng = np.random.default_rng(9)
    base = Rf.random_rotations(rng, 3)
    half_turn = np.stack([np.diag([1.0, -1.0, -1.0]), np.diag([-1.0, 1.0, -1.0]), np.diag([-1.0, -1.0, 1.0])])
    Rs = np.stack((base, base @ half_turn), axis=1).astype(np.float32)             # [3, 2, 3, 3]
    for weights in (None, np.full((3, 2), 0.5, np.float32)):
        R, margin = F.so3_mean(D(gpu, Rs), D(gpu, weights), return_margin=True)
        R, margin = H(R).astype(np.float64), H(margin)
        assert np.abs(np.einsum('bji,bjk->bik', R, R) - np.eye(3)).max() <= 1e-6
        assert (np.linalg.det(R) > 0).all()
        assert (margin < 1e-3).all() and (margin >= 0).all()
    R, margin = F.so3_mean(D(gpu, Rs), torch.zeros(3, 2, device=gpu), return_margin=True)
    assert np.array_equal(H(R), np.broadcast_to(np.eye(3, dtype=np.float32), (3, 3, 3))) and (H(margin) == 0).all()


# ----------------------------------------------------------------------------------------------- decode
@pytest.mark.parametrize("case", Rf.DECODE_CASES, ids=str)
def test_decode(gpu, case):
    wts, y, anchors, label, T, ref = Rf.decode_case(*case)
    check_decode(run_decode(gpu, wts, y, anchors, label, T), ref)


def test_decode_optional_arguments(gpu):
    """Without label there are no hits, without gt no err; a host label and int64 labels are accepted; the other outputs do
    not depend on either."""
    wts, y, anchors, label, T, ref = Rf.decode_case(*Rf.DECODE_CASES[14])
    full = run_decode(gpu, wts, y, anchors, label, T)
    bare = run_decode(gpu, wts, y, anchors)
    check_decode(bare, ref, with_label=False, with_gt=False)
    from epn_pointcloud_amd import alignment
    host = alignment.decode_rotation(D(gpu, wts), D(gpu, y), D(gpu, anchors), torch.from_numpy(label).long(), None)
    check_decode(host, ref, with_gt=False)
    for a, b in zip(full[:5], bare[:5]):
        assert torch.equal(a, b)
    assert torch.equal(host.hits, full.hits)
    empty = alignment.decode_rotation(D(gpu, wts[:0]), D(gpu, y[:0]), D(gpu, anchors), gt=D(gpu, T[:0]))
    assert empty.pred_R.shape == (0, 3, 3) and empty.err.shape == (0,) and empty.hits is None


def test_mean_angular_error(gpu):
    import epn_pointcloud_amd.vgtk.functional as F
    wts, y, anchors, label, T, ref = Rf.decode_case(*Rf.DECODE_CASES[15])
    got = run_decode(gpu, wts, y, anchors, label, T)
    err = F.mean_angular_error(got.pred_R, D(gpu, T))
    want = Rf.acos_safe(0.5 * ((H(got.pred_R).astype(np.float64) * T.astype(np.float64)).sum(axis=(1, 2)) - 1))
    assert err.dtype == torch.float32 and np.abs(H(err) - want).max() <= 2.0 ** -22
    assert np.abs(H(err) - ref["err"]).max() <= TOL_ERR           # from the rounded pred_R (nine roundings of 2^-25, halved)


@pytest.mark.parametrize("A", [1, 12, 60, 64])
@pytest.mark.parametrize("nr", [4, 6])
def test_round_trip(gpu, A, nr):
    """Labels from the device for random T, an ideal head output built from them (wts peaked at the label, y the quaternion
    or 6-d form of R_target[a]), decode: T comes back.  The restatement's own defect on these cases, which fp32 anchors, T and
    y leave, is 2.2e-8 to 3.3e-8 in pred_R and 3.9e-6 rad in err (test_rotation_spec.py prints and bounds them); the device may
    be off by four times the value measured here."""
    import epn_pointcloud_amd.vgtk.functional as F
    case = Rf.round_trip_case(A, nr)
    wts, y, anchors, label, T, ref = case
    dR, derr = Rf.round_trip_defect(case)
    got_R, got_label = F.label_relative_rotation(D(gpu, anchors), D(gpu, T))
    assert np.array_equal(H(got_label), label)
    R_target = H(got_R).astype(np.float64)
    ideal = Rf.rot_to_quat(R_target) if nr == 4 else np.concatenate((R_target[..., 0], R_target[..., 1]), axis=-1)   # [b, A, nr]
    y_dev = np.ascontiguousarray(np.broadcast_to(ideal.transpose(0, 2, 1)[:, :, None, :], y.shape).astype(np.float32))
    got = run_decode(gpu, wts, y_dev, anchors, label, T)
    assert np.array_equal(H(got.preds), label) and (H(got.hits) == A).all()
    assert np.abs(H(got.pred_R) - T).max() <= 4 * dR
    assert np.abs(H(got.err)).max() <= 4 * derr


def test_ties_go_to_the_lower_target_anchor(gpu):
    """Two target rows of wts are duplicates and hold the maximum of most columns; y differs between them, so the choice
    shows in every output.  The lower row wins, as in the restatement (np.argmax: the first maximum)."""
    wts, y, anchors, label, T, _ = Rf.decode_case(*Rf.DECODE_CASES[14])
    wts = wts.copy()
    lo, hi = 7, 41
    wts[:, lo, ::2] += np.float32(1.0)
    wts[:, hi] = wts[:, lo]
    ref = Rf.decode(wts, y, anchors, label, T)
    assert (ref["preds"][:, ::2] == lo).all() and not (ref["preds"] == hi).any() and ref["margin"].min() >= Rf.MIN_MARGIN
    check_decode(run_decode(gpu, wts, y, anchors, label, T), ref)


def _raw_decode(gpu, wts, y, anchors, label, T, guard=64):
    """The C entry on sentinel-filled buffers with `guard` elements either side of every output.  -> (outputs, guards intact)."""
    from epn_pointcloud_amd import _lib
    b, A, nr = wts.shape[0], wts.shape[1], y.shape[1]
    ins = [D(gpu, wts), D(gpu, y), D(gpu, anchors), D(gpu, label), D(gpu, T)]
    sizes = dict(pred_R=(9 * b, torch.float32), preds=(b * A, torch.int32), conf=(b * A, torch.float32), margin=(b, torch.float32),
                 pred_Rs=(9 * b * A, torch.float32), hits=(b, torch.int32), err=(b, torch.float32))
    bufs = {k: torch.full((n + 2 * guard,), -777, dtype=dt, device=gpu) for k, (n, dt) in sizes.items()}
    ptr = lambda k: ctypes.c_void_p(bufs[k].data_ptr() + 4 * guard)
    p = _lib.dev_ptr
    rc = _lib.get_lib().epn_rotation_decode_f32(p(ins[0], "wts"), p(ins[1], "y"), p(ins[2], "anchors"), p(ins[3], "label", torch.int32),
                                                p(ins[4], "gt_T"), b, A, nr, ptr("pred_R"), ptr("preds"), ptr("conf"), ptr("margin"),
                                                ptr("pred_Rs"), ptr("hits"), ptr("err"), _lib.stream_of(ins[0]))
    assert rc == 0
    torch.cuda.synchronize()
    intact = all((v[:guard] == -777).all().item() and (v[-guard:] == -777).all().item() for v in bufs.values())
    return {k: v[guard:-guard].cpu().numpy() for k, v in bufs.items()}, intact


@pytest.mark.nonfinite_inputs
@pytest.mark.parametrize("nr", [4, 6])
def test_poisoned_pair_stays_alone(gpu, nr):
    """NaN in wts and inf in y of the middle pair of three: the other two pairs' rows are bit-identical to the clean run, the
    poisoned pair's preds still lie in 0..A-1, every output element of the three pairs is written and nothing around the
    output buffers changes."""
    wts, y, anchors, label, T, _ = Rf.decode_case(60, 3, nr, 990 + nr)
    clean, ok = _raw_decode(gpu, wts, y, anchors, label, T)
    assert ok
    wts, y = wts.copy(), y.copy()
    wts[1, ::3, 1::2] = np.nan
    wts[1, 0, 0] = np.nan
    y[1, :, 5::7] = np.inf
    y[1, 0, 3] = -np.inf
    dirty, ok = _raw_decode(gpu, wts, y, anchors, label, T)
    assert ok
    b, A = 3, 60
    rows = dict(pred_R=9, preds=A, conf=A, margin=1, pred_Rs=9 * A, hits=1, err=1)
    for k, n in rows.items():
        c, d = clean[k].reshape(b, n), dirty[k].reshape(b, n)
        assert np.array_equal(c[[0, 2]].view(np.uint32), d[[0, 2]].view(np.uint32)), k
        assert not (c == -777).any() and not (d == -777).any(), k               # every element written (NaN != -777)
    p1 = dirty["preds"].reshape(b, A)[1]
    assert ((0 <= p1) & (p1 < A)).all()


def test_two_runs_are_bitwise_equal(gpu):
    import epn_pointcloud_amd.vgtk.functional as F
    wts, y, anchors, label, T, _ = Rf.decode_case(*Rf.DECODE_CASES[17])
    first, second = (run_decode(gpu, wts, y, anchors, label, T) for _ in range(2))
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    Rs, weights, _ = Rf.mean_case(*Rf.MEAN_CASES[17])
    m1, m2 = (F.so3_mean(D(gpu, Rs), D(gpu, weights), return_margin=True) for _ in range(2))
    assert torch.equal(m1[0], m2[0]) and torch.equal(m1[1], m2[1])
    anchors, T, _ = Rf.label_case(*Rf.LABEL_CASES[8])
    l1, l2 = (F.label_relative_rotation(D(gpu, anchors), D(gpu, T)) for _ in range(2))
    assert torch.equal(l1[0], l2[0]) and torch.equal(l1[1], l2[1])


# ----------------------------------------------------------------------------------------------- model level
def _tiny_reg(gpu):
    from test_models_cpu import fill_state_dict, product_model
    return fill_state_dict(product_model("reg")).to(gpu)


def _pairs(k, n, seed):
    from conftest import unit_ball_cloud
    rng = np.random.default_rng(seed)
    tgt = unit_ball_cloud(rng, k, n).transpose(0, 2, 1)                                 # [k, n, 3]
    T = Rf.random_rotations(rng, k).astype(np.float32)
    src = np.einsum('kij,knj->kni', T, tgt).astype(np.float32)
    return np.ascontiguousarray(src), np.ascontiguousarray(tgt), T


def test_estimate_rotation(gpu):
    """k = 5 pairs, batch = 2: two full batches and one padded with a zero pair.  Every row equals decode_rotation(*model(x))
    on the same batches bit for bit, the padded row is dropped, training mode raises."""
    from epn_pointcloud_amd import alignment
    m = _tiny_reg(gpu)
    src, tgt, _ = _pairs(5, 256, 21)
    src, tgt = D(gpu, src), D(gpu, tgt)
    with pytest.raises(RuntimeError, match="eval"):
        m.train().estimate_rotation(src, tgt, batch=2)
    m.eval()
    R, margin, preds, conf = m.estimate_rotation(src, tgt, batch=2)
    assert R.shape == (5, 3, 3) and margin.shape == (5,) and preds.shape == (5, 60) and conf.shape == (5, 60)
    assert preds.dtype == torch.int32 and torch.isfinite(R).all() and not R.requires_grad
    assert (R.transpose(1, 2) @ R - torch.eye(3, device=gpu)).abs().max().item() <= 1e-6
    anchors = m.get_anchor()
    with torch.no_grad():
        for r0 in (0, 2, 4):
            x = torch.stack((src[r0:r0 + 2], tgt[r0:r0 + 2]), dim=1)
            rows = x.shape[0]
            if rows < 2:
                x = torch.cat((x, x.new_zeros(1, 2, 256, 3)))
            d = alignment.decode_rotation(*m(x), anchors)
            assert d.pred_R.shape[0] == 2
            assert torch.equal(d.pred_R[:rows], R[r0:r0 + rows]) and torch.equal(d.margin[:rows], margin[r0:r0 + rows])
            assert torch.equal(d.preds[:rows], preds[r0:r0 + rows]) and torch.equal(d.conf[:rows], conf[r0:r0 + rows])
    one = m.estimate_rotation(src[:1], tgt[:1])                   # batch = 32: one batch, 31 padded rows
    assert one[0].shape == (1, 3, 3) and one[2].shape == (1, 60)


def test_evaluate_alignment(gpu):
    """Clouds rotated by a known T through an untrained model: finite errors in [0, pi + slack], the documented shapes, the
    accuracy a count over k * A anchors, the median in degrees of the same errors.  What an untrained model scores is not
    asserted."""
    from epn_pointcloud_amd import alignment
    m = _tiny_reg(gpu).eval()
    src, tgt, T = _pairs(3, 256, 22)
    r = alignment.evaluate_alignment(m, D(gpu, src), D(gpu, tgt), D(gpu, T), batch=2)
    assert isinstance(r.errors, np.ndarray) and r.errors.shape == (3,) and r.errors.dtype == np.float32
    assert np.isfinite(r.errors).all() and (r.errors > -1e-3).all() and (r.errors < np.pi + 1e-3).all()
    assert 0.0 <= r.accuracy <= 1.0 and abs(r.accuracy * 180 - round(r.accuracy * 180)) < 1e-9
    assert r.median_deg == pytest.approx(float(np.median(r.errors)) * 180 / np.pi)
    assert r.pred_R.shape == (3, 3, 3) and r.margin.shape == (3,)
    R, margin, _, _ = m.estimate_rotation(D(gpu, src), D(gpu, tgt), batch=2)
    assert torch.equal(R, r.pred_R) and torch.equal(margin, r.margin)
