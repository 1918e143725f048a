"""The training loss of the descriptor network without a GPU: the numpy fp64 restatement (tests/triplet_ref.py) against the
reference's own results (tests/golden/triplet_loss.npz, gen_golden_triplet.py), the conditions test_gpu_triplet.py's tolerances
rest on, asserted for every case of the tables, and the refusals of epn_pointcloud_amd.losses and the mirror class.

Tolerances against the golden.  The reference works in fp32 from the expansion |x|^2 + |y|^2 - 2 x.y; the fixture stores the
largest difference between its distance matrix and the restatement's on the recorded inputs (dist_err, measured when the
fixture was written, 5.7e-7).  FACTOR = 4 throughout:
  values     every output is a distance, a mean of distances or a 1-Lipschitz function of two of them (relu, softplus), so it
             is within 2 dist_err of the restatement; a factor 2 on top for the reference's own fp32 sums and roundings.
  gradients  an element is (1/N) g (s - t) / d summed over at most a few rows, |g| <= 1, |s - t| <= d.  Dividing by a distance
             that is off by dist_err moves it by dist_err / (N d_min); the reference's autograd forms 2 g (x - y) / (2 d) from
             fp32 products of entries below 1, another 2^-22 / (N d_min).  FACTOR covers the rows that meet in one tgt row.
  interpolation  trace_err (2.8e-7, stored likewise) is the largest difference of the top-3 traces.  A softmax weight moves by
             at most 2 trace_err / sigma, the output by that times the sum of the three |features|; FACTOR covers the
             reference's fp32 softmax and sum."""
import types

import numpy as np
import pytest
import torch

import triplet_ref as Tf
from conftest import golden

FACTOR = 4.0


@pytest.fixture(scope="module")
def G():
    return golden("triplet_loss.npz")


# ----------------------------------------------------------------------------------------------- restatement against the golden
@pytest.mark.parametrize("mode", Tf.MODES)
def test_batch_hard_restatement_matches_the_reference(G, mode):
    src, tgt, margin, err = G["src"], G["tgt"], float(G[f"{mode}_margin"]), float(G["dist_err"])
    assert margin == Tf.margin_for(src, tgt, mode)
    fwd = Tf.batch_hard(src, tgt, mode, margin)
    dsrc, dtgt, _, _ = Tf.batch_hard_bwd(1.0, src, tgt, fwd, mode, margin)
    assert np.array_equal(fwd["nn_idx"], G[f"{mode}_match_idx"][:, 0])
    tol = FACTOR * err
    got = fwd["scalars"]
    print(f"{mode}: |scalars - golden| {np.abs(got - G[f'{mode}_out'])}, tol {tol:.2e}")
    assert np.abs(got - G[f"{mode}_out"]).max() <= tol
    assert got[1] == G[f"{mode}_out"][1]
    assert np.abs(fwd["d_pos"] - G[f"{mode}_fpos"]).max() <= tol
    assert np.abs(fwd["d_neg"] - G[f"{mode}_cneg"]).max() <= tol
    N = src.shape[0]
    d_min = min(fwd["d_pos"].min(), fwd["d_neg"].min())
    gtol = FACTOR * (err + 2.0 ** -22) / (N * d_min)
    e_s, e_t = np.abs(dsrc - G[f"{mode}_dsrc"]).max(), np.abs(dtgt - G[f"{mode}_dtgt"]).max()
    print(f"{mode}: max |dsrc - golden| {e_s:.2e}, max |dtgt - golden| {e_t:.2e}, tol {gtol:.2e}, max |dsrc| {np.abs(dsrc).max():.2e}")
    assert e_s <= gtol and e_t <= gtol
    assert np.abs(G[f"{mode}_dsrc"]).max() > 100 * gtol                  # the comparison says something


def test_golden_hard_case_has_active_and_inactive_rows(G):
    fwd = Tf.batch_hard(G["src"], G["tgt"], "hard", float(G["hard_margin"]))
    active = (fwd["row_flags"] & Tf.FLAG_HINGE_ACTIVE) != 0
    assert active.any() and not active.all()


def test_interpolation_restatement_matches_the_reference(G):
    """Every nb = 1 golden one by one; then the restatement at nb = 3 equals the three nb = 1 results stacked, which is the
    per-sample semantics the reference's commented-out line intends."""
    T, f, anchors, err = G["interp_T"], G["interp_feature"], G["anchors"], float(G["trace_err"])
    singles = []
    for b in range(T.shape[0]):
        r = Tf.anchor_interp(f[b:b + 1], T[b:b + 1], anchors, Tf.SIGMA)
        assert r["trace_gap"] > Tf.TRACE_GAP
        assert np.array_equal(r["idx"][0], G["interp_idx"][b])
        tol = FACTOR * 2 * err / Tf.SIGMA * np.abs(f[b].astype(np.float64)[:, r["idx"][0]]).sum(-1)
        diff = np.abs(r["out"][0] - G["interp_out"][b])
        print(f"T {b}: max |out - golden| {diff.max():.2e}, smallest tol {tol.min():.2e}")
        assert (diff <= tol + 1e-7).all()
        singles.append(r)
    batch = Tf.anchor_interp(f[:3], T[:3], anchors, Tf.SIGMA)
    for key in ("out", "idx", "w"):
        assert np.array_equal(batch[key], np.concatenate([s[key] for s in singles[:3]]))
    rolled = Tf.anchor_interp(f[:3], T[[1, 2, 0]], anchors, Tf.SIGMA)       # the neighbours follow the sample's own T
    assert not np.array_equal(rolled["idx"], batch["idx"])


def test_expansion_form_loses_what_the_direct_form_keeps(G):
    """Why the entry works from the differences: on the golden's inputs the fp32 expansion is dist_err away from the fp64
    distances, more than the 2^-24 relative one rounding of the direct fp64 form leaves."""
    dist, _ = Tf.distances(G["src"], G["tgt"])
    assert float(G["dist_err"]) > 2.0 ** -24 * dist.max()


# ----------------------------------------------------------------------------------------------- conditions of the GPU tolerances
def _check_conditions(fwd, mode, exempt_rows=(), zero_ok=False, both=True):
    keep = np.ones(fwd["d_pos"].shape[0], bool)
    keep[list(exempt_rows)] = False
    assert (fwd["neg_gap"][keep] > Tf.ARG_GAP).all() and (fwd["nn_gap"][keep] > Tf.ARG_GAP).all()
    assert (fwd["kink"] > Tf.KINK_GAP).all()
    d2 = fwd["d2"]
    near = (d2 > Tf.EPS / 2) & (d2 < Tf.EPS * 2)
    assert not near.any()
    if not zero_ok:
        assert (d2 >= Tf.EPS * 2).all()
    if mode == "hard" and both:
        active = (fwd["row_flags"] & Tf.FLAG_HINGE_ACTIVE) != 0
        assert active.any() and not active.all()


@pytest.mark.parametrize("case", Tf.BH_CASES, ids=str)
def test_batch_hard_cases_are_well_conditioned(case):
    src, tgt, margin, fwd, _ = Tf.bh_case(*case)
    assert src.dtype == tgt.dtype == np.float32 and src.shape == tgt.shape == case[:2]
    _check_conditions(fwd, case[2])
    assert fwd["neg_idx"].min() >= 0 and (fwd["neg_idx"] != np.arange(case[0])).all()


def test_built_cases_are_what_they_claim():
    src, tgt, mode, margin, fwd, _ = Tf.built_case("dup")
    assert np.array_equal(tgt[2], tgt[5]) and fwd["neg_idx"][0] == 2 and fwd["nn_idx"][0] == 2
    assert fwd["d2"][0, 2] == fwd["d2"][0, 5] == fwd["d2"][0].min()      # an exact tie, and it is the minimum
    tied = [i for i in range(8) if fwd["neg_idx"][i] in (2, 5) or fwd["nn_idx"][i] in (2, 5)]
    _check_conditions(fwd, mode, exempt_rows=tied)
    src, tgt, mode, margin, fwd, (dsrc, dtgt, _, _) = Tf.built_case("zero")
    assert np.array_equal(src[3], tgt[3]) and fwd["d2"][3, 3] == 0.0 and fwd["d_pos"][3] == np.sqrt(Tf.EPS)
    assert fwd["row_flags"][3] & Tf.FLAG_POS_CLAMPED and not (fwd["row_flags"] & Tf.FLAG_NEG_CLAMPED).any()
    _check_conditions(fwd, mode, zero_ok=True)
    src, tgt, mode, margin, fwd, _ = Tf.built_case("crowd")
    assert (fwd["neg_idx"][1:] == 0).all() and src.shape == (1030, 257)      # 1029 rows > one round of the backward's list
    _check_conditions(fwd, mode)
    src, tgt, mode, margin, fwd, _ = Tf.built_case("soft")
    bx = margin * (fwd["d_pos"] - fwd["d_neg"])
    assert mode == "soft" and margin == 16.0 and (bx > 20).sum() >= 2 and (bx < 20).sum() >= 2
    _check_conditions(fwd, mode)


@pytest.mark.parametrize("case", Tf.INTERP_CASES, ids=str)
def test_interpolation_cases_are_well_conditioned(case):
    feature, T, anchors, dout, fwd, _ = Tf.interp_case(*case)
    assert fwd["trace_gap"] > Tf.TRACE_GAP
    assert np.abs(fwd["w"].sum(-1) - 1).max() < 1e-12 and fwd["idx"].min() >= 0 and fwd["idx"].max() < case[2]


@pytest.mark.parametrize("alpha", [0.0, 0.5])
def test_mirror_case_is_well_conditioned(alpha):
    m = Tf.mirror_case(alpha)
    _check_conditions(m["inv"], "hard")
    if alpha > 0:
        _check_conditions(m["equi"], "hard", both=False)     # the margin was split on the invariant term
        assert m["interp"]["trace_gap"] > Tf.TRACE_GAP


# ----------------------------------------------------------------------------------------------- refusals, on host tensors
def _opt(loss_type="hard", margin=0.5):
    return types.SimpleNamespace(device="cpu", train_loss=types.SimpleNamespace(loss_type=loss_type, margin=margin))


def test_batch_hard_refusals():
    from epn_pointcloud_amd import losses
    x = torch.zeros(4, 8)
    with pytest.raises(ValueError, match="N >= 2"):
        losses.batch_hard_triplet(torch.zeros(1, 8), torch.zeros(1, 8))
    with pytest.raises(ValueError, match="differ in shape"):
        losses.batch_hard_triplet(x, torch.zeros(4, 9))
    with pytest.raises(ValueError):
        losses.batch_hard_triplet(torch.zeros(4), torch.zeros(4))
    with pytest.raises(TypeError, match="float32"):
        losses.batch_hard_triplet(x.double(), x.double())
    with pytest.raises(TypeError, match="float32"):
        losses.batch_hard_triplet(x, x.half())
    with pytest.raises(TypeError):
        losses.batch_hard_triplet(x.numpy(), x)
    with pytest.raises(ValueError, match="mode"):
        losses.batch_hard_triplet(x, x, mode="semi-hard")
    with pytest.raises(ValueError, match="margin"):
        losses.batch_hard_triplet(x, x, mode="soft", margin=0.0)
    with pytest.raises(ValueError, match="margin"):
        losses.batch_hard_triplet(x, x, margin=float("nan"))
    with pytest.raises(RuntimeError, match="CUDA"):                        # no CPU fallback
        losses.batch_hard_triplet(x, x)


def test_interpolation_refusals():
    from epn_pointcloud_amd import losses
    f, T, an = torch.zeros(2, 4, 60), torch.eye(3).repeat(2, 1, 1), torch.eye(3).repeat(60, 1, 1)
    with pytest.raises(ValueError, match="A in"):
        losses.interpolate_anchor_features(torch.zeros(2, 4, 7), T, torch.eye(3).repeat(7, 1, 1))
    with pytest.raises(ValueError):
        losses.interpolate_anchor_features(torch.zeros(2, 4, 12), T, an)
    with pytest.raises(ValueError):
        losses.interpolate_anchor_features(f, torch.eye(3).repeat(3, 1, 1), an)
    with pytest.raises(ValueError):
        losses.interpolate_anchor_features(f, torch.zeros(2, 3, 4), an)
    with pytest.raises(TypeError, match="float32"):
        losses.interpolate_anchor_features(f.double(), T, an)
    with pytest.raises(ValueError, match="sigma"):
        losses.interpolate_anchor_features(f, T, an, sigma=0.0)
    with pytest.raises(RuntimeError, match="CUDA"):
        losses.interpolate_anchor_features(f, torch.eye(4).repeat(2, 1, 1), an)


def test_mirror_class_signature_and_refusals(vgtk_alias):
    import inspect
    import vgtk
    from vgtk.loss import TripletBatchLoss
    assert vgtk.TripletBatchLoss is TripletBatchLoss
    assert list(inspect.signature(TripletBatchLoss.__init__).parameters) == ["self", "opt", "anchors", "sigma", "interpolation", "alpha"]
    assert list(inspect.signature(TripletBatchLoss.forward).parameters) == ["self", "src", "tgt", "T", "equi_src", "equi_tgt"]
    an = torch.eye(3).repeat(60, 1, 1)
    crit = TripletBatchLoss(_opt("soft", 2.0), an, alpha=0.5)
    assert (crit.loss, crit.margin, crit.sigma, crit.alpha, crit.k_precision) == ("soft", 2.0, 0.2, 0.5, 1)
    assert "anchors" in dict(crit.named_buffers()) and not hasattr(crit, "_forward_attention")
    with pytest.raises(ValueError, match="loss_type"):
        TripletBatchLoss(_opt("none"), an)
    with pytest.raises(ValueError, match="N >= 2"):
        crit(torch.zeros(1, 8), torch.zeros(1, 8), None)
    with pytest.raises(ValueError, match="knn"):
        crit._interpolate(torch.zeros(2, 4, 60), torch.eye(3).repeat(2, 1, 1), knn=4)


def test_mirror_class_without_both_equivariant_features_takes_the_invariance_form(vgtk_alias, monkeypatch):
    """alpha > 0 with one equivariant feature missing falls back to the invariance form, as upstream does."""
    from epn_pointcloud_amd import losses
    from vgtk.loss import TripletBatchLoss
    calls = []

    def fake_rows(src, tgt, mode, margin):
        calls.append((tuple(src.shape), mode, margin))
        z = torch.zeros(())
        n = torch.zeros(src.shape[0], dtype=torch.int32)
        return losses.TripletResult(z, z, z, z, n, n), dict(d_pos=n.float(), d_neg=n.float())
    monkeypatch.setattr(losses, "batch_hard_rows", fake_rows)
    monkeypatch.setattr(losses, "interpolate_anchor_features", lambda *a, **k: pytest.fail("the equivariance form ran"))
    crit = TripletBatchLoss(_opt("hard", 0.5), torch.eye(3).repeat(60, 1, 1), alpha=0.5)
    x, e = torch.zeros(4, 8), torch.zeros(4, 2, 60)
    for kw in (dict(equi_src=e), dict(equi_tgt=e), dict()):
        out = crit(x, x, None, **kw)
        assert isinstance(out, tuple) and len(out) == 4
    assert calls == [((4, 8), "hard", 0.5)] * 3
    assert crit.match_idx.shape == (4, 1) and crit.fpos.shape == crit.cneg.shape == (4,)
