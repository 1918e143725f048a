"""3DMatch batches on the device (csrc/pair_batch.hip through epn_pointcloud_amd.data.fragment_pair_batch) against the numpy
restatement (tests/pair_batch_ref.py) and against the library's own patch extraction, one fragment and one keypoint at a time.

Exact: idx, counts and choice (with key_bits = 2 that is the tie rule across chunk and wave boundaries); the patch values against
the restatement evaluated from the device's own R_aug (three exact fp64 products of fp32 values, two additions, one rounding:
no room for a difference); every output between two calls, under a permutation of the samples, and between a graph replay and
the eager call.  Within 2^-23 (pair_batch_ref.TOL): R_aug, T and T_aug -- entries of magnitude <= 1, one fp32 rounding of an
fp64 result; fp64 sin / cos or a contracted multiply-add may differ in the last place before that rounding.

Shapes: fragments of 1, 255, 256, 257 and 700 points and an empty one (the sweep's chunk is 256 points); n_sample 1, 8, 64 with
keypoints whose patches hold 0, 1, 2, fewer than, exactly and more than n_sample points; npt 1 and 3; B 1 and 3 with fragment 4
shared by two samples and one sample whose source is its target."""
import functools

import numpy as np
import pytest
import torch

import pair_batch_ref as Pr

pytestmark = pytest.mark.gpu

SEED = 2913
RADIUS = 0.3
FIELDS = ("src", "tgt", "idx", "counts", "choice", "T", "R_aug", "T_aug", "status")
SIZES = (1, 255, 256, 257, 700, 0)
PAIRS = {1: [(4, 3)], 3: [(4, 3), (2, 4), (1, 1)]}             # fragment 4 twice; source == target


@functools.lru_cache(maxsize=None)
def _scene():
    """Six fragments: points uniform in the unit cube seen from six poses -> (points, offsets, poses)."""
    rng = np.random.default_rng(77)
    frags, poses = [], []
    for n in SIZES:
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        pose = np.eye(4)
        pose[:3, :3], pose[:3, 3] = q * np.sign(np.linalg.det(q)), rng.standard_normal(3)
        poses.append(pose)
        frags.append(((rng.random((n, 3)) - pose[:3, 3]) @ pose[:3, :3]).astype(np.float32))
    off = np.concatenate(([0], np.cumsum(SIZES))).astype(np.int32)
    return np.concatenate(frags), off, np.stack(poses)


def _frame(world, pose):
    return ((world - pose[:3, 3]) @ pose[:3, :3]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _batch(B):
    """(pairs, corr, corr_offsets): per sample 5 correspondences, scene points inside and outside the cube so that full, thin
    and empty patches occur."""
    _, _, poses = _scene()
    rng = np.random.default_rng(500 + B)
    corr = []
    for a, b in PAIRS[B]:
        world = rng.random((5, 3)) * 1.5 - 0.25
        corr.append(np.stack((_frame(world, poses[a]), _frame(world, poses[b])), axis=1))
    coff = np.arange(len(corr) + 1, dtype=np.int32) * 5
    return np.asarray(PAIRS[B], dtype=np.int32), np.concatenate(corr), coff


def _dev(gpu, a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(gpu)


def _run(gpu, points, off, pairs, corr, coff, poses, n_sample, npt, radius=RADIUS, ids=None, **kw):
    from epn_pointcloud_amd import data
    ids = None if ids is None else _dev(gpu, ids, np.int64)
    return data.fragment_pair_batch(_dev(gpu, points, np.float32), _dev(gpu, off, np.int32), _dev(gpu, pairs, np.int32).view(-1, 2),
                                    _dev(gpu, corr, np.float32).view(-1, 2, 3), _dev(gpu, coff, np.int32), _dev(gpu, poses), n_sample,
                                    npt, radius, ids=ids, **kw)


def _np(out):
    return {k: getattr(out, k).cpu().numpy() for k in FIELDS}


def _bitwise(a, b, fields=FIELDS):
    return [k for k in fields if not np.array_equal(a[k].view(np.int32), b[k].view(np.int32))]


def _close(got, want, name):
    err = float(np.abs(got.astype(np.float64) - np.asarray(want, dtype=np.float64)).max()) if got.size else 0.0
    print(f"{name}: max |device - expected| = {err:.3e} (bound {Pr.TOL:.3e})")
    assert err <= Pr.TOL, name


def _check(gpu, inputs, n_sample, npt, ids, **kw):
    """One call against the restatement and against radius_patches; -> (device outputs, restatement)."""
    points, off, pairs, corr, coff, poses = inputs
    out = _np(_run(gpu, *inputs, n_sample, npt, ids=ids, seed=SEED, **kw))
    ref = Pr.fragment_pair_batch(*inputs, n_sample, npt, RADIUS, seed=SEED, ids=ids, max_degree=kw.get("max_degree", 30),
                                 center=int(kw.get("center", False)), key_bits=kw.get("key_bits", 32))
    B = len(pairs)
    assert out["src"].shape == (B, npt, n_sample, 3) == out["tgt"].shape and out["idx"].shape == (B, 2, npt, n_sample)
    assert out["counts"].shape == (B, 2, npt) and out["choice"].shape == (B, npt) and out["R_aug"].shape == (B, 2, 3, 3)
    assert np.array_equal(out["status"], ref["status"])
    assert np.array_equal(out["choice"], ref["choice"])
    assert np.array_equal(out["counts"], ref["counts"]) and np.array_equal(out["idx"], ref["idx"])
    _close(out["R_aug"], ref["R_aug"], "R_aug")
    _close(out["T"], ref["T"], "T")
    _close(out["T_aug"], ref["T_aug"], "T_aug")
    R = out["R_aug"].astype(np.float64)
    assert np.abs(np.einsum('bsji,bsjk->bsik', R, R) - np.eye(3)).max() <= 1e-6
    if kw.get("max_degree", 30) <= 1:                            # randint(0, 1) is 0 as well
        assert np.array_equal(out["R_aug"], np.broadcast_to(np.eye(3, dtype=np.float32), (B, 2, 3, 3)))
    mine = Pr.fragment_pair_batch(*inputs, n_sample, npt, RADIUS, seed=SEED, ids=ids, center=int(kw.get("center", False)),
                                  key_bits=kw.get("key_bits", 32), R_aug=out["R_aug"])      # from the device's own rotations
    assert not _bitwise(out, mine, ("src", "tgt"))
    _close(out["T_aug"], mine["T_aug"], "T_aug from the device's R_aug")
    # the library's own patch extraction, one fragment and one keypoint at a time, with kpt_row0 = Q'
    from epn_pointcloud_amd.vgtk.cuda import grouping
    for b in range(B):
        if out["status"][b]:
            continue
        for s in (0, 1):
            f = pairs[b][s]
            if off[f + 1] - off[f] < 1:
                continue                                         # radius_patches refuses an empty fragment
            pc = _dev(gpu, points[off[f]:off[f + 1]], np.float32)
            for j in range(npt):
                kpt = _dev(gpu, corr[coff[b] + out["choice"][b, j], s][None], np.float32)
                idx, counts, _ = grouping.radius_patches(pc, kpt, RADIUS, n_sample, seed=SEED, kpt_row0=Pr.stream(ids[b], s, j, npt),
                                                         key_bits=kw.get("key_bits", 32))
                assert np.array_equal(idx.cpu().numpy()[0], out["idx"][b, s, j]), (b, s, j)
                assert int(counts[0]) == out["counts"][b, s, j], (b, s, j)
    return out, ref


# (key_bits, max_degree, center) cycle through their values over the twelve shapes: every value occurs
_VARIANTS = [(32, 30, False), (2, 0, True), (32, 360, True), (2, 1, False)]
_SHAPES = [(B, npt, ns) for B in (1, 3) for npt in (1, 3) for ns in (1, 8, 64)]


@pytest.mark.parametrize("case", range(len(_SHAPES)), ids=lambda i: "B{}-npt{}-ns{}-kb{}-deg{}-c{:d}".format(*_SHAPES[i], *_VARIANTS[i % 4]))
def test_batch_matches_the_restatement_and_radius_patches(gpu, case):
    (B, npt, n_sample), (key_bits, max_degree, center) = _SHAPES[case], _VARIANTS[case % 4]
    points, off, poses = _scene()
    ids = np.arange(B, dtype=np.int64) * 1000003 + 2 ** 39
    out, _ = _check(gpu, (points, off, *_batch(B), poses), n_sample, npt, ids, key_bits=key_bits, max_degree=max_degree, center=center)
    assert (out["status"] == 0).all()


@pytest.mark.parametrize("n_sample", [1, 8, 64])
def test_every_count_case(gpu, n_sample):
    """One correspondence per sample (choice = 0), its source keypoint placed so that the patch in the 700-point fragment holds
    0, 1, 2, fewer than, exactly and more than n_sample points; the targets are the one-point and the empty fragment."""
    points, off, poses = _scene()
    frag = points[off[4]:off[5]]
    rng = np.random.default_rng(9)
    cand = _frame(rng.random((6000, 3)) * 1.8 - 0.4, poses[4])
    counts = np.array([Pr.P.in_radius(frag, k, RADIUS).sum() for k in cand])
    want = sorted({0, 1, 2, max(n_sample - 3, 2), n_sample, n_sample + 1, n_sample + 5})
    rows = [int(np.nonzero(counts == c)[0][0]) for c in want]   # IndexError: the candidates miss a case
    corr = np.stack([np.stack((cand[r], cand[r] * 0)) for r in rows])
    pairs = [(4, 0) if i % 2 else (4, 5) for i in range(len(rows))]
    coff = np.arange(len(rows) + 1, dtype=np.int32)
    ids = np.arange(len(rows), dtype=np.int64) + 5
    for key_bits in (32, 2):
        out, _ = _check(gpu, (points, off, np.asarray(pairs, np.int32), corr, coff, poses), n_sample, 1, ids, key_bits=key_bits)
        assert out["counts"][:, 0, 0].tolist() == want and (out["counts"][:, 1] <= 1).all() and not out["tgt"].any()
        assert (out["status"] == 0).all()                        # an empty patch is no status


def test_status_rows_and_their_neighbours(gpu):
    points, off, poses = _scene()
    _, corr3, _ = _batch(3)
    poses = np.concatenate((poses, poses[:1]))
    poses[6, 2, 3] = np.nan
    off = np.concatenate((off, [off[-1] - 10]))                  # fragment 6 descends
    corr = np.concatenate((corr3[:5], corr3[5:10], np.full((1, 2, 3), np.inf, np.float32), corr3[10:15]))
    pairs = np.array([(4, 3), (4, 6), (2, 4), (7, 1), (-1, 1), (4, 3), (1, 1)], dtype=np.int32)
    coff = np.array([0, 5, 10, 10, 10, 10, 11, 16], dtype=np.int32)    # good, bad offsets, none, bad pair x2, inf keypoint, good
    ids = np.arange(7, dtype=np.int64) + 40
    out, ref = _check(gpu, (points, off, pairs, corr, coff, poses), 8, 3, ids)
    assert out["status"].tolist() == [0, 8, 1, 8, 8, 4, 0]
    off_ok = off.copy()
    off_ok[-1] = off_ok[-2]                                      # fragment 6 empty but well delimited: its pose is not finite
    bad_corr = coff.copy()
    bad_corr[3] = 17                                             # corr_offsets beyond C, then descending
    more, _ = _check(gpu, (points, off_ok, pairs, corr, bad_corr, poses), 8, 3, ids)
    assert more["status"].tolist() == [0, 4, 8, 8, 8, 4, 0]
    for o in (out, more):
        for b in range(1, 6):
            assert (o["idx"][b] == -1).all() and (o["choice"][b] == -1).all() and not o["counts"][b].any()
            assert not o["src"][b].any() and not o["tgt"][b].any() and not o["T"][b].any() and not o["T_aug"][b].any()
        _close(o["R_aug"], ref["R_aug"], "R_aug is still drawn")
    # the healthy samples are what they are without the bad ones
    good = _np(_run(gpu, points, off[:7], pairs[[0, 6]], np.concatenate((corr[:5], corr[11:])), [0, 5, 10], poses[:6], 8, 3,
                    ids=ids[[0, 6]], seed=SEED))
    for k in FIELDS:
        assert np.array_equal(out[k][[0, 6]].view(np.int32), good[k].view(np.int32)), k
        assert np.array_equal(more[k][[0, 6]].view(np.int32), good[k].view(np.int32)), k


def test_two_calls_are_bitwise_equal_and_shuffled_ids_permute_the_outputs(gpu):
    points, off, poses = _scene()
    pairs, corr, coff = _batch(3)
    ids = np.array([77, 2 ** 40 - 1, 5], dtype=np.int64)
    kw = dict(seed=SEED, key_bits=2, center=True)
    first = _np(_run(gpu, points, off, pairs, corr, coff, poses, 64, 3, ids=ids, **kw))
    again = _np(_run(gpu, points, off, pairs, corr, coff, poses, 64, 3, ids=ids, **kw))
    assert not _bitwise(first, again)
    order = [2, 0, 1]
    shuffled = _np(_run(gpu, points, off, pairs[order], corr.reshape(3, 5, 2, 3)[order].reshape(-1, 2, 3), coff, poses, 64, 3,
                        ids=ids[order], **kw))
    alone = _np(_run(gpu, points, off, pairs[1:2], corr[5:10], coff[:2], poses, 64, 3, ids=ids[1:2], **kw))
    for k in FIELDS:
        assert np.array_equal(first[k][order].view(np.int32), shuffled[k].view(np.int32)), k
        assert np.array_equal(first[k][1].view(np.int32), alone[k][0].view(np.int32)), k
    other = _np(_run(gpu, points, off, pairs, corr, coff, poses, 64, 3, ids=ids + 1, **kw))
    assert not np.array_equal(other["R_aug"], first["R_aug"])    # another id: other draws
    default = _np(_run(gpu, points, off, pairs, corr, coff, poses, 64, 3, **kw))
    named = _np(_run(gpu, points, off, pairs, corr, coff, poses, 64, 3, ids=np.arange(3), **kw))
    assert not _bitwise(default, named)                          # ids default to the position in the batch
    p32 = poses.astype(np.float32)                               # fp32 poses are widened, nothing else
    assert not _bitwise(_np(_run(gpu, points, off, pairs, corr, coff, p32, 64, 3, ids=ids, **kw)),
                        _np(_run(gpu, points, off, pairs, corr, coff, p32.astype(np.float64), 64, 3, ids=ids, **kw)))


def test_graph_capture_replays_with_new_ids(gpu):
    from epn_pointcloud_amd import data
    points, off, poses = _scene()
    pairs, corr, coff = _batch(3)
    t = [_dev(gpu, points), _dev(gpu, off), _dev(gpu, pairs), _dev(gpu, corr), _dev(gpu, coff), _dev(gpu, poses)]
    ids = torch.arange(3, device=gpu, dtype=torch.int64)
    call = lambda i: data.fragment_pair_batch(*t, 8, 3, RADIUS, seed=SEED, ids=i)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                # warm-up off the capture, as torch asks
        call(ids)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call(ids)
    new_ids = torch.arange(3, device=gpu, dtype=torch.int64) * 13 + 1000
    ids.copy_(new_ids)                                           # in place: the graph reads the same buffer
    graph.replay()
    torch.cuda.synchronize()
    eager = call(new_ids)
    assert not _bitwise(_np(out), _np(eager))
    assert not torch.equal(eager.R_aug, call(torch.arange(3, device=gpu, dtype=torch.int64)).R_aug)


def test_batch_feeds_the_descriptor_network_and_its_loss(gpu):
    """batch -> the tiny inv model's forward on both sides -> losses.batch_hard_triplet: a finite loss."""
    from conftest import golden
    from test_models_cpu import fill_state_dict, product_model
    from epn_pointcloud_amd import losses
    n = golden("model_inv_tiny.npz")["pts"].shape[1]             # the patch size the tiny model's schedule was built for
    model = fill_state_dict(product_model("inv")).to(gpu).train()
    points, off, poses = _scene()
    world = np.random.default_rng(3).random((6, 3)) * 0.4 + 0.3  # keypoints well inside the cube: full patches
    corr = np.stack((_frame(world, poses[4]), _frame(world, poses[4])), axis=1)
    out = _run(gpu, points, off, [(4, 4)], corr, [0, 6], poses, n, 3, radius=0.45, seed=SEED, center=True)
    assert out.status.tolist() == [0] and int(out.counts.min()) > 1
    src, _ = model(out.src.reshape(-1, n, 3))
    tgt, _ = model(out.tgt.reshape(-1, n, 3))
    loss = losses.batch_hard_triplet(src, tgt).loss
    assert loss.dim() == 0 and bool(torch.isfinite(loss))
