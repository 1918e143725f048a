"""ModelNet batches on the device (csrc/modelnet_batch.hip through epn_pointcloud_amd.data) against the numpy restatement
(tests/modelnet_batch_ref.py) and, for given rotations, against what the reference's own functions gave
(tests/golden/modelnet_batch.npz).

Exact: idx (with key_bits = 4 that is the tie rule across chunk and wave boundaries), R_label against the arg max recomputed
from the device's own R, every output between two calls, a cloud's rows wherever it stands in a batch, a graph replay against
the eager call.  Within 2^-23 (modelnet_batch_ref.TOL): R, pc, pc_plain and R_res -- values of magnitude <= 1, one fp32 rounding
of an fp64 result moves a value by at most 2^-25, an fp64 difference in sin / cos / sqrt or a sum's order can flip that rounding
by one ulp, 2^-24, and the bound is twice that."""
import functools

import numpy as np
import pytest
import torch

from conftest import golden
import modelnet_batch_ref as Mr
import rotation_ref as Rf

pytestmark = pytest.mark.gpu

SEED = 2913
FIELDS = ("pc", "idx", "R", "R_label", "R_res", "status", "pc_plain")


def _sizes(n_sample):
    """The ragged batch of one n_sample, in a fixed order without repeats (n_sample - 1 = 0 is an empty cloud)."""
    out = []
    for n in (1, 2, 255, 256, 257, n_sample - 1, n_sample, n_sample + 1, 5000):
        if n not in out:
            out.append(n)
    return out


@functools.lru_cache(maxsize=None)
def _clouds(n_sample):
    """Raw clouds: off-centre, not unit scale, like a dataset's -> (points f32 [M,3], offsets i32 [B+1])."""
    rng = np.random.default_rng(100 + n_sample)
    sizes = _sizes(n_sample)
    pts = np.concatenate([(rng.standard_normal((n, 3)) * (1 + 0.3 * i) + 5.0 * rng.standard_normal(3)).astype(np.float32)
                          for i, n in enumerate(sizes)])
    off = np.concatenate(([0], np.cumsum(sizes))).astype(np.int32)
    return pts, off


@functools.lru_cache(maxsize=None)
def _anchors():
    return Rf.anchors_for(60)


@functools.lru_cache(maxsize=None)
def _reference(n_sample, key_bits):
    pts, off = _clouds(n_sample)
    ids = np.arange(off.size - 1) * 7 + 3
    return ids, Mr.modelnet_batch(pts, off, n_sample, seed=SEED, ids=ids, anchors=_anchors(), key_bits=key_bits)


def _run(gpu, pts, off, n_sample, **kw):
    from epn_pointcloud_amd import data
    kw = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(gpu) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    return data.modelnet_batch(torch.from_numpy(np.ascontiguousarray(pts)).to(gpu), torch.from_numpy(np.asarray(off, np.int32)).to(gpu),
                               n_sample, **kw)


def _np(out):
    return {k: (None if getattr(out, k) is None else getattr(out, k).cpu().numpy()) for k in FIELDS}


def _bitwise(a, b):
    return all(np.array_equal(a[k].view(np.int32), b[k].view(np.int32)) for k in FIELDS if a[k] is not None or b[k] is not None)


def _close(got, want, name):
    err = float(np.abs(got.astype(np.float64) - np.asarray(want, dtype=np.float64)).max()) if got.size else 0.0
    print(f"{name}: max |device - expected| = {err:.3e} (bound {Mr.TOL:.3e})")
    assert err <= Mr.TOL, name


@pytest.mark.parametrize("key_bits", [32, 4])
@pytest.mark.parametrize("n_sample", [1, 64, 1024])
def test_ragged_batch_matches_the_restatement(gpu, n_sample, key_bits):
    pts, off = _clouds(n_sample)
    ids, ref = _reference(n_sample, key_bits)
    kw = dict(seed=SEED, ids=ids.astype(np.int64), anchors=_anchors(), key_bits=key_bits, return_plain=True)
    out = _np(_run(gpu, pts, off, n_sample, **kw))
    again = _np(_run(gpu, pts, off, n_sample, **kw))
    assert out["pc"].shape == (off.size - 1, n_sample, 3) and out["idx"].dtype == np.int32 and out["R_label"].dtype == np.int32
    assert np.array_equal(out["status"], ref["status"])
    # a one-point cloud has no extent; n_sample = 1 selects one point of every cloud
    want_status = [1 if n == 0 else 2 if (n == 1 or n_sample == 1) else 0 for n in _sizes(n_sample)]
    assert out["status"].tolist() == want_status
    assert np.array_equal(out["idx"], ref["idx"])
    _close(out["R"], ref["R"], "R")
    _close(out["pc"], ref["pc"], "pc")
    _close(out["pc_plain"], ref["pc_plain"], "pc_plain")
    an = _anchors()
    for c in range(off.size - 1):
        label, res, gap = Mr.anchor_label(an, out["R"][c])       # from the device's own R
        assert out["R_label"][c] == label, (c, gap)
        _close(out["R_res"][c], res if out["status"][c] == 0 else np.zeros((3, 3)), f"R_res[{c}]")
    assert _bitwise(out, again)


def test_a_cloud_gives_the_same_rows_wherever_it_stands(gpu):
    """The cloud with id 77: alone, at position 0 of a batch of 5, and at position 4."""
    rng = np.random.default_rng(7)
    mine = (rng.standard_normal((700, 3)) * 2 + 1).astype(np.float32)
    others = [(rng.standard_normal((n, 3)) + i).astype(np.float32) for i, n in enumerate((300, 64, 1500, 90))]
    kw = dict(seed=SEED, anchors=_anchors(), return_plain=True)

    def run(clouds, ids):
        off = np.concatenate(([0], np.cumsum([len(c) for c in clouds])))
        return _np(_run(gpu, np.concatenate(clouds), off, 256, ids=np.asarray(ids, dtype=np.int64), **kw))

    alone = run([mine], [77])
    first = run([mine] + others, [77, 1, 2, 3, 4])
    last = run(others + [mine], [4, 3, 2, 1, 77])
    assert alone["status"].tolist() == [0]
    for k in FIELDS:
        assert np.array_equal(alone[k][0].view(np.int32), first[k][0].view(np.int32)), k
        assert np.array_equal(alone[k][0].view(np.int32), last[k][4].view(np.int32)), k
    assert not np.array_equal(first["idx"][1], last["idx"][0])   # another id: other draws for the same cloud


def test_status_rows_and_their_neighbours(gpu):
    rng = np.random.default_rng(5)
    pts = rng.standard_normal((400, 3)).astype(np.float32)
    pts[100:200] = pts[100]                                      # one repeated point
    pts[230, 1] = np.nan
    off = np.array([0, 100, 100, 200, 300, 250, 400])            # good, empty, repeated, NaN, descending, good
    kw = dict(seed=3, anchors=_anchors(), return_plain=True)
    out = _np(_run(gpu, pts, off, 128, **kw))
    ref = Mr.modelnet_batch(pts, off, 128, seed=3, anchors=_anchors())
    assert out["status"].tolist() == [0, 1, 2, 4, 8, 0] == ref["status"].tolist()
    for c in (1, 2, 3, 4):
        assert (out["idx"][c] == -1).all()
        assert not out["pc"][c].any() and not out["pc_plain"][c].any() and not out["R_res"][c].any()
        _close(out["R"][c], ref["R"][c], f"R[{c}]")              # still drawn
        assert out["R_label"][c] == Mr.anchor_label(_anchors(), out["R"][c])[0]
    assert np.array_equal(out["idx"], ref["idx"])
    _close(out["pc"], ref["pc"], "pc")
    good = _np(_run(gpu, np.concatenate((pts[:100], pts[250:400])), [0, 100, 250], 128, ids=np.array([0, 5]), **kw))
    for k in FIELDS:                                             # the neighbours of the bad rows are what they are without them
        assert np.array_equal(out[k][[0, 5]].view(np.int32), good[k].view(np.int32)), k


def test_rotation_modes(gpu):
    pts, off = _clouds(64)
    out = _run(gpu, pts, off, 64, seed=SEED, rotation="none", anchors=_anchors(), return_plain=True)
    assert torch.equal(out.R, torch.eye(3, device=gpu).expand(off.size - 1, 3, 3))
    assert torch.equal(out.pc, out.pc_plain) and out.pc.abs().max() > 0.5
    g = golden("modelnet_batch.npz")
    given = _np(_run(gpu, g["points"], g["offsets"], Mr.GOLDEN_NSAMPLE, seed=Mr.GOLDEN_SEED, rotation=g["R"], anchors=_anchors(),
                     return_plain=True))
    assert (given["status"] == 0).all() and np.array_equal(given["idx"], g["idx"]) and np.array_equal(given["R"], g["R"])
    assert np.array_equal(given["R_label"], g["label"])
    _close(given["pc"], g["pc"], "pc vs reference")
    _close(given["pc_plain"], g["plain"], "pc_plain vs reference")
    _close(given["R_res"], g["res"], "R_res vs reference")


def test_alignment_batch(gpu):
    from epn_pointcloud_amd import data
    import epn_pointcloud_amd.vgtk.functional as F
    pts, off = _clouds(64)
    keep = [i for i, n in enumerate(_sizes(64)) if n > 1]        # the clouds with an extent
    clouds = [pts[off[i]:off[i + 1]] for i in keep]
    points, offsets = data.pack_clouds(clouds, gpu)
    assert points.is_cuda and offsets.dtype == torch.int32 and offsets.tolist() == np.concatenate(([0], np.cumsum([len(c) for c in clouds]))).tolist()
    anchors = torch.from_numpy(_anchors()).to(gpu)
    ids = torch.arange(len(keep), device=gpu, dtype=torch.int64) + 11
    d = data.modelnet_alignment_batch(points, offsets, 64, anchors, seed=SEED, ids=ids)
    plain = data.modelnet_batch(points, offsets, 64, seed=SEED, ids=ids, return_plain=True)
    assert tuple(d["pc"].shape) == (len(keep), 2, 64, 3) and (d["status"] == 0).all()
    assert torch.equal(d["pc"][:, 0], plain.pc) and torch.equal(d["pc"][:, 1], plain.pc_plain) and torch.equal(d["T"], plain.R)
    R, R_label = F.label_relative_rotation(anchors, d["T"])
    assert torch.equal(d["R"], R) and torch.equal(d["R_label"], R_label) and tuple(R_label.shape) == (len(keep), 60)
    want_R, want_label, gap = Rf.label_relative_rotation(_anchors(), d["T"].cpu().numpy())   # independent of the library
    assert gap.min() > Rf.LABEL_GAP and np.array_equal(d["R_label"].cpu().numpy(), want_label)
    _close(d["R"].cpu().numpy(), want_R, "alignment R")
    assert plain.R_label is None and plain.R_res is None


def test_graph_capture_replays_with_new_ids(gpu):
    from epn_pointcloud_amd import data
    pts, off = _clouds(64)
    points, offsets = torch.from_numpy(pts.copy()).to(gpu), torch.from_numpy(off).to(gpu)
    anchors = torch.from_numpy(_anchors()).to(gpu)
    B = off.size - 1
    ids = torch.arange(B, device=gpu, dtype=torch.int64)
    call = lambda i: data.modelnet_batch(points, offsets, 64, seed=SEED, ids=i, anchors=anchors, return_plain=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                # warm-up off the capture, as torch asks
        call(ids)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call(ids)
    new_ids = torch.arange(B, device=gpu, dtype=torch.int64) * 13 + 1000
    ids.copy_(new_ids)                                           # in place: the graph reads the same buffer
    graph.replay()
    torch.cuda.synchronize()
    eager = call(new_ids)
    assert _bitwise(_np(out), _np(eager))
    assert not torch.equal(eager.R, call(torch.arange(B, device=gpu, dtype=torch.int64)).R)
