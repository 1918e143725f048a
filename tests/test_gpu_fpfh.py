"""FPFH descriptors on the GPU (csrc/fpfh.hip behind vgtk.pc.PointGrid.fpfh / compute_fpfh_feature / describe_fpfh and the
planar-patch filter of keypoint_pairs) against the numpy restatement of their specification (tests/fpfh_ref.py: brute-force
neighbourhoods, float64 pair features, integer histograms and fixed-point sums).  The bin counts and the neighbourhood sizes are
compared exactly, the descriptors and the flags bit for bit, and no pair is left out: every input comes from fpfh_ref.py, and
tests/test_fpfh_spec.py holds each of them to zero edge pairs (no value within 2^-30 of a bin border, where the device's atan2
could land in the other bin).  Nothing here has been compared with open3d."""
import numpy as np
import pytest
import torch

import fpfh_ref as F
import grid_nn_ref as G

pytestmark = pytest.mark.gpu

CASES = F.gpu_cases()
_WANT = {}


def want_of(name):
    """The restatement of a case, computed once and shared"""
    if name not in _WANT:
        c = CASES[name]
        _WANT[name] = F.point_fpfh(c["points"], c["normals"], c["radius"], c["valid"])
    return _WANT[name]


def D(gpu, a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(gpu)


def grid_of(gpu, c):
    from epn_pointcloud_amd.vgtk import pc as pctk
    valid = None if c["valid"] is None else D(gpu, c["valid"], np.uint8)
    return pctk.PointGrid(D(gpu, c["points"]), c["max_radius"], valid=valid)


def compare(got, want):
    fpfh, count, flags, spfh = (t.cpu().numpy() for t in got)
    assert fpfh.dtype == np.float32 and count.dtype == np.int32 and flags.dtype == np.int32 and spfh.dtype == np.int32
    assert fpfh.shape == want["fpfh"].shape and spfh.shape == want["spfh"].shape
    assert np.array_equal(count, want["count"])
    assert np.array_equal(flags, want["flags"])
    assert np.array_equal(spfh, want["spfh"])
    assert np.array_equal(fpfh.view(np.uint32), want["fpfh"].view(np.uint32))
    return fpfh


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_restatement(gpu, name):
    c, want = CASES[name], want_of(name)
    assert want["edge_pairs"] == 0                                  # the condition, held on the CPU by test_fpfh_spec.py
    grid = grid_of(gpu, c)
    got = grid.fpfh(D(gpu, c["normals"]), c["radius"], return_spfh=True)
    fpfh = compare(got, want)
    again = grid.fpfh(D(gpu, c["normals"]), c["radius"], return_spfh=True)
    assert all(torch.equal(a, b) for a, b in zip(got, again))       # two runs, bit for bit
    plain = grid.fpfh(D(gpu, c["normals"]), c["radius"])
    assert plain.spfh is None and torch.equal(plain.features, got.features)
    if fpfh.shape[0]:
        live = want["flags"] == 0
        assert (fpfh[~live] == 0).all() and (fpfh[live].reshape(-1, 3, 11).sum(axis=2) > 99.99).all()


def test_the_isolation_argument_on_the_device(gpu):
    """the row is zero exactly where nearest(exclude_self=True) finds nobody."""
    c = CASES["edges"]
    grid = grid_of(gpu, c)
    feats = grid.fpfh(D(gpu, c["normals"])).features
    idx = grid.nearest(grid.points, c["radius"], exclude_self=True)[0]
    assert torch.equal((feats == 0).all(dim=1), idx < 0) and int((idx < 0).sum()) == 1


def test_null_pointers_are_refused_with_a_real_grid(gpu):
    import ctypes
    from epn_pointcloud_amd import _lib
    lib = _lib.get_lib()
    c = CASES["n=3"]
    grid = grid_of(gpu, c)
    t = torch.zeros(3 * 34 + 8, dtype=torch.int64, device=gpu)
    p = t.data_ptr()
    args = dict(points=grid.points.data_ptr(), normals=p, fpfh=p, count=p, flags=p, workspace=p)
    for missing in list(args) + ["bytes"]:
        a = dict(args, **({missing: 0} if missing != "bytes" else {}))
        rc = lib.epn_point_fpfh_f32(ctypes.c_void_p(grid._workspace.data_ptr()), 3, *(ctypes.c_void_p(a[k]) for k in
                                    ("points", "normals")), c["radius"], *(ctypes.c_void_p(a[k]) for k in ("fpfh", "count", "flags")),
                                    None, ctypes.c_void_p(a["workspace"]), 0 if missing == "bytes" else t.numel() * 8,
                                    _lib.stream_of(t))
        assert rc == -1, missing
    with pytest.raises(ValueError, match="max_radius"):
        grid.fpfh(D(gpu, c["normals"]), 2 * c["max_radius"])


def test_graph_capture_and_replay(gpu):
    from epn_pointcloud_amd.vgtk.cuda import grouping
    c, want = CASES["dense"], want_of("dense")
    grid = grid_of(gpu, c)
    normals = D(gpu, c["normals"])
    eager = grid.fpfh(normals, c["radius"], return_spfh=True)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        grouping.point_fpfh(grid._workspace, grid.n, grid.points, normals, c["radius"], return_spfh=True)      # warm the allocator
        stream.synchronize()
        with torch.cuda.graph(graph, stream=stream):
            out = grouping.point_fpfh(grid._workspace, grid.n, grid.points, normals, c["radius"], return_spfh=True)
    for t in out:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, out))
    compare(out, want)


def test_compute_fpfh_feature_from_points_and_from_a_grid(gpu, vgtk_alias):
    import vgtk.pc as pctk
    c, want = CASES["smaller_radius"], want_of("smaller_radius")
    pts, normals = D(gpu, c["points"]), D(gpu, c["normals"])
    a = pctk.compute_fpfh_feature(pts, normals, c["radius"])        # builds its own grid at max_radius = radius
    b = pctk.compute_fpfh_feature(grid_of(gpu, c), normals, c["radius"])
    assert isinstance(a, pctk.PointFPFH) and a.spfh is None and a.features.device == pts.device
    assert torch.equal(a.features, b.features) and torch.equal(a.count, b.count) and torch.equal(a.flags, b.flags)
    assert np.array_equal(a.features.cpu().numpy().view(np.uint32), want["fpfh"].view(np.uint32))
    with pytest.raises(ValueError, match="built for radii"):
        pctk.compute_fpfh_feature(grid_of(gpu, c), normals, 2 * c["max_radius"])


# ------------------------------------------------------------------------------------------------ the planar-patch filter
@pytest.fixture(scope="module")
def fragments(gpu):
    """The two synthetic fragments, the device's centroid normals and the restatement's pairs at a parameter taken from the
    restatement: the median of the candidates' larger standard deviation, so about half of them survive."""
    from epn_pointcloud_amd.vgtk import pc as pctk
    src, tgt = F.fragment_pair()
    cen = [pctk.voxel_down_sample(D(gpu, p), 0.05)[0] for p in (src, tgt)]
    normals = [pctk.estimate_normals(c, 0.15, max_nn=30).normals.cpu().numpy() for c in cen]
    cand = F.keypoint_candidates(src, tgt, normals)
    param = float(np.median(cand["std"].max(axis=1)))
    assert np.abs(cand["std"] - param).min() > 1e-6                 # no candidate sits on the threshold
    return src, tgt, cand, param


def test_keypoint_pairs_without_the_filter_is_the_present_path(gpu, fragments):
    from epn_pointcloud_amd.vgtk import pc as pctk
    src, tgt = D(gpu, fragments[0]), D(gpu, fragments[1])
    a, b = pctk.keypoint_pairs(src, tgt), pctk.keypoint_pairs(src, tgt, nonplanar_param=-1.0)
    assert a.rows.shape[0] > 128 and all(torch.equal(x, y) for x, y in zip(a, b))
    rows, sel, d2 = G.keypoint_pairs(fragments[0], fragments[1])
    assert np.array_equal(a.rows.cpu().numpy(), rows) and np.array_equal(a.src_centroid_row.cpu().numpy(), sel)


def test_keypoint_pairs_with_the_filter(gpu, fragments):
    from epn_pointcloud_amd.vgtk import pc as pctk
    src, tgt, cand, param = fragments
    rows, sel, d2 = F.keypoint_pairs(cand, param, min_keypoints=1)
    assert 0 < rows.shape[0] < cand["sel"].size                     # the filter removes some and keeps some
    assert F.keypoint_pairs(cand, param, min_keypoints=rows.shape[0] + 1)[0].shape == (0, 2)
    got = pctk.keypoint_pairs(D(gpu, src), D(gpu, tgt), nonplanar_param=param, min_keypoints=1)
    assert np.array_equal(got.rows.cpu().numpy(), rows)
    assert np.array_equal(got.src_centroid_row.cpu().numpy(), sel)
    assert np.array_equal(got.d2.cpu().numpy().view(np.uint32), d2.view(np.uint32))
    few = pctk.keypoint_pairs(D(gpu, src), D(gpu, tgt), nonplanar_param=param, min_keypoints=rows.shape[0] + 1)
    assert few.rows.shape == (0, 2) and few.src_centroid_row.numel() == 0 and few.d2.numel() == 0
    exact = pctk.keypoint_pairs(D(gpu, src), D(gpu, tgt), nonplanar_param=param, min_keypoints=rows.shape[0])
    assert torch.equal(exact.rows, got.rows)
    scene, _ = pctk.scene_keypoint_pairs([D(gpu, src), D(gpu, tgt)], nonplanar_param=param, min_keypoints=1)
    assert torch.equal(scene[(0, 1)], got.rows)


# ------------------------------------------------------------------------------------------------ the baseline descriptor
def test_describe_fpfh_matches_a_rigid_copy_to_itself(gpu):
    """200 points of a wavy height field and the same points after a rigid motion, the view point moved along: the descriptor
    is invariant up to rounding, so the mutual nearest neighbour of every valid keypoint is itself."""
    from epn_pointcloud_amd import matching
    from epn_pointcloud_amd.vgtk import pc as pctk
    rng = np.random.default_rng(17)
    u = rng.uniform(0, 1.5, (200, 2))
    frag = np.stack((u[:, 0], u[:, 1], 0.2 * np.sin(4 * u[:, 0]) * np.cos(3 * u[:, 1]) + 0.1 * u[:, 0] * u[:, 1]), axis=1).astype(np.float32)
    view = np.array([0.75, 0.75, 5.0])
    copy, R, t = F.rigid_copy(frag)
    rows = torch.arange(200, device=gpu)
    a, va = pctk.describe_fpfh(D(gpu, frag), rows, normal_radius=0.3, feature_radius=0.4, view=view.astype(np.float32).tolist())
    b, vb = pctk.describe_fpfh(D(gpu, copy), D(gpu, copy), normal_radius=0.3, feature_radius=0.4,
                               view=(R @ view + t).astype(np.float32).tolist())
    assert a.shape == (200, 33) and a.dtype == torch.float32 and va.dtype == torch.bool and va.shape == (200,)
    assert int(va.sum()) > 190 and torch.equal(va, vb)
    s2t, t2s, mutual = matching.match_descriptors(a, b, va, vb)
    own = torch.arange(200, device=gpu, dtype=s2t.dtype)
    assert torch.equal(s2t[va], own[va]) and torch.equal(t2s[vb], own[vb]) and bool(mutual[vb].all())
    # integer rows and their coordinates are the same keypoints; a keypoint far from the cloud is not valid
    c, vc = pctk.describe_fpfh(D(gpu, frag), D(gpu, frag), normal_radius=0.3, feature_radius=0.4, view=view.astype(np.float32).tolist())
    assert torch.equal(a, c) and torch.equal(va, vc)
    far, vfar = pctk.describe_fpfh(D(gpu, frag), D(gpu, frag[:2] + 50), normal_radius=0.3, feature_radius=0.4)
    assert not bool(vfar.any()) and bool((far == 0).all())
    down, vd = pctk.describe_fpfh(D(gpu, frag), rows, voxel_size=0.2, normal_radius=0.4, feature_radius=0.5)
    assert down.shape == (200, 33) and bool(vd.all()) and bool((down.reshape(200, 3, 11).sum(dim=2) > 99.99).all())
