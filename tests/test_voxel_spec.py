"""Voxel-grid downsampling without a GPU: the entry points exist at every layer, the argument checks run before any HIP runtime
call, and the specification (tests/voxel_ref.py, the numpy restatement of include/epn_so3conv.h: epn_voxel_downsample_f32)
agrees with an independent formulation (np.unique on the keys, fp64 means), does not depend on the order of the points and
puts boundary points where open3d's floor() puts them.  Nothing here has been compared with open3d itself."""
import ctypes
import inspect

import numpy as np
import pytest

import voxel_ref as V

EINVAL = -1


def test_symbols_resolve_and_are_bound_at_every_layer(vgtk_alias):
    from epn_pointcloud_amd import _lib, models
    from epn_pointcloud_amd.vgtk.cuda import grouping
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("epn_voxel_downsample_workspace_bytes", "epn_voxel_downsample_f32"):
        assert name in _lib.EXPORTS
        assert hasattr(cdll, name)
    assert callable(grouping.voxel_downsample)
    import vgtk.pc
    assert callable(vgtk.pc.voxel_down_sample) and vgtk.pc.voxel_down_sample is vgtk_alias.pc.voxel_down_sample
    assert callable(vgtk.pc.reference_voxel_size)
    par = inspect.signature(models.InvSO3ConvModel.describe).parameters["voxel_size"]
    assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is None


N_OK = 1000


def _ws_bytes(n):
    from epn_pointcloud_amd import _lib
    return int(_lib.get_lib().epn_voxel_downsample_workspace_bytes(n))


def _call(**over):
    """Pointers: non-NULL, 8-byte aligned and never dereferenced (every call is refused, or n = 0)."""
    from epn_pointcloud_amd import _lib
    a = dict(pc=16, n=N_OK, voxel_size=0.03, centroids=16, counts=16, first_idx=16, point_voxel=16, status=16, workspace=16,
             workspace_bytes=_ws_bytes(N_OK))
    a.update(over)
    vp = lambda v: ctypes.c_void_p(v) if v else None
    return _lib.get_lib().epn_voxel_downsample_f32(vp(a["pc"]), a["n"], a["voxel_size"], vp(a["centroids"]), vp(a["counts"]),
                                                   vp(a["first_idx"]), vp(a["point_voxel"]), vp(a["status"]), vp(a["workspace"]),
                                                   a["workspace_bytes"], None)


@pytest.mark.parametrize("bad", [dict(n=-1), dict(n=2 ** 22 + 1, workspace_bytes=2 ** 40), dict(voxel_size=0.0),
                                 dict(voxel_size=-0.03), dict(voxel_size=float("nan")), dict(voxel_size=float("inf")),
                                 dict(pc=0), dict(centroids=0), dict(counts=0), dict(first_idx=0), dict(point_voxel=0),
                                 dict(status=0), dict(workspace=0), dict(workspace=20), dict(workspace_bytes=0),
                                 dict(workspace_bytes=None)], ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_bad_arguments_are_refused_before_any_runtime_call(bad):
    if "workspace_bytes" in bad and bad["workspace_bytes"] is None:
        bad = dict(workspace_bytes=_ws_bytes(N_OK) - 1)            # one byte short
    assert _call(**bad) == EINVAL


def test_no_points_is_success_and_launches_nothing():
    assert _call(n=0) == 0
    assert _call(n=0, pc=0, centroids=0, counts=0, first_idx=0, point_voxel=0, status=0, workspace=0, workspace_bytes=0) == 0
    assert _call(n=0, voxel_size=0.0) == EINVAL                    # the other checks still hold


def test_workspace_holds_the_table_at_every_size():
    assert _ws_bytes(0) == 0 and _ws_bytes(-3) == 0 and _ws_bytes(2 ** 22 + 1) == 0
    prev = 0
    for n in (1, 63, 64, 65, 1000, 65536, 65537, 2 ** 22):
        b = _ws_bytes(n)
        assert b >= 8 * V.capacity(n) + 4 * n and b >= prev         # a 64-bit key per slot, a slot per point
        prev = b
    assert [V.capacity(n) for n in (1, 64, 65, 2 ** 22)] == [128, 128, 256, 2 ** 23]


def _cloud(voxel_size, n=200_000, snapped=5000, seed=0):
    rng = np.random.default_rng(seed)
    pc = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    rows = rng.choice(n, snapped, replace=False)
    pc[rows] = (np.rint(pc[rows] / voxel_size) * voxel_size).astype(np.float32)      # on (or an ulp from) voxel faces and centres
    return pc


@pytest.mark.parametrize("voxel_size", [0.015, 0.03, 2.0 ** -5])
def test_restatement_against_unique_keys_and_fp64_means(voxel_size):
    """|centroid - mean| <= 2^-33 + 2^-24 |mean| + 2^-50 per coordinate: the fixed-point quantisation (half a unit of 2^-32 per
    point, so at most that in the mean), the final fp32 rounding (half an ulp <= 2^-24 |mean|), the fp64 mean's own rounding
    (|x| <= 3: sums of a handful of terms, far below 2^-50)."""
    pc = _cloud(voxel_size)
    cen, cnt, first, pv, keys, flags = V.voxel_downsample(pc, voxel_size)
    assert flags == 0
    _, idx, _ = V.voxel_indices(pc, voxel_size)
    k = V.make_key(idx[:, 0], idx[:, 1], idx[:, 2])
    uniq, inverse, ucnt = np.unique(k, return_inverse=True, return_counts=True)
    order = np.argsort(keys)
    assert np.array_equal(keys[order], uniq)                        # the same set of voxels
    assert np.array_equal(cnt[order], ucnt)
    assert cnt.sum() == pc.shape[0] and (pv >= 0).all()
    assert np.array_equal(keys[pv], k)                              # every point's row is its voxel's
    assert np.array_equal(np.minimum.reduceat(np.argsort(pv, kind="stable"), np.cumsum(cnt) - cnt), first)
    assert (np.diff(first) > 0).all()                               # rows in ascending order of the lowest member index
    p64 = pc.astype(np.float64)
    mean = np.stack([np.bincount(inverse, weights=p64[:, c]) for c in range(3)], axis=1) / ucnt[:, None]
    err = np.abs(cen[order].astype(np.float64) - mean)
    bound = 2.0 ** -33 + 2.0 ** -24 * np.abs(mean) + 2.0 ** -50
    print(f"voxel_size {voxel_size}: {uniq.size} voxels, worst |centroid - mean| / bound = {(err / bound).max():.4f}")
    assert (err <= bound).all()


def test_shuffling_the_points_changes_only_the_row_order():
    pc = _cloud(0.03, n=20_000, snapped=500, seed=1)
    perm = np.random.default_rng(2).permutation(pc.shape[0])
    assert V.voxel_map(pc, 0.03) == V.voxel_map(pc[perm], 0.03)     # key -> (integer sums, count), bit for bit
    a, b = V.voxel_downsample(pc, 0.03), V.voxel_downsample(pc[perm], 0.03)
    oa, ob = np.argsort(a[4]), np.argsort(b[4])
    assert np.array_equal(a[4][oa], b[4][ob]) and np.array_equal(a[1][oa], b[1][ob])
    assert np.array_equal(a[0][oa].view(np.uint32), b[0][ob].view(np.uint32))
    assert not np.array_equal(a[4], b[4])                           # the row order did change
    assert np.array_equal(a[4][a[3]], b[4][b[3]][np.argsort(perm)])  # every point still lands in the same voxel


def test_points_on_a_voxel_face_belong_to_the_upper_voxel():
    """voxel_size 2^-5, grid-valued coordinates: everything is exact.  lo = (-1, -1, -1); the faces of the grid are at
    lo + (k - 1/2) voxel_size, so the minimum point sits half a voxel inside voxel 0."""
    vs = 2.0 ** -5
    lo = -1.0
    face = lambda k: lo + (k - 0.5) * vs
    pc = np.array([[lo, lo, lo],                                    # voxel (0, 0, 0), half a voxel inside it
                   [face(1), lo, lo],                               # on the face between 0 and 1 along x: voxel 1
                   [np.nextafter(np.float32(face(1)), np.float32(-9)), lo, lo],  # an ulp below it: voxel 0
                   [lo, face(7), face(3)],
                   [lo, lo, face(2 ** 10)]], dtype=np.float32)
    _, idx, flags = V.voxel_indices(pc, vs)
    assert flags == 0
    assert idx.tolist() == [[0, 0, 0], [1, 0, 0], [0, 0, 0], [0, 7, 3], [0, 0, 1024]]
    frac = (pc[0].astype(np.float64) - (lo - 0.5 * vs)) / vs
    assert frac.tolist() == [0.5, 0.5, 0.5]
    cen, cnt, first, pv, keys, _ = V.voxel_downsample(pc, vs)
    assert pv.tolist() == [0, 1, 0, 2, 3] and cnt.tolist() == [2, 1, 1, 1] and first.tolist() == [0, 1, 3, 4]
    assert cen[0].tolist() == [float(np.float32((np.float64(pc[0, 0]) + np.float64(pc[2, 0])) / 2)), lo, lo]


def test_non_finite_points_are_dropped_and_range_errors_are_flagged():
    pc = np.array([[0.5, 0.5, 0.5], [np.nan, 0, 0], [0.25, -np.inf, 0], [0.5, 0.5, 0.5], [-7, np.inf, np.nan]], dtype=np.float32)
    cen, cnt, first, pv, _, flags = V.voxel_downsample(pc, 0.03)
    assert flags == 0 and pv.tolist() == [0, -1, -1, 0, -1] and cnt.tolist() == [2] and first.tolist() == [0]
    assert cen.tolist() == [[0.5, 0.5, 0.5]]                        # the dropped rows' finite coordinates moved no bound
    assert V.voxel_downsample(np.array([[0, 0, 300.0]], np.float32), 0.03)[5] == V.FLAG_COORD
    assert V.voxel_downsample(np.array([[0, 0, 0], [200.0, 0, 0]], np.float32), 1e-5)[5] == V.FLAG_INDEX
    assert V.voxel_downsample(np.full((3, 3), np.nan, np.float32), 0.03)[3].tolist() == [-1, -1, -1]


@pytest.mark.parametrize("home", [5, 127])
def test_collision_clouds_share_one_home_slot(home):
    pc, idx = V.colliding_cloud(64, home)
    assert V.capacity(64) == 128 and len({tuple(r) for r in idx.tolist()}) == 64
    assert {V.home_slot(int(V.make_key(*r)), 128) for r in idx.tolist()} == {home}
    assert np.array_equal(V.voxel_indices(pc, 2.0 ** -5)[1], idx)   # the indices the specification derives from the points


def test_reference_voxel_size(vgtk_alias):
    import vgtk.pc
    assert [vgtk.pc.reference_voxel_size(n) for n in (512, 1024, 2048)] == [0.03, 0.015, 0.015]
