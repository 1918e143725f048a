"""TSDF fusion without a GPU: the entry points exist at every layer, every refusal is decided before any HIP runtime call, and
the specification (tests/tsdf_ref.py, the numpy restatement of include/epn_so3conv.h: epn_tsdf_fuse_f32, epn_tsdf_extract_f32)
gives hand-derived answers on a fronto-parallel plane, fuse_sequence cuts the windows the reference's loop cuts, and the frustum
box holds every unit the restatement allocates.  Nothing here has been compared with open3d itself."""
import ctypes

import numpy as np
import pytest

import tsdf_ref as T

EINVAL, EWORKSPACE, ENULL = -1, -2, -3
VL = 2.0 ** -7
UL = 16 * VL
K = (60.0, 45.0, 19.5, 14.5)


def test_symbols_resolve_and_are_bound_at_every_layer(vgtk_alias):
    from epn_pointcloud_amd import _lib, fusion
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("epn_tsdf_fuse_workspace_bytes", "epn_tsdf_fuse_f32", "epn_tsdf_extract_f32"):
        assert name in _lib.EXPORTS and hasattr(cdll, name)
    assert "epn_tsdf_fuse_workspace_bytes" in _lib._HOST_ONLY and "epn_tsdf_fuse_f32" not in _lib._HOST_ONLY
    import vgtk.pc
    assert vgtk.pc.fuse_fragment is fusion.fuse_fragment and vgtk.pc.fuse_sequence is fusion.fuse_sequence


# ---- the plane z = 0.25 = 32 VL, one frame, identity pose -------------------------------------------------------------------

def _plane():
    depth = np.full((1, 30, 40), 250, dtype=np.uint16)
    eye = np.eye(4)[None]
    lo, dims = [-2, -2, 0], [4, 4, 4]
    vol = T.fuse(depth, eye, eye, K, lo, dims, 1 << 17, voxel_length=VL, sdf_trunc=0.04, stride=4)
    return depth, lo, dims, vol


def test_plane_allocates_the_units_around_it_with_mask_one():
    """Samples: u = 0..36, v = 0..28 in steps of 4, x = (u - 19.5) / 240 in [-0.08125, 0.06875], y = (v - 14.5) / 180 in [-0.0806,
    0.075], z = 0.25; +- 0.04 reaches x, y in (-0.125, 0.125): units -1 and 0, and z in [0.21, 0.29]: units 1 and 2."""
    _, lo, dims, vol = _plane()
    want = [[x, y, z] for x in (-1, 0) for y in (-1, 0) for z in (1, 2)]
    assert vol["n_blocks"] == 8 and vol["flags"] == 0 and vol["n_outside"] == 0
    assert vol["block_unit"].tolist() == want                          # ascending directory order: x slowest, z fastest
    assert (vol["block_mask"] == 1).all()


def test_tsdf_of_the_column_through_the_principal_ray():
    """Voxel (x, y) = (0.5, 0.5) VL at depth z = (k + 0.5) VL projects to u_f = 30 / (k + 0.5) + 20, v_f = 22.5 / (k + 0.5) + 15: for
    k >= 30 that is pixel (20, 15), whose multiplier is m = sqrt((0.5 / 60)^2 + (0.5 / 45)^2 + 1).  tsdf = min(1, (0.25 - z) m /
    0.04) rounded to fp32, weight 1 while sdf > -0.04: z < 0.25 + 0.04 / m, i.e. k <= 36."""
    _, _, _, vol = _plane()
    m = np.sqrt(((20 - 19.5) / 60.0) ** 2 + ((15 - 14.5) / 45.0) ** 2 + 1.0)
    assert vol["block_unit"][6].tolist() == [0, 0, 1] and vol["block_unit"][7].tolist() == [0, 0, 2]
    col = {16 + i: (vol["tsdf"][6][0, 0, i], vol["weight"][6][0, 0, i]) for i in range(16)}
    col.update({32 + i: (vol["tsdf"][7][0, 0, i], vol["weight"][7][0, 0, i]) for i in range(16)})
    for k in range(30, 48):
        z = (k + 0.5) * VL
        sdf = (0.25 - z) * m
        if k <= 36:
            assert sdf > -0.04 and col[k] == (np.float32(min(1.0, sdf / 0.04)), 1), k
        else:
            assert sdf <= -0.04 and col[k] == (0.0, 0), k
    assert col[31][0] > 0 > col[32][0] and col[26][0] == 1.0           # the surface between voxels 31 and 32; the clamp in front


def test_points_lie_on_axis_two_within_the_bound_the_multipliers_imply():
    """With f_k = (d - z_k) m_k / s on both sides (neither is clamped inside the band), a = d - z0, b = z1 - d, a + b = VL, the crossing
    is at d + a b (m0 - m1) / (a m0 + b m1): |z - d| <= (VL / 4) |m0 - m1| / min(m0, m1), m0 and m1 the multipliers of the pixels the
    two bracketing voxels project to (they differ only where the 2 % change of depth moves the projection over a pixel border).
    Rounding adds 2^-23 (d + VL): the two fp32 values and the fp32 result."""
    _, lo, dims, vol = _plane()
    pts, M, flags = T.extract(vol["tsdf"], vol["weight"], vol["block_unit"], lo, dims, VL)
    assert M == len(pts) > 300 and flags == 0
    fx, fy, cx, cy = K
    p = pts.astype(np.float64)
    frac = p / VL - 0.5
    assert (frac[:, :2] == np.rint(frac[:, :2])).all()                # x and y are voxel centres: every point is a crossing on axis 2
    assert ((p[:, 2] > 31.5 * VL) & (p[:, 2] < 32.5 * VL)).all()

    def multiplier(z):
        pu, pv = np.floor((p[:, 0] * fx) / z + cx + 0.5), np.floor((p[:, 1] * fy) / z + cy + 0.5)
        return np.sqrt(((pu - cx) / fx) ** 2 + ((pv - cy) / fy) ** 2 + 1.0)

    m0, m1 = multiplier(31.5 * VL), multiplier(32.5 * VL)
    bound = VL / 4 * np.abs(m0 - m1) / np.minimum(m0, m1) + 2.0 ** -23 * (0.25 + VL)
    err = np.abs(p[:, 2] - 0.25)
    print(f"{M} points, worst |z - d| = {err.max() / VL:.2e} VL, worst bound = {bound.max() / VL:.2e} VL, worst ratio {(err / bound).max():.3f}")
    assert (err <= bound).all() and (m0 != m1).any() and bound.max() < 5e-3 * VL


# ---- refusals through the C ABI, no device ----------------------------------------------------------------------------------

def _lib_():
    from epn_pointcloud_amd import _lib
    return _lib.get_lib()


OK = dict(depth=16, F=2, H=30, W=40, cam2base=16, base2cam=16, fx=60.0, fy=45.0, cx=19.5, cy=14.5, depth_scale=1000.0, depth_trunc=6.0,
          voxel_length=VL, sdf_trunc=0.04, stride=4, lo=(-2, -2, 0), dims=(4, 4, 4), max_blocks=64, block_unit=16, block_mask=16, tsdf=16,
          weight=16, status=16, workspace=16, workspace_bytes=None)


def _ws(a):
    return int(_lib_().epn_tsdf_fuse_workspace_bytes(a["F"], a["H"], a["W"], a["stride"], *a["dims"], a["max_blocks"]))


def _vp(v):
    return ctypes.c_void_p(v) if v else None


def _fuse(**over):
    """Pointers: non-NULL, 16-byte aligned and never dereferenced (every call is refused)."""
    a = dict(OK)
    a.update(over)
    wb = _ws(OK) if a["workspace_bytes"] is None else a["workspace_bytes"]
    return _lib_().epn_tsdf_fuse_f32(_vp(a["depth"]), a["F"], a["H"], a["W"], _vp(a["cam2base"]), _vp(a["base2cam"]), a["fx"], a["fy"],
                                     a["cx"], a["cy"], a["depth_scale"], a["depth_trunc"], a["voxel_length"], a["sdf_trunc"], a["stride"],
                                     *a["lo"], *a["dims"], a["max_blocks"], _vp(a["block_unit"]), _vp(a["block_mask"]), _vp(a["tsdf"]),
                                     _vp(a["weight"]), _vp(a["status"]), _vp(a["workspace"]), wb, None)


NAN, INF = float("nan"), float("inf")
BAD = [dict(F=0), dict(F=65), dict(H=0), dict(W=0), dict(W=16385), dict(stride=0), dict(stride=-4)] \
    + [{k: v} for k in ("fx", "fy", "depth_scale", "depth_trunc", "voxel_length", "sdf_trunc") for v in (0.0, -1.0, NAN, INF)] \
    + [dict(cx=NAN), dict(cy=INF), dict(depth_scale=1e39), dict(sdf_trunc=8 * VL * (1 + 2.0 ** -52)), dict(dims=(4, 0, 4)), dict(dims=(-1, 4, 4)),
       dict(dims=(256, 256, 257)), dict(dims=(65536, 65536, 65536)), dict(lo=(2 ** 24 + 1, 0, 0)), dict(lo=(0, 0, -2 ** 24 - 1)),
       dict(max_blocks=0), dict(max_blocks=2 ** 17 + 1), dict(tsdf=24), dict(weight=8)]


@pytest.mark.parametrize("bad", BAD, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_bad_arguments_are_refused_before_any_runtime_call(bad):
    assert _fuse(workspace_bytes=2 ** 40, **bad) == EINVAL


@pytest.mark.parametrize("name", ["depth", "cam2base", "base2cam", "block_unit", "block_mask", "tsdf", "weight", "status"])
def test_null_pointers_are_refused(name):
    assert _fuse(**{name: 0}) == ENULL


def test_workspace_refusals_and_the_query():
    assert _fuse(workspace=0) == EWORKSPACE and _fuse(workspace=20) == EWORKSPACE and _fuse(workspace_bytes=_ws(OK) - 1) == EWORKSPACE
    assert _fuse(sdf_trunc=8 * VL, workspace=0) == EWORKSPACE          # sdf_trunc = 8 voxel_length itself is allowed
    D, nt, touch = 64, 1, 2 * 1                                         # 10 x 8 samples per frame: one workgroup each
    assert _ws(OK) >= 64 + 12 * D + 4 * (64 + nt + touch)
    for bad in (dict(F=0), dict(F=65), dict(stride=0), dict(dims=(256, 256, 257)), dict(max_blocks=0), dict(H=0)):
        assert _ws({**OK, **bad}) == 0
    assert _ws({**OK, "dims": (256, 256, 256)}) >= 12 * 2 ** 24


def _extract(**over):
    a = dict(tsdf=16, weight=16, block_unit=16, max_blocks=64, lo=(-2, -2, 0), dims=(4, 4, 4), voxel_length=VL, points=16, max_points=100,
             status=16, workspace=16, workspace_bytes=2 ** 40)
    a.update(over)
    return _lib_().epn_tsdf_extract_f32(_vp(a["tsdf"]), _vp(a["weight"]), _vp(a["block_unit"]), a["max_blocks"], *a["lo"], *a["dims"],
                                        a["voxel_length"], _vp(a["points"]), a["max_points"], _vp(a["status"]), _vp(a["workspace"]),
                                        a["workspace_bytes"], None)


def test_extract_refusals():
    for bad in (dict(voxel_length=0.0), dict(voxel_length=NAN), dict(dims=(4, 4, 0)), dict(dims=(256, 256, 257)), dict(max_blocks=0),
                dict(max_blocks=2 ** 17 + 1), dict(max_points=-1), dict(lo=(0, -2 ** 24 - 1, 0))):
        assert _extract(**bad) == EINVAL, bad
    for name in ("tsdf", "weight", "block_unit", "status", "points"):
        assert _extract(**{name: 0}) == ENULL, name
    assert _extract(workspace=0) == EWORKSPACE and _extract(workspace=12) == EWORKSPACE
    assert _extract(workspace_bytes=64 + 12 * 64 + 4 * 64 - 1) == EWORKSPACE
    assert _extract(points=0, max_points=0, workspace=0) == EWORKSPACE   # no points wanted: the pointer may be NULL


# ---- the Python layer -------------------------------------------------------------------------------------------------------

def _reference_windows(n, nframes=50):
    """the loop of run_fusion.py:84-98, its arithmetic only"""
    out, head, tail = [], 0, min(nframes, n)
    while tail <= n:
        out.append((head, tail))
        head = tail
        tail += nframes
    return out


@pytest.mark.parametrize("n", [49, 50, 99, 100, 101])
def test_windows_are_the_reference_loops(n):
    from epn_pointcloud_amd import fusion
    assert fusion.fragment_windows(n, 50) == _reference_windows(n)
    assert fusion.fragment_windows(n, 50) == {49: [(0, 49)], 50: [(0, 50)], 99: [(0, 50)], 100: [(0, 50), (50, 100)],
                                              101: [(0, 50), (50, 100)]}[n]


def test_fuse_sequence_cuts_those_windows(monkeypatch):
    from epn_pointcloud_amd import fusion
    seen = []
    monkeypatch.setattr(fusion, "fuse_fragment", lambda d, p, k, **kw: seen.append((d[0, 0, 0], len(d), len(p), kw)) or len(seen))
    depth = np.arange(101, dtype=np.uint16)[:, None, None] * np.ones((1, 2, 2), np.uint16)
    assert fusion.fuse_sequence(depth, np.tile(np.eye(4), (101, 1, 1)), K, stride=2) == [1, 2]
    assert seen == [(0, 50, 50, dict(stride=2)), (50, 50, 50, dict(stride=2))]
    with pytest.raises(ValueError):
        fusion.fuse_sequence(depth, np.tile(np.eye(4), (100, 1, 1)), K)


def _rot(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(4)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def test_frustum_box_holds_every_unit_the_restatement_allocates():
    from epn_pointcloud_amd import fusion
    rng = np.random.default_rng(5)
    for trial in range(6):
        F = 3
        poses = [np.eye(4)]
        for _ in range(F - 1):
            P = _rot(int(rng.integers(3)), rng.uniform(-0.6, 0.6)) @ _rot(int(rng.integers(3)), rng.uniform(-0.6, 0.6))
            P[:3, 3] = rng.uniform(-0.3, 0.3, 3)
            poses.append(P)
        world = _rot(1, 0.4)
        world[:3, 3] = (3.0, -2.0, 1.0)
        cam2world = np.stack([world @ P for P in poses])
        depth = rng.integers(0, 900, (F, 30, 40)).astype(np.uint16)     # anything from no measurement to beyond depth_trunc
        depth[:, 0, 0], depth[:, 28, 36] = 800, 800                      # the far corners of the sampled image, at depth_trunc
        cam2base, base2cam, pose = fusion.relative_poses(cam2world)
        assert np.array_equal(pose, cam2world[0]) and np.abs(cam2base[0] - np.eye(4)).max() < 1e-14
        assert np.abs(cam2base @ base2cam - np.eye(4)).max() < 1e-13
        lo, dims = fusion.frustum_unit_box(cam2base, K, 30, 40, 0.8, VL, 0.04)
        masks, n_outside = T.touch(depth, cam2base, K, 1000.0, 0.8, VL, 0.04, 4, lo, dims)
        assert n_outside == 0 and np.count_nonzero(masks) > 20
        wide = T.touch(depth, cam2base, K, 1000.0, 0.8, VL, 0.04, 4, [v - 3 for v in lo], [d + 6 for d in dims])[0]
        assert np.count_nonzero(wide) == np.count_nonzero(masks)         # nothing was allocated outside it either
        assert dims[0] * dims[1] * dims[2] < 40 ** 3                     # and it is a box around the frusta, not the world


def test_fuse_fragment_checks_its_arguments_before_the_device():
    from epn_pointcloud_amd import fusion
    d = np.zeros((2, 30, 40), np.uint16)
    eye2 = np.tile(np.eye(4), (2, 1, 1))
    for kw, text in ((dict(sdf_trunc=0.05), "8 voxel_length"), (dict(stride=0), "stride"), (dict(voxel_length=-1.0), "voxel_length"),
                     (dict(depth_trunc=float("nan")), "depth_trunc")):
        with pytest.raises(ValueError, match=text):
            fusion.fuse_fragment(d, eye2, K, **kw)
    with pytest.raises(ValueError, match="intrinsic"):
        fusion.fuse_fragment(d, eye2, (1.0, 2.0, 3.0))
    with pytest.raises(TypeError, match="uint16"):
        fusion.fuse_fragment(d.astype(np.float32), eye2, K)
    assert fusion._intrinsic(np.array([[60.0, 0, 19.5], [0, 45.0, 14.5], [0, 0, 1]])) == K
