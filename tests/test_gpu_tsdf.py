"""TSDF fusion on the device (csrc/tsdf_fusion.hip) against the numpy restatement of its specification (tests/tsdf_ref.py,
include/epn_so3conv.h: epn_tsdf_fuse_f32, epn_tsdf_extract_f32): EXACT equality on every output -- n_blocks, block_unit,
block_mask, weight, tsdf, M, points and the flags -- on scenes that are the smallest at which each mechanism can go wrong.  Every
operation of the specification is an IEEE fp64 operation rounded once (+, -, *, /, sqrt, floor) or an fp32 one formed through
fp64 (tsdf_math.h), so no ulp is allowed anywhere.  Rows past the limits are pre-filled with a sentinel and must keep it.

Scenes use voxel_length 2^-7 (unit_length 1/8) so that the named voxels' coordinates are exact; images are at most 40 x 30."""
import numpy as np
import pytest
import torch

import tsdf_ref as T

pytestmark = pytest.mark.gpu

VL = 2.0 ** -7
UL = 16 * VL
SENT_F, SENT_I = -7.5, -77


def _eye(n=1):
    return np.tile(np.eye(4), (n, 1, 1))


def _shift(x=0.0, y=0.0, z=0.0):
    T4 = np.eye(4)
    T4[:3, 3] = (x, y, z)
    return T4


def _box(scene, pad=0):
    """the tight box of the units the restatement's samples touch (+ pad)"""
    lo, hi = [], []
    for f in range(scene["depth"].shape[0]):
        p = T.sample_points(scene["depth"], scene["cam2base"], scene["K"], scene["depth_scale"], scene["depth_trunc"], scene["stride"], f)
        if p.size:
            lo.append(np.floor((p - scene["sdf_trunc"]) / UL).min(axis=0))
            hi.append(np.floor((p + scene["sdf_trunc"]) / UL).max(axis=0))
    lo, hi = np.min(lo, axis=0).astype(int) - pad, np.max(hi, axis=0).astype(int) + pad
    return [int(v) for v in lo], [int(v) for v in hi - lo + 1]


def make(depth, cam2base, K, sdf_trunc=0.04, stride=4, depth_trunc=6.0, depth_scale=1000.0):
    cam2base = np.ascontiguousarray(cam2base, dtype=np.float64)
    return dict(depth=np.ascontiguousarray(depth, dtype=np.uint16), cam2base=cam2base, base2cam=np.ascontiguousarray(np.linalg.inv(cam2base)),
                K=K, sdf_trunc=sdf_trunc, stride=stride, depth_trunc=depth_trunc, depth_scale=depth_scale)


def ref_fuse(s, lo, dims, max_blocks):
    return T.fuse(s["depth"], s["cam2base"], s["base2cam"], s["K"], lo, dims, max_blocks, depth_scale=s["depth_scale"],
                  depth_trunc=s["depth_trunc"], voxel_length=VL, sdf_trunc=s["sdf_trunc"], stride=s["stride"])


def dev_run(gpu, s, lo, dims, max_blocks, max_points, stream_repeat=False):
    """-> dict of host arrays: the WHOLE output tensors (sentinel rows included) and the two status words"""
    from epn_pointcloud_amd import fusion
    depth = torch.from_numpy(s["depth"].view(np.int16)).to(gpu)
    c2b, b2c = torch.from_numpy(s["cam2base"]).to(gpu), torch.from_numpy(s["base2cam"]).to(gpu)
    mb = max_blocks
    out = (torch.full((mb, 3), SENT_I, dtype=torch.int32, device=gpu), torch.full((mb,), SENT_I, dtype=torch.int64, device=gpu),
           torch.full((mb, 16, 16, 16), SENT_F, dtype=torch.float32, device=gpu), torch.full((mb, 16, 16, 16), SENT_I, dtype=torch.int32, device=gpu))
    points = torch.full((max(max_points, 1) + 2, 3), SENT_F, dtype=torch.float32, device=gpu)
    for _ in range(2 if stream_repeat else 1):      # the second pass is queued behind the first without a synchronisation
        bu, bm, ts, w, status, ws = fusion.tsdf_fuse(depth, c2b, b2c, s["K"], lo, dims, mb, depth_scale=s["depth_scale"],
                                                     depth_trunc=s["depth_trunc"], voxel_length=VL, sdf_trunc=s["sdf_trunc"],
                                                     stride=s["stride"], out=out)
        _, xstatus = fusion.tsdf_extract(ts, w, bu, ws, lo, dims, VL, max_points, points=points)
    torch.cuda.synchronize()
    return dict(block_unit=bu.cpu().numpy(), block_mask=bm.cpu().numpy().view(np.uint64), tsdf=ts.cpu().numpy(), weight=w.cpu().numpy(),
                status=status.tolist(), points=points.cpu().numpy(), xstatus=xstatus.tolist())


def check(gpu, s, lo=None, dims=None, max_blocks=None, max_points=None, **kw):
    """device == restatement on every output; -> (reference volume, reference points, device outputs)"""
    if lo is None:
        lo, dims = _box(s)
    full = ref_fuse(s, lo, dims, 1 << 17)
    mb = full["n_blocks"] if max_blocks is None else max_blocks
    ref = full if mb >= full["n_blocks"] else ref_fuse(s, lo, dims, mb)
    nb = min(ref["n_blocks"], mb)
    pts, M, _ = T.extract(ref["tsdf"], ref["weight"], ref["block_unit"], lo, dims, VL)
    mp = M if max_points is None else max_points
    got = dev_run(gpu, s, lo, dims, mb, mp, **kw)
    assert got["status"] == [ref["n_blocks"], ref["flags"], ref["n_outside"], 0]
    assert np.array_equal(got["block_unit"][:nb], ref["block_unit"]) and np.array_equal(got["block_mask"][:nb], ref["block_mask"])
    assert np.array_equal(got["weight"][:nb], ref["weight"])
    assert np.array_equal(got["tsdf"][:nb].view(np.uint32), ref["tsdf"].view(np.uint32))
    assert (got["block_unit"][nb:] == SENT_I).all() and (got["weight"][nb:] == SENT_I).all() and (got["tsdf"][nb:] == SENT_F).all()
    assert (got["block_mask"][nb:] == np.int64(SENT_I).astype(np.uint64)).all()
    assert got["xstatus"] == [M, T.FLAG_POINTS if M > mp else 0]
    k = min(M, mp)
    assert np.array_equal(got["points"][:k].view(np.uint32), pts[:k].view(np.uint32))
    assert (got["points"][k:] == SENT_F).all()
    return ref, pts, got


def flat(H, W, raw):
    return np.full((1, H, W), raw, dtype=np.uint16)


def voxel(ref, unit, idx):
    r = np.nonzero((ref["block_unit"] == np.asarray(unit)).all(axis=1))[0]
    assert r.size == 1, f"unit {unit} is not allocated"
    return float(ref["tsdf"][r[0]][tuple(idx)]), int(ref["weight"][r[0]][tuple(idx)])


K_EDGE = (60.0, 45.0, 19.5, 14.5)


def test_image_borders_exactly(gpu):
    """Plane at z = 0.25 = 32 voxels.  Voxel centres are half-integers of VL, so x fx / z is exact where the quotient is: the voxel
    (x, z) = (10.5, 31.5) VL has u_f = 20 + 19.5 + 0.5 = 40 = W exactly (skipped), its twin at x = -10.5 VL has u_f = 0 (kept: pixel
    0), and one voxel nearer to the camera in z they fall just outside, one farther just inside; the same on v with fy = 45."""
    s = make(flat(30, 40, 250), _eye(), K_EDGE)
    ref, pts, _ = check(gpu, s)
    fx, fy, cx, cy = K_EDGE
    assert ((10.5 * VL * fx) / (31.5 * VL) + cx) + 0.5 == 40.0 and ((-10.5 * VL * fx) / (31.5 * VL) + cx) + 0.5 == 0.0
    assert ((10.5 * VL * fy) / (31.5 * VL) + cy) + 0.5 == 30.0 and ((-10.5 * VL * fy) / (31.5 * VL) + cy) + 0.5 == 0.0
    assert voxel(ref, (0, 0, 1), (10, 0, 15))[1] == 0 and voxel(ref, (-1, 0, 1), (5, 0, 15))[1] == 1         # u_f = W, u_f = 0
    assert voxel(ref, (0, 0, 2), (10, 0, 0))[1] == 1 and voxel(ref, (-1, 0, 1), (5, 0, 14))[1] == 0          # just below W, just below 0
    assert voxel(ref, (0, 0, 1), (0, 10, 15))[1] == 0 and voxel(ref, (0, -1, 1), (0, 5, 15))[1] == 1         # v_f = H, v_f = 0
    assert voxel(ref, (0, 0, 2), (0, 10, 0))[1] == 1 and voxel(ref, (0, -1, 1), (0, 5, 14))[1] == 0
    assert (ref["block_unit"] < 0).any() and (ref["tsdf"] == 1.0).any()      # negative coordinates by floor; the clamp at 1
    # the surface sits on the face between voxel 15 of unit 1 and voxel 0 of unit 2: every point crosses it, on axis 2
    assert len(pts) and ((pts[:, 2] > 31.5 * VL) & (pts[:, 2] < 32.5 * VL)).all()


K_WIDE = (20.0, 20.0, 20.0, 15.0)


def test_sdf_at_the_truncation_and_depth_at_the_limit(gpu):
    """cx, cy integers: pixel (20, 15) has multiplier 1, so sdf = d - z exactly.  sdf_trunc = 3.5 VL: the voxel at z = 35.5 VL has
    sdf = -sdf_trunc exactly (skipped: strict), the one before it sdf = -2.5 VL (kept).  depth_trunc = 0.25: raw 250 is AT the
    limit (kept), raw 251 above it (no measurement), raw 0 none either."""
    d = flat(30, 40, 250)
    d[0, :, :8] = 251
    d[0, :12, 8:16] = 0
    s = make(d, _eye(), K_WIDE, sdf_trunc=3.5 * VL, depth_trunc=0.25)
    ref, _, _ = check(gpu, s)
    assert np.float64(np.float32(250) / np.float32(1000)) - 35.5 * VL == -3.5 * VL
    assert voxel(ref, (0, 0, 2), (0, 0, 3))[1] == 0 and voxel(ref, (0, 0, 2), (0, 0, 2)) == (float(np.float32(-2.5 / 3.5)), 1)
    dv = T.depth_values(d, 1000.0, 0.25)
    assert (dv[0, :, :8] == 0).all() and (dv[0, 12:, 8:] == 0.25).all()
    units_x = ref["block_unit"][:, 0]
    assert units_x.min() > np.floor(((0 - 20.0) * 0.251 / 20.0) / UL)          # the columns above the limit touched nothing


def test_behind_the_camera_and_a_unit_only_the_second_frame_touches(gpu):
    """Frame 1 stands at z = -6.5 VL, behind frame 0, and sees the same plane (raw 301) and one near pixel (raw 30, at z = -0.02):
    the units z = -1 and 0 around that pixel are touched by frame 1 alone (mask 2).  Frame 0 sees the voxels of unit z = 0 (they
    project into its image, where the plane's depth would give t = 1), yet they carry frame 1's observation alone (weight <= 1).
    The voxels of unit z = -1 at index <= 9 are behind frame 1 (c_2 <= 0, index 9 exactly 0) and behind frame 0."""
    d = np.repeat(flat(30, 40, 250), 2, axis=0)
    d[1] = 301
    d[1, 12, 20] = 30
    s = make(d, np.stack((np.eye(4), _shift(z=-6.5 * VL))), K_WIDE)
    ref, _, _ = check(gpu, s)
    only = ref["block_mask"] == 2
    assert only.any() and (ref["block_mask"] == 3).any() and not (ref["block_mask"] == 1).any()
    assert ref["weight"][only].max() == 1 and ref["weight"][ref["block_mask"] == 3].max() == 2
    assert {-1, 0} <= set(ref["block_unit"][only][:, 2].tolist())
    zc = T.transform(s["base2cam"][1], np.array([[0.5 * VL, 0.5 * VL, -6.5 * VL], [0.5 * VL, 0.5 * VL, -7.5 * VL]]))[:, 2]
    assert zc[0] == 0.0 and zc[1] < 0
    assert voxel(ref, (0, 0, -1), (0, 0, 9))[1] == 0 and voxel(ref, (0, 0, -1), (0, 0, 12))[1] == 1


def test_stride_that_divides_neither_side_and_two_units_on_every_axis(gpu):
    s = make(T.render_plane(29, 37, K_WIDE, np.eye(4), (0.3, -0.2, 1.0), 0.2)[None], _eye(), K_WIDE, stride=3)
    check(gpu, s)
    p = T.sample_points(s["depth"], s["cam2base"], s["K"], 1000.0, 6.0, 3, 0)
    assert p.shape[0] == 13 * 10                                               # ceil(37 / 3) x ceil(29 / 3), all with a measurement
    two = (np.floor((p - 0.04) / UL) != np.floor((p + 0.04) / UL)).all(axis=1)
    assert two.any()                                                           # a sample whose box spans 2 x 2 x 2 units


def test_sixty_four_frames_with_bit_63(gpu):
    K = (10.0, 10.0, 4.0, 3.0)
    poses = np.stack([_shift(x=0.003 * f, y=-0.002 * f) for f in range(64)])
    s = make(np.repeat(flat(6, 8, 250), 64, axis=0), poses, K, stride=2)
    ref, _, _ = check(gpu, s)
    assert (ref["block_mask"] >> np.uint64(63)).any() and ref["weight"].max() == 64


def test_directory_longer_than_one_scan_pass(gpu):
    """41^3 = 68 921 entries = 270 tiles: the scan of the tile sums takes two passes of 256, and the scene's last units lie in the
    last tile (x = y = 40), its first ones in the first pass."""
    s = make(flat(30, 40, 250), _eye(), K_WIDE)
    lo, dims = _box(s)
    hi = [a + b - 1 for a, b in zip(lo, dims)]
    lo41 = [h - 40 for h in hi]
    ref, _, _ = check(gpu, s, lo41, [41, 41, 41])
    rel = ref["block_unit"] - np.asarray(lo41)
    e = (rel[:, 0] * 41 + rel[:, 1]) * 41 + rel[:, 2]
    assert e.max() == 41 ** 3 - 1 and e.min() < 65536 and (np.diff(e) > 0).all()


@pytest.mark.parametrize("where", ["first", "last", "alone"])
def test_a_single_unit_at_either_end_of_the_directory(gpu, where):
    d = np.zeros((1, 30, 40), dtype=np.uint16)
    d[0, 20, 24] = 310                                                         # (0.062, 0.0775, 0.31): +- 0.03125 stays in unit (0, 0, 2)
    s = make(d, _eye(), K_WIDE, sdf_trunc=4 * VL)
    lo, dims = {"first": ([0, 0, 2], [3, 3, 3]), "last": ([-2, -2, 0], [3, 3, 3]), "alone": ([0, 0, 2], [1, 1, 1])}[where]
    ref, _, _ = check(gpu, s, lo, dims)
    assert ref["n_blocks"] == 1 and ref["flags"] == 0 and ref["block_unit"].tolist() == [[0, 0, 2]]


def test_samples_outside_the_box_are_flagged_and_counted(gpu):
    """The box stops below unit z = 2, which the samples of the plane at 0.25 touch: all of them are counted, the flag is raised,
    the crossing between voxel 15 of unit 1 and the unit outside the box gives no point, and nothing is read out of range."""
    s = make(flat(30, 40, 250), _eye(), K_EDGE)
    lo, dims = _box(s)
    assert lo[2] == 1 and dims[2] == 2
    ref, pts, _ = check(gpu, s, lo, [dims[0], dims[1], 1])
    assert ref["flags"] == T.FLAG_OUTSIDE and ref["n_outside"] == 10 * 8 and len(pts) == 0


def test_crossings_between_units_on_each_axis(gpu):
    """Three frames, each looking along one axis at the plane (axis = 0.25), which is a face between two units: points of all three
    axes between voxel 15 of one unit and voxel 0 of the next."""
    Rx = np.array([[0, 0, 1, 0], [0, 1, 0, 0], [-1, 0, 0, 0], [0, 0, 0, 1.0]])          # the camera's z is the base's x
    Ry = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0], [0, 0, 0, 1.0]])          # the camera's z is the base's y
    s = make(np.repeat(flat(30, 40, 250), 3, axis=0), np.stack((np.eye(4), Rx, Ry)), K_EDGE)
    ref, pts, _ = check(gpu, s)
    frac = pts.astype(np.float64) / VL - 0.5
    for a in range(3):
        on_a = (pts[:, a] > 31.5 * VL) & (pts[:, a] < 32.5 * VL) & (frac[:, a] != np.rint(frac[:, a]))
        assert on_a.any(), f"no crossing of a unit face on axis {a}"


def test_next_unit_absent(gpu):
    """sdf_trunc = VL / 2 and the plane at raw 244 = 31.232 VL: the samples touch z in 30.7 .. 31.8 VL, unit 1 only.  Voxel 15 (31.5 VL)
    takes part, its +z neighbour's unit was never allocated: no point, no read."""
    s = make(flat(30, 40, 244), _eye(), K_WIDE, sdf_trunc=0.5 * VL)
    ref, pts, _ = check(gpu, s)
    assert set(ref["block_unit"][:, 2].tolist()) == {1}
    f, w = voxel(ref, (0, 0, 1), (0, 0, 15))
    assert w == 1 and -0.98 <= f < 0 and len(pts) == 0


def test_one_block_short_and_one_point_short(gpu):
    s = make(flat(30, 40, 250), _eye(), K_EDGE)
    full, pts, _ = check(gpu, s)
    ref, short_pts, _ = check(gpu, s, *_box(s), max_blocks=full["n_blocks"] - 1)
    assert ref["flags"] == T.FLAG_BLOCKS and ref["n_blocks"] == full["n_blocks"] and 0 < len(short_pts) < len(pts)
    _, _, got = check(gpu, s, max_points=len(pts) - 1)
    assert got["xstatus"] == [len(pts), T.FLAG_POINTS]


def test_two_runs_and_a_queued_repeat_are_bitwise_equal(gpu):
    s = make(np.stack((T.render_plane(30, 40, K_WIDE, np.eye(4), (0.1, 0.2, 1.0), 0.25),
                       T.render_plane(30, 40, K_WIDE, _shift(x=0.02), (0.1, 0.2, 1.0), 0.25))), np.stack((np.eye(4), _shift(x=0.02))), K_WIDE)
    _, _, a = check(gpu, s)
    _, _, b = check(gpu, s, stream_repeat=True)
    for k in ("block_unit", "block_mask", "weight", "status", "xstatus"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["tsdf"].view(np.uint32), b["tsdf"].view(np.uint32))
    assert np.array_equal(a["points"].view(np.uint32), b["points"].view(np.uint32))


def test_fuse_two_views_then_normals(gpu, vgtk_alias):
    """fuse_fragment -> PointGrid -> estimate_normals(view = origin) on two fronto-parallel views of the plane z = 0.25.
    Bound on the points: a frame's observation of a voxel at depth z is t = min(1, (d - z) m / s) with m its pixel's multiplier in
    [1, m_max], m_max = sqrt(1 + a_max^2 + b_max^2) over the image; a clamped t equals (d - z) m' / s with 1 <= m' <= m (clamping
    needs (d - z) / s < 1 for the voxel to take part at all).  So the mean over frames is (d - z) M / s with M in [1, m_max], and the
    crossing between z0 < d < z1 (a = d - z0, b = z1 - d, a + b = VL) lies at d + a b (M0 - M1) / (a M0 + b M1): within
    eps = (VL / 4) (m_max - 1) of d, plus the fp32 roundings of the two values and of the result, 2^-23 (d + VL).
    Bound on the normal: with the points (x, y, d + e), |e| <= eps, the covariance is [[Cxy, c], [c^T, v]], |c| <= eps sqrt(lam2),
    v <= eps^2, and its lowest eigenvalue mu <= v; its eigenvector satisfies (Cxy - mu) n_xy = -c n_z, so
    tan(angle to the z axis) <= eps sqrt(lam2) / (lam1 - eps^2), lam1 <= lam2 the in-plane eigenvalues of the neighbourhood."""
    import vgtk.pc as pc
    K = (60.0, 60.0, 19.5, 14.5)
    poses = np.stack((_shift(x=1.0, y=2.0, z=3.0), _shift(x=1.02, y=2.01, z=3.0)))        # the world is not the base frame
    frag = pc.fuse_fragment(np.repeat(flat(30, 40, 250), 2, axis=0), poses, K, voxel_length=VL, stride=4, device=gpu)
    assert np.array_equal(frag.pose_base2world, poses[0]) and frag.flags == 0 and frag.n_blocks > 0
    pts = frag.points.cpu().numpy().astype(np.float64)
    m_max = np.sqrt(1.0 + (20.5 / 60.0) ** 2 + (15.5 / 60.0) ** 2)
    eps = VL / 4 * (m_max - 1.0) + 2.0 ** -23 * (0.25 + VL)
    # the sampled pixels alone span 36 / 60 x 28 / 60 at depth 0.25: 19 x 14 voxel columns
    assert len(pts) > 19 * 14 and np.abs(pts[:, 2] - 0.25).max() <= eps
    radius = 4.3 * VL          # squared lattice distances are integers of VL^2: 18 is inside, 20 outside, no tie for fp32 to break
    normals = pc.estimate_normals(pc.PointGrid(frag.points, radius), radius, max_nn=0, view=(0.0, 0.0, 0.0))
    n = normals.normals.cpu().numpy().astype(np.float64)
    ok = normals.flags.cpu().numpy() == 0
    d2 = ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(axis=2)
    worst, tested = 0.0, 0
    for i in np.nonzero(ok)[0]:
        near = d2[i] <= radius * radius
        if near.sum() < 8:
            continue
        lam = np.linalg.eigvalsh(np.cov(pts[near, :2].T, bias=True))
        if lam[0] <= 100 * eps * eps:
            continue
        bound = np.arctan(eps * np.sqrt(lam[1]) / (lam[0] - eps * eps)) + 2.0 ** -20
        angle = np.arccos(np.clip(-n[i, 2] / np.linalg.norm(n[i]), -1, 1))
        worst = max(worst, angle / bound)
        tested += 1
    print(f"{tested} normals, worst angle / bound = {worst:.3f}, eps = {eps / VL:.4f} VL")
    assert tested > 19 * 14 and worst <= 1.0
