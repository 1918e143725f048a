"""Voxel-grid downsampling on the GPU (csrc/voxel_grid.hip behind vgtk.cuda.grouping.voxel_downsample) against the numpy
restatement of its specification (tests/voxel_ref.py): bit for bit, every output.  Nothing here has been compared with
open3d itself."""
import numpy as np
import pytest
import torch

import voxel_ref as V

pytestmark = pytest.mark.gpu

T = 256                                   # the scan tile: points per workgroup of the ranking kernels (include/epn_so3conv.h)


def run(gpu, pc, voxel_size):
    from epn_pointcloud_amd.vgtk.cuda import grouping
    out = grouping.voxel_downsample(torch.from_numpy(np.ascontiguousarray(pc, dtype=np.float32)).to(gpu), voxel_size)
    return [o.cpu().numpy() for o in out]


def check(gpu, pc, voxel_size):
    """The four outputs equal the restatement's, bit for bit; returns them."""
    cen, cnt, first, pv, _, flags = V.voxel_downsample(pc, voxel_size)
    assert flags == 0
    got = run(gpu, pc, voxel_size)
    assert got[0].shape == cen.shape and got[0].dtype == np.float32
    assert np.array_equal(got[1], cnt) and np.array_equal(got[2], first) and np.array_equal(got[3], pv)
    assert np.array_equal(got[0].view(np.uint32), cen.view(np.uint32))
    return got


def test_one_point(gpu):
    got = check(gpu, np.array([[0.3, -0.2, 7.0]], np.float32), 0.03)
    assert got[0].tolist() == [[np.float32(0.3), np.float32(-0.2), 7.0]] and got[3].tolist() == [0]


def test_one_voxel_holds_every_point(gpu):
    """1000 points inside one voxel of edge 1, negative coordinates included: every atomic of the call lands on one slot."""
    pc = np.random.default_rng(0).uniform(-0.2, 0.2, (1000, 3)).astype(np.float32)
    got = check(gpu, pc, 1.0)
    assert got[1].tolist() == [1000] and (pc < 0).any() and (got[3] == 0).all()


def test_every_point_in_its_own_voxel(gpu):
    rng = np.random.default_rng(1)
    cells = rng.choice(40 ** 3, 5000, replace=False)
    idx = np.stack((cells // 1600, cells // 40 % 40, cells % 40), axis=1)
    pc = ((idx - 20) * 0.25 + rng.uniform(-0.05, 0.05, (5000, 3))).astype(np.float32)
    got = check(gpu, pc, 0.25)
    assert got[1].shape == (5000,) and (got[1] == 1).all() and np.array_equal(got[3], np.arange(5000))


def test_grid_valued_boundary_points(gpu):
    """voxel_size 2^-5, coordinates on multiples of half a voxel from the minimum: every odd multiple lies on a voxel face and
    belongs to the upper voxel; all arithmetic is exact."""
    vs = 2.0 ** -5
    rng = np.random.default_rng(2)
    half = rng.integers(0, 24, (3000, 3))
    half[0] = 0                                                     # the minimum on every axis
    pc = (-1.0 + half * (vs / 2)).astype(np.float32)
    got = check(gpu, pc, vs)
    want = (half + 1) // 2                                          # floor(m / 2 + 1 / 2)
    cells = {tuple(r) for r in want.tolist()}
    assert got[1].shape == (len(cells),)
    rows = got[3]
    assert np.array_equal(want[got[2]][rows], want)                 # every point shares its voxel's first point's cell


def test_non_finite_rows_are_dropped(gpu):
    rng = np.random.default_rng(3)
    pc = rng.uniform(-1, 1, (2000, 3)).astype(np.float32)
    bad = rng.choice(2000, 300, replace=False)
    pc[bad[:100], 0] = np.nan
    pc[bad[100:200], 1] = np.inf
    pc[bad[200:], 2] = -np.inf                                      # would be the minimum if it counted
    pc[bad[:50], 1] = -200.0                                        # finite coordinates of dropped rows move no bound either
    got = check(gpu, pc, 0.1)
    assert (got[3][bad] == -1).all() and (np.delete(got[3], bad) >= 0).all() and got[1].sum() == 1700
    none = run(gpu, np.full((70, 3), np.nan, np.float32), 0.1)
    assert none[0].shape == (0, 3) and none[1].shape == (0,) and (none[3] == -1).all()


@pytest.mark.parametrize("home", [5, 127], ids=["one_home_slot", "wraps_past_the_last_slot"])
def test_hash_collisions(gpu, home):
    """n = 64 -> capacity 128; 64 distinct voxels whose keys share one home slot, so the probes run up to 63 slots on; from
    home slot 127 they wrap to slot 0."""
    pc, idx = V.colliding_cloud(64, home)
    got = check(gpu, pc, 2.0 ** -5)
    assert got[1].shape == (64,) and np.array_equal(got[3], np.arange(64))


@pytest.mark.parametrize("n", [T - 1, T, T + 1, 2 * T + 1, T * T + 1])
def test_scan_edges(gpu, n):
    """One tile less a point, exactly one, one more, two and a point; T * T + 1 points give T + 1 per-tile sums, which the
    single scanning workgroup takes in two passes."""
    pc = np.random.default_rng(n).uniform(-1, 1, (n, 3)).astype(np.float32)
    got = check(gpu, pc, 0.1)
    assert 1 < got[1].shape[0] < n


def test_the_largest_cloud(gpu):
    """n = 2^22: 4096 points repeated 1024 times.  The voxels are the 4096 points' own, every count 1024-fold, and the centroids
    unchanged (sum and count scale by the same power of two)."""
    base = np.random.default_rng(5).uniform(-2, 2, (4096, 3)).astype(np.float32)
    cen, cnt, first, pv, _, _ = V.voxel_downsample(base, 0.25)
    got = run(gpu, np.tile(base, (1024, 1)), 0.25)
    assert np.array_equal(got[0].view(np.uint32), cen.view(np.uint32))
    assert np.array_equal(got[1], cnt * 1024) and np.array_equal(got[2], first)
    assert np.array_equal(got[3], np.tile(pv, 1024))


def test_range_errors_are_loud(gpu):
    pc = np.random.default_rng(6).uniform(-1, 1, (500, 3)).astype(np.float32)
    far = pc.copy()
    far[77, 1] = 300.0
    with pytest.raises(ValueError, match="bit 0"):
        run(gpu, far, 0.03)
    wide = pc.copy()
    wide[:, 0] *= 100.0                                             # extent 200
    with pytest.raises(ValueError, match="bit 1"):
        run(gpu, wide, 1e-5)
    check(gpu, pc, 0.03)                                            # the device is fine afterwards


def test_repeatable_and_independent_of_the_point_order(gpu):
    rng = np.random.default_rng(7)
    pc = (rng.uniform(-1.5, 1.5, (30_000, 3)) * [1, 1, 0.02]).astype(np.float32)       # a slab: about five points per voxel
    a, b = check(gpu, pc, 0.03), run(gpu, pc, 0.03)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    perm = rng.permutation(pc.shape[0])
    c = check(gpu, pc[perm], 0.03)
    ka = V.voxel_downsample(pc, 0.03)[4]
    kc = V.voxel_downsample(pc[perm], 0.03)[4]
    oa, oc = np.argsort(ka), np.argsort(kc)
    assert np.array_equal(ka[oa], kc[oc])
    assert np.array_equal(a[0][oa].view(np.uint32), c[0][oc].view(np.uint32)) and np.array_equal(a[1][oa], c[1][oc])
    assert np.array_equal(ka[a[3]][perm], kc[c[3]])                 # every point in the same voxel


def test_describe_downsamples_first(gpu):
    """The model of tests/test_gpu_patches.py::test_describe; four keypoints given as rows of the original fragment."""
    from epn_pointcloud_amd import models as M
    from epn_pointcloud_amd.vgtk import pc as pctk
    from test_models_cpu import fill_state_dict
    rng = np.random.default_rng(8)
    cloud = torch.from_numpy(rng.uniform(-1, 1, (4000, 3)).astype(np.float32)).to(gpu)
    rows = torch.from_numpy(rng.choice(4000, 4, replace=False)).to(gpu)
    m = fill_state_dict(M.build_inv(input_num=1024, search_radius=0.8, width_div=2)).to(gpu).eval()
    same = lambda a, b: torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    v = 0.1
    centroids = pctk.voxel_down_sample(cloud, v)[0]
    assert 1000 < centroids.shape[0] < 4000
    down = m.describe(cloud, rows, batch=4, seed=3, voxel_size=v)
    assert down[1].all() and same(down, m.describe(centroids, cloud[rows], batch=4, seed=3))
    plain = m.describe(cloud, rows, batch=4, seed=3)
    assert same(plain, m.describe(cloud, rows, batch=4, seed=3, voxel_size=None)) and not same(plain, down)
    assert pctk.reference_voxel_size(m.input_num) == 0.015
    assert same(m.describe(cloud, rows, batch=4, seed=3, voxel_size="reference"),
                m.describe(cloud, rows, batch=4, seed=3, voxel_size=0.015))
