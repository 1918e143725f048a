"""The point grid on the GPU (csrc/point_grid.hip behind vgtk.pc.PointGrid) and the keypoint stage built on it
(epn_pointcloud_amd/correspondence.py) against the numpy restatement of their specification (tests/grid_nn_ref.py: brute force,
no grid): bit for bit, nn_idx and the bits of nn_d2.  Nothing here has been compared with open3d."""
import itertools

import numpy as np
import pytest
import torch

import grid_nn_ref as G
import voxel_ref as V

pytestmark = pytest.mark.gpu

R = 0.25                                   # the max_radius of most cases
E = float(G.cell_edge(R))                  # its cell edge; with a reference point at the origin cell k is centred on k * E


def D(gpu, a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(gpu)


def grid_of(gpu, ref, max_radius, valid=None):
    from epn_pointcloud_amd.vgtk import pc as pctk
    ref = np.asarray(ref, np.float32).reshape(-1, 3)
    return pctk.PointGrid(D(gpu, ref), max_radius, None if valid is None else D(gpu, valid, np.uint8))


def check(gpu, ref, qry, radius, max_radius=None, valid=None, exclude_self=False, grid=None):
    """nn_idx, the bits of nn_d2 and hits equal the restatement's; returns (nn_idx, nn_d2) of the device."""
    ref, qry = np.asarray(ref, np.float32).reshape(-1, 3), np.asarray(qry, np.float32).reshape(-1, 3)
    grid = grid or grid_of(gpu, ref, max_radius or radius, valid)
    idx, d2, hits = grid.nearest(D(gpu, qry), radius, exclude_self=exclude_self, count=True)
    want_idx, want_d2 = G.nearest(ref, qry, radius, valid=valid, exclude_self=exclude_self)
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    assert idx.dtype == np.int32 and d2.dtype == np.float32 and idx.shape == want_idx.shape
    assert np.array_equal(idx, want_idx)
    assert np.array_equal(d2.view(np.uint32), want_d2.view(np.uint32))
    assert hits.tolist() == [int((want_idx >= 0).sum())]
    return idx, d2


@pytest.mark.parametrize("n, m", list(itertools.product((0, 1), (0, 1))))
def test_empty_and_single(gpu, n, m):
    ref = np.array([[0.5, -0.25, 1.0]], np.float32)[:n]
    qry = np.array([[0.5, -0.125, 1.0]], np.float32)[:m]
    idx, d2 = check(gpu, ref, qry, R)
    if n and m:
        assert idx.tolist() == [0] and d2.tolist() == [0.015625]
    elif m:
        assert idx.tolist() == [-1] and np.isinf(d2).all()


@pytest.mark.parametrize("m", [1, 3, 4, 5])
def test_query_counts_around_a_workgroup_of_four_waves(gpu, m):
    rng = np.random.default_rng(m)
    ref = rng.uniform(-1, 1, (300, 3)).astype(np.float32)
    idx, _ = check(gpu, ref, ref[100:100 + m] + np.float32(0.01), R)
    assert (idx >= 0).all()


NEIGHBOURS = [d for d in itertools.product((-1, 0, 1), repeat=3) if d != (0, 0, 0)]


def test_every_neighbouring_cell_is_searched_and_no_further(gpu):
    """The origin fixes the grid; the query sits at the centre of cell (5, 5, 5).  One more reference point per case, half a cell
    and 0.01 along every moved axis: in the neighbouring cell, at most sqrt(3) * 0.1351 = 0.2340 away.  Found at radius ==
    max_radius and at 0.24 on the same grid.  A point two cells on is beyond every radius the grid admits: not found."""
    q = np.full((1, 3), 5 * E, np.float32)
    for d in NEIGHBOURS:
        p = q[0] + np.array(d) * (E / 2 + 0.01)
        ref = np.array([[0, 0, 0], p], np.float32)
        _, cells, flags = G.cell_indices(ref, R)
        assert flags == 0 and cells.tolist() == [[0, 0, 0], [5 + d[0], 5 + d[1], 5 + d[2]]]
        grid = grid_of(gpu, ref, R)
        for radius in (R, 0.24):
            assert check(gpu, ref, q, radius, grid=grid)[0].tolist() == [1], (d, radius)
    for axis in range(3):
        for side in (-1, 1):
            ref = np.zeros((2, 3), np.float32)
            ref[1] = q[0]
            ref[1, axis] += side * (1.5 * E + 0.01)
            assert G.cell_indices(ref, R)[1][1, axis] == 5 + 2 * side
            grid = grid_of(gpu, ref, R)
            for radius in (R, 0.24):
                assert check(gpu, ref, q, radius, grid=grid)[0].tolist() == [-1]


def test_a_query_on_a_cell_border_reaches_the_lower_cells(gpu):
    """The query just above the corner shared by cells (4..5)^3: seven of its neighbours hold a point 0.1 below the corner on
    every moved axis."""
    corner = 4.5 * E
    q = np.full((1, 3), corner + 1e-4, np.float32)
    assert G.cell_indices(np.vstack((np.zeros((1, 3)), q)), R)[1][1].tolist() == [5, 5, 5]
    for d in itertools.product((-1, 0), repeat=3):
        if d == (0, 0, 0):
            continue
        ref = np.array([[0, 0, 0], q[0] + np.array(d) * 0.1], np.float32)
        assert G.cell_indices(ref, R)[1][1].tolist() == [5 + d[0], 5 + d[1], 5 + d[2]]
        assert check(gpu, ref, q, R)[0].tolist() == [1]


def test_the_radius_edge_is_inside(gpu):
    ref = np.zeros((1, 3), np.float32)
    above = np.nextafter(np.float32(0.5), np.float32(1))
    qry = np.array([[0.5, 0, 0], [above, 0, 0], [0, -0.5, 0], [0, 0, -above]], np.float32)
    idx, d2 = check(gpu, ref, qry, 0.5)
    assert idx.tolist() == [0, -1, 0, -1] and d2[0] == 0.25         # d2 == r2 = 0.25 exactly; the next float's square is above
    assert check(gpu, ref, qry, 0.5, max_radius=1.0)[0].tolist() == [0, -1, 0, -1]


def test_ties_return_the_lowest_row(gpu):
    rng = np.random.default_rng(11)
    far = rng.uniform(2, 3, (60, 3)).astype(np.float32)
    two = np.vstack((far[:20], [[0.125, 0, 0]], far[20:40], [[-0.125, 0, 0]], far[40:]))
    assert check(gpu, two, np.zeros((1, 3)), R)[0].tolist() == [20]
    three = np.vstack((far[:7], [[0, 0, -0.125]], far[7:30], [[0, 0.125, 0]], far[30:], [[0.125, 0, 0]]))
    assert check(gpu, three, np.zeros((1, 3)), R)[0].tolist() == [7]
    dup = np.vstack((far[:3], [[0.5, 0.5, 0.5]], far[3:33], [[0.5, 0.5, 0.5]] * 70))   # 71 copies: more than one pass of a wave
    idx, d2 = check(gpu, dup, [[0.5, 0.5, 0.5], [0.5, 0.4375, 0.5]], R)
    assert idx.tolist() == [3, 3] and d2.tolist() == [0.0, 0.00390625]


def test_cells_of_many_sizes_next_to_empty_ones(gpu):
    """Clusters of 1, 63, 64, 65, 129 and 257 points, each inside one cell, three cells apart: a wave's passes of 64 candidates
    end inside, at and just past a cell's run."""
    rng = np.random.default_rng(12)
    sizes = (1, 63, 64, 65, 129, 257)
    centres = np.array([[3 * k * E, (k % 2) * 3 * E, 0] for k in range(1, len(sizes) + 1)])   # cell centres, given the anchor
    ref = np.vstack([np.full((1, 3), -3 * E)] + [c + rng.uniform(-0.1, 0.1, (s, 3)) for c, s in zip(centres, sizes)]).astype(np.float32)
    _, cells, _ = G.cell_indices(ref, R)
    assert sorted(np.unique(cells, axis=0, return_counts=True)[1].tolist()) == sorted((1,) + sizes)
    qry = np.vstack([c + rng.uniform(-0.3, 0.3, (40, 3)) for c in centres]).astype(np.float32)
    idx, _ = check(gpu, ref[rng.permutation(ref.shape[0])], qry, R)
    assert 0.3 < (idx >= 0).mean() < 1.0
    check(gpu, ref, qry, 0.05, max_radius=R)


@pytest.mark.parametrize("home", [5, 127], ids=["one_home_slot", "wraps_past_the_last_slot"])
def test_hash_collisions(gpu, home):
    """n = 64 -> capacity 128; 64 occupied cells whose keys share one home slot, so a lookup probes up to 63 slots on and, from
    home slot 127, wraps to slot 0.  max_radius is chosen so that the cell edge is 2^-5, the collision cloud's."""
    max_radius = 2.0 ** -5 / (1 + 2.0 ** -10)
    pc, cells = V.colliding_cloud(64, home)
    part, got, flags = G.cell_indices(pc, max_radius)
    assert flags == 0 and np.array_equal(got, cells)
    assert {V.home_slot(int(V.make_key(*c)), 128) for c in cells.tolist()} == {home}
    qry = (pc + np.random.default_rng(home).uniform(-0.005, 0.005, pc.shape)).astype(np.float32)
    idx, _ = check(gpu, pc, qry, max_radius)
    assert np.array_equal(idx, np.arange(64))
    far = qry + np.float32(2.0 ** -5) * np.float32([0, 0, 40])      # cells that share the probe sequences but hold nothing
    assert (check(gpu, pc, far, max_radius)[0] == -1).all()


def test_queries_out_of_range_and_non_finite_rows(gpu):
    rng = np.random.default_rng(13)
    ref = rng.uniform(-1, 1, (500, 3)).astype(np.float32)
    ref[7] = [np.nan, 0, 0]
    ref[8] = [0, np.inf, 0]
    ref[9] = [0, 0, -np.inf]                                        # would move the minimum if it counted
    qry = [[0, 0, 0]]
    for axis in range(3):
        for v in (-1000.0, 1000.0, -3e5, 3e5, -1e30, 1e30, np.nan, np.inf, -np.inf):
            q = [0.0, 0.0, 0.0]
            q[axis] = v
            qry.append(q)
    qry += [[0, np.inf, 0], [0, 0, -1.0], ref[8].tolist(), [0, 0.9, 0]]
    idx, _ = check(gpu, ref, qry, R)
    assert idx[0] >= 0 and (idx[1:28] == -1).all()
    assert not np.isin(idx, (7, 8, 9)).any()
    near = np.nan_to_num(ref[7:10], nan=0.0, posinf=0.99, neginf=-0.99).astype(np.float32)
    assert not np.isin(check(gpu, ref, near, R)[0], (7, 8, 9)).any()


def test_range_errors_are_loud(gpu):
    ref = np.random.default_rng(14).uniform(-1, 1, (300, 3)).astype(np.float32)
    far = ref.copy()
    far[77, 1] = 300.0
    with pytest.raises(ValueError, match="bit 0"):
        grid_of(gpu, far, R)
    masked = np.ones(300, np.uint8)
    masked[77] = 0
    check(gpu, far, ref[:20], R, valid=masked)                      # a point that takes no part raises no flag
    wide = ref.copy()
    wide[:, 0] *= 100.0                                             # extent 200
    with pytest.raises(ValueError, match="bit 1"):
        grid_of(gpu, wide, 1e-5)
    g = grid_of(gpu, ref, R)
    with pytest.raises(ValueError, match="max_radius"):
        g.nearest(D(gpu, ref[:4]), 0.26)
    check(gpu, ref, ref[:20], R, grid=g)                            # the device is fine afterwards


def test_the_valid_mask(gpu):
    rng = np.random.default_rng(15)
    ref = rng.uniform(-1, 1, (400, 3)).astype(np.float32)
    qry = rng.uniform(-1, 1, (100, 3)).astype(np.float32)
    first = G.nearest(ref, qry, 0.5)[0]
    valid = np.ones(400, np.uint8)
    valid[first[first >= 0]] = 0                                    # every query's nearest point is masked
    idx, _ = check(gpu, ref, qry, 0.5, valid=valid)
    assert (idx >= 0).any() and not np.isin(idx[idx >= 0], first).any()
    from epn_pointcloud_amd.vgtk import pc as pctk
    g = pctk.PointGrid(D(gpu, ref), 0.5, torch.from_numpy(valid.astype(bool)).to(gpu))   # bool is taken as well
    assert g.kept == int(valid.sum())
    check(gpu, ref, qry, 0.5, valid=valid, grid=g)
    assert (check(gpu, ref, qry, 0.5, valid=np.zeros(400, np.uint8))[0] == -1).all()


def test_exclude_self(gpu):
    rng = np.random.default_rng(16)
    ref = rng.uniform(-1, 1, (600, 3)).astype(np.float32)
    ref[500] = ref[20]                                              # a duplicate at another row
    idx, d2 = check(gpu, ref, ref, R)
    assert np.array_equal(np.delete(idx, 500), np.delete(np.arange(600), 500)) and idx[500] == 20 and (d2 == 0).all()
    idx, d2 = check(gpu, ref, ref, R, exclude_self=True)
    assert (idx != np.arange(600)).all() and idx[20] == 500 and idx[500] == 20 and d2[20] == 0 and d2[500] == 0
    assert (np.delete(d2, (20, 500)) > 0).all() and (idx == -1).any() and (idx >= 0).any()


@pytest.mark.parametrize("radius", [0.25, 0.0625])
def test_lattice_clouds(gpu, radius):
    """The clouds of tests/test_grid_nn_spec.py's sklearn comparison: every distance is exact, ties included."""
    ref, qry = G.lattice_clouds()
    idx, _ = check(gpu, ref, qry, radius, max_radius=0.25)
    assert (idx >= 0).any() and (radius == 0.25 or (idx == -1).any())


def test_repeatable_and_replayed_from_a_captured_graph(gpu):
    """Two runs are bitwise equal.  Build and query, captured into one HIP graph on a single stream through the raw wrappers
    (nothing is read back), replay after the queries were rewritten in place."""
    from epn_pointcloud_amd.vgtk.cuda import grouping
    rng = np.random.default_rng(17)
    ref = (rng.uniform(-1.5, 1.5, (20_000, 3)) * [1, 1, 0.02]).astype(np.float32)
    sets = [rng.uniform(-1.5, 1.5, (1000, 3)).astype(np.float32) * np.float32([1, 1, 0.02]) for _ in range(3)]
    a, b = check(gpu, ref, sets[0], 0.03), check(gpu, ref, sets[0], 0.03)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    dref, dq = D(gpu, ref), D(gpu, sets[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                            # warm-up off the capture, as torch asks
        ws, _ = grouping.point_grid_build(dref, 0.03)
        grouping.point_grid_nn(ws, ref.shape[0], dq, 0.03, count=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ws, status = grouping.point_grid_build(dref, 0.03)
        idx, d2, hits = grouping.point_grid_nn(ws, ref.shape[0], dq, 0.03, count=True)
    for k in (1, 2, 0):
        dq.copy_(D(gpu, sets[k]))
        graph.replay()
        torch.cuda.synchronize()
        want_idx, want_d2 = G.nearest(ref, sets[k], 0.03)
        assert np.array_equal(idx.cpu().numpy(), want_idx)
        assert np.array_equal(d2.cpu().numpy().view(np.uint32), want_d2.view(np.uint32))
        assert hits.tolist() == [int((want_idx >= 0).sum())] and status.tolist() == [20_000, 0]


# ------------------------------------------------------------------------------------------------ the keypoint stage
def test_fragment_overlap(gpu):
    """1000 target points; the source is 400 of them moved by 0.05 (inside the margin 0.075 of their origin) and 600 points far
    away.  300 = 0.3 * 1000 source points must hit: 400 do.  With 299 near points the count is one short."""
    from epn_pointcloud_amd.vgtk import pc as pctk
    rng = np.random.default_rng(18)
    tgt = rng.uniform(-2, 2, (1000, 3)).astype(np.float32)
    away = (rng.uniform(-2, 2, (701, 3)) + [10, 0, 0]).astype(np.float32)
    for near, want in ((400, True), (300, True), (299, False)):
        src = np.vstack((tgt[:near] + np.float32([0.05, 0, 0]), away[:1000 - near])).astype(np.float32)
        hits, overlaps = pctk.fragment_overlap(D(gpu, src), D(gpu, tgt))
        assert hits.device.type == "cuda" and overlaps.dtype == torch.bool and overlaps.device.type == "cuda"
        assert int(hits) == near == int((G.nearest(tgt, src, 0.075)[0] >= 0).sum()) and bool(overlaps) is want
    grid = pctk.PointGrid(D(gpu, tgt), 0.1)                         # a prebuilt grid of the target, a larger max_radius
    hits, overlaps = pctk.fragment_overlap(D(gpu, src), grid)
    assert int(hits) == 299 and not bool(overlaps)
    hits, overlaps = pctk.fragment_overlap(D(gpu, src), grid, ratio=0.299)
    assert int(hits) == 299 and bool(overlaps)                      # 0.299 * 1000 = 299.0 (fp64) is reached


def _box_and_plane(rng, n):
    """About n points on the faces of a 1.2 x 0.8 x 0.6 box standing on a 3 x 3 floor, sampled at random."""
    k = n // 2
    floor = np.stack((rng.uniform(-1.5, 1.5, k), rng.uniform(-1.5, 1.5, k), np.zeros(k)), axis=1)
    u = rng.uniform(0, 1, (n - k, 3)) * [1.2, 0.8, 0.6]
    face = rng.integers(0, 5, n - k)                                # four walls and the top
    u[face == 0, 0] = 0
    u[face == 1, 0] = 1.2
    u[face == 2, 1] = 0
    u[face == 3, 1] = 0.8
    u[face == 4, 2] = 0.6
    return np.vstack((floor, u - [0.6, 0.4, 0])).astype(np.float32)


@pytest.fixture(scope="module")
def fragments():
    """(src, tgt, T_src, T_tgt, src_local, tgt_local, want): the source is the scene; the target is 70 % of it, jittered by up to
    5 mm; each is also given in a fragment frame of its own (a rotation about z and a shift), from which the poses take it back;
    want = the restatement's keypoint pairs, computed once."""
    rng = np.random.default_rng(19)
    src = _box_and_plane(rng, 20_000)
    rows = np.sort(rng.choice(src.shape[0], 14_000, replace=False))
    tgt = (src[rows] + rng.uniform(-0.005, 0.005, (rows.size, 3))).astype(np.float32)

    def pose(angle, shift):
        c, s = np.cos(angle), np.sin(angle)
        T = np.eye(4)
        T[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
        T[:3, 3] = shift
        return T
    Ts, Tt = pose(0.3, [0.5, -0.2, 0.1]), pose(-1.1, [-0.4, 0.3, 0.0])
    local = lambda p, T: ((p.astype(np.float64) - T[:3, 3]) @ T[:3, :3]).astype(np.float32)
    return src, tgt, Ts, Tt, local(src, Ts), local(tgt, Tt), G.keypoint_pairs(src, tgt)


def test_keypoint_pairs(gpu, fragments):
    from epn_pointcloud_amd import data
    from epn_pointcloud_amd.vgtk import pc as pctk
    src, tgt, Ts, Tt, src_local, tgt_local, (want_rows, want_cen, want_d2) = fragments
    got = pctk.keypoint_pairs(D(gpu, src), D(gpu, tgt))
    rows = got.rows.cpu().numpy()
    assert rows.dtype == np.int32 and rows.shape[0] > 200
    assert np.array_equal(rows, want_rows) and np.array_equal(got.src_centroid_row.cpu().numpy(), want_cen)
    assert np.array_equal(got.d2.cpu().numpy().view(np.uint32), want_d2.view(np.uint32))
    assert (np.diff(want_cen) > 0).all()
    dist = np.linalg.norm(src[rows[:, 0]].astype(np.float64) - tgt[rows[:, 1]].astype(np.float64), axis=1)
    assert (dist <= 0.03 + 2 * 0.05 * np.sqrt(3)).all()
    grids = [pctk.PointGrid(D(gpu, p), 0.1) for p in (src, tgt)]    # prebuilt raw grids give the same rows
    assert torch.equal(pctk.keypoint_pairs(*grids).rows, got.rows)
    with pytest.raises(ValueError, match="is needed"):
        pctk.keypoint_pairs(pctk.PointGrid(D(gpu, src), 0.05), grids[1])
    # the fragment-frame coordinates feed the training batch
    corr = np.stack((src_local[rows[:, 0]], tgt_local[rows[:, 1]]), axis=1)
    points, offsets = data.pack_clouds([src_local, tgt_local], gpu)
    corr_d, corr_off = data.pack_correspondences([corr], gpu)
    batch = data.fragment_pair_batch(points, offsets, D(gpu, [[0, 1]], np.int32), corr_d, corr_off, D(gpu, np.stack((Ts, Tt)), np.float64),
                                     64, 8, 0.3, seed=1)
    assert batch.status.tolist() == [0] and (batch.counts > 0).all()


def test_scene_keypoint_pairs(gpu, fragments):
    """Four fragments: 0 and 1 are the pair above, 2 is fragment 0 moved 10 m away, 3 is fragment 1 again.  stride 1 and window 3
    schedule (0,1) (0,2) (1,2) (1,3) (2,3); only (0,1) and (1,3) overlap."""
    from epn_pointcloud_amd.vgtk import pc as pctk
    src, tgt, Ts, Tt, src_local, tgt_local, want = fragments
    world = [D(gpu, p) for p in (src, tgt, src + np.float32([10, 0, 0]), tgt)]
    local = [D(gpu, p) for p in (src_local, tgt_local, src_local, tgt_local)]
    rows, corrs = pctk.scene_keypoint_pairs(world, local, stride=1, window=3)
    assert list(rows) == [(0, 1), (1, 3)] and len(corrs) == 2
    assert np.array_equal(rows[(0, 1)].cpu().numpy(), want[0])
    for (i, j), c in zip(rows, corrs):
        r = rows[(i, j)].to(torch.int64)
        assert c.shape == (r.shape[0], 2, 3) and c.dtype == torch.float32 and r.shape[0] > 200
        assert torch.equal(c[:, 0], local[i][r[:, 0]]) and torch.equal(c[:, 1], local[j][r[:, 1]])
    assert (rows[(1, 3)][:, 0] == rows[(1, 3)][:, 1]).all()         # a fragment against itself: every keypoint is its own match
    assert pctk.scene_keypoint_pairs(world, stride=1, window=3)[1] is None
    assert list(pctk.scene_keypoint_pairs(world)[0]) == [(0, 1)]    # the reference's stride 4, window 20: (0,1), (1,2), (2,3)


def test_transform_points(gpu, fragments):
    """R p + t in fp64, rounded once: within an fp32 ulp of 4 (2^-21) of the world cloud the fragment frame was made from (the
    fragment frame was itself rounded to fp32 once)."""
    from epn_pointcloud_amd.vgtk import pc as pctk
    src, _, Ts, _, src_local, _, _ = fragments
    got = pctk.transform_points(D(gpu, src_local), Ts)
    assert got.dtype == torch.float32 and got.shape == src.shape
    assert np.abs(got.cpu().numpy().astype(np.float64) - src).max() <= 2.0 ** -21
    with pytest.raises(ValueError):
        pctk.transform_points(D(gpu, src_local), np.eye(3))
