"""Surface normals and patch frames on the GPU (csrc/point_normals.hip behind vgtk.pc.PointGrid.normals / estimate_normals /
orient_patches) against the numpy restatement of their specification (tests/normals_ref.py: brute-force neighbourhoods, integer
moments, numpy's eigh).  count, flags, the neighbour rows and the moments are compared exactly; the frames and rotated patches
bit for bit; the normals and eigenvalues within the one tolerance

    |n - n_ref| <= 2^-23 + c 2^-52 lam2 / (lam1 - lam0)          |eig - eig_ref| <= 2^-23 |eig_ref| + c 2^-52 max|lam| radius^2

with c = normals_ref.C_JACOBI = 82, 8 x the worst ratio the host build of csrc/plane_fit.h showed against eigh
(tests/test_plane_fit_host.py).  Queries whose direction is not determined (flag bit 2) are compared on the
eigenvalues only.  Nothing here has been compared with open3d."""
import itertools

import numpy as np
import pytest
import torch

import grid_nn_ref as G
import normals_ref as N

pytestmark = pytest.mark.gpu

R = 0.5                                    # the radius of the lattice cases; the lattice's spacing is 0.25
E = float(G.cell_edge(R))


def D(gpu, a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(gpu)


def grid_of(gpu, ref, max_radius):
    from epn_pointcloud_amd.vgtk import pc as pctk
    return pctk.PointGrid(D(gpu, np.asarray(ref, np.float32).reshape(-1, 3)), max_radius)


def check(gpu, ref, qry, radius, max_nn=30, view=None, max_radius=None, grid=None, gap_share=1.0):
    """Every output of one call against the restatement; qry None = the grid's own points.  Returns the device's PointNormals
    as numpy arrays and the restatement."""
    ref = np.asarray(ref, np.float32).reshape(-1, 3)
    q = ref if qry is None else np.asarray(qry, np.float32).reshape(-1, 3)
    grid = grid or grid_of(gpu, ref, max_radius or radius)
    got = grid.normals(None if qry is None else D(gpu, q), radius, max_nn=max_nn, view=view, return_moments=True,
                       return_neighbors=max_nn > 0)
    want = N.point_normals(ref, q, radius, max_nn=max_nn, view=view)
    normals, eig, count, flags, moments = (t.cpu().numpy() for t in got[:5])
    assert normals.dtype == np.float32 and eig.dtype == np.float32 and moments.dtype == np.int64
    assert normals.shape == (q.shape[0], 3) and eig.shape == (q.shape[0], 3) and moments.shape == (q.shape[0], 9)
    assert np.array_equal(count, want["count"])
    assert np.array_equal(moments, want["moments"])
    if max_nn > 0:
        assert np.array_equal(got.neighbors.cpu().numpy(), N.neighbor_table(want["neighbors"], max_nn))
    else:
        assert got.neighbors is None
    gap = want["lam"][:, 1] - want["lam"][:, 0]
    edge = (want["flags"] & N.FLAG_FEW == 0) & (np.abs(gap - N.GAP_MIN) <= 2.0 ** -50 * N.C_JACOBI * np.abs(want["lam"]).max(axis=1))
    assert np.array_equal(flags[~edge], want["flags"][~edge])       # bit 2 may differ only where the gap is within the bound of 2^-40
    err_e = np.abs(eig.astype(np.float64) - want["eig"])
    print(f"max eig error / bound: {(err_e / np.maximum(N.eig_bound(want['lam'], radius), 1e-300)).max() if q.shape[0] else 0:.3f}")
    assert (err_e <= N.eig_bound(want["lam"], radius)).all()
    sure = (flags & N.FLAG_GAP == 0) & (want["flags"] & N.FLAG_GAP == 0)
    assert (~sure).mean() <= gap_share if q.shape[0] else True
    bound = N.normal_bound(want["lam"][sure] if sure.any() else np.ones((0, 3)))
    few = want["flags"][sure] & N.FLAG_FEW != 0
    bound[few] = 0.0                                                # the fallback (0, 0, 1) is exact
    # The sign rule decides on a comparison -- of the two largest magnitudes, or of n . (view - q) with zero.  Where the two sides
    # of that comparison are closer than the bound on n allows to tell (lattice clouds: normals like (1, -1, 0) / sqrt 2), either
    # sign is the rule's answer for some admissible n, and the row is compared up to the sign.
    ref_n, dev_n = want["normals"][sure], normals.astype(np.float64)[sure]
    if view is None:
        mags = np.sort(np.abs(ref_n), axis=1)
        tie = mags[:, 2] - mags[:, 1] <= 2 * bound
    else:
        to_view = np.asarray(view, np.float32).astype(np.float64)[None] - q.astype(np.float64)[sure]
        tie = np.abs((ref_n * to_view).sum(axis=1)) <= 3 * bound * np.abs(to_view).max(axis=1)
    tie &= ~few
    err_n = np.abs(dev_n - ref_n)
    err_n[tie] = np.minimum(err_n[tie].max(axis=1), np.abs(dev_n[tie] + ref_n[tie]).max(axis=1))[:, None]
    print(f"max normal error / bound: {(err_n.max(axis=1) / np.maximum(bound, 1e-300))[~few].max() if (~few).any() else 0:.3f}")
    assert (err_n <= bound[:, None]).all()
    assert np.abs(np.linalg.norm(normals.astype(np.float64), axis=1) - 1).max() <= 2.0 ** -22 if q.shape[0] else True
    return (normals, eig, count, flags, moments), want


# ------------------------------------------------------------------------------------------------ degenerate sizes
@pytest.mark.parametrize("ref", [np.zeros((0, 3)), [[0.25, -0.25, 0.0]], [[0, 0, 0], [0.25, 0, 0]],
                                 [[0, 0, 0], [0.125, 0.125, 0], [0.25, 0.25, 0]], [[0, 0, 0], [0.25, 0, 0], [0, 0.25, 0.125]]],
                         ids=["empty", "one", "two", "collinear", "triangle"])
def test_degenerate_sizes(gpu, ref):
    ref = np.asarray(ref, np.float32).reshape(-1, 3)
    qry = np.array([[0, 0, 0], [0.1, 0.1, 0.1], [5, 5, 5]], np.float32)
    grid = grid_of(gpu, ref, R)
    (normals, eig, count, flags, _), _ = check(gpu, ref, qry, R, grid=grid)
    n = ref.shape[0]
    assert flags[2] == N.FLAG_FEW and count[2] == 0
    if n < 3:
        assert (flags == N.FLAG_FEW).all() and (normals == [0, 0, 1]).all() and (eig == 0).all() and count[:2].max() == n
    elif n == 3 and ref[2, 2] == 0:
        assert flags[0] == N.FLAG_GAP                               # a line: the direction is not determined
    else:
        assert flags[0] == 0
    check(gpu, ref, np.zeros((0, 3)), R, grid=grid)                 # m = 0
    if n:
        check(gpu, ref, None, R, grid=grid)


# ------------------------------------------------------------------------------------------------ distance boundaries and ties
def lattice():
    """5 x 5 x 5 points at spacing 0.25, rows shuffled, with three more copies of one point at rows of their own"""
    pts = np.array(list(itertools.product(range(-2, 3), repeat=3)), np.float64) / 4.0
    pts = pts[np.random.default_rng(3).permutation(125)]
    return np.vstack((pts[:40], [[0.25, 0, 0]], pts[40:], [[0.25, 0, 0]] * 2)).astype(np.float32)


def test_lattice_ties_and_every_max_nn(gpu):
    """radius 0.5 on spacing 0.25: the six points two steps along an axis sit at d2 == r2 exactly (inside), and the shells hold 6,
    12, 8 and 6 points at equal d2 in different cells (the cell edge is just above 0.5), so every cut below the whole set falls
    inside a tie and is decided by the row."""
    ref = lattice()
    grid = grid_of(gpu, ref, R)
    centre = np.zeros((1, 3), np.float32)
    count, rows = N.neighbourhood(ref, centre[0], R, 0)
    assert count == 33 + 3                                          # 1 + 6 + 12 + 8 + 6 lattice points and the three copies
    d = ref[rows].astype(np.float64)
    assert ((d * d).sum(axis=1) == 0.25).sum() == 6
    assert len({tuple(c) for c in G.cell_indices(ref[rows], R)[1].tolist()}) > 8
    for max_nn in (1, count - 1, count, count + 1, 0, 7, 20):
        (_, _, got_count, _, _), _ = check(gpu, ref, centre, R, max_nn=max_nn, grid=grid)
        assert got_count.tolist() == [count]
    check(gpu, ref, None, R, max_nn=10, grid=grid)                  # every point of the lattice, a cut inside a tie each
    check(gpu, ref, None, R, max_nn=0, grid=grid)
    check(gpu, ref, ref[:30] + np.float32(0.0625), 0.375, max_nn=5, grid=grid)       # a smaller radius on the same grid


# ------------------------------------------------------------------------------------------------ cell geometry
def test_all_27_cells_a_cell_face_outside_and_non_finite_queries(gpu):
    """The origin fixes the grid; q sits at the centre of cell (5, 5, 5) with one point in each of the 27 cells around it, half a
    cell and 0.0075 along every moved axis (at most sqrt(3) * 0.2578 = 0.4465 away).  The face query lies 1e-4 above the face between cells 4 and 5 on x."""
    q = np.full(3, 5 * E)
    around = np.array([q + np.array(d) * (E / 2 + 0.0075) for d in itertools.product((-1, 0, 1), repeat=3)])
    ref = np.vstack(([[0, 0, 0]], around, q + [[0.05, 0.02, -0.03], [-0.04, 0.03, 0.01]])).astype(np.float32)
    cells = G.cell_indices(ref, R)[1][1:28]
    assert {tuple(c) for c in cells.tolist()} == set(itertools.product((4, 5, 6), repeat=3))
    face = np.array([4.5 * E + 1e-4, 5 * E, 5 * E])
    assert G.cell_indices(np.vstack(([[0, 0, 0]], [face])), R)[1][1].tolist() == [5, 5, 5]
    qry = np.vstack((q, face, [30, 30, 30], [-7, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e30, 0, 0])).astype(np.float32)
    (normals, eig, count, flags, moments), want = check(gpu, ref, qry, R, max_nn=0)
    assert count[0] == 29 and count[1] >= 10
    assert count[2:].tolist() == [0] * 6
    assert flags[2:].tolist() == [1, 1, 3, 3, 3, 1]
    assert (normals[2:] == [0, 0, 1]).all() and (eig[2:] == 0).all() and (moments[2:] == 0).all()
    check(gpu, ref, qry, R, max_nn=12)


# ------------------------------------------------------------------------------------------------ stride loops
def test_cells_of_65_300_and_1100_records(gpu):
    """Flat clusters inside one cell each, three cells apart: a wave's passes of 64 candidates end just past a run and in the
    middle of one; the third holds more members than max_nn admits at its largest, with and without a cut."""
    rng = np.random.default_rng(4)
    sizes = (65, 300, 1100)
    centres = np.array([[3 * (k + 1) * E, 0, 0] for k in range(3)])
    ref = np.vstack([[[0, 0, 0]]] + [c + rng.uniform(-0.1, 0.1, (s, 3)) * [1, 1, 0.05] for c, s in zip(centres, sizes)]).astype(np.float32)
    counts = np.unique(G.cell_indices(ref, R)[1], axis=0, return_counts=True)[1]
    assert sorted(counts.tolist()) == [1, 65, 300, 1100]
    qry = np.vstack([c + rng.uniform(-0.05, 0.05, (3, 3)) for c in centres]).astype(np.float32)
    grid = grid_of(gpu, ref[rng.permutation(ref.shape[0])], R)
    ref = grid.points.cpu().numpy()
    (_, _, count, _, _), _ = check(gpu, ref, qry, R, max_nn=0, grid=grid)
    assert count.tolist() == [65] * 3 + [300] * 3 + [1100] * 3      # count > 1024, no limit
    for max_nn in (30, 64, 65, 1024):
        check(gpu, ref, qry, R, max_nn=max_nn, grid=grid)
    check(gpu, ref, qry, 0.06, max_nn=30, grid=grid)


# ------------------------------------------------------------------------------------------------ order-freedom
def test_reversed_rows_give_the_same_moments_and_two_calls_the_same_bits(gpu):
    rng = np.random.default_rng(6)
    ref = (rng.uniform(-1, 1, (1500, 3)) * [1, 1, 0.1]).astype(np.float32)
    (n1, e1, c1, f1, m1), _ = check(gpu, ref, None, 0.3, max_nn=0)
    (n2, e2, c2, f2, m2), _ = check(gpu, ref[::-1], None, 0.3, max_nn=0)
    assert np.array_equal(m1, m2[::-1]) and np.array_equal(c1, c2[::-1]) and np.array_equal(f1, f2[::-1])
    assert np.array_equal(n1.view(np.uint32), n2[::-1].view(np.uint32)) and np.array_equal(e1.view(np.uint32), e2[::-1].view(np.uint32))
    grid = grid_of(gpu, ref, 0.3)
    a = grid.normals(None, 0.3, max_nn=30, return_moments=True, return_neighbors=True)
    b = grid.normals(None, 0.3, max_nn=30, return_moments=True, return_neighbors=True)
    assert all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ the noisy sphere
@pytest.fixture(scope="module")
def sphere():
    return N.noisy_sphere()


@pytest.mark.parametrize("view", [None, [0.0, 0.0, 0.0], [0.3, -0.2, 0.1], [4.0, 1.0, -2.0]],
                         ids=["largest_component", "centre", "inside", "outside"])
def test_noisy_sphere(gpu, sphere, view):
    from epn_pointcloud_amd.vgtk import pc as pctk
    grid = grid_of(gpu, sphere, 0.25)
    (normals, eig, count, flags, _), want = check(gpu, sphere, None, 0.2, max_nn=30, view=view, grid=grid, gap_share=0.02)
    assert (flags & N.FLAG_FEW == 0).all() and count.min() >= 5
    outward = sphere / np.linalg.norm(sphere, axis=1, keepdims=True)
    dots = (normals * outward).sum(axis=1)
    assert (np.abs(dots) > 0.9).all()
    if view is None:
        top = np.abs(normals).argmax(axis=1)
        assert (normals[np.arange(2000), top] > 0).all()
    else:
        to_view = np.float32(view)[None] - sphere
        assert ((normals.astype(np.float64) * to_view).sum(axis=1) >= -1e-6).all()
        if view == [0.0, 0.0, 0.0]:
            assert (dots < 0).all()                                 # every normal looks at the centre
        if view == [4.0, 1.0, -2.0]:
            assert (dots > 0).any() and (dots < 0).any()            # the near side looks out, the far side in
    # separate queries at the same coordinates, and the one-call form, give the same bits
    sep = grid.normals(D(gpu, sphere), 0.2, max_nn=30, view=view)
    one = pctk.estimate_normals(grid, 0.2, max_nn=30, view=view)
    for t in (sep, one):
        assert np.array_equal(t.normals.cpu().numpy().view(np.uint32), normals.view(np.uint32))
        assert np.array_equal(t.eig.cpu().numpy().view(np.uint32), eig.view(np.uint32))
        assert np.array_equal(t.count.cpu().numpy(), count) and np.array_equal(t.flags.cpu().numpy(), flags)
        assert t.moments is None and t.neighbors is None
    with pytest.raises(ValueError, match="max_radius"):
        grid.normals(None, 0.26)
    with pytest.raises(ValueError, match="return_neighbors"):
        grid.normals(None, 0.2, max_nn=0, return_neighbors=True)
    with pytest.raises(ValueError, match="shape"):
        grid.normals(None, 0.2, view=torch.zeros(4, device=gpu))


# ------------------------------------------------------------------------------------------------ patch frames
@pytest.mark.parametrize("k, n_sample", [(0, 7), (1, 1), (1, 1024), (3, 7), (3, 1024)])
def test_orient_patches(gpu, k, n_sample):
    from epn_pointcloud_amd.vgtk import pc as pctk
    from epn_pointcloud_amd.vgtk.cuda import grouping
    rng = np.random.default_rng(k * 10000 + n_sample)
    patches = rng.uniform(-1, 1, (k, n_sample, 3)).astype(np.float32)
    normals = rng.standard_normal((k, 3)).astype(np.float32)
    if k == 3:
        normals[1] = [0, -2.5, 0]                                   # parallel to up: the frame's x and y collapse
        patches[2, n_sample // 2] = 0                               # a zero row
        patches[0] = 0                                              # a zero patch, as radius_patches leaves for an empty ball
    want_out, want_axis = N.orient_patches(patches, normals)
    out, axis = grouping.orient_patches(D(gpu, patches), D(gpu, normals))
    assert out.shape == (k, n_sample, 3) and axis.shape == (k, 3, 3)
    assert np.array_equal(axis.cpu().numpy().view(np.uint32), want_axis.view(np.uint32))
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want_out.view(np.uint32))
    assert torch.isfinite(out).all() and torch.isfinite(axis).all()
    if k == 3:
        assert (axis[1, :, :2] == 0).all() and (out[0] == 0).all() and (out[2, n_sample // 2] == 0).all()
    assert torch.equal(pctk.orient_patches(D(gpu, patches), D(gpu, normals)), out)
    inplace = D(gpu, patches)
    back, _ = grouping.orient_patches(inplace, D(gpu, normals), out=inplace)
    assert back.data_ptr() == inplace.data_ptr() and torch.equal(inplace, out)
    if k:
        with pytest.raises(ValueError, match="shape"):
            pctk.orient_patches(D(gpu, patches), D(gpu, np.zeros((k + 1, 3))))


# ------------------------------------------------------------------------------------------------ end to end
def test_radius_patches_and_describe_take_normals(gpu):
    """A plane tilted about x, 3000 points: its normals from estimate_normals; radius_patches(normals=...) is orient_patches of
    radius_patches(), the oriented patches lie flat in their frame's z, and describe(normals=...) runs on a small model and
    differs from describe()."""
    from epn_pointcloud_amd import models as M
    from epn_pointcloud_amd.vgtk import pc as pctk
    from test_models_cpu import fill_state_dict
    rng = np.random.default_rng(9)
    uv = rng.uniform(-1, 1, (3000, 2))
    c, s = np.cos(0.6), np.sin(0.6)
    cloud = np.column_stack((uv[:, 0], c * uv[:, 1], s * uv[:, 1])).astype(np.float32)
    pc = D(gpu, cloud)
    fit = pctk.estimate_normals(pc, 0.2, view=[0.0, -5.0, 5.0])
    assert (fit.flags == 0).all()
    assert (fit.normals - torch.tensor([0.0, -s, c], device=gpu)).abs().max().item() < 1e-4
    rows = torch.tensor([5, 700, 1234, 2999], device=gpu)
    plain, idx, counts = pctk.radius_patches(pc, rows, 0.4, 64, seed=2, center=True)
    turned, idx2, counts2 = pctk.radius_patches(pc, rows, 0.4, 64, seed=2, center=True, normals=fit.normals[rows])
    assert torch.equal(idx, idx2) and torch.equal(counts, counts2) and counts.min().item() > 64
    assert torch.equal(turned, pctk.orient_patches(plain, fit.normals[rows]))
    assert turned[:, :, 2].abs().max().item() < 1e-4 < plain[:, :, 2].abs().max().item()
    m = fill_state_dict(M.build_inv(input_num=1024, search_radius=0.8, width_div=8)).to(gpu).eval()
    base, valid = m.describe(pc, rows, batch=4, seed=3)
    with_rows, valid2 = m.describe(pc, rows, batch=4, seed=3, normals=fit.normals)          # [n,3], gathered at the rows
    with_kpts, _ = m.describe(pc, pc[rows], batch=4, seed=3, normals=fit.normals[rows])      # [k,3], as given
    assert valid.all() and torch.equal(valid, valid2) and torch.isfinite(with_rows).all()
    assert torch.equal(with_rows, with_kpts)
    assert (with_rows.norm(dim=1) - 1).abs().max().item() < 1e-4
    assert (with_rows - base).abs().max().item() > 1e-3
