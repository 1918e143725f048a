"""The point grid without a GPU: the entry points exist at every layer, the argument checks run before any HIP runtime call, and
the restatement of the query (tests/grid_nn_ref.py: brute force in the specification's fp32 order) gives the hand-derived
answers and agrees with sklearn's NearestNeighbors on inputs where both are exact."""
import ctypes

import numpy as np
import pytest

import grid_nn_ref as G
import voxel_ref as V

EINVAL = -1


def test_symbols_resolve_and_are_bound_at_every_layer(vgtk_alias):
    from epn_pointcloud_amd import _lib, correspondence
    from epn_pointcloud_amd.vgtk.cuda import grouping
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("epn_point_grid_workspace_bytes", "epn_point_grid_build_f32", "epn_point_grid_nn_f32"):
        assert name in _lib.EXPORTS
        assert hasattr(cdll, name)
    assert callable(grouping.point_grid_build) and callable(grouping.point_grid_nn)
    import vgtk.pc
    for name in ("PointGrid", "fragment_overlap", "keypoint_pairs", "scene_keypoint_pairs", "transform_points"):
        assert getattr(vgtk.pc, name) is getattr(correspondence, name)


def test_wrappers_refuse_host_tensors(vgtk_alias):
    import torch
    import vgtk.pc
    from epn_pointcloud_amd.vgtk.cuda import grouping
    pc = torch.zeros((8, 3))
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        grouping.point_grid_build(pc, 0.1)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        grouping.point_grid_nn(torch.zeros(64, dtype=torch.int64), 8, pc, 0.1)
    with pytest.raises(ValueError, match="shape"):                  # data._tensor's order: type, shape, dtype, device
        grouping.point_grid_build(torch.zeros((8, 2)), 0.1)
    with pytest.raises(TypeError, match="float32"):
        grouping.point_grid_build(pc.double(), 0.1)
    for f in (vgtk.pc.PointGrid, vgtk.pc.fragment_overlap, vgtk.pc.keypoint_pairs):
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
            f(pc, pc) if f is not vgtk.pc.PointGrid else f(pc, 0.1)


def test_the_pair_schedule_is_the_reference_s(vgtk_alias):
    import vgtk.pc
    for n in (0, 1, 2, 5, 6, 21, 30):
        assert vgtk.pc.pair_schedule(n) == [(i, j) for i in range(n) for j in range(i + 1, min(i + 20, n), 4)]
    assert vgtk.pc.pair_schedule(6) == [(0, 1), (0, 5), (1, 2), (2, 3), (3, 4), (4, 5)]
    assert vgtk.pc.pair_schedule(4, stride=1, window=3) == [(0, 1), (0, 2), (1, 2), (1, 3), (2, 3)]


# ------------------------------------------------------------------------------------------------ ABI refusals
N_OK = 1000
_built = []


def _lib_():
    from epn_pointcloud_amd import _lib
    return _lib.get_lib()


def _ws_bytes(n):
    return int(_lib_().epn_point_grid_workspace_bytes(n))


def _vp(v):
    return ctypes.c_void_p(v) if v else None


def _build(**over):
    """Pointers: non-NULL, 16-byte aligned and never dereferenced (every call is refused, or n = 0)."""
    a = dict(ref=16, n=N_OK, valid=0, max_radius=0.1, workspace=4096, workspace_bytes=_ws_bytes(N_OK), status=16)
    a.update(over)
    return _lib_().epn_point_grid_build_f32(_vp(a["ref"]), a["n"], _vp(a["valid"]), a["max_radius"], _vp(a["workspace"]),
                                            a["workspace_bytes"], _vp(a["status"]), None)


EMPTY_GRID = 8192          # the address an empty grid (n = 0: nothing is launched, nothing dereferenced) is "built" at


def _nn(**over):
    if not _built:
        assert _build(n=0, workspace=EMPTY_GRID, workspace_bytes=_ws_bytes(0), max_radius=0.1) == 0
        _built.append(True)
    a = dict(workspace=EMPTY_GRID, n=0, qry=16, m=0, radius=0.1, exclude_row=0, nn_idx=16, nn_d2=16, hits=0)
    a.update(over)
    return _lib_().epn_point_grid_nn_f32(_vp(a["workspace"]), a["n"], _vp(a["qry"]), a["m"], a["radius"], a["exclude_row"],
                                         _vp(a["nn_idx"]), _vp(a["nn_d2"]), _vp(a["hits"]), None)


@pytest.mark.parametrize("bad", [dict(n=-1), dict(n=2 ** 22 + 1, workspace_bytes=2 ** 40), dict(max_radius=0.0),
                                 dict(max_radius=-0.1), dict(max_radius=float("nan")), dict(max_radius=float("inf")),
                                 dict(max_radius=2.0 ** -61), dict(ref=0), dict(status=0), dict(workspace=0), dict(workspace=4104),
                                 dict(workspace_bytes=0), dict(workspace_bytes=None)],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_bad_build_arguments_are_refused_before_any_runtime_call(bad):
    if "workspace_bytes" in bad and bad["workspace_bytes"] is None:
        bad = dict(workspace_bytes=_ws_bytes(N_OK) - 1)            # one byte short
    assert _build(**bad) == EINVAL


@pytest.mark.parametrize("bad", [dict(n=-1), dict(n=2 ** 22 + 1), dict(m=-1), dict(m=2 ** 22 + 1), dict(radius=0.0),
                                 dict(radius=-0.05), dict(radius=float("nan")), dict(radius=float("inf")),
                                 dict(radius=0.1000001), dict(radius=0.2), dict(exclude_row=1, m=5), dict(exclude_row=2),
                                 dict(workspace=0), dict(workspace=EMPTY_GRID + 8), dict(workspace=EMPTY_GRID + 4096),
                                 dict(n=1), dict(m=3, qry=0), dict(m=3, nn_idx=0), dict(m=3, nn_d2=0)],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_bad_query_arguments_are_refused_before_any_runtime_call(bad):
    """radius above the build's max_radius, exclude_row with m != n, NULL pointers, a workspace no build was called with (or
    built with another n): all decided on the host."""
    assert _nn(**bad) == EINVAL


def test_an_empty_grid_and_no_queries_launch_nothing():
    assert _nn() == 0                                               # m = 0, no hits asked for
    assert _nn(qry=0, nn_idx=0, nn_d2=0) == 0
    assert _nn(exclude_row=1) == 0                                  # m == n == 0
    assert _nn(radius=0.1) == 0 and _nn(radius=0.05) == 0           # up to and including max_radius
    assert _build(n=0, workspace=EMPTY_GRID, workspace_bytes=_ws_bytes(0) - 1) == EINVAL
    assert _build(n=0, ref=0, status=0, workspace=EMPTY_GRID, workspace_bytes=_ws_bytes(0)) == 0


def test_workspace_holds_records_table_and_scan_at_every_size():
    assert _ws_bytes(-3) == 0 and _ws_bytes(2 ** 22 + 1) == 0
    prev = 0
    for n in (0, 1, 63, 64, 65, 1000, 65536, 65537, 2 ** 22):
        b = _ws_bytes(n)
        assert b >= 64 + 16 * n + 16 * V.capacity(n) + 4 * n and b > prev   # a record and a slot index per point, a slot per key
        prev = b


# ------------------------------------------------------------------------------------------------ the restatement by hand
def test_restatement_on_hand_derived_cases():
    ref = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [1, 0, 0], [np.nan, 0, 0], [0, 0, -0.5]], np.float32)
    qry = np.array([[0.25, 0, 0], [1, 0, 0], [0.5, 0, 0], [0, 1, 0], [9, 9, 9], [0, np.inf, 0], [0, 0, -0.25]], np.float32)
    idx, d2 = G.nearest(ref, qry, 1.0)
    assert idx.tolist() == [0, 1, 0, 0, -1, -1, 0]                  # [1]: rows 1 and 3 coincide; [2], [3], [6]: ties, lowest row
    assert d2.tolist() == [0.0625, 0.0, 0.25, 1.0, np.inf, np.inf, 0.0625]
    idx, d2 = G.nearest(ref, qry, 0.25)
    assert idx.tolist() == [0, 1, -1, -1, -1, -1, 0] and d2[2] == np.inf     # d2 == r2 is inside: 0.0625 <= 0.0625
    idx, _ = G.nearest(ref, qry, 1.0, valid=[0, 0, 1, 1, 1, 1])
    assert idx.tolist() == [5, 3, 3, 2, -1, -1, 5]                  # the NaN row never answers, masked rows neither
    idx, d2 = G.nearest(ref, ref, 1.0, exclude_self=True)
    assert idx.tolist() == [5, 3, -1, 1, -1, 0] and d2.tolist() == [0.25, 0.0, np.inf, 0.0, np.inf, 0.25]
    assert G.nearest(np.zeros((0, 3)), qry, 1.0)[0].tolist() == [-1] * 7
    assert G.nearest(ref, np.zeros((0, 3)), 1.0)[0].shape == (0,)


def test_the_distance_is_rounded_operation_by_operation():
    """dx = 1 + 2^-12: dx*dx = 1 + 2^-11 + 2^-24 rounds to 1 + 2^-11 in fp32 (a tie, to even), and with r2 = 1 + 2^-11 that
    point is inside, though its exact distance is above the radius."""
    ref = np.array([[1 + 2.0 ** -12, 0, 0]], np.float32)
    r = np.sqrt(np.float64(1 + 2.0 ** -11))
    assert np.float32(r * r) == np.float32(1 + 2.0 ** -11)
    idx, d2 = G.nearest(ref, np.zeros((1, 3), np.float32), r)
    assert idx.tolist() == [0] and d2[0] == np.float32(1 + 2.0 ** -11)
    assert (1 + 2.0 ** -12) ** 2 > r * r


def test_cells_are_the_voxel_rule_at_the_cell_edge():
    edge = G.cell_edge(0.25)
    assert edge == 0.25 * (1 + 2.0 ** -10)
    ref = np.array([[0, 0, 0], [edge / 2 * 0.999, 0, 0], [edge / 2 * 1.001, 0, 0], [0, 5 * edge, 2 * edge], [np.inf, 0, 0]])
    part, idx, flags = G.cell_indices(ref, 0.25)
    assert part.tolist() == [True, True, True, True, False] and flags == 0
    assert idx.tolist() == [[0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 5, 2]]   # the minimum sits half a cell inside cell 0
    assert G.cell_indices(np.array([[0, 0, 300.0]]), 0.25)[2] == V.FLAG_COORD
    assert G.cell_indices(np.array([[0, 0, 0], [200.0, 0, 0]]), 1e-5)[2] == V.FLAG_INDEX
    assert G.cell_indices(np.array([[0, 0, 300.0], [0, 0, 0]]), 0.25, valid=[0, 1])[2] == 0


def test_keypoint_pairs_restatement_on_a_hand_case():
    """voxel 1, isolation 1.5, match 0.3.  Source centroids (0.5, 0.5, 0.5) [two raw points], (1.5, 0.5, 0.5) and the isolated
    (9.5, 0.5, 0.5); the target is the source moved by 0.1 in y without the isolated point's neighbourhood."""
    src = np.array([[0.4, 0.5, 0.5], [0.6, 0.5, 0.5], [1.5, 0.5, 0.5], [9.5, 0.5, 0.5]], np.float32)
    tgt = (src[[2, 0, 1]] + np.float32([0, 0.1, 0])).astype(np.float32)
    rows, cen_row, d2 = G.keypoint_pairs(src, tgt, voxel_size=1.0, isolation_radius=1.5, match_radius=0.3)
    assert cen_row.tolist() == [0, 1]
    assert rows.tolist() == [[0, 1], [2, 0]]                        # nearest raw rows; (0.4, ..) and (0.6, ..) tie: the lower row
    assert np.allclose(d2, 0.01, rtol=1e-5)


# ------------------------------------------------------------------------------------------------ sklearn
def test_restatement_against_sklearn_on_lattice_clouds():
    """Coordinates on multiples of 2^-8 in [-2, 2]: d2 is exact in fp32 and fp64 alike, so the squared distances must be equal
    and the rows must agree wherever the minimum is unique; tied queries (left out of the row comparison) may be at most 1 %."""
    neighbors = pytest.importorskip("sklearn.neighbors")
    ref, qry = G.lattice_clouds()
    assert ref.shape == (5000, 3) and qry.shape == (3000, 3)
    idx, d2 = G.nearest(ref, qry, 8.0)                              # every query finds one: the cube's diagonal is below 8
    assert (idx >= 0).all()
    nn = neighbors.NearestNeighbors(n_neighbors=1, algorithm="kd_tree").fit(ref.astype(np.float64))
    dist, rows = nn.kneighbors(qry.astype(np.float64))
    e = ((ref.astype(np.float64)[rows[:, 0]] - qry.astype(np.float64)) ** 2).sum(axis=1)   # exact: sklearn returns the root
    assert np.array_equal(d2.astype(np.float64), e)
    assert np.array_equal(dist[:, 0], np.sqrt(e))                   # the tree returns the root of the same exact sum
    all_d2 = ((ref.astype(np.float64)[None] - qry.astype(np.float64)[:, None]) ** 2).sum(axis=2)
    assert np.array_equal(all_d2.min(axis=1), e)
    tied = (all_d2 == e[:, None]).sum(axis=1) > 1
    print(f"tied queries: {tied.mean():.4%}; within 0.25: {(e <= 0.0625).mean():.2%}")
    assert tied.mean() <= 0.01
    assert np.array_equal(idx[~tied], rows[~tied, 0])
    for radius in (0.25, 0.0625):                                   # the bounded query cuts the same answers off at r2
        bi, bd = G.nearest(ref, qry, radius)
        inside = e <= radius * radius
        assert np.array_equal(bi >= 0, inside) and np.array_equal(bi[inside], idx[inside])
        assert np.array_equal(bd[inside], d2[inside]) and np.isinf(bd[~inside]).all()
