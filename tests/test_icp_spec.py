"""The ICP stage's specification without a device (include/epn_so3conv.h: epn_icp_refine_f32): answers derived by
hand and met by the restatement tests/icp_ref.py, every refusal of the entry through the built library (a refusal is decided
before any HIP runtime call, so it needs no GPU), the Cayley increment, and the header's overflow bound re-derived in Python
ints."""
import ctypes

import numpy as np
import pytest

import icp_ref as I

EINVAL, EWORKSPACE, ENULL = -1, -2, -3


# ------------------------------------------------------------------------------------------------ answers derived by hand
def _lattice(k=5, spacing=0.25):
    ax = (np.arange(k) - (k - 1) / 2) * spacing
    return np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)


def test_a_shifted_lattice_is_recovered_in_one_iteration_and_the_loop_stops():
    """Coordinates and the shift are multiples of 2^-5, the shift is below half the spacing: every correspondence is the true
    mate, every term is exact in the fixed point, C = sum (p - pbar)(p - pbar)^T is diagonal, so R = I and t = the shift up to
    the rounding of the fp64 step: 3 * 125 products of magnitude <= 1/4 subtracted in C (below 1e-13 absolute on C of size >=
    15), and three subtractions for t.  Bound: 1e-12.  Iteration 1 then sees rmse = 0 against |shift| and updates by the
    identity; iteration 2 sees no change and stops: two updates, as open3d counts them."""
    tgt = _lattice()
    shift = np.array([2.0 ** -4, -(2.0 ** -5), 3 * 2.0 ** -5])
    src = (tgt.astype(np.float64) - shift).astype(np.float32)
    assert np.array_equal(src.astype(np.float64) + shift, tgt.astype(np.float64))
    ref = I.run(tgt, src, np.eye(4), 0.2, 5)
    assert np.array_equal(ref["steps"][0]["nn_idx"], np.arange(len(tgt)))
    T1 = ref["trace"][0, :16].reshape(4, 4)
    want = np.eye(4)
    want[:3, 3] = shift
    assert np.abs(T1 - want).max() <= 1e-12
    assert ref["trace"][0, 16] == 125 and abs(ref["trace"][0, 18] - np.linalg.norm(shift)) <= 1e-15
    assert ref["trace"][1, 19] == 0 and ref["trace"][1, 18] <= 1e-12                # the second update: from rmse = 0
    assert np.abs(ref["trace"][1, :16].reshape(4, 4) - want).max() <= 1e-12
    assert ref["trace"][2, 19] == I.CONVERGED and ref["iterations"] == 2 and ref["status"] == I.CONVERGED
    assert np.array_equal(ref["trace"][3], ref["trace"][2]) and np.array_equal(ref["trace"][4], ref["trace"][2])
    assert np.array_equal(ref["T"], ref["trace"][1, :16].reshape(4, 4))


def test_a_rotation_about_the_centroid_is_recovered_in_one_iteration():
    """0.05 rad about z through the lattice's centroid (the origin) moves a point by at most 0.05 * 0.5 sqrt(2) < half the
    spacing: true mates.  Horn's fit of exact mates is exact; what is left is the fp32 rounding of the rotated source (2^-25
    relative per coordinate) and the 2^-24 quantum of the nine product sums: |dC|_F <= 3 N (2^-25 + 2 * 2^-25 c^2) with c = the
    largest coordinate, and the projection moves by at most 2 |dC| / (s1 margin)."""
    tgt = _lattice()
    truth = I.rigid([0.0, 0.0, 0.05], [0.0, 0.0, 0.0])
    src = (tgt.astype(np.float64) @ truth[:3, :3]).astype(np.float32)               # R^T p: T takes it back
    ref = I.run(tgt, src, np.eye(4), 0.2, 1)
    assert np.array_equal(ref["steps"][0]["nn_idx"], np.arange(len(tgt)))
    N, c = len(tgt), float(np.abs(tgt).max())
    P = tgt.astype(np.float64)
    s = np.linalg.svd(P.T @ P, compute_uv=False)
    margin = (s[1] + s[2]) / s[0]
    bound = 2.0 * 3.0 * N * (2.0 ** -25 + 2.0 * 2.0 ** -25 * c * c) / (s[0] * margin)
    assert bound < 1e-5
    assert np.abs(ref["T"][:3, :3] - truth[:3, :3]).max() <= bound
    assert np.abs(ref["T"][:3, 3]).max() <= 3.0 * bound * c + 2.0 ** -25 * 3 * c


def test_point_to_plane_converges_on_a_corner_where_point_to_point_slides():
    """Three noise-free orthogonal planes, the source another sampling of them: point-to-point pairs every source point with
    a DIFFERENT point of the plane and is held off the truth by the sampling (it slides along the planes), while every
    point-to-plane residual vanishes at the truth, where the three normals span the space.  What is left for point-to-plane is
    the fp32 rounding of the moved source, 2^-24 relative on coordinates below 1.2, through a system whose conditioning the
    builder holds above 2^-12 per pivot: below 1e-5."""
    rng = np.random.default_rng(5)
    tgt, nrm = I.corner_scene(rng, 300)
    fresh, _ = I.corner_scene(rng, 300)
    truth = I.rigid([0.01, -0.015, 0.02], [0.012, -0.008, 0.01])
    inv = np.linalg.inv(truth)
    src = (fresh.astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    plane = I.run(tgt, src, np.eye(4), 0.1, 30, normals=nrm)
    point = I.run(tgt, src, np.eye(4), 0.1, 30)
    err = lambda T: np.abs(T - truth).max()
    assert plane["status"] == I.CONVERGED and err(plane["T"]) <= 1e-5
    assert err(point["T"]) >= 1e-4 and err(point["T"]) >= 10.0 * err(plane["T"])
    assert err(plane["T"]) < err(np.eye(4))


def test_cayley_increment_is_a_rotation():
    rng = np.random.default_rng(0)
    for _ in range(2000):
        w = rng.standard_normal(3)
        w *= rng.uniform(0, 1) / np.linalg.norm(w)
        R = I.cayley(list(w))
        assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-15 and np.linalg.det(R) > 0
        # the rotation about w / |w| by 2 atan(|w| / 2): second-order agreement with the rotation vector w
        assert np.abs(R - I.rigid(w * (2.0 * np.arctan(0.5 * np.linalg.norm(w)) / max(np.linalg.norm(w), 1e-300)), [0, 0, 0])[:3, :3]
                      ).max() <= 1e-15
    assert np.array_equal(I.cayley([0.0, 0.0, 0.0]), np.eye(3))


def test_overflow_bound_of_the_header_in_integers():
    """|p_i|, |q_i| <= 2^6, |n_i| <= 1: the largest value of every kind of term, scaled and rounded, times the library's limit
    on m, stays inside int64.  The header pads the largest product, 9 * 2^14, to 2^18 and takes the limit from that: 2^20.  By
    the unpadded figure 2^21 points would still fit and 2^22 would not; the one bit of slack is stated in the header."""
    from epn_pointcloud_amd import _lib
    lib = _lib.get_lib()
    max_m = 2 ** 20
    assert lib.epn_icp_workspace_bytes(max_m) > 0 and lib.epn_icp_workspace_bytes(max_m + 1) == 0      # the library's own limit
    assert I.MAX_M == max_m
    c = 64
    cross, d = 2 * c, 2 * c
    r = 3 * d
    products = dict(pq=c * c, dd=3 * d * d, JJ=cross * cross, Jr=cross * r, rr=r * r)
    assert max(products.values()) == r * r == 9 * 2 ** 14 < 2 ** 18
    padded, true = 2 ** 18 * 2 ** 24 + 1, 9 * 2 ** 14 * 2 ** 24 + 1
    assert max_m * padded < 2 ** 63 <= 2 * max_m * padded                      # the padded bound allows 2^20 and not 2^21
    assert 2 * max_m * true < 2 ** 63 <= 4 * max_m * true                      # the slack: one doubling
    assert max_m * c * 2 ** 32 < 2 ** 63
    # the restatement's tables address 17 and 30 distinct sums of the 32
    assert sorted(e for e, *_ in I.term_table(False)) == list(range(17))
    assert sorted(e for e, *_ in I.term_table(True)) == list(range(30))


def test_out_of_range_pairs_are_counted_not_dropped():
    tgt = np.array([[63.9, 0, 0], [0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=np.float32)
    inside, outside = np.float32(64.0), np.nextafter(np.float32(64.0), np.float32(np.inf))
    for x, flagged in ((inside, False), (outside, True)):
        src = np.array([[x, 0, 0], [0, 0, 0.01], [1, 0, 0.01], [0, 1, 0.01]], dtype=np.float32)
        ref = I.run(tgt, src, np.eye(4), 0.5, 1)
        assert (ref["sums"][30] == 1) == flagged and (ref["status"] == I.RANGE) == flagged
        assert ref["sums"][0] == (3 if flagged else 4)


# ------------------------------------------------------------------------------------------------ ABI refusals
EMPTY_GRID = 20480         # the address an empty grid (n = 0: nothing is launched, nothing dereferenced) is "built" at
_built = []


def _lib_():
    from epn_pointcloud_amd import _lib
    return _lib.get_lib()


def _vp(v):
    return ctypes.c_void_p(v) if v else None


def _icp(**over):
    """Pointers: non-NULL, 16-byte aligned and never dereferenced (every call here is refused)."""
    lib = _lib_()
    if not _built:
        assert lib.epn_point_grid_build_f32(None, 0, None, 0.1, _vp(EMPTY_GRID), int(lib.epn_point_grid_workspace_bytes(0)), None,
                                            None) == 0
        _built.append(True)
    a = dict(grid=EMPTY_GRID, n=0, normals=0, src=16, m=8, T_init=16, max_dist=0.1, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6,
             ws=32, ws_bytes=None, T=16, trace=16, iterations=16, status=16, sums=0, nn_idx=0)
    a.update(over)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = int(lib.epn_icp_workspace_bytes(max(min(a["m"], 2 ** 20), 0)))
    return lib.epn_icp_refine_f32(_vp(a["grid"]), a["n"], _vp(a["normals"]), _vp(a["src"]), a["m"], _vp(a["T_init"]), a["max_dist"],
                                  a["max_iter"], a["rel_fitness"], a["rel_rmse"], _vp(a["ws"]), a["ws_bytes"], _vp(a["T"]),
                                  _vp(a["trace"]), _vp(a["iterations"]), _vp(a["status"]), _vp(a["sums"]), _vp(a["nn_idx"]), None)


@pytest.mark.parametrize("bad,code", [
    (dict(n=-1), EINVAL), (dict(n=2 ** 22 + 1), EINVAL), (dict(m=-1), EINVAL), (dict(m=2 ** 20 + 1), EINVAL),
    (dict(max_dist=0.0), EINVAL), (dict(max_dist=-0.1), EINVAL), (dict(max_dist=float("nan")), EINVAL),
    (dict(max_dist=float("inf")), EINVAL), (dict(max_dist=0.1000001), EINVAL), (dict(max_iter=-1), EINVAL),
    (dict(max_iter=1025), EINVAL), (dict(rel_fitness=-1e-9), EINVAL), (dict(rel_fitness=float("nan")), EINVAL),
    (dict(rel_rmse=-1e-9), EINVAL), (dict(rel_rmse=float("inf")), EINVAL), (dict(grid=0), EINVAL), (dict(grid=EMPTY_GRID + 8), EINVAL),
    (dict(grid=EMPTY_GRID + 4096), EINVAL), (dict(n=1), EINVAL),
    (dict(T_init=0), ENULL), (dict(T=0), ENULL), (dict(iterations=0), ENULL), (dict(status=0), ENULL), (dict(src=0), ENULL),
    (dict(trace=0), ENULL),
    (dict(ws=0), EWORKSPACE), (dict(ws=40), EWORKSPACE), (dict(ws_bytes=255), EWORKSPACE), (dict(m=2 ** 20, ws_bytes=256 + 1024 * 256 - 1), EWORKSPACE),
], ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()) if isinstance(d, dict) else str(d))
def test_bad_arguments_are_refused_before_any_runtime_call(bad, code):
    assert _icp(**bad) == code


def test_refusals_come_in_the_stated_order():
    assert _icp(m=-1, T=0, ws=0) == EINVAL and _icp(T=0, ws=0) == ENULL


def test_workspace_bytes():
    lib = _lib_()
    assert lib.epn_icp_workspace_bytes(-1) == 0 and lib.epn_icp_workspace_bytes(2 ** 20 + 1) == 0
    assert lib.epn_icp_workspace_bytes(0) == 256 + 256 == lib.epn_icp_workspace_bytes(4)
    assert lib.epn_icp_workspace_bytes(5) == 256 + 2 * 256
    assert lib.epn_icp_workspace_bytes(4096) == 256 + 1024 * 256 == lib.epn_icp_workspace_bytes(2 ** 20)
    assert _lib_().epn_abi_version() == 3                              # entry points alone do not bump it


# ------------------------------------------------------------------------------------------------ the Python surface
def test_wrappers_refuse_host_tensors_and_bad_arguments(vgtk_alias):
    import torch
    import epn_pointcloud_amd as E
    from epn_pointcloud_amd.vgtk.cuda import grouping
    pc, ws, T = torch.zeros((8, 3)), torch.zeros(64, dtype=torch.int64), torch.eye(4, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        grouping.icp_refine(ws, 8, pc, T, 0.1)
    with pytest.raises(ValueError, match="shape"):
        grouping.icp_refine(ws, 8, torch.zeros((8, 2)), T, 0.1)
    with pytest.raises(TypeError, match="float32"):
        grouping.icp_refine(ws, 8, pc.double(), T, 0.1)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        E.refine_registration(pc, pc, np.eye(4), 0.1)
    with pytest.raises(ValueError, match="T_init"):
        E.refine_scene([pc, pc], [[0, 1]], np.eye(4)[None].repeat(2, axis=0), 0.1)
    with pytest.raises(ValueError, match="pairs"):
        E.refine_scene([pc, pc], [[0, 2]], np.eye(4)[None], 0.1)
    assert E.IcpResult._fields == ("T", "fitness", "inlier_rmse", "iterations", "status", "trace")
