"""Surface normals and patch frames without a GPU: the entry points exist at every layer, their argument checks run before any
HIP runtime call, and the restatement the GPU tests compare with (tests/normals_ref.py) is held to independent statements of
the same thing: a stable lexsort for the neighbourhood cut, planes whose normal is known in closed form, and a direct float64
transcription of the reference's three frame formulas."""
import ctypes

import numpy as np
import pytest

import normals_ref as N

EINVAL = -1


def test_symbols_resolve_and_are_bound_at_every_layer(vgtk_alias):
    from epn_pointcloud_amd import _lib, correspondence
    from epn_pointcloud_amd.vgtk.cuda import grouping
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("epn_point_normals_f32", "epn_orient_patches_f32"):
        assert name in _lib.EXPORTS
        assert hasattr(cdll, name)
    assert callable(grouping.point_normals) and callable(grouping.orient_patches)
    import vgtk.pc
    for name in ("PointNormals", "estimate_normals", "orient_patches"):
        assert getattr(vgtk.pc, name) is getattr(correspondence, name)
    assert callable(vgtk.pc.PointGrid.normals)
    assert vgtk.pc.PointNormals._fields == ("normals", "eig", "count", "flags", "moments", "neighbors")
    assert _lib.get_lib().epn_abi_version() == 3                    # entry points alone do not bump it


# ------------------------------------------------------------------------------------------------ the restatement
def test_the_key_cut_is_a_stable_k_nearest():
    """Lattice coordinates (multiples of 2^-2, duplicates included): many equal distances.  The max_nn smallest (d2 bits, row) keys are the first
    max_nn rows of a stable sort by (d2, row), and d2 orders like its bits."""
    rng = np.random.default_rng(0)
    ref = (rng.integers(-4, 5, (400, 3)) / 4.0).astype(np.float32)
    ties = 0
    for q in ref[:20]:
        d = ref.astype(np.float64) - q.astype(np.float64)
        d2 = (d * d).sum(axis=1)                                    # exact on this lattice, in fp32 and fp64 alike
        inside = np.nonzero(d2 <= 0.25)[0]
        order = inside[np.lexsort((inside, d2[inside]))]
        ties += int((np.diff(d2[order]) == 0).sum())
        for max_nn in (0, 1, 5, order.size - 1, order.size, order.size + 1):
            count, rows = N.neighbourhood(ref, q, 0.5, max_nn)
            assert count == order.size
            assert rows.tolist() == (order if max_nn == 0 else order[:max_nn]).tolist()
    assert ties > 100                                               # ties are what this is about


def test_the_radius_edge_and_non_finite_rows():
    ref = np.array([[0.5, 0, 0], [np.nextafter(np.float32(0.5), np.float32(1)), 0, 0], [np.nan, 0, 0], [0, 0, 0]], np.float32)
    assert N.neighbourhood(ref, [0, 0, 0], 0.5, 0)[1].tolist() == [3, 0]             # d2 == r2 is inside; NaN rows never
    assert N.neighbourhood(ref, [np.inf, 0, 0], 0.5, 0) [0] == 0
    out = N.point_normals(ref, [[np.nan, 0, 0], [9, 9, 9], [0, 0, 0]], 0.5)
    assert out["flags"].tolist() == [N.FLAG_FEW | N.FLAG_QUERY, N.FLAG_FEW, N.FLAG_FEW]
    assert out["count"].tolist() == [0, 0, 2] and (out["normals"] == [0, 0, 1]).all() and (out["eig"] == 0).all()


def test_moments_are_exact_integers_on_a_lattice():
    """t = 1/4, -1/2: rint(t 2^40) and rint(t t 2^40) are exact, so the sums are known by hand."""
    ref = np.array([[0.25, 0, 0], [0, -0.5, 0], [0.25, -0.5, 0.25]], np.float32)
    mom = N.moments_of(ref, [0, 0, 0], np.arange(3), 1.0)
    u = 2 ** 40
    assert mom.tolist() == [u // 2, -u, u // 4, u // 8, -u // 8, u // 16, u // 2, -u // 8, u // 16]
    assert N.moments_of(ref[::-1], [0, 0, 0], np.arange(3), 1.0).tolist() == mom.tolist()       # any order


@pytest.mark.parametrize("view, sign", [(None, 1), ([0, 0, 5], 1), ([0, 0, -5], -1)])
def test_lattice_planes_have_their_closed_form_normals(view, sign):
    grid = np.array([[x, y] for x in range(-2, 3) for y in range(-2, 3)]) / 4.0
    flat = np.column_stack((grid, np.zeros(25))).astype(np.float32)                  # z = 0
    out = N.point_normals(flat, flat, 0.5, max_nn=0, view=view)
    assert (out["flags"] == 0).all() and (out["count"] >= 6).all()
    assert np.abs(out["normals"] - [0, 0, sign]).max() <= 2.0 ** -50 and np.abs(out["lam"][:, 0]).max() <= 2.0 ** -50
    diag = np.column_stack((grid[:, 0], grid[:, 0], grid[:, 1])).astype(np.float32)  # x = y
    out = N.point_normals(diag, diag, 0.75, max_nn=0, view=None if view is None else [view[2], -view[2], 0])
    s = np.sqrt(0.5)
    assert (out["flags"] == 0).all()
    if view is None:          # |n0| == |n1|: the rule's tie is decided by the last bit of either; the direction is what is known
        assert np.abs(np.abs(out["normals"] @ np.array([s, -s, 0])) - 1).max() <= 2.0 ** -50
    else:
        assert np.abs(out["normals"] - np.array([s, -s, 0]) * sign).max() <= 2.0 ** -50


def test_three_points_span_their_plane():
    rng = np.random.default_rng(1)
    for _ in range(50):
        tri = rng.uniform(-0.2, 0.2, (3, 3)).astype(np.float32)
        out = N.point_normals(tri, tri[:1], 1.0)
        want = np.cross(tri[1].astype(np.float64) - tri[0], tri[2].astype(np.float64) - tri[0])
        want /= np.linalg.norm(want)
        want *= np.sign(want[np.argmax(np.abs(want))])
        gap = out["lam"][0, 1] - out["lam"][0, 0]
        assert out["count"][0] == 3 and out["flags"][0] == 0
        # each of the 3 + 3 terms of an entry of C is within 2^-41 of its exact value: |dC| <= 2^-38, and |dn| <= |dC| / gap
        assert np.abs(out["normals"][0] - want).max() <= 2.0 ** -38 / gap
    line = np.outer([0.0, 1.0, 2.0], [0.1, 0.05, -0.1]).astype(np.float32)
    assert N.point_normals(line, line[:1], 1.0)["flags"][0] == N.FLAG_GAP


def _frame_direct(normal):
    """transform_with_normals' three formulas, transcribed in float64 with numpy's own norm and cross"""
    unit = lambda v: v / (np.linalg.norm(v) + 1e-5)
    z = unit(np.asarray(normal, np.float32).astype(np.float64))
    x = unit(np.cross(np.array([0.0, -1.0, 0.0]), z))
    y = unit(np.cross(z, x))
    return np.concatenate((x[:, None], y[:, None], z[:, None]), axis=1)


def test_patch_frames_against_a_direct_transcription():
    rng = np.random.default_rng(2)
    normals = np.vstack((rng.standard_normal((300, 3)), 1e-3 * rng.standard_normal((50, 3)))).astype(np.float32)
    for n in normals:
        axis = N.patch_frame(n)
        want = _frame_direct(n)
        assert axis.dtype == np.float32 and np.abs(axis - want).max() <= 2.0 ** -24     # one rounding to fp32 of a value <= 1
        if np.linalg.norm(n) > 0.1:
            assert np.abs(axis.astype(np.float64).T @ axis - np.eye(3)).max() < 1e-3    # orthonormal up to the 1e-5 terms
    for n in ([0, -1, 0], [0, 1, 0], [0, -0.01, 0], [0, 0, 0]):                          # parallel to up: x and y collapse to zero
        axis = N.patch_frame(n)
        assert np.isfinite(axis).all() and (axis[:, :2] == 0).all() and np.abs(axis - _frame_direct(n)).max() <= 2.0 ** -24
    patches = rng.uniform(-1, 1, (3, 7, 3)).astype(np.float32)
    patches[1, 4] = 0
    out, axis = N.orient_patches(patches, normals[:3])
    assert np.abs(out - np.einsum("kni,kij->knj", patches.astype(np.float64), axis.astype(np.float64))).max() <= 2.0 ** -23
    assert (out[1, 4] == 0).all()


def test_the_noisy_sphere_is_well_conditioned():
    """The cloud of the GPU tests: at most 2 % of its points may carry the undetermined-direction flag, and the restatement's
    normals point outwards to within the noise."""
    pts = N.noisy_sphere()
    out = N.point_normals(pts, pts[::10], 0.2, max_nn=30, view=[0, 0, 0])
    share = (out["flags"] & N.FLAG_GAP != 0).mean()
    print(f"flag bit 2 on {share:.2%} of the noisy sphere's queries; smallest count {out['count'].min()}")
    assert share <= 0.02 and (out["flags"] & N.FLAG_FEW == 0).all()
    outward = pts[::10] / np.linalg.norm(pts[::10], axis=1, keepdims=True)
    assert ((out["normals"] * outward).sum(axis=1) < -0.9).all()    # towards the view at the centre


# ------------------------------------------------------------------------------------------------ ABI refusals
EMPTY_GRID = 12288         # the address an empty grid (n = 0: nothing is launched, nothing dereferenced) is "built" at
_built = []


def _lib_():
    from epn_pointcloud_amd import _lib
    return _lib.get_lib()


def _vp(v):
    return ctypes.c_void_p(v) if v else None


def _normals(**over):
    """Pointers: non-NULL, 16-byte aligned and never dereferenced (every call is refused, or m = 0)."""
    lib = _lib_()
    if not _built:
        assert lib.epn_point_grid_build_f32(None, 0, None, 0.1, _vp(EMPTY_GRID), int(lib.epn_point_grid_workspace_bytes(0)), None,
                                            None) == 0
        _built.append(True)
    a = dict(workspace=EMPTY_GRID, n=0, qry=16, m=0, radius=0.1, max_nn=30, self_rows=0, view=0, normals=16, eig=16, count=16,
             flags=16, moments=0, nbr_idx=0)
    a.update(over)
    return lib.epn_point_normals_f32(_vp(a["workspace"]), a["n"], _vp(a["qry"]), a["m"], a["radius"], a["max_nn"], a["self_rows"],
                                     _vp(a["view"]), _vp(a["normals"]), _vp(a["eig"]), _vp(a["count"]), _vp(a["flags"]),
                                     _vp(a["moments"]), _vp(a["nbr_idx"]), None)


@pytest.mark.parametrize("bad", [dict(n=-1), dict(n=2 ** 22 + 1), dict(m=-1), dict(m=2 ** 22 + 1), dict(radius=0.0),
                                 dict(radius=-0.05), dict(radius=float("nan")), dict(radius=float("inf")),
                                 dict(radius=0.1000001), dict(max_nn=-1), dict(max_nn=1025), dict(max_nn=0, nbr_idx=16),
                                 dict(self_rows=2), dict(self_rows=1, m=5), dict(workspace=0), dict(workspace=EMPTY_GRID + 8),
                                 dict(workspace=EMPTY_GRID + 4096), dict(n=1), dict(m=3, qry=0), dict(m=3, normals=0),
                                 dict(m=3, eig=0), dict(m=3, count=0), dict(m=3, flags=0)],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_bad_normals_arguments_are_refused_before_any_runtime_call(bad):
    assert _normals(**bad) == EINVAL


def test_no_queries_launch_nothing():
    assert _normals() == 0
    assert _normals(qry=0, normals=0, eig=0, count=0, flags=0) == 0
    assert _normals(max_nn=0) == 0 and _normals(max_nn=1024, nbr_idx=16, moments=16) == 0
    assert _normals(self_rows=1) == 0                               # m == n == 0
    assert _normals(radius=0.05, view=16) == 0


def _orient(**over):
    a = dict(patches=16, normals=16, k=0, n_sample=1024, axis=16, out=16)
    a.update(over)
    return _lib_().epn_orient_patches_f32(_vp(a["patches"]), _vp(a["normals"]), a["k"], a["n_sample"], _vp(a["axis"]),
                                          _vp(a["out"]), None)


@pytest.mark.parametrize("bad", [dict(k=-1), dict(k=2 ** 22 + 1), dict(n_sample=0), dict(n_sample=-4), dict(n_sample=8193),
                                 dict(k=2, patches=0), dict(k=2, normals=0), dict(k=2, axis=0), dict(k=2, out=0)],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_bad_orient_arguments_are_refused_before_any_runtime_call(bad):
    assert _orient(**bad) == EINVAL


def test_no_patches_launch_nothing():
    assert _orient() == 0 and _orient(patches=0, normals=0, axis=0, out=0) == 0 and _orient(n_sample=1) == 0
    assert _orient(n_sample=8192) == 0


# ------------------------------------------------------------------------------------------------ the Python surface
def test_wrappers_refuse_host_tensors_and_bad_shapes(vgtk_alias):
    import torch
    import vgtk.pc
    from epn_pointcloud_amd.vgtk.cuda import grouping
    pc, ws = torch.zeros((8, 3)), torch.zeros(64, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        grouping.point_normals(ws, 8, pc, 0.1)
    with pytest.raises(ValueError, match="shape"):                  # data._tensor's order: type, shape, dtype, device
        grouping.point_normals(ws, 8, torch.zeros((8, 2)), 0.1)
    with pytest.raises(TypeError, match="float32"):
        grouping.point_normals(ws, 8, pc.double(), 0.1)
    with pytest.raises(TypeError, match="torch tensor"):
        grouping.point_normals(ws, 8, pc.numpy(), 0.1)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        vgtk.pc.estimate_normals(pc, 0.1)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        vgtk.pc.orient_patches(torch.zeros((2, 5, 3)), torch.zeros((2, 3)))
    with pytest.raises(ValueError, match="shape"):
        vgtk.pc.orient_patches(torch.zeros((2, 5)), torch.zeros((2, 3)))
    with pytest.raises(TypeError, match="float32"):
        vgtk.pc.orient_patches(torch.zeros((2, 5, 3), dtype=torch.float64), torch.zeros((2, 3)))
    with pytest.raises(ValueError, match=r"normals must be a \[k,3\]"):
        vgtk.pc.radius_patches(pc, pc[:4], 0.1, 16, normals=torch.zeros((5, 3)))
    with pytest.raises(TypeError):
        vgtk.pc.radius_patches(pc, pc[:4], 0.1, 16, 0, False, 1.0, None, torch.zeros((4, 3)))   # keyword-only


def test_describe_checks_its_normals_before_any_device_work(vgtk_alias):
    import torch
    from epn_pointcloud_amd import models
    model = models.InvSO3ConvModel.__new__(models.InvSO3ConvModel)
    torch.nn.Module.__init__(model)
    model.search_radius, model.input_num = 0.3, 16
    model.eval()
    pc, rows = torch.zeros((8, 3)), torch.arange(4)
    with pytest.raises(ValueError, match="normals must be a"):
        model.describe(pc, rows, normals=torch.zeros((4, 2)))
    with pytest.raises(ValueError, match="one row per keypoint"):
        model.describe(pc, rows, normals=torch.zeros((5, 3)))
    with pytest.raises(ValueError, match="one row per keypoint"):
        model.describe(pc, pc[:4], normals=torch.zeros((8, 3)))    # [n,3] is gathered only through integer rows
