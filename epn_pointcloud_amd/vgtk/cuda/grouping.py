"""`vgtk.cuda.grouping` -- same function names/signatures as vgtk/vgtk/cuda/grouping_cuda.cpp:176-181."""
import ctypes

import numpy as np
import torch

from ... import _lib


def ball_query(new_xyz, xyz, radius, nsample):
    """(new_xyz f[b,3,m], xyz f[b,3,n], float radius, int nsample) -> int32 [b,m,nsample]; float32 or float64 coordinates
    (grouping_cuda.cpp:71-86; AT_DISPATCH_FLOATING_TYPES, grouping_cuda_kernel.cu:477)."""
    lib = _lib.get_lib()
    dt = _lib.float_dtype(xyz, "xyz")
    q, s = _lib.dev_ptr(new_xyz, "new_xyz", dt), _lib.dev_ptr(xyz, "xyz", dt)
    b, _, m = new_xyz.shape
    n = xyz.shape[2]
    idx = torch.empty((b, m, int(nsample)), dtype=torch.int32, device=xyz.device)
    fn = lib.epn_ball_query_f64 if dt == torch.float64 else lib.epn_ball_query_f32
    _lib.check(fn(q, s, b, n, m, float(radius), int(nsample), _lib.dev_ptr(idx, "idx", torch.int32), _lib.stream_of(xyz)),
               "ball_query")
    return idx


def furthest_point_sampling(source_xyz, m):
    """(xyz f[b,3,n], int m) -> int32 [b,m]; float32 or float64 coordinates (grouping_cuda.cpp:160-174; the fp64
    instantiation keeps its running minima in a temp tensor like the reference, :167-168)."""
    lib = _lib.get_lib()
    dt = _lib.float_dtype(source_xyz, "source_xyz")
    p = _lib.dev_ptr(source_xyz, "source_xyz", dt)
    b, _, n = source_xyz.shape
    idx = torch.empty((b, int(m)), dtype=torch.int32, device=source_xyz.device)
    if dt == torch.float64:
        temp = torch.empty((b, n), dtype=torch.float64, device=source_xyz.device)
        _lib.check(lib.epn_fps_f64(p, b, n, int(m), _lib.dev_ptr(temp, "temp", dt),
                                   _lib.dev_ptr(idx, "sampled_idx", torch.int32), _lib.stream_of(source_xyz)),
                   "furthest_point_sampling")
        return idx
    if n > 32768:        # beyond the register-resident kernels: the reference's own structure, minima in `temp` (:167-168)
        temp = torch.empty((b, n), dtype=torch.float32, device=source_xyz.device)
        _lib.check(lib.epn_fps_temp_f32(p, b, n, int(m), _lib.dev_ptr(temp, "temp", dt),
                                        _lib.dev_ptr(idx, "sampled_idx", torch.int32), _lib.stream_of(source_xyz)),
                   "furthest_point_sampling")
        return idx
    _lib.check(lib.epn_fps_f32(p, b, n, int(m), _lib.dev_ptr(idx, "sampled_idx", torch.int32),
                               _lib.stream_of(source_xyz)), "furthest_point_sampling")
    return idx


def radius_patches(pc, kpts, radius, n_sample, seed=0, kpt_row0=0, key_bits=32, center=False, scale=1.0):
    """(pc f[n,3], kpts f[k,3], float radius, int n_sample) -> (idx int32 [k,n_sample], counts int32 [k],
    patches f[k,n_sample,3]): the points of one fragment within `radius` of every keypoint, resampled to n_sample
    (epn_radius_patches_f32, include/epn_so3conv.h; no counterpart among the reference's extensions -- it replaces the
    host KD-tree path of match_3dmatch.py:154-177 and vgtk/pc/sample.py:16-36).  kpt_row0 is the global row of kpts[0]."""
    lib = _lib.get_lib()
    _lib.same_device(pc, kpts)
    p, q = _lib.dev_ptr(pc, "pc"), _lib.dev_ptr(kpts, "kpts")
    if pc.dim() != 2 or pc.shape[1] != 3 or kpts.dim() != 2 or kpts.shape[1] != 3:
        raise ValueError(f"pc must be [n,3] and kpts [k,3], got {tuple(pc.shape)} and {tuple(kpts.shape)}")
    n, k, ns = pc.shape[0], kpts.shape[0], int(n_sample)
    if not 1 <= ns <= 8192:
        raise ValueError(f"n_sample must be in 1..8192, got {ns}")
    idx = torch.empty((k, ns), dtype=torch.int32, device=pc.device)
    counts = torch.empty((k,), dtype=torch.int32, device=pc.device)
    patches = torch.empty((k, ns, 3), dtype=torch.float32, device=pc.device)
    _lib.check(lib.epn_radius_patches_f32(p, n, q, k, int(kpt_row0), float(radius), ns, int(seed) & (2 ** 64 - 1),
                                          int(key_bits), int(bool(center)), float(scale),
                                          _lib.dev_ptr(idx, "idx", torch.int32), _lib.dev_ptr(counts, "counts", torch.int32),
                                          _lib.dev_ptr(patches, "patches"), _lib.stream_of(pc)), "radius_patches")
    return idx, counts, patches


_VOXEL_FLAGS = ("bit 0: a coordinate exceeds 256 in magnitude",
                "bit 1: a voxel index reaches 2^21 (the cloud's extent / voxel_size is too large)",
                "bit 2: the hash table overflowed")


def voxel_downsample(pc, voxel_size):
    """(pc f[n,3], float voxel_size) -> (centroids f[M,3], counts int32 [M], first_idx int32 [M], point_voxel int32 [n]): one
    centroid per occupied voxel of a fragment, voxels in ascending order of their lowest point index, point_voxel the row of
    every point's voxel (-1 for a point with a non-finite coordinate) (epn_voxel_downsample_f32, include/epn_so3conv.h; no
    counterpart among the reference's extensions -- it replaces open3d's voxel_down_sample of match_3dmatch.py:107-139).  The
    status word is read back once; a range error raises ValueError naming its bit."""
    lib = _lib.get_lib()
    p = _lib.dev_ptr(pc, "pc")
    if pc.dim() != 2 or pc.shape[1] != 3:
        raise ValueError(f"pc must be [n,3], got {tuple(pc.shape)}")
    vs = float(voxel_size)
    if not (np.isfinite(vs) and vs > 0.0):
        raise ValueError(f"voxel_size must be finite and > 0, got {voxel_size}")
    n = pc.shape[0]
    if n > 2 ** 22:
        raise ValueError(f"voxel_downsample takes at most 2^22 points, got {n}")
    i32 = dict(dtype=torch.int32, device=pc.device)
    centroids = torch.empty((n, 3), dtype=torch.float32, device=pc.device)
    counts, first_idx, point_voxel = torch.empty((n,), **i32), torch.empty((n,), **i32), torch.empty((n,), **i32)
    if n == 0:
        return centroids, counts, first_idx, point_voxel
    status = torch.empty((2,), **i32)
    ws_bytes = int(lib.epn_voxel_downsample_workspace_bytes(n))
    ws = torch.empty(((ws_bytes + 7) // 8,), dtype=torch.int64, device=pc.device)
    _lib.check(lib.epn_voxel_downsample_f32(p, n, vs, _lib.dev_ptr(centroids, "centroids"),
                                            _lib.dev_ptr(counts, "counts", torch.int32),
                                            _lib.dev_ptr(first_idx, "first_idx", torch.int32),
                                            _lib.dev_ptr(point_voxel, "point_voxel", torch.int32),
                                            _lib.dev_ptr(status, "status", torch.int32), ctypes.c_void_p(ws.data_ptr()),
                                            ws.numel() * 8, _lib.stream_of(pc)), "voxel_downsample")
    m, flags = status.tolist()
    if flags:
        raise ValueError("voxel_downsample: status " + "; ".join(t for b, t in enumerate(_VOXEL_FLAGS) if flags >> b & 1)
                         + f" (flags = {flags}, voxel_size = {vs})")
    return centroids[:m], counts[:m], first_idx[:m], point_voxel


MAX_GRID_POINTS = 2 ** 22
MIN_GRID_RADIUS = 2.0 ** -60


def point_grid_build(ref, max_radius, valid=None):
    """(ref f[n,3], float max_radius, valid u8/bool [n] or None) -> (workspace int64 tensor, status int32 [2] = {kept, flags}
    on the device, or None when n == 0): the hashed grid of one cloud with its points sorted by cell, for point_grid_nn with
    any radius <= max_radius (epn_point_grid_build_f32, include/epn_so3conv.h; no counterpart among the reference's
    extensions -- it replaces the host trees of SPConvNets/datasets/preprocess/run_keypoint.py).  Nothing is read back: the
    caller looks at status[1] (the flags of voxel_downsample) when it wants to."""
    from ...data import _tensor
    lib = _lib.get_lib()
    ref = _tensor(ref, "ref", (None, 3), torch.float32)
    n = ref.shape[0]
    if valid is not None:
        valid = _tensor(valid, "valid", (n,), (torch.uint8, torch.bool))
        if valid.dtype == torch.bool:
            valid = valid.to(torch.uint8)
    r = float(max_radius)
    if not (np.isfinite(r) and r >= MIN_GRID_RADIUS):
        raise ValueError(f"max_radius must be finite and >= 2^-60, got {max_radius}")
    if n > MAX_GRID_POINTS:
        raise ValueError(f"a point grid takes at most 2^22 points, got {n}")
    _lib.same_device(ref, valid)
    ws_bytes = int(lib.epn_point_grid_workspace_bytes(n))
    ws = torch.empty(((ws_bytes + 7) // 8,), dtype=torch.int64, device=ref.device)
    status = torch.empty((2,), dtype=torch.int32, device=ref.device) if n else None
    _lib.check(lib.epn_point_grid_build_f32(_lib.dev_ptr(ref, "ref"), n, _lib.dev_ptr(valid, "valid", torch.uint8), r,
                                            ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8,
                                            _lib.dev_ptr(status, "status", torch.int32), _lib.stream_of(ref)), "point_grid_build")
    return ws, status


def point_grid_nn(workspace, n, queries, radius, exclude_row=False, count=False):
    """(workspace from point_grid_build of n points, queries f[m,3], float radius <= the build's max_radius) -> (nn_idx int32
    [m], nn_d2 f[m][, hits int32 [1]]): per query the nearest point of the grid within radius -- the smallest fp32 squared
    distance, the lowest row on a tie -- or -1 and +inf; exclude_row skips the candidate at the query's own row (m == n);
    hits, with count, is the number of queries that found one, on the device (epn_point_grid_nn_f32)."""
    from ...data import _tensor
    lib = _lib.get_lib()
    workspace = _tensor(workspace, "workspace", (None,), torch.int64)
    queries = _tensor(queries, "queries", (None, 3), torch.float32)
    n, m, r = int(n), queries.shape[0], float(radius)
    if not (np.isfinite(r) and r > 0.0):
        raise ValueError(f"radius must be finite and > 0, got {radius}")
    if m > MAX_GRID_POINTS:
        raise ValueError(f"a call takes at most 2^22 queries, got {m}")
    if exclude_row and m != n:
        raise ValueError(f"exclude_row needs the grid's own {n} points as queries, got {m}")
    _lib.same_device(workspace, queries)
    nn_idx = torch.empty((m,), dtype=torch.int32, device=queries.device)
    nn_d2 = torch.empty((m,), dtype=torch.float32, device=queries.device)
    hits = torch.empty((1,), dtype=torch.int32, device=queries.device) if count else None
    _lib.check(lib.epn_point_grid_nn_f32(ctypes.c_void_p(workspace.data_ptr()), n, _lib.dev_ptr(queries, "queries"), m, r,
                                         int(bool(exclude_row)), _lib.dev_ptr(nn_idx, "nn_idx", torch.int32),
                                         _lib.dev_ptr(nn_d2, "nn_d2"), _lib.dev_ptr(hits, "hits", torch.int32),
                                         _lib.stream_of(queries)), "point_grid_nn")
    return (nn_idx, nn_d2, hits) if count else (nn_idx, nn_d2)


MAX_NORMAL_NN = 1024


def point_normals(workspace, n, queries, radius, max_nn=30, self_rows=False, view=None, return_moments=False,
                  return_neighbors=False):
    """(workspace from point_grid_build of n points, queries f[m,3], float radius <= the build's max_radius, int max_nn with
    0 = no limit, view f[3] on the device or None) -> (normals f[m,3], eig f[m,3], count int32 [m], flags int32 [m], moments
    int64 [m,9] or None, neighbors int32 [m,max_nn] or None): the plane fitted to every query's neighbourhood in the grid
    (epn_point_normals_f32, include/epn_so3conv.h; no counterpart among the reference's extensions -- it replaces open3d's
    estimate_normals of SPConvNets/datasets/preprocess/run_fusion.py:48).  self_rows states that the queries are the grid's
    own points."""
    from ...data import _tensor
    lib = _lib.get_lib()
    queries = _tensor(queries, "queries", (None, 3), torch.float32)
    workspace = _tensor(workspace, "workspace", (None,), torch.int64)
    if view is not None:
        view = _tensor(view, "view", (3,), torch.float32)
    n, m, r, nn = int(n), queries.shape[0], float(radius), int(max_nn)
    if not (np.isfinite(r) and r > 0.0):
        raise ValueError(f"radius must be finite and > 0, got {radius}")
    if not 0 <= nn <= MAX_NORMAL_NN:
        raise ValueError(f"max_nn must be in 0..{MAX_NORMAL_NN} (0 = no limit), got {max_nn}")
    if return_neighbors and nn == 0:
        raise ValueError("return_neighbors needs max_nn >= 1: the rows of an unlimited neighbourhood have no fixed width")
    if m > MAX_GRID_POINTS:
        raise ValueError(f"a call takes at most 2^22 queries, got {m}")
    if self_rows and m != n:
        raise ValueError(f"self_rows needs the grid's own {n} points as queries, got {m}")
    _lib.same_device(workspace, queries, view)
    f32, i32 = dict(dtype=torch.float32, device=queries.device), dict(dtype=torch.int32, device=queries.device)
    normals, eig = torch.empty((m, 3), **f32), torch.empty((m, 3), **f32)
    count, flags = torch.empty((m,), **i32), torch.empty((m,), **i32)
    moments = torch.empty((m, 9), dtype=torch.int64, device=queries.device) if return_moments else None
    neighbors = torch.empty((m, nn), **i32) if return_neighbors else None
    _lib.check(lib.epn_point_normals_f32(ctypes.c_void_p(workspace.data_ptr()), n, _lib.dev_ptr(queries, "queries"), m, r, nn,
                                         int(bool(self_rows)), _lib.dev_ptr(view, "view"), _lib.dev_ptr(normals, "normals"),
                                         _lib.dev_ptr(eig, "eig"), _lib.dev_ptr(count, "count", torch.int32),
                                         _lib.dev_ptr(flags, "flags", torch.int32),
                                         _lib.dev_ptr(moments, "moments", torch.int64),
                                         _lib.dev_ptr(neighbors, "neighbors", torch.int32), _lib.stream_of(queries)),
               "point_normals")
    return normals, eig, count, flags, moments, neighbors


def orient_patches(patches, normals, out=None):
    """(patches f[k,n_sample,3], normals f[k,3]) -> (out f[k,n_sample,3], axis f[k,3,3]): every patch in the frame of its normal,
    out = patch @ axis (epn_orient_patches_f32, include/epn_so3conv.h; no counterpart among the reference's extensions -- it
    replaces transform_with_normals of SPConvNets/datasets/match_3dmatch.py:141-152).  out may be `patches` itself."""
    from ...data import _tensor
    lib = _lib.get_lib()
    patches = _tensor(patches, "patches", (None, None, 3), torch.float32)
    k, ns = patches.shape[0], patches.shape[1]
    normals = _tensor(normals, "normals", (k, 3), torch.float32)
    if not 1 <= ns <= 8192:
        raise ValueError(f"n_sample must be in 1..8192, got {ns}")
    if k > MAX_GRID_POINTS:
        raise ValueError(f"a call takes at most 2^22 patches, got {k}")
    if out is None:
        out = torch.empty_like(patches)
    else:
        if isinstance(out, torch.Tensor) and not out.is_contiguous():
            raise RuntimeError("out must be contiguous: the result is written into it")
        out = _tensor(out, "out", (k, ns, 3), torch.float32)
    _lib.same_device(patches, normals, out)
    axis = torch.empty((k, 3, 3), dtype=torch.float32, device=patches.device)
    _lib.check(lib.epn_orient_patches_f32(_lib.dev_ptr(patches, "patches"), _lib.dev_ptr(normals, "normals"), k, ns,
                                          _lib.dev_ptr(axis, "axis"), _lib.dev_ptr(out, "out"), _lib.stream_of(patches)),
               "orient_patches")
    return out, axis


FPFH_WIDTH = 33


def point_fpfh(workspace, n, points, normals, radius, return_spfh=False):
    """(workspace from point_grid_build of the n points `points` f[n,3], normals f[n,3], float radius <= the build's max_radius)
    -> (fpfh f[n,33], count int32 [n], flags int32 [n], spfh int32 [n,33] or None): the FPFH descriptor of every point of the
    grid's own cloud over its in-radius neighbourhood (epn_point_fpfh_f32, include/epn_so3conv.h; no counterpart among the
    reference's extensions -- it replaces open3d's compute_fpfh_feature of SPConvNets/datasets/preprocess/run_keypoint.py:40-50).
    flags bit 0: no neighbour; bit 1: a non-finite coordinate or normal, or a point the grid leaves out; the row is zero with
    either."""
    from ...data import _tensor
    lib = _lib.get_lib()
    workspace = _tensor(workspace, "workspace", (None,), torch.int64)
    n, r = int(n), float(radius)
    points = _tensor(points, "points", (n, 3), torch.float32)
    normals = _tensor(normals, "normals", (n, 3), torch.float32)
    if not (np.isfinite(r) and r > 0.0):
        raise ValueError(f"radius must be finite and > 0, got {radius}")
    if n > MAX_GRID_POINTS:
        raise ValueError(f"a point grid takes at most 2^22 points, got {n}")
    _lib.same_device(workspace, points, normals)
    i32 = dict(dtype=torch.int32, device=points.device)
    fpfh = torch.empty((n, FPFH_WIDTH), dtype=torch.float32, device=points.device)
    count, flags = torch.empty((n,), **i32), torch.empty((n,), **i32)
    spfh = torch.empty((n, FPFH_WIDTH), **i32) if return_spfh else None
    ws_bytes = int(lib.epn_point_fpfh_workspace_bytes(n))
    ws = torch.empty(((ws_bytes + 7) // 8,), dtype=torch.int64, device=points.device)
    _lib.check(lib.epn_point_fpfh_f32(ctypes.c_void_p(workspace.data_ptr()), n, _lib.dev_ptr(points, "points"),
                                      _lib.dev_ptr(normals, "normals"), r, _lib.dev_ptr(fpfh, "fpfh"),
                                      _lib.dev_ptr(count, "count", torch.int32), _lib.dev_ptr(flags, "flags", torch.int32),
                                      _lib.dev_ptr(spfh, "spfh", torch.int32), ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8,
                                      _lib.stream_of(points)), "point_fpfh")
    return fpfh, count, flags, spfh


MAX_ICP_POINTS = 2 ** 20
MAX_ICP_ITER = 1024
ICP_FLAGS = ("bit 0: converged (the stop test was met)",
             "bit 1: too few correspondences (fewer than 3, or 6 for point-to-plane)",
             "bit 2: the iteration's system is singular or ill-conditioned",
             "bit 3: a matched coordinate exceeds 64 in magnitude (or a normal component exceeds 1)")


def icp_refine(workspace, n, src, T_init, max_dist, tgt_normals=None, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6,
               return_sums=False, return_nn=False):
    """(workspace from point_grid_build of the n target points, src f[m,3], T_init f64 [4,4] on the device taking src into the
    target's frame, float max_dist <= the build's max_radius, tgt_normals f[n,3] or None) -> (T f64 [4,4], trace f64
    [max_iter,20], iterations int32 [1], status int32 [1], sums int64 [32] or None, nn_idx int32 [m] or None), device tensors:
    ICP from T_init, point-to-point without normals and point-to-plane with them; a trace record is {T after the iteration
    (16), count, sum of squared distances, rmse, flags} (epn_icp_refine_f32, include/epn_so3conv.h; no counterpart in the
    reference -- the host tool for this step is open3d's registration_icp).  Nothing is read back."""
    from ...data import _tensor
    lib = _lib.get_lib()
    src = _tensor(src, "src", (None, 3), torch.float32)
    T_init = _tensor(T_init, "T_init", (4, 4), torch.float64)
    workspace = _tensor(workspace, "workspace", (None,), torch.int64)
    n, m, r, K = int(n), src.shape[0], float(max_dist), int(max_iter)
    if tgt_normals is not None:
        tgt_normals = _tensor(tgt_normals, "tgt_normals", (n, 3), torch.float32)
    if not (np.isfinite(r) and r > 0.0):
        raise ValueError(f"max_dist must be finite and > 0, got {max_dist}")
    if not 0 <= K <= MAX_ICP_ITER:
        raise ValueError(f"max_iter must be in 0..{MAX_ICP_ITER}, got {max_iter}")
    if m > MAX_ICP_POINTS:
        raise ValueError(f"a call takes at most 2^20 source points, got {m}")
    for name, v in (("rel_fitness", rel_fitness), ("rel_rmse", rel_rmse)):
        if not (np.isfinite(v) and v >= 0.0):
            raise ValueError(f"{name} must be finite and >= 0, got {v}")
    _lib.same_device(workspace, src, T_init, tgt_normals)
    f64, i32 = dict(dtype=torch.float64, device=src.device), dict(dtype=torch.int32, device=src.device)
    T, trace = torch.empty((4, 4), **f64), torch.empty((K, 20), **f64)
    iterations, status = torch.empty((1,), **i32), torch.empty((1,), **i32)
    sums = torch.empty((32,), dtype=torch.int64, device=src.device) if return_sums else None
    nn_idx = torch.empty((m,), **i32) if return_nn else None
    ws_bytes = int(lib.epn_icp_workspace_bytes(m))
    ws = torch.empty(((ws_bytes + 15) // 16 * 2,), dtype=torch.int64, device=src.device)
    _lib.check(lib.epn_icp_refine_f32(ctypes.c_void_p(workspace.data_ptr()), n, _lib.dev_ptr(tgt_normals, "tgt_normals"),
                                      _lib.dev_ptr(src, "src"), m, _lib.dev_ptr(T_init, "T_init", torch.float64), r, K,
                                      float(rel_fitness), float(rel_rmse), ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8,
                                      _lib.dev_ptr(T, "T", torch.float64), _lib.dev_ptr(trace, "trace", torch.float64),
                                      _lib.dev_ptr(iterations, "iterations", torch.int32),
                                      _lib.dev_ptr(status, "status", torch.int32), _lib.dev_ptr(sums, "sums", torch.int64),
                                      _lib.dev_ptr(nn_idx, "nn_idx", torch.int32), _lib.stream_of(src)), "icp_refine")
    return T, trace, iterations, status, sums, nn_idx


def _scene_tables(frag_off, pairs, device):
    """Host copies (contiguous numpy: what the library's argument checks read) and device copies (what its kernels read) of a
    scene's tables, with out_off / tgt_off computed from them (include/epn_so3conv.h, "Scene tables")."""
    fo = np.ascontiguousarray(np.asarray(frag_off, dtype=np.int64).reshape(-1))
    pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    if fo.size < 2:
        raise ValueError("frag_off must hold F + 1 >= 2 offsets")
    if pr.size and (pr.min() < 0 or pr.max() >= fo.size - 1):
        raise ValueError(f"pairs must index fragments 0..{fo.size - 2}")
    rows = np.diff(fo)
    out_off = np.concatenate(([0], np.cumsum(rows[pr[:, 0]] + rows[pr[:, 1]]))).astype(np.int64)
    tgt_off = np.concatenate(([0], np.cumsum(rows[pr[:, 1]]))).astype(np.int64)
    host = dict(frag_off=fo, pairs=pr, out_off=out_off, tgt_off=tgt_off)
    dev = {k: torch.from_numpy(v).to(device) for k, v in host.items()}
    return host, dev


def _table_args(host, dev, *names):
    args = []
    for n in names:
        args += [ctypes.c_void_p(host[n].ctypes.data), ctypes.c_void_p(dev[n].data_ptr())]
    return args


def nn_match(feats, frag_off, pairs, valid=None):
    """(feats f[R,C] device, frag_off i64[F+1] host, pairs i32[P,2] host, valid u8/bool [R] device or None) ->
    (nn_idx int32 [out_off[P]], nn_d2 f[out_off[P]], out_off int64 [P+1] host tensor): the exact nearest valid row of the other
    fragment in descriptor space, both directions of every pair in one launch; pair p's block holds its src rows, then its tgt
    rows (epn_nn_match_f32, include/epn_so3conv.h; no counterpart among the reference's extensions -- it replaces the two
    sklearn KDTrees of evaluation_3dmatch.py:77-84)."""
    lib = _lib.get_lib()
    f = _lib.dev_ptr(feats, "feats")
    if feats.dim() != 2 or not 1 <= feats.shape[1] <= 128:
        raise ValueError(f"feats must be [R,C] with 1 <= C <= 128, got {tuple(feats.shape)}")
    if valid is not None:
        _lib.same_device(feats, valid)
        if valid.dtype == torch.bool:
            valid = valid.to(torch.uint8)
        if valid.shape != (feats.shape[0],):
            raise ValueError(f"valid must be [R] = [{feats.shape[0]}], got {tuple(valid.shape)}")
    host, dev = _scene_tables(frag_off, pairs, feats.device)
    n_out, P = int(host["out_off"][-1]), host["pairs"].shape[0]
    nn_idx = torch.empty((n_out,), dtype=torch.int32, device=feats.device)
    nn_d2 = torch.empty((n_out,), dtype=torch.float32, device=feats.device)
    ws_bytes = int(lib.epn_nn_match_workspace_bytes(n_out))
    ws = torch.empty((ws_bytes // 8,), dtype=torch.int64, device=feats.device)
    _lib.check(lib.epn_nn_match_f32(f, feats.shape[0], feats.shape[1], _lib.dev_ptr(valid, "valid", torch.uint8),
                                    host["frag_off"].size - 1, *_table_args(host, dev, "frag_off"), P,
                                    *_table_args(host, dev, "pairs", "out_off"), ctypes.c_void_p(ws.data_ptr()), ws_bytes,
                                    _lib.dev_ptr(nn_idx, "nn_idx", torch.int32), _lib.dev_ptr(nn_d2, "nn_d2"),
                                    _lib.stream_of(feats)), "nn_match")
    return nn_idx, nn_d2, torch.from_numpy(host["out_off"])


def match_inliers(kp_xyz, frag_off, pairs, nn_idx, gt, tau1):
    """(kp_xyz f[R,3] device, frag_off, pairs as for nn_match, nn_idx from nn_match, gt f64 [P,4,4] taking tgt into src
    coordinates, float tau1) -> (match_src int32 [tgt_off[P]], match_dist f64 [tgt_off[P]], n_match int32 [P],
    n_inlier int32 [P], tgt_off int64 [P+1] host tensor): the mutual check tgt -> src -> tgt, the transformed distance in
    fp64 and the counts per pair (epn_match_inliers_f64; replaces evaluation_3dmatch.py:86-100)."""
    lib = _lib.get_lib()
    _lib.same_device(kp_xyz, nn_idx)
    k = _lib.dev_ptr(kp_xyz, "kp_xyz")
    if kp_xyz.dim() != 2 or kp_xyz.shape[1] != 3:
        raise ValueError(f"kp_xyz must be [R,3], got {tuple(kp_xyz.shape)}")
    host, dev = _scene_tables(frag_off, pairs, kp_xyz.device)
    n_out, n_tgt, P = int(host["out_off"][-1]), int(host["tgt_off"][-1]), host["pairs"].shape[0]
    if nn_idx.shape != (n_out,):
        raise ValueError(f"nn_idx must be [{n_out}] for these pairs, got {tuple(nn_idx.shape)}")
    gt = torch.as_tensor(gt, dtype=torch.float64).reshape(-1, 4, 4).contiguous().to(kp_xyz.device)
    if gt.shape[0] != P:
        raise ValueError(f"gt must be [{P},4,4], got {tuple(gt.shape)}")
    match_src = torch.empty((n_tgt,), dtype=torch.int32, device=kp_xyz.device)
    match_dist = torch.empty((n_tgt,), dtype=torch.float64, device=kp_xyz.device)
    n_match = torch.empty((P,), dtype=torch.int32, device=kp_xyz.device)
    n_inlier = torch.empty((P,), dtype=torch.int32, device=kp_xyz.device)
    _lib.check(lib.epn_match_inliers_f64(k, kp_xyz.shape[0], host["frag_off"].size - 1, *_table_args(host, dev, "frag_off"), P,
                                         *_table_args(host, dev, "pairs", "out_off", "tgt_off"),
                                         _lib.dev_ptr(nn_idx, "nn_idx", torch.int32), _lib.dev_ptr(gt, "gt", torch.float64),
                                         float(tau1), _lib.dev_ptr(match_src, "match_src", torch.int32),
                                         _lib.dev_ptr(match_dist, "match_dist", torch.float64),
                                         _lib.dev_ptr(n_match, "n_match", torch.int32),
                                         _lib.dev_ptr(n_inlier, "n_inlier", torch.int32), _lib.stream_of(kp_xyz)), "match_inliers")
    return match_src, match_dist, n_match, n_inlier, torch.from_numpy(host["tgt_off"])


def ransac_register(all_kps, frag_off, pairs, match_src, tgt_off, tau, hypotheses, seed, min_margin, pair0=0):
    """(all_kps f[R,3] device, frag_off, pairs as for nn_match, match_src int32 [tgt_off[P]] and tgt_off from match_inliers,
    float tau, int hypotheses per pair, int seed, float min_margin, int pair0 = the counter word of pairs[0]) ->
    (T f64 [P,4,4], best_h int32 [P], hyp_count int32 [P,H], n_inlier int32 [P], rmse f64 [P], margin f64 [P]), device tensors:
    the rigid transform tgt -> src of every pair by RANSAC over its mutual matches and one refit on the winner's inliers
    (epn_ransac_register_f64, include/epn_so3conv.h; no counterpart in the reference -- the host tool for this step is open3d's
    registration_ransac_based_on_feature_matching)."""
    lib = _lib.get_lib()
    _lib.same_device(all_kps, match_src)
    k = _lib.dev_ptr(all_kps, "all_kps")
    if all_kps.dim() != 2 or all_kps.shape[1] != 3:
        raise ValueError(f"all_kps must be [R,3], got {tuple(all_kps.shape)}")
    H = int(hypotheses)
    if not 1 <= H <= 65536:
        raise ValueError(f"hypotheses must be in 1..65536, got {hypotheses}")
    if not (np.isfinite(tau) and tau > 0.0):
        raise ValueError(f"tau must be finite and > 0, got {tau}")
    if not 0.0 <= min_margin < 1.0:
        raise ValueError(f"min_margin must be in [0, 1), got {min_margin}")
    host, dev = _scene_tables(frag_off, pairs, all_kps.device)
    n_tgt, P = int(host["tgt_off"][-1]), host["pairs"].shape[0]
    if not np.array_equal(np.asarray(tgt_off, dtype=np.int64).reshape(-1), host["tgt_off"]):
        raise ValueError("tgt_off does not belong to these pairs")
    if match_src.shape != (n_tgt,):
        raise ValueError(f"match_src must be [{n_tgt}] for these pairs, got {tuple(match_src.shape)}")
    f64, i32 = dict(dtype=torch.float64, device=all_kps.device), dict(dtype=torch.int32, device=all_kps.device)
    T, best_h, hyp_count = torch.empty((P, 4, 4), **f64), torch.empty((P,), **i32), torch.empty((P, H), **i32)
    n_inlier, rmse, margin = torch.empty((P,), **i32), torch.empty((P,), **f64), torch.empty((P,), **f64)
    ws_bytes = int(lib.epn_ransac_register_workspace_bytes(n_tgt))
    ws = torch.empty((ws_bytes // 8,), dtype=torch.int64, device=all_kps.device)
    _lib.check(lib.epn_ransac_register_f64(k, all_kps.shape[0], host["frag_off"].size - 1, *_table_args(host, dev, "frag_off"), P,
                                           *_table_args(host, dev, "pairs", "tgt_off"),
                                           _lib.dev_ptr(match_src, "match_src", torch.int32), float(tau), H,
                                           int(seed) & (2 ** 64 - 1), int(pair0), float(min_margin),
                                           ctypes.c_void_p(ws.data_ptr()), ws_bytes, _lib.dev_ptr(T, "T", torch.float64),
                                           _lib.dev_ptr(best_h, "best_h", torch.int32),
                                           _lib.dev_ptr(hyp_count, "hyp_count", torch.int32),
                                           _lib.dev_ptr(n_inlier, "n_inlier", torch.int32),
                                           _lib.dev_ptr(rmse, "rmse", torch.float64),
                                           _lib.dev_ptr(margin, "margin", torch.float64), _lib.stream_of(all_kps)),
               "ransac_register")
    return T, best_h, hyp_count, n_inlier, rmse, margin


def initial_anchor_query(centers, xyz, kernel_points, radius, sigma):
    """(centers f[b,3,nc], xyz f[m,3], kernel_points f[ks,na,3], radius, sigma) ->
    [anchor_weights f[b,ks,nc,na], anchor_ctn f[b,ks,nc,na]]  (grouping_cuda.cpp:138-158; KernelPropagation).  float32 or
    float64 after xyz, outputs in the same dtype (dispatch grouping_cuda_kernel.cu:558-563, outputs :149-154)."""
    lib = _lib.get_lib()
    dt = _lib.float_dtype(xyz, "xyz")
    c, x, k = (_lib.dev_ptr(centers, "centers", dt), _lib.dev_ptr(xyz, "xyz", dt),
               _lib.dev_ptr(kernel_points, "kernel_points", dt))
    b, _, nc = centers.shape
    m = xyz.shape[0]
    ks, na = kernel_points.shape[0], kernel_points.shape[1]
    wts = torch.empty((b, ks, nc, na), dtype=dt, device=xyz.device)
    ctn = torch.empty((b, ks, nc, na), dtype=dt, device=xyz.device)
    fn = lib.epn_initial_anchor_query_f64 if dt == torch.float64 else lib.epn_initial_anchor_query_f32
    _lib.check(fn(c, x, k, b, nc, m, na, ks, float(radius), float(sigma), _lib.dev_ptr(wts, "anchor_weights", dt),
                  _lib.dev_ptr(ctn, "anchor_ctn", dt), _lib.stream_of(xyz)), "initial_anchor_query")
    return [wts, ctn]


def anchor_query(sample_idx, grouped_indices, grouped_xyz, anchors, kernel_points, nq):
    """(sample_idx i[b,p], grouped_indices i[b,p,nn], grouped_xyz f[b,3,p,nn], anchors f[na,3], kernel_points f[ks,2],
    int nq) -> [anchor_weights f[b,p,na,ks,nn]]  (grouping_cuda.cpp:88-108; legacy ZPConv).  float32 or float64 after
    grouped_xyz (dispatch grouping_cuda_kernel.cu:505-510).  sample_idx, grouped_indices and nq are checked like the
    reference does (CHECK_INPUT) and otherwise unused, as in its kernel."""
    lib = _lib.get_lib()
    _lib.dev_ptr(sample_idx, "sample_idx", torch.int32)
    _lib.dev_ptr(grouped_indices, "grouped_indices", torch.int32)
    dt = _lib.float_dtype(grouped_xyz, "grouped_xyz")
    g, a, k = (_lib.dev_ptr(grouped_xyz, "grouped_xyz", dt), _lib.dev_ptr(anchors, "anchors", dt),
               _lib.dev_ptr(kernel_points, "kernel_points", dt))
    b, _, p, nn = grouped_xyz.shape
    na, ks = anchors.shape[0], kernel_points.shape[0]
    w = torch.empty((b, p, na, ks, nn), dtype=dt, device=grouped_xyz.device)
    fn = lib.epn_anchor_query_f64 if dt == torch.float64 else lib.epn_anchor_query_f32
    _lib.check(fn(g, a, k, b, p, nn, na, ks, _lib.dev_ptr(w, "anchor_weights", dt), _lib.stream_of(grouped_xyz)),
               "anchor_query")
    return [w]
