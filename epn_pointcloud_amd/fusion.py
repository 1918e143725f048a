"""TSDF fusion of depth frames into a fragment's surface points on the device: the first stage of the reference's 3DMatch
preprocessing, which it runs on the host with open3d (SPConvNets/datasets/preprocess/run_fusion.py:20-49: a ScalableTSDFVolume
per window of 50 frames, extract_point_cloud, estimate_normals; the settings are preprocess/tool.py:17-27).  The kernels are
csrc/tsdf_fusion.hip, the contract is include/epn_so3conv.h (epn_tsdf_fuse_f32, epn_tsdf_extract_f32):

  fuse_fragment   FusionFromRGBD (:20-49) without colour: depth frames and camera poses -> the fragment's points, in the first
                  frame's coordinates, and that frame's pose
  fuse_sequence   the window loop (:83-98) over a whole sequence

The normals of run_fusion.py:48 are the next stage's: estimate_normals(PointGrid(points, radius), radius, view=(0, 0, 0)) -- a
fused fragment's own origin is a camera position.  The correspondence with open3d is argued from open3d's algorithm, not run
against it.  Inputs on the host are uploaded; there is no CPU fallback."""
import collections
import ctypes
import math

import numpy as np
import torch

from . import _lib

Fragment = collections.namedtuple("Fragment", ["points", "pose_base2world", "n_blocks", "flags", "volume"])
TsdfVolume = collections.namedtuple("TsdfVolume", ["block_unit", "block_mask", "tsdf", "weight", "unit_lo", "unit_dims",
                                                   "n_outside"])

UNIT = 16
MAX_FRAMES = 64
MAX_DIRECTORY = 2 ** 24
MAX_BLOCKS = 2 ** 17
FLAG_OUTSIDE, FLAG_BLOCKS, FLAG_POINTS = 1, 2, 4           # Fragment.flags: the fuse's two bits, the extract's bit shifted up
_FLAGS = ("bit 0: a depth sample touches a unit outside the unit box",
          "bit 1: more units are allocated than max_blocks",
          "bit 2: more surface points than max_points")
_FIRST_POOL = 4096                                         # blocks of the first attempt when max_blocks is None (128 MiB of volume)


def _intrinsic(intrinsic):
    k = np.asarray(intrinsic.cpu() if isinstance(intrinsic, torch.Tensor) else intrinsic, dtype=np.float64)
    if k.shape == (3, 3):
        k = np.array([k[0, 0], k[1, 1], k[0, 2], k[1, 2]])
    if k.shape != (4,):
        raise ValueError(f"intrinsic must be (fx, fy, cx, cy) or a 3 x 3 matrix, got shape {k.shape}")
    fx, fy, cx, cy = (float(v) for v in k)
    if not (np.isfinite(k).all() and fx > 0 and fy > 0):
        raise ValueError(f"intrinsic must be finite with fx, fy > 0, got {k.tolist()}")
    return fx, fy, cx, cy


def _depth(depth, device):
    """-> a contiguous device tensor [F,H,W] whose 16-bit elements are the raw depths (dtype uint16 or int16: the bits count)."""
    if isinstance(depth, np.ndarray):
        if depth.dtype != np.uint16:
            raise TypeError(f"a numpy depth must be uint16, got {depth.dtype}")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        t = torch.from_numpy(np.ascontiguousarray(depth).view(np.int16)).to(device)
    elif isinstance(depth, torch.Tensor):
        if not depth.is_cuda:
            raise RuntimeError("depth must be a CUDA tensor (or a numpy uint16 array)")
        if depth.dtype == torch.uint16:
            t = depth.contiguous()
        elif depth.dtype == torch.int16:
            if depth.numel() and int(depth.min()) < 0:
                raise ValueError("depth (int16) holds a negative value; raw depths are 0..65535")
            t = depth.contiguous()
        elif depth.dtype == torch.int32:
            if depth.numel() and (int(depth.min()) < 0 or int(depth.max()) > 65535):
                raise ValueError("depth (int32) holds a value outside 0..65535")
            t = (depth - ((depth >= 32768).to(torch.int32) << 16)).to(torch.int16).contiguous()     # the same low 16 bits
        else:
            raise TypeError(f"depth must be uint16, int16 or int32, got {depth.dtype}")
    else:
        raise TypeError(f"depth must be a device tensor or a numpy uint16 array, got {type(depth).__name__}")
    if t.dim() != 3 or 0 in t.shape:
        raise ValueError(f"depth must be [F,H,W] with no empty dimension, got {tuple(t.shape)}")
    return t


def relative_poses(cam2world):
    """cam2world [F,4,4] -> (cam2base f64 [F,4,4], base2cam f64 [F,4,4], pose_base2world f64 [4,4]) on the host: the first pose
    is the fragment's frame, cam2base[f] = inv(pose[0]) @ pose[f] (run_fusion.py:33-40) and base2cam its inverse (:45)."""
    p = np.asarray(cam2world.cpu() if isinstance(cam2world, torch.Tensor) else cam2world, dtype=np.float64)
    if p.ndim != 3 or p.shape[1:] != (4, 4) or p.shape[0] < 1:
        raise ValueError(f"cam2world must be [F,4,4], got {p.shape}")
    if not np.isfinite(p).all():
        raise ValueError("cam2world holds a non-finite entry")
    cam2base = np.linalg.inv(p[0])[None] @ p
    return np.ascontiguousarray(cam2base), np.ascontiguousarray(np.linalg.inv(cam2base)), p[0].copy()


def frustum_unit_box(cam2base, intrinsic, H, W, depth_trunc, voxel_length, sdf_trunc):
    """-> (unit_lo [3], unit_dims [3]) ints: a box of units that holds every unit a sample of these frames can touch.  A sample
    of frame f is cam2base[f] applied to ((u - cx) d / fx, (v - cy) d / fy, d) with 0 <= u <= W - 1, 0 <= v <= H - 1 and 0 < d <=
    depth_trunc: it lies in the pyramid spanned by the camera centre and the four image corners at depth_trunc, so the box of those
    five points per frame, widened by sdf_trunc and by one unit on every side for the roundings, holds its +- sdf_trunc box."""
    fx, fy, cx, cy = intrinsic
    unit_length = UNIT * float(voxel_length)
    d = float(depth_trunc)
    corners = np.array([[0.0, 0.0, 0.0, 1.0]] + [[(u - cx) * d / fx, (v - cy) * d / fy, d, 1.0]
                                                 for u in (0.0, W - 1.0) for v in (0.0, H - 1.0)])
    pts = np.einsum("fij,kj->fki", np.asarray(cam2base, dtype=np.float64), corners)[..., :3].reshape(-1, 3)
    lo = np.floor((pts.min(axis=0) - sdf_trunc) / unit_length).astype(np.int64) - 1
    hi = np.floor((pts.max(axis=0) + sdf_trunc) / unit_length).astype(np.int64) + 1
    return [int(v) for v in lo], [int(v) for v in hi - lo + 1]


def tsdf_fuse(depth, cam2base, base2cam, intrinsic, unit_lo, unit_dims, max_blocks, *, depth_scale=1000.0, depth_trunc=6.0,
              voxel_length=3.0 / 512, sdf_trunc=0.04, stride=4, out=None):
    """The C entry on tensors: depth [F,H,W] (16-bit, device), cam2base / base2cam f64 [F,4,4] (device) -> (block_unit int32
    [max_blocks,3], block_mask int64 [max_blocks] (the bits of the u64), tsdf f32 [max_blocks,16,16,16], weight int32 alike,
    status int32 [4] = {n_blocks, flags, n_outside, 0}, workspace): epn_tsdf_fuse_f32.  Nothing is read back.  out: the four
    volume tensors to write into (rows past min(n_blocks, max_blocks) are left as they are)."""
    lib = _lib.get_lib()
    F, H, W = depth.shape
    fx, fy, cx, cy = intrinsic
    dev = depth.device
    i32 = dict(dtype=torch.int32, device=dev)
    mb = int(max_blocks)
    if out is None:
        out = (torch.empty((mb, 3), **i32), torch.empty((mb,), dtype=torch.int64, device=dev),
               torch.empty((mb, UNIT, UNIT, UNIT), dtype=torch.float32, device=dev), torch.empty((mb, UNIT, UNIT, UNIT), **i32))
    block_unit, block_mask, tsdf, weight = out
    status = torch.empty((4,), **i32)
    ws_bytes = int(lib.epn_tsdf_fuse_workspace_bytes(F, H, W, int(stride), *unit_dims, mb))
    if ws_bytes == 0:
        raise ValueError(f"tsdf_fuse: F = {F} (1..{MAX_FRAMES}), image {H} x {W}, stride {stride}, unit box {list(unit_dims)} (product <= "
                         f"2^24) or max_blocks = {mb} (1..2^17) is out of range")
    ws = torch.empty((ws_bytes // 8,), dtype=torch.int64, device=dev)
    _lib.same_device(depth, cam2base, base2cam, block_unit, block_mask, tsdf, weight)
    _lib.check(lib.epn_tsdf_fuse_f32(_lib.dev_ptr(depth, "depth", depth.dtype), F, H, W,
                                     _lib.dev_ptr(cam2base, "cam2base", torch.float64),
                                     _lib.dev_ptr(base2cam, "base2cam", torch.float64), fx, fy, cx, cy, float(depth_scale),
                                     float(depth_trunc), float(voxel_length), float(sdf_trunc), int(stride), *unit_lo, *unit_dims, mb,
                                     _lib.dev_ptr(block_unit, "block_unit", torch.int32),
                                     _lib.dev_ptr(block_mask, "block_mask", torch.int64), _lib.dev_ptr(tsdf, "tsdf"),
                                     _lib.dev_ptr(weight, "weight", torch.int32), _lib.dev_ptr(status, "status", torch.int32),
                                     ctypes.c_void_p(ws.data_ptr()), ws.numel() * 8, _lib.stream_of(depth)), "tsdf_fuse")
    return block_unit, block_mask, tsdf, weight, status, ws


def tsdf_extract(tsdf, weight, block_unit, workspace, unit_lo, unit_dims, voxel_length, max_points, points=None):
    """The volume and workspace of tsdf_fuse -> (points f32 [max_points,3] or None with max_points == 0, status int32 [2] = {M,
    flags}): epn_tsdf_extract_f32.  Nothing is read back; rows past min(M, max_points) are left as they are."""
    lib = _lib.get_lib()
    dev = tsdf.device
    mp = int(max_points)
    if points is None and mp > 0:
        points = torch.empty((mp, 3), dtype=torch.float32, device=dev)
    status = torch.empty((2,), dtype=torch.int32, device=dev)
    _lib.same_device(tsdf, weight, block_unit, workspace, points)
    _lib.check(lib.epn_tsdf_extract_f32(_lib.dev_ptr(tsdf, "tsdf"), _lib.dev_ptr(weight, "weight", torch.int32),
                                        _lib.dev_ptr(block_unit, "block_unit", torch.int32), tsdf.shape[0], *unit_lo, *unit_dims,
                                        float(voxel_length), _lib.dev_ptr(points, "points"), mp,
                                        _lib.dev_ptr(status, "status", torch.int32), ctypes.c_void_p(workspace.data_ptr()),
                                        workspace.numel() * 8, _lib.stream_of(tsdf)), "tsdf_extract")
    return points, status


def _raise_flags(flags, what):
    raise ValueError(f"fuse_fragment: status " + "; ".join(t for b, t in enumerate(_FLAGS) if flags >> b & 1) + f" (flags = {flags}; {what})")


def fuse_fragment(depth, cam2world, intrinsic, *, depth_scale=1000, depth_trunc=6.0, voxel_length=3.0 / 512, sdf_trunc=0.04,
                  stride=4, max_blocks=None, max_points=None, return_volume=False, device=None):
    """(depth [F,H,W]: a device tensor of uint16, int16 or int32 in 0..65535, or a numpy uint16 array; cam2world [F,4,4];
    intrinsic (fx, fy, cx, cy) or 3 x 3; 1 <= F <= 64) -> Fragment(points f32 [M,3] in the first frame's coordinates,
    pose_base2world f64 [4,4] (numpy: the first frame's pose), n_blocks, flags = 0, volume): the reference's FusionFromRGBD
    (run_fusion.py:20-49) without colour and without normals.  The unit box is the frames' frusta out to depth_trunc
    (frustum_unit_box).  max_blocks None: a first attempt with 4096 blocks, repeated once with the number the device reports when
    that was too few; max_points None: the extract is run once to count and once to write.  Any flag left raises ValueError
    with its meaning, as vgtk.pc.voxel_down_sample does.  volume (with return_volume) is TsdfVolume(block_unit int32 [n,3],
    block_mask int64 [n] (the u64's bits), tsdf f32 [n,16,16,16], weight int32 alike, unit_lo, unit_dims, n_outside).  The status
    words are read back: two or three host synchronisations per fragment."""
    vl, st, dtr, dsc, strd = float(voxel_length), float(sdf_trunc), float(depth_trunc), float(depth_scale), int(stride)
    for name, v in (("depth_scale", dsc), ("depth_trunc", dtr), ("voxel_length", vl), ("sdf_trunc", st)):
        if not (math.isfinite(v) and v > 0.0):
            raise ValueError(f"{name} must be finite and > 0, got {v}")
    if st > 8.0 * vl:
        raise ValueError(f"sdf_trunc must not exceed 8 voxel_length = {8.0 * vl} (a sample touches at most 2 units per axis), got {st}")
    if strd < 1:
        raise ValueError(f"stride must be >= 1, got {stride}")
    K = _intrinsic(intrinsic)
    depth = _depth(depth, device)
    F, H, W = depth.shape
    if not 1 <= F <= MAX_FRAMES:
        raise ValueError(f"a fragment takes 1..{MAX_FRAMES} frames, got {F}")
    cam2base, base2cam, pose = relative_poses(cam2world)
    if cam2base.shape[0] != F:
        raise ValueError(f"cam2world must hold the {F} poses of the depth frames, got {cam2base.shape[0]}")
    lo, dims = frustum_unit_box(cam2base, K, H, W, dtr, vl, st)
    D = dims[0] * dims[1] * dims[2]
    if D > MAX_DIRECTORY:
        raise ValueError(f"the frusta of these frames span {dims} units, more than 2^24: lower depth_trunc or raise voxel_length")
    c2b, b2c = torch.from_numpy(cam2base).to(depth.device), torch.from_numpy(base2cam).to(depth.device)
    kw = dict(depth_scale=dsc, depth_trunc=dtr, voxel_length=vl, sdf_trunc=st, stride=strd)
    mb = min(D, _FIRST_POOL) if max_blocks is None else int(max_blocks)
    block_unit, block_mask, tsdf, weight, status, ws = tsdf_fuse(depth, c2b, b2c, K, lo, dims, mb, **kw)
    n_blocks, flags, n_outside, _ = status.tolist()
    if flags & FLAG_BLOCKS and max_blocks is None and n_blocks <= MAX_BLOCKS:
        mb = n_blocks
        block_unit, block_mask, tsdf, weight, status, ws = tsdf_fuse(depth, c2b, b2c, K, lo, dims, mb, **kw)
        n_blocks, flags, n_outside, _ = status.tolist()
    if flags:
        _raise_flags(flags, f"n_blocks = {n_blocks}, max_blocks = {mb}, samples outside the box = {n_outside}, box = {lo} + {dims}")
    if max_points is None:
        max_points = tsdf_extract(tsdf, weight, block_unit, ws, lo, dims, vl, 0)[1].tolist()[0]
    points, xstatus = tsdf_extract(tsdf, weight, block_unit, ws, lo, dims, vl, int(max_points))
    m, xflags = xstatus.tolist()
    if xflags:
        _raise_flags(FLAG_POINTS, f"M = {m}, max_points = {max_points}")
    if points is None:
        points = torch.empty((0, 3), dtype=torch.float32, device=depth.device)
    volume = TsdfVolume(block_unit[:n_blocks], block_mask[:n_blocks], tsdf[:n_blocks], weight[:n_blocks], lo, dims,
                        n_outside) if return_volume else None
    return Fragment(points[:m], pose, n_blocks, 0, volume)


def fragment_windows(n_frames, frames_per_frag=50):
    """[(head, tail)]: the reference's window loop (run_fusion.py:84-98): whole windows of frames_per_frag frames, a trailing
    partial window dropped -- except that a sequence shorter than one window is fused as its single fragment."""
    n, k = int(n_frames), int(frames_per_frag)
    if k < 1:
        raise ValueError(f"frames_per_frag must be >= 1, got {frames_per_frag}")
    out, head, tail = [], 0, min(k, n)
    while tail <= n and tail > head:
        out.append((head, tail))
        head, tail = tail, tail + k
    return out


def fuse_sequence(depth, cam2world, intrinsic, frames_per_frag=50, **kw):
    """(depth [N,H,W], cam2world [N,4,4]) -> [Fragment]: fuse_fragment over the windows of fragment_windows(N, frames_per_frag)."""
    if len(depth) != len(cam2world):
        raise ValueError(f"{len(depth)} depth frames but {len(cam2world)} poses")
    return [fuse_fragment(depth[h:t], cam2world[h:t], intrinsic, **kw) for h, t in fragment_windows(len(depth), frames_per_frag)]
