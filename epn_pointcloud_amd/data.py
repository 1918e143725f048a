"""Training batches on the device: what the reference's ModelNet loaders build per sample on the host
(SPConvNets/datasets/modelnet40.py:50-80 Dataloader_ModelNet40.__getitem__ and :115-160 Dataloader_ModelNet40Alignment.__getitem__:
pctk.uniform_resample_np, p3dtk.normalize_np, pctk.rotate_point_cloud, rotation_distance_np, label_relative_rotation_np), as one
launch of csrc/modelnet_batch.hip per batch through the C ABI (epn_modelnet_batch_f32: include/epn_so3conv.h).

The draws are the library's own (Philox keys per (seed, sample id); Shoemake's uniform rotation), so a batch is reproduced from
its seed and ids whatever the order and the batch size, and the call can be captured into a HIP graph.  Inputs are device
tensors; a host tensor raises like every other wrapper of the library (no CPU fallback).  Reading .mat files, the 3DMatch
loader's max_degree Euler augmentation and normals are out of scope."""
import collections

import numpy as np
import torch

from . import _lib

MAX_SAMPLE = 8192           # the selection's limit (one workgroup per cloud), as in vgtk.pc.radius_patches

ModelNetBatch = collections.namedtuple("ModelNetBatch", ["pc", "idx", "R", "R_label", "R_res", "status", "pc_plain"])

STATUS_EMPTY, STATUS_ZERO_EXTENT, STATUS_NONFINITE, STATUS_BAD_OFFSETS = 1, 2, 4, 8


def pack_clouds(clouds, device):
    """list of [n_i,3] arrays or tensors -> (points f32 [M,3], offsets int32 [B+1]) on `device`: the ragged form
    modelnet_batch takes.  Host clouds are concatenated once, together with the offsets, and copied once; device tensors are
    concatenated where they are."""
    if not isinstance(clouds, (list, tuple)):
        raise TypeError(f"clouds must be a list of [n,3] arrays or tensors, got {type(clouds).__name__}")
    for i, c in enumerate(clouds):
        if not isinstance(c, (np.ndarray, torch.Tensor)):
            raise TypeError(f"clouds[{i}] must be a numpy array or a torch tensor, got {type(c).__name__}")
        if c.ndim != 2 or c.shape[1] != 3:
            raise ValueError(f"clouds[{i}] must be [n,3], got {tuple(c.shape)}")
    sizes = [int(c.shape[0]) for c in clouds]
    off = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum(sizes, out=off[1:])
    if off[-1] > 2 ** 31 - 1:
        raise ValueError(f"a batch holds at most 2^31 - 1 points, got {int(off[-1])}")
    off = off.astype(np.int32)
    M = int(off[-1])
    device = torch.device(device)
    if clouds and all(isinstance(c, torch.Tensor) and c.device == device for c in clouds) and device.type != "cpu":
        points = torch.cat([c.to(torch.float32) for c in clouds]).contiguous()
        return points, torch.from_numpy(off).to(device)
    host = np.empty(12 * M + 4 * off.size, dtype=np.uint8)       # the points' bytes, then the offsets': one buffer, one copy
    rows, at = host[:12 * M].view(np.float32), 0
    for c, n in zip(clouds, sizes):
        c = c.detach().cpu().numpy() if isinstance(c, torch.Tensor) else c
        rows[at:at + 3 * n] = np.asarray(c, dtype=np.float32).reshape(-1)
        at += 3 * n
    host[12 * M:].view(np.int32)[:] = off
    buf = torch.from_numpy(host).to(device)                      # both results are views of it: they share one allocation
    return buf[:12 * M].view(torch.float32).view(M, 3), buf[12 * M:].view(torch.int32)


def _rot():
    """vgtk.functional.rotation, on first use: vgtk.pc re-exports this module's functions, so neither imports the other at
    import time."""
    from .vgtk.functional import rotation
    return rotation


def _tensor(t, name, shape, dtype):
    """The check order of vgtk/functional/rotation.py: type, shape, dtype, device -- all from metadata -- then contiguity.
    `shape` entries that are None match any size."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch tensor, got {type(t).__name__}")
    if t.dim() != len(shape) or any(want is not None and got != want for got, want in zip(t.shape, shape)):
        want = "[" + ",".join("*" if s is None else str(s) for s in shape) + "]"
        raise ValueError(f"{name} must have shape {want}, got {tuple(t.shape)}")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")
    return t.contiguous()


def modelnet_batch(points, offsets, n_sample, *, seed=0, ids=None, rotation="random", anchors=None, key_bits=32,
                   return_plain=False):
    """(points f32 [M,3], offsets int32 [B+1], both on the device: pack_clouds) -> ModelNetBatch(pc f32 [B,n_sample,3],
    idx int32 [B,n_sample], R f32 [B,3,3], R_label int32 [B], R_res f32 [B,3,3], status int32 [B], pc_plain f32 [B,n_sample,3]).

    Per cloud: resample to n_sample points, centre on their mean and scale their largest norm to 1, rotate (pc = R p, the
    reference's convention), and label R against the anchors: R_label = arg max_i tr(A_i^T R), R_res = A_label^T R.
    ids int64 [B] on the device (default: the position in the batch) is the sample's identity -- dataset index + epoch *
    dataset length, say: every draw of a cloud depends on (seed, id) only.
    rotation: "random" (uniform on SO(3)), "none" (R = I) or a tensor f32 [B,3,3] that is applied as given.
    anchors f32 [A,3,3], 1 <= A <= 64; without them R_label and R_res are None.  pc_plain (the normalised points before the
    rotation) is None unless return_plain.  status is 0 for a good cloud, else one of 1 (empty), 2 (zero extent), 4 (a
    non-finite coordinate), 8 (offsets descending or out of range): such a cloud's pc, pc_plain and R_res are zeros and its idx
    is -1.  The specification is include/epn_so3conv.h: epn_modelnet_batch_f32."""
    points = _tensor(points, "points", (None, 3), torch.float32)
    offsets = _tensor(offsets, "offsets", (None,), torch.int32)
    if offsets.shape[0] < 1:
        raise ValueError("offsets must hold B + 1 entries, got none")
    B, M = offsets.shape[0] - 1, points.shape[0]
    if M > 2 ** 31 - 1:
        raise ValueError(f"a batch holds at most 2^31 - 1 points, got {M}")
    if ids is not None:
        ids = _tensor(ids, "ids", (B,), torch.int64)
    R_in = None
    if isinstance(rotation, str):
        mode = {"none": 0, "random": 1}.get(rotation)
        if mode is None:
            raise ValueError(f'rotation must be "random", "none" or a [B,3,3] tensor, got {rotation!r}')
    else:
        mode, R_in = 2, _tensor(rotation, "rotation", (B, 3, 3), torch.float32)
    if anchors is not None:
        anchors = _rot().check_anchors(anchors)
    n_sample, key_bits = int(n_sample), int(key_bits)
    if not 1 <= n_sample <= MAX_SAMPLE:
        raise ValueError(f"n_sample must be in 1..{MAX_SAMPLE}, got {n_sample}")
    if not 1 <= key_bits <= 32:
        raise ValueError(f"key_bits must be in 1..32, got {key_bits}")
    _lib.same_device(points, offsets, ids, R_in, anchors)

    dev = points.device
    f32 = dict(dtype=torch.float32, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    pc = torch.empty((B, n_sample, 3), **f32)
    plain = torch.empty((B, n_sample, 3), **f32) if return_plain else None
    idx = torch.empty((B, n_sample), **i32)
    R = torch.empty((B, 3, 3), **f32)
    status = torch.empty((B,), **i32)
    R_label = torch.empty((B,), **i32) if anchors is not None else None
    R_res = torch.empty((B, 3, 3), **f32) if anchors is not None else None
    if B > 0:
        _lib.check(_lib.get_lib().epn_modelnet_batch_f32(
            _lib.dev_ptr(points, "points"), M, _lib.dev_ptr(offsets, "offsets", torch.int32), B,
            _lib.dev_ptr(ids, "ids", torch.int64), n_sample, int(seed) & (2 ** 64 - 1), key_bits, mode,
            _lib.dev_ptr(R_in, "rotation"), _lib.dev_ptr(anchors, "anchors"), 0 if anchors is None else anchors.shape[0],
            _lib.dev_ptr(pc, "pc"), _lib.dev_ptr(plain, "pc_plain"), _lib.dev_ptr(idx, "idx", torch.int32), _lib.dev_ptr(R, "R"),
            _lib.dev_ptr(R_label, "R_label", torch.int32), _lib.dev_ptr(R_res, "R_res"),
            _lib.dev_ptr(status, "status", torch.int32), _lib.stream_of(points)), "modelnet_batch")
    return ModelNetBatch(pc, idx, R, R_label, R_res, status, plain)


def modelnet_alignment_batch(points, offsets, n_sample, anchors, *, seed=0, ids=None):
    """The dictionary of the reference's alignment loader (modelnet40.py:115-160), for a whole batch on the device:
    pc f32 [B,2,n_sample,3] (the rotated source, the plain target), T f32 [B,3,3] (the rotation that was applied),
    R f32 [B,A,3,3] and R_label int32 [B,A] = vgtk.functional.label_relative_rotation(anchors, T); and status int32 [B] as in
    modelnet_batch."""
    points = _tensor(points, "points", (None, 3), torch.float32)       # the order of modelnet_batch: points, offsets, anchors
    offsets = _tensor(offsets, "offsets", (None,), torch.int32)
    anchors = _rot().check_anchors(anchors)
    out = modelnet_batch(points, offsets, n_sample, seed=seed, ids=ids, rotation="random", return_plain=True)
    R, R_label = _rot().label_relative_rotation(anchors, out.R)
    return {"pc": torch.stack((out.pc, out.pc_plain), dim=1), "T": out.R, "R": R, "R_label": R_label, "status": out.status}
