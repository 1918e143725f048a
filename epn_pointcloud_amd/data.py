"""Training batches on the device: what the reference's ModelNet loaders build per sample on the host
(SPConvNets/datasets/modelnet40.py:50-80 Dataloader_ModelNet40.__getitem__ and :115-160 Dataloader_ModelNet40Alignment.__getitem__:
pctk.uniform_resample_np, p3dtk.normalize_np, pctk.rotate_point_cloud, rotation_distance_np, label_relative_rotation_np), as one
launch of csrc/modelnet_batch.hip per batch through the C ABI (epn_modelnet_batch_f32: include/epn_so3conv.h);
and what its 3DMatch loader builds per fragment pair (SPConvNets/datasets/match_3dmatch.py:301-354 FragmentLoader.__getitem__:
the keypoint draw, the radius patches of both fragments, their resampling, the max_degree Euler augmentation and T), as one
launch of csrc/pair_batch.hip per batch (epn_fragment_pair_batch_f32).

The draws are the library's own (Philox keys per (seed, sample id); Shoemake's uniform rotation), so a batch is reproduced from
its seed and ids whatever the order and the batch size, and the call can be captured into a HIP graph.  Inputs are device
tensors; a host tensor raises like every other wrapper of the library (no CPU fallback).  Reading .mat, .ply and .npy files and normals are out of
scope."""
import collections

import numpy as np
import torch

from . import _lib

MAX_SAMPLE = 8192           # the selection's limit (one workgroup per cloud), as in vgtk.pc.radius_patches

ModelNetBatch = collections.namedtuple("ModelNetBatch", ["pc", "idx", "R", "R_label", "R_res", "status", "pc_plain"])

FragmentPairBatch = collections.namedtuple("FragmentPairBatch", ["src", "tgt", "idx", "counts", "choice", "T", "R_aug", "T_aug",
                                                                 "status"])

STATUS_EMPTY, STATUS_ZERO_EXTENT, STATUS_NONFINITE, STATUS_BAD_OFFSETS = 1, 2, 4, 8
MAX_NPT, MAX_ID = 4096, 2 ** 40     # fragment_pair_batch: keypoints per sample; ids below MAX_ID keep (id * 2 + s) * npt + j exact


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


def pack_correspondences(corrs, device):
    """list of [P_b,2,3] arrays or tensors -> (corr f32 [C,2,3], corr_offsets int32 [B+1]) on `device`: the ragged form
    fragment_pair_batch takes.  Entry [:,0] is a keypoint in the source fragment's frame, [:,1] its match in the target's
    (the reference: np.stack((rawA[k[:,0]], rawB[k[:,1]]), 1)).  One buffer, one copy, as in pack_clouds."""
    if not isinstance(corrs, (list, tuple)):
        raise TypeError(f"corrs must be a list of [P,2,3] arrays or tensors, got {type(corrs).__name__}")
    for i, c in enumerate(corrs):
        if not isinstance(c, (np.ndarray, torch.Tensor)):
            raise TypeError(f"corrs[{i}] must be a numpy array or a torch tensor, got {type(c).__name__}")
        if c.ndim != 3 or tuple(c.shape[1:]) != (2, 3):
            raise ValueError(f"corrs[{i}] must be [P,2,3], got {tuple(c.shape)}")
    sizes = [int(c.shape[0]) for c in corrs]
    off = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum(sizes, out=off[1:])
    if off[-1] > 2 ** 31 - 1:
        raise ValueError(f"a batch holds at most 2^31 - 1 correspondences, got {int(off[-1])}")
    C = int(off[-1])
    host = np.empty(24 * C + 4 * off.size, dtype=np.uint8)       # the coordinates' bytes, then the offsets'
    vals, at = host[:24 * C].view(np.float32), 0
    for c, n in zip(corrs, sizes):
        c = c.detach().cpu().numpy() if isinstance(c, torch.Tensor) else c
        vals[at:at + 6 * n] = np.asarray(c, dtype=np.float32).reshape(-1)
        at += 6 * n
    host[24 * C:].view(np.int32)[:] = off
    buf = torch.from_numpy(host).to(torch.device(device))        # both results are views of it: they share one allocation
    return buf[:24 * C].view(torch.float32).view(C, 2, 3), buf[24 * C:].view(torch.int32)


def _rot():
    """vgtk.functional.rotation, on first use: vgtk.pc re-exports this module's functions, so neither imports the other at
    import time."""
    from .vgtk.functional import rotation
    return rotation


def _tensor(t, name, shape, dtype):
    """The check order of vgtk/functional/rotation.py: type, shape, dtype, device -- all from metadata -- then contiguity.
    `shape` entries that are None match any size; `dtype` may be a tuple of accepted dtypes."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch tensor, got {type(t).__name__}")
    if t.dim() != len(shape) or any(want is not None and got != want for got, want in zip(t.shape, shape)):
        want = "[" + ",".join("*" if s is None else str(s) for s in shape) + "]"
        raise ValueError(f"{name} must have shape {want}, got {tuple(t.shape)}")
    if t.dtype not in (dtype if isinstance(dtype, tuple) else (dtype,)):
        want = " or ".join(str(d) for d in dtype) if isinstance(dtype, tuple) else dtype
        raise TypeError(f"{name} must be {want}, got {t.dtype}")
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


def fragment_pair_batch(points, offsets, pairs, corr, corr_offsets, poses, n_sample, npt, radius, *, seed=0, ids=None,
                        max_degree=30, center=False, key_bits=32):
    """The batch of the reference's 3DMatch training loader (match_3dmatch.py:301-354 FragmentLoader.__getitem__) in one launch:
    (points f32 [M,3], offsets int32 [F+1]: the F downsampled fragments, pack_clouds of vgtk.pc.voxel_down_sample outputs;
    pairs int32 [B,2]: source and target fragment of each sample; corr f32 [C,2,3], corr_offsets int32 [B+1]: the samples'
    keypoint correspondences as coordinates, pack_correspondences; poses f32 or f64 [F,4,4]) -> FragmentPairBatch(src, tgt f32
    [B,npt,n_sample,3], idx int32 [B,2,npt,n_sample], counts int32 [B,2,npt], choice int32 [B,npt], T f32 [B,3,3], R_aug f32
    [B,2,3,3], T_aug f32 [B,3,3], status int32 [B]).

    Per sample: npt correspondences drawn with replacement (choice), the radius patch around each keypoint in both fragments
    resampled to n_sample points by the rule of vgtk.pc.radius_patches (idx, counts), one Euler rotation per side with integer
    degrees below max_degree (R_aug; max_degree = 0 is the reference's no_augmentation), src / tgt = R_aug (p - center * keypoint),
    T = R_A^T R_B from the poses (what the reference returns) and T_aug = R_aug_src T R_aug_tgt^T, the relation the augmented
    patches satisfy.  ids int64 [B] on the device (default: the position in the batch), 0 <= id < 2^40: every draw of a sample
    depends on (seed, id, npt) only.  status is 0 for a good sample, else 8 (pairs / offsets / corr_offsets out of range), 1 (no
    correspondences) or 4 (a non-finite pose or chosen keypoint): such a sample's src, tgt, T and T_aug are zeros, its idx and
    choice -1, its counts 0.  An empty patch shows in counts.  The specification is include/epn_so3conv.h:
    epn_fragment_pair_batch_f32."""
    points = _tensor(points, "points", (None, 3), torch.float32)
    offsets = _tensor(offsets, "offsets", (None,), torch.int32)
    if offsets.shape[0] < 1:
        raise ValueError("offsets must hold F + 1 entries, got none")
    F, M = offsets.shape[0] - 1, points.shape[0]
    pairs = _tensor(pairs, "pairs", (None, 2), torch.int32)
    B = pairs.shape[0]
    corr = _tensor(corr, "corr", (None, 2, 3), torch.float32)
    corr_offsets = _tensor(corr_offsets, "corr_offsets", (B + 1,), torch.int32)
    poses = _tensor(poses, "poses", (F, 4, 4), (torch.float64, torch.float32)).to(torch.float64)
    if ids is not None:
        ids = _tensor(ids, "ids", (B,), torch.int64)
    C = corr.shape[0]
    if max(M, C) > 2 ** 31 - 1:
        raise ValueError(f"a batch holds at most 2^31 - 1 points and correspondences, got {M} and {C}")
    n_sample, npt, key_bits, max_degree, radius = int(n_sample), int(npt), int(key_bits), int(max_degree), float(radius)
    if not 1 <= n_sample <= MAX_SAMPLE:
        raise ValueError(f"n_sample must be in 1..{MAX_SAMPLE}, got {n_sample}")
    if not 1 <= npt <= MAX_NPT:
        raise ValueError(f"npt must be in 1..{MAX_NPT}, got {npt}")
    if B * 2 * npt > 2 ** 31 - 1:
        raise ValueError(f"B * 2 * npt must stay below 2^31, got {B} * 2 * {npt}")
    if not (np.isfinite(radius) and radius > 0.0):
        raise ValueError(f"radius must be finite and positive, got {radius}")
    if not 0 <= max_degree <= 360:
        raise ValueError(f"max_degree must be in 0..360, got {max_degree}")
    if not 1 <= key_bits <= 32:
        raise ValueError(f"key_bits must be in 1..32, got {key_bits}")
    _lib.same_device(points, offsets, pairs, corr, corr_offsets, poses, ids)

    dev = points.device
    f32 = dict(dtype=torch.float32, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    out = FragmentPairBatch(torch.empty((B, npt, n_sample, 3), **f32), torch.empty((B, npt, n_sample, 3), **f32),
                            torch.empty((B, 2, npt, n_sample), **i32), torch.empty((B, 2, npt), **i32),
                            torch.empty((B, npt), **i32), torch.empty((B, 3, 3), **f32), torch.empty((B, 2, 3, 3), **f32),
                            torch.empty((B, 3, 3), **f32), torch.empty((B,), **i32))
    if B > 0:
        i32p = lambda t, name: _lib.dev_ptr(t, name, torch.int32)
        _lib.check(_lib.get_lib().epn_fragment_pair_batch_f32(
            _lib.dev_ptr(points, "points"), M, i32p(offsets, "offsets"), F, i32p(pairs, "pairs"), B, _lib.dev_ptr(corr, "corr"), C,
            i32p(corr_offsets, "corr_offsets"), _lib.dev_ptr(poses, "poses", torch.float64), _lib.dev_ptr(ids, "ids", torch.int64),
            n_sample, npt, radius, int(seed) & (2 ** 64 - 1), key_bits, max_degree, int(bool(center)),
            _lib.dev_ptr(out.src, "src"), _lib.dev_ptr(out.tgt, "tgt"), i32p(out.idx, "idx"), i32p(out.counts, "counts"),
            i32p(out.choice, "choice"), _lib.dev_ptr(out.T, "T"), _lib.dev_ptr(out.R_aug, "R_aug"), _lib.dev_ptr(out.T_aug, "T_aug"),
            i32p(out.status, "status"), _lib.stream_of(points)), "fragment_pair_batch")
    return out
