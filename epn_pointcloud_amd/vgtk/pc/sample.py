"""Index-based point-cloud operators (vgtk/vgtk/pc/sample.py:46-77)."""
import torch

from ..cuda import grouping as cuda_nn
from .. import utils


def group_nd(pc, idx):
    """[b,c,n] x [b,m1(,m2,...)] -> [b,c,m1(,m2,...)]   (sample.py:46-50)"""
    b = idx.shape[0]
    pc = utils.batch_gather(pc, idx.view(b, -1).contiguous(), dim=2)
    return pc.view(b, -1, *idx.shape[1:])


def ball_query_index(query_points, support_points, radius, n_sample):
    """[b,3,m] x [b,3,n] -> int32 [b,m,k]   (sample.py:54-59)"""
    return cuda_nn.ball_query(query_points, support_points, radius, n_sample)


def radius_patches(pc, keypoints, radius, n_sample, *, seed=0, center=False, scale=1.0, rows_per_call=None,
                   normals=None):
    """[n,3] x keypoints -> (patches f[k,n_sample,3], idx int32 [k,n_sample], counts int32 [k]): around every keypoint,
    the points of the fragment within `radius`, resampled to n_sample.  The device form of what the reference does on the
    host with a KD-tree and np.random.choice (match_3dmatch.py:154-177, sample.py:16-36), in the library's deterministic
    statement of it (include/epn_so3conv.h: epn_radius_patches_f32): rows with counts <= 1 are idx -1 / zero patches.
    keypoints: float [k,3] coordinates, or an integer [k] tensor of rows of pc (what the reference passes).
    rows_per_call splits the keypoints over several launches; the result is the same by specification.
    normals f32 [k,3], the fragment's normals at the keypoints: every patch is turned into its keypoint's normal frame
    (orient_patches, in place on the result), what the reference's loader does with return_normals (match_3dmatch.py:136-137)."""
    if not keypoints.is_floating_point():
        if keypoints.dim() != 1:
            raise ValueError(f"integer keypoints must be [k] rows of pc, got {tuple(keypoints.shape)}")
        keypoints = pc.index_select(0, keypoints.long())
    keypoints = keypoints.contiguous()
    k = keypoints.shape[0]
    if normals is not None and (not isinstance(normals, torch.Tensor) or tuple(normals.shape) != (k, 3)):
        raise ValueError(f"normals must be a [k,3] = [{k},3] tensor, one normal per keypoint, got "
                         f"{tuple(normals.shape) if isinstance(normals, torch.Tensor) else type(normals).__name__}")
    step = k if rows_per_call is None else int(rows_per_call)
    if rows_per_call is not None and step < 1:
        raise ValueError(f"rows_per_call must be >= 1, got {rows_per_call}")
    if step >= k:
        idx, counts, patches = cuda_nn.radius_patches(pc, keypoints, radius, n_sample, seed=seed, center=center, scale=scale)
    else:
        parts = [cuda_nn.radius_patches(pc, keypoints[r0:r0 + step], radius, n_sample, seed=seed, kpt_row0=r0, center=center,
                                        scale=scale) for r0 in range(0, k, step)]
        idx, counts, patches = (torch.cat([p[i] for p in parts]) for i in range(3))
    if normals is not None:
        cuda_nn.orient_patches(patches, normals, out=patches)
    return patches, idx, counts


def voxel_down_sample(pc, voxel_size):
    """[n,3] -> (centroids f[M,3], counts int32 [M], first_idx int32 [M], point_voxel int32 [n]): the centroid of every
    occupied voxel of edge voxel_size, on the device.  What the reference does on the host with open3d before it searches a
    fragment (pcd.voxel_down_sample, match_3dmatch.py:107-139), in the library's deterministic statement of it
    (include/epn_so3conv.h: epn_voxel_downsample_f32): voxels in ascending order of their lowest point index, points with a
    non-finite coordinate dropped (point_voxel -1), a cloud out of range raises ValueError."""
    return cuda_nn.voxel_downsample(pc.contiguous(), voxel_size)


def reference_voxel_size(input_num):
    """The voxel size the reference's 3DMatch loaders downsample a fragment with before extracting patches of input_num
    points (match_3dmatch.py:258, :371, :445)."""
    return 0.03 if input_num < 1024 else 0.015


def furthest_sample_index(pc, n_sample, lazy_sample):
    """sample.py:63-72: arange when nothing is dropped or lazy_sample, FPS kernel otherwise."""
    if pc.shape[2] == n_sample or lazy_sample:
        nb = pc.shape[0]
        return torch.arange(n_sample, dtype=torch.int32, device=pc.device).view(1, -1).expand(nb, -1).contiguous()
    return cuda_nn.furthest_point_sampling(pc, n_sample)


def furthest_sample(pc, n_sample, lazy_sample=True):
    """[b,3,n] -> ([b,m] int32, [b,3,m])   (sample.py:75-77)"""
    idx = furthest_sample_index(pc, n_sample, lazy_sample)
    return idx, group_nd(pc, idx)
