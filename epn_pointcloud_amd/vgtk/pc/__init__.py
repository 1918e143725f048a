"""Mirror of vgtk/vgtk/pc: the index-based operators (vgtk/vgtk/pc/sample.py:46-77), load_ply, and the device form of what the
reference's loaders do per sample on the host with this package's uniform_resample_np / rotate_point_cloud and
point3d.normalize_np: radius_patches (3DMatch test loaders), fragment_pair_batch / pack_correspondences (3DMatch training
loader), modelnet_batch / modelnet_alignment_batch / pack_clouds (ModelNet; epn_pointcloud_amd/data.py), and of the keypoint stage
that writes the 3DMatch correspondences (preprocess/run_keypoint.py): PointGrid, fragment_overlap, keypoint_pairs,
scene_keypoint_pairs, transform_points, of the --normals switch: estimate_normals, orient_patches, and of the FPFH descriptor
behind the planar-patch filter and the classical baseline: compute_fpfh_feature, describe_fpfh
(epn_pointcloud_amd/correspondence.py), and of the fusion stage that makes the fragments (preprocess/run_fusion.py): fuse_fragment,
fuse_sequence (epn_pointcloud_amd/fusion.py)."""
from .sample import group_nd, ball_query_index, furthest_sample_index, furthest_sample, radius_patches  # noqa: F401
from .sample import voxel_down_sample, reference_voxel_size  # noqa: F401
from .io import load_ply  # noqa: F401
from ...data import pack_clouds, modelnet_batch, modelnet_alignment_batch  # noqa: F401
from ...data import pack_correspondences, fragment_pair_batch  # noqa: F401
from ...correspondence import PointGrid, KeypointPairs, transform_points, fragment_overlap  # noqa: F401
from ...correspondence import keypoint_pairs, pair_schedule, scene_keypoint_pairs  # noqa: F401
from ...correspondence import PointNormals, estimate_normals, orient_patches  # noqa: F401
from ...correspondence import PointFPFH, compute_fpfh_feature, describe_fpfh  # noqa: F401
from ...fusion import Fragment, TsdfVolume, fuse_fragment, fuse_sequence, fragment_windows, frustum_unit_box  # noqa: F401
