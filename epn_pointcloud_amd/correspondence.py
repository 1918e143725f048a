"""Keypoint correspondences of 3DMatch fragment pairs on the device: what the reference computes on the host, once per dataset,
with sklearn trees and open3d (SPConvNets/datasets/preprocess/run_keypoint.py) and stores as the cloud_bin_i-cloud_bin_j.npy
files its training loader reads (SPConvNets/datasets/match_3dmatch.py:233-304).  Every step is one primitive, the nearest point
of a cloud within a bound, served by a hashed grid (csrc/point_grid.hip; include/epn_so3conv.h: epn_point_grid_build_f32,
epn_point_grid_nn_f32):

  fragment_overlap      test_scenes_overlap (:98-112): how many source points have a target point within the margin
  keypoint_pairs        generate_kp (:114-141): downsample both fragments, drop isolated centroids, match the rest across the
                        fragments, map every matched centroid back to a raw row
  scene_keypoint_pairs  run_KeypointSelection's pair schedule (:162-185) over the fragments of one scene

The clouds are in the WORLD frame (transform_points applies a pose); inputs are device tensors, and a host tensor raises like
every other wrapper of the library (no CPU fallback).  With the reference's default nonplanar_param = -1 the FPFH descriptor is
not computed: all cross_filtering_via_fpfh then uses of it is whether it is zero (:58-59), and in open3d's algorithm a point's
descriptor is zero exactly when no other point of its cloud lies within the FPFH radius -- the isolation filter below
(tests/test_fpfh_spec.py holds the FPFH of this package to that).  With nonplanar_param > 0 the descriptor is computed
(compute_fpfh_feature: csrc/fpfh.hip, epn_point_fpfh_f32) and the planar-patch filter (:77-92) runs on it.
describe_fpfh is the same descriptor at a fragment's keypoints, the classical baseline of the 3DMatch tables.  All of this is
argued from open3d's algorithm, not run against it."""
import collections
import math

import torch

from . import _lib
from .data import _tensor

KeypointPairs = collections.namedtuple("KeypointPairs", ["rows", "src_centroid_row", "d2"])
PointNormals = collections.namedtuple("PointNormals", ["normals", "eig", "count", "flags", "moments", "neighbors"])
PointFPFH = collections.namedtuple("PointFPFH", ["features", "count", "flags", "spfh"])


def _grouping():
    """vgtk.cuda.grouping, on first use: vgtk.pc re-exports this module's functions, so neither imports the other at import
    time."""
    from .vgtk.cuda import grouping
    return grouping


def transform_points(pc, T):
    """(pc f[n,3], T [4,4]) -> f32 [n,3]: R p + t, computed in fp64 and rounded once (the reference transforms with open3d, in
    fp64, before it searches: run_keypoint.py:118, :166)."""
    T = torch.as_tensor(T, dtype=torch.float64, device=pc.device)
    if T.shape != (4, 4):
        raise ValueError(f"T must be [4,4], got {tuple(T.shape)}")
    return (pc.to(torch.float64) @ T[:3, :3].T + T[:3, 3]).to(torch.float32)


class PointGrid:
    """The grid of one cloud: PointGrid(points f32 [n,3], max_radius, valid=None) builds it (seven launches) and owns its
    workspace; .nearest() answers any radius up to max_radius.  Points with a non-finite coordinate, and those whose `valid`
    byte is zero, are never an answer.  The status word is read back once; a range error raises ValueError naming its bit, as
    vgtk.pc.voxel_down_sample does."""

    def __init__(self, points, max_radius, valid=None):
        self.points = _tensor(points, "points", (None, 3), torch.float32)
        self.n = self.points.shape[0]
        self.max_radius = float(max_radius)
        grouping = _grouping()
        self._workspace, status = grouping.point_grid_build(self.points, self.max_radius, valid)
        self.kept = 0
        if status is not None:
            self.kept, flags = status.tolist()
            if flags:
                raise ValueError("PointGrid: status " + "; ".join(t for b, t in enumerate(grouping._VOXEL_FLAGS) if flags >> b & 1)
                                 + f" (flags = {flags}, max_radius = {self.max_radius})")

    def nearest(self, queries, radius, exclude_self=False, count=False):
        """queries f32 [m,3] -> (idx int32 [m], d2 f32 [m][, hits int32 [1]]): the row of the nearest point within radius (the
        smallest fp32 squared distance, the lowest row on a tie) and that distance, -1 and +inf without one.  exclude_self: the
        queries are the grid's own points, and each skips its own row (a duplicate at another row is still found).  count: also
        the number of queries that found a point, on the device."""
        if not float(radius) <= self.max_radius:
            raise ValueError(f"radius must not exceed the grid's max_radius {self.max_radius}, got {radius}")
        return _grouping().point_grid_nn(self._workspace, self.n, queries, radius, exclude_row=exclude_self, count=count)

    def normals(self, queries=None, radius=None, max_nn=30, view=None, return_moments=False, return_neighbors=False):
        """queries f32 [m,3] (None: the grid's own points) -> PointNormals(normals f32 [m,3], eig f32 [m,3], count int32 [m],
        flags int32 [m], moments int64 [m,9], neighbors int32 [m,max_nn]), the last two None unless asked for: the plane
        through every query's neighbourhood -- the grid's points within radius, cut to the max_nn nearest (the lowest row on a
        distance tie; 0 = no limit) -- as
        include/epn_so3conv.h states it (epn_point_normals_f32): the unit normal, the covariance's eigenvalues in ascending
        order (in the cloud's squared units), the size of the in-radius set, and flags bit 0 (fewer than three neighbours: the
        normal is (0, 0, 1)), bit 1 (a non-finite query) and bit 2 (the two smallest eigenvalues coincide: a line or a point,
        the direction is arbitrary).  view (three floats or a device tensor: a camera position, the fragment's own origin for
        a fused fragment) turns every normal towards it; without it the normal's largest component is positive.  radius
        defaults to the grid's max_radius."""
        radius = self.max_radius if radius is None else radius
        if not float(radius) <= self.max_radius:
            raise ValueError(f"radius must not exceed the grid's max_radius {self.max_radius}, got {radius}")
        if view is not None and not isinstance(view, torch.Tensor):
            view = torch.as_tensor(view, dtype=torch.float32).reshape(-1).to(self.points.device)
        return PointNormals(*_grouping().point_normals(
            self._workspace, self.n, self.points if queries is None else queries, radius, max_nn=max_nn,
            self_rows=queries is None, view=view, return_moments=return_moments, return_neighbors=return_neighbors))

    def fpfh(self, normals, radius=None, return_spfh=False):
        """normals f32 [n,3], one per point of the grid's cloud -> PointFPFH(features f32 [n,33], count int32 [n], flags int32
        [n], spfh int32 [n,33] or None): the FPFH descriptor of every point over the grid's points within radius (its own row
        apart), as include/epn_so3conv.h states it (epn_point_fpfh_f32): open3d's compute_fpfh_feature with
        KDTreeSearchParamRadius, made independent of the neighbours' order; features is open3d's .data.T.  count is the size of
        the neighbourhood; flags bit 0: it is empty; bit 1: a non-finite coordinate or normal, or a point the grid leaves out
        (`valid`); the row is zero with either.  spfh holds the integer bin counts of the simplified histogram.  radius
        defaults to the grid's max_radius."""
        radius = self.max_radius if radius is None else radius
        if not float(radius) <= self.max_radius:
            raise ValueError(f"radius must not exceed the grid's max_radius {self.max_radius}, got {radius}")
        return PointFPFH(*_grouping().point_fpfh(self._workspace, self.n, self.points, normals, radius, return_spfh=return_spfh))


def _grid(cloud, name, max_radius):
    """cloud: a PointGrid (its max_radius must cover max_radius) or a tensor to build one from."""
    if isinstance(cloud, PointGrid):
        if cloud.max_radius < max_radius:
            raise ValueError(f"{name}: the grid was built for radii up to {cloud.max_radius}, {max_radius} is needed")
        return cloud
    return PointGrid(_tensor(cloud, name, (None, 3), torch.float32), max_radius)


def estimate_normals(points_or_grid, radius, max_nn=30, view=None):
    """(points f32 [n,3] or their PointGrid, built with max_radius >= radius) -> PointNormals of the cloud's own points: the
    device form of open3d's pc.estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)) followed, with a view, by
    orient_normals_towards_camera_location(view) (the reference: SPConvNets/datasets/preprocess/run_fusion.py:48).  The
    correspondence with open3d is argued from its algorithm; it has not been run against open3d."""
    return _grid(points_or_grid, "points", float(radius)).normals(None, radius, max_nn=max_nn, view=view)


def compute_fpfh_feature(points_or_grid, normals, radius):
    """(points f32 [n,3] or their PointGrid, built with max_radius >= radius; normals f32 [n,3]) -> PointFPFH of the cloud's own
    points: the device form of open3d's compute_fpfh_feature(pc, KDTreeSearchParamRadius(radius)) (the reference:
    SPConvNets/datasets/preprocess/run_keypoint.py:40-50, which reads .data.T: features is that [n,33] array).  The
    correspondence with open3d is argued from its algorithm; it has not been run against open3d."""
    return _grid(points_or_grid, "points", float(radius)).fpfh(normals, radius)


def describe_fpfh(pc, keypoints, *, voxel_size=None, normal_radius, feature_radius, view=None):
    """(pc f32 [n,3], keypoints f32 [k,3] or integer rows [k]) -> (descriptors f32 [k,33], valid bool [k]): the FPFH descriptor
    at a fragment's keypoints, with the shape contract of InvSO3ConvModel.describe, so that the result goes unchanged into
    match_descriptors, evaluate_scene and register_scene -- the hand-crafted baseline of the 3DMatch tables.  voxel_size
    downsamples the fragment to its voxel centroids first (vgtk.pc.voxel_down_sample); integer keypoints are rows of the
    ORIGINAL pc, resolved to coordinates before that.  The normals are estimated on the (downsampled) cloud
    (estimate_normals(normal_radius, max_nn=30, view)), the descriptors computed for all of its points at feature_radius, and
    every keypoint takes the row of the cloud's nearest point within max(feature_radius, the voxel's diagonal).  valid is False
    where there is no such point or its flags bit 0 or 1 is set (no neighbour, a non-finite input); the descriptor is zero
    there."""
    if not isinstance(keypoints, torch.Tensor):
        raise TypeError(f"keypoints must be a torch tensor, got {type(keypoints).__name__}")
    if not keypoints.is_floating_point() and keypoints.dim() != 1:
        raise ValueError(f"integer keypoints must be [k] rows of pc, got {tuple(keypoints.shape)}")
    pc = _tensor(pc, "pc", (None, 3), torch.float32)
    if not keypoints.is_floating_point():
        keypoints = pc.index_select(0, keypoints.long())
    keypoints = _tensor(keypoints, "keypoints", (None, 3), torch.float32)
    reach = float(feature_radius)
    if voxel_size is not None:
        from .vgtk.pc import voxel_down_sample
        pc = voxel_down_sample(pc, float(voxel_size))[0]
        reach = max(reach, raw_radius(voxel_size))
    grid = PointGrid(pc, max(float(normal_radius), reach))
    normals = grid.normals(None, normal_radius, max_nn=30, view=view).normals
    desc = grid.fpfh(normals, feature_radius)
    row = grid.nearest(keypoints, reach)[0].to(torch.int64)
    found = row >= 0
    row = row.clamp(min=0)
    valid = found & (desc.flags.index_select(0, row) == 0) if grid.n else found
    out = desc.features.index_select(0, row) if grid.n else keypoints.new_zeros((keypoints.shape[0], 33))
    return out * valid[:, None].to(out.dtype), valid


def orient_patches(patches, normals):
    """(patches f32 [k,n_sample,3], normals f32 [k,3]) -> f32 [k,n_sample,3]: every patch in the frame of its keypoint's normal,
    the reference's transform_with_normals (SPConvNets/datasets/match_3dmatch.py:141-152) as include/epn_so3conv.h states it
    (epn_orient_patches_f32).  A zero patch stays zero."""
    return _grouping().orient_patches(patches, normals)[0]


def fragment_overlap(src, tgt, margin=0.075, ratio=0.3):
    """(src f32 [n_src,3], tgt f32 [n_tgt,3] or its PointGrid, both in the world frame) -> (hits int32 [], overlaps bool [], on
    the device): hits = the number of source points with a target point within margin; overlaps = hits >= ratio *
    max(n_src, n_tgt), the reference's test_scenes_overlap (run_keypoint.py:98-112; the product in fp64 as there).  The
    reference subsamples both clouds to subsample_maxpoints first; that is the caller's here (rows drawn with torch.randint)."""
    src = _tensor(src, "src", (None, 3), torch.float32)
    grid = _grid(tgt, "tgt", float(margin))
    hits = grid.nearest(src, margin, count=True)[2][0]
    need = math.ceil(float(ratio) * max(src.shape[0], grid.n))      # an integer count reaches the product iff it reaches its ceiling
    return hits, hits >= need


def raw_radius(voxel_size):
    """voxel_size * sqrt(3), the voxel's diagonal: a centroid lies inside its voxel, which holds a raw point."""
    return float(voxel_size) * math.sqrt(3.0)


def _population_std(x):
    """numpy.std of every row, in fp64: sqrt(mean(|x - mean(x)|^2))"""
    x = x.to(torch.float64)
    return ((x - x.mean(dim=1, keepdim=True)) ** 2).mean(dim=1).sqrt()


def keypoint_pairs(src_world, tgt_world, *, voxel_size=0.05, isolation_radius=0.15, match_radius=0.03, nonplanar_param=-1.0,
                   min_keypoints=128, normal_radius=None, views=None):
    """(src_world, tgt_world: f32 [n,3] in the world frame, or the PointGrid of one, built with max_radius >=
    raw_radius(voxel_size)) -> KeypointPairs(rows int32 [P,2], src_centroid_row int32 [P], d2 f32 [P]): the reference's
    generate_kp (run_keypoint.py:125-141) for one pair.  In this order:
      1. vgtk.pc.voxel_down_sample of both clouds at voxel_size;
      2. a centroid is kept when another centroid of its cloud lies within isolation_radius (the zero-FPFH filter, :58-59);
      3. every kept source centroid takes the nearest kept target centroid within match_radius (:66-67), or drops out;
      4. each surviving centroid is replaced by the row of the nearest raw point of its fragment (:131-138), searched within
         raw_radius(voxel_size); a centroid without one is a bug and raises RuntimeError.
    rows[:,0] are rows of the source cloud and rows[:,1] of the target cloud, in ascending source-centroid row; d2 is the squared
    centroid distance of step 3.  The survivors are compacted with a torch mask, and the status words of the two downsamplings and
    of the grids built here are read back: a handful of host synchronisations per pair of fragments, none per point.
    nonplanar_param > 0 adds the planar-patch filter of cross_filtering_via_fpfh (:77-92) between steps 3 and 4: the FPFH of
    both centroid clouds at isolation_radius (compute_fpfh_feature; normals from estimate_normals(normal_radius or
    isolation_radius, max_nn=30, view=views[side] if views is given)), and a pair stays only when the population standard
    deviation (numpy.std, in fp64) of both its 33-vectors is below nonplanar_param; with fewer than min_keypoints survivors the
    result is empty (upstream returns None and saves nothing).  One deviation: upstream's centroid normals are open3d's voxel
    averages of the raw cloud's normals; here they are estimated on the centroids, because voxel_down_sample carries no
    normals.  nonplanar_param <= 0 (the reference's default, -1) computes no descriptor."""
    from .vgtk.pc import voxel_down_sample
    R = raw_radius(voxel_size)
    raw = [_grid(src_world, "src_world", R), _grid(tgt_world, "tgt_world", R)]
    cen = [voxel_down_sample(g.points, voxel_size)[0] for g in raw]
    planar = float(nonplanar_param) > 0.0
    if planar:
        nr = float(isolation_radius if normal_radius is None else normal_radius)
        if views is not None and len(views) != 2:
            raise ValueError(f"views must hold the two fragments' view points, got {len(views)}")
        iso = [PointGrid(c, max(float(isolation_radius), nr)) for c in cen]
        desc = [g.fpfh(g.normals(None, nr, max_nn=30, view=None if views is None else views[side]).normals, isolation_radius)
                for side, g in enumerate(iso)]
    else:
        iso = [PointGrid(c, isolation_radius) for c in cen]
    keep = [g.nearest(c, isolation_radius, exclude_self=True)[0] >= 0 for g, c in zip(iso, cen)]
    idx, d2 = PointGrid(cen[1], match_radius, valid=keep[1]).nearest(cen[0], match_radius)
    sel = torch.nonzero(keep[0] & (idx >= 0)).reshape(-1)           # ascending; the one compaction
    if planar:
        partner = idx[sel].to(torch.int64)
        flat = ((_population_std(desc[0].features[sel]) < float(nonplanar_param))
                & (_population_std(desc[1].features[partner]) < float(nonplanar_param)))
        sel = sel[flat]
        if sel.numel() < int(min_keypoints):
            sel = sel[:0]
    partner = idx[sel].to(torch.int64)
    rows = torch.stack((raw[0].nearest(cen[0][sel], R)[0], raw[1].nearest(cen[1][partner], R)[0]), dim=1)
    if sel.numel() and int(rows.min()) < 0:
        raise RuntimeError("keypoint_pairs: a voxel centroid has no raw point within its voxel's diagonal")
    return KeypointPairs(rows, sel.to(torch.int32), d2[sel])


def pair_schedule(n_fragments, stride=4, window=20):
    """[(i, j)]: for every fragment i, j in range(i + 1, min(i + window, n), stride) (run_keypoint.py:162, :175)."""
    return [(i, j) for i in range(n_fragments) for j in range(i + 1, min(i + window, n_fragments), stride)]


def scene_keypoint_pairs(clouds_world, clouds_local=None, *, stride=4, window=20, margin=0.075, ratio=0.3, voxel_size=0.05,
                         isolation_radius=0.15, match_radius=0.03, nonplanar_param=-1.0, min_keypoints=128, normal_radius=None,
                         views=None):
    """(clouds_world: the F fragments of a scene in the world frame, f32 [n_i,3] each; clouds_local: the same fragments
    untransformed, or None) -> ({(i, j): rows int32 [P,2]}, corrs): keypoint_pairs for every pair of pair_schedule that passes
    fragment_overlap (source i, target j, the whole clouds: see fragment_overlap on subsampling), the others skipped as in
    run_keypoint.py:124.  corrs is None without clouds_local, else the list of f32 [P,2,3] fragment-frame coordinates, in the
    order of the dictionary: [:,0] = clouds_local[i][rows[:,0]], [:,1] = clouds_local[j][rows[:,1]] -- what
    vgtk.pc.pack_correspondences takes.  Every fragment is indexed once, for all the pairs it takes part in; the gate reads one
    bool per pair back to the host.  nonplanar_param, min_keypoints and normal_radius are keypoint_pairs'; views, if given, holds
    one view point per fragment (its camera origin in the world frame)."""
    if not isinstance(clouds_world, (list, tuple)):
        raise TypeError(f"clouds_world must be a list of [n,3] tensors, got {type(clouds_world).__name__}")
    F = len(clouds_world)
    if clouds_local is not None and len(clouds_local) != F:
        raise ValueError(f"clouds_local must hold the same {F} fragments, got {len(clouds_local)}")
    for k in range(F):
        _tensor(clouds_world[k], f"clouds_world[{k}]", (None, 3), torch.float32)
        if clouds_local is not None:
            _tensor(clouds_local[k], f"clouds_local[{k}]", (clouds_world[k].shape[0], 3), torch.float32)
    _lib.same_device(*clouds_world, *(clouds_local or ()))
    R = max(float(margin), raw_radius(voxel_size))
    grids = {}

    def grid(k):
        if k not in grids:
            grids[k] = PointGrid(clouds_world[k], R)
        return grids[k]

    rows, corrs = {}, None if clouds_local is None else []
    for i, j in pair_schedule(F, stride, window):
        if not bool(fragment_overlap(grid(i).points, grid(j), margin, ratio)[1]):
            continue
        r = keypoint_pairs(grid(i), grid(j), voxel_size=voxel_size, isolation_radius=isolation_radius,
                           match_radius=match_radius, nonplanar_param=nonplanar_param, min_keypoints=min_keypoints,
                           normal_radius=normal_radius, views=None if views is None else (views[i], views[j])).rows
        rows[(i, j)] = r
        if corrs is not None:
            r64 = r.to(torch.int64)
            corrs.append(torch.stack((clouds_local[i][r64[:, 0]], clouds_local[j][r64[:, 1]]), dim=1))
    return rows, corrs
