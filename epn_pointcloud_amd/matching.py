"""Descriptor matching and the 3DMatch inlier ratio / feature-match recall on the GPU: the step after
`InvSO3ConvModel.describe()`.

In-memory counterpart of the reference's SPConvNets/datasets/evaluation_3dmatch.py:56-123 (evaluate_fragment_pair) and
:197-205 (the recall over the pairs of a scene): nearest neighbours in descriptor space in both directions, the mutual check
"tgt -> src -> tgt", the ground-truth transform applied to the matched keypoints and the share of matches closer than tau1.
The file readers (.ply, keypoint lists, gt.log) stay with the caller.  Specification: include/epn_so3conv.h
(epn_nn_match_f32, epn_match_inliers_f64) and DESIGN.md 3.1a; kernels: csrc/desc_match.hip through vgtk.cuda.grouping.

Descriptors, keypoints and masks are device tensors (what describe() returns); the small per-pair results come back as numpy
arrays, like the reference's.  A whole scene is one nearest-neighbour launch and one inlier launch.

Without ground truth: `register_scene` / `register_fragment_pair` turn the mutual matches into the rigid transform between
the fragments (RANSAC over three-point samples and a refit; epn_ransac_register_f64, DESIGN.md 3.1c, csrc/ransac_register.hip),
and `registration_errors` / `registration_recall` score such transforms against known ones on the host.
`refine_registration` / `refine_scene` then refine such a transform on the dense clouds by ICP, point-to-point or point-to-plane
(epn_icp_refine_f32, DESIGN.md 3.1m, csrc/icp_refine.hip): open3d's registration_icp, the whole loop on the device.
"""
import collections

import numpy as np
import torch

from .vgtk.cuda import grouping

TAU_RANGE = (0.05, 0.1, 0.2)            # evaluation_3dmatch.py:126

SceneResult = collections.namedtuple("SceneResult", "n_inlier n_match inlier_ratio matches distances recall")
SceneResult.__doc__ = """evaluate_scene's result: n_inlier, n_match int32 [P], inlier_ratio float64 [P] (0 where n_match is 0),
matches (list of int32 [n_match, 2] arrays of (src row, tgt row) in ascending tgt row), distances (list of float64 [n_match]
arrays) and recall, the reference's [(tau, 100 * mean(inlier_ratio > tau))]."""

RegistrationResult = collections.namedtuple("RegistrationResult", "T n_match n_inlier rmse margin best_h")
RegistrationResult.__doc__ = """register_scene's result, numpy arrays: T float64 [P,4,4] taking tgt coordinates into src coordinates
(the identity for a failed pair), n_match int32 [P] mutual matches, n_inlier int32 [P] and rmse float64 [P] under T (0 and +inf
for a failed pair), margin float64 [P], the conditioning of the refit's rotation (0: not unique), best_h int32 [P], the
winning hypothesis (-1: the pair failed -- fewer than three matches, or no hypothesis with three inliers)."""


def _concat(kps, feats, valids):
    F = len(feats)
    if F < 1 or len(kps) != F or (valids is not None and len(valids) != F):
        raise ValueError("kps, feats and valids must be lists with one entry per fragment")
    for k, f in zip(kps, feats):
        if k.shape[0] != f.shape[0]:
            raise ValueError(f"a fragment has {k.shape[0]} keypoints and {f.shape[0]} descriptors")
    frag_off = np.concatenate(([0], np.cumsum([f.shape[0] for f in feats]))).astype(np.int64)
    all_feats = torch.cat([f.float() for f in feats]).contiguous()
    all_kps = torch.cat([k.float() for k in kps]).contiguous()
    valid = None
    if valids is not None and any(v is not None for v in valids):
        valid = torch.cat([torch.ones(f.shape[0], dtype=torch.uint8, device=f.device) if v is None else v.to(torch.uint8)
                           for v, f in zip(valids, feats)]).contiguous()
    return all_kps, all_feats, valid, frag_off


def evaluate_scene(kps, feats, valids, pairs, gt_transforms, tau1=0.1, taus=TAU_RANGE):
    """(kps: F tensors f[k_f,3], feats: F tensors f[k_f,C], valids: F masks [k_f] (or None, or None entries), pairs int [P,2] of
    (src fragment, tgt fragment), gt_transforms f64 [P,4,4] taking tgt coordinates into src coordinates) -> SceneResult.
    Every pair and both directions go through ONE nearest-neighbour launch; rows masked out by `valids` (describe()'s `valid`)
    never match and are never matched."""
    all_kps, all_feats, valid, frag_off = _concat(kps, feats, valids)
    pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    gt = np.asarray(torch.as_tensor(gt_transforms).cpu(), dtype=np.float64).reshape(-1, 4, 4)
    nn_idx, _, _ = grouping.nn_match(all_feats, frag_off, pairs, valid)
    match_src, match_dist, n_match, n_inlier, tgt_off = grouping.match_inliers(all_kps, frag_off, pairs, nn_idx, gt, tau1)
    match_src, match_dist = match_src.cpu().numpy(), match_dist.cpu().numpy()
    n_match, n_inlier, tgt_off = n_match.cpu().numpy(), n_inlier.cpu().numpy(), tgt_off.numpy()
    matches, distances = [], []
    for p in range(pairs.shape[0]):
        s = match_src[tgt_off[p]:tgt_off[p + 1]]
        rows = np.flatnonzero(s >= 0).astype(np.int32)
        matches.append(np.stack((s[rows], rows), axis=1))
        distances.append(match_dist[tgt_off[p]:tgt_off[p + 1]][rows])
    ratio = np.where(n_match > 0, n_inlier / np.maximum(n_match, 1), 0.0)
    recall = [(tau, 100.0 * float(np.mean(ratio > tau))) if ratio.size else (tau, 0.0) for tau in taus]
    return SceneResult(n_inlier, n_match, ratio, matches, distances, recall)


def evaluate_fragment_pair(src_kp, tgt_kp, src_feats, tgt_feats, gt_transform, tau1=0.1, src_valid=None, tgt_valid=None):
    """-> (n_inlier int, inlier_ratio float, matches int32 [n_match, 2] of (src row, tgt row), distances f64 [n_match]): the
    reference's evaluate_fragment_pair on arrays (its n_inlier and inlier_ratio; its `kpts` are matches[distances < tau1]).
    inlier_ratio is 0.0 when nothing matches, where the reference divides by zero."""
    r = evaluate_scene([src_kp, tgt_kp], [src_feats, tgt_feats], [src_valid, tgt_valid], [[0, 1]],
                       np.asarray(torch.as_tensor(gt_transform).cpu(), dtype=np.float64).reshape(1, 4, 4), tau1=tau1, taus=())
    return int(r.n_inlier[0]), float(r.inlier_ratio[0]), r.matches[0], r.distances[0]


def match_descriptors(src_feats, tgt_feats, src_valid=None, tgt_valid=None):
    """-> (src_to_tgt int32 [n_src], tgt_to_src int32 [n_tgt], mutual_tgt_mask bool [n_tgt]), device tensors: each row's
    nearest valid row of the other set (-1: none), and the tgt rows j with src_to_tgt[tgt_to_src[j]] == j."""
    ns, nt = src_feats.shape[0], tgt_feats.shape[0]
    kp = [src_feats.new_zeros((ns, 3), dtype=torch.float32), tgt_feats.new_zeros((nt, 3), dtype=torch.float32)]
    all_kps, all_feats, valid, frag_off = _concat(kp, [src_feats, tgt_feats], [src_valid, tgt_valid])
    nn_idx, _, _ = grouping.nn_match(all_feats, frag_off, [[0, 1]], valid)
    match_src = grouping.match_inliers(all_kps, frag_off, [[0, 1]], nn_idx, np.eye(4)[None], 0.0)[0]
    return nn_idx[:ns], nn_idx[ns:], match_src >= 0


def register_scene(kps, feats, valids, pairs, tau=0.05, hypotheses=4096, seed=0, min_margin=1e-2):
    """(kps, feats, valids, pairs as for evaluate_scene; tau: the inlier distance; hypotheses per pair; seed of the draws;
    min_margin: three-point samples whose fit is conditioned worse are rejected) -> RegistrationResult.  No ground truth: the
    mutual matches come from the nearest-neighbour launch and the mutual check run the way match_descriptors runs it (identity
    transforms, tau1 = 0), then the registration entry's three launches (compact, score, finish) cover every pair of the scene.
    Pair p draws with the counter (p, seed): the same pair at the same position gives the same transform, bit for bit."""
    all_kps, all_feats, valid, frag_off = _concat(kps, feats, valids)
    pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    P = pairs.shape[0]
    nn_idx, _, _ = grouping.nn_match(all_feats, frag_off, pairs, valid)
    match_src, _, n_match, _, tgt_off = grouping.match_inliers(all_kps, frag_off, pairs, nn_idx, np.tile(np.eye(4), (P, 1, 1)), 0.0)
    T, best_h, _, n_inlier, rmse, margin = grouping.ransac_register(all_kps, frag_off, pairs, match_src, tgt_off, tau, hypotheses,
                                                                    seed, min_margin)
    host = lambda x: x.cpu().numpy()
    return RegistrationResult(host(T), host(n_match), host(n_inlier), host(rmse), host(margin), host(best_h))


def register_fragment_pair(src_kp, tgt_kp, src_feats, tgt_feats, tau=0.05, hypotheses=4096, seed=0, min_margin=1e-2,
                           src_valid=None, tgt_valid=None):
    """-> (T float64 [4,4] taking tgt into src coordinates, n_match int, n_inlier int, rmse float, margin float, best_h int):
    register_scene on one pair (best_h == -1: the pair failed and T is the identity)."""
    r = register_scene([src_kp, tgt_kp], [src_feats, tgt_feats], [src_valid, tgt_valid], [[0, 1]], tau=tau, hypotheses=hypotheses,
                       seed=seed, min_margin=min_margin)
    return r.T[0], int(r.n_match[0]), int(r.n_inlier[0]), float(r.rmse[0]), float(r.margin[0]), int(r.best_h[0])


def registration_errors(T_est, T_gt):
    """(T_est, T_gt float [P,4,4] or [4,4]) -> (rre_deg float64 [P], rte float64 [P]): the angle of R_gt^T R_est in degrees and
    |t_est - t_gt|, numpy fp64 on the host."""
    A = np.asarray(T_est, dtype=np.float64).reshape(-1, 4, 4)
    B = np.asarray(T_gt, dtype=np.float64).reshape(-1, 4, 4)
    if A.shape != B.shape:
        raise ValueError(f"T_est and T_gt must have the same shape, got {A.shape} and {B.shape}")
    tr = np.einsum("pij,pij->p", B[:, :3, :3], A[:, :3, :3])
    rre = np.degrees(np.arccos(np.clip(0.5 * (tr - 1.0), -1.0, 1.0)))
    return rre, np.linalg.norm(A[:, :3, 3] - B[:, :3, 3], axis=1)


def registration_recall(T_est, T_gt, rre_deg=15.0, rte=0.3):
    """The share of pairs with a rotation error below rre_deg degrees and a translation error below rte (the convention of the
    learned-registration literature; both are parameters) -> float in [0, 1], 0.0 without pairs."""
    r, t = registration_errors(T_est, T_gt)
    return float(np.mean((r < rre_deg) & (t < rte))) if r.size else 0.0


IcpResult = collections.namedtuple("IcpResult", "T fitness inlier_rmse iterations status trace")
IcpResult.__doc__ = """refine_registration's result, host values: T float64 [4,4] taking src into the target's frame; fitness
(correspondences / source points) and inlier_rmse of the last live iteration -- after a stop those of T itself, otherwise those of
the transform the last iteration started from; iterations, the number of iterations that updated T; status, the flags met (bit
0: the stop test was met, bit 1: too few correspondences, bit 2: a singular system -- with 1 or 2 T is the last good transform);
trace float64 [max_iter,20], per iteration {T after it (16), count, sum of squared distances, rmse, flags}."""


def _invert_rigid(T):
    """The inverse of a rigid [4,4] in numpy fp64: (R^T, -R^T t).  The ONE place where refine_scene turns a pair's transform."""
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return out


def refine_registration(src_points, tgt_points_or_grid, T_init, max_dist, *, tgt_normals=None, max_iter=30, rel_fitness=1e-6,
                        rel_rmse=1e-6):
    """(src_points f32 [m,3]; tgt_points_or_grid: f32 [n,3] or its PointGrid, built with max_radius >= max_dist; T_init [4,4]
    taking src into the target's frame; max_dist: the correspondence distance) -> IcpResult: open3d's registration_icp on the
    device, as include/epn_so3conv.h states it (epn_icp_refine_f32).  The TARGET is the gridded cloud; every
    iteration moves the source by the current transform and pairs each of its points with the nearest target point within
    max_dist.  Without tgt_normals the update is point-to-point (Horn's fit), with tgt_normals f32 [n,3] (PointGrid.normals)
    point-to-plane.  The defaults are open3d's ICPConvergenceCriteria.  The whole loop runs on the device; the result is read
    back once, at the end.  A matched coordinate beyond 64 raises ValueError naming the flag's bit, as PointGrid does; too few
    correspondences and a singular system are returned in status, with the last good transform."""
    from .correspondence import _grid
    grid = _grid(tgt_points_or_grid, "tgt_points", float(max_dist))
    T0 = torch.as_tensor(np.ascontiguousarray(np.asarray(torch.as_tensor(T_init).cpu(), dtype=np.float64).reshape(4, 4)))
    T, trace, iterations, status, _, _ = grouping.icp_refine(grid._workspace, grid.n, src_points, T0.to(grid.points.device), max_dist,
                                                             tgt_normals=tgt_normals, max_iter=max_iter, rel_fitness=rel_fitness,
                                                             rel_rmse=rel_rmse)
    packed = torch.cat((T.reshape(-1), trace.reshape(-1), iterations.to(torch.float64), status.to(torch.float64))).cpu().numpy()
    T, trace, iterations, status = packed[:16].reshape(4, 4), packed[16:-2].reshape(-1, 20), int(packed[-2]), int(packed[-1])
    if status & 8:
        raise ValueError("refine_registration: status " + grouping.ICP_FLAGS[3] + f" (flags = {status})")
    m = src_points.shape[0]
    live = min(iterations + (1 if status else 0), trace.shape[0]) - 1   # a stop writes one more live record than it updates T
    count, rmse = (trace[live, 16], trace[live, 18]) if live >= 0 else (0.0, 0.0)
    return IcpResult(T, float(count) / m if m else 0.0, float(rmse), iterations, status, trace)


def refine_scene(clouds, pairs, T_init, max_dist, *, normals=None, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6):
    """(clouds: F tensors f32 [n_f,3], each in its fragment's own frame; pairs int [P,2] of (src fragment, tgt fragment); T_init
    f64 [P,4,4] as RegistrationResult.T holds it: taking tgt coordinates into src coordinates) -> (T float64 [P,4,4] in the same
    convention, results: the P IcpResults).  The pair's TGT fragment is the gridded cloud and its SRC fragment the moving one, so
    the stage runs from the inverse of T_init[p] (src into tgt) and its result is inverted back: both in _invert_rigid, numpy fp64
    on the host.  One PointGrid is built per fragment that appears as a tgt, with max_radius = max_dist (or the normals' radius,
    if that is larger).  normals: None (point-to-point), a float radius (the normals of every tgt fragment are estimated once,
    PointGrid.normals(radius=normals, max_nn=30)), or a list of F tensors f32 [n_f,3] (entries of fragments that are never a tgt
    may be None).  Every pair is one refine_registration call, and equals it bit for bit."""
    from .correspondence import PointGrid
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    T_init = np.asarray(torch.as_tensor(T_init).cpu(), dtype=np.float64).reshape(-1, 4, 4)
    if T_init.shape[0] != pairs.shape[0]:
        raise ValueError(f"T_init must be [{pairs.shape[0]},4,4], got {T_init.shape}")
    if pairs.size and (pairs.min() < 0 or pairs.max() >= len(clouds)):
        raise ValueError(f"pairs must index fragments 0..{len(clouds) - 1}")
    estimate = isinstance(normals, (int, float)) and not isinstance(normals, bool)
    if normals is not None and not estimate and len(normals) != len(clouds):
        raise ValueError(f"normals must be a radius or hold one entry per fragment, got {len(normals)} for {len(clouds)}")
    grids, nrm = {}, {}
    for j in sorted(set(pairs[:, 1].tolist())):
        grids[j] = PointGrid(clouds[j], max(float(max_dist), float(normals)) if estimate else float(max_dist))
        nrm[j] = None if normals is None else (grids[j].normals(radius=float(normals), max_nn=30).normals if estimate
                                               else normals[j])
        if normals is not None and nrm[j] is None:
            raise ValueError(f"normals[{j}] is None, but fragment {j} is the tgt of a pair")
    T, results = np.tile(np.eye(4), (pairs.shape[0], 1, 1)), []
    for p, (i, j) in enumerate(pairs.tolist()):
        r = refine_registration(clouds[i], grids[j], _invert_rigid(T_init[p]), max_dist, tgt_normals=nrm[j], max_iter=max_iter,
                                rel_fitness=rel_fitness, rel_rmse=rel_rmse)
        results.append(r)
        T[p] = _invert_rigid(r.T)
    return T, results
