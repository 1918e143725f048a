"""Descriptor matching and the 3DMatch inlier ratio / feature-match recall on the GPU: the step after
`InvSO3ConvModel.describe()`.

In-memory counterpart of the reference's SPConvNets/datasets/evaluation_3dmatch.py:56-123 (evaluate_fragment_pair) and
:197-205 (the recall over the pairs of a scene): nearest neighbours in descriptor space in both directions, the mutual check
"tgt -> src -> tgt", the ground-truth transform applied to the matched keypoints and the share of matches closer than tau1.
The file readers (.ply, keypoint lists, gt.log) stay with the caller.  Specification: include/epn_so3conv.h
(epn_nn_match_f32, epn_match_inliers_f64) and DESIGN.md 3.1a; kernels: csrc/desc_match.hip through vgtk.cuda.grouping.

Descriptors, keypoints and masks are device tensors (what describe() returns); the small per-pair results come back as numpy
arrays, like the reference's.  A whole scene is one nearest-neighbour launch and one inlier launch.
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
