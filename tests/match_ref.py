"""numpy restatement of the descriptor-matching specification (include/epn_so3conv.h: epn_nn_match_f32,
epn_match_inliers_f64), independent of the library: fp64 distances from the differences, np.argmin (whose
first-minimum rule is the tie rule) and the valid masks."""
import numpy as np


def d2_matrix(a, b):
    """fp64 [n_a, n_b] squared distances from the differences."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    D = np.empty((a.shape[0], b.shape[0]))
    step = max(1, (1 << 22) // max(1, b.shape[0] * a.shape[1]))      # rows of a per block: 32 MB of differences
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(0, a.shape[0], step):
            diff = a[r:r + step, None, :] - b[None, :, :]
            D[r:r + step] = np.einsum("ijc,ijc->ij", diff, diff)
    return D


def nearest(a, b, a_valid=None, b_valid=None):
    """Rows of a query the rows of b -> (idx int32 [n_a], d2 float64 [n_a], D float64 [n_a, n_b] with inadmissible entries
    at +inf).  Admissible: b row valid and d2 finite.  (-1, +inf) for an invalid query or one without a candidate."""
    D = d2_matrix(a, b)
    D = np.where(np.isfinite(D), D, np.inf)
    if b_valid is not None:
        D[:, ~np.asarray(b_valid, dtype=bool)] = np.inf
    if a_valid is not None:
        D[~np.asarray(a_valid, dtype=bool), :] = np.inf
    if D.shape[1] == 0:
        return np.full(D.shape[0], -1, np.int32), np.full(D.shape[0], np.inf), D
    idx = np.argmin(D, axis=1).astype(np.int32)
    d2 = D[np.arange(D.shape[0]), idx]
    idx[~np.isfinite(d2)] = -1
    return idx, d2, D


def nn_match(feats, frag_off, pairs, valid=None):
    """-> (nn_idx int32 [out_off[P]], nn_d2 float64 [out_off[P]], out_off int64 [P+1]) in the library's layout: pair p's src
    rows, then its tgt rows."""
    frag_off = np.asarray(frag_off, dtype=np.int64)
    idx, d2, off = [], [], [0]
    for s, t in np.asarray(pairs).reshape(-1, 2):
        rs, rt = slice(frag_off[s], frag_off[s + 1]), slice(frag_off[t], frag_off[t + 1])
        vs, vt = (None, None) if valid is None else (valid[rs], valid[rt])
        i1, d1, _ = nearest(feats[rs], feats[rt], vs, vt)
        i2, d2_, _ = nearest(feats[rt], feats[rs], vt, vs)
        idx += [i1, i2]
        d2 += [d1, d2_]
        off.append(off[-1] + i1.size + i2.size)
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    return cat(idx, np.int32), cat(d2, np.float64), np.asarray(off, dtype=np.int64)


def inliers(src_kp, tgt_kp, src_to_tgt, tgt_to_src, gt, tau1):
    """The mutual check tgt -> src -> tgt and the transformed distances -> (match_src int32 [n_tgt] (-1: not mutual),
    match_dist float64 [n_tgt] (+inf: not mutual), n_match, n_inlier)."""
    src_kp, tgt_kp, gt = (np.asarray(x, dtype=np.float64) for x in (src_kp, tgt_kp, gt))
    n_tgt = tgt_to_src.shape[0]
    s = tgt_to_src.astype(np.int64)
    mutual = (s >= 0) & (src_to_tgt[np.maximum(s, 0)] == np.arange(n_tgt)) if src_to_tgt.size else np.zeros(n_tgt, bool)
    moved = tgt_kp @ gt[:3, :3].T + gt[:3, 3]
    dist = np.full(n_tgt, np.inf)
    dist[mutual] = np.sqrt(((src_kp[s[mutual]] - moved[mutual]) ** 2).sum(axis=1))
    match_src = np.where(mutual, s, -1).astype(np.int32)
    return match_src, dist, int(mutual.sum()), int((dist < tau1).sum())


def evaluate_fragment_pair(src_kp, tgt_kp, src_feats, tgt_feats, gt, tau1=0.1, src_valid=None, tgt_valid=None):
    """-> (n_inlier, inlier_ratio, matches int32 [n_match, 2] (src row, tgt row), distances float64 [n_match])."""
    s2t, _, _ = nearest(src_feats, tgt_feats, src_valid, tgt_valid)
    t2s, _, _ = nearest(tgt_feats, src_feats, tgt_valid, src_valid)
    match_src, dist, n_match, n_inlier = inliers(src_kp, tgt_kp, s2t, t2s, gt, tau1)
    rows = np.flatnonzero(match_src >= 0).astype(np.int32)
    ratio = n_inlier / n_match if n_match else 0.0
    return n_inlier, ratio, np.stack((match_src[rows], rows), axis=1), dist[rows]


# ----------------------------------------------------------------------------- seeded inputs shared by the tests

def frag_offsets(sizes):
    return np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)


def unit_scene(sizes, C, seed):
    """Generic float descriptors, unit rows: fragment 0 is random; in every other fragment two rows of three are noisy copies
    (sigma 0.05 per component before normalising) of random rows of fragment 0, the rest random -> (feats f32 [R,C], frag_off)."""
    rng = np.random.default_rng(seed)
    unit = lambda x: x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-30)
    base = unit(rng.standard_normal((sizes[0], C)))
    frags = [base]
    for n in sizes[1:]:
        x = unit(rng.standard_normal((n, C)))
        copy = rng.random(n) < 2.0 / 3.0
        x[copy] = unit(base[rng.integers(0, sizes[0], int(copy.sum()))] + 0.05 * rng.standard_normal((int(copy.sum()), C)))
        frags.append(x)
    return np.concatenate(frags).astype(np.float32), frag_offsets(sizes)


def quantised_scene(sizes, C, seed, seg=512):
    """Descriptors on the grid of multiples of 2^-8 in [-1, 1]: every d2 is a multiple of 2^-16 below 2^9 (C <= 128) and exact
    in fp32 in any summation order.  Every fragment carries duplicated rows: row 0 again at rows 2 and n - 1, and the row before
    each multiple of `seg` (the kernel's target-segment length) again right after it, so that one duplicate pair straddles every
    segment boundary; row 1 of every OTHER fragment is set to such a duplicated row, which makes the tie the minimum
    (d2 = 0) -> (feats f32 [R,C], frag_off)."""
    rng = np.random.default_rng(seed)
    frags = [rng.integers(-256, 257, (n, C)).astype(np.float64) / 256.0 for n in sizes]
    for x in frags:
        n = x.shape[0]
        if n > 2:
            x[2] = x[0]
            x[n - 1] = x[0]
        for b in range(seg, n, seg):
            x[b] = x[b - 1]
    for i, x in enumerate(frags):
        other = frags[(i + 1) % len(frags)]
        if x.shape[0] > 1 and other is not x:
            b = seg if other.shape[0] > seg else 0
            x[1] = other[b - 1 if b else 0]
    return np.concatenate(frags).astype(np.float32), frag_offsets(sizes)
