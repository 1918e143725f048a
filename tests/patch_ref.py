"""numpy restatement of the patch extraction (include/epn_so3conv.h: epn_radius_patches_f32), independent of
the kernel: brute force over every (keypoint, point) pair, a full sort for the selection, fp32 arithmetic in the stated order.

For keypoint row q, Q = kpt_row0 + q:
    S = { i : d2(i) <= r2 },  d2 = (dx*dx + dy*dy) + dz*dz,  r2 = radius*radius, every operation rounded to fp32
    key(i) = word0(Philox4x32-10(counter = {i, 0, lo32(Q), hi32(Q)}, key = seed)) >> (32 - key_bits)
    count <= 1: idx -1, patch 0.   count >= n_sample: the n_sample smallest (key, i), in ascending i.
    1 < count < n_sample: S in ascending i, then slot j repeats slot word1(Philox({j, 0, lo32(Q), hi32(Q)}, seed)) mod count.
    patches = (pc[idx] - center * kpt) * scale, the subtraction rounded first."""
import numpy as np

from philox_ref import philox4x32_10

_M64 = 2 ** 64 - 1
F = np.float32


def _words(ctr_lo, Q, seed):
    Q, seed = int(Q) & _M64, int(seed) & _M64
    lo = np.asarray(ctr_lo, dtype=np.uint64)
    return philox4x32_10([lo & np.uint64(0xFFFFFFFF), lo >> np.uint64(32), Q & 0xFFFFFFFF, Q >> 32], [seed & 0xFFFFFFFF, seed >> 32])


def keys(indices, Q, seed, key_bits=32):
    """uint32 key of every point index in `indices` for global keypoint row Q."""
    return _words(indices, Q, seed)[0] >> np.uint32(32 - key_bits)


def in_radius(pc, kpt, radius):
    """bool[n]: membership of S for one keypoint, in individually rounded fp32."""
    pc, kpt = np.asarray(pc, dtype=F), np.asarray(kpt, dtype=F)
    d = pc - kpt[None, :]                               # fp32 - fp32 -> fp32, one rounding each
    sq = d * d
    d2 = (sq[:, 0] + sq[:, 1]) + sq[:, 2]
    return d2 <= F(radius) * F(radius)


def select(members, Q, n_sample, seed, key_bits=32):
    """The idx row (int32 [n_sample]) for the ascending array `members` of in-radius point indices."""
    members = np.asarray(members, dtype=np.int64)
    count = members.size
    row = np.full(n_sample, -1, dtype=np.int32)
    if count <= 1:
        return row
    if count >= n_sample:
        k = keys(members, Q, seed, key_bits).astype(np.int64)
        order = np.lexsort((members, k))                # primary key, then index
        return np.sort(members[order[:n_sample]]).astype(np.int32)
    row[:count] = members
    j = np.arange(count, n_sample)
    row[count:] = row[(_words(j, Q, seed)[1].astype(np.int64) % count)]
    return row


def radius_patches(pc, kpts, radius, n_sample, seed=0, kpt_row0=0, key_bits=32, center=0, scale=1.0):
    """-> (idx int32 [k,n_sample], counts int32 [k], patches float32 [k,n_sample,3])."""
    pc, kpts = np.ascontiguousarray(pc, dtype=F), np.ascontiguousarray(kpts, dtype=F).reshape(-1, 3)
    k = kpts.shape[0]
    idx = np.full((k, n_sample), -1, dtype=np.int32)
    counts = np.zeros(k, dtype=np.int32)
    patches = np.zeros((k, n_sample, 3), dtype=F)
    for q in range(k):
        members = np.nonzero(in_radius(pc, kpts[q], radius))[0]
        counts[q] = members.size
        idx[q] = select(members, kpt_row0 + q, n_sample, seed, key_bits)
        if members.size > 1:
            c = kpts[q] if center else np.zeros(3, dtype=F)
            patches[q] = (pc[idx[q]] - c[None, :]) * F(scale)
    return idx, counts, patches
