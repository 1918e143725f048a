"""Numpy restatement of the voxel-grid downsampling specification (include/epn_so3conv.h: epn_voxel_downsample_f32; DESIGN.md
3.1), written from the specification and not from the kernel: a stable sort by voxel index and integer segment sums, no hash
table.  The hash function is restated separately (home_slot) because tests construct collisions from it."""
import numpy as np

FLAG_COORD, FLAG_INDEX = 1, 2
HASH = 0x9E3779B97F4A7C15


def capacity(n):
    """The smallest power of two >= max(2n, 128)."""
    cap = 128
    while cap < 2 * n:
        cap *= 2
    return cap


def home_slot(key, cap):
    """(key * HASH mod 2^64) >> (64 - log2(cap)), in Python integers."""
    return ((int(key) * HASH) & (2 ** 64 - 1)) >> (64 - (cap.bit_length() - 1))


def make_key(ix, iy, iz):
    return (np.asarray(ix, dtype=np.int64) << 42) | (np.asarray(iy, dtype=np.int64) << 21) | np.asarray(iz, dtype=np.int64)


def voxel_indices(pc, voxel_size):
    """(kept bool [n], idx int64 [kept, 3], flags): the fp64 voxel index of every kept point and the status flags."""
    pc = np.asarray(pc, dtype=np.float32).reshape(-1, 3)
    kept = np.isfinite(pc).all(axis=1)
    p = pc[kept]
    if p.shape[0] == 0:
        return kept, np.zeros((0, 3), dtype=np.int64), 0
    flags = FLAG_COORD if (np.abs(p) > 256).any() else 0
    lo = p.min(axis=0)                                              # fp32
    vmin = lo.astype(np.float64) - 0.5 * np.float64(voxel_size)
    f = np.floor((p.astype(np.float64) - vmin) / np.float64(voxel_size))
    if (f >= 2 ** 21).any():
        flags |= FLAG_INDEX
    return kept, np.clip(f, 0, 2 ** 21 - 1).astype(np.int64), flags


def fixed_point(p):
    """llrint((double)x * 2^32), round half to even."""
    return np.rint(np.asarray(p, dtype=np.float32).astype(np.float64) * 4294967296.0).astype(np.int64)


def voxel_map(pc, voxel_size):
    """{key: (sum_x, sum_y, sum_z, count)} in Python integers: what the permutation test compares."""
    kept, idx, flags = voxel_indices(pc, voxel_size)
    assert flags == 0
    key = make_key(idx[:, 0], idx[:, 1], idx[:, 2])
    fx = fixed_point(np.asarray(pc, dtype=np.float32).reshape(-1, 3)[kept])
    out = {}
    for k, f in zip(key.tolist(), fx.tolist()):
        s = out.setdefault(k, [0, 0, 0, 0])
        s[0] += f[0]; s[1] += f[1]; s[2] += f[2]; s[3] += 1
    return {k: tuple(v) for k, v in out.items()}


def voxel_downsample(pc, voxel_size):
    """-> (centroids f32 [M,3], counts i32 [M], first_idx i32 [M], point_voxel i32 [n], keys i64 [M], flags).  With flags != 0
    only flags is meaningful."""
    pc = np.asarray(pc, dtype=np.float32).reshape(-1, 3)
    n = pc.shape[0]
    kept, idx, flags = voxel_indices(pc, voxel_size)
    point_voxel = np.full(n, -1, dtype=np.int32)
    rows = np.nonzero(kept)[0]
    if rows.size == 0 or flags:
        return (np.zeros((0, 3), np.float32), np.zeros(0, np.int32), np.zeros(0, np.int32), point_voxel, np.zeros(0, np.int64),
                flags)
    order = np.lexsort((rows, idx[:, 2], idx[:, 1], idx[:, 0]))     # by voxel, then by point index
    sidx = idx[order]
    start = np.concatenate(([True], (np.diff(sidx, axis=0) != 0).any(axis=1)))
    seg = np.nonzero(start)[0]
    sums = np.add.reduceat(fixed_point(pc[rows[order]]), seg, axis=0)            # int64, exact
    counts = np.diff(np.concatenate((seg, [order.size])))
    first = rows[order][seg]                                        # the lowest point index of every voxel
    out = np.argsort(first, kind="stable")                          # output order: ascending first index
    centroids = (sums[out].astype(np.float64) / (counts[out].astype(np.float64)[:, None] * 4294967296.0)).astype(np.float32)
    rank = np.empty(seg.size, dtype=np.int64)
    rank[out] = np.arange(seg.size)
    point_voxel[rows[order]] = rank[np.cumsum(start) - 1]
    keys = make_key(sidx[seg][out, 0], sidx[seg][out, 1], sidx[seg][out, 2])
    return centroids, counts[out].astype(np.int32), first[out].astype(np.int32), point_voxel, keys, flags


def colliding_cloud(n, home, voxel_size=2.0 ** -5, span=32):
    """n grid-valued points in n distinct voxels whose keys all have home slot `home` at capacity(n), found by brute search over
    the voxel indices [0, span)^3; every axis has a point with index 0, so the indices are the voxel indices the kernel derives
    (lo = 0, a point at index k sits at k * voxel_size, half a voxel inside voxel k).  -> (pc f32 [n,3], idx int64 [n,3])."""
    cap = capacity(n)
    g = np.arange(span)
    cand = [(x, y, z) for x in g for y in g for z in g if home_slot(int(make_key(x, y, z)), cap) == home]
    chosen = []
    for axis in range(3):                                           # one candidate with a zero on every axis first
        zero = [c for c in cand if c[axis] == 0 and c not in chosen]
        assert zero, f"no candidate with index 0 on axis {axis}: raise span"
        chosen.append(zero[0])
    chosen += [c for c in cand if c not in chosen][:n - len(chosen)]
    assert len(chosen) == n, "too few candidates: raise span"
    idx = np.array(chosen, dtype=np.int64)
    return (idx * voxel_size).astype(np.float32), idx
