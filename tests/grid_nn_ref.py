"""Numpy restatement of the point-grid specification (include/epn_so3conv.h: epn_point_grid_build_f32, epn_point_grid_nn_f32;
DESIGN.md 3.1j), written from the specification and not from the kernel: the query is brute force over all reference points,
with no grid at all -- the grid may change nothing of the answer.  The cell rule is restated separately (cell_indices, through
tests/voxel_ref.py, whose rule it is) because tests place points in chosen cells and construct hash collisions.  keypoint_pairs
restates epn_pointcloud_amd.correspondence.keypoint_pairs from these and voxel_ref.voxel_downsample."""
import math

import numpy as np

import voxel_ref as V

MAX_N = 2 ** 22


def cell_edge(max_radius):
    return np.float64(max_radius) * (1.0 + 2.0 ** -10)


def participates(ref, valid=None):
    ref = np.asarray(ref, dtype=np.float32).reshape(-1, 3)
    part = np.isfinite(ref).all(axis=1)
    return part if valid is None else part & (np.asarray(valid).reshape(-1) != 0)


def cell_indices(ref, max_radius, valid=None):
    """(participates bool [n], idx int64 [participating, 3], flags): the voxel rule at voxel_size = the cell edge."""
    ref = np.asarray(ref, dtype=np.float32).reshape(-1, 3)
    part = participates(ref, valid)
    _, idx, flags = V.voxel_indices(ref[part], cell_edge(max_radius))
    return part, idx, flags


def nearest(ref, qry, radius, valid=None, exclude_self=False, rows_per_pass=512):
    """-> (nn_idx int32 [m], nn_d2 float32 [m]).  Per query: among the participating reference points with d2 <= r2 the smallest
    d2, the lowest row on a tie; -1 and +inf without one.  d2 = (dx*dx + dy*dy) + dz*dz in float32 arrays (numpy rounds every
    operation), r2 = float32 of the float64 product."""
    ref = np.asarray(ref, dtype=np.float32).reshape(-1, 3)
    qry = np.asarray(qry, dtype=np.float32).reshape(-1, 3)
    n, m = ref.shape[0], qry.shape[0]
    assert not exclude_self or m == n
    r2 = np.float32(np.float64(radius) * np.float64(radius))
    out = ~participates(ref, valid)
    nn_idx = np.full(m, -1, dtype=np.int32)
    nn_d2 = np.full(m, np.inf, dtype=np.float32)
    if n == 0:
        return nn_idx, nn_d2
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, m, rows_per_pass):
            q = qry[a:a + rows_per_pass]
            dx = ref[None, :, 0] - q[:, None, 0]
            dy = ref[None, :, 1] - q[:, None, 1]
            dz = ref[None, :, 2] - q[:, None, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            ok = d2 <= r2                                           # NaN compares false
            ok[:, out] = False
            ok[~np.isfinite(q).all(axis=1)] = False
            if exclude_self:
                rows = np.arange(a, a + q.shape[0])
                ok[rows - a, rows] = False
            d2 = np.where(ok, d2, np.float32(np.inf))
            best = d2.argmin(axis=1)                                # the first of equal minima: the lowest row
            found = ok[np.arange(q.shape[0]), best]
            nn_idx[a:a + q.shape[0]] = np.where(found, best, -1)
            nn_d2[a:a + q.shape[0]] = d2[np.arange(q.shape[0]), best]
    return nn_idx, nn_d2


def raw_radius(voxel_size):
    return float(voxel_size) * math.sqrt(3.0)


def keypoint_pairs(src, tgt, voxel_size=0.05, isolation_radius=0.15, match_radius=0.03):
    """-> (rows int32 [P,2], src_centroid_row int32 [P], d2 float32 [P]): downsample, drop the centroids without another
    centroid of their cloud within isolation_radius, match every kept source centroid to the nearest kept target centroid within
    match_radius, map the survivors to their nearest raw rows; in ascending source-centroid row."""
    raw = [np.asarray(src, dtype=np.float32), np.asarray(tgt, dtype=np.float32)]
    cen = [V.voxel_downsample(p, voxel_size)[0] for p in raw]
    keep = [nearest(c, c, isolation_radius, exclude_self=True)[0] >= 0 for c in cen]
    idx, d2 = nearest(cen[1], cen[0], match_radius, valid=keep[1])
    sel = np.nonzero(keep[0] & (idx >= 0))[0]
    R = raw_radius(voxel_size)
    rows = np.stack((nearest(raw[0], cen[0][sel], R)[0], nearest(raw[1], cen[1][idx[sel]], R)[0]), axis=1)
    assert (rows >= 0).all()
    return rows.astype(np.int32), sel.astype(np.int32), d2[sel]


def lattice_clouds(n_ref=5000, n_qry=3000, seed=7):
    """Coordinates on multiples of 2^-8 in [-2, 2]: differences, squares and their sums are exact in fp32 and fp64 alike (at
    most 11 + 11 bits per square, below 2^6)."""
    rng = np.random.default_rng(seed)
    ref = (rng.integers(-512, 513, (n_ref, 3)) / 256.0).astype(np.float32)
    qry = (rng.integers(-512, 513, (n_qry, 3)) / 256.0).astype(np.float32)
    return ref, qry
