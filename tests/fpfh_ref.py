"""Numpy restatement of the FPFH specification (include/epn_so3conv.h: epn_point_fpfh_f32), written from the
specification and not from the kernel: the neighbourhoods are brute force over all pairs, with no grid at all.  Float64 arrays
round every operation on its own, which is the stated arithmetic; the operations are written in the stated order.  It is open3d's
ComputePairFeatures / ComputeSPFHFeature / ComputeFPFHFeature as argued from open3d's algorithm, not run against it.

Besides the outputs it returns an EDGE CENSUS: for every (ordered) neighbour pair and each of the three features, the distance of
the value whose floor is the bin from the nearest integer.  A pair is an edge pair when that distance is below EDGE = 2^-30:
there another atan2 (the device's, another host's) may legitimately land in the other bin.  A value at or beyond the clamped ends
(nearest integer <= 0 or >= 11) is no edge: both sides of that integer give the same clamped bin.

Every input of tests/test_gpu_fpfh.py is generated here (the case_* functions), and tests/test_fpfh_spec.py holds each of them to
zero edge pairs, on the CPU."""
import numpy as np

import grid_nn_ref as G
import voxel_ref as V

BINS, WIDTH = 11, 33
FIX = 2.0 ** 40
EDGE = 2.0 ** -30
FLAG_ALONE, FLAG_INPUT = 1, 2


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack((a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]), axis=-1)


def pair_features(pi, ni, pk, nk):
    """(float32 [..., 3] each: the query's point and normal, the neighbour's point and normal) -> f float64 [..., 3]"""
    pi, ni, pk, nk = (np.asarray(a, np.float32) for a in (pi, ni, pk, nk))
    ok = np.isfinite(ni).all(axis=-1) & np.isfinite(nk).all(axis=-1)
    pi, pk = pi.astype(np.float64), pk.astype(np.float64)
    a = np.where(ok[..., None], ni, np.float32(0)).astype(np.float64)
    b = np.where(ok[..., None], nk, np.float32(0)).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = pk - pi
        length = np.sqrt(_dot(d, d))
        a1, a2 = _dot(a, d) / length, _dot(b, d) / length
        swap = np.abs(a1) < np.abs(a2)
        n1, n2 = np.where(swap[..., None], b, a), np.where(swap[..., None], a, b)
        d = np.where(swap[..., None], -d, d)
        f3 = np.where(swap, -a2, a1)
        v = _cross(d, n1)
        vn = np.sqrt(_dot(v, v))
        v = v / vn[..., None]
        w = _cross(n1, v)
        y = _dot(w, n2)
        y = np.where(y == 0.0, 0.0, y)                              # -0 counts as +0
        f = np.stack((np.arctan2(y, _dot(n1, n2)), _dot(v, n2), f3), axis=-1)
    zero = ~ok | (length == 0.0) | (vn == 0.0)
    return np.where(zero[..., None], 0.0, f)


def bin_values(f):
    f = np.asarray(f, np.float64)
    return np.stack(((11.0 * (f[..., 0] + np.pi)) / (2.0 * np.pi), (11.0 * (f[..., 1] + 1.0)) * 0.5,
                     (11.0 * (f[..., 2] + 1.0)) * 0.5), axis=-1)


def bins_of(t):
    return np.clip(np.floor(t), 0.0, 10.0).astype(np.int64)


def edge_distance(t):
    """|t - nearest integer|, +inf where that integer is <= 0 or >= 11 (the clamp gives one bin on both sides)"""
    t = np.asarray(t, np.float64)
    near = np.rint(t)
    return np.where((near <= 0.0) | (near >= 11.0), np.inf, np.abs(t - near))


def pair_bins(pi, ni, pk, nk):
    """-> (h int64 [..., 3], edge distance float64 [..., 3])"""
    t = bin_values(pair_features(pi, ni, pk, nk))
    return bins_of(t), edge_distance(t)


def neighbour_pairs(points, radius, valid=None, rows_per_pass=512):
    """-> (i int64 [P], k int64 [P], d2 float32 [P]): every ordered pair i != k of participating points with d2 <= r2, d2 =
    (dx*dx + dy*dy) + dz*dz in float32 arrays and r2 = float32 of the float64 product -- grid_nn_ref.nearest's rule."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    part = G.participates(points, valid)
    r2 = np.float32(np.float64(radius) * np.float64(radius))
    I, K, D = [], [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, points.shape[0], rows_per_pass):
            q = points[a:a + rows_per_pass]
            dx = points[None, :, 0] - q[:, None, 0]
            dy = points[None, :, 1] - q[:, None, 1]
            dz = points[None, :, 2] - q[:, None, 2]
            d2 = (dx * dx + dy * dy) + dz * dz
            ok = (d2 <= r2) & part[None, :] & part[a:a + q.shape[0], None]
            rows = np.arange(q.shape[0])
            ok[rows, rows + a] = False
            i, k = np.nonzero(ok)
            I.append(i + a)
            K.append(k)
            D.append(d2[i, k])
    if not I:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
    return np.concatenate(I), np.concatenate(K), np.concatenate(D)


def point_fpfh(points, normals, radius, valid=None):
    """-> dict(fpfh float32 [n,33], count int32 [n], flags int32 [n], spfh int32 [n,33], pairs = (i, k, d2), edge float64 [P,3]
    = the census, edge_pairs = the number of pairs with an entry below EDGE)."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    normals = np.asarray(normals, np.float32).reshape(-1, 3)
    n = points.shape[0]
    assert normals.shape[0] == n
    part = G.participates(points, valid)
    whole = part & np.isfinite(normals).all(axis=1)
    i, k, d2 = neighbour_pairs(points, radius, valid)
    used = np.bincount(i, minlength=n).astype(np.int64)
    h, edge = pair_bins(points[i], normals[i], points[k], normals[k])
    counted = whole[i]                                              # a point with a bad normal keeps a zero row
    c = np.zeros((n, WIDTH), np.int64)
    for g in range(3):
        np.add.at(c, (i[counted], g * BINS + h[counted, g]), 1)
    edge = np.where(counted[:, None], edge, np.inf)
    flags = np.where(used == 0, FLAG_ALONE, 0) | np.where(whole, 0, FLAG_INPUT)
    # the weighted sums, in fixed point
    pos = d2 > 0
    d2min = np.full(n, np.inf, np.float32)
    np.minimum.at(d2min, i[pos], d2[pos])
    ip, kp = i[pos], k[pos]
    w = d2min[ip].astype(np.float64) / d2[pos].astype(np.float64)
    s = c[kp].astype(np.float64) / used[kp].astype(np.float64)[:, None]
    term = np.rint((w[:, None] * s) * FIX).astype(np.int64)
    A = np.zeros((n, WIDTH), np.int64)
    np.add.at(A, ip, term)
    Gs = np.repeat(A.reshape(n, 3, BINS).sum(axis=2), BINS, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        nb = np.where(Gs != 0, (100.0 * A.astype(np.float64)) / Gs.astype(np.float64), 0.0)
        own = (100.0 * c.astype(np.float64)) / used.astype(np.float64)[:, None]
        out = (nb + own).astype(np.float32)
    out[flags != 0] = 0.0
    return dict(fpfh=out, count=used.astype(np.int32), flags=flags.astype(np.int32), spfh=c.astype(np.int32), pairs=(i, k, d2),
                edge=edge, edge_pairs=int((edge < EDGE).any(axis=1).sum()) if edge.size else 0, A=A)


def std_filter(fa, fb, nonplanar_param):
    """bool [P]: the pair survives when the population standard deviation of both 33-vectors is below the parameter
    (cross_filtering_via_fpfh, run_keypoint.py:77-92: numpy.std of each descriptor)"""
    fa, fb = np.asarray(fa, np.float64), np.asarray(fb, np.float64)
    return (fa.std(axis=1) < nonplanar_param) & (fb.std(axis=1) < nonplanar_param)


def keypoint_candidates(src, tgt, cen_normals, voxel_size=0.05, isolation_radius=0.15, match_radius=0.03):
    """Steps 1-3 of grid_nn_ref.keypoint_pairs and the descriptors the planar-patch filter looks at: cen_normals = the normals
    of the two centroid clouds (the device's: the plane fit is held to a tolerance, not to bits, by its own tests).  -> dict(raw,
    cen, sel int64 [C], idx, d2, std float64 [C,2]); the two descriptor clouds must hold no edge pair."""
    raw = [np.asarray(src, dtype=np.float32), np.asarray(tgt, dtype=np.float32)]
    cen = [V.voxel_downsample(p, voxel_size)[0] for p in raw]
    desc = [point_fpfh(c, nrm, isolation_radius) for c, nrm in zip(cen, cen_normals)]
    assert all(d["edge_pairs"] == 0 for d in desc)
    keep = [G.nearest(c, c, isolation_radius, exclude_self=True)[0] >= 0 for c in cen]
    idx, d2 = G.nearest(cen[1], cen[0], match_radius, valid=keep[1])
    sel = np.nonzero(keep[0] & (idx >= 0))[0]
    fa, fb = desc[0]["fpfh"][sel], desc[1]["fpfh"][idx[sel]]
    std = np.stack((fa.astype(np.float64).std(axis=1), fb.astype(np.float64).std(axis=1)), axis=1)
    return dict(raw=raw, cen=cen, sel=sel, idx=idx, d2=d2, std=std, fa=fa, fb=fb, voxel_size=voxel_size)


def keypoint_pairs(cand, nonplanar_param, min_keypoints=128):
    """(keypoint_candidates' result) -> (rows int32 [P,2], src_centroid_row int32 [P], d2 float32 [P]): the candidates whose
    two descriptors both pass std_filter, none at all below min_keypoints of them, mapped to their nearest raw rows"""
    sel = cand["sel"][std_filter(cand["fa"], cand["fb"], nonplanar_param)]
    if sel.size < min_keypoints:
        sel = sel[:0]
    R = G.raw_radius(cand["voxel_size"])
    rows = np.stack((G.nearest(cand["raw"][0], cand["cen"][0][sel], R)[0],
                     G.nearest(cand["raw"][1], cand["cen"][1][cand["idx"][sel]], R)[0]), axis=1)
    return rows.astype(np.int32), sel.astype(np.int32), cand["d2"][sel]


# ------------------------------------------------------------------------------------------------ the GPU tests' inputs
def unit_normals(rng, n):
    v = rng.standard_normal((n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def case(points, normals, radius, max_radius=None, valid=None):
    return dict(points=np.ascontiguousarray(points, np.float32).reshape(-1, 3),
                normals=np.ascontiguousarray(normals, np.float32).reshape(-1, 3), radius=float(radius),
                max_radius=float(max_radius or radius), valid=valid)


def case_tiny(n):
    """n = 0..3 points, each within the radius of the others"""
    rng = np.random.default_rng(100 + n)
    return case(rng.uniform(0, 0.2, (n, 3)), unit_normals(rng, n), 0.5)


CLUSTERS = (1, 2, 64, 65, 66, 130, 258)


def case_clusters():
    """One tight cluster per entry of CLUSTERS, each inside ONE cell (the point at the origin fixes the cells' corner: a centre
    at a multiple of the edge sits mid-cell) and three cell edges from the next: a cluster of s points gives each of them s - 1
    neighbours -- 0, 1, 63, 64, 65 (the wave's stride), 129 and 257 -- and the cells hold 1 .. 258 records."""
    rng = np.random.default_rng(11)
    r = 0.25
    edge = float(G.cell_edge(r))
    pts = []
    for j, s in enumerate(CLUSTERS):
        centre = np.array([3 * edge * (j % 3), 3 * edge * (j // 3), 0.0])
        off = rng.uniform(0, 0.3 * r, (s, 3))
        off[0] = 0
        pts.append(centre + off)
    pts = np.vstack(pts)
    return case(pts, unit_normals(rng, pts.shape[0]), r)


def case_dense(radius_share=1.0, seed=5, n=700):
    """Uniform points in a box of 3.2 cell edges, the first 28 of them placed: row 0 at the origin fixes the cells' corner, row 1
    sits in the middle of cell (1, 1, 1) and rows 2..27 lie 0.55 edges from it along every combination of the axes -- one in each
    of the 26 cells around, all within the radius (0.55 sqrt 3 < 1).  radius_share < 1: a radius below the build's max_radius."""
    rng = np.random.default_rng(seed)
    r = 0.25
    edge = float(G.cell_edge(r))
    pts = rng.uniform(0, 3.2 * r, (n, 3))
    pts[0] = 0
    pts[1] = edge
    steps = [s for s in np.ndindex(3, 3, 3) if s != (1, 1, 1)]
    pts[2:28] = edge + 0.55 * edge * (np.array(steps) - 1)
    return case(pts, unit_normals(rng, n), r * radius_share, max_radius=r)


def case_edges():
    """Hand-made rows around the origin (normal +z), radius 0.5:
      1      at d2 == r2 exactly: a neighbour            2      one ulp beyond on the other side: nobody's neighbour
      3, 4   two rows at one place: d2 = 0 between them  5      on the origin's normal: d parallel to n, |v| == 0
      6..8   three rows at one far place: all of a point's neighbours coincide with it (no d2 > 0: the weighted sum is empty)
      9      a second copy of the origin"""
    rng = np.random.default_rng(21)
    beyond = np.nextafter(np.float32(0.5), np.float32(1))
    pts = np.array([[0, 0, 0], [0.5, 0, 0], [-beyond, 0, 0], [0.1, 0.25, 0.05], [0.1, 0.25, 0.05], [0, 0, 0.25],
                    [9, 9, 9], [9, 9, 9], [9, 9, 9], [0, 0, 0]], np.float32)
    nrm = unit_normals(rng, pts.shape[0])
    nrm[0] = nrm[5] = nrm[9] = [0, 0, 1]
    return case(pts, nrm, 0.5)


def case_collision(home=5):
    """64 occupied cells whose keys share one home slot at capacity 256, two points in each (n = 128): every lookup of the 27
    cells probes along the chain.  The twin is the only neighbour: the cells' spacing is above the radius."""
    rng = np.random.default_rng(31)
    max_radius = 2.0 ** -5 / (1 + 2.0 ** -10)
    pc, cells = V.colliding_cloud(128, home, span=48)
    pc, cells = pc[:64], cells[:64]
    twin = (pc + rng.uniform(0.0, 0.3 * 2.0 ** -5, pc.shape)).astype(np.float32)
    pts = np.vstack((pc, twin))
    out = case(pts, unit_normals(rng, 128), max_radius)
    out["cells"], out["home"] = np.vstack((cells, cells)), home
    return out


def case_nonfinite():
    """A dense cloud with NaN / inf coordinates at rows 3, 4, 5, NaN / inf normals at rows 10, 11, 12 (they stay neighbours) and
    a valid mask that leaves rows 20..29 out."""
    c = case_dense(seed=41, n=300)
    c["points"][3, 0] = np.nan
    c["points"][4, 1] = np.inf
    c["points"][5, 2] = -np.inf
    c["normals"][10, 0] = np.nan
    c["normals"][11, 2] = np.inf
    c["normals"][12] = [-np.inf, np.nan, 0]
    valid = np.ones(300, np.uint8)
    valid[20:30] = 0
    c["valid"] = valid
    return c


def gpu_cases():
    """{name: case}: every input of tests/test_gpu_fpfh.py's comparisons"""
    out = {f"n={n}": case_tiny(n) for n in range(4)}
    out.update(clusters=case_clusters(), dense=case_dense(), smaller_radius=case_dense(0.7), edges=case_edges(),
               collision=case_collision(), nonfinite=case_nonfinite())
    return out


def fragment_pair(n=6000, seed=3):
    """Two overlapping synthetic fragments in one frame for keypoint_pairs: a wavy floor and a wall, sampled twice with
    different noise.  -> (src float32 [n,3], tgt float32 [n,3])"""
    rng = np.random.default_rng(seed)

    def sample(shift):
        u = rng.uniform(0, 1.5, (n, 2))
        floor = np.stack((u[:, 0] + shift, u[:, 1], 0.05 * np.sin(5 * u[:, 0]) * np.cos(4 * u[:, 1])), axis=1)
        wall = np.stack((u[:, 0] + shift, 0.02 * np.sin(7 * u[:, 1]), u[:, 1]), axis=1)
        pick = rng.random(n) < 0.6
        return (np.where(pick[:, None], floor, wall) + rng.normal(0, 0.002, (n, 3))).astype(np.float32)

    return sample(0.0), sample(0.2)


def rigid_copy(points, seed=9):
    """(points float32 [n,3]) -> (the same points moved by a random rotation and shift, float32; R, t)"""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    t = rng.uniform(-0.5, 0.5, 3)
    return (np.asarray(points, np.float64) @ q.T + t).astype(np.float32), q, t
