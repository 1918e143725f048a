"""Numpy restatement of the normals specification (include/epn_so3conv.h: epn_point_normals_f32, epn_orient_patches_f32;
DESIGN.md 3.1k), written from the specification and not from the kernel: the in-radius sets are brute force over all points with
no grid at all, the cut sorts (d2 bits, row) keys, the moments are integer sums of np.rint in float64, and the eigen-solve is
numpy.linalg.eigh -- another algorithm than the kernel's Jacobi, which is what the one tolerance of the tests is about."""
import numpy as np

FIX = 2.0 ** 40
GAP_MIN = 2.0 ** -40
FLAG_FEW, FLAG_QUERY, FLAG_GAP = 1, 2, 4
C_JACOBI = 82.0           # the constant of normal_bound / eig_bound: 8 x the worst ratio observed on the host, 10.22


def member_keys(ref, q, radius):
    """-> uint64 keys d2 bits << 32 | row of the in-radius set of ONE query, ascending.  d2 = (dx*dx + dy*dy) + dz*dz in float32
    arrays (numpy rounds every operation), r2 = float32 of the float64 product, inclusive; a non-finite point is never in."""
    ref = np.asarray(ref, dtype=np.float32).reshape(-1, 3)
    q = np.asarray(q, dtype=np.float32).reshape(3)
    if ref.shape[0] == 0 or not np.isfinite(q).all():
        return np.zeros(0, np.uint64)
    r2 = np.float32(np.float64(radius) * np.float64(radius))
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = ref[:, 0] - q[0], ref[:, 1] - q[1], ref[:, 2] - q[2]
        d2 = (dx * dx + dy * dy) + dz * dz
        inside = (d2 <= r2) & np.isfinite(ref).all(axis=1)
    rows = np.nonzero(inside)[0]
    keys = (d2[rows].view(np.uint32).astype(np.uint64) << np.uint64(32)) | rows.astype(np.uint64)
    return np.sort(keys)


def neighbourhood(ref, q, radius, max_nn):
    """-> (count, rows int32 [used] in ascending key order): the cut keeps the max_nn smallest keys."""
    keys = member_keys(ref, q, radius)
    used = keys if max_nn == 0 else keys[:max_nn]
    return keys.size, (used & np.uint64(0xFFFFFFFF)).astype(np.int32)


def moments_of(ref, q, rows, radius):
    """-> int64 [9] = {S_x, S_y, S_z, M_xx, M_xy, M_xz, M_yy, M_yz, M_zz}"""
    ref = np.asarray(ref, dtype=np.float32).reshape(-1, 3)
    t = (ref[rows].astype(np.float64) - np.asarray(q, dtype=np.float32).astype(np.float64)) / np.float64(radius)
    S = np.rint(t * FIX).astype(np.int64).sum(axis=0)
    M = [np.rint((t[:, i] * t[:, j]) * FIX).astype(np.int64).sum() for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    return np.concatenate((S, np.array(M, dtype=np.int64))).astype(np.int64)


def covariance(mom, used):
    """-> C float64 [3,3] from the moments, every operation rounded on its own"""
    mom = np.asarray(mom, dtype=np.int64)
    k = np.float64(used)
    mean = (mom[:3].astype(np.float64) / FIX) / k
    second = (mom[3:].astype(np.float64) / FIX) / k
    C = np.empty((3, 3))
    for e, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        C[i, j] = C[j, i] = second[e] - mean[i] * mean[j]
    return C


def orient(n, q, view):
    n = np.array(n, dtype=np.float64)
    if view is not None:
        d = np.asarray(view, dtype=np.float32).astype(np.float64) - np.asarray(q, dtype=np.float32).astype(np.float64)
        flip = (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2] < 0.0
    else:
        flip = n[int(np.argmax(np.abs(n)))] < 0.0                  # argmax: the first of equal maxima, the lowest axis
    return -n if flip else n


def plane_fit(mom, used, q, view=None):
    """-> (normal float64 [3], lam float64 [3] ascending in the units of C, flags): eigh on C from the moments"""
    if used < 3:
        return np.array([0.0, 0.0, 1.0]), np.zeros(3), FLAG_FEW
    lam, vec = np.linalg.eigh(covariance(mom, used))
    n = vec[:, 0] / np.linalg.norm(vec[:, 0])
    return orient(n, q, view), lam, (FLAG_GAP if lam[1] - lam[0] <= GAP_MIN else 0)


def point_normals(ref, qry, radius, max_nn=30, view=None):
    """-> dict(normals f64 [m,3], lam f64 [m,3], eig f64 [m,3] = lam * radius^2, count, flags, moments int64 [m,9],
    neighbors: list of int32 rows per query).  normals and eig are left in float64: the tests round and bound them."""
    ref = np.asarray(ref, dtype=np.float32).reshape(-1, 3)
    qry = np.asarray(qry, dtype=np.float32).reshape(-1, 3)
    m = qry.shape[0]
    out = dict(normals=np.zeros((m, 3)), lam=np.zeros((m, 3)), eig=np.zeros((m, 3)), count=np.zeros(m, np.int32),
               flags=np.zeros(m, np.int32), moments=np.zeros((m, 9), np.int64), neighbors=[])
    for i in range(m):
        count, rows = neighbourhood(ref, qry[i], radius, max_nn)
        mom = moments_of(ref, qry[i], rows, radius)
        n, lam, flags = plane_fit(mom, rows.size, qry[i], view)
        if not np.isfinite(qry[i]).all():
            flags |= FLAG_QUERY
        out["normals"][i], out["lam"][i], out["eig"][i] = n, lam, lam * (np.float64(radius) * np.float64(radius))
        out["count"][i], out["flags"][i], out["moments"][i] = count, flags, mom
        out["neighbors"].append(rows)
    return out


def neighbor_table(neighbors, max_nn):
    """the rows per query as the entry point writes them: int32 [m,max_nn], -1 beyond used"""
    t = np.full((len(neighbors), max_nn), -1, np.int32)
    for i, rows in enumerate(neighbors):
        t[i, :rows.size] = rows
    return t


def normal_bound(lam, c=C_JACOBI):
    """per component |n - n_ref| <= 2^-23 + c 2^-52 lam2 / (lam1 - lam0): the fp32 rounding of both sides (half an ulp of a value
    below 1 each) and the eigenvector's first-order sensitivity to a backward error of c 2^-52 |C|, |C| = lam2."""
    lam = np.asarray(lam, dtype=np.float64).reshape(-1, 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 2.0 ** -23 + c * 2.0 ** -52 * lam[:, 2] / (lam[:, 1] - lam[:, 0])


def eig_bound(lam, radius, c=C_JACOBI):
    """|eig - eig_ref| <= 2^-23 |eig_ref| + c 2^-52 |C| radius^2 with |C| = max |lam|: an eigenvalue of a symmetric matrix moves
    by at most the norm of the backward error; the first term is the fp32 rounding of both sides."""
    lam = np.asarray(lam, dtype=np.float64).reshape(-1, 3)
    r2 = np.float64(radius) * np.float64(radius)
    return 2.0 ** -23 * np.abs(lam) * r2 + (c * 2.0 ** -52 * np.abs(lam).max(axis=1) * r2)[:, None]


# ------------------------------------------------------------------------------------------------ patch frames
def _unit_eps(v):
    return v / (np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + 1e-5)


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def patch_frame(normal):
    """-> axis float32 [3,3] with x, y, z as columns: float64 throughout, rounded once"""
    n = np.asarray(normal, dtype=np.float32).astype(np.float64)
    up = np.array([0.0, -1.0, 0.0])
    z = _unit_eps(n)
    x = _unit_eps(_cross(up, z))
    y = _unit_eps(_cross(z, x))
    return np.stack((x, y, z), axis=1).astype(np.float32)


def orient_patches(patches, normals):
    """-> (out float32 [k,n_sample,3], axis float32 [k,3,3]): out = patch @ axis, ((p0 a0 + p1 a1) + p2 a2) in float64 from the
    rounded axis, rounded once"""
    patches = np.asarray(patches, dtype=np.float32)
    axis = np.stack([patch_frame(n) for n in np.asarray(normals, dtype=np.float32).reshape(-1, 3)]) if len(normals) else \
        np.zeros((0, 3, 3), np.float32)
    p, a = patches.astype(np.float64), axis.astype(np.float64)
    out = (p[:, :, 0, None] * a[:, None, 0, :] + p[:, :, 1, None] * a[:, None, 1, :]) + p[:, :, 2, None] * a[:, None, 2, :]
    return out.astype(np.float32), axis


# ------------------------------------------------------------------------------------------------ shared clouds
def noisy_sphere(n=2000, radius=1.0, noise=0.01, seed=5):
    """n points on a sphere about the origin with radial noise; the outward direction is points / |points|"""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((n, 3))
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    return (g * (radius + noise * rng.standard_normal((n, 1)))).astype(np.float32)
