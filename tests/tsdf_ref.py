"""Numpy restatement of the TSDF fusion specification (include/epn_so3conv.h: epn_tsdf_fuse_f32, epn_tsdf_extract_f32; DESIGN.md
3.1l).  fp64 throughout, every operation a numpy ufunc of its own (numpy never fuses a product into a sum), the fp32 steps formed
with np.float32 operations in the stated order.  The GPU tests compare every output with this bit for bit."""
import numpy as np

UNIT = 16
FLAG_OUTSIDE, FLAG_BLOCKS = 1, 2
FLAG_POINTS = 1
BAND = np.float32(0.98)
F32_1 = np.float32(1.0)


def depth_values(depth, depth_scale, depth_trunc):
    """u16 [...] -> f32 [...]: (float)raw / (float)depth_scale, 0 where raw == 0 or the value exceeds depth_trunc"""
    d = depth.astype(np.float32) / np.float32(depth_scale)
    d[(depth == 0) | (d.astype(np.float64) > float(depth_trunc))] = 0
    return d


def transform(T, p):
    """((T_i0 p_0 + T_i1 p_1) + T_i2 p_2) + T_i3 on the last axis of p"""
    return np.stack([((T[i, 0] * p[..., 0] + T[i, 1] * p[..., 1]) + T[i, 2] * p[..., 2]) + T[i, 3] for i in range(3)], axis=-1)


def back_project(u, v, d, K):
    fx, fy, cx, cy = K
    z = d.astype(np.float64)
    return np.stack((((u - cx) * z) / fx, ((v - cy) * z) / fy, z), axis=-1)


def sample_points(depth, cam2base, K, depth_scale, depth_trunc, stride, f):
    """the touch's samples of frame f in the base frame: f64 [n,3] (row-major over the sampled pixels with a measurement)"""
    d = depth_values(depth[f], depth_scale, depth_trunc)
    H, W = d.shape
    v, u = np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), indexing="ij")
    dd = d[v, u]
    keep = dd != 0
    return transform(cam2base[f], back_project(u[keep].astype(np.float64), v[keep].astype(np.float64), dd[keep], K))


def touch(depth, cam2base, K, depth_scale, depth_trunc, voxel_length, sdf_trunc, stride, unit_lo, unit_dims):
    """-> (masks u64 [D], n_outside)"""
    lo_box, dims = np.asarray(unit_lo, dtype=np.float64), np.asarray(unit_dims, dtype=np.int64)
    unit_length = 16.0 * voxel_length
    masks = np.zeros(int(dims.prod()), dtype=np.uint64)
    n_outside = 0
    for f in range(depth.shape[0]):
        p = sample_points(depth, cam2base, K, depth_scale, depth_trunc, stride, f)
        with np.errstate(invalid="ignore"):
            lo = np.floor((p - sdf_trunc) / unit_length)
            hi = np.floor((p + sdf_trunc) / unit_length)
            outside = np.zeros(p.shape[0], dtype=bool)
            for k in range(8):
                pick = np.array([k >> 2 & 1, k >> 1 & 1, k & 1], dtype=bool)
                again = (pick[None, :] & (hi == lo)).any(axis=1)      # the same unit as a corner already visited
                rel = np.where(pick[None, :], hi, lo) - lo_box
                inside = ((rel >= 0) & (rel < dims)).all(axis=1)
                outside |= ~again & ~inside
                r = rel[~again & inside].astype(np.int64)
                e = (r[:, 0] * dims[1] + r[:, 1]) * dims[2] + r[:, 2]
                masks[np.unique(e)] |= np.uint64(1) << np.uint64(f)
        n_outside += int(outside.sum())
    return masks, n_outside


def fuse(depth, cam2base, base2cam, K, unit_lo, unit_dims, max_blocks, depth_scale=1000.0, depth_trunc=6.0, voxel_length=3.0 / 512,
         sdf_trunc=0.04, stride=4):
    """-> dict(n_blocks, flags, n_outside, block_unit i32 [nb,3], block_mask u64 [nb], tsdf f32 [nb,16,16,16], weight i32 alike),
    nb = min(n_blocks, max_blocks): the rows the device writes"""
    fx, fy, cx, cy = K
    F, H, W = depth.shape
    dims = np.asarray(unit_dims, dtype=np.int64)
    masks, n_outside = touch(depth, cam2base, K, depth_scale, depth_trunc, voxel_length, sdf_trunc, stride, unit_lo, unit_dims)
    alloc = np.nonzero(masks)[0]
    n_blocks = alloc.size
    nb = min(n_blocks, max_blocks)
    flags = (FLAG_OUTSIDE if n_outside else 0) | (FLAG_BLOCKS if n_blocks > max_blocks else 0)
    alloc = alloc[:nb]
    block_unit = (np.stack(np.unravel_index(alloc, tuple(dims)), axis=1) + np.asarray(unit_lo)).astype(np.int32).reshape(nb, 3)
    block_mask = masks[alloc]
    idx = np.arange(UNIT)
    centre = [((16 * block_unit[:, a].astype(np.int64)[:, None] + idx[None, :]).astype(np.float64) + 0.5) * voxel_length for a in range(3)]
    P = np.stack(np.broadcast_arrays(centre[0][:, :, None, None], centre[1][:, None, :, None], centre[2][:, None, None, :]), axis=-1)
    tsdf = np.zeros((nb, UNIT, UNIT, UNIT), dtype=np.float32)
    weight = np.zeros((nb, UNIT, UNIT, UNIT), dtype=np.int32)
    d = depth_values(depth, depth_scale, depth_trunc)
    for f in range(F):
        rows = np.nonzero((block_mask >> np.uint64(f)) & np.uint64(1))[0]
        if rows.size == 0:
            continue
        c = transform(base2cam[f], P[rows])
        with np.errstate(all="ignore"):
            ok = c[..., 2] > 0
            uf = ((c[..., 0] * fx) / c[..., 2] + cx) + 0.5
            vf = ((c[..., 1] * fy) / c[..., 2] + cy) + 0.5
            ok &= (uf >= 0) & (uf < W) & (vf >= 0) & (vf < H)
            pu, pv = np.where(ok, uf, 0).astype(np.int64), np.where(ok, vf, 0).astype(np.int64)
            dd = d[f][pv, pu]
            ok &= dd != 0
            a, b = (pu.astype(np.float64) - cx) / fx, (pv.astype(np.float64) - cy) / fy
            sdf = (dd.astype(np.float64) - c[..., 2]) * np.sqrt((a * a + b * b) + 1.0)
            ok &= sdf > -sdf_trunc
            q = sdf / sdf_trunc
            t = np.where(q < 1.0, q, 1.0).astype(np.float32)
            fw = weight[rows].astype(np.float32)
            new = (tsdf[rows] * fw + t) / (fw + F32_1)
        assert new.dtype == np.float32
        tsdf[rows] = np.where(ok, new, tsdf[rows])
        weight[rows] += ok
    return dict(n_blocks=n_blocks, flags=flags, n_outside=n_outside, block_unit=block_unit, block_mask=block_mask, tsdf=tsdf,
                weight=weight)


def extract(tsdf, weight, block_unit, unit_lo, unit_dims, voxel_length, max_points=None):
    """the rows a fuse wrote -> (points f32 [min(M, max_points),3], M, flags)"""
    nb = tsdf.shape[0]
    lo, dims = np.asarray(unit_lo), np.asarray(unit_dims)
    part = (weight != 0) & (tsdf >= -BAND) & (tsdf < BAND)
    val = np.where(part, tsdf, np.float32(np.nan))
    rank = {tuple(int(x) for x in u): r for r, u in enumerate(block_unit)
            if ((u - lo >= 0) & (u - lo < dims)).all()}
    out = []
    for r in range(nb):
        f0 = val[r]
        unit = block_unit[r].astype(np.int64)
        centre = [((16 * unit[a] + np.arange(UNIT)).astype(np.float64) + 0.5) * voxel_length for a in range(3)]
        C = np.stack(np.broadcast_arrays(centre[0][:, None, None], centre[1][None, :, None], centre[2][None, None, :]), axis=-1)
        hits, f1s = [], []
        for a in range(3):
            e = unit.copy()
            e[a] += 1
            n = rank.get(tuple(int(x) for x in e))
            face = np.full((UNIT, UNIT), np.nan, dtype=np.float32) if n is None else np.take(val[n], 0, axis=a)
            f1 = np.concatenate((np.delete(f0, 0, axis=a), np.expand_dims(face, a)), axis=a)
            with np.errstate(invalid="ignore"):
                hits.append(~np.isnan(f0) & ~np.isnan(f1) & (f0.astype(np.float64) * f1.astype(np.float64) < 0))
            f1s.append(f1)
        hit = np.stack(hits, axis=-1)
        for x, y, z, a in zip(*np.nonzero(hit)):                       # C order: x, y, z, then the axis
            p = C[x, y, z].copy()
            r0, r1 = abs(np.float64(f0[x, y, z])), abs(np.float64(f1s[a][x, y, z]))
            p0 = p[a]
            p[a] = (p0 * r1 + (p0 + voxel_length) * r0) / (r0 + r1)
            out.append(p.astype(np.float32))
    M = len(out)
    pts = np.array(out, dtype=np.float32).reshape(M, 3)
    if max_points is None:
        return pts, M, 0
    return pts[:max_points], M, FLAG_POINTS if M > max_points else 0


def render_plane(H, W, K, cam2base, normal, offset, depth_scale=1000.0):
    """depth u16 [H,W] of the plane {x : normal . x = offset} (base frame) seen by a camera: the z-depth along every pixel's ray,
    rounded to the nearest raw unit; 0 where the ray misses or the raw value leaves 1..65535"""
    fx, fy, cx, cy = K
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ray = np.stack(((u - cx) / fx, (v - cy) / fy, np.ones_like(u)), axis=-1) @ cam2base[:3, :3].T
    with np.errstate(all="ignore"):
        z = (offset - np.dot(cam2base[:3, 3], normal)) / (ray @ np.asarray(normal, dtype=np.float64))
        raw = np.rint(z * depth_scale)
    raw[~np.isfinite(raw) | (raw < 1) | (raw > 65535)] = 0
    return raw.astype(np.uint16)
