"""numpy restatement of the 3DMatch batch entry (include/epn_so3conv.h: epn_fragment_pair_batch_f32),
independent of the kernel: patch_ref (brute force, a full sort) for the patches, plain numpy for the draws, the Euler rotation
and the transforms.

For sample b with id = ids[b] (default b), side s (0 source, 1 target), slot j: Q' = (id * 2 + s) * npt + j.
    choice      word0(Philox4x32-10({0, 1, lo32(Q'(0,j)), hi32(Q'(0,j))}, seed)) mod P_b            (ctr_lo = 2^32)
    patch       patch_ref.radius_patches of the side's fragment, keypoint corr[choice, s], kpt_row0 = Q'
    rotation    w = Philox4x32-10({1, 1, lo32(Q'(s,0)), hi32(Q'(s,0))}, seed), d_k = w[k] mod max_degree  (ctr_lo = 2^32 + 1);
                R = Rz(d2) Ry(d1) Rx(d0) in fp64 at angles (d * pi) / 180, rounded once
    values      ((r0 x + r1 y) + r2 z) in fp64 from the rounded R and the fp32 difference p - center * q, rounded once
    T, T_aug    R_A^T R_B from the poses; (R_aug_src T) R_aug_tgt^T from the rounded matrices; fp64, rounded once
    status      8 bad pairs / offsets / corr_offsets, else 1 no correspondences, else 4 non-finite pose or chosen keypoint"""
import numpy as np

import patch_ref as P

F = np.float32
TOL = 2.0 ** -23            # entries of magnitude <= 1: one fp32 rounding of an fp64 result
_M64 = 2 ** 64 - 1


def stream(id_, s, j, npt):
    """Q'(s, j) of sample id_, modulo 2^64 as the kernel computes it."""
    return ((int(id_) * 2 + s) * npt + j) & _M64


def choices(id_, npt, P_b, seed):
    """int64 [npt]: the correspondences of a sample with P_b >= 1 of them."""
    return np.array([int(P._words(1 << 32, stream(id_, 0, j, npt), seed)[0][0]) % P_b for j in range(npt)], dtype=np.int64)


def degrees(id_, s, npt, seed, max_degree):
    """The three integer Euler angles of side s, in degrees."""
    if max_degree == 0:
        return (0, 0, 0)
    w = P._words((1 << 32) + 1, stream(id_, s, 0, npt), seed)
    return tuple(int(w[k][0]) % max_degree for k in range(3))


def euler_matrix(deg):
    """fp64 [3,3]: Rz(d2) Ry(d1) Rx(d0), the reference's R_from_euler_np at np.random.randint(...) * np.pi / 180.0."""
    a = np.asarray(deg, dtype=np.int64) * np.pi / 180.0
    c, s = np.cos(a), np.sin(a)
    Rx = np.array([[1, 0, 0], [0, c[0], -s[0]], [0, s[0], c[0]]], dtype=np.float64)
    Ry = np.array([[c[1], 0, s[1]], [0, 1, 0], [-s[1], 0, c[1]]], dtype=np.float64)
    Rz = np.array([[c[2], -s[2], 0], [s[2], c[2], 0], [0, 0, 1]], dtype=np.float64)
    return Rz @ (Ry @ Rx)


def augmentation(id_, s, npt, seed, max_degree):
    """float32 [3,3]: R_aug of side s."""
    return euler_matrix(degrees(id_, s, npt, seed, max_degree)).astype(F)


def rotate(R, diff):
    """(R f32 [3,3], diff f32 [n,3]) -> f32 [n,3]: each component ((r0 x + r1 y) + r2 z) in fp64, rounded once."""
    R, d = np.asarray(R, dtype=F).astype(np.float64), np.asarray(diff, dtype=F).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([(R[r, 0] * d[:, 0] + R[r, 1] * d[:, 1]) + R[r, 2] * d[:, 2] for r in range(3)], axis=1).astype(F)


def patch_values(pc, idx_row, kpt, center, R):
    """The patch row (f32 [n_sample,3]) for an idx row of a fragment: zeros where idx is -1."""
    pc = np.asarray(pc, dtype=F).reshape(-1, 3)
    out = np.zeros((idx_row.size, 3), dtype=F)
    ok = idx_row >= 0
    if ok.any():
        c = np.asarray(kpt, dtype=F) if center else np.zeros(3, dtype=F)
        out[ok] = rotate(R, pc[idx_row[ok]] - c[None, :])        # fp32 - fp32: one rounding
    return out


def relative_rotation(poseA, poseB):
    """float32 [3,3]: R_A^T R_B, each entry ((a0 b0 + a1 b1) + a2 b2) in fp64, rounded once."""
    A, B = np.asarray(poseA, dtype=np.float64)[:3, :3], np.asarray(poseB, dtype=np.float64)[:3, :3]
    return np.array([[(A[0, r] * B[0, c] + A[1, r] * B[1, c]) + A[2, r] * B[2, c] for c in range(3)] for r in range(3)]).astype(F)


def augmented_transform(Rs, T, Rt):
    """float32 [3,3]: (R_aug_src T) R_aug_tgt^T from the rounded matrices."""
    Rs, T, Rt = (np.asarray(x, dtype=F).astype(np.float64) for x in (Rs, T, Rt))
    U = np.array([[(Rs[r, 0] * T[0, c] + Rs[r, 1] * T[1, c]) + Rs[r, 2] * T[2, c] for c in range(3)] for r in range(3)])
    return np.array([[(U[r, 0] * Rt[c, 0] + U[r, 1] * Rt[c, 1]) + U[r, 2] * Rt[c, 2] for c in range(3)] for r in range(3)]).astype(F)


def fragment_pair_batch(points, offsets, pairs, corr, corr_offsets, poses, n_sample, npt, radius, seed=0, ids=None, max_degree=30,
                        center=0, key_bits=32, R_aug=None):
    """-> dict(src, tgt f32 [B,npt,n_sample,3], idx i32 [B,2,npt,n_sample], counts i32 [B,2,npt], choice i32 [B,npt],
    T f32 [B,3,3], R_aug f32 [B,2,3,3], T_aug f32 [B,3,3], status i32 [B]).  R_aug given ([B,2,3,3]): the patch values and T_aug
    are evaluated from it instead of the restatement's own rotations (a device's, say)."""
    points = np.ascontiguousarray(points, dtype=F).reshape(-1, 3)
    corr = np.ascontiguousarray(corr, dtype=F).reshape(-1, 2, 3)
    offsets, corr_offsets = np.asarray(offsets, dtype=np.int64), np.asarray(corr_offsets, dtype=np.int64)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    B, Fn, M, C = pairs.shape[0], offsets.size - 1, points.shape[0], corr.shape[0]
    ids = np.arange(B) if ids is None else np.asarray(ids)
    out = dict(src=np.zeros((B, npt, n_sample, 3), F), tgt=np.zeros((B, npt, n_sample, 3), F),
               idx=np.full((B, 2, npt, n_sample), -1, np.int32), counts=np.zeros((B, 2, npt), np.int32),
               choice=np.full((B, npt), -1, np.int32), T=np.zeros((B, 3, 3), F), R_aug=np.zeros((B, 2, 3, 3), F),
               T_aug=np.zeros((B, 3, 3), F), status=np.zeros(B, np.int32))
    for b in range(B):
        id_ = int(ids[b])
        for s in (0, 1):
            out["R_aug"][b, s] = augmentation(id_, s, npt, seed, max_degree) if R_aug is None else np.asarray(R_aug[b, s], dtype=F)
        st = 0
        for f in pairs[b]:
            if f < 0 or f >= Fn or offsets[f] < 0 or offsets[f + 1] > M or offsets[f + 1] < offsets[f]:
                st = 8
        c0, c1 = int(corr_offsets[b]), int(corr_offsets[b + 1])
        if c0 < 0 or c1 > C or c1 < c0:
            st = 8
        if st == 0 and c1 == c0:
            st = 1
        if st == 0:
            ch = choices(id_, npt, c1 - c0, seed)
            if not (np.isfinite(poses[pairs[b]]).all() and np.isfinite(corr[c0 + ch]).all()):
                st = 4
        out["status"][b] = st
        if st:
            continue
        out["choice"][b] = ch
        out["T"][b] = relative_rotation(poses[pairs[b, 0]], poses[pairs[b, 1]])
        out["T_aug"][b] = augmented_transform(out["R_aug"][b, 0], out["T"][b], out["R_aug"][b, 1])
        for s, name in ((0, "src"), (1, "tgt")):
            f = pairs[b, s]
            pc = points[offsets[f]:offsets[f + 1]]
            for j in range(npt):
                kpt = corr[c0 + ch[j], s]
                idx, counts, _ = P.radius_patches(pc, kpt[None], radius, n_sample, seed=seed, kpt_row0=stream(id_, s, j, npt),
                                                  key_bits=key_bits)
                out["idx"][b, s, j], out["counts"][b, s, j] = idx[0], counts[0]
                out[name][b, j] = patch_values(pc, idx[0], kpt, center, out["R_aug"][b, s])
    return out


# ----------------------------------------------------------------------------------------------- the golden file's inputs
GOLDEN_SEED, GOLDEN_NSAMPLE, GOLDEN_NPT, GOLDEN_RADIUS, GOLDEN_MAX_DEGREE = 11, 8, 3, 0.3, 30
GOLDEN_SIZES = (150, 90, 120)                           # three fragments
GOLDEN_PAIRS = ((0, 1), (2, 0))                         # fragment 0 serves both samples
GOLDEN_BOUNDARY = 1e-4                                  # no point within this relative distance of the radius


def golden_inputs():
    """-> (points f32 [M,3], offsets i32 [4], pairs i32 [2,2], corr f32 [C,2,3], corr_offsets i32 [3], poses f64 [3,4,4]): three
    fragments of one scene seen from three poses; the correspondences are scene points (three of seven moved away from the
    scene), in each fragment's frame."""
    rng = np.random.default_rng(30303)
    poses, frags = [], []
    scene = rng.random((400, 3))
    for n in GOLDEN_SIZES:
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        q = q * np.sign(np.linalg.det(q))
        pose = np.eye(4)
        pose[:3, :3], pose[:3, 3] = q, rng.standard_normal(3)
        poses.append(pose)
        world = scene[rng.choice(400, n, replace=False)]
        frags.append(((world - pose[:3, 3]) @ q).astype(F))          # x_frag = R^T (x_world - t)
    corr, sizes = [], []
    for a, b in GOLDEN_PAIRS:
        k = scene[rng.choice(400, 7, replace=False)]
        k[4:] += 3.0                                                 # keypoints with nothing around them: empty patches
        corr.append(np.stack([((k - poses[f][:3, 3]) @ poses[f][:3, :3]).astype(F) for f in (a, b)], axis=1))
        sizes.append(7)
    off = np.concatenate(([0], np.cumsum(GOLDEN_SIZES))).astype(np.int32)
    coff = np.concatenate(([0], np.cumsum(sizes))).astype(np.int32)
    return (np.concatenate(frags), off, np.asarray(GOLDEN_PAIRS, dtype=np.int32), np.concatenate(corr), coff, np.stack(poses))
