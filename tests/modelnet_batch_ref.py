"""numpy fp64 restatement of the ModelNet batch entry (include/epn_so3conv.h: epn_modelnet_batch_f32),
independent of the kernel: a full sort for the selection (patch_ref.select, unchanged, with every point a member), plain numpy
for the normalisation, the rotation and the anchor label.

For cloud c with n_c rows and Q = ids[c] (default c):
    selection   n_c >= n_sample: the n_sample indices smallest in (key, i), ascending; n_c < n_sample: 0..n_c-1, then slot j is
                word1(Philox4x32-10({j, 0, lo32(Q), hi32(Q)}, seed)) mod n_c
    normalise   c = mean of the selected rows (duplicates counted), s = max |p - c|, p' = (p - c) / s, in fp64
    rotation    "random": Shoemake's quaternion from Philox4x32-10({0, 1, lo32(Q), hi32(Q)}, seed), u_k = (w[k] + 0.5) / 2^32;
                its matrix rounded once to fp32 is R; pc = R p' in fp64 from the rounded R, rounded once
    label       arg max_i tr(A_i^T R) in fp64, the lowest i on a tie; R_res = A_label^T R, rounded once
    status      8 bad offsets, else 1 empty, else 4 non-finite among the selected rows, else 2 zero extent; pc, pc_plain, R_res
                zeros and idx -1 for such a cloud."""
import numpy as np

import patch_ref as P
from philox_ref import philox4x32_10

F = np.float32
TOL = 2.0 ** -23            # outputs of magnitude <= 1: one fp32 rounding (2^-25) + a flipped rounding (2^-24), doubled


def select(n, Q, n_sample, seed, key_bits=32):
    """int32 [n_sample]: the selected rows of a cloud of n >= 1 points, before any status is applied."""
    if n == 1:                                          # patch_ref.select refuses one member (a patch needs two); here slot j
        return np.zeros(n_sample, dtype=np.int32)       # of a one-point cloud is word1 mod 1 = 0
    return P.select(np.arange(n), Q, n_sample, seed, key_bits)


def quat_matrix(w, x, y, z):
    """The standard unit-quaternion matrix, taken as it is (no normalisation)."""
    return np.array([[1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * z * w, 2 * x * z + 2 * y * w],
                     [2 * x * y + 2 * z * w, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * x * w],
                     [2 * x * z - 2 * y * w, 2 * y * z + 2 * x * w, 1 - 2 * x * x - 2 * y * y]], dtype=np.float64)


def random_rotation(Q, seed):
    """float32 [3,3]: the rotation of sample Q."""
    Q, seed = int(Q) & (2 ** 64 - 1), int(seed) & (2 ** 64 - 1)
    w = philox4x32_10([0, 1, Q & 0xFFFFFFFF, Q >> 32], [seed & 0xFFFFFFFF, seed >> 32])    # ctr_lo = 2^32
    u0, u1, u2 = ((float(w[k][0]) + 0.5) / 4294967296.0 for k in range(3))
    r1, r2 = np.sqrt(1.0 - u0), np.sqrt(u0)
    x, y = r1 * np.sin(2.0 * np.pi * u1), r1 * np.cos(2.0 * np.pi * u1)
    z, ww = r2 * np.sin(2.0 * np.pi * u2), r2 * np.cos(2.0 * np.pi * u2)
    return quat_matrix(ww, x, y, z).astype(F)


def anchor_label(anchors, R):
    """(anchors f32 [A,3,3], R f32 [3,3]) -> (label, R_res f32 [3,3], gap): tr(A_i^T R) = sum_e A_i[e] R[e] in fp64; gap is the
    best trace minus the runner-up (inf for one anchor)."""
    An, Rd = np.asarray(anchors, dtype=np.float64), np.asarray(R, dtype=np.float64)
    tr = np.zeros(An.shape[0])
    for e in range(9):                                  # row-major order, as specified: each product is exact in fp64
        tr = tr + An.reshape(-1, 9)[:, e] * Rd.reshape(9)[e]
    label = int(np.argmax(tr))                          # the first maximum: the lowest i on a tie
    rest = np.delete(tr, label)
    gap = float(tr[label] - rest.max()) if rest.size else float("inf")
    return label, (An[label].T @ Rd).astype(F), gap


def normalise(rows):
    """fp64 [n,3] -> (p' fp64 [n,3], s)."""
    rows = np.asarray(rows, dtype=np.float64)
    d = rows - rows.mean(axis=0, keepdims=True)
    s = np.sqrt((d * d).sum(axis=1).max())
    with np.errstate(invalid="ignore", divide="ignore"):
        return d / s, s


def modelnet_batch(points, offsets, n_sample, seed=0, ids=None, rotation="random", anchors=None, key_bits=32):
    """-> dict(pc, pc_plain f32 [B,n_sample,3], idx i32 [B,n_sample], R f32 [B,3,3], R_label i32 [B], R_res f32 [B,3,3],
    status i32 [B], gap f64 [B]); R_label, R_res and gap only with anchors.  rotation: "random", "none" or f32 [B,3,3]."""
    points = np.ascontiguousarray(points, dtype=F).reshape(-1, 3)
    offsets = np.asarray(offsets, dtype=np.int64)
    B, M = offsets.size - 1, points.shape[0]
    ids = np.arange(B) if ids is None else np.asarray(ids)
    out = dict(pc=np.zeros((B, n_sample, 3), F), pc_plain=np.zeros((B, n_sample, 3), F), idx=np.full((B, n_sample), -1, np.int32),
               R=np.zeros((B, 3, 3), F), status=np.zeros(B, np.int32))
    if anchors is not None:
        out.update(R_label=np.zeros(B, np.int32), R_res=np.zeros((B, 3, 3), F), gap=np.zeros(B))
    for c in range(B):
        Q = int(ids[c])
        if isinstance(rotation, str):
            R = random_rotation(Q, seed) if rotation == "random" else np.eye(3, dtype=F)
        else:
            R = np.asarray(rotation[c], dtype=F)
        out["R"][c] = R
        o0, o1 = int(offsets[c]), int(offsets[c + 1])
        st, sel, pn = 0, None, None
        if o0 < 0 or o1 > M or o1 < o0:
            st = 8
        elif o1 == o0:
            st = 1
        else:
            sel = select(o1 - o0, Q, n_sample, seed, key_bits)
            rows = points[o0:o1][sel]
            if not np.isfinite(rows).all():
                st = 4
            else:
                pn, s = normalise(rows)
                if not s > 0.0:
                    st = 2
        out["status"][c] = st
        if anchors is not None:
            label, res, gap = anchor_label(anchors, R)
            out["R_label"][c], out["gap"][c] = label, gap
            if st == 0:
                out["R_res"][c] = res
        if st == 0:
            out["idx"][c] = sel
            out["pc_plain"][c] = pn.astype(F)
            out["pc"][c] = (pn @ R.astype(np.float64).T).astype(F)
    return out


# ----------------------------------------------------------------------------------------------- the golden file's inputs
GOLDEN_SEED, GOLDEN_NSAMPLE = 5, 48
GOLDEN_SIZES = (48, 131, 20)                            # n_b == n_sample, above it, below it


def golden_clouds():
    """Three small raw clouds (f32, off-centre, not unit scale) -> (points [M,3], offsets [4])."""
    rng = np.random.default_rng(20260)
    clouds = [(rng.standard_normal((n, 3)) * (0.5 + i) + 3.0 * rng.standard_normal(3)).astype(F)
              for i, n in enumerate(GOLDEN_SIZES)]
    return np.concatenate(clouds), np.concatenate(([0], np.cumsum(GOLDEN_SIZES))).astype(np.int32)
