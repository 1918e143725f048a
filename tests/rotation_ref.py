"""numpy fp64 restatement of the rotation-estimation entries of include/epn_so3conv.h (epn_rotation_labels_f32,
epn_so3_mean_f32, epn_rotation_decode_f32) and the case tables of tests/test_gpu_rotation.py.

The restatement is written from the specification, not from the kernels: np.linalg.svd for the projection onto SO(3), a plain
loop over the pairs, np.einsum for the products.  Inputs are the fp32 arrays the device sees; everything after the conversion
is fp64 and nothing is rounded back, so a device result (fp64 inside, rounded once to fp32) lies within one fp32 rounding of
these values wherever the projection is well conditioned (margin, below).

The case tables are checked on the CPU by tests/test_rotation_spec.py: every label row has a fp64 gap above LABEL_GAP between
its best and second-best trace, every compared pair of a mean or decode case has margin >= MIN_MARGIN."""
import functools

import numpy as np

LABEL_GAP = 1e-9
MIN_MARGIN = 1e-3
EPS_ACOS = 1e-4
TET = [3, 4, 5, 27, 28, 29, 39, 40, 41, 48, 49, 50]         # the tetrahedral subgroup of the 60 anchors (tests/test_gpu_conv.py)


# ----------------------------------------------------------------------------------------------- the specification
def acos_safe(x, eps=EPS_ACOS):
    """vgtk/vgtk/spconv/functional.py:138-143 in fp64."""
    x = np.asarray(x, dtype=np.float64)
    slope = np.arccos(1 - eps) / eps
    sign = np.sign(x)
    inner = np.arccos(np.clip(x, -1, 1))
    return np.where(np.abs(x) <= 1 - eps, inner, np.arccos(sign * (1 - eps)) - slope * sign * (np.abs(x) - 1 + eps))


def _normalize(v):
    return v / np.maximum(np.sqrt((v * v).sum(-1, keepdims=True)), 1e-8)


def quat_matrix(q):
    """[..., 4] (w, x, y, z) -> [..., 3, 3]: rotation.py:379-417 (normalised by max(|q|, 1e-8) first)."""
    q = _normalize(np.asarray(q, dtype=np.float64))
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    rows = [1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * z * w, 2 * x * z + 2 * y * w,
            2 * x * y + 2 * z * w, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * x * w,
            2 * x * z - 2 * y * w, 2 * y * z + 2 * x * w, 1 - 2 * x * x - 2 * y * y]
    return np.stack(rows, axis=-1).reshape(q.shape[:-1] + (3, 3))


def ortho6d_matrix(v):
    """[..., 6] -> [..., 3, 3]: rotation.py:443-478, columns (x, y, z)."""
    v = np.asarray(v, dtype=np.float64)
    x = _normalize(v[..., 0:3])
    z = _normalize(np.cross(x, v[..., 3:6]))
    y = np.cross(z, x)
    return np.stack((x, y, z), axis=-1)


def label_relative_rotation(anchors, T):
    """(anchors f32 [A,3,3], T f32 [b,3,3]) -> (R_target f64 [b,A,3,3], label i32 [b,A], gap f64 [b,A]); gap is the difference
    between the best and the second-best trace (inf for A = 1)."""
    An, T = np.asarray(anchors, dtype=np.float64), np.asarray(T, dtype=np.float64)
    A = An.shape[0]
    M = np.einsum('abc,nbj,ijk->naick', An, T, An)            # [b, a, i, 3, 3] = A_a^T T A_i
    tr = np.einsum('naicc->nai', M)
    label = np.argmax(tr, axis=2)
    srt = np.sort(tr, axis=2)
    gap = srt[..., -1] - srt[..., -2] if A > 1 else np.full(label.shape, np.inf)
    R_target = np.take_along_axis(M, label[:, :, None, None, None], axis=2)[:, :, 0]
    return R_target, label.astype(np.int32), gap


def project(Ce):
    """Ce f64 [3,3] -> (the rotation maximising tr(R^T Ce), margin = (s2 + det(U V^T) s3) / s1)."""
    if not Ce.any():
        return np.eye(3), 0.0
    U, s, Vt = np.linalg.svd(Ce)
    d = np.linalg.det(U @ Vt)
    d = 1.0 if d > 0 else -1.0
    return U @ np.diag([1.0, 1.0, d]) @ Vt, (s[1] + d * s[2]) / s[0]


def so3_mean(Rs, weights=None):
    """(Rs f32 [b,N,3,3], weights f32 [b,N] or None) -> (R f64 [b,3,3], margin f64 [b])."""
    Rs = np.asarray(Rs, dtype=np.float64)
    w = np.ones(Rs.shape[:2]) if weights is None else np.asarray(weights, dtype=np.float64)
    out = [project(np.einsum('n,nij->ij', w[p], Rs[p])) for p in range(Rs.shape[0])]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out])


def decode(wts, y, anchors, label=None, gt_T=None):
    """The decode entry -> dict(pred_R [b,3,3], preds i32 [b,A], conf [b,A], margin [b], pred_Rs [b,A,3,3], hits i32 [b] or
    None, err [b] or None); everything but the integers in fp64."""
    wts, y, An = np.asarray(wts), np.asarray(y, dtype=np.float64), np.asarray(anchors, dtype=np.float64)
    assert wts.dtype == np.float32
    b, A = wts.shape[0], wts.shape[1]
    nr = y.shape[1]
    rot_map = quat_matrix if nr == 4 else ortho6d_matrix
    out = dict(pred_R=np.zeros((b, 3, 3)), preds=np.zeros((b, A), np.int32), conf=np.zeros((b, A)), margin=np.zeros(b),
               pred_Rs=np.zeros((b, A, 3, 3)), hits=None if label is None else np.zeros(b, np.int32),
               err=None if gt_T is None else np.zeros(b))
    for p in range(b):
        preds = np.argmax(wts[p], axis=0)                     # over the target anchors, the first maximum (fp32 comparison)
        c = wts[p][preds, np.arange(A)].astype(np.float64)
        conf = c / (1e-6 + c.sum())
        Ra = rot_map(y[p][:, preds, np.arange(A)].T)          # [A, 3, 3]
        pred_Rs = np.einsum('aij,ajk,alk->ail', An, Ra, An[preds])
        R, margin = project(np.einsum('a,aij->ij', conf, pred_Rs))
        out["preds"][p], out["conf"][p], out["pred_Rs"][p], out["pred_R"][p], out["margin"][p] = preds, conf, pred_Rs, R, margin
        if label is not None:
            out["hits"][p] = int((preds == np.asarray(label)[p]).sum())
        if gt_T is not None:
            out["err"][p] = acos_safe(0.5 * ((R * np.asarray(gt_T, dtype=np.float64)[p]).sum() - 1))
    return out


# ----------------------------------------------------------------------------------------------- helpers of the cases
def random_rotations(rng, n):
    q, r = np.linalg.qr(rng.standard_normal((n, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[:, :, 0] *= np.sign(np.linalg.det(q))[:, None]
    return q


def rot_to_quat(R):
    """[..., 3, 3] -> [..., 4] (w, x, y, z), fp64: the eigenvector form (the top eigenvector of Horn's matrix of R)."""
    R = np.asarray(R, dtype=np.float64)
    K = np.empty(R.shape[:-2] + (4, 4))
    K[..., 0, 0] = R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2]
    K[..., 1, 1] = R[..., 0, 0] - R[..., 1, 1] - R[..., 2, 2]
    K[..., 2, 2] = -R[..., 0, 0] + R[..., 1, 1] - R[..., 2, 2]
    K[..., 3, 3] = -R[..., 0, 0] - R[..., 1, 1] + R[..., 2, 2]
    K[..., 0, 1] = K[..., 1, 0] = R[..., 2, 1] - R[..., 1, 2]
    K[..., 0, 2] = K[..., 2, 0] = R[..., 0, 2] - R[..., 2, 0]
    K[..., 0, 3] = K[..., 3, 0] = R[..., 1, 0] - R[..., 0, 1]
    K[..., 1, 2] = K[..., 2, 1] = R[..., 0, 1] + R[..., 1, 0]
    K[..., 1, 3] = K[..., 3, 1] = R[..., 0, 2] + R[..., 2, 0]
    K[..., 2, 3] = K[..., 3, 2] = R[..., 1, 2] + R[..., 2, 1]
    return np.linalg.eigh(K)[1][..., -1]


def anchors_for(A):
    """f32 [A,3,3]: 60 the icosahedral table, 12 its tetrahedral subgroup, 1 the identity anchor, 64 random rotations (decode
    and mean need no group)."""
    import epn_pointcloud_amd
    epn_pointcloud_amd.install_vgtk_alias()
    import vgtk.so3conv.functional as L
    full = np.asarray(L.get_anchors(60), dtype=np.float32)
    if A == 60:
        return np.ascontiguousarray(full)
    if A == 12:
        return np.ascontiguousarray(full[TET])
    if A == 1:
        return np.ascontiguousarray(full[29:30])
    assert A == 64
    return np.ascontiguousarray(random_rotations(np.random.default_rng(6400), 64).astype(np.float32))


def orthogonality_defect(anchors):
    """max_a |A_a^T A_a - I|_max of the fp32 table, in fp64."""
    An = np.asarray(anchors, dtype=np.float64)
    return float(np.abs(np.einsum('aji,ajk->aik', An, An) - np.eye(3)).max())


# ----------------------------------------------------------------------------------------------- the case tables
A_SET, B_SET, NR_SET, N_SET = (1, 12, 60, 64), (1, 3, 65), (4, 6), (1, 60, 257)
LABEL_CASES = [(A, b, 100 + 10 * i + j) for i, A in enumerate(A_SET) for j, b in enumerate(B_SET)]
DECODE_CASES = [(A, b, nr, 200 + 20 * i + 2 * j + k) for i, A in enumerate(A_SET) for j, b in enumerate(B_SET)
                for k, nr in enumerate(NR_SET)]
MEAN_CASES = [(b, N, w, 300 + 10 * i + 2 * j + w) for i, b in enumerate(B_SET) for j, N in enumerate(N_SET) for w in (0, 1)]


@functools.lru_cache(maxsize=None)
def label_case(A, b, seed):
    """-> (anchors f32, T f32 [b,3,3], reference (R_target, label, gap))."""
    anchors = anchors_for(A)
    T = np.ascontiguousarray(random_rotations(np.random.default_rng(seed), b).astype(np.float32))
    return anchors, T, label_relative_rotation(anchors, T)


@functools.lru_cache(maxsize=None)
def decode_case(A, b, nr, seed):
    """-> (wts f32 [b,A,A], y f32 [b,nr,A,A], anchors f32, label i32 [b,A], gt_T f32 [b,3,3], reference dict).  Even pairs
    look like a trained head's output (confidence peaked near the label, y near the label's relative rotation, 0.2 of noise),
    odd pairs are noise: a softmax over random logits and Gaussian y."""
    rng = np.random.default_rng(seed)
    anchors = anchors_for(A)
    T = random_rotations(rng, b).astype(np.float32)
    R_target, label, _ = label_relative_rotation(anchors, T)
    logits = rng.standard_normal((b, A, A))
    y = rng.standard_normal((b, nr, A, A))
    for p in range(0, b, 2):
        logits[p][label[p], np.arange(A)] += 3.0
        good = rot_to_quat(R_target[p]) if nr == 4 else np.concatenate((R_target[p][:, :, 0], R_target[p][:, :, 1]), axis=1)
        y[p] = good.T[:, None, :] + 0.2 * rng.standard_normal((nr, A, A))
    e = np.exp(3.0 * (logits - logits.max(axis=1, keepdims=True)))
    wts = np.ascontiguousarray((e / e.sum(axis=1, keepdims=True)).astype(np.float32))
    y = np.ascontiguousarray(y.astype(np.float32))
    return wts, y, anchors, label, np.ascontiguousarray(T), decode(wts, y, anchors, label, T)


@functools.lru_cache(maxsize=None)
def mean_case(b, N, weighted, seed):
    """-> (Rs f32 [b,N,3,3], weights f32 [b,N] or None, reference (R, margin)).  Even pairs scatter within about 0.5 rad of a
    centre, odd pairs are uniform over SO(3)."""
    rng = np.random.default_rng(seed)
    Rs = random_rotations(rng, b * N).reshape(b, N, 3, 3)
    for p in range(0, b, 2):
        centre = random_rotations(rng, 1)[0]
        q = np.concatenate((np.ones((N, 1)), 0.25 * rng.standard_normal((N, 3))), axis=1)
        Rs[p] = centre @ quat_matrix(q)
    Rs = np.ascontiguousarray(Rs.astype(np.float32))
    weights = np.ascontiguousarray(rng.uniform(0.05, 1.0, (b, N)).astype(np.float32)) if weighted else None
    return Rs, weights, so3_mean(Rs, weights)


@functools.lru_cache(maxsize=None)
def round_trip_case(A, nr, seed=77, b=3):
    """An ideal head output for random T: wts peaked at the label, y the exact representation (rounded to fp32) of
    R_target[a] on every target row.  -> (wts, y, anchors, label, T f32, reference dict)."""
    anchors = anchors_for(A)
    T = np.ascontiguousarray(random_rotations(np.random.default_rng(seed), b).astype(np.float32))
    R_target, label, _ = label_relative_rotation(anchors, T)
    wts = np.full((b, A, A), 0.1 / A, np.float32)
    y = np.zeros((b, nr, A, A), np.float32)
    for p in range(b):
        wts[p][label[p], np.arange(A)] += np.float32(0.9)
        good = rot_to_quat(R_target[p]) if nr == 4 else np.concatenate((R_target[p][:, :, 0], R_target[p][:, :, 1]), axis=1)
        y[p] = good.T[:, None, :]
    return wts, y, anchors, label, T, decode(wts, y, anchors, label, T)


def round_trip_defect(case):
    """(max |pred_R - T|, max |err|) of the restatement on a round-trip case: what the fp32 anchors, T and y leave."""
    T, ref = case[4], case[5]
    return float(np.abs(ref["pred_R"] - T.astype(np.float64)).max()), float(np.abs(ref["err"]).max())
