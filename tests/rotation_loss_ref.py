"""numpy fp64 restatement of the rotation network's training loss (include/epn_so3conv.h: epn_rotation_loss_f32 and
epn_rotation_loss_bwd_f32) and the case tables of tests/test_gpu_rotation_loss.py.

Written from the specification, not from the kernels: the forward with numpy over all rows at once, the backward as the explicit
Jacobian of the rotation map (forward mode: a product of small matrices per row; the kernels go through it in reverse).  Inputs
are the fp32 arrays the device sees; everything after the conversion is fp64 and nothing is rounded back except where the
specification rounds (the scalars are sums of the ROUNDED per-row outputs).

Next to every value the restatement returns the magnitude the GPU test's tolerance needs: the sum of the absolute values of the
terms that were added to form it (and, for the rotation map, its conditioning), see test_gpu_rotation_loss.py.

Inputs of the table cases are rotation_ref.decode_case(A, b, nr, seed) plus R_target from rotation_ref.label_relative_rotation.
The tolerances rest on one condition, asserted in case(): outside the tie case no column of wts has its two largest entries
equal in fp32 (preds would depend on the rule).  RESEEDED counts the cases whose seed had to be changed for that: none."""
import functools

import numpy as np

from rotation_ref import anchors_for, decode_case, label_relative_rotation, ortho6d_matrix, quat_matrix

FLAG_BAD_LABEL, FLAG_NORM_CLAMPED = 1, 2
CLAMP = 1e-8
W = 10.0                                 # the reference's default weight of the L2 term


# ----------------------------------------------------------------------------------------------- the specification, forward
def _gather_y(y, L):
    """y f64 [b,nr,A,A], L [b,A] (in range) -> [b,A,nr]: y[p,:,L[p,a],a]."""
    b, nr, A, _ = y.shape
    return y[np.arange(b)[:, None], :, L, np.arange(A)[None, :]]


def _norms(v):
    """The norms entering the rotation map of v [..., nr] -> [..., 2] (nr = 4: |q| twice; nr = 6: |v[0:3]|, |x cross v[3:6]|)."""
    if v.shape[-1] == 4:
        n = np.sqrt((v * v).sum(-1))
        return np.stack((n, n), -1)
    na = np.sqrt((v[..., :3] ** 2).sum(-1))
    x = v[..., :3] / np.maximum(na, CLAMP)[..., None]
    c = np.cross(x, v[..., 3:])
    return np.stack((na, np.sqrt((c * c).sum(-1))), -1)


def forward(wts, y, label, R_target, w=W):
    """-> dict of row_ce, row_l2 f64 [b,A], preds, row_flags i32 [b,A], sel_R f64 [b,A,3,3], scalars f64 [4] (loss, cls_loss, reg,
    r_acc: fp64 sums of the per-row values ROUNDED to fp32), and the magnitudes mag_ce, mag_l2 [b,A], cond [b,A] (>= 1: by how
    much the rotation map amplifies a relative rounding of its input), mag_scalars [4]."""
    wts, y, label = np.asarray(wts), np.asarray(y), np.asarray(label)
    assert wts.dtype == np.float32 and y.dtype == np.float32
    b, A = label.shape
    nr = y.shape[1]
    bad = (label < 0) | (label >= A)
    L = np.where(bad, 0, label)
    preds = np.argmax(wts, axis=1).astype(np.int32)          # the first maximum, compared in fp32
    w64 = wts.astype(np.float64)
    m = w64.max(axis=1)
    s = np.zeros((b, A))
    for t in range(A):                                       # t ascending
        s = s + np.exp(w64[:, t] - m)
    wl = np.take_along_axis(w64, L[:, None, :], axis=1)[:, 0]
    row_ce = np.where(bad, 0.0, m + np.log(s) - wl)
    mag_ce = np.where(bad, 0.0, 1.0 + np.abs(m) + np.abs(np.log(s)) + np.abs(wl))
    v = _gather_y(y.astype(np.float64), L)
    norms = _norms(v)
    R = (quat_matrix if nr == 4 else ortho6d_matrix)(v)
    R = np.where(bad[:, :, None, None], 0.0, R)
    clamped = (norms < CLAMP).any(-1) & ~bad
    if nr == 6:                                              # z = n(x cross y2): relative error of the cross product
        x = v[..., :3] / np.maximum(norms[..., 0], CLAMP)[..., None]
        cond = 1.0 + np.sqrt((x * x).sum(-1)) * np.sqrt((v[..., 3:] ** 2).sum(-1)) / np.maximum(norms[..., 1], 1e-300)
        cond = np.where(clamped, 1.0, cond)
    else:
        cond = np.ones((b, A))
    d = np.where(bad[:, :, None, None], 0.0, np.asarray(R_target, dtype=np.float64) - R).reshape(b, A, 9)
    row_l2 = np.zeros((b, A))
    for e in range(9):                                       # row-major
        row_l2 = row_l2 + d[..., e] * d[..., e]
    mag_l2 = 2.0 * cond * np.maximum(np.abs(R).max(axis=(2, 3)), 1.0) * np.abs(d).sum(-1) + row_l2
    flags = (bad * FLAG_BAD_LABEL + clamped * FLAG_NORM_CLAMPED).astype(np.int32)
    n = b * A
    ce32, l232 = row_ce.astype(np.float32).astype(np.float64), row_l2.astype(np.float32).astype(np.float64)
    cls, reg = ce32.sum() / n, w * l232.sum() / (9.0 * n)
    scalars = np.array([cls + reg, cls, reg, (preds == label).sum() / n])
    mag_cls, mag_reg = np.abs(ce32).sum() / n, abs(w) * l232.sum() / (9.0 * n)
    return dict(row_ce=row_ce, row_l2=row_l2, preds=preds, row_flags=flags, sel_R=R, scalars=scalars, mag_ce=mag_ce, mag_l2=mag_l2,
                cond=cond, mag_scalars=np.array([mag_cls + mag_reg, mag_cls, mag_reg, 0.0]), v=v, norms=norms, m=m, s=s, bad=bad)


# ----------------------------------------------------------------------------------------------- the specification, backward
def _skew(u):
    """[...,3] -> [...,3,3]: the matrix of u cross ."""
    o = np.zeros(u.shape[:-1] + (3, 3))
    o[..., 0, 1], o[..., 0, 2] = -u[..., 2], u[..., 1]
    o[..., 1, 0], o[..., 1, 2] = u[..., 2], -u[..., 0]
    o[..., 2, 0], o[..., 2, 1] = -u[..., 1], u[..., 0]
    return o


def _normalize_jac(v, norm):
    """d n(v) / d v [..., k, k] and the same with every term taken in absolute value: (I -+ u u^T) / |v| where |v| >= 1e-8,
    I / 1e-8 where the clamp was active."""
    k = v.shape[-1]
    eye = np.broadcast_to(np.eye(k), v.shape[:-1] + (k, k))
    live = (norm >= CLAMP)[..., None, None]
    safe = np.where(norm >= CLAMP, norm, 1.0)
    u = v / safe[..., None]
    uu = u[..., :, None] * u[..., None, :]
    return (np.where(live, (eye - uu) / safe[..., None, None], eye / CLAMP),
            np.where(live, (eye + np.abs(uu)) / safe[..., None, None], eye / CLAMP))


def map_jacobian(v, norms):
    """The Jacobian of the rotation map at v [..., nr] -> (J [..., 9, nr], Jabs likewise: the same products with every factor
    and every term in absolute value, which bounds the sum of the magnitudes of the terms behind every entry)."""
    nr = v.shape[-1]
    if nr == 4:
        N, Nabs = _normalize_jac(v, norms[..., 0])
        q = v / np.maximum(norms[..., 0], CLAMP)[..., None]
        w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
        o = np.zeros_like(w)
        D = 2.0 * np.stack([                                  # d R_k / d (w, x, y, z), k row-major
            np.stack([o, o, -2 * y, -2 * z], -1), np.stack([-z, y, x, -w], -1), np.stack([y, z, w, x], -1),
            np.stack([z, y, x, w], -1), np.stack([o, -2 * x, o, -2 * z], -1), np.stack([-x, -w, z, y], -1),
            np.stack([-y, z, -w, x], -1), np.stack([x, w, z, y], -1), np.stack([o, -2 * x, -2 * y, o], -1)], -2)
        return D @ N, np.abs(D) @ Nabs
    a, b2 = v[..., :3], v[..., 3:]
    Na, Na_abs = _normalize_jac(a, norms[..., 0])
    x = a / np.maximum(norms[..., 0], CLAMP)[..., None]
    c = np.cross(x, b2)
    Nc, Nc_abs = _normalize_jac(c, norms[..., 1])
    z = c / np.maximum(norms[..., 1], CLAMP)[..., None]
    zero, eye = np.zeros_like(Na), np.broadcast_to(np.eye(3), Na.shape)
    dx = np.concatenate((Na, zero), -1)                       # [..., 3, 6]
    dx_abs = np.concatenate((Na_abs, zero), -1)
    sel = np.concatenate((zero, eye), -1)
    dc = -_skew(b2) @ dx + _skew(x) @ sel                     # c = x cross b2
    dc_abs = np.abs(_skew(b2)) @ dx_abs + np.abs(_skew(x)) @ sel
    dz, dz_abs = Nc @ dc, Nc_abs @ dc_abs
    dy = -_skew(x) @ dz + _skew(z) @ dx                       # y = z cross x
    dy_abs = np.abs(_skew(x)) @ dz_abs + np.abs(_skew(z)) @ dx_abs
    J = np.stack((dx, dy, dz), -2).reshape(v.shape[:-1] + (9, 6))          # R[3 i + j] = (x, y, z)[j][i]
    Jabs = np.stack((dx_abs, dy_abs, dz_abs), -2).reshape(v.shape[:-1] + (9, 6))
    return J, Jabs


def backward(g, wts, y, label, R_target, fwd, w=W):
    """-> (dwts f64 [b,A,A], dy f64 [b,nr,A,A], mag_wts, mag_y): the gradients of g * loss and, per element, the sum of the
    magnitudes of the terms behind it."""
    wts, y, label = np.asarray(wts), np.asarray(y), np.asarray(label)
    b, A = label.shape
    nr = y.shape[1]
    n = b * A
    bad = fwd["bad"]
    L = np.where(bad, -1, label)
    p = np.exp(wts.astype(np.float64) - fwd["m"][:, None, :]) / fwd["s"][:, None, :]
    hot = (np.arange(A)[None, :, None] == L[:, None, :]).astype(np.float64)
    dwts = np.where(bad[:, None, :], 0.0, g / n * (p - hot))
    mag_wts = np.where(bad[:, None, :], 0.0, abs(g) / n * (p + hot))
    coef = g * 2.0 * w / (9.0 * n)
    G = coef * (fwd["sel_R"] - np.asarray(R_target, dtype=np.float64)).reshape(b, A, 9)
    Gmag = abs(coef) * (fwd["cond"][..., None] + np.abs(fwd["sel_R"]).reshape(b, A, 9) +
                        np.abs(np.asarray(R_target, dtype=np.float64)).reshape(b, A, 9))
    J, Jabs = map_jacobian(fwd["v"], fwd["norms"])
    dv = np.where(bad[..., None], 0.0, np.einsum('bake,bak->bae', J, G))
    mv = np.where(bad[..., None], 0.0, np.einsum('bake,bak->bae', Jabs, Gmag))
    dy, mag_y = np.zeros((b, nr, A, A)), np.zeros((b, nr, A, A))
    for pq in range(b):
        for a in range(A):
            if not bad[pq, a]:
                dy[pq, :, L[pq, a], a] = dv[pq, a]
                mag_y[pq, :, L[pq, a], a] = mv[pq, a]
    return dwts, dy, mag_wts, mag_y


# ----------------------------------------------------------------------------------------------- the case tables
A_SET, B_SET, NR_SET = (1, 12, 60, 64), (1, 3, 65), (4, 6)
CASES = [(A, b, nr, 500 + 20 * i + 2 * j + k) for i, A in enumerate(A_SET) for j, b in enumerate(B_SET) for k, nr in enumerate(NR_SET)]
CASES += [(60, 5, 4, 590), (60, 5, 6, 591)]                  # 300 rows: just past the 256 threads of a reduction
RESEEDED = 0                                                 # cases whose seed was changed to avoid an fp32 tie: none
UPSTREAM = 1.0


def no_top_tie(wts):
    """No column of wts [b,A,A] has its two largest entries equal in fp32 (A = 1 has one entry)."""
    if wts.shape[1] == 1:
        return True
    srt = np.sort(wts, axis=1)
    return bool((srt[:, -1] > srt[:, -2]).all())


def evaluate(wts, y, label, R_target, g=UPSTREAM, w=W):
    fwd = forward(wts, y, label, R_target, w)
    return fwd, backward(g, wts, y, label, R_target, fwd, w)


@functools.lru_cache(maxsize=None)
def case(A, b, nr, seed):
    """-> (wts f32 [b,A,A], y f32 [b,nr,A,A], label i32 [b,A], R_target f32 [b,A,3,3], anchors f32, T f32 [b,3,3], fwd, bwd).
    decode_case's wts are a softmax's output (in 0..1); the loss takes them as logits, as the reference does."""
    wts, y, anchors, label, T, _ = decode_case(A, b, nr, seed)
    R_target = np.ascontiguousarray(label_relative_rotation(anchors, T)[0].astype(np.float32))
    assert no_top_tie(wts), (A, b, nr, seed)
    fwd, bwd = evaluate(wts, y, label, R_target)
    return wts, y, label, R_target, anchors, T, fwd, bwd


@functools.lru_cache(maxsize=None)
def built_case(name):
    """-> (wts, y, label, R_target, fwd, bwd), A = 12, b = 3:
    tie     nr = 4; column 5 of pair 1 has its maximum at t = 3 and t = 7 with the same fp32 bits: preds is 3.
    bad     nr = 6; label[0,2] = -1 and label[2,11] = 12 = A: bit 0, zero rows, zero gradients.
    clamp4  nr = 4; a quaternion of norm 1e-9 at row (1, 4): bit 1 and the clamped Jacobian.
    clamp6  nr = 6; a 6-d vector whose first triple is zero at row (1, 4), so both norms are zero and clamped.  (torch's autograd
            returns NaN there: the backward of sqrt at 0 is 0 * inf.  The specification's v / 1e-8 is what autograd gives
            for every norm in (0, 1e-8), which the next two cases show, and is finite at 0.)
    clamp6_tiny   the first triple has norm 1e-9: the first norm is clamped, the second is not.
    clamp6_cross  (1, 0, 0, 2, 1e-9, 0): the first norm is 1, x cross y[3:6] = (0, 0, 1e-9): the second norm is clamped.
    big     nr = 4; logits of +-80 (plus the case's own values in 0..1): softmax weights of e^-160 beside the maximum.
    huge    the same with +-100: exp(100) overflows fp32 (exp(80) = 5.5e34 does not yet), the maximum is taken out first."""
    nr = 6 if name in ("bad", "clamp6", "clamp6_tiny", "clamp6_cross") else 4
    wts, y, anchors, label, T, _ = decode_case(12, 3, nr, 700 + nr)
    wts, y, label = wts.copy(), y.copy(), label.copy()
    R_target = np.ascontiguousarray(label_relative_rotation(anchors, T)[0].astype(np.float32))
    if name == "tie":
        wts[1, 3, 5] = wts[1, 7, 5] = np.float32(wts[1, :, 5].max() * 2)
    elif name == "bad":
        label[0, 2], label[2, 11] = -1, 12
    elif name == "clamp4":
        q = np.array([3.0, -4.0, 12.0, 84.0]) / 85.0 * 1e-9
        y[1, :, label[1, 4], 4] = q.astype(np.float32)
    elif name == "clamp6":
        y[1, :3, label[1, 4], 4] = 0.0
    elif name == "clamp6_tiny":
        y[1, :3, label[1, 4], 4] = (np.array([3.0, -4.0, 12.0]) / 13.0 * 1e-9).astype(np.float32)
    elif name == "clamp6_cross":
        y[1, :, label[1, 4], 4] = np.array([1.0, 0.0, 0.0, 2.0, 1e-9, 0.0], dtype=np.float32)
    elif name in ("big", "huge"):
        size = np.float32(80.0 if name == "big" else 100.0)
        wts = np.where(np.random.default_rng(77).random(wts.shape) < 0.5, size, -size) + wts
        wts = np.ascontiguousarray(wts.astype(np.float32))
    else:
        raise KeyError(name)
    fwd, bwd = evaluate(wts, y, label, R_target)
    return wts, y, label, R_target, fwd, bwd


BUILT = ("tie", "bad", "clamp4", "clamp6", "clamp6_tiny", "clamp6_cross", "big", "huge")
GOLDEN_SHAPE = (60, 2)                                       # tests/golden/rotation_loss.npz: A, b, both nr


def golden_inputs(nr):
    """The inputs recorded in tests/golden/rotation_loss.npz (gen_golden_rotation_loss.py writes what this returns)."""
    A, b = GOLDEN_SHAPE
    wts, y, anchors, label, T, _ = decode_case(A, b, nr, 800 + nr)
    R_target = np.ascontiguousarray(label_relative_rotation(anchors, T)[0].astype(np.float32))
    return wts, y, label, R_target, anchors, T
