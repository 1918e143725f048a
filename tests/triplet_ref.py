"""numpy fp64 restatement of the four training-loss entries of include/epn_so3conv.h (epn_triplet_batch_hard_f32 and its backward,
epn_anchor_interp_f32 and its backward) and the tables of cases shared by test_triplet_spec.py (CPU: the
restatement against the reference's golden, and the conditions the GPU tolerances rest on) and test_gpu_triplet.py."""
import functools

import numpy as np

import rotation_ref as Rf

EPS = 1e-6
MODES = ("hard", "soft", "contrastive")
FLAG_POS_CLAMPED, FLAG_NEG_CLAMPED, FLAG_HINGE_ACTIVE = 1, 2, 4
ARG_GAP = 1e-9              # relative gap between the smallest and the second-smallest distance of a row
KINK_GAP = 1e-6             # distance of a hinge argument (and of softplus's threshold argument) from its kink
TRACE_GAP = 1e-6            # separation of the four largest traces of every (b, n)


# ----------------------------------------------------------------------------------------------- the specification
def distances(src, tgt, eps=EPS):
    """-> (dist f64 [N,N], d2 f64 [N,N]) from the differences."""
    s, t = np.asarray(src), np.asarray(tgt)
    assert s.dtype == t.dtype == np.float32
    s64, t64 = s.astype(np.float64), t.astype(np.float64)
    d2 = np.empty((s.shape[0], t.shape[0]))
    for r in range(0, s.shape[0], 64):                       # in blocks of rows: the [N, N, D] differences of the large case
        diff = s64[r:r + 64, None, :] - t64[None, :, :]
        d2[r:r + 64] = (diff * diff).sum(-1)
    return np.sqrt(np.where(d2 < eps, eps, d2)), d2


def batch_hard(src, tgt, mode, margin, eps=EPS):
    """-> dict of the entry's outputs: d_pos, d_neg, row_loss f64 [N] (unrounded), neg_idx, nn_idx, row_flags i32 [N], scalars
    f64 [4] (the fp64 means of the per-row values ROUNDED to fp32, as the entry defines them), and the conditioning numbers
    neg_gap, nn_gap (relative gap to the runner-up, inf if there is none), kink (distance of the hinge / threshold argument
    from its kink) and d2 itself."""
    dist, d2 = distances(src, tgt, eps)
    N = dist.shape[0]
    ar = np.arange(N)
    d_pos = dist[ar, ar].copy()
    off = dist.copy()
    off[ar, ar] = np.inf
    neg_idx = off.argmin(1)                                  # numpy: the first (lowest) index of the minimum
    d_neg = off[ar, neg_idx]
    nn_idx = dist.argmin(1)

    def gap(m, best):
        if m.shape[1] < 2:
            return np.full(N, np.inf)
        second = np.sort(m, axis=1)[:, 1]
        return (second - best) / best
    neg_gap, nn_gap = gap(off, d_neg), gap(dist, dist[ar, nn_idx])
    x = d_pos - d_neg
    if mode == "hard":
        active = x + margin > 0
        row_loss = np.where(active, x + margin, 0.0)
        kink = np.abs(x + margin)
    elif mode == "soft":
        active = np.ones(N, bool)
        with np.errstate(over="ignore"):
            row_loss = np.where(margin * x > 20.0, x, np.log1p(np.exp(np.minimum(margin * x, 700.0))) / margin)
        kink = np.abs(margin * x - 20.0)
    else:
        assert mode == "contrastive"
        active = margin - d_neg > 0
        row_loss = d_pos + np.where(active, margin - d_neg, 0.0)
        kink = np.abs(margin - d_neg)
    flags = (np.where(d2[ar, ar] < eps, FLAG_POS_CLAMPED, 0) | np.where(d2[ar, neg_idx] < eps, FLAG_NEG_CLAMPED, 0)
             | np.where(active, FLAG_HINGE_ACTIVE, 0)).astype(np.int32)
    r32 = lambda v: v.astype(np.float32).astype(np.float64)
    scalars = np.array([r32(row_loss).mean(), (nn_idx == ar).sum() / N, r32(d_pos).mean(), r32(d_neg).mean()])
    return dict(d_pos=d_pos, d_neg=d_neg, row_loss=row_loss, neg_idx=neg_idx.astype(np.int32), nn_idx=nn_idx.astype(np.int32),
                row_flags=flags, scalars=scalars, neg_gap=neg_gap, nn_gap=nn_gap, kink=kink, d2=d2)


def batch_hard_bwd(upstream, src, tgt, fwd, mode, margin):
    """The backward entry on the forward's per-row outputs (d_pos, d_neg rounded to fp32 first: that is what it is given) ->
    (dsrc, dtgt f64 [N,D], mag_src, mag_tgt f64 [N,D]: the sums of the absolute values of the terms each element is made of)."""
    s, t = np.asarray(src, dtype=np.float64), np.asarray(tgt, dtype=np.float64)
    N = s.shape[0]
    dp = fwd["d_pos"].astype(np.float32).astype(np.float64)
    dn = fwd["d_neg"].astype(np.float32).astype(np.float64)
    f, ni = fwd["row_flags"], fwd["neg_idx"]
    act = (f & FLAG_HINGE_ACTIVE) != 0
    if mode == "hard":
        gp = gn = act.astype(np.float64)
    elif mode == "soft":
        bx = margin * (dp - dn)
        with np.errstate(over="ignore"):
            gp = gn = np.where(bx > 20.0, 1.0, 1.0 / (1.0 + np.exp(-bx)))
    else:
        gp, gn = np.ones(N), act.astype(np.float64)
    scale = float(upstream) / N
    cp = np.where(f & FLAG_POS_CLAMPED, 0.0, scale * gp / dp)
    cn = np.where(f & FLAG_NEG_CLAMPED, 0.0, scale * gn / dn)
    pos = cp[:, None] * (s - t)
    neg = cn[:, None] * (s - t[ni])
    dsrc = pos - neg
    dtgt, mag_tgt = -pos, np.abs(pos)
    for i in range(N):                                       # ascending i, as the entry adds them
        dtgt[ni[i]] += neg[i]
        mag_tgt[ni[i]] += np.abs(neg[i])
    return dsrc, dtgt, np.abs(pos) + np.abs(neg), mag_tgt


def traces(T, anchors):
    """-> f64 [nb,A,A]: trace[b,n,m] = tr(T_b^T A_n A_m^T), T the rotation block."""
    R = np.asarray(T, dtype=np.float64)[:, :3, :3]
    An = np.asarray(anchors, dtype=np.float64)
    P = np.einsum('bji,njk->bnik', R, An)                   # T_b^T A_n
    return np.einsum('bnik,mik->bnm', P, An)


def anchor_interp(feature, T, anchors, sigma):
    """-> dict(out f64 [nb,C,A], idx i32 [nb,A,3], w f64 [nb,A,3], trace_gap: the smallest separation among the four largest
    traces of any (b, n))."""
    f = np.asarray(feature, dtype=np.float64)
    tr = traces(T, anchors)
    order = np.argsort(-tr, axis=2, kind="stable")          # descending, the lower m first on a tie
    idx = order[:, :, :3]
    top = np.take_along_axis(tr, order[:, :, :4], axis=2)
    e = np.exp((top[:, :, :3] - top[:, :, :1]) / sigma)
    w = e / e.sum(2, keepdims=True)
    nb = f.shape[0]
    out = np.stack([(f[b][:, idx[b]] * w[b][None]).sum(-1) for b in range(nb)]) if nb else f.copy()
    gap = float((top[:, :, :-1] - top[:, :, 1:]).min()) if nb else np.inf
    return dict(out=out, idx=idx.astype(np.int32), w=w, trace_gap=gap)


def anchor_interp_bwd(dout, idx, w):
    """(dout [nb,C,A], idx [nb,A,3], w [nb,A,3] rounded to fp32 first) -> (dfeature f64 [nb,C,A], mag f64 [nb,C,A])."""
    g = np.asarray(dout, dtype=np.float64)
    w = np.asarray(w).astype(np.float32).astype(np.float64)
    nb, C, A = g.shape
    df, mag = np.zeros_like(g), np.zeros_like(g)
    for b in range(nb):
        for n in range(A):
            for k in range(3):
                df[b, :, idx[b, n, k]] += w[b, n, k] * g[b, :, n]
                mag[b, :, idx[b, n, k]] += np.abs(w[b, n, k] * g[b, :, n])
    return df, mag


# ----------------------------------------------------------------------------------------------- the case tables
SHAPES = [(2, 1), (3, 32), (8, 33), (65, 32), (192, 32), (193, 64), (8, 3840)]
BH_CASES = [(N, D, mode, 503 + 10 * i + k) for i, (N, D) in enumerate(SHAPES) for k, mode in enumerate(MODES)]
INTERP_CASES = [(1, 1, 60, 700), (2, 4, 60, 701), (3, 64, 60, 702), (5, 3, 12, 703)]
SIGMA = 0.2
MIRROR_CASE = (6, 32, 4, 60, 800)                             # N, D, C, A, seed


def descriptors(rng, N, D):
    """Unit-norm rows (D > 1), tgt a perturbed src: the perturbation of row i has norm 0.05 .. 1.2 before renormalising, so the
    positives range from much nearer to farther than the nearest negative."""
    x = rng.standard_normal((N, D))
    noise = rng.standard_normal((N, D))
    noise *= rng.uniform(0.05, 1.2, (N, 1)) / np.linalg.norm(noise, axis=1, keepdims=True)
    y = x / np.linalg.norm(x, axis=1, keepdims=True) + noise if D > 1 else x + noise
    if D > 1:
        x = x / np.linalg.norm(x, axis=1, keepdims=True)
        y = y / np.linalg.norm(y, axis=1, keepdims=True)
    return np.ascontiguousarray(x.astype(np.float32)), np.ascontiguousarray(y.astype(np.float32))


def _split_margin(values):
    """The midpoint of the widest gap between neighbours of the sorted values: a threshold with values on either side of it."""
    v = np.sort(values)
    k = int(np.argmax(np.diff(v)))
    return float(np.float32(0.5 * (v[k] + v[k + 1])))


def margin_for(src, tgt, mode):
    """hard: -(the split point of d_pos - d_neg), so that some rows are active and some are not; contrastive: the split point of
    d_neg; soft: beta = 2."""
    if mode == "soft":
        return 2.0
    r = batch_hard(src, tgt, "hard", 0.0)
    return -_split_margin(r["d_pos"] - r["d_neg"]) if mode == "hard" else _split_margin(r["d_neg"])


@functools.lru_cache(maxsize=None)
def bh_case(N, D, mode, seed):
    """-> (src, tgt f32 [N,D], margin, forward dict, (dsrc, dtgt, mag_src, mag_tgt) for upstream = 1)."""
    src, tgt = descriptors(np.random.default_rng(seed), N, D)
    margin = margin_for(src, tgt, mode)
    fwd = batch_hard(src, tgt, mode, margin)
    return src, tgt, margin, fwd, batch_hard_bwd(1.0, src, tgt, fwd, mode, margin)


@functools.lru_cache(maxsize=None)
def built_case(name):
    """The four constructed cases -> (src, tgt, mode, margin, forward dict, backward tuple).
    crowd N = 1030, D = 257: the src rows cluster around one point, tgt[0] lies in the cluster and every positive far from it,
          so tgt[0] is the hardest negative of all rows but row 0: more rows than the 1024 the backward's list holds per round,
          and more columns than one pass of a workgroup covers
    dup   N = 8, D = 32: tgt[5] is a copy of tgt[2] and src[0] lies next to both, so row 0's hardest negative and its nearest
          row are an exact tie between 2 and 5: the lower index wins
    zero  src[3] == tgt[3] bitwise: d_pos[3] = sqrt(eps), flag bit 0, no positive gradient
    soft  N = 16, D = 8, rows of norm about 3 sqrt(8), margin (beta) = 16: beta x is above torch's threshold of 20 on some rows
          and below it on others"""
    rng = np.random.default_rng({"dup": 901, "zero": 902, "soft": 903, "crowd": 904}[name])
    mode, margin = "hard", None
    if name == "crowd":
        N, Dm = 1030, 257
        centre = rng.standard_normal(Dm)
        src = (centre + 0.1 * rng.standard_normal((N, Dm))).astype(np.float32)
        away = rng.standard_normal((N, Dm))
        tgt = (src + rng.uniform(8.0, 12.0, (N, 1)) * away / np.linalg.norm(away, axis=1, keepdims=True)).astype(np.float32)
        tgt[0] = (centre + 0.1 * rng.standard_normal(Dm)).astype(np.float32)
    elif name == "soft":
        src = (3.0 * rng.standard_normal((16, 8))).astype(np.float32)
        tgt = (src + rng.uniform(0.0, 4.0, (16, 1)) * rng.standard_normal((16, 8))).astype(np.float32)
        mode, margin = "soft", 16.0
    else:
        src, tgt = descriptors(rng, 8, 32)
        if name == "dup":
            tgt[5] = tgt[2]
            src[0] = tgt[2] + np.float32(0.01) * rng.standard_normal(32).astype(np.float32)
        else:
            src[3] = tgt[3]
    src, tgt = np.ascontiguousarray(src), np.ascontiguousarray(tgt)
    if margin is None:
        margin = margin_for(src, tgt, mode)
    fwd = batch_hard(src, tgt, mode, margin)
    return src, tgt, mode, margin, fwd, batch_hard_bwd(1.0, src, tgt, fwd, mode, margin)


@functools.lru_cache(maxsize=None)
def interp_case(nb, C, A, seed):
    """-> (feature f32 [nb,C,A], T f32 [nb,3,3], anchors f32 [A,3,3], dout f32 [nb,C,A], forward dict, (dfeature, mag))."""
    rng = np.random.default_rng(seed)
    anchors = Rf.anchors_for(A)
    T = np.ascontiguousarray(Rf.random_rotations(rng, nb).astype(np.float32))
    feature = np.ascontiguousarray(rng.standard_normal((nb, C, A)).astype(np.float32))
    dout = np.ascontiguousarray(rng.standard_normal((nb, C, A)).astype(np.float32))
    fwd = anchor_interp(feature, T, anchors, SIGMA)
    return feature, T, anchors, dout, fwd, anchor_interp_bwd(dout, fwd["idx"], fwd["w"])


@functools.lru_cache(maxsize=None)
def mirror_case(alpha, mode="hard"):
    """The mirror class end to end -> dict of the inputs (src, tgt, T [N,4,4], equi_src, equi_tgt, anchors, margin) and of the
    restatement's results: inv / equi forward dicts, total, and the gradients of total with respect to the four inputs."""
    N, D, C, A, seed = MIRROR_CASE
    rng = np.random.default_rng(seed)
    src, tgt = descriptors(rng, N, D)
    anchors = Rf.anchors_for(A)
    T = np.zeros((N, 4, 4), np.float32)
    T[:, :3, :3] = Rf.random_rotations(rng, N)
    T[:, :3, 3] = rng.standard_normal((N, 3))
    T[:, 3, 3] = 1
    e_src, e_tgt = descriptors(rng, N, C * A)
    e_src, e_tgt = e_src.reshape(N, C, A), e_tgt.reshape(N, C, A)
    margin = margin_for(src, tgt, mode)
    inv = batch_hard(src, tgt, mode, margin)
    dsrc, dtgt, mag_s, mag_t = batch_hard_bwd(1.0, src, tgt, inv, mode, margin)
    out = dict(src=src, tgt=tgt, T=T, equi_src=e_src, equi_tgt=e_tgt, anchors=anchors, margin=margin, inv=inv,
               dsrc=dsrc, dtgt=dtgt, mag_src=mag_s, mag_tgt=mag_t)
    if alpha > 0:
        it = anchor_interp(e_tgt, T, anchors, SIGMA)
        flat_t = np.ascontiguousarray(it["out"].astype(np.float32).reshape(N, -1))
        flat_s = np.ascontiguousarray(e_src.reshape(N, -1))
        equi = batch_hard(flat_s, flat_t, mode, margin)
        des, det, mes, met = batch_hard_bwd(float(np.float32(alpha)), flat_s, flat_t, equi, mode, margin)
        det32 = det.astype(np.float32).reshape(N, C, A)
        d_et, m_et = anchor_interp_bwd(det32, it["idx"], it["w"])
        total = float(np.float32(inv["scalars"][0])) + float(np.float32(alpha)) * float(np.float32(equi["scalars"][0]))
        out.update(interp=it, equi=equi, total=total, d_equi_src=des.reshape(N, C, A), mag_equi_src=mes.reshape(N, C, A),
                   d_equi_tgt=d_et, mag_equi_tgt=m_et, mag_flat_tgt=met.reshape(N, C, A))
    return out
