"""What the exact convolution tests judge by (tests/test_gpu_conv_exact.py on the device, tests/test_conv_spec.py without one):
numpy float64 restatements of InterSO3Conv and IntraSO3Conv at the C boundary of include/epn_so3conv.h, written over the
definition -- gather, weight, einsum -- and not over the kernels' tiles.  Layouts are the boundary's: features channels-last
[b, p, a, c], xyz [b, 3, p], W [cout, cin * ks] with column c * ks + k.  Nothing here needs the library or torch."""
import numpy as np

F64 = np.float64


# ------------------------------------------------------------------------------------------------ inter
def inter_gather(xyz, new_xyz, ball_idx):
    """g[b, p, n, :] = xyz[b, :, idx] - new_xyz[b, :, p] (float64) and valid[b, p, n]: an index outside 0 .. p1 - 1 (the ball
    query writes p1) is the zero shadow row."""
    xyz, new_xyz = np.asarray(xyz, F64), np.asarray(new_xyz, F64)
    idx = np.asarray(ball_idx)
    p1 = xyz.shape[2]
    valid = (idx >= 0) & (idx < p1)
    safe = np.where(valid, idx, 0)
    b = np.arange(xyz.shape[0])[:, None, None]
    g = xyz.transpose(0, 2, 1)[b, safe] - new_xyz.transpose(0, 2, 1)[:, :, None, :]
    return g, valid, safe


def inter_weights(xyz, new_xyz, ball_idx, anchors, kernels, sigma):
    """w[b, p, a, k, n] = max(0, 1 - |g - R_a kappa_k|^2 / sigma), 0 in a shadow slot; also returns (g, valid, safe, rk)."""
    g, valid, safe = inter_gather(xyz, new_xyz, ball_idx)
    rk = np.einsum("ade,ke->akd", np.asarray(anchors, F64), np.asarray(kernels, F64))          # R_a kappa_k
    diff = g[:, :, None, None, :, :] - rk[None, None, :, :, None, :]                           # [b, p, a, k, n, 3]
    w = np.maximum(0.0, 1.0 - (diff * diff).sum(-1) / float(sigma))
    return w * valid[:, :, None, None, :], g, valid, safe, rk


def inter_conv(xyz, new_xyz, ball_idx, anchors, kernels, sigma, F, W, gOut, want=("out", "dF", "dW")):
    """Returns dict(w, G, out, dF, dW):
      G[b, p, a, c, k]  = sum_n F[b, idx[b, p, n], a, c] w[b, p, a, k, n]      (a duplicate index counts once per slot)
      out[b, p, a, o]   = sum_{c, k} W[o, c * ks + k] G[b, p, a, c, k]
      dF[b, q, a, c]    = sum_{p, n : idx[b, p, n] = q} sum_k w[b, p, a, k, n] dG[b, p, a, c, k],  dG = sum_o W[o, ck] gOut[.., o]
      dW[o, c * ks + k] = sum_{b, p, a} gOut[b, p, a, o] G[b, p, a, c, k]
    (`want`: which of out, dF, dW are computed -- the large weight-gradient cases need dW only)."""
    w, g, valid, safe, rk = inter_weights(xyz, new_xyz, ball_idx, anchors, kernels, sigma)
    F, W, gOut = np.asarray(F, F64), np.asarray(W, F64), np.asarray(gOut, F64)
    b, p1, na, cin = F.shape
    ks, cout = w.shape[3], W.shape[0]
    W3 = W.reshape(cout, cin, ks)
    bi = np.arange(b)[:, None, None]
    Fg = F[bi, safe]                                                                           # [b, p, n, a, c]
    G = np.einsum("bpnac,bpakn->bpack", Fg, w, optimize=True)
    res = dict(w=w, G=G)
    if "out" in want:
        res["out"] = np.einsum("ock,bpack->bpao", W3, G, optimize=True)
    if "dF" in want:
        res["dF"] = _scatter(w, W3, gOut, safe, F.shape)
    if "dW" in want:
        res["dW"] = np.einsum("bpao,bpack->ock", gOut, G, optimize=True).reshape(cout, cin * ks)
    return res


def _scatter(w, W3, gOut, safe, fshape):
    dG = np.einsum("ock,bpao->bpack", W3, gOut, optimize=True)
    T = np.einsum("bpakn,bpack->bpnac", w, dG, optimize=True)                                  # per-slot contribution
    dF = np.zeros(fshape)
    for bb in range(fshape[0]):
        np.add.at(dF[bb], safe[bb].reshape(-1), T[bb].reshape(-1, fshape[2], fshape[3]))       # (shadow slots carry w = 0)
    return dF


def inter_group(xyz, new_xyz, ball_idx, anchors, kernels, sigma, F):
    """The gather of inter_conv on its own, as the matrix the grouping entries write in the plain column order:
      G[(b, p, a), c * ks + k] = sum_n F[b, idx[b, p, n], a, c] w[b, p, a, k, n]"""
    w, g, valid, safe, rk = inter_weights(xyz, new_xyz, ball_idx, anchors, kernels, sigma)
    F = np.asarray(F, F64)
    Fg = F[np.arange(F.shape[0])[:, None, None], safe]                                         # [b, p, n, a, c]
    G = np.einsum("bpnac,bpakn->bpack", Fg, w, optimize=True)
    return G.reshape(-1, F.shape[3] * w.shape[3])


def inter_ungroup(xyz, new_xyz, ball_idx, anchors, kernels, sigma, dG, cin):
    """The transpose of inter_group: dF[b, q, a, c] = sum_{p, n : idx[b, p, n] = q} sum_k w[b, p, a, k, n] dG[(b, p, a), c * ks + k]"""
    w, g, valid, safe, rk = inter_weights(xyz, new_xyz, ball_idx, anchors, kernels, sigma)
    b, p2, na, ks, nn = w.shape
    T = np.einsum("bpakn,bpack->bpnac", w, np.asarray(dG, F64).reshape(b, p2, na, cin, ks), optimize=True)
    dF = np.zeros((b, np.asarray(xyz).shape[2], na, cin))
    for bb in range(b):
        np.add.at(dF[bb], safe[bb].reshape(-1), T[bb].reshape(-1, na, cin))                    # (shadow slots carry w = 0)
    return dF


def inverse_list(ball_idx, p1):
    """(off[b, p1 + 1], ent[b, p2 * nn]) of epn_inter_inverse_list: per cloud the CSR inverse of the index table -- the entries
    p * nn + n that name a point, by point, then ascending; indices outside 0 .. p1 - 1 dropped, the tail of ent -1."""
    idx = np.asarray(ball_idx)
    b = idx.shape[0]
    off = np.zeros((b, p1 + 1), np.int32)
    ent = np.full((b, idx.shape[1] * idx.shape[2]), -1, np.int32)
    for bb in range(b):
        flat = idx[bb].reshape(-1)
        valid = np.nonzero((flat >= 0) & (flat < p1))[0]
        order = valid[np.argsort(flat[valid], kind="stable")]
        off[bb, 1:] = np.cumsum(np.bincount(flat[valid], minlength=p1))
        ent[bb, :len(order)] = order
    return off, ent


def inter_abs_sums(xyz, new_xyz, ball_idx, anchors, kernels, sigma, F, W, gOut, expanded=False, want=("out", "dF", "dW")):
    """Sums of ABSOLUTE values of the terms of every element of out, dF and dW -- what the largest partial sum of any summation
    order is bounded by.  expanded: w is replaced by w + |g|^2 / sigma + |g . r| + |beta| (r = (2 / sigma) R_a kappa_k,
    beta = -|kappa_k|^2 / sigma), which covers the cancellation inside the expanded form the kernels evaluate."""
    w, g, valid, safe, rk = inter_weights(xyz, new_xyz, ball_idx, anchors, kernels, sigma)
    if expanded:
        s = float(sigma)
        w = w + valid[:, :, None, None, :] * ((g * g).sum(-1)[:, :, None, None, :] / s
                                              + np.abs(np.einsum("bpnd,akd->bpakn", g, rk)) * 2.0 / s
                                              + ((rk * rk).sum(-1) / s)[None, None, :, :, None])
    F, W, gOut = np.abs(np.asarray(F, F64)), np.abs(np.asarray(W, F64)), np.abs(np.asarray(gOut, F64))
    b, p1, na, cin = F.shape
    ks, cout = w.shape[3], W.shape[0]
    W3 = W.reshape(cout, cin, ks)
    Fg = F[np.arange(b)[:, None, None], safe]
    G = np.einsum("bpnac,bpakn->bpack", Fg, w, optimize=True)
    res = {}
    if "out" in want:
        res["out"] = np.einsum("ock,bpack->bpao", W3, G, optimize=True)
    if "dF" in want:
        res["dF"] = _scatter(w, W3, gOut, safe, F.shape)
    if "dW" in want:
        res["dW"] = np.einsum("bpao,bpack->ock", gOut, G, optimize=True).reshape(cout, cin * ks)
    return res


# ------------------------------------------------------------------------------------------------ intra
def intra_conv(F, W, intra_idx, gOut):
    """Returns dict(out, dF, dW):
      out[b, p, a, o]   = sum_{c, k} W[o, c * kn + k] F[b, p, idx[a, k], c]
      dF[b, p, s, c]    = sum_{a, k : idx[a, k] = s} sum_o W[o, c * kn + k] gOut[b, p, a, o]
      dW[o, c * kn + k] = sum_{b, p, a} gOut[b, p, a, o] F[b, p, idx[a, k], c]"""
    F, W, gOut = np.asarray(F, F64), np.asarray(W, F64), np.asarray(gOut, F64)
    idx = np.asarray(intra_idx)
    b, p, na, cin = F.shape
    kn, cout = idx.shape[1], W.shape[0]
    W3 = W.reshape(cout, cin, kn)
    Fg = F[:, :, idx, :]                                                                       # [b, p, a, k, c]
    out = np.einsum("ock,bpakc->bpao", W3, Fg, optimize=True)
    dFg = np.einsum("ock,bpao->bpakc", W3, gOut, optimize=True)
    dF = np.zeros_like(F)
    for a in range(na):
        for k in range(kn):
            dF[:, :, idx[a, k], :] += dFg[:, :, a, k, :]
    dW = np.einsum("bpao,bpakc->ock", gOut, Fg, optimize=True).reshape(cout, cin * kn)
    return dict(out=out, dF=dF, dW=dW)


def inverse_intra_idx(intra_idx):
    """inv[idx[a, k], k] = a (every column of idx a permutation of the anchors), as epn_pointcloud_amd.ops builds it."""
    idx = np.asarray(intra_idx)
    na, kn = idx.shape
    inv = np.full((na, kn), -1, dtype=np.int32)
    for k in range(kn):
        assert sorted(idx[:, k].tolist()) == list(range(na)), f"column {k} is no permutation"
        inv[idx[:, k], k] = np.arange(na, dtype=np.int32)
    return inv
