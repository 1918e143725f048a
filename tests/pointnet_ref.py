"""float64 restatement of the PointNet head (csrc/pointnet.hip) in the kernels' own layouts, numpy only, no device:
    F[b][p][a][c], xyz[b][3][p], anchors[a][3][3] or None (identity: na == 1), W[co][c + 3], bias[co] or None,
    out / arg / gout [b][a][co], centre [b][3], dF [b][p][a][c], dZ [b][p][a][co], dW [co][c + 3], dbias [co].
The arg-max follows torch.max: the first maximum wins, NaN IS the maximum and the first NaN wins.  What
tests/test_gpu_pointnet_exact.py and tests/test_pointnet_spec.py judge by."""
import numpy as np

from gemm_ref import bf16_rne

F64 = np.float64


def centre_of(xyz):
    return np.asarray(xyz, F64).mean(axis=2)


def ext_of(xyz, anchors, centre):
    """ext[b][p][a][i] = sum_j R_a[j][i] (xyz[b][j][p] - centre[b][j]) (einsum 'aji,bjn->bina'); anchors None: a = 1, identity."""
    v = np.asarray(xyz, F64) - np.asarray(centre, F64)[:, :, None]
    if anchors is None:
        return np.ascontiguousarray(v.transpose(0, 2, 1)[:, :, None, :])
    return np.einsum("aji,bjp->bpai", np.asarray(anchors, F64), v)


def embed(F, xyz, anchors, W, bias, centre=None):
    """z[b][p][a][co]: the embedding the max runs over."""
    F, W = np.asarray(F, F64), np.asarray(W, F64)
    c = F.shape[3]
    ctr = centre_of(xyz) if centre is None else np.asarray(centre, F64)
    z = F @ W[:, :c].T + ext_of(xyz, anchors, ctr) @ W[:, c:].T
    return z if bias is None else z + np.asarray(bias, F64)


def max_first(z, axis=1):
    """(max, arg-max) along `axis` as torch.max: first maximum; any NaN -> the first NaN."""
    z = np.asarray(z)
    nan = np.isnan(z)
    arg = np.where(nan, -np.inf, z).argmax(axis=axis)                   # numpy: the first occurrence
    arg = np.where(nan.any(axis=axis), nan.argmax(axis=axis), arg)
    out = np.take_along_axis(z, np.expand_dims(arg, axis), axis=axis).squeeze(axis)
    return out, arg.astype(np.int32)


def forward(F, xyz, anchors, W, bias):
    """out[b][a][co] (float64), arg[b][a][co] (int32), centre[b][3]."""
    ctr = centre_of(xyz)
    out, arg = max_first(embed(F, xyz, anchors, W, bias, ctr), axis=1)
    return out, arg, ctr


def max_of(Z, xyz, anchors, W, bias, c):
    """epn_pointnet_max_f32: Z[b][p][a][co] is the feature part of the embedding; (Z + bias) + coordinate terms, as the kernel
    adds them (a -0.0 of Z becomes +0.0: the kernel adds a zero bias when none is given)."""
    ctr = centre_of(xyz)
    z = np.asarray(Z, F64) + (0.0 if bias is None else np.asarray(bias, F64))
    z = z + ext_of(xyz, anchors, ctr) @ np.asarray(W, F64)[:, c:].T
    out, arg = max_first(z, axis=1)
    return out, arg, ctr


def dz(gout, arg, p, dtype="f32"):
    """dZ[b][p][a][co] = arg[b][a][co] == p ? gout : 0; "bf16": every element rounded to the nearest bf16, ties to even."""
    g = np.asarray(gout)
    if dtype == "bf16":
        g = bf16_rne(g.astype(np.float32))
    hit = np.asarray(arg)[:, None] == np.arange(p)[None, :, None, None]
    return np.where(hit, g.astype(F64)[:, None], 0.0)


def bwd_data(gout, arg, W, p):
    """dF[b][p][a][c] = sum_{o: arg[b][a][o] == p} gout[b][a][o] W[o][c]."""
    W = np.asarray(W, F64)
    return dz(gout, arg, p) @ W[:, :W.shape[1] - 3]


def _gather(X, arg):
    """X[b][p][a][k], arg[b][a][o] -> X[b][arg[b][a][o]][a][:] as [b][a][o][k]."""
    b, _, a, _ = X.shape
    return X[np.arange(b)[:, None, None], np.asarray(arg), np.arange(a)[None, :, None]]


def bwd_coord(gout, arg, xyz, anchors, centre):
    """The three coordinate columns dW[:, c:] ([co][3]) and dbias[co]."""
    g = np.asarray(gout, F64)
    e = _gather(ext_of(xyz, anchors, centre), arg)
    return np.einsum("bao,baoi->oi", g, e), g.sum(axis=(0, 1))


def bwd_weight(gout, arg, F, xyz, anchors, centre):
    """dW[co][c + 3], dbias[co]."""
    g = np.asarray(gout, F64)
    dWf = np.einsum("bao,baoc->oc", g, _gather(np.asarray(F, F64), arg))
    dWx, db = bwd_coord(gout, arg, xyz, anchors, centre)
    return np.concatenate([dWf, dWx], axis=1), db


def magnitudes(F, xyz, anchors, W, bias, gout, arg):
    """Sums of absolute values of each output's terms (the real tier's S): dict out [b][a][co] (the column's largest
    per-point sum), dF, dW, dbias.  A coordinate term counts as |w| sum_j |R_ji| (|x_j| + |centre_j|)."""
    F, W, g = np.abs(np.asarray(F, F64)), np.abs(np.asarray(W, F64)), np.abs(np.asarray(gout, F64))
    c, p = F.shape[3], F.shape[1]
    ax = np.abs(np.asarray(xyz, F64)) + np.abs(centre_of(xyz))[:, :, None]
    if anchors is None:
        e = np.ascontiguousarray(ax.transpose(0, 2, 1)[:, :, None, :])
    else:
        e = np.einsum("aji,bjp->bpai", np.abs(np.asarray(anchors, F64)), ax)
    s = F @ W[:, :c].T + e @ W[:, c:].T + (0.0 if bias is None else np.abs(np.asarray(bias, F64)))
    hit = np.asarray(arg)[:, None] == np.arange(p)[None, :, None, None]
    dZ = np.where(hit, g[:, None], 0.0)
    dW = np.concatenate([np.einsum("bao,baoc->oc", g, _gather(F, arg)), np.einsum("bao,baoi->oi", g, _gather(e, arg))], axis=1)
    return dict(out=s.max(axis=1), dF=dZ @ W[:, :c], dW=dW, dbias=g.sum(axis=(0, 1)))
