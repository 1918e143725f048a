"""float64 restatement of csrc/so3_basis.hip (include/epn_so3conv.h "Change of anchor basis"), independent of the kernels: the
transform, the two layouts as explicit index functions, the per-point statistics, the maximum, the norm's backward partials and
the spectral weights; and numpy emulations of the three arithmetic families (what tests/test_basis_spec.py measures the
real-data margins with).  Nothing here needs the library or a device."""
import numpy as np

from gemm_ref import bf16_rne, split3

F32, F64 = np.float32, np.float64
U24 = 2.0 ** -24
FAMILIES = ("f32", "x3", "bf16")      # so3_basis_kernel<float>, so3_basis_x3_kernel, so3_basis_bf16_kernel


# ------------------------------------------------------------------------------------------------ layouts
def blocks_of(dims):
    """blocks i32[na][2] = (first spectral row of the irreducible block, d*d) per spectral row, blocks of d*d rows in order."""
    rows, base = [], 0
    for d in dims:
        rows += [(base, d * d)] * (d * d)
        base += d * d
    return np.asarray(rows, dtype=np.int32)


def plain_index(pts, na, c):
    """i64[pts][na][c]: the flat element offset of (point, row, channel) in the plain channels-last layout."""
    pt, r, ch = np.ogrid[:pts, :na, :c]
    return ((pt * na + r) * c + ch).astype(np.int64)


def spectral_index(blocks, pts, c):
    """i64[pts][na][c]: ((base_f pts + pt d2_f + (f - base_f)) c + ch), row f of a point inside the buffer of its block."""
    blocks = np.asarray(blocks, dtype=np.int64)
    na = blocks.shape[0]
    pt, f, ch = np.ogrid[:pts, :na, :c]
    base, d2 = blocks[:, 0].reshape(1, na, 1), blocks[:, 1].reshape(1, na, 1)
    return (base * pts + pt * d2 + (f - base)) * c + ch


def layout_index(spectral, blocks, pts, c):
    return spectral_index(blocks, pts, c) if spectral else plain_index(pts, len(blocks), c)


def to_flat(x, index, check=False):
    """logical [pts][na][c] -> the flat buffer of the layout (both layouts are bijections onto pts*na*c elements; check=True
    asserts it)."""
    flat = np.empty(x.size, dtype=x.dtype)
    if check:
        assert np.array_equal(np.sort(index.reshape(-1)), np.arange(x.size)), "the layout is not a bijection"
    flat[index.reshape(-1)] = x.reshape(-1)
    return flat


def from_flat(flat, index):
    return np.asarray(flat).reshape(-1)[index]


# ------------------------------------------------------------------------------------------------ the operations
def transform(M, x):
    """Out[pt][r][ch] = sum_s M[r][s] In[pt][s][ch] in float64."""
    return np.einsum("rs,psc->prc", np.asarray(M, F64), np.asarray(x, F64))


def abs_budget(M, x):
    """S[pt][r][ch] = sum_s |M[r][s]| |In[pt][s][ch]|."""
    return np.einsum("rs,psc->prc", np.abs(np.asarray(M, F64)), np.abs(np.asarray(x, F64)))


def stored(out64, family):
    """The float64 result as the family stores it: float32, or one rounding to bf16."""
    o = np.asarray(out64, F64).astype(F32)
    return bf16_rne(o) if family == "bf16" else o


def point_stats(out_stored):
    """f64[pts][c][2] = (sum, sum of squares) over the rows of every point, of the values AS STORED."""
    o = np.asarray(out_stored, F64)
    return np.stack((o.sum(1), (o * o).sum(1)), -1)


def amax(out_stored):
    """max |stored finite output| as float32 (0 when there is none)."""
    o = np.abs(np.asarray(out_stored, F32))
    o = o[np.isfinite(o)]
    return F32(o.max()) if o.size else F32(0)


def norm_params(sums, groups, pts_per_group, na, eps, frozen=False):
    """(mean, rstd) f64[groups][c] of sb_norm_load, restated: frozen statistics are (mean, var) as they are; the others are
    m = s1 inv, var = max(s2 inv - m^2, 0) with inv the float32 1 / (float(pts_per_group) float(na)) the launcher passes."""
    s = np.asarray(sums, F64).reshape(groups, -1, 2)
    if frozen:
        return s[..., 0], 1.0 / np.sqrt(s[..., 1] + F64(F32(eps)))
    inv = F64(F32(1.0) / (F32(pts_per_group) * F32(na)))
    m = s[..., 0] * inv
    var = np.maximum(s[..., 1] * inv - m * m, 0.0)
    return m, 1.0 / np.sqrt(var + F64(F32(eps)))


def norm_on_load(x, mean, rstd, gamma, beta, slope, pts_per_group):
    """leaky((x - mean) rstd gamma + beta) of x [pts][na][c] with the group of point pt = pt // pts_per_group: (y, n, xhat)."""
    pts, na, c = x.shape
    g = np.arange(pts) // pts_per_group if mean.shape[0] > 1 else np.zeros(pts, dtype=np.int64)
    xhat = (np.asarray(x, F64) - mean[g][:, None, :]) * rstd[g][:, None, :]
    n = xhat * (np.asarray(gamma, F64) if gamma is not None else 1.0) + (np.asarray(beta, F64) if beta is not None else 0.0)
    return np.where(n > 0, n, n * F64(F32(slope))), n, xhat


def dstats(dy_stored, n, xhat, slope):
    """f64[pts][c][2] = (sum d, sum d xhat) over the rows of every point, d = dy leaky'(n); sum |d xhat| and sum |d| (budgets)."""
    d = np.asarray(dy_stored, F64) * np.where(n > 0, 1.0, F64(F32(slope)))
    return np.stack((d.sum(1), (d * xhat).sum(1)), -1), np.abs(d * xhat).sum(1), np.abs(d).sum(1)


# ------------------------------------------------------------------------------------------------ spectral weights
def dim_of(d2):
    d = int(round(d2 ** 0.5))
    assert d * d == d2 and 1 <= d <= 7, "block dimensions above 7 are not supported (include/epn_so3conv.h)"
    return d


def weight_index(blocks, cin, cout, transposed):
    """i64[na][cin][cout]: the flat offset of What value (f, c, o) -- block rho at base cin cout as a row-major [d cin][d cout]
    matrix with row (j, c) and column (i, o), f = base + i d + j; transposed: [d cout][d cin] with row (i, o), column (j, c)."""
    blocks = np.asarray(blocks, dtype=np.int64)
    na = blocks.shape[0]
    idx = np.empty((na, cin, cout), dtype=np.int64)
    c, o = np.ogrid[:cin, :cout]
    for f in range(na):
        base, d = int(blocks[f, 0]), dim_of(int(blocks[f, 1]))
        i, j = divmod(f - base, d)
        if transposed:
            idx[f] = base * cin * cout + (i * cout + o) * (d * cin) + j * cin + c
        else:
            idx[f] = base * cin * cout + (j * cin + c) * (d * cout) + i * cout + o
    return idx


def spectral_weights(W, R):
    """What[f][c][o] = sum_k W[o][c][k] R[f][k] in float64 (logical; weight_index places it)."""
    return np.einsum("ock,fk->fco", np.asarray(W, F64), np.asarray(R, F64))


def spectral_weights_bwd(gwhat_logical, R):
    """dW[o][c][k] = sum_f dWhat[f][c][o] R[f][k]."""
    return np.einsum("fco,fk->ock", np.asarray(gwhat_logical, F64), np.asarray(R, F64))


# ------------------------------------------------------------------------------------------------ emulations of the families
def _partials(acc, Mp, xp, keep, na):
    """acc += the kept (plane of M, plane of x) products in the kernels' order (32 contraction rows, then the kept terms, then the
    rows of the term), as ONE fp32 chain with a rounding per product.  What v_mfma_f32_16x16x32_bf16 does with its 32 products
    inside is not documented; the f32 MFMA is a k-ordered fmaf chain, and this model gives the bf16 one no more than that: a
    rounding per product is the most a summation of these products in any order can make."""
    for k0 in range(0, na, 32):
        for a, b in keep:
            for s in range(k0, min(k0 + 32, na)):
                part = Mp[a][:, s].astype(F64)[None, :, None] * xp[b][:, s, :].astype(F64)[:, None, :]
                acc = (acc.astype(F64) + part).astype(F32)
    return acc


X3_KEPT = ((0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0))      # the six EPN_SB_TERM products: (plane of M, plane of x)


def emulate(family, M, x, rounded=True):
    """The family's arithmetic on logical x [pts][na][c] -> what it stores (float32 array; bf16 values for the bf16 family, the
    fp32 accumulator instead with rounded=False).
    f32: sequential fp32 accumulation over s, one rounding per step -- the k-ordered fmaf chain v_mfma_f32_16x16x4_f32 is
         (the kernel reproduces this emulation bit for bit).
    x3:  M and x in three bf16 planes, the six kept products.   bf16: hi + lo of M against the bf16 inputs, one store rounding."""
    M = np.asarray(M, F32)
    x = np.asarray(x, F32)
    acc = np.zeros((x.shape[0], M.shape[0], x.shape[2]), F32)
    if family == "f32":
        for s in range(M.shape[1]):
            acc = (acc.astype(F64) + M[:, s].astype(F64)[None, :, None] * x[:, s, :].astype(F64)[:, None, :]).astype(F32)
        return acc
    if family == "x3":
        return _partials(acc, split3(M), split3(x), X3_KEPT, M.shape[1])
    hi = bf16_rne(M)
    lo = bf16_rne((M - hi).astype(F32))
    assert np.array_equal(bf16_rne(x), x), "the bf16 family reads bf16 values"
    acc = _partials(acc, (hi, lo), (x,), ((0, 0), (1, 0)), M.shape[1])
    return bf16_rne(acc) if rounded else acc
