"""Case tables of the basis-change tests (tests/test_gpu_basis_exact.py on the device, tests/test_basis_spec.py without one):
the shapes, the operand sets, the restated dispatch of so3_basis_any (csrc/so3_basis.hip) and the instances it can reach.

Operand sets (logical x [pts][na][c], M [na][na]):
  P   M a random signed permutation, x full-mantissa values (bf16 family: their bf16 roundings): every output is +- one input.
  I   M integers in [-1000, 1000], x integers in [-250, 250] with sum |M||x| < 2^24: exact in any order, every slot has weight.
  Is  the same with |M| <= 2, |x| <= 3: the sums of squares of a point's outputs stay below 2^24 as well (the statistics).
  S   x selects: one +-2^e per (point, channel); M full-mantissa (bf16 family: 16-bit mantissas): the output is a column of M.
      bf16 family, odd channels: x holds +2^e in row 2k and -2^e in row 2k+1, and column 2k+1 of M is the bf16 rounding of
      column 2k, so the output is the LOW plane of M times 2^e (the single rounding of a stored bf16 output returns the high
      plane of a lone column whatever the low plane holds; the pair is what sees a dropped low plane).
  X   (x3 only) M = signed permutation times 1 + 2^-9 (planes: 1, 2^-9, 0), x twelve-bit values (planes: 8 bits, 4 bits, 0): the
      product has 22 bits and is the sum of the four kept hi / mid cross terms, am bm included."""
from collections import namedtuple

import numpy as np
import torch

import basis_ref as B
import gemm_ref as R

F32, F64 = np.float32, np.float64
EPN_EINVAL = -1
DIMS = {60: [1, 3, 3, 4, 5], 64: [1, 3, 3, 4, 5, 2], 12: [1, 1, 1, 3], 4: [2]}
DIRECTIONS = ((0, 0), (0, 1), (1, 0), (1, 1))        # (in_spectral, out_spectral)
ESZ = {"f32": 4, "x3": 4, "bf16": 2}
Shape = namedtuple("Shape", "na c pts in_spec out_spec")


def sid(s):
    return f"a{s.na}_c{s.c}_p{s.pts}_{'s' if s.in_spec else 'p'}{'s' if s.out_spec else 'p'}"


# ------------------------------------------------------------------------------------------------ dispatch, restated
def is_small(family, na, c, pts):
    """so3_basis_any: 32-bit row offsets when the tensor is below 2 GiB, pts < 2^24 and a point's stride fits 24 bits (the stride
    test is in fp32 bytes for every family)."""
    return pts * na * c * ESZ[family] < 0x7fffff00 and pts < (1 << 24) and na * c * 4 < (1 << 24)


def is_pair(family, na, c, pts):
    """Two points per task: c == 32 below 2 GiB (and only in the SMALL kernels, which c == 32 always selects: na <= 64)."""
    return c == 32 and pts * na * c * ESZ[family] < 0x7fffff00 and pts < (1 << 24)


def instance(family, na, c, pts, frozen=False):
    t = lambda b: "true" if b else "false"
    small = is_small(family, na, c, pts)
    if family == "f32":
        return f"so3_basis_kernel<float,{t(small)},{t(frozen)}>"
    return f"so3_basis_{family}_kernel<{t(small)},{t(frozen)}>"


def phantom_lanes(family, na, c, pts):
    """Lanes that own no channels exist: the second point of the last pair task, or lanes x >= 8 of a half-empty last block."""
    return (pts % 2 == 1) if is_pair(family, na, c, pts) else (c % 64 == 32)


BASIS_INSTANCES = {instance(f, 60, c, 1, fr) for f in B.FAMILIES for c in (64, 1 << 17) for fr in (False, True)}
WEIGHT_INSTANCES = {"spectral_weights_kernel<false,float>", "spectral_weights_kernel<true,float>",
                    "spectral_weights_kernel<false,bf16>", "spectral_weights_kernel<true,bf16>", "spectral_weights_bwd_kernel"}
REACHABLE = BASIS_INSTANCES | WEIGHT_INSTANCES


def normalise(name):
    from gemm_cases import normalise as n
    return n(name)


# ------------------------------------------------------------------------------------------------ shapes
def _transform_shapes():
    """na = 60: every width x every point count, the direction cycling so that each width and each count meets all four;
    na = 64 (no padding rows), 12 and 4 (the entry's minimum): pair mode and the half-empty block at an even count, at odd counts
    on either side of a workgroup's 16 tasks, and the full widths at 2 points."""
    out, k = [], 0
    for c in (32, 64, 96, 128):
        for pts in (1, 2, 15, 16, 17, 33, 65):
            out.append(Shape(60, c, pts, *DIRECTIONS[k % 4]))
            k += 1
    for na in (64, 12, 4):
        for c, pts in ((32, 1), (32, 17), (32, 33), (96, 1), (96, 17), (96, 33), (64, 2), (128, 2)):
            out.append(Shape(na, c, pts, *DIRECTIONS[k % 4]))
            k += 1
    return out


TRANSFORM_SHAPES = _transform_shapes()
SETS = {"f32": ("P", "I", "S"), "x3": ("P", "I", "S", "X"), "bf16": ("P", "I", "S")}
# the 64-bit-address instances without 2 GiB tensors: na c 4 >= 2^24
BIG_SHAPES = ((60, 69920, 3), (64, 65536, 2))
STATS_SHAPES = [Shape(60, 32, 17, 1, 0), Shape(60, 96, 33, 0, 0), Shape(64, 64, 2, 1, 0), Shape(12, 128, 16, 0, 0),
                Shape(4, 32, 2, 1, 0)]
AMAX_SHAPES = [Shape(60, 96, 17, 0, 1), Shape(60, 32, 15, 0, 0), Shape(64, 32, 1, 0, 1), Shape(60, 64, 16, 0, 1),
               Shape(60, 69920, 3, 0, 1)]
# (shape, groups): c takes the widths the norm glue takes (c / 4 a power of two); odd pts_per_group at c = 32 makes a pair task
# straddle two groups
NORM_SHAPES = [(Shape(60, 32, 15, 0, 1), 3), (Shape(60, 32, 17, 0, 0), 1), (Shape(60, 64, 33, 0, 1), 3), (Shape(64, 128, 2, 0, 0), 1),
               (Shape(12, 32, 9, 0, 1), 3)]
DSTATS_SHAPES = [(Shape(60, 32, 15, 1, 0), 3), (Shape(60, 96, 17, 1, 0), 1), (Shape(64, 64, 2, 1, 0), 1), (Shape(60, 128, 33, 1, 0), 3)]
DSTATS_TAU = 1.0e-3
DSTATS_SLOPE = 0.25
# roundings between an element and point_dstats[..][1] at mean 0 (dstats_ref derives the count and the mean's terms)
DSTATS_K = 24
REAL_CASES = [(c, d) for c in (32, 64, 96) for d in ("fwd", "inv")]
REAL_PTS = 33


def _seed(*k):
    return int(sum((i + 1) * 7919 * int(v) for i, v in enumerate(k)) % (1 << 31))


def blocks(na):
    return B.blocks_of(DIMS[na])


# ------------------------------------------------------------------------------------------------ operand sets
def signed_perm(na, seed):
    rng = np.random.default_rng(seed)
    perm, sign = rng.permutation(na), rng.choice(np.array([-1.0, 1.0]), na)
    M = np.zeros((na, na), F32)
    M[np.arange(na), perm] = sign
    return M, perm, sign


def _t(a):
    return a.numpy() if isinstance(a, torch.Tensor) else a


def sixteen_bit(shape, seed):
    """sign (1 + i / 2^15): 16-bit mantissas, exactly hi + lo of the bf16 family's split."""
    rng = np.random.default_rng(seed)
    return ((1.0 + rng.integers(0, 1 << 15, shape) / float(1 << 15)) * rng.choice(np.array([-1.0, 1.0]), shape)).astype(F32)


def operands(family, kind, na, c, pts, with_ref=True):
    """(M f32[na][na], x f32[pts][na][c] logical, ref f64 -- the exact result, representable as the family stores it after at
    most the one bf16 rounding basis_ref.stored applies)."""
    seed = _seed(na, c, pts, len(kind), ord(kind[0]))
    bf = family == "bf16"
    if kind in ("P", "X"):
        M, perm, sign = signed_perm(na, seed)
        if kind == "X":
            M = (M * F32(1.0 + 2.0 ** -9)).astype(F32)
            x = _t(R.twelve_bit((pts * na, c), seed + 1)).reshape(pts, na, c)
        else:
            x = _t(R.full_mantissa((pts * na, c), seed + 1)).reshape(pts, na, c)
            x = R.bf16_rne(x) if bf else x
        scale = F64(M[0, perm[0]]) * sign[0]          # |entry| of M
        ref = x[:, perm, :].astype(F64) * (sign * scale)[None, :, None] if with_ref else None
        return M, np.ascontiguousarray(x, F32), ref
    if kind in ("I", "Is"):
        qm, qx = (1000, 250) if kind == "I" else (2, 3)
        M = _t(R.ints((na, na), qm, seed)).astype(F32)
        x = _t(R.ints((pts * na, c), qx, seed + 1)).reshape(pts, na, c).astype(F32)
        return M, x, (B.transform(M, x) if with_ref else None)
    assert kind == "S"
    rng = np.random.default_rng(seed)
    M = sixteen_bit((na, na), seed) if bf else _t(R.full_mantissa((na, na), seed))
    val = np.ldexp(1.0, rng.integers(-8, 9, (pts, c))) * rng.choice(np.array([-1.0, 1.0]), (pts, c))
    x = np.zeros((pts, na, c), F32)
    pt, ch = np.meshgrid(np.arange(pts), np.arange(c), indexing="ij")
    if bf:
        M[:, 1::2] = R.bf16_rne(M[:, 0::2])
        row = 2 * rng.integers(0, na // 2, (pts, c))
        x[pt, row, ch] = val
        odd = (ch % 2 == 1)
        x[pt[odd], row[odd] + 1, ch[odd]] = -val[odd]
    else:
        x[pt, rng.integers(0, na, (pts, c)), ch] = val
    return M.astype(F32), x, (B.transform(M, x) if with_ref else None)


def stats_over_256(na=12, c=64, pts=5):
    """bf16 statistics case: integer outputs up to 600, so the stored values are multiples of 2 and 4 and differ from the exact
    ones; the sums of the ROUNDED values and of their squares stay below 2^24."""
    M = _t(R.ints((na, na), 5, 31)).astype(F32)
    x = _t(R.ints((pts * na, c), 10, 32)).reshape(pts, na, c).astype(F32)
    return M, x, B.transform(M, x)


# ------------------------------------------------------------------------------------------------ norm on load / dstats inputs
def norm_inputs(family, s, groups, affine, seed=0):
    """x [pts][na][c] normal around a per-channel mean (values the family stores), sums f32[groups][c][2] of x in float64 rounded
    once, gamma / beta (None without affine)."""
    rng = np.random.default_rng(_seed(s.na, s.c, s.pts, groups, seed))
    x = (rng.standard_normal((s.pts, s.na, s.c)) * rng.uniform(0.3, 3.0, s.c) + rng.uniform(-1.0, 1.0, s.c)).astype(F32)
    x = R.bf16_rne(x) if family == "bf16" else x
    xg = x.astype(F64).reshape(groups, -1, s.c)
    sums = np.stack((xg.sum(1), (xg * xg).sum(1)), -1).astype(F32)
    gamma = rng.uniform(0.5, 1.5, s.c).astype(F32) * rng.choice(np.array([-1.0, 1.0], F32), s.c) if affine else None
    beta = rng.normal(0.0, 0.5, s.c).astype(F32) if affine else None
    return x, sums, gamma, beta


def frozen_stats(c, seed):
    rng = np.random.default_rng(seed)
    return np.stack((rng.uniform(-1.0, 1.0, c), rng.uniform(0.25, 4.0, c)), -1).astype(F32)


def exact_frozen(family, na, c, pts):
    """A frozen norm on load that is exact in fp32: var = 1, eps = 0 (rstd = 1), gamma = +-2^k, beta = 0, slope = 1/4, the mean a
    multiple of the inputs' grid (x - mean has at most 18 bits).  -> (M, x, stats, gamma, slope, ref f64): the 64-bit-path
    frozen cases, whose widths the norm glue does not take."""
    seed = _seed(na, c, pts, 77)
    rng = np.random.default_rng(seed)
    bits = 7 if family == "bf16" else 16
    M, perm, sign = signed_perm(na, seed)
    x = ((1.0 + rng.integers(0, 1 << bits, (pts, na, c)) / float(1 << bits)) * rng.choice(np.array([-1.0, 1.0]), (pts, na, c))).astype(F32)
    mean = (rng.integers(-(1 << bits), (1 << bits) + 1, c) / float(1 << bits)).astype(F32)
    stats = np.stack((mean, np.ones(c, F32)), -1).astype(F32)
    gamma = (np.ldexp(1.0, rng.integers(-2, 3, c)) * rng.choice(np.array([-1.0, 1.0]), c)).astype(F32)
    n = (x.astype(F64) - mean.astype(F64)) * gamma.astype(F64)
    y = np.where(n > 0, n, 0.25 * n)
    y = B.stored(y, family).astype(F64)            # bf16: the kernel rounds the normalised value as the unfolded path stores it
    return M, x, stats, gamma, 0.25, y[:, perm, :] * sign[None, :, None]


DSTATS_KAPPA = (1.0, -0.5, 2.0)      # mean / std of the groups' channels: every group has its own nonzero mean


def dstats_inputs(family, s, groups):
    """The gradient (spectral side, integers: every sum of d = dy or dy / 4 is exact), the signed permutation, and x from
    norm_ref.real_inputs, one call per group with the group's own kappa = mean / std (DSTATS_KAPPA) and spread of variances, so
    that no pre-activation lies within DSTATS_TAU of zero under the group's OWN statistics; sums[g][c] = (sum x, sum x^2) of the
    group in float64, rounded once -- the genuine batch (groups = 1) / instance statistics; gamma, beta."""
    import norm_ref as N
    seed = _seed(s.na, s.c, s.pts, groups, 5)
    rng = np.random.default_rng(seed)
    dt = torch.bfloat16 if family == "bf16" else torch.float32
    M, perm, sign = signed_perm(s.na, seed)
    g = rng.integers(-8, 9, (s.pts, s.na, s.c)).astype(F32)
    gamma = (rng.uniform(0.5, 1.5, s.c) * rng.choice(np.array([-1.0, 1.0]), s.c)).astype(F32)
    beta = rng.normal(0.0, 0.5, s.c).astype(F32)
    ppg = s.pts // groups
    xs, left = [], 0
    for gi in range(groups):
        x4, n = N.real_inputs((1, s.c, ppg, s.na), DSTATS_KAPPA[gi % 3], seed + gi, DSTATS_TAU, kind="batch",
                              gamma=torch.from_numpy(gamma).double(), beta=torch.from_numpy(beta).double(), eps=1e-5, dtype=dt)
        xs.append(x4[0].permute(1, 2, 0).numpy())
        left += n
    x = np.concatenate(xs, 0).astype(F32)
    xg = x.astype(F64).reshape(groups, ppg * s.na, s.c)
    sums = np.stack((xg.sum(1), (xg * xg).sum(1)), -1).astype(F32)
    return dict(M=M, perm=perm, sign=sign, g=g, x=x, sums=sums, gamma=gamma, beta=beta, eps=1e-5, left=left, ppg=ppg)


def dstats_ref(family, s, groups, d):
    """(dy f64 logical, point_dstats f64[pts][c][2], tolerance of point_dstats[..][1], n, k2 f64[groups][c]).  The statistics
    are those the kernel computes, restated in float64 from the same float32 sums (basis_ref.norm_params).  Tolerance, with
    u = 2^-24 and k2 = mean^2 / (var + eps) of the point's group and channel:
        u [ (DSTATS_K + 3.5 k2) sum |d xhat| + 2 sqrt(k2) sum |d| ]
    counted on sb_point_dstats: inv = 1 / rows and m = s1 inv round once each (m: 2 u); var = s2 inv - m m: the product s2 inv
    2 u of var + m^2, m m 5 u of m^2, the subtraction 1 u -> u (3 + 7 k2) of var + eps; var + eps 1 u; halved by the root:
    u (2 + 3.5 k2), rsqrtf 1 ulp = 2 u; x - m rounds once (1 u of xhat) and carries the mean's 2 u |m| = 2 u sqrt(k2) in units of
    xhat -- the term that is NOT proportional to |xhat| and therefore stands against sum |d|; the product with rstd 1 u: xhat is
    off by u [(6 + 3.5 k2) |xhat| + 2 sqrt(k2)].  A lane's chain of 16 fmaf, one rounding each relative to at most
    sum |d xhat|: 16; the two shuffle adds: 2.  DSTATS_K = 6 + 16 + 2."""
    dy = d["g"][:, d["perm"], :].astype(F64) * d["sign"][None, :, None]
    mean, rstd = B.norm_params(d["sums"], groups, d["ppg"], s.na, d["eps"])
    k2 = mean * mean * rstd * rstd
    _, n, xhat = B.norm_on_load(d["x"], mean, rstd, d["gamma"], d["beta"], DSTATS_SLOPE, d["ppg"])
    ds, sum_dx, sum_d = B.dstats(dy, n, xhat, DSTATS_SLOPE)
    gi = np.arange(s.pts) // d["ppg"] if groups > 1 else np.zeros(s.pts, dtype=np.int64)
    tol = B.U24 * ((DSTATS_K + 3.5 * k2[gi]) * sum_dx + 2.0 * np.sqrt(k2[gi]) * sum_d)
    return dy, ds, tol, n, k2


# ------------------------------------------------------------------------------------------------ real data
_REAL = {}


def shipped_basis():
    import epn_pointcloud_amd  # noqa: F401
    from epn_pointcloud_amd import so3_fourier
    from epn_pointcloud_amd.vgtk.so3conv import functional as L
    b = so3_fourier.build(np.asarray(L.get_intra_idx()))
    assert list(b["dims"]) == DIMS[60]
    return np.ascontiguousarray(b["U"], F32)


def real_case(family, c, direction):
    """Shipped U (inverse: in spectral, M = U) or U^T (forward: out spectral), normal inputs -> dict(M, x, ref f64, S, shape,
    ratio: the emulated family's worst |emulation - fp64| / (2^-24 S), before the bf16 store rounding)."""
    key = (family, c, direction)
    if key not in _REAL:
        U = shipped_basis()
        M = np.ascontiguousarray(U.T) if direction == "fwd" else U
        rng = np.random.default_rng(_seed(c, len(direction)))
        x = rng.standard_normal((REAL_PTS, 60, c)).astype(F32)
        x = R.bf16_rne(x) if family == "bf16" else x
        ref, S = B.transform(M, x), B.abs_budget(M, x)
        emu = B.emulate(family, M, x, rounded=False).astype(F64)
        s = Shape(60, c, REAL_PTS, 0, 1) if direction == "fwd" else Shape(60, c, REAL_PTS, 1, 0)
        _REAL[key] = dict(M=M, x=x, ref=ref, S=S, shape=s, ratio=float((np.abs(emu - ref) / (B.U24 * S)).max()))
    return _REAL[key]


def m_family(family):
    """The worst emulated ratio over the real cases of the family: the GPU test allows twice this."""
    return max(real_case(family, c, d)["ratio"] for c, d in REAL_CASES)


# ------------------------------------------------------------------------------------------------ spectral weights
WDIMS = {60: [[1, 3, 3, 4, 5]], 64: [[1, 1, 2, 3, 7], [1, 1, 1, 3, 4, 6]], 12: [[1, 1, 1, 3]]}
Wcase = namedtuple("Wcase", "cin cout kn na dims which")      # which: "w", "t", "wt" (what, what_t, both)


def _weight_cases():
    """(5, 7) and (32, 64): kn 1, 12, 16 x na 60, 64, the na = 64 cases alternating between the dims with a 7- and with a
    6-dimensional block, the outputs cycling through what / what_t / both.  (256, 256) (6 row slices) and (512, 512) (4 row
    slices) are large: kn 12 and 16 only, and (512, 512) with 60 rows is 63 MB per layout in fp32, so it runs with what_t alone
    there, with both layouts at 12 rows, and with `what` alone in bf16."""
    out, k, k64 = [], 0, 0
    for cin, cout in ((5, 7), (32, 64)):
        for kn in (1, 12, 16):
            for na in (60, 64):
                dims = WDIMS[na][k64 % 2] if na == 64 else WDIMS[na][0]
                k64 += na == 64
                out.append(Wcase(cin, cout, kn, na, tuple(dims), ("w", "t", "wt")[k % 3]))
                k += 1
    out += [Wcase(256, 256, 12, 60, tuple(WDIMS[60][0]), "wt"), Wcase(256, 256, 16, 64, tuple(WDIMS[64][0]), "t"),
            Wcase(256, 256, 16, 64, tuple(WDIMS[64][1]), "w"),
            Wcase(512, 512, 12, 12, tuple(WDIMS[12][0]), "wt"), Wcase(512, 512, 12, 60, tuple(WDIMS[60][0]), "t")]
    return out


WEIGHT_CASES = _weight_cases()
WEIGHT_CASES_BF16 = WEIGHT_CASES[:-1] + [Wcase(512, 512, 12, 60, tuple(WDIMS[60][0]), "w")]


def wid(w):
    return f"{w.cin}x{w.cout}_k{w.kn}_a{w.na}_d{max(w.dims)}_{w.which}"


def weight_slices(cin, cout):
    grid = (cin * cout + 255) // 256
    return 4 if grid >= 1024 else (6 if grid >= 256 else 12)


def weight_operands(w, kind):
    """(W f32[cout][cin][kn], R f32[na][kn]): integers, or a one-hot W (+-2^e at one k per (o, c)) against full-mantissa R."""
    seed = _seed(w.cin, w.cout, w.kn, w.na, len(kind))
    if kind == "I":
        return (_t(R.ints((w.cout * w.cin, w.kn), 15, seed)).reshape(w.cout, w.cin, w.kn).astype(F32),
                _t(R.ints((w.na, w.kn), 7, seed + 1)).astype(F32))
    m, _, _ = R.selection_rows(w.cout * w.cin, w.kn, seed)
    return _t(m).reshape(w.cout, w.cin, w.kn).astype(F32), _t(R.full_mantissa((w.na, w.kn), seed + 1)).astype(F32)


def weight_grad_operands(w, kind):
    """(dWhat f32[na][cin][cout] logical, R): integers, or one +-2^e per (c, o) in a random spectral row."""
    seed = _seed(w.cin, w.cout, w.kn, w.na, len(kind), 3)
    if kind == "I":
        return (_t(R.ints((w.na, w.cin * w.cout), 3, seed)).reshape(w.na, w.cin, w.cout).astype(F32),
                _t(R.ints((w.na, w.kn), 7, seed + 1)).astype(F32))
    m, _, _ = R.selection_rows(w.cin * w.cout, w.na, seed)
    return (np.ascontiguousarray(_t(m).reshape(w.cin, w.cout, w.na).transpose(2, 0, 1)).astype(F32),
            _t(R.full_mantissa((w.na, w.kn), seed + 1)).astype(F32))
