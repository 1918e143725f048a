"""Case tables, builders and the restated dispatch of the exact tests of the PointNet head (csrc/pointnet.hip):
tests/test_gpu_pointnet_exact.py on the device, tests/test_pointnet_spec.py without one.  Nothing here needs a device.

Why `==` is legitimate: features, W, bias and the upstream gradient are small integers, anchors signed permutation matrices,
coordinates multiples of 1/8 in [-1, 1] laid out as +- pairs around a dyadic per-cloud mean (plus the mean itself when p is odd),
so the fp32 sequential sum of a coordinate row is exact and so is its division by p.  Every term of every output is then a
multiple of 1/8 and every partial sum stays below 2^24 such units: the result is the same float under any summation or atomic
order.  build() PROVES that for the case it returns (assertions on float64 sums and on an fp32 replay of the mean).

Small integers tie all the time, which is the point: which of several equal maxima wins is visible in arg, dF and dW of nearly
every case.  The tie cases place exact copies of a point at chosen distances on top of that."""
from collections import namedtuple

import numpy as np

import pointnet_ref as P
from conv_cases import _rotations24, hash_name, normalise  # noqa: F401  (normalise: the tests' spelling of kernel names)
from gemm_ref import bf16_rne

EPN_EINVAL = -1
UNIT = 8.0                      # every term is a multiple of 1 / UNIT
Q = 3                           # operand magnitude
_CACHE = {}

# name, clouds, points, anchors (1: anchors NULL), channels, output channels, bias given, ((original, copy), ...) of the tie
# builder, index of a cloud whose points are all identical (or None)
PnCase = namedtuple("PnCase", "name b p a c co bias ties ident", defaults=(True, (), None))
# routing: "fwd" (the forward pass's own arg-max) | "random" | an integer (every column routed to that point; -1: p - 1)
BwdCase = namedtuple("BwdCase", "name b p a c co routing bias", defaults=(True,))
DzCase = namedtuple("DzCase", "name b p a co")


# ------------------------------------------------------------------------------------------------ dispatch restatement
def fwd_kernel(c):
    """epn_pointnet_so3conv_fwd_f32: the MFMA kernel iff c % 16 == 0."""
    return "pointnet_fwd_mfma_kernel" if c % 16 == 0 else "pointnet_fwd_kernel"


KERNEL = dict(bwd_data="pointnet_bwd_data_kernel", bwd_weight="pointnet_bwd_weight_kernel", max="pointnet_max_kernel",
              dz_f32="pointnet_dz_kernel<float>", dz_bf16="pointnet_dz_kernel<__bf16>", bwd_coord="pointnet_bwd_coord_kernel")
REACHABLE_POINTNET = {"pointnet_fwd_mfma_kernel", "pointnet_fwd_kernel"} | set(KERNEL.values())


def weight_slices(nba):
    """launcher of pointnet_bwd_weight_kernel: (slices, (b, a) pairs per slice, empty slices)."""
    slices = min(nba, 16)
    per = (nba + slices - 1) // slices
    return slices, per, sum(1 for y in range(slices) if y * per >= nba)


# ------------------------------------------------------------------------------------------------ the cases
# One edge per case, the smallest shapes on both sides of it; b <= 3.
C = PnCase
_V = dict(b=2, p=33, a=2, c=5, co=9)            # VALU forward (c % 16 != 0): tiles of 32 points, 64 channels, 128 outputs
_M = dict(b=2, p=17, a=2, c=16, co=8)           # MFMA forward: tiles of 64 points (4 x 16, lane groups of 4), chunks of 64 channels


def _vary(prefix, base, **axes):
    out = []
    for key, values in axes.items():
        for v in values:
            out.append(C(f"{prefix}_{key}{v}", **{**base, key: v}))
    return out


FWD_CASES = (
    _vary("valu", _V, c=(1, 4, 63, 65, 70), p=(1, 31, 32, 33, 65), co=(1, 127, 128, 129), a=(1, 2))
    + [C("valu_nobias", **_V, bias=False), C("valu_b3_p2", **{**_V, "b": 3, "p": 2})]
    + _vary("mfma", _M, c=(16, 48, 64, 80, 144), p=(1, 3, 4, 15, 16, 17, 63, 64, 65, 129),
            co=(1, 15, 17, 31, 33, 127, 128, 129, 257), a=(1, 2, 60))
    + [C("mfma_nobias", **_M, bias=False), C("mfma_p2_co33", **{**_M, "p": 2, "co": 33})]
)

# Where the copy sits relative to its original; two pairs per case (A and B carry opposite features and opposite coordinate
# offsets, so that one of them is the maximum of most columns).
PLACES = {
    "same_lane_group": ((4, 6), (5, 7)),            # indices 4j .. 4j + 3 of a 16-tile: one lane of the MFMA kernel
    "other_lane_group": ((1, 9), (2, 14)),          # the same 16-tile, another lane group: the cross-lane combine
    "other_tile16": ((2, 18), (3, 35)),             # another 16-tile of the same lane group
    "across_tile32": ((30, 34), (31, 33)),          # the VALU kernel's point tile
    "across_tile64": ((60, 70), (63, 64)),          # the point tile of the MFMA and of the max kernel
    "across_unroll8": ((7, 8), (15, 16)),           # the 8-row unrolled scan of pointnet_max_kernel
}
TIE_P, TIE_CO = 75, 24
TIE_CASES = ([C(f"tie_valu_{k}", 2, TIE_P, 2, 5, TIE_CO, True, v) for k, v in PLACES.items()]
             + [C(f"tie_mfma_{k}", 2, TIE_P, 2, 16, TIE_CO, True, v) for k, v in PLACES.items()]
             + [C("tie_valu_identical_cloud", 2, 37, 2, 5, TIE_CO, True, (), 1),
                C("tie_mfma_identical_cloud", 2, 37, 2, 16, TIE_CO, True, (), 1)])

# epn_pointnet_max_f32: Z supplied directly (exact), bias NULL, anchors NULL; 256 output channels per workgroup, 64-point tiles,
# rows scanned in eights
_X = dict(b=2, p=9, a=1, c=16, co=8, bias=False)
MAX_CASES = _vary("max", _X, co=(8, 248, 256, 264), p=(1, 7, 8, 9, 63, 64, 65, 72, 129)) + [C("max_a2_bias", 2, 9, 2, 16, 8, True)]

B = BwdCase
_D = dict(b=2, p=5, a=2, c=5, co=8)
BWD_DATA_CASES = (
    [B(f"dF_co{v}", **{**_D, "co": v}, routing="fwd") for v in (1, 3, 4, 5, 7, 9)]
    + [B(f"dF_c{v}", **{**_D, "c": v, "co": 5}, routing="fwd") for v in (1, 127, 128, 129)]
    + [B(f"dF_p{v}", **{**_D, "p": v, "co": 7}, routing="random") for v in (1, 63, 64, 65, 130)]
    + [B("dF_all0", **{**_D, "p": 65, "co": 7}, routing=0), B("dF_all_last", **{**_D, "p": 65, "co": 7}, routing=-1),
       B("dF_all63", **{**_D, "p": 65, "co": 7}, routing=63), B("dF_all64", **{**_D, "p": 65, "co": 7}, routing=64),
       B("dF_all63_p64", **{**_D, "p": 64, "co": 6}, routing=63), B("dF_fwd_p130", **{**_D, "p": 130, "co": 9}, routing="fwd")]
)
_BA = {1: (1, 1), 7: (1, 7), 8: (2, 4), 9: (3, 3), 15: (3, 5), 16: (2, 8), 17: (1, 17), 33: (3, 11), 128: (2, 64), 131: (1, 131)}
BWD_WEIGHT_CASES = (
    [B(f"dW_ba{n}", b, 5, a, 5, 3, "fwd" if n % 2 else "random") for n, (b, a) in _BA.items()]
    + [B(f"dW_c{v}", 3, 5, 3, v, 3, "fwd") for v in (1, 253, 254, 256)]
    + [B("dW_co1", 3, 5, 3, 5, 1, "fwd"), B("dW_nobias", 1, 5, 17, 5, 3, "random", False),
       B("dW_all_last_p65", 3, 65, 11, 5, 3, -1)]
)
_CBA = {1: (1, 1), 255: (3, 85), 256: (2, 128), 257: (1, 257), 513: (3, 171)}
BWD_COORD_CASES = ([B(f"coord_ba{n}", b, 5, a, 16, 8, "random") for n, (b, a) in _CBA.items()]
                   + [B("coord_nobias", 3, 5, 85, 16, 8, "random", False), B("coord_fwd_co3", 2, 9, 2, 5, 3, "fwd")])
# octets = b p a co / 8 against the 256 threads of a workgroup
DZ_CASES = [DzCase("dz_co8_255", 3, 5, 17, 8), DzCase("dz_co8_256", 2, 8, 16, 8), DzCase("dz_co8_257", 1, 257, 1, 8),
            DzCase("dz_co16_256", 2, 8, 8, 16), DzCase("dz_co16_258", 1, 43, 3, 16), DzCase("dz_co24_255", 1, 5, 17, 24),
            DzCase("dz_co24_258", 2, 43, 1, 24)]
# every entry with b = 0 returns 0 and writes nothing, but the weight gradient (zero-fills dW and dbias) and the coordinate
# gradient (writes zeros into its three columns and dbias)
EMPTY_SHAPE = dict(p=5, a=2, c=16, co=8)
# the fused forward cases both forms of ops.pointnet_so3conv accept (c % 16 == 0, co % 8 == 0)
OPS_CASES = ([c for c in FWD_CASES if c.name in ("mfma_c16", "mfma_c48", "mfma_c80", "mfma_p1", "mfma_p3", "mfma_p65", "mfma_a1",
                                                 "mfma_nobias")]
             + [c for c in TIE_CASES if c.c % 16 == 0])

# Special values.  Fused forward: NaN features at the two points of a pair of PLACES, in one (b, a) row.  Max kernel: Z written
# directly, one pattern per pair: name -> ((point, value), ...) on a background of negative integers (first / second: the pair)
SPECIAL_PATTERNS = {
    "two_nans": lambda i, j: ((i, np.nan), (j, np.nan)),
    "nan_after_inf": lambda i, j: ((i, np.inf), (j, np.nan)),
    "nan_before_inf": lambda i, j: ((i, np.nan), (j, np.inf)),
    "inf_twice": lambda i, j: ((i, np.inf), (j, np.inf)),
    "neg_zero_first": lambda i, j: ((i, -0.0), (j, 0.0)),
    "pos_zero_first": lambda i, j: ((i, 0.0), (j, -0.0)),
}
SPECIAL_PAIRS = [v[0] for v in PLACES.values()]


def special_Z(pattern, pair, co=8, p=TIE_P):
    """Z[1][p][1][co] of the max kernel: negative integers, the pattern's two values at the pair's points in every column but the
    last (left clean); "all_neg_inf": every value -inf."""
    rng = np.random.default_rng(hash_name(f"{pattern}{pair}"))
    Z = -rng.integers(1, 9, size=(1, p, 1, co)).astype(np.float32)
    if pattern == "all_neg_inf":
        Z[:] = -np.inf
        return Z
    for point, value in SPECIAL_PATTERNS[pattern](*pair):
        Z[0, point, 0, :co - 1] = value
    return Z


# ------------------------------------------------------------------------------------------------ builders
def _ints(rng, shape, q=Q):
    """Integers in [-q, q], no zeros, as float32."""
    return (rng.integers(1, q + 1, size=shape) * (1 - 2 * rng.integers(0, 2, size=shape))).astype(np.float32)


def _coords(rng, b, p, pairs=(), ident=None):
    """xyz[b][3][p]: per cloud and coordinate a mean m (multiple of 1/8, |m| <= 1/2) and offsets +-d (d <= 1/2) in shuffled
    order, m itself when an odd point is left.  Tie pairs: the points of pair A sit at m + d, those of pair B at m - d (two and
    two: the mean stays m).  ident: that cloud's points all equal m."""
    xyz = np.empty((b, 3, p), np.float32)
    tied = [i for pr in pairs for i in pr]
    free = [i for i in range(p) if i not in tied]
    for bb in range(b):
        for j in range(3):
            m = rng.integers(-4, 5) / UNIT
            d = rng.integers(0, 5, size=len(free) // 2) / UNIT
            vals = np.concatenate([m + d, m - d, [m] * (len(free) % 2)])
            rng.shuffle(vals)
            xyz[bb, j, free] = vals
            if pairs:
                dd = rng.integers(1, 5) / UNIT
                xyz[bb, j, list(pairs[0])] = m + dd
                xyz[bb, j, list(pairs[1])] = m - dd
            if ident == bb:
                xyz[bb, j, :] = m
            # the kernels' mean: sequential fp32 sum, one division -- exact
            s = np.float32(0)
            for v in xyz[bb, j]:
                s = np.float32(s + v)
            assert np.float32(s / np.float32(p)) == np.float32(m) == np.float64(xyz[bb, j].astype(np.float64).mean()), (bb, j)
    return xyz


def _anchors(a):
    return None if a == 1 else np.ascontiguousarray(_rotations24()[np.arange(a) % 24].astype(np.float32))


def _routing(rng, c, fwd_arg):
    if c.routing == "fwd":
        return fwd_arg
    if c.routing == "random":
        return rng.integers(0, c.p, size=fwd_arg.shape).astype(np.int32)
    return np.full(fwd_arg.shape, c.routing % c.p if c.routing < 0 else c.routing, np.int32)


def _prove(c, d, r):
    """Every output of the restatement is a multiple of 1 / UNIT and every sum of absolute terms stays below 2^24 units."""
    S = P.magnitudes(d["F"], d["xyz"], d["anchors"], d["W"], d["bias"], d["gout"], r["arg"])
    bits = {k: float(v.max()) * UNIT / 2.0 ** 24 if v.size else 0.0 for k, v in S.items()}
    assert max(bits.values()) < 1.0, (c, bits)
    for k in ("out", "centre", "dF", "dW", "dbias"):
        assert np.array_equal(r[k] * UNIT, np.round(r[k] * UNIT)), (c, k)
        assert np.array_equal(r[k], r[k].astype(np.float32)), (c, k)
    return bits


def build(c):
    """The exact (or tie) case of a PnCase / BwdCase: float32 / int32 arrays at the C boundary (F, xyz, anchors or None, W, bias
    or None, gout, arg: the routing table of the backward passes), and the float64 results out, arg_fwd, centre, Z (the feature
    part of the embedding, exact in fp32), dF, dW, dbias (through `arg`), `bits` (sums of absolute terms / 2^24 units)."""
    rng = np.random.default_rng(hash_name(c.name))
    ties, ident = getattr(c, "ties", ()), getattr(c, "ident", None)
    F = _ints(rng, (c.b, c.p, c.a, c.c))
    if ties:
        # the copied points carry +5 s and -5 s (s: signs), every other point 0 or +-1, mostly 0: one of the two pairs is the
        # maximum of most columns
        F = (rng.integers(-1, 2, size=F.shape) * (rng.random(F.shape) < 0.5)).astype(np.float32)
        s = _ints(rng, (c.b, c.a, c.c), 1) * 5
        (a0, a1), (b0, b1) = ties
        F[:, a0] = F[:, a1] = s
        F[:, b0] = F[:, b1] = -s
    if ident is not None:
        F[ident] = F[ident, :1]
    xyz = _coords(rng, c.b, c.p, ties, ident)
    d = dict(F=F, xyz=xyz, anchors=_anchors(c.a), W=_ints(rng, (c.co, c.c + 3)), bias=_ints(rng, (c.co,)) if c.bias else None,
             gout=_ints(rng, (c.b, c.a, c.co)))
    out, arg_fwd, centre = P.forward(d["F"], xyz, d["anchors"], d["W"], d["bias"])
    d["arg"] = _routing(rng, c, arg_fwd) if isinstance(c, BwdCase) else arg_fwd
    dW, dbias = P.bwd_weight(d["gout"], d["arg"], d["F"], xyz, d["anchors"], centre)
    r = dict(out=out, arg=d["arg"], arg_fwd=arg_fwd, centre=centre, dF=P.bwd_data(d["gout"], d["arg"], d["W"], c.p), dW=dW,
             dbias=dbias, Z=d["F"].astype(np.float64) @ d["W"].astype(np.float64)[:, :c.c].T)
    r["bits"] = _prove(c, d, r)
    if ties or ident is not None:
        _prove_ties(c, d, r)
    d["ref"] = r
    return d


def _prove_ties(c, d, r):
    """At least half of the columns have a tied maximum whose first point is an original and whose copy holds the same value
    (identical cloud: every column of that cloud ties over all p and its arg-max is 0)."""
    z = P.embed(d["F"], d["xyz"], d["anchors"], d["W"], d["bias"])
    top = z.max(axis=1, keepdims=True)
    if c.ident is not None:
        assert np.all(z[c.ident] == top[c.ident]) and np.all(r["arg_fwd"][c.ident] == 0), c
        return
    hit = np.zeros(r["arg_fwd"].shape, bool)
    for i, j in c.ties:
        assert np.array_equal(z[:, i], z[:, j]), c
        hit |= (r["arg_fwd"] == i) & (z[:, j] == top[:, 0])
    r["tied_fraction"] = float(hit.mean())
    assert r["tied_fraction"] >= 0.5, (c, r["tied_fraction"])


def case(c):
    if c not in _CACHE:
        _CACHE[c] = build(c)
    return _CACHE[c]


def nan_features(c, pair):
    """The case's features with a NaN at each point of the pair (first and last channel), in ONE (cloud, anchor) row:
    (F, (cloud, anchor))."""
    F = case(c)["F"].copy()
    F[0, pair[0], c.a - 1, 0] = np.nan
    F[0, pair[1], c.a - 1, c.c - 1] = np.nan
    return F, (0, c.a - 1)


def build_dz(c):
    """gout with all 24 bits in use (not representable in bf16), among them exact halves between two bf16 neighbours (ties to
    even in both directions), a random routing table; dZ in both forms."""
    rng = np.random.default_rng(hash_name(c.name))
    g = ((1.0 + rng.random((c.b, c.a, c.co))) * (1 - 2 * rng.integers(0, 2, size=(c.b, c.a, c.co)))).astype(np.float32)
    halves = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 2.0 - 2.0 ** -8, 3.0e38], np.float32)
    flat = g.reshape(-1)
    flat[:min(flat.size, halves.size)] = halves[:flat.size]
    arg = rng.integers(0, c.p, size=g.shape).astype(np.int32)
    arg.reshape(-1)[:min(flat.size, halves.size)] = np.arange(min(flat.size, halves.size)) % c.p
    assert not np.array_equal(bf16_rne(g), g)
    return dict(gout=g, arg=arg, f32=P.dz(g, arg, c.p, "f32"), bf16=P.dz(g, arg, c.p, "bf16"))


# ------------------------------------------------------------------------------------------------ real-geometry tier
# (clouds, channels, output channels, points, anchors): the MFMA forward with a partial channel chunk, the VALU forward across
# its output-channel block with 60 anchors, and the widest head
REAL_SHAPES = [(2, 80, 72, 70, 12), (1, 70, 130, 33, 60), (2, 256, 264, 40, 12)]
# |kernel - fp64| <= REAL_M 2^-24 S element by element.  REAL_M is the smallest integer that is at least twice the worst
# |fp32 - fp64| / (2^-24 S) of a CPU fp32 restatement of the forward pass and of the two fused gradients over these shapes in
# several summation orders (sequential, blocks of four, chunks of 64, coordinates first / last, random permutations;
# tests/test_pointnet_spec.py re-measures it and fails if this constant is not that): worst ratio REAL_RATIO_MEASURED, never
# taken from a kernel run, and far below the sequential-sum ceiling c + 5.
REAL_RATIO_MEASURED = 5.991     # dW of (2, 256, 264, 40, 12) under a random permutation; out 4.468, dF 3.208, dbias 2.292
REAL_M = 12


def real_case(shape):
    """Icosahedral anchors (the first `a` of the 60 rotations), a unit-ball cloud, normal features and gradients, full-mantissa W; the float64 forward result."""
    import torch
    from conftest import unit_ball_cloud
    from epn_pointcloud_amd.vgtk.so3conv import functional as L
    from gemm_ref import full_mantissa
    if ("real", shape) not in _CACHE:
        b, c, co, p, a = shape
        seed = hash_name(f"real{shape}") % 100000
        rng = np.random.default_rng(seed)
        g = torch.Generator().manual_seed(seed)
        d = dict(F=torch.randn(b, p, a, c, generator=g).numpy(), xyz=unit_ball_cloud(rng, b, p),
                 anchors=np.ascontiguousarray(np.asarray(L.get_anchors(60), dtype=np.float32)[:a]),
                 W=(full_mantissa((co, c + 3), seed + 1) / (c + 3) ** 0.5).numpy(), bias=full_mantissa((co,), seed + 2).numpy() * 0.25,
                 gout=torch.randn(b, a, co, generator=g).numpy())
        d["z64"] = P.embed(d["F"], d["xyz"], d["anchors"], d["W"], d["bias"])
        d["out64"], d["arg64"] = P.max_first(d["z64"], axis=1)
        _CACHE[("real", shape)] = d
    return _CACHE[("real", shape)]
