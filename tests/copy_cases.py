"""Case tables, numpy restatements and the restated launch conditions of the kernels that only move data: the casts of
csrc/gemm.hip (epn_cast, epn_cast_add_bf16, epn_transpose_cast) and the copy glue of csrc/glue.hip (epn_gather_rows,
epn_scatter_rows, epn_scatter_rows_add, epn_intra_group_*, epn_conv1x1_c1_*).  tests/test_gpu_copy_exact.py runs them on the
device, tests/test_copy_spec.py proves what is here without one.  Nothing here needs a device or the library.

Why `==` is legitimate: every one of these is a copy, ONE rounding (fp32 -> bf16, ties to even), one fp32 multiply, or a short
sum whose order the header promises (ascending rows, from the first occurrence).  bf16 data lives here as uint16 bit patterns,
raw rows as uint32 words, and results are compared as bits.  The one comparison that is not `==` is the weight gradient of the
single-channel convolution on real-valued data (C1_REAL below)."""
from collections import namedtuple

import numpy as np

from conv_cases import hash_name, normalise as _normalise
from gemm_ref import bf16_rne, full_mantissa

EPN_EINVAL, EPN_EWORKSPACE, EPN_ENULL = -1, -2, -3
F32, U16, U32 = np.float32, np.uint16, np.uint32
_CACHE = {}


# Two instances of cast_kernel the C++ runtime demangles WRONGLY (it reads the bf16 type DF16b followed by `f` or `Lb1E` as a
# fixed-point type); no other kernel of the library has these texts.
_MISREAD = {"cast_kernel<bool_Accum,false>": "cast_kernel<__bf16,float,false>",
            "cast_kernel<float,bool_Accum,bool,E>": "cast_kernel<float,__bf16,true>"}


def normalise(name):
    """conv_cases.normalise, the demangler's spelling of the 16-byte element type as the source's, and _MISREAD."""
    name = _normalise(name).replace("float__vector(4)", "f32x4").replace("Dv4_f", "f32x4")
    return _MISREAD.get(name, name)


def _rng(name):
    return np.random.default_rng(hash_name(name))


# ------------------------------------------------------------------------------------------------ conversions
def to_bf16_bits(x):
    """float32 -> bf16 bit patterns (uint16): gemm_ref.bf16_rne (ties to even; overflow to inf), NaN stays a NaN."""
    x = np.ascontiguousarray(x, dtype=F32)
    bits = (bf16_rne(x).view(U32) >> 16).astype(U16)
    return np.where(np.isnan(x), U16(0x7FC0), bits).astype(U16).reshape(x.shape)


def from_bf16_bits(bits):
    """bf16 bit patterns -> float32: bits << 16."""
    bits = np.ascontiguousarray(bits, dtype=U16)
    return (bits.astype(U32) << 16).view(F32).reshape(bits.shape)


def cast_add(src, add_bits):
    """epn_cast_add_bf16: bf16(src + float(add)) -- one fp32 add, one rounding."""
    return to_bf16_bits((np.asarray(src, F32) + from_bf16_bits(add_bits)).astype(F32))


def same_bits(got, want, nan_as_nan=False):
    """Bit equality of two arrays of one integer / float type; nan_as_nan: any NaN equals any NaN (payloads are not pinned)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return False
    if got.dtype == U16 and nan_as_nan:
        gn, wn = np.isnan(from_bf16_bits(got)), np.isnan(from_bf16_bits(want))
        return bool(np.all((got == want) | (gn & wn)) and np.array_equal(gn, wn))
    if got.dtype == F32:
        if nan_as_nan:
            gn, wn = np.isnan(got), np.isnan(want)
            return bool(np.all((got.view(U32) == want.view(U32)) | (gn & wn)) and np.array_equal(gn, wn))
        return bool(np.array_equal(got.view(U32), want.view(U32)))
    return bool(np.array_equal(got, want))


# ------------------------------------------------------------------------------------------------ cast: launcher + cases
CAST_GRID_MAX, CAST_BLOCK = 8192, 256
N_LADDER = (1, 3, 4, 5, 1023, 1024, 1027)
N_VECTOR_WRAP = CAST_GRID_MAX * CAST_BLOCK * 4 + 7      # second trip of the four-wide loop, n % 4 == 3
N_SCALAR_WRAP = CAST_GRID_MAX * CAST_BLOCK + 5          # second trip of the scalar kernel's loop
assert N_VECTOR_WRAP % 4 == 3

_TYPE = {"f32": "float", "bf16": "__bf16"}


def cast_launch(n, src, dst, src_shift=0, dst_shift=0, null=False):
    """launch_cast restated: (return code, kernel name or "").  src / dst: "f32" | "bf16"; shifts in elements from a 16-byte
    aligned address."""
    if n == 0:
        return 0, ""
    if null:
        return EPN_ENULL, ""
    if src == dst:
        return EPN_EINVAL, ""
    size = {"f32": 4, "bf16": 2}
    aligned = (src_shift * size[src]) % 16 == 0 and (dst_shift * size[dst]) % 16 == 0
    if aligned:
        return 0, f"cast_kernel<{_TYPE[src]},{_TYPE[dst]},false>"
    return 0, f"cast_scalar_kernel<{_TYPE[src]},{_TYPE[dst]}>"


def cast_trips(n, aligned):
    """How often the kernel's main loop runs for its busiest thread (grid capped at CAST_GRID_MAX blocks)."""
    work = (n + 3) // 4 if aligned else n
    grid = min((work + CAST_BLOCK - 1) // CAST_BLOCK, CAST_GRID_MAX)
    per = n // 4 if aligned else n
    return -(-per // (grid * CAST_BLOCK)) if grid else 0


def cast_add_launch(n, shifts=(0, 0, 0), null=False):
    """launch_cast_add restated; shifts: elements of (src f32, add bf16, dst bf16)."""
    if n == 0:
        return 0, ""
    if null:
        return EPN_ENULL, ""
    if (shifts[0] * 4) % 16 or (shifts[1] * 2) % 16 or (shifts[2] * 2) % 16:
        return EPN_EINVAL, ""
    return 0, "cast_kernel<float,__bf16,true>"


def transpose_launch(rows, cols, src, dst):
    if rows < 1 or cols < 1:
        return EPN_EINVAL, ""
    return 0, f"transpose_cast_kernel<{_TYPE[src]},{_TYPE[dst]}>"


CastCase = namedtuple("CastCase", "name n src dst src_shift dst_shift null", defaults=(0, 0, False))
_DIRS = (("f32", "bf16"), ("bf16", "f32"))
CAST_CASES = (
    [CastCase(f"{s}_{d}_n{n}", n, s, d) for s, d in _DIRS for n in N_LADDER + (N_VECTOR_WRAP,)]
    + [CastCase(f"{s}_{d}_n{n}_src+1", n, s, d, 1, 0) for s, d in _DIRS for n in N_LADDER]
    + [CastCase(f"{s}_{d}_n{n}_dst+1", n, s, d, 0, 1) for s, d in _DIRS for n in (1, 5, 1027)]
    + [CastCase(f"{s}_{d}_scalar_wrap", N_SCALAR_WRAP, s, d, 1, 0) for s, d in _DIRS]
)
CAST_REFUSALS = (
    [CastCase("n0_null", 0, "f32", "bf16", null=True), CastCase("n0_null_same", 0, "f32", "f32", null=True)]
    + [CastCase(f"same_{s}", 5, s, s) for s in ("f32", "bf16")]
    + [CastCase(f"null_{s}_{d}", 5, s, d, null=True) for s, d in _DIRS]
)

# fp32 bit patterns whose rounding to bf16 is an edge (name -> (fp32 bits, bf16 bits)): the expected bits are written out by hand
# here and tests/test_copy_spec.py holds to_bf16_bits and torch to them
SPECIAL_F32 = {
    "tie_above_even": (0x3F808000, 0x3F80),         # 1 + 2^-8: halfway between 0x3F80 (even) and 0x3F81 -> down
    "tie_above_odd": (0x3F818000, 0x3F82),          # halfway between 0x3F81 (odd) and 0x3F82 -> up
    "below_tie_even": (0x3F807FFF, 0x3F80),
    "above_tie_even": (0x3F808001, 0x3F81),
    "below_tie_odd": (0x3F817FFF, 0x3F81),
    "above_tie_odd": (0x3F818001, 0x3F82),
    "neg_tie_above_even": (0xBF808000, 0xBF80),
    "neg_tie_above_odd": (0xBF818000, 0xBF82),
    "max_finite_bf16": (0x7F7F0000, 0x7F7F),
    "largest_that_stays_finite": (0x7F7F7FFF, 0x7F7F),
    "smallest_that_overflows": (0x7F7F8000, 0x7F80),    # the tie above the odd 0x7F7F rounds up to +inf
    "flt_max": (0x7F7FFFFF, 0x7F80),
    "neg_largest_that_stays_finite": (0xFF7F7FFF, 0xFF7F),
    "neg_smallest_that_overflows": (0xFF7F8000, 0xFF80),
    "pos_zero": (0x00000000, 0x0000),
    "neg_zero": (0x80000000, 0x8000),
    "min_subnormal_f32": (0x00000001, 0x0000),
    "neg_min_subnormal_f32": (0x80000001, 0x8000),
    "subnormal_tie_to_zero": (0x00008000, 0x0000),      # halfway between 0 (even) and the smallest bf16 subnormal
    "subnormal_above_tie": (0x00008001, 0x0001),
    "subnormal_exact": (0x00010000, 0x0001),
    "subnormal_tie_above_odd": (0x00018000, 0x0002),
    "largest_subnormal_f32": (0x007FFFFF, 0x0080),      # rounds up into the smallest normal
    "min_normal": (0x00800000, 0x0080),
    "pos_inf": (0x7F800000, 0x7F80),
    "neg_inf": (0xFF800000, 0xFF80),
    "quiet_nan": (0x7FC00000, 0x7FC0),
    "nan_payload_low_bits": (0x7F800001, 0x7FC0),       # a NaN whose payload lies in the dropped half: must not become inf
    "neg_nan": (0xFFC12345, 0xFFC1),
}


def special_f32(rot=0):
    """(float32 inputs, expected bf16 bits) of SPECIAL_F32: every value four times in a row (the vector body) and three more at the
    end (the scalar tail; which three turns with `rot`, SPECIAL_ROTATIONS puts every value there once)."""
    bits = np.array([v[0] for v in SPECIAL_F32.values()], U32)
    want = np.array([v[1] for v in SPECIAL_F32.values()], U16)
    order = np.roll(np.arange(bits.size), -rot)
    order = np.concatenate([np.repeat(order, 4), order[:3]])
    return bits[order].view(F32), want[order]


SPECIAL_ROTATIONS = tuple(range(0, len(SPECIAL_F32), 3))


def all_bf16():
    """All 65536 bf16 bit patterns and one more (a scalar tail)."""
    return np.concatenate([np.arange(65536, dtype=np.uint32).astype(U16), np.array([0x3F81], U16)])


def cast_data(c):
    """(source array, expected result) of a CastCase: float32 / uint16 bit arrays."""
    rng = _rng("cast" + c.name)
    if c.src == "f32":
        src = full_mantissa((c.n,), int(rng.integers(1 << 30))).numpy() * np.ldexp(F32(1), rng.integers(-20, 21, size=c.n)).astype(F32)
        return src, to_bf16_bits(src)
    src = rng.integers(0, 0x7F80, size=c.n).astype(U16) | (rng.integers(0, 2, size=c.n).astype(U16) << 15)     # finite
    return src, from_bf16_bits(src)


def cast_add_data(n, seed=0):
    """src fp32, add bf16 bits, built so that one rounding of the fp32 sum differs from bf16(src) + add and from a sum rounded
    to bf16 per step: the first elements are hand-made, the rest full-mantissa values around them."""
    rng = _rng(f"cast_add{n}_{seed}")
    src = full_mantissa((n,), int(rng.integers(1 << 30))).numpy()
    add = to_bf16_bits(full_mantissa((n,), int(rng.integers(1 << 30))).numpy() * F32(0.125))
    # just below a tie, pushed over it by the addend (bf16(src) + add stays below); just above one, pulled back under it
    hand_src = np.array([1 + 2.0 ** -8 - 2.0 ** -20, 1 + 2.0 ** -8 + 2.0 ** -20, -(1 + 2.0 ** -8 - 2.0 ** -20)], F32)
    hand_add = to_bf16_bits(np.array([2.0 ** -10, -2.0 ** -10, -2.0 ** -10], F32))
    k = min(n, 3)
    src[:k], add[:k] = hand_src[:k], hand_add[:k]
    return src, add, cast_add(src, add)


def cast_add_mutants(src, add):
    """Wrong forms of cast_add a loose test would let through: bf16(src) + add rounded again; the addend dropped."""
    double = to_bf16_bits((from_bf16_bits(to_bf16_bits(src)) + from_bf16_bits(add)).astype(F32))
    return dict(double_rounded=double, addend_dropped=to_bf16_bits(src))


def drop_tail(want, fill):
    """The mutant that loses the n % 4 elements after the four-wide body."""
    out = np.array(want, copy=True)
    n = out.size
    if n % 4:
        out[n - n % 4:] = fill
    return out


CAST_ADD_SHIFTS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 4, 0), (0, 0, 4), (2, 0, 0))      # each pointer misaligned in turn

TRANSPOSE_SHAPES = ((1, 1), (1, 33), (33, 1), (31, 32), (32, 32), (33, 65), (64, 24), (100, 7))
TRANSPOSE_PAIRS = (("f32", "f32"), ("f32", "bf16"), ("bf16", "f32"), ("bf16", "bf16"))
TRANSPOSE_REFUSALS = ((0, 5), (5, 0), (0, 0), (-1, 4))


def transpose_data(rows, cols, src, dst):
    """(source [rows, cols], expected [cols, rows]) in the bit representation of each side."""
    rng = _rng(f"tr{rows}x{cols}{src}{dst}")
    v = full_mantissa((rows, cols), int(rng.integers(1 << 30))).numpy() * np.ldexp(F32(1), rng.integers(-9, 10, size=(rows, cols))).astype(F32)
    s = v if src == "f32" else to_bf16_bits(v)
    wide = s if src == "f32" else from_bf16_bits(s)
    want = np.ascontiguousarray(wide.T)
    return s, (want if dst == "f32" else to_bf16_bits(want))


# ------------------------------------------------------------------------------------------------ row gather / scatter
ROWS_P2_MAX = 8192
FILL_WORD = 0x3F3F3F3F          # what a destination row holds before the gather (out-of-range indices leave it)


def rows_launch(entry, b, p1, p2, row_bytes, bf16=False):
    """The three entries' argument checks restated: (return code, kernel name or "" when nothing is launched)."""
    if b < 0 or p1 < 1 or p2 < 0 or row_bytes < 16 or row_bytes % 16:
        return EPN_EINVAL, ""
    if entry == "scatter_add" and p2 > ROWS_P2_MAX:
        return EPN_EINVAL, ""
    if b * p2 == 0:
        return 0, ""
    if entry == "scatter_add":
        return 0, f"rows_scatter_add_kernel<{'true' if bf16 else 'false'}>"
    return 0, "rows_gather_kernel"


def gather_rows(src, idx, fill=None):
    """src [b][p1][e], idx [b][p2] -> [b][p2][e]; a row whose index is out of range keeps `fill`."""
    b, p1, e = src.shape
    out = np.empty((b, idx.shape[1], e), src.dtype)
    out[...] = 0 if fill is None else fill
    for bb in range(b):
        for p in range(idx.shape[1]):
            q = int(idx[bb, p])
            if 0 <= q < p1:
                out[bb, p] = src[bb, q]
    return out


def scatter_rows(g, idx, p1):
    """Plain transpose (distinct indices): g [b][p2][e] -> [b][p1][e], rows not indexed zero, out-of-range skipped."""
    b, p2, e = g.shape
    out = np.zeros((b, p1, e), g.dtype)
    for bb in range(b):
        for p in range(p2):
            q = int(idx[bb, p])
            if 0 <= q < p1:
                out[bb, q] = g[bb, p]
    return out


def scatter_rows_add(g, idx, p1, bf16=False, order="ascending", per_step=False, lose_at=None):
    """The accumulating transpose.  g: float32 [b][p2][e], or bf16 bits (uint16) with bf16=True.  An index that occurs several
    times receives the sequential fp32 sum of its rows in ascending row order starting from the first occurrence; bf16 rows are
    widened, summed in fp32 and rounded ONCE.  The keyword arguments build the mutants: order="descending" | "float64",
    per_step (bf16: round after every add), lose_at (a later occurrence at this row position is not added)."""
    wide = from_bf16_bits(g) if bf16 else np.asarray(g, F32)
    b, p2, e = wide.shape
    out = np.zeros((b, p1, e), F32)
    for bb in range(b):
        done = set()
        for p in range(p2):
            q = int(idx[bb, p])
            if q < 0 or q >= p1 or q in done:
                continue
            done.add(q)
            rows = [int(k) for k in np.flatnonzero(idx[bb] == q)]
            if lose_at is not None:
                rows = rows[:1] + [k for k in rows[1:] if k != lose_at]
            if order == "float64":
                out[bb, q] = wide[bb, rows].astype(np.float64).sum(axis=0).astype(F32)
                continue
            if order == "descending":
                rows = rows[::-1]
            acc = wide[bb, rows[0]].copy()
            for k in rows[1:]:
                acc = (acc + wide[bb, k]).astype(F32)
                if per_step and bf16:
                    acc = bf16_rne(acc)
            out[bb, q] = acc
    return to_bf16_bits(out) if bf16 else out


# ---- index patterns: f(rng, cloud, p1, p2) -> int32[p2]
def _distinct(rng, p1, p2):
    """A random selection without repeats; positions beyond p1 hold the out-of-range values -1 and p1 in turn."""
    idx = np.where(np.arange(p2) % 2 == 0, -1, p1).astype(np.int32)
    m = min(p1, p2)
    idx[rng.permutation(p2)[:m]] = rng.permutation(p1)[:m]
    return idx


def _pat_none(rng, cloud, p1, p2):
    return _distinct(rng, p1, p2)


def _pat_fps_pad(rng, cloud, p1, p2):
    """FPS on a cloud with few live points: index 0 first, some distinct points, then index 0 to the end."""
    live = max(1, min(p1, p2 // (2 + cloud)))
    idx = np.zeros(p2, np.int32)
    idx[:live] = np.concatenate([[0], 1 + rng.permutation(p1 - 1)])[:live]
    return idx


def _pat_positions(rng, cloud, p1, p2):
    """ONE index at the row positions 0, 255, 256 and 300 (cloud 1: 1, 256, 257; others: none), distinct elsewhere."""
    at = [(0, 255, 256, 300), (1, 256, 257)][cloud] if cloud < 2 else ()
    at = [k for k in at if k < p2]
    q = int(rng.integers(p1))
    rest = [v for v in rng.permutation(p1) if v != q]
    idx = np.full(p2, -1, np.int32)
    free = [k for k in range(p2) if k not in at]
    idx[free[:len(rest)]] = rest[:len(free)]
    idx[at] = q
    return idx


def _pat_all_equal(rng, cloud, p1, p2):
    return np.full(p2, (p1 - 1 - cloud) % p1, np.int32)


def _pat_two_clusters(rng, cloud, p1, p2):
    """Two indices in turn over the first rows (cloud 0: from row 0; cloud 1: from row 1), distinct values after them and -1 where
    those run out."""
    if p1 < 2:
        return _distinct(rng, p1, p2)
    perm = rng.permutation(p1)
    q, keep = perm[:2], perm[2:]
    start, n = cloud % 2, min(p2, 7 + 2 * cloud)
    idx = np.full(p2, -1, np.int32)
    idx[start:n] = q[np.arange(max(n - start, 0)) % 2]
    free = [k for k in range(p2) if not start <= k < n]
    m = min(len(free), len(keep))
    idx[free[:m]] = keep[:m]
    return idx


def _pat_boundary(rng, cloud, p1, p2):
    """The last row of cloud 0 and the first row of cloud 1 name the same index, which occurs once in each: a scan that ran
    across the cloud boundary would take them for one repeat.  (_pat_boundary_absent is the variant without cloud 1's row.)"""
    q = p1 // 2
    rest = np.array([v for v in rng.permutation(p1) if v != q] + [-1] * p2, np.int32)[:p2]
    idx = rest.copy()
    if cloud == 0:
        idx[p2 - 1] = q
    elif cloud == 1:
        idx[0] = q
    return idx


def _pat_boundary_absent(rng, cloud, p1, p2):
    """The issue's own wording of the boundary case: an index whose only occurrence in cloud 0 is its LAST row and which does not
    occur in cloud 1 at all (nor in any later cloud) -- that row of every other cloud's target stays zero."""
    q = p1 // 2
    idx = np.array([v for v in rng.permutation(p1) if v != q] + [-1] * p2, np.int32)[:p2]
    if cloud == 0:
        idx[p2 - 1] = q
    return idx


PATTERNS = dict(none=_pat_none, fps_pad=_pat_fps_pad, positions=_pat_positions, all_equal=_pat_all_equal,
                two_clusters=_pat_two_clusters, boundary=_pat_boundary, boundary_absent=_pat_boundary_absent)

# name, clouds, source rows, gathered rows, bytes per row, index pattern, out-of-range values mixed in
RowsCase = namedtuple("RowsCase", "name b p1 p2 row_bytes pattern oob", defaults=("none", False))
_RB = dict(b=3, p1=7, p2=9)
ROWS_CASES = (
    [RowsCase(f"rb{v}_{pat}", **_RB, row_bytes=v, pattern=pat) for v in (16, 48, 16 * 255, 16 * 256, 16 * 257, 15360)
     for pat in ("none", "fps_pad")]
    + [RowsCase(f"p2_{v}_{pat}", 3, 300, v, 16, pat) for v in (0, 1, 255, 256, 257) for pat in ("none", "fps_pad", "all_equal")]
    + [RowsCase(f"p2_8192_{pat}", 1, 300, 8192, 16, pat) for pat in ("none", "fps_pad", "all_equal")]
    + [RowsCase("p2_8192_distinct", 1, 8192, 8192, 16, "none")]
    + [RowsCase(f"p1_{v}_{pat}", b, v, 9, 48, pat) for v in (1, 7, 300) for b, pat in ((1, "none"), (3, "all_equal"), (3, "fps_pad"))]
    + [RowsCase(f"positions_b{b}", b, 300, 301, 32, "positions") for b in (1, 3)]
    + [RowsCase("positions_oob", 3, 300, 301, 16, "positions", True)]
    + [RowsCase(f"clusters_rb{v}", 3, 7, 12, v, "two_clusters") for v in (16, 16 * 257)]
    + [RowsCase("clusters_oob", 3, 7, 12, 48, "two_clusters", True), RowsCase("fps_pad_oob", 3, 300, 257, 16, "fps_pad", True),
       RowsCase("all_equal_oob", 1, 7, 257, 16, "all_equal", True)]
    + [RowsCase(f"boundary_p2_{v}", 3, 300, v, 48, "boundary") for v in (2, 256, 257)]
    + [RowsCase(f"boundary_absent_p2_{v}", 3, 300, v, 48, "boundary_absent") for v in (2, 256, 257)]
    + [RowsCase("real_row_fps_pad", 3, 7, 12, 15360, "fps_pad", True)]
)
# gather and the plain scatter have no limit on p2
ROWS_CASES_BEYOND = [RowsCase("p2_8193", 1, 300, 8193, 16, "none")]
# (entry or None for all three, b, p1, p2, row_bytes)
ROWS_REFUSALS = [(None, 2, 7, 5, 8), (None, 2, 7, 5, 24), (None, 2, 7, 5, 0), (None, 2, 0, 5, 16), ("scatter_add", 1, 300, 8193, 16)]


def rows_index(c):
    if ("idx", c) not in _CACHE:
        rng = _rng("idx" + c.name)
        idx = np.stack([PATTERNS[c.pattern](rng, bb, c.p1, c.p2) for bb in range(c.b)]).astype(np.int32).reshape(c.b, c.p2)
        if c.oob and c.p2 >= 4:
            for bb in range(c.b):
                at = rng.permutation(np.arange(1, c.p2))[:4]            # (row 0 stays: the patterns' first occurrence)
                idx[bb, at] = np.array([-1, c.p1, -1, c.p1 + 5], np.int32)
        _CACHE[("idx", c)] = idx
    return _CACHE[("idx", c)]


def is_distinct(idx, p1):
    """No in-range index twice in a cloud: what the plain scatter requires."""
    return all(len(set(v)) == len(v) for v in ([int(q) for q in row if 0 <= q < p1] for row in idx))


def max_repeat(idx, p1):
    return max([int(np.bincount(row[(row >= 0) & (row < p1)], minlength=1).max()) for row in idx if row.size] + [0])


def rows_words(c, rows):
    """Raw rows of any element type: random 32-bit words [b][rows][row_bytes / 4] (uint32)."""
    return _rng("words" + c.name).integers(0, 1 << 32, size=(c.b, rows, c.row_bytes // 4), dtype=np.uint64).astype(U32)


def rows_grad(c, tier):
    """The gathered-side gradient [b][p2][elements] of the accumulating scatter: float32, or bf16 bits for the bf16 tiers.
    exact / exact_bf16: integers in [-3, 3] (any order gives the same sum; 8192 x 3 < 2^24).
    order: full-mantissa floats under per-row powers of two -- ascending, descending and float64 sums differ.
    round_bf16: full 8-bit bf16 mantissas under per-row powers of two -- one rounding differs from one per add."""
    rng = _rng(f"grad{tier}" + c.name)
    bf = tier.endswith("bf16")
    shape = (c.b, c.p2, c.row_bytes // (2 if bf else 4))
    if tier.startswith("exact"):
        v = rng.integers(-3, 4, size=shape).astype(F32)
    else:
        v = full_mantissa(shape, int(rng.integers(1 << 30))).numpy() * np.ldexp(F32(1), rng.integers(-3, 4, size=(c.b, c.p2, 1))).astype(F32)
    return to_bf16_bits(v) if bf else v


TIERS = ("exact", "exact_bf16", "order", "round_bf16")


def rows_add_case(c, tier):
    """(gradient, indices, expected result) of one accumulating-scatter case, computed once."""
    if (c, tier) not in _CACHE:
        g, idx = rows_grad(c, tier), rows_index(c)
        _CACHE[(c, tier)] = (g, idx, scatter_rows_add(g, idx, c.p1, tier.endswith("bf16")))
    return _CACHE[(c, tier)]


def tiers_of(c):
    """Every case runs the exact tiers; cases with an index that occurs three times or more also the order tiers (at p2 = 8192 the
    two patterns with one long repeat: the restatement's cost grows with the number of distinct indices)."""
    return TIERS if max_repeat(rows_index(c), c.p1) >= 3 and (c.p2 <= 512 or c.pattern in ("all_equal", "fps_pad")) else TIERS[:2]


# ------------------------------------------------------------------------------------------------ intra grouping
IntraCase = namedtuple("IntraCase", "name c na kn p table bf16 b", defaults=(False, 2))
_NAKN = ((1, 1), (12, 5), (60, 12))
_TABLES = ("identity", "permutation", "repeats")


def _intra_cases(cs, bf16):
    out = []
    for i, c in enumerate(cs):
        for j, (na, kn) in enumerate(_NAKN):
            for p in (1, 3):
                t = _TABLES[(i + j + p) % 3]
                out.append(IntraCase(f"{'bf16' if bf16 else 'f32'}_c{c}_na{na}_kn{kn}_p{p}_{t}", c, na, kn, p, t, bf16))
    return out


INTRA_CASES = _intra_cases((1, 3, 4, 5, 8, 64), False) + _intra_cases((8, 16, 64), True)
INTRA_REFUSALS = [IntraCase(f"bf16_c{c}", c, 12, 5, 3, "identity", True) for c in (4, 12)] \
    + [IntraCase("f32_c0", 0, 12, 5, 3, "identity"), IntraCase("f32_na0", 4, 0, 5, 3, "identity"),
       IntraCase("f32_kn0", 4, 12, 0, 3, "identity")]


def intra_launch(c):
    if c.bf16 and (c.c < 8 or c.c % 8):
        return EPN_EINVAL, ""
    ch = c.c // 2 if c.bf16 else c.c           # the bf16 entry hands pairs of channels to the fp32 one
    if c.b < 0 or c.p < 0 or c.na < 1 or c.kn < 1 or ch < 1:
        return EPN_EINVAL, ""
    if c.b == 0 or c.p == 0:
        return 0, ""
    return 0, "intra_group_kernel<f32x4>" if ch % 4 == 0 else "intra_group_kernel<float>"


def intra_table(c):
    rng = _rng("table" + c.name)
    if c.table == "identity":
        return np.repeat(np.arange(c.na, dtype=np.int32)[:, None], c.kn, axis=1)
    if c.table == "permutation":
        return np.stack([rng.permutation(c.na) for _ in range(c.kn)], axis=1).astype(np.int32)
    return rng.integers(0, c.na, size=(c.na, c.kn)).astype(np.int32)


def intra_group(feats, table):
    """feats [b][p][na][c], table [na][kn] -> [b*p*na][kn*c]: feats[b, p, table[a, k], :]."""
    b, p, na, c = feats.shape
    out = np.empty((b * p * na, table.shape[1] * c), feats.dtype)
    for bb in range(b):
        for pp in range(p):
            for a in range(na):
                for k in range(table.shape[1]):
                    out[(bb * p + pp) * na + a, k * c:(k + 1) * c] = feats[bb, pp, table[a, k]]
    return out


def intra_feats(c):
    """Random bits: uint32 words (fp32 channels) or uint16 (bf16 channels)."""
    rng = _rng("feats" + c.name)
    if c.bf16:
        return rng.integers(0, 1 << 16, size=(c.b, c.p, c.na, c.c)).astype(U16)
    return rng.integers(0, 1 << 32, size=(c.b, c.p, c.na, c.c), dtype=np.uint64).astype(U32)


# ------------------------------------------------------------------------------------------------ conv1x1, one input channel
C1_COUT = (4, 8, 64, 512, 1024)
C1_COUT_REFUSED = (0, 2, 6, 1028)
C1_COUT_FWD_ONLY = (12, 20, 24)
C1_ROWS = (0, 1, 63, 64, 65, 1000, 65535, 65536, 65537)
# (rows, cout): the rows ladder at a narrow width, the width ladder at few rows
C1_SHAPES = [(r, 8) for r in C1_ROWS] + [(r, c) for c in (4, 64, 512, 1024) for r in (0, 65, 1000)] + [(65537, 4)]


def c1_accepts(entry, cout):
    """The argument check of the three entries on cout ("fwd" | "bwd" | "bwd_ws")."""
    ok = cout >= 4 and cout % 4 == 0 and cout <= 1024
    return ok if entry == "fwd" else ok and 256 % (cout // 4) == 0


def c1_plan(rows, cout):
    """The launchers' split of the weight gradient: (rows per block, row lanes of a block, blocks)."""
    blocks = (rows + 63) // 64 if rows < 1024 * 64 else 1024
    rpb = -(-rows // blocks)
    return rpb, 256 // (cout // 4), -(-rows // rpb)


def c1_workspace_bytes(rows, cout):
    return c1_plan(rows, cout)[2] * cout * 4


def c1_launch(entry, rows, cout, workspace="ok"):
    """(return code, kernel name); workspace: "ok" | "short" | "misaligned" | "null" (the ws form only)."""
    if rows < 0 or not c1_accepts(entry, cout):
        return EPN_EINVAL, ""
    if rows == 0:
        return 0, ""
    if entry == "fwd":
        return 0, "c1_outer_kernel"
    if entry == "bwd_ws" and workspace != "ok":
        return EPN_EWORKSPACE, ""
    return 0, f"c1_outer_bwd_kernel<{'true' if entry == 'bwd_ws' else 'false'}>"


def c1_chain(rows, cout):
    """L: the longest chain of roundings behind one element of the weight gradient -- a row lane's sequential sum
    (ceil(rpb / rstep) terms), the block's sum over its rstep lanes, the sum over the nb blocks (in block order, or by atomics in
    any order), and one for the products."""
    rpb, rstep, nb = c1_plan(rows, cout)
    return -(-rpb // rstep) + rstep + nb + 1


def c1_forward(x, w):
    return (np.asarray(x, F32)[:, None] * np.asarray(w, F32)[None, :]).astype(F32)


def c1_grad64(x, dy):
    return (np.asarray(x, np.float64)[:, None] * np.asarray(dy, np.float64)).sum(axis=0)


def c1_grad_fp32(x, dy, drop=None):
    """The kernels' order in fp32 on the CPU (products rounded on their own): lane rl of block blk sums rows r0 + rl, r0 + rl +
    rstep, ...; the block adds its lanes in lane order, the blocks are added in block order.  drop = (block, row of the block):
    that row is left out (the mutant)."""
    x, dy = np.asarray(x, F32), np.asarray(dy, F32)
    rows, cout = dy.shape
    rpb, rstep, nb = c1_plan(rows, cout)
    steps = -(-rpb // rstep)
    xp = np.zeros(nb * steps * rstep, F32)
    dp = np.zeros((nb * steps * rstep, cout), F32)
    live = np.zeros(nb * steps * rstep, bool)
    r = np.arange(rows)
    pos = (r // rpb) * steps * rstep + r % rpb
    xp[pos], dp[pos], live[pos] = x, dy, True
    if drop is not None:
        live[drop[0] * steps * rstep + drop[1]] = False
    prod = np.where(live[:, None], (xp[:, None] * dp).astype(F32), F32(0)).reshape(nb, steps, rstep, cout)
    lane = np.zeros((nb, rstep, cout), F32)
    for s in range(steps):
        lane = (lane + prod[:, s]).astype(F32)
    blk = lane[:, 0].copy()
    for t in range(1, rstep):
        blk = (blk + lane[:, t]).astype(F32)
    out = np.zeros(cout, F32)
    for b in range(nb):
        out = (out + blk[b]).astype(F32)
    return out


def c1_ints(rows, cout):
    """Integers in [-3, 3]: every sum stays below 65537 x 9 < 2^24, so any order gives the float64 sum."""
    rng = _rng(f"c1int{rows}x{cout}")
    return (rng.integers(-3, 4, size=rows).astype(F32), rng.integers(-3, 4, size=cout).astype(F32),
            rng.integers(-3, 4, size=(rows, cout)).astype(F32))


# the real-valued tier of the weight gradient: |got - fp64| <= L 2^-24 sum|x dy| per column, L = c1_chain(rows, cout)
C1_REAL = ((1000, 64), (65, 1024), (1000, 8), (65537, 8))
C1_REAL_L = {(1000, 64): 37, (65, 1024): 37, (1000, 8): 146, (65537, 8): 1139}
# worst |fp32 restatement - fp64| / (L 2^-24 sum|x dy|) over C1_REAL on the CPU (tests/test_copy_spec.py re-measures it and
# holds it below this): the slack the bound leaves
C1_REAL_CPU_RATIO_MAX = 0.1        # measured: 0.0166, 0.0795, 0.0068, 0.0002 in the order of C1_REAL


def c1_real(rows, cout):
    """x = 1 + u / 64 (u uniform in [0, 1): an occupancy-like feature with every mantissa bit in use), dy normal with every 97th row 64 times larger and the column means removed (near-cancelling columns, as
    behind a normalisation); float64 gradient and the per-column sum of absolute terms."""
    if ("c1real", rows, cout) not in _CACHE:
        rng = _rng(f"c1real{rows}x{cout}")
        x = (1.0 + (np.abs(full_mantissa((rows,), int(rng.integers(1 << 30))).numpy().astype(np.float64)) - 1.0) / 64.0).astype(F32)
        dy = rng.standard_normal((rows, cout))
        dy[::97] *= 64.0
        dy = (dy - dy.mean(axis=0, keepdims=True)).astype(F32)
        S = (np.abs(x.astype(np.float64))[:, None] * np.abs(dy.astype(np.float64))).sum(axis=0)
        _CACHE[("c1real", rows, cout)] = dict(x=x, dy=dy, g64=c1_grad64(x, dy), S=S, L=c1_chain(rows, cout))
    return _CACHE[("c1real", rows, cout)]


def c1_ratio(got, d):
    """max over columns of |got - fp64| / (L 2^-24 sum|x dy|)."""
    return float((np.abs(np.asarray(got, np.float64) - d["g64"]) / (d["L"] * 2.0 ** -24 * d["S"])).max())


# ------------------------------------------------------------------------------------------------ every kernel named above
REACHABLE_COPY = (
    {f"cast_kernel<{_TYPE[s]},{_TYPE[d]},false>" for s, d in _DIRS} | {f"cast_scalar_kernel<{_TYPE[s]},{_TYPE[d]}>" for s, d in _DIRS}
    | {"cast_kernel<float,__bf16,true>"} | {f"transpose_cast_kernel<{_TYPE[s]},{_TYPE[d]}>" for s, d in TRANSPOSE_PAIRS}
    | {"rows_gather_kernel", "rows_scatter_add_kernel<true>", "rows_scatter_add_kernel<false>", "intra_group_kernel<f32x4>",
       "intra_group_kernel<float>", "c1_outer_kernel", "c1_outer_bwd_kernel<true>", "c1_outer_bwd_kernel<false>"}
)


def conv1x1_c1_condition():
    """ops.conv1x1's own condition for the outer-product kernels at cin = 1: the predicate its branch calls."""
    from epn_pointcloud_amd import ops
    return ops.conv1x1_c1_takes
