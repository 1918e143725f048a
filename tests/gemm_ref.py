"""What the GEMM tests judge by (tests/test_gpu_gemm_exact.py on the device, tests/test_gemm_spec.py without one): numpy
emulations of the operand splits of csrc/gemm.h (split3: three bf16 pieces; f2_split_pair: two fp16 pieces under a power-of-two
scale), the input builders (integers, selection matrices, row scales) and the poisoned buffers operands and outputs live in.
Nothing here needs the library; only the builders that are asked for a device need one."""
import numpy as np
import torch

F64 = torch.float64


# ------------------------------------------------------------------------------------------------ the splits of gemm.h
def bf16_rne(x):
    """float32 array -> the nearest bf16 (ties to even), as float32: v_cvt_pk_bf16_f32 on finite values."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def split3(x):
    """gemm.h split3: h = rne(x), m = rne(x - h), l = rne(x - h - m), every difference taken in float32."""
    x = np.asarray(x, dtype=np.float32)
    h = bf16_rne(x)
    r = (x - h).astype(np.float32)
    m = bf16_rne(r)
    return h, m, bf16_rne((r - m).astype(np.float32))


def f2_scale_of(amax):
    """gemm.h f2_scale_of: the power of two s with amax * s in [2^14, 2^15); exponents below 14 (zero, tiny) clamp."""
    e = (np.asarray(amax, dtype=np.float32).view(np.uint32) >> 23) & 255
    e = np.maximum(e, 14)
    return ((268 - e).astype(np.uint32) << 23).view(np.float32)


def f2_split(x, s):
    """gemm.h f2_split_pair on an array: (h, l) as float16 of x * s."""
    xs = (np.asarray(x, dtype=np.float32) * np.float32(s)).astype(np.float32)
    h = xs.astype(np.float16)
    return h, (xs - h.astype(np.float32)).astype(np.float32).astype(np.float16)


def f2_bound(x, amax):
    """The bound gemm.h states for the two-piece form: per element max(|x| 2^-22, max|x| 2^-39) (float64)."""
    return np.maximum(np.abs(np.asarray(x, dtype=np.float64)) * 2.0 ** -22, float(amax) * 2.0 ** -39)


# ------------------------------------------------------------------------------------------------ inputs
def ints(shape, q, seed, device=None, dtype=torch.float32):
    """Integers uniform in [-q, q] (float32 / bf16 values); row 0 is all +q and the last row alternates +-q, so that some
    output of every tile row reaches the largest sum the exactness condition allows for."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(-q, q + 1, shape, generator=g).float()
    if shape[0] > 0 and shape[1] > 0:
        t[0] = q
        t[-1] = q * (1 - 2 * (torch.arange(shape[1]) % 2)).float()
    return t.to(dtype).to(device) if device is not None else t.to(dtype)


def full_mantissa(shape, seed, device=None):
    """sign * (1 + u), u uniform in [0, 1): float32 values with all 24 bits in use and no element near zero (a power-of-two
    factor of 2^+-100 leaves every bf16 / fp16 piece of them a normal number)."""
    g = torch.Generator().manual_seed(seed)
    v = 1.0 + torch.rand(shape, generator=g)
    v = v * (1 - 2 * torch.randint(0, 2, shape, generator=g)).float()
    return v.to(device) if device is not None else v


def twelve_bit(shape, seed, device=None):
    """sign * (1 + i / 2048), i uniform in 0 .. 2047: twelve significant bits.  The product of two such values has at most 24 and
    is exact in fp32, while their three-piece split has a non-zero MIDDLE piece on both sides (h: 8 bits, m: the other 4)."""
    g = torch.Generator().manual_seed(seed)
    v = (1.0 + torch.randint(0, 2048, shape, generator=g).float() / 2048.0) * (1 - 2 * torch.randint(0, 2, shape, generator=g)).float()
    return v.to(device) if device is not None else v


def selection_rows(rows, cols, seed, device=None):
    """[rows, cols] with ONE non-zero per row, +-2^e (e in -8 .. 8) in a random column: returns (matrix, column, value)."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(0, cols, (rows,), generator=g)
    v = torch.ldexp(torch.ones(rows), torch.randint(-8, 9, (rows,), generator=g)) * (1 - 2 * torch.randint(0, 2, (rows,), generator=g))
    m = torch.zeros(rows, cols)
    m[torch.arange(rows), k] = v
    if device is not None:
        m, k, v = m.to(device), k.to(device), v.to(device)
    return m, k, v


def selection_cols(rows, cols, seed, device=None):
    """[rows, cols] with ONE non-zero per COLUMN (rows >= cols, distinct rows): the X operand of a TN product that selects.
    Returns (matrix, row of every column, value)."""
    g = torch.Generator().manual_seed(seed)
    r = torch.randperm(rows, generator=g)[:cols]
    v = torch.ldexp(torch.ones(cols), torch.randint(-8, 9, (cols,), generator=g)) * (1 - 2 * torch.randint(0, 2, (cols,), generator=g))
    m = torch.zeros(rows, cols)
    m[r, torch.arange(cols)] = v
    if device is not None:
        m, r, v = m.to(device), r.to(device), v.to(device)
    return m, r, v


def row_scales(n, device=None):
    """2^((7 n mod 41) - 20) per row n: neighbours differ by 2^7, the 41 values cover 2^-20 .. 2^20."""
    s = torch.ldexp(torch.ones(n), (7 * torch.arange(n)) % 41 - 20)
    return s.to(device) if device is not None else s


# ------------------------------------------------------------------------------------------------ poisoned buffers
SENTINEL32 = 0x7FC5A5A5     # a quiet NaN no kernel produces
SENTINEL16 = 0x7FC5


def _int_view(t):
    return t.view(torch.int32 if t.element_size() == 4 else (torch.int16 if t.element_size() == 2 else torch.uint8))


def _sentinel(t):
    return SENTINEL32 if t.element_size() == 4 else (SENTINEL16 if t.element_size() == 2 else 0xA5)


class Arena:
    """Several 2-D regions of one dtype carved out of ONE buffer filled with a sentinel bit pattern.  specs: (rows, cols, ld,
    col0, shift) per region -- leading dimension ld >= col0 + cols (guard columns on both sides when ld > cols), the region's
    rows starting `shift` elements past a 256-byte aligned address; `guard` sentinel rows of 64 elements lie before, between and
    after the regions.  `.t[i]` are the regions; check() asserts that every element outside them still holds the sentinel."""

    def __init__(self, dtype, device, specs, guard=4):
        self.specs, off, starts = [], guard * 64, []
        for rows, cols, ld, col0, shift in specs:
            ld = cols if ld is None else ld
            assert ld >= col0 + cols
            start = (off + 63) // 64 * 64 + shift
            starts.append(start)
            self.specs.append((rows, cols, ld, col0))
            off = start + rows * ld + guard * 64
        self.flat = torch.empty(off + 64, dtype=dtype, device=device)
        _int_view(self.flat).fill_(_sentinel(self.flat))
        self.bodies = [self.flat[s:s + r * ld].view(r, ld) for s, (r, c, ld, c0) in zip(starts, self.specs)]
        self.t = [b[:, c0:c0 + c] for b, (r, c, ld, c0) in zip(self.bodies, self.specs)]

    def check(self, what=""):
        regions = [_int_view(b)[:, c0:c0 + c] for b, (r, c, ld, c0) in zip(self.bodies, self.specs)]
        saved = [r.clone() for r in regions]
        for r in regions:
            r.fill_(_sentinel(self.flat))
        bad = int((_int_view(self.flat) != _sentinel(self.flat)).sum().item())
        for r, s in zip(regions, saved):
            r.copy_(s)
        assert bad == 0, f"{what}: {bad} element(s) outside the output region(s) {self.specs} were written"

    def untouched(self):
        """True when the whole buffer, regions included, still holds the sentinel (a refused call wrote nothing)."""
        return bool((_int_view(self.flat) == _sentinel(self.flat)).all().item())


def guarded(rows, cols, dtype, device, ld=None, col0=0, shift=0):
    """One region in an arena of its own: (arena, region)."""
    a = Arena(dtype, device, [(rows, cols, ld, col0, shift)])
    return a, a.t[0]


def place(t, ld=None, col0=0, shift=0):
    """A copy of the 2-D tensor t as a view with leading dimension ld (columns col0 .. col0 + cols of a wider tensor whose other
    columns hold a large finite value: reading them would show), shifted by `shift` elements from an aligned address."""
    rows, cols = t.shape
    ld = cols if ld is None else ld
    assert ld >= col0 + cols
    flat = torch.full((shift + max(rows, 1) * ld + 64,), 3.0e4, dtype=t.dtype, device=t.device)
    v = flat[shift:shift + rows * ld].view(rows, ld)[:, col0:col0 + cols]
    v.copy_(t)
    return v
