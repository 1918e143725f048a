"""Case tables of the exact tests of the cloud-resident grouping transpose (csrc/inter_ungroup_cloud.hip behind
epn_inter_ungroup_cloud_{f32,bf16}): tests/test_gpu_ungroup_cloud_exact.py on the device, tests/test_cloud_spec.py without one.
A restatement of the launcher's choice (inter_ungroup_cloud_ok, uc_channels_per_wg, the instance table), the cases, and the
builders with the proofs that make `==` legitimate.  Geometry, index tables, bf16 rounding and seeds are those of
tests/conv_cases.py; the float64 reference is tests/conv_ref.py's inter_ungroup (the plain sum over valid slots).

Why `==` is legitimate.  The kernel's contract is "every contribution rounded once to the unit, the sum exact, one rounding to
the output type".  With the dyadic geometry of conv_cases.build_group every weight is a multiple of 1/16 in [0, 1]; dG holds small
non-zero integers.  A contribution m sum_k w dG (m: the slot's multiplicity after the table kernel folded a cyclic row) is then a
multiple of 1/16 whose partial sums over k stay below 2^24 last-bit units in any order, it is far above the unit 2^-43 max|dG|, the
64-bit sum is exact, and a destination sum below 2^24 last-bit units makes (float)acc * 2^-s exact: the fp32 result equals float64
and the bf16 result is the round-to-nearest-even bf16 of it.  The bf16 instances hold m w as bf16: it must have 8 significant
bits at the most.  build_cloud() PROVES these statements on float64 sums for the case it returns."""
from collections import namedtuple

import numpy as np

import conv_cases as C
import conv_ref as R
from conv_cases import _bf16, _index_table, _rotations24, hash_name, normalise  # noqa: F401  (normalise: re-exported)

EPN_EINVAL = C.EPN_EINVAL
UC_DUMMY, UC_LDS_MAX, UC_PTS, UC_WAVES = 4, 160 * 1024, 8, 16
_CACHE = {}
# rows: the special rows of _cloud_table are written into the index table
CloudCase = namedtuple("CloudCase", "name nn ks cin na b p2 p1 sigma rows", defaults=(2, 6, 6, 0.25, True))


# ------------------------------------------------------------------------------------------------ dispatch restatement
def _cap(nn, bf16):
    """uc_channels_per_wg: the widest workgroup whose registers fit 16 waves."""
    return (64 if bf16 else 16) if nn > 32 else 64 if (not bf16 and nn > 16) else 128


def channels_per_wg(c, bf16):
    """uc_channels_per_wg: the largest power of two from 16 that divides cin, stays under the cap and fits the LDS; 0: none."""
    best, cr = 0, 16
    while cr <= _cap(c.nn, bf16) and cr <= c.cin:
        if c.cin % cr == 0 and (c.p1 + UC_DUMMY) * cr * 8 + 16 <= UC_LDS_MAX:
            best = cr
        cr *= 2
    return best


def cloud_ok(c):
    """inter_ungroup_cloud_ok."""
    return (C.group_is_mfma(c) and c.na >= 1 and c.nn <= 64 and c.ks <= 32 and c.p1 + UC_DUMMY <= 65536 and c.p2 <= 4096
            and c.cin % 16 == 0 and channels_per_wg(c, 0) > 0 and c.b * c.p2 * c.na * c.cin * c.ks < 2 ** 40)


def _nt(nn):
    return 1 if nn <= 16 else 2 if nn <= 32 else 4


def _name(nt, kt, bf16, nl):
    return f"inter_ungroup_cloud_kernel<{nt},{kt},{'__bf16' if bf16 else 'float'},{UC_WAVES},{nl}>"


def cloud_instance(c, bf16):
    """The instance launch_inter_ungroup_cloud runs; None: the entry refuses the shape (EPN_EINVAL)."""
    if not cloud_ok(c):
        return None
    return _name(_nt(c.nn), (c.ks + 15) // 16, bf16, channels_per_wg(c, bf16) // 16)


def workspace_extra_bytes(c):
    """inter_ungroup_cloud_extra_bytes: offsets [b][p2][16 NT], neighbourhood table [b][p2][5][16 NT], 256 bytes of scalars."""
    r256 = lambda v: (v + 255) & ~255
    return r256(c.b * c.p2 * 16 * _nt(c.nn) * 4) + r256(c.b * c.p2 * _nt(c.nn) * 80 * 4) + 256


# All 48 instances are instantiated; the launcher reaches the 38 under the register caps of uc_channels_per_wg.
_ALL = [(nt, kt, bf16, nl) for nt in (1, 2, 4) for kt in (1, 2) for bf16 in (0, 1) for nl in (1, 2, 4, 8)]
_NN_OF = {1: 16, 2: 32, 4: 64}
REACHABLE_CLOUD = {_name(*i) for i in _ALL if 16 * i[3] <= _cap(_NN_OF[i[0]], i[2])}
UNREACHABLE_CLOUD = {_name(*i): f"uc_channels_per_wg caps {'bf16' if i[2] else 'fp32'} at {_cap(_NN_OF[i[0]], i[2])} channels for "
                                f"NT = {i[0]} (the wider instances spill under the 128-register cap of 16 waves)"
                     for i in _ALL if 16 * i[3] > _cap(_NN_OF[i[0]], i[2])}

# ------------------------------------------------------------------------------------------------ the cases
# The smallest shapes on both sides of every edge.  b = 2 clouds of p1 = 6 points and p2 = 6 output points unless the edge is one
# of them: twelve rows hold the five special rows of conv_cases._index_table and the seven of _cloud_table.  na = 1 .. 5 (the entry
# accepts na >= 1; the anchor is only a grid coordinate).  The comment of a line names what the case is there for; the instances
# are checked by tests/test_cloud_spec.py against INSTANCES below.
K = CloudCase


def _cases():
    out = []
    # nn: the NT edges 16 | 17 and 32 | 33, lanes beyond nn inside a tile (1, 15, 17, 33), all 64 lanes
    for i, nn in enumerate((1, 15, 16, 17, 32, 33, 64)):
        out.append(K(f"nn{nn}", nn, 24, 32, 1 + i % 5))
    # ks: KT = 1 | 2 at 16 | 20, the tail rule koff[kt] = 16 kt + 4 (16 kt + 4 j < ks ? j : 0) at 12, 20, 28, and ks = 32
    for i, ks in enumerate((4, 12, 16, 20, 24, 28, 32)):
        out.append(K(f"ks{ks}", 17, ks, 16, 1 + (i + 2) % 5))
    out += [K("ks12_n64", 64, 12, 16, 2), K("ks28_n64", 64, 28, 32, 3), K("ks32_n64", 64, 32, 16, 1), K("ks20_n16", 16, 20, 32, 4)]
    # cin: every NL under each cap (fp32: 128 / 64 / 16 channels at NT = 1 / 2 / 4, bf16: 128 / 128 / 64), 48 and 96 (the largest
    # power of two that divides them: 16, 32), 256 (two blocks of 128); several channel blocks per grid row wherever cin > cap
    for nn in (16, 32, 64):
        for i, cin in enumerate((16, 32, 48, 64, 96, 128, 256)):
            out.append(K(f"cin{cin}_n{nn}", nn, 24, cin, 1 + (i + nn // 16) % 5))
        for i, cin in enumerate((16, 32, 64, 128)):
            out.append(K(f"cin{cin}_n{nn}_k12", nn, 12, cin, 1 + (i + nn // 32) % 5))
    # LDS capacity (p1 + 4) cr 8 + 16 <= 160 KB: cr 128 -> 64 at p1 = 155 | 156, 64 -> 32 at 315 | 316, 32 -> 16 at 635 | 636,
    # 16 -> refused at 1275 | 1276; p2 = 3; nn and type that allow the cr in question
    for nn, cin, p1 in ((16, 128, 155), (32, 128, 155), (32, 64, 315), (64, 64, 315), (16, 32, 635), (64, 32, 635), (64, 16, 1275),
                        (16, 16, 1275)):
        for q in (p1, p1 + 1):
            out.append(K(f"lds_c{cin}_n{nn}_p{q}", nn, 24, cin, 2, 2, 3, q))
    # p2 against the 16 waves of a workgroup (wave < p2, p += 16, the prefetch of point p + 16)
    for p2 in (1, 15, 16, 17, 33):
        out.append(K(f"p2_{p2}", 17, 24, 32, 2, 2, p2))
    out += [K("p2_17_n64", 64, 32, 16, 1, 2, 17), K("p2_33_n16", 16, 12, 64, 3, 2, 33)]
    # b p2 against the table kernel's 8 points per wave and 32 per workgroup (a ragged tail repeats the last point)
    for b, p2 in ((1, 1), (1, 7), (2, 4), (3, 3), (1, 31), (2, 16), (3, 11)):
        out.append(K(f"pts{b * p2}", 33, 20, 16, 2, b, p2))
    return out


CLOUD_CASES = _cases()
REFUSED = {"lds_c16_n64_p1276", "lds_c16_n16_p1276"}                 # cloud_ok turns False: EPN_EINVAL, nothing written
# (fp32 instance, bf16 instance) the comment of a case claims, for the cases that are there for an instance
INSTANCES = {
    "nn16": (_name(1, 2, 0, 2), _name(1, 2, 1, 2)), "nn17": (_name(2, 2, 0, 2), _name(2, 2, 1, 2)),
    "nn32": (_name(2, 2, 0, 2), _name(2, 2, 1, 2)), "nn33": (_name(4, 2, 0, 1), _name(4, 2, 1, 2)),
    "ks16": (_name(2, 1, 0, 1), _name(2, 1, 1, 1)), "ks20": (_name(2, 2, 0, 1), _name(2, 2, 1, 1)),
    "cin128_n16": (_name(1, 2, 0, 8), _name(1, 2, 1, 8)), "cin256_n16": (_name(1, 2, 0, 8), _name(1, 2, 1, 8)),
    "cin48_n16": (_name(1, 2, 0, 1), _name(1, 2, 1, 1)), "cin96_n16": (_name(1, 2, 0, 2), _name(1, 2, 1, 2)),
    "cin128_n32": (_name(2, 2, 0, 4), _name(2, 2, 1, 8)), "cin256_n64": (_name(4, 2, 0, 1), _name(4, 2, 1, 4)),
    "cin64_n64_k12": (_name(4, 1, 0, 1), _name(4, 1, 1, 4)),
    "lds_c128_n16_p155": (_name(1, 2, 0, 8), _name(1, 2, 1, 8)), "lds_c128_n16_p156": (_name(1, 2, 0, 4), _name(1, 2, 1, 4)),
    "lds_c128_n32_p155": (_name(2, 2, 0, 4), _name(2, 2, 1, 8)), "lds_c128_n32_p156": (_name(2, 2, 0, 4), _name(2, 2, 1, 4)),
    "lds_c64_n32_p315": (_name(2, 2, 0, 4), _name(2, 2, 1, 4)), "lds_c64_n32_p316": (_name(2, 2, 0, 2), _name(2, 2, 1, 2)),
    "lds_c64_n64_p315": (_name(4, 2, 0, 1), _name(4, 2, 1, 4)), "lds_c64_n64_p316": (_name(4, 2, 0, 1), _name(4, 2, 1, 2)),
    "lds_c32_n16_p635": (_name(1, 2, 0, 2), _name(1, 2, 1, 2)), "lds_c32_n16_p636": (_name(1, 2, 0, 1), _name(1, 2, 1, 1)),
    "lds_c32_n64_p635": (_name(4, 2, 0, 1), _name(4, 2, 1, 2)), "lds_c32_n64_p636": (_name(4, 2, 0, 1), _name(4, 2, 1, 1)),
    "lds_c16_n64_p1275": (_name(4, 2, 0, 1), _name(4, 2, 1, 1)), "lds_c16_n64_p1276": (None, None),
    "lds_c16_n16_p1275": (_name(1, 2, 0, 1), _name(1, 2, 1, 1)), "lds_c16_n16_p1276": (None, None),
}
# Tier 3 (maximum and scale) and tier 4 (invariances) run on these
SCALE_CASES = ("nn16", "nn32", "nn64")                               # NT = 1, 2, 4
INVARIANCE_CASES = (("nn15", 17), ("nn32", 33))                      # (case, nn after shadow slots are appended)
# Real-geometry tier: |kernel - fp64| <= CLOUD_REAL_M[type] 2^-24 S element by element, S = sum |w| |dG| of the destination.
# Twice the worst such ratio of emulate_cloud() -- the DOCUMENTED arithmetic in numpy, never the kernel -- over
# conv_cases.REAL_INTER, rounded up to a power of two; tests/test_cloud_spec.py re-measures it and fails if these are not that.
CLOUD_REAL_M = {"f32": 64.0, "bf16": 262144.0}

SPECIAL_KINDS = ("one_point", "cyclic_ragged", "cyclic_breaks", "duplicates", "cyclic_inner", "negative", "beyond")


# ------------------------------------------------------------------------------------------------ the table kernel's folding
def row_period(q):
    """uc_slots_kernel's cnt of one row: the distance to the first repeat of the row's first entry if the whole row repeats with
    that period (a genuinely cyclic row), else the row's length."""
    q = np.asarray(q)
    nn = len(q)
    rep = np.nonzero(q[1:] == q[0])[0]
    cnt = int(rep[0]) + 1 if len(rep) else nn
    return nn if np.any(q[cnt:] != q[:nn - cnt]) else cnt


def slot_multiplicity(idx, p1):
    """uc_slots_kernel's multiplicities m[b, p2, nn]: a genuinely cyclic row (its first cnt entries repeated to the end, the ball
    query's padding) keeps its first cnt slots with the number of slots holding their point, every other row keeps every slot
    once; a slot that names no point (index outside 0 .. p1 - 1) has 0."""
    idx = np.asarray(idx)
    nn = idx.shape[2]
    m = np.zeros(idx.shape, np.int64)
    n = np.arange(nn)
    for bb in range(idx.shape[0]):
        for pp in range(idx.shape[1]):
            q = idx[bb, pp]
            cnt = row_period(q)
            m[bb, pp] = np.where((q >= 0) & (q < p1) & (n < cnt), (nn - 1 - n) // cnt + 1, 0)
    return m


def permute_slots(idx, rng):
    """Another order of the same multiset in every row; a cyclic row stays cyclic: its period is permuted, the nn % cnt points
    that hold one slot more among themselves."""
    out = np.array(idx)
    nn = out.shape[2]
    for bb in range(out.shape[0]):
        for pp in range(out.shape[1]):
            cnt = row_period(out[bb, pp])
            if cnt == nn:
                out[bb, pp] = rng.permutation(out[bb, pp])
            else:
                r = nn % cnt
                period = np.concatenate([rng.permutation(out[bb, pp, :r]), rng.permutation(out[bb, pp, r:cnt])])
                out[bb, pp] = period[np.arange(nn) % cnt]
            assert sorted(out[bb, pp].tolist()) == sorted(np.asarray(idx)[bb, pp].tolist())
    return np.ascontiguousarray(out)


def duplicate_rows(idx, p1):
    """Rows whose KEPT slots (every slot of a row that is not cyclic, the period of a cyclic one) name a point more than once:
    their contributions meet in one accumulator, and the table kernel reports nn as their multiplicity.  True per [b, p2]."""
    idx = np.asarray(idx)
    m = slot_multiplicity(idx, p1)
    out = np.zeros(idx.shape[:2], bool)
    for bb in range(idx.shape[0]):
        for pp in range(idx.shape[1]):
            q = idx[bb, pp][m[bb, pp] > 0]
            out[bb, pp] = len(np.unique(q)) < len(q)
    return out


def fits_bf16(v):
    v = np.asarray(v, np.float32)
    return np.array_equal(_bf16(v), v)


# ------------------------------------------------------------------------------------------------ builders
def _row_weights(xyz_b, centre, q, rk, sigma):
    """w[a, k] of one neighbour offset xyz_b[:, q] - centre in float64."""
    g = np.asarray(xyz_b, np.float64)[:, q] - np.asarray(centre, np.float64)
    d = g[None, None, :] - rk
    return np.maximum(0.0, 1.0 - (d * d).sum(-1) / float(sigma))


def _cloud_table(rng, c, xyz, new_xyz, rk):
    """conv_cases._index_table plus, on rows it left ordinary (from the last row backwards, in an order that turns with the
    case's name so that small cases take different ones), the rows the table kernel must fold or must not fold:
      one_point      one point in every slot: cyclic, multiplicity nn (its centre is moved, if need be, to where nn w has 8
                     significant bits for every anchor and kernel point and is not zero everywhere)
      cyclic_ragged  cnt distinct points repeated, cnt no divisor of nn: multiplicities differ by one
      cyclic_breaks  [1, 2, 1, 3, ...]: starts cyclic and breaks -- every slot once
      duplicates     [3, 5, 3, 3, ...]: one point many times without being cyclic -- every slot once
      cyclic_inner   [1, 2, 2, 4, 2] repeated: cyclic, folded, and its period names point 2 three times
      negative       an index of -1 early in the row and in the last slot (the last neighbour tile)
      beyond         indices p1 + 1 and 2^30 early in the row and in the last slot
    Returns (idx, new_xyz, {kind: (b, p)})."""
    p1, nn = c.p1, c.nn
    base = c if c.b >= 2 or c.b * c.p2 < 6 else c._replace(b=2)          # (_index_table writes cloud 1's rows from six rows on)
    idx = _index_table(rng, base)[:c.b].copy()
    new_xyz = new_xyz.copy()
    placed = {}
    if not c.rows:
        return idx, new_xyz, placed
    taken = {(0, 0), (0, 1), (0, 2), (1, 0), (1, 1)} if c.b * c.p2 >= 6 else set()
    free = [(bb, pp) for bb in range(c.b) for pp in range(c.p2) if (bb, pp) not in taken][::-1]
    turn = hash_name(c.name) % len(SPECIAL_KINDS)
    n = np.arange(nn)
    for kind in SPECIAL_KINDS[turn:] + SPECIAL_KINDS[:turn]:
        if not free:
            break
        bb, pp = free[0]
        row = idx[bb, pp].copy()
        if kind == "one_point":
            grid = [new_xyz[bb, :, pp].copy()] + [(np.array(v, np.float32) - 2) / 8 for v in np.ndindex(5, 5, 5)]
            found = None
            for centre in grid:
                for q in range(min(p1, 6)):
                    w = _row_weights(xyz[bb], centre, q, rk, c.sigma)
                    if w.max() > 0 and fits_bf16(nn * w):
                        found = (centre, q)
                        break
                if found:
                    break
            if not found:
                continue
            new_xyz[bb, :, pp] = found[0]
            row[:] = found[1]
        elif kind == "cyclic_ragged":
            cnt = next((k for k in (5, 6, 7, 3, 4, 2) if k < nn and nn % k and (nn + k - 1) // k <= 15 and k <= p1), None)
            if cnt is None:
                continue
            row[:] = (n % cnt + 1) % p1
        elif kind == "cyclic_breaks":
            if nn < 4:
                continue
            row[:4] = (1, 2, 1, 3)
            row[4:] = np.where(row[4:] >= p1, 4, row[4:])
        elif kind == "duplicates":
            if nn < 4:
                continue
            row[:] = 3
            row[1] = 5
        elif kind == "cyclic_inner":
            if nn < 10 or p1 < 5:
                continue
            row[:] = np.array([1, 2, 2, 4, 2])[n % 5]
        elif kind == "negative":
            row[min(1, nn - 1)] = row[nn - 1] = -1
        else:
            row[min(2, nn - 1)] = p1 + 1
            row[nn - 1] = 2 ** 30
        idx[bb, pp] = row
        placed[kind] = free.pop(0)
    return idx.astype(np.int32), new_xyz, placed


def _geometry(c, rng):
    anchors = _rotations24()[np.arange(c.na) % 24].astype(np.float32)
    eighth = lambda shape, m: (rng.integers(-m, m + 1, size=shape) / 8.0).astype(np.float32)
    kernels = eighth((c.ks, 3), 2)
    xyz, new_xyz = eighth((c.b, 3, c.p1), 2), eighth((c.b, 3, c.p2), 2)
    return anchors, kernels, xyz, new_xyz


def prove_exact(c, geo, dG, add=None):
    """The conditions of the module's docstring for one operand set, asserted on float64 sums.  Returns (ref, bits): the float64
    dF and the largest partial / destination sum in units of 2^24 last bits (1/16: the weights' last bit)."""
    xyz, new_xyz, idx, anchors, kernels, sigma = geo
    w = R.inter_weights(*geo)[0]
    assert np.array_equal(w * 16.0, np.round(w * 16.0)) and w.max() <= 1.0, c                     # multiples of 1/16 in [0, 1]
    m = slot_multiplicity(idx, c.p1)
    mw = m[:, :, None, None, :] * w
    assert fits_bf16(mw), (c, "a weight times its multiplicity needs more than bf16's 8 significant bits")
    ref = R.inter_ungroup(*geo, dG, c.cin)
    # what the kernel adds up: per folded slot m sum_k w dG -- the same total as the plain sum over valid slots
    dG5 = np.asarray(dG, np.float64).reshape(c.b, c.p2, c.na, c.cin, c.ks)
    folded = np.einsum("bpakn,bpack->bpnac", mw, dG5, optimize=True)
    plain = np.einsum("bpakn,bpack->bpnac", w, dG5, optimize=True)
    safe = R.inter_gather(xyz, new_xyz, idx)[2]
    chk, chk2 = np.zeros_like(ref), np.zeros_like(ref)
    for bb in range(c.b):
        np.add.at(chk[bb], safe[bb].reshape(-1), folded[bb].reshape(-1, c.na, c.cin))
        np.add.at(chk2[bb], safe[bb].reshape(-1), plain[bb].reshape(-1, c.na, c.cin))
    assert np.array_equal(chk, ref) and np.array_equal(chk2, ref), c
    part = np.einsum("bpakn,bpack->bpnac", mw, np.abs(dG5), optimize=True)                        # bounds every partial sum over k
    dest = R.inter_ungroup(*geo, np.abs(dG), c.cin) + (0 if add is None else np.abs(add))
    bits = dict(partial=float(part.max(initial=0)) * 16.0 / 2.0 ** 24, dest=float(dest.max(initial=0)) * 16.0 / 2.0 ** 24)
    assert max(bits.values()) < 1.0, (c, bits)
    assert np.array_equal(ref * 16.0, np.round(ref * 16.0)) and np.array_equal(ref, ref.astype(np.float32)), c
    return ref, bits


def build_cloud(c):
    """The dyadic case: geometry of conv_cases.build_group, the index table of _cloud_table, dG of non-zero integers of magnitude
    <= q (the largest of 3, 2, 1 whose sums of absolute values stay below 2^24 last-bit units, picked as build_inter picks it) and
    `add` of integers in [-4, 4]; `ref` (float64 dF without add), `bits`, `special`.  Deterministic in the case's name."""
    rng = np.random.default_rng(hash_name(c.name))
    anchors, kernels, xyz, new_xyz = _geometry(c, rng)
    rk = np.einsum("ade,ke->akd", anchors.astype(np.float64), kernels.astype(np.float64))
    idx, new_xyz, special = _cloud_table(rng, c, xyz, new_xyz, rk)
    geo = (xyz, new_xyz, idx, anchors, kernels, c.sigma)
    shape = (c.b * c.p2 * c.na, c.cin * c.ks)
    sign = (1 - 2 * rng.integers(0, 2, size=shape)).astype(np.float32)
    mag = rng.integers(1, 4, size=shape)
    add = rng.integers(-4, 5, size=(c.b, c.p1, c.na, c.cin)).astype(np.float32)
    # every |term| grows with q: one evaluation at q = 1 picks q, prove_exact at that q is the proof
    first = float(R.inter_ungroup(*geo, np.abs(sign), c.cin).max(initial=0)) * 16.0 / 2.0 ** 24
    q = 3 if 3 * first + 4 * 16.0 / 2.0 ** 24 < 1.0 else 2 if 2 * first + 4 * 16.0 / 2.0 ** 24 < 1.0 else 1
    dG = sign * np.minimum(mag, q).astype(np.float32)
    ref, bits = prove_exact(c, geo, dG, add)
    return dict(xyz=xyz, new_xyz=new_xyz, idx=idx, anchors=anchors, kernels=kernels, sigma=c.sigma, dG=dG, add=add, ref=ref, q=q,
                bits=bits, special=special)


def cloud_case(c):
    if c not in _CACHE:
        _CACHE[c] = build_cloud(c)
    return _CACHE[c]


def by_name(name):
    return next(c for c in CLOUD_CASES if c.name == name)


def expected(ref, add, out_bf16):
    """What the entry must write, bit for bit: float64 (+ add) as fp32, or its round-to-nearest-even bf16 (as float32 values)."""
    v = (ref if add is None else ref + add.astype(np.float64)).astype(np.float32)
    return _bf16(v) if out_bf16 else v


# ---- coinciding kernel points: every kernel point sits on the one neighbour offset there is, so that w = 1 for every k
AMAX_TOP = np.float32(255.0 / 256.0)         # just below a power of two, 8 significant bits (bf16 holds it)


def _coinciding(c, row, dG_value):
    v = np.array([0.125, 0.0, 0.125], np.float32)
    anchors = np.eye(3, dtype=np.float32)[None]
    kernels = np.tile(v, (c.ks, 1))
    xyz = np.tile(v[None, :, None], (c.b, 1, c.p1))
    new_xyz = np.zeros((c.b, 3, c.p2), np.float32)
    idx = np.tile(np.asarray(row, np.int32), (c.b, c.p2, 1))
    geo = (xyz, new_xyz, idx, anchors, kernels, c.sigma)
    w = R.inter_weights(*geo)[0]
    assert np.array_equal(w, np.ones_like(w)), "w = 1 for every kernel point"
    return geo, np.asarray(dG_value, np.float32)


def extreme_case():
    """The bound's extreme INSIDE the contract: nn = 64, ks = 32, w = 1 everywhere, every |dG| = AMAX_TOP (random signs), every
    row one point 64 times (cyclic: multiplicity 64).  One contribution is 64 * 32 * amax = 2^50 (1 - 2^-8) units.  Three output
    points: the sums stay below 2^24 units of amax's last bit, so the result is exact."""
    c = CloudCase("extreme", 64, 32, 16, 1, 1, 3, 6, 0.25, False)
    rng = np.random.default_rng(hash_name(c.name))
    sign = (1 - 2 * rng.integers(0, 2, size=(c.b * c.p2 * c.na, c.cin * c.ks))).astype(np.float32)
    geo, dG = _coinciding(c, np.full(64, 3), sign * AMAX_TOP)
    assert slot_multiplicity(geo[2], c.p1).max() == 64
    ref = R.inter_ungroup(*geo, dG, c.cin)
    units = R.inter_ungroup(*geo, np.abs(dG), c.cin) * 256.0                       # in amax's last bit
    assert units.max() < 2 ** 24 and np.array_equal(ref, ref.astype(np.float32)) and np.any(ref != 0)
    return c, geo, dG, ref


# Rows whose kept slots meet in one accumulator, nn = 64: (row, the point that is named most, kept slots naming it, multiplicity
# of a kept slot, the other point).  "plain": not cyclic, every slot kept once.  "period": cyclic with period 32, every kept slot
# twice, 31 of them on point 2 -- folded, and still many contributions into one accumulator.
WRAP_ROWS = {"plain": (np.array([3, 5] + [3] * 62), 3, 63, 1, 5),
             "period": (np.array(([1] + [2] * 31) * 2), 2, 31, 2, 1)}


def wrap_crossing(kind):
    """w = 1, ks = 32, dG = +AMAX_TOP, every row WRAP_ROWS[kind].  With only the folded multiplicity m reported, uc_scale lets
    m ks amax reach 2^50 (1 - 2^-8) units per kept slot; the accumulator of the point holds `slots` p2 of them.  Returns the
    smallest p2 whose float64 sum of units reaches 2^63 (131 and 266)."""
    row, point, slots, m, other = WRAP_ROWS[kind]
    scale = 2.0 ** (50 - 5 - (m - 1))                                              # 2^s = 2^(50 - ceil(log2(m ks))), amax < 2^0
    per_point = slots * m * 32.0 * float(AMAX_TOP) * scale
    p2 = int(np.ceil(2.0 ** 63 / per_point))
    assert (p2 - 1) * per_point < 2.0 ** 63 <= p2 * per_point
    return p2


def wrap_case(kind, p2):
    row, point, slots, m, other = WRAP_ROWS[kind]
    c = CloudCase(f"wrap_{kind}_p{p2}", 64, 32, 16, 1, 1, p2, 6, 0.25, False)
    geo, dG = _coinciding(c, row, np.full((c.b * c.p2 * c.na, c.cin * c.ks), AMAX_TOP))
    assert duplicate_rows(geo[2], c.p1).all() and slot_multiplicity(geo[2], c.p1).max() == m
    assert (row_period(row) == 64) == (kind == "plain")
    ref = R.inter_ungroup(*geo, dG, c.cin)                                         # exact in float64: integers below 2^53 / 256
    assert np.array_equal(ref[0, point], np.full((1, c.cin), slots * m * 32.0 * p2 * float(AMAX_TOP)))
    assert np.array_equal(ref[0, other], np.full((1, c.cin), (64 - slots * m) * 32.0 * p2 * float(AMAX_TOP)))
    assert not ref[0, [q for q in range(6) if q not in (point, other)]].any()
    # one rounding: float64 -> bf16 directly and through fp32 give the same value here (checked, not assumed)
    assert np.array_equal(_bf16(ref.astype(np.float32)).astype(np.float64), _round_bf16_from_f64(ref))
    return c, geo, dG, ref


def _round_bf16_from_f64(v):
    """Round-to-nearest-even of float64 values to 8 significant bits (values far from the exponent limits)."""
    v = np.asarray(v, np.float64)
    m, e = np.frexp(v)
    return np.ldexp(np.round(m * 256.0), e - 8)                                    # np.round: half to even


# ------------------------------------------------------------------------------------------------ real geometry
def real_cloud_reference(entry):
    """(CloudCase, arrays, float64 dF, S) of a geometry of conv_cases.REAL_INTER with a normal, bf16-representable dG (one
    operand serves both types); S[b, q, a, c] = sum |w| |dG| of the destination."""
    if ("real", entry) not in _CACHE:
        ic, d = C.real_inter_case(entry)
        c = CloudCase(ic.name, ic.nn, ic.ks, ic.cin, ic.na, ic.b, ic.p2, ic.p1, ic.sigma, False)
        rng = np.random.default_rng(hash_name("cloud " + c.name))
        dG = _bf16(rng.standard_normal((c.b * c.p2 * c.na, c.cin * c.ks)))
        geo = (d["xyz"], d["new_xyz"], d["idx"], d["anchors"], d["kernels"], np.float32(d["sigma"]))
        d = dict(d, dG=dG)
        _CACHE[("real", entry)] = (c, d, R.inter_ungroup(*geo, dG, c.cin), R.inter_ungroup(*geo, np.abs(dG), c.cin))
    return _CACHE[("real", entry)]


def weights_fp32(d):
    """w[b, p, a, k, n] as the kernel's tables and its S-MFMA evaluate it, in float32 with one rounding per fused step:
    alpha_n + g . r_ak + beta_ak, g = xyz - centre, alpha = 1 - |g|^2 / sigma, r = (2 / sigma) R_a kappa_k,
    beta = -|R_a kappa_k|^2 / sigma; clamped at 0; 0 in a slot that names no point."""
    f32, f64 = np.float32, np.float64
    fma = lambda a, b, c: (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)
    g, valid, safe = R.inter_gather(d["xyz"], d["new_xyz"], d["idx"])
    g = g.astype(f32)
    A, Kp = np.asarray(d["anchors"], f32), np.asarray(d["kernels"], f32)
    rk = np.stack([fma(A[:, None, i, 2], Kp[None, :, 2], fma(A[:, None, i, 1], Kp[None, :, 1], (A[:, None, i, 0] * Kp[None, :, 0]).astype(f32)))
                   for i in range(3)], -1)                                                         # [a, k, 3]
    sinv = f32(1.0) / f32(d["sigma"])
    g2 = fma(g[..., 2], g[..., 2], fma(g[..., 1], g[..., 1], (g[..., 0] * g[..., 0]).astype(f32)))
    alpha = (f32(1.0) - (g2 * sinv).astype(f32)).astype(f32)[:, :, None, None, :]
    r = (f32(2.0) * sinv * rk).astype(f32)
    r2 = fma(rk[..., 2], rk[..., 2], fma(rk[..., 1], rk[..., 1], (rk[..., 0] * rk[..., 0]).astype(f32)))
    s = np.broadcast_to(alpha, alpha.shape[:2] + rk.shape[:2] + alpha.shape[-1:])
    for i in range(3):
        s = fma(np.broadcast_to(g[:, :, None, None, :, i], s.shape), np.broadcast_to(r[None, None, :, :, None, i], s.shape), s)
    s = (s - np.broadcast_to((r2 * sinv).astype(f32)[None, None, :, :, None], s.shape)).astype(f32)
    return (np.maximum(s, f32(0.0)) * valid[:, :, None, None, :]).astype(f32)


def emulate_cloud(c, d, w32, bf16):
    """The documented arithmetic of the kernel in numpy: fp32 weights w32[b, p, a, k, n] (times the folded multiplicity and
    rounded to bf16 for the bf16 instances), fp32 products, an exact sum (float64 here), one rounding to the output type."""
    m = slot_multiplicity(d["idx"], c.p1)
    if bf16:
        wm = _bf16((m[:, :, None, None, :].astype(np.float32) * w32).astype(np.float32))
    else:
        wm = w32 * (m > 0)[:, :, None, None, :]
        mult = m.astype(np.float64)
    dG5 = d["dG"].reshape(c.b, c.p2, c.na, c.cin, c.ks)
    T = np.zeros((c.b, c.p2, c.nn, c.na, c.cin))
    for k in range(c.ks):
        prod = wm[:, :, :, k, :].transpose(0, 1, 3, 2)[..., None] * dG5[:, :, None, :, :, k]          # float32 products
        assert prod.dtype == np.float32
        T += prod
    if not bf16:
        T *= mult[:, :, :, None, None]
    safe = R.inter_gather(d["xyz"], d["new_xyz"], d["idx"])[2]
    dF = np.zeros((c.b, c.p1, c.na, c.cin))
    for bb in range(c.b):
        np.add.at(dF[bb], safe[bb].reshape(-1), T[bb].reshape(-1, c.na, c.cin))
    return _round_bf16_from_f64(dF) if bf16 else dF.astype(np.float32).astype(np.float64)
