"""Case tables of the exact convolution tests (tests/test_gpu_conv_exact.py, tests/test_conv_spec.py), of the instance tests of the
grouping entries (tests/test_gpu_group_dispatch.py) and a restatement of the
dispatch of csrc/inter_mfma.hip and csrc/intra_mfma.hip: which kernel instance epn_last_kernel() must name for a descriptor and a
pass.  Nothing here needs a device; only the real-geometry builders need the package and the CPU oracle.

Why `==` is legitimate for the inter convolution: anchors are signed permutation matrices, coordinates multiples of
1/8 in [-1, 1] (here in [-1/4, 1/4], so that the clamp cuts about half of the weights), sigma a power of two, features, W and
upstream gradients small integers.  Every term of w = relu(1 - |g - R_a kappa_k|^2 / sigma) and of its expanded form
alpha_n + beta_k + g . r is then a multiple of 1/16 of a few bits, w is the same float under any evaluation order, and every
partial sum of out, dF and dW stays below 2^24 last-bit units -- build_inter() PROVES the last two statements for the case it
returns (assertions on float64 sums), tests/test_conv_spec.py the first."""
import itertools
import re
from collections import namedtuple

import numpy as np

import conv_ref as R

PASSES = ("fwd", "bwd_data", "bwd_weight")
OUTPUT = dict(fwd="out", bwd_data="dF", bwd_weight="dW")          # the tensor of conv_ref's result a pass is compared with
EPN_KS_MAX, EPN_NN_MAX = 32, 128

_CACHE = {}
InterCase = namedtuple("InterCase", "name nn ks cin cout na b p2 passes sigma p1", defaults=(PASSES, 0.25, 6))
GroupCase = namedtuple("GroupCase", "name nn ks cin na p2 b p1 sigma", defaults=(2, 6, 0.25))
InvCase = namedtuple("InvCase", "name b p1 p2 nn")
IntraCase = namedtuple("IntraCase", "name kn cin cout na b p", defaults=(2, 3))


def normalise(name):
    """epn_last_kernel()'s text -> the spelling used here: no namespace, no blanks.  A name the C++ runtime could not demangle
    (it does not know DF16b, the bf16 type of the grouping kernels' template arguments) comes back mangled and is read here."""
    if isinstance(name, bytes):
        name = name.decode()
    if name.startswith("_Z"):
        name = _demangle(name)
    # ... and ONE such name it does demangle, wrongly: `DF16b Li2E Li1E` (bf16, GP = 2, NB = 1: the K = 128 scatter) is read as a
    # fixed-point type and the two integers are lost.  No other instance has that text (tests/test_conv_spec.py).
    return name.replace("epn::", "").replace(" ", "").replace("bool_Accum,int,EL,int,E", "__bf16,2,1")


def _demangle(m):
    """_ZN3epn12_GLOBAL__N_1<len><kernel>I<args>E...: a kernel template of the library's anonymous namespace whose arguments are
    integers, booleans, float or bf16."""
    mo = re.match(r"_ZN3epn12_GLOBAL__N_1(\d+)", m)
    if not mo:
        raise ValueError(m)
    start = mo.end()
    kernel, rest = m[start:start + int(mo.group(1))], m[start + int(mo.group(1)):]
    if not rest.startswith("I"):
        return kernel
    rest, args = rest[1:], []
    while not rest.startswith("E"):
        mo = re.match(r"Li(\d+)E|Lb([01])E|(f)|(DF16b)", rest)
        if not mo:
            raise ValueError(m)
        args.append(mo.group(1) or (("false", "true")[int(mo.group(2))] if mo.group(2) else "float" if mo.group(3) else "__bf16"))
        rest = rest[mo.end():]
    return f"{kernel}<{','.join(args)}>"


# ------------------------------------------------------------------------------------------------ dispatch restatement
def inter_is_fused(c):
    """conv_internal.h inter_mfma_shape_ok."""
    return (c.cin % 16 == 0 and c.cout % 16 == 0 and 16 <= c.cout <= 256 and c.cin >= 16 and c.ks <= EPN_KS_MAX
            and c.ks % 4 == 0 and c.nn <= EPN_NN_MAX)


def intra_is_fused(c):
    """intra_mfma.hip intra_uses_mfma."""
    return c.cin % 16 == 0 and c.cout % 16 == 0 and 16 <= c.cin <= 256 and 16 <= c.cout <= 256


def use8(c):
    """inter_mfma.hip use8: the 8-wave forward / weight-gradient kernels."""
    return c.na >= 16 and 16 < c.ks <= 32 and c.nn <= 32


def _nt(nn):
    """inter_mfma.hip nt_slot: neighbour tiles of 16, rounded up to 1, 2, 4, 8."""
    t = (nn + 15) // 16
    return 1 if t <= 1 else 2 if t <= 2 else 4 if t <= 4 else 8


def inter_instance(c, which):
    assert inter_is_fused(c), c
    nt, kt = _nt(c.nn), (c.ks + 15) // 16
    nt8 = 1 if c.nn <= 16 else 2
    if which == "fwd":
        mt = c.cout // 16
        if use8(c) and mt in (1, 2, 4, 8, 16):
            return f"inter_fwd8_kernel<{nt8},{mt}>"
        return f"inter_fwd_kernel<{nt},{kt}>"
    if which == "bwd_data":
        if c.na >= 16 and c.nn <= 32 and c.ks in (16, 24, 32):
            return f"inter_bwd_data8_kernel<{nt8},{1 if c.ks == 16 else 2},{c.ks // 2}>"
        return f"inter_bwd_data_kernel<{nt},{kt},{'true' if c.ks == 32 else 'false'}>"
    if which == "bwd_weight":
        if use8(c) and c.ks == 24 and (c.cout % 128 == 0 or c.cout in (32, 64)):
            return f"inter_bwd_weight8_kernel<{nt8},{8 if c.cout >= 128 else c.cout // 16}>"
        return f"inter_bwd_weight_kernel<{nt},{kt}>"
    raise ValueError(which)


def inter_weight_grad_plan(c):
    """(column tiles, col_tiles_per_wg, workgroups along x) of launch_inter_bwd_weight_mfma."""
    ncol = c.b * c.p2 * c.na
    eight = "8_kernel" in inter_instance(c, "bwd_weight")
    width, fill = (128, 256 * 2) if eight else (64, 256 * 4)
    tiles = (ncol + width - 1) // width
    blocks = (c.cin // 16) * ((c.cout + 127) // 128)
    splits = max(1, min((fill + blocks - 1) // blocks, tiles))
    per = (tiles + splits - 1) // splits
    return tiles, per, (tiles + per - 1) // per


def intra_instance(c, which):
    assert intra_is_fused(c), c
    if which in ("fwd", "bwd_data"):
        return "intra_gemm_kernel"
    if c.cin % 64 == 0 and c.cout % 64 == 0:
        return "intra_bwd_weight_pt_kernel" if 4 <= c.kn <= 12 and c.na <= 64 else "intra_bwd_weight_v4_kernel"
    return "intra_bwd_weight_kernel"


def intra_point_tile_plan(c):
    """(points, pts_per_wg, workgroups along x) of intra_bwd_weight_pt_kernel in launch_intra_bwd_weight_mfma."""
    npts = c.b * c.p
    blocks = (c.cout // 64) * (c.cin // 64)
    wgs = min((256 * 2 + blocks - 1) // blocks, npts)
    per = (npts + wgs - 1) // wgs
    return npts, per, (npts + per - 1) // per


def intra_weight_grad_plan(c):
    """(column tiles, col_tiles_per_wg) of launch_intra_bwd_weight_mfma (the one-wave-per-k kernels)."""
    tiles = (c.b * c.p * c.na + 15) // 16
    blocks = ((c.kn + 3) // 4) * ((c.cout + 63) // 64) * ((c.cin + 63) // 64)
    splits = (256 * 4 + blocks - 1) // blocks
    if c.kn == 1:
        splits = (splits + 3) // 4
    splits = max(1, min(splits, tiles))
    return tiles, (tiles + splits - 1) // splits


# ---- grouping and its transposes (launch_inter_group_mfma, launch_inter_ungroup_mfma, launch_inter_ungroup_det_mfma and
# launch_inverse_list of inter_mfma.hip behind the epn_inter_group* / epn_inter_ungroup* / epn_inter_inverse_list entries)
MORTON_MAX = USH_TAB = 4096
INV_LDS_ENT, INV_LDS_P1 = 32768, 4096
EPN_EINVAL = -1


def group_is_mfma(c):
    """conv_internal.h inter_group_mfma_ok (anything else takes the generic kernels of conv_generic.hip)."""
    return c.cin % 16 == 0 and c.ks <= EPN_KS_MAX and c.ks % 4 == 0 and c.nn <= EPN_NN_MAX and c.p1 * c.na * c.cin < 2 ** 31


def group_packed_ok(c):
    """conv_internal.h inter_group_packed_ok."""
    return group_is_mfma(c) and c.na >= 16 and c.cin % 32 == 0 and c.nn <= 64


def _tg(bf16):
    return "__bf16" if bf16 else "float"


def group_instance(c, bf16, packed):
    """Instance of epn_inter_group{,_packed}_{f32,bf16}; None: the entry refuses the shape (EPN_EINVAL)."""
    assert group_is_mfma(c), c
    if packed and not group_packed_ok(c):
        return None
    nt, kt = _nt(c.nn), 1 if (c.ks + 15) // 16 == 1 else 2
    if c.na >= 16 and c.cin % 32 == 0 and c.nn <= 64 and (bf16 or c.nn > 16 or packed):
        return f"inter_group_wide_kernel<{nt},{kt},{_tg(bf16)},{4 if c.cin % 64 == 0 else 2}>"
    return f"inter_group_kernel<{nt},{kt},{_tg(bf16)}>"


def ungroup_group_points(c):
    """inter_mfma.hip ungroup_group_points: output points per workgroup of the LDS-reduced scatter."""
    nt = (c.nn + 15) // 16
    return 8 if nt <= 1 else (16 if c.p2 % 16 == 0 else 8) if nt <= 2 else (8 if c.p2 % 8 == 0 else 4) if nt <= 4 else 2


def _shared_ok(c, gp):
    return c.p2 % gp == 0 and c.p2 <= MORTON_MAX and c.p1 <= USH_TAB


def _shared(c, bf16, gp, det, cw):
    nt, kt = _nt(c.nn), 1 if (c.ks + 15) // 16 == 1 else 2
    nb = 2 if nt == 1 and gp == 8 else 1
    return f"inter_ungroup_shared_kernel<{nt},{kt},{_tg(bf16)},{gp},{nb},{'true' if det else 'false'},{cw},1>"


def ungroup_plan(c):
    """(points per workgroup, chunks per anchor step) of the LDS-reduced scatter of launch_inter_ungroup_mfma, or None where
    the per-slot atomic scatter runs (p2 no multiple of the group, or beyond the Morton sort / the destination table)."""
    nt = (c.nn + 15) // 16
    gp = ungroup_group_points(c)
    if nt == 2 and c.cin % 64 != 0 and c.cin % 32 == 0 and c.p2 % 8 == 0:
        gp = 8
    if not _shared_ok(c, gp):
        return None
    wide = c.cin % 64 == 0 and nt <= 2
    wide2 = not wide and c.cin % 32 == 0 and ((2 < nt <= 4 and gp == 8) or nt == 2)
    return gp, 4 if wide else 2 if wide2 else 1


def ungroup_instance(c, bf16):
    """Instance of epn_inter_ungroup_{f32,bf16} (default kernel policy; the entries always pass the Morton-order scratch)."""
    assert group_is_mfma(c), c
    plan = ungroup_plan(c)
    if plan is None:
        return f"inter_ungroup_kernel<{_nt(c.nn)},{1 if (c.ks + 15) // 16 == 1 else 2},{_tg(bf16)}>"
    return _shared(c, bf16, plan[0], False, plan[1])


def ungroup_det_instance(c, bf16):
    """Instance of epn_inter_ungroup_det_{f32,bf16} given a slab with room for the row marks; None: refused (c_api.hip: fewer
    than 16 anchors, or rows that are no multiple of four floats)."""
    assert group_is_mfma(c), c
    if c.na < 16 or (c.na * c.cin) % 4:
        return None
    gp = ungroup_group_points(c)
    if _shared_ok(c, gp):
        return _shared(c, bf16, gp, True, 1)
    return f"inter_ungroup_slots_kernel<{_nt(c.nn)},{1 if (c.ks + 15) // 16 == 1 else 2},{_tg(bf16)}>"


def inverse_list_instance(c):
    """launch_inverse_list: the counting sort in LDS while a cloud's entries and points fit it."""
    return "inverse_list_lds_kernel" if c.p2 * c.nn <= INV_LDS_ENT and c.p1 <= INV_LDS_P1 else "inverse_list_kernel"


def packed_position(cin, ks):
    """conv_internal.h inter_packed_position for every plain column c * ks + k."""
    cg = 4 if cin % 64 == 0 else 2
    c, k = np.divmod(np.arange(cin * ks), ks)
    cl = c % (16 * cg)
    slot = c - cl + 16 * (cl % cg) + cl // cg
    w0 = min(ks, 16)
    return np.where(k < 16, slot * w0 + k, w0 * cin + slot * (ks - 16) + (k - 16))


# Every instance the launchers can reach.  (No instance of the two files is unreachable: the 4-wave forward and data-gradient
# kernels at ks = 32, and the 8-wave data gradient <*, 2, 16>, asked for more than the 160 KB of LDS until this table was
# written -- CHANGELOG -- and are reachable since.)
REACHABLE = {
    ("inter", "fwd"): {f"inter_fwd_kernel<{n},{k}>" for n in (1, 2, 4, 8) for k in (1, 2)}
                      | {f"inter_fwd8_kernel<{n},{m}>" for n in (1, 2) for m in (1, 2, 4, 8, 16)},
    ("inter", "bwd_data"): {f"inter_bwd_data_kernel<{n},{k},false>" for n in (1, 2, 4, 8) for k in (1, 2)}
                           | {f"inter_bwd_data_kernel<{n},2,true>" for n in (1, 2, 4, 8)}
                           | {f"inter_bwd_data8_kernel<{n},{k},{m}>" for n in (1, 2) for k, m in ((1, 8), (2, 12), (2, 16))},
    ("inter", "bwd_weight"): {f"inter_bwd_weight_kernel<{n},{k}>" for n in (1, 2, 4, 8) for k in (1, 2)}
                             | {f"inter_bwd_weight8_kernel<{n},{m}>" for n in (1, 2) for m in (2, 4, 8)},
    ("intra", "fwd"): {"intra_gemm_kernel"},
    ("intra", "bwd_data"): {"intra_gemm_kernel"},
    ("intra", "bwd_weight"): {"intra_bwd_weight_kernel", "intra_bwd_weight_v4_kernel", "intra_bwd_weight_pt_kernel"},
}
# The grouping families (a dictionary of their own: the keys of REACHABLE are (layer, pass)).  Instantiated in inter_mfma.hip but out of the launchers' reach, hence not listed: the wide grouping with
# NT = 8 (it is asked for at nn <= 64 only) and the scatter <2, *, *, 16, 1, false, 2, 1> (two chunks per step at NT = 2 means
# cin % 64 = 32, where a p2 that 16 divides is moved to groups of 8).
_NK = [(n, k) for n in (1, 2, 4, 8) for k in (1, 2)]
_T = ("float", "__bf16")
_GROUPS = ((1, 8, 2), (2, 16, 1), (2, 8, 1), (4, 8, 1), (4, 4, 1), (8, 2, 1))        # (NT, GP, NB) of the LDS-reduced scatter
REACHABLE_GROUPING = {
    "group": {f"inter_group_kernel<{n},{k},{t}>" for n, k in _NK for t in _T}
             | {f"inter_group_wide_kernel<{n},{k},{t},{g}>" for n, k in _NK if n <= 4 for t in _T for g in (2, 4)},
    "ungroup": {f"inter_ungroup_kernel<{n},{k},{t}>" for n, k in _NK for t in _T}
               | {f"inter_ungroup_shared_kernel<{n},{k},{t},{gp},{nb},false,{cw},1>" for n, gp, nb in _GROUPS for k in (1, 2)
                  for t in _T for cw in (1, 2, 4)
                  if cw == 1 or (cw == 4 and n <= 2) or (cw == 2 and (n, gp) in ((2, 8), (4, 8)))},
    "ungroup_det": {f"inter_ungroup_slots_kernel<{n},{k},{t}>" for n, k in _NK for t in _T}
                   | {f"inter_ungroup_shared_kernel<{n},{k},{t},{gp},{nb},true,1,1>" for n, gp, nb in _GROUPS for k in (1, 2)
                      for t in _T},
    "inverse_list": {"inverse_list_lds_kernel", "inverse_list_kernel"},
}

# ------------------------------------------------------------------------------------------------ the cases
# Column counts b p2 na against the 64 columns of a 4-wave and the 128 of an 8-wave workgroup: 63 / 64 / 65 and 127 / 128 / 129
# need an odd product, hence the few cases with b = 1 or 3 (every other case has two clouds with different index tables).
I = InterCase
INTER_CASES = [
    # ks = 24: the 8-wave kernels, every (NT, MT) of the forward pass and every (NT, MO) of the weight gradient
    I("k24_n1_16", 1, 24, 16, 16, 60, 2, 3),            # fwd8<1,1>; cout = 16 is refused by the 8-wave weight gradient
    I("k24_n15_32", 15, 24, 32, 32, 60, 2, 2),
    I("k24_n16_64_c64", 16, 24, 16, 64, 16, 2, 2),      # 64 columns
    I("k24_n16_128", 16, 24, 48, 128, 24, 2, 3),
    I("k24_n15_256", 15, 24, 16, 256, 60, 2, 1),        # p2 = 1; two output-channel blocks
    I("k24_n17_16_c63", 17, 24, 16, 16, 21, 3, 1),      # 63 columns
    I("k24_n32_32_c128", 32, 24, 16, 32, 16, 2, 4),     # 128 columns
    I("k24_n17_64_c129", 17, 24, 32, 64, 43, 3, 1),     # 129 columns
    I("k24_n32_128_c65", 32, 24, 16, 128, 65, 1, 1),    # 65 columns
    I("k24_n32_256", 32, 24, 16, 256, 60, 2, 2),
    I("k24_n16_48", 16, 24, 16, 48, 60, 2, 3),          # cout = 48, 80: the 4-wave kernels at nn <= 32
    I("k24_n32_80", 32, 24, 16, 80, 60, 2, 2),
    I("k24_n33_64", 33, 24, 16, 64, 60, 2, 3),          # nn > 32 leaves the 8-wave kernels
    I("k24_n64_32_c127", 64, 24, 16, 32, 127, 1, 1),    # 127 columns
    I("k24_n65_16", 65, 24, 16, 16, 60, 2, 2),
    I("k24_n128_48_a12", 128, 24, 16, 48, 12, 2, 3),    # na < 16: neighbourhoods re-derived per column
    # ks <= 16: KT = 1
    I("k4_n1", 1, 4, 16, 16, 60, 2, 2),
    I("k12_n17", 17, 12, 32, 48, 60, 2, 3),
    I("k16_n33", 33, 16, 16, 80, 16, 2, 2),
    I("k12_n65_a12", 65, 12, 16, 32, 12, 2, 2),
    I("k16_n16", 16, 16, 16, 64, 60, 2, 2),             # bwd_data8<1,1,8>
    I("k16_n32", 32, 16, 48, 16, 24, 2, 2),             # bwd_data8<2,1,8>
    # ks = 20, 28: second kernel-point tile of 4 and 12; the 8-wave data gradient refuses them
    I("k20_n15", 15, 20, 16, 32, 60, 2, 2),
    I("k28_n17", 17, 28, 32, 64, 60, 2, 3),
    I("k28_n33_256", 33, 28, 16, 256, 16, 2, 2),
    I("k28_n33_192", 33, 28, 16, 192, 16, 2, 2),        # the 4-wave forward asked for 164 KB of LDS here (CHANGELOG)
    I("k20_n65", 65, 20, 16, 128, 60, 2, 1),
    # ks = 32: MH = 16 and the unpadded 4-wave data gradient
    I("k32_n16", 16, 32, 16, 16, 60, 2, 2),
    I("k32_n17", 17, 32, 32, 128, 16, 2, 2),
    I("k32_n15_a12", 15, 32, 16, 48, 12, 2, 3),
    I("k32_n32_a12", 32, 32, 16, 80, 12, 2, 2),
    I("k32_n33_256", 33, 32, 16, 256, 60, 2, 1),
    I("k32_n65", 65, 32, 16, 64, 16, 2, 2),
    # cin = 256 in every pass; the weight gradient with col_tiles_per_wg = 2 and a short last workgroup (8-wave: 17 tiles of
    # 128 columns over 16 splits; 4-wave: 35 tiles of 64 over 32)
    I("c256_all", 16, 24, 256, 16, 16, 2, 1),
    I("dw_tiles8", 16, 24, 256, 256, 24, 2, 45, ("bwd_weight",)),
    I("dw_tiles4", 33, 24, 256, 256, 24, 2, 46, ("bwd_weight",)),
]
J = IntraCase
INTRA_CASES = [
    J("kn1_16", 1, 16, 16, 60),
    J("kn4_64_pt", 4, 64, 64, 60, 2, 1),                # p = 1; 512 threads, waves 4 .. 7 only stage
    J("kn5_48_128", 5, 48, 128, 12),
    J("kn12_128_64_pt", 12, 128, 64, 60),
    J("kn13_64_128_v4", 13, 64, 128, 60, 2, 2),
    J("kn1_256_64_v4", 1, 256, 64, 12),
    J("kn12_64_256_pt_a12", 12, 64, 256, 12, 2, 5),
    J("kn13_16_48", 13, 16, 48, 60, 2, 1),
    J("kn4_256_256_pt", 4, 256, 256, 60, 2, 1),
    J("kn5_128_16", 5, 128, 16, 60, 2, 2),
    # 143 column tiles over fewer splits: col_tiles_per_wg > 1, short last workgroup
    J("kn13_128_128_v4_tiles", 13, 128, 128, 60, 2, 19),
    J("kn13_48_128_tiles", 13, 48, 128, 60, 2, 19),
    J("kn1_256_256_v4_tiles", 1, 256, 256, 60, 2, 19),  # single neighbour: the four waves split the tiles
    # 39 points over 32 workgroups per (o, c) block: the point-tile kernel's double-buffered loop walks two points, the last
    # workgroup one
    J("kn4_256_256_pt_points", 4, 256, 256, 60, 3, 13),
]

# Grouping and its transposes: the smallest shapes at which the launchers' choice can go wrong, one per reachable instance and
# edge.  Two clouds of p1 = 6 points; ks = 12 takes the lower side of every neighbour-count edge (16 | 17, 32 | 33, 64 | 65),
# ks = 24 the upper one (and 128); cin = 16 / 32 / 64 = narrow grouping and one chunk per scatter step / CG = 2 and two chunks /
# CG = 4 and four; p2 = 16, 8, 4 are the scatter's group sizes and 3 is a multiple of none (per-slot atomic scatter, slot-slab
# deterministic form); na = 12 is refused by the wide grouping, the packed order and the deterministic entry.
def _group_cases():
    out = []
    for ks, (n1, n2, n4, n8) in ((12, (16, 17, 33, 65)), (24, (16, 32, 64, 128))):
        for nn, cin, na, p2 in (
                (n1, 16, 60, 8), (n1, 32, 60, 3), (n1, 64, 60, 8), (n1, 32, 12, 8),
                (n2, 64, 60, 16), (n2, 64, 60, 8), (n2, 32, 60, 16), (n2, 16, 60, 16), (n2, 16, 60, 8), (n2, 32, 60, 3),
                (n2, 64, 12, 16),
                (n4, 32, 60, 8), (n4, 16, 60, 8), (n4, 64, 60, 4), (n4, 16, 60, 3),
                (n8, 16, 60, 4), (n8, 16, 60, 3), (n8, 32, 60, 2)):
            out.append(GroupCase(f"k{ks}_n{nn}_c{cin}_a{na}_p{p2}", nn, ks, cin, na, p2))
    return out


GROUP_CASES = _group_cases()
# both sides of INV_LDS_ENT (entries of a cloud) and of INV_LDS_P1 (points of a cloud); one cloud is enough for the large ones
INV_CASES = [InvCase("small", 2, 6, 3, 16), InvCase("ent_32768", 1, 300, 256, 128), InvCase("ent_32896", 1, 300, 257, 128),
             InvCase("p1_4096", 2, 4096, 5, 16), InvCase("p1_4097", 2, 4097, 5, 16)]

# Real-geometry tier: (name, schedule, layer, cin, cout, points per cloud) -- nn, stride, radius and sigma are the layer's: the
# first layer of the classification schedule (nn = 32: the 8-wave kernels) and a K = 64 layer of the rotation-estimation one
REAL_INTER = [("cls_first_layer", "cls", 0, 16, 32, 64), ("reg_K64_layer", "reg", 2, 16, 48, 80)]
REAL_INTRA = [IntraCase("real_gemm_plain", 12, 16, 48, 60, 2, 3), IntraCase("real_v4", 13, 64, 64, 60, 2, 3),
              IntraCase("real_pt", 12, 64, 128, 60, 2, 3)]
# |kernel - fp64| <= REAL_M 2^-24 S element by element (S: conv_ref.inter_abs_sums(expanded=True)).  REAL_M is twice the worst
# such ratio of the CPU fp32 oracle (oracle/so3conv_ref.py, direct form, torch's summation order) over the real-geometry cases,
# rounded up to a power of two; tests/test_conv_spec.py re-measures the oracle and fails if this constant is not that.
REAL_M = 0.5


# ------------------------------------------------------------------------------------------------ builders
def real_inter_case(entry):
    """A real-geometry case on the host (needs the package and the CPU oracle, not a device): icosahedral anchors, the 24 shipped
    kernel points scaled as the module scales them, a unit-ball cloud, nn, stride, radius and sigma of the named layer of the
    named schedule.  Returns (InterCase, dict of arrays at the C boundary)."""
    import torch
    from conftest import unit_ball_cloud
    from epn_pointcloud_amd import schedule
    from epn_pointcloud_amd.vgtk import functional as fr
    from epn_pointcloud_amd.vgtk.so3conv import functional as L
    from oracle import so3conv_ref as O
    name, sched, layer, cin, cout, n = entry
    lay = {"cls": schedule.cls_so3net_schedule, "reg": schedule.reg_so3net_schedule}[sched]()[layer]
    nn, stride = lay.nn, lay.stride
    rng = np.random.default_rng(hash_name(name))
    # (the schedule's radius belongs to 1024-point clouds; the small cloud is scaled so that a ball holds about nn / 2 points)
    scale = lay.radius * (n / (0.5 * nn)) ** (1.0 / 3.0)
    xyz = torch.from_numpy(unit_ball_cloud(rng, 2, n, scale=scale))
    anchors = torch.from_numpy(np.asarray(L.get_anchors(60), dtype=np.float32))
    kernels = O.scaled_kernel_points(torch.from_numpy(np.asarray(fr.kernel_points_raw(24), dtype=np.float32)), lay.radius)
    grouped, idx, sidx, new_xyz = O.inter_grouping_ball(xyz, stride, lay.radius, nn, lazy_sample=True)
    g = torch.Generator().manual_seed(hash_name(name))
    F = torch.randn(2, n, 60, cin, generator=g)
    W = torch.randn(cout, cin * 24, generator=g) / (cin * 24) ** 0.5
    gOut = torch.randn(2, new_xyz.shape[2], 60, cout, generator=g)
    c = InterCase(name, nn, 24, cin, cout, 60, 2, new_xyz.shape[2], PASSES, float(lay.sigma), n)
    d = dict(xyz=xyz.numpy(), new_xyz=new_xyz.contiguous().numpy(), idx=idx.int().numpy(), anchors=anchors.numpy(),
             kernels=kernels.numpy(), sigma=float(lay.sigma), F=F.numpy(), W=W.numpy(), gOut=gOut.numpy())
    return c, d


def real_inter_reference(entry):
    """(case, arrays, float64 reference, S) of a real-geometry case; S: inter_abs_sums of the expanded form."""
    if ("real", entry) not in _CACHE:
        c, d = real_inter_case(entry)
        geo = (d["xyz"], d["new_xyz"], d["idx"], d["anchors"], d["kernels"], np.float32(d["sigma"]))
        _CACHE[("real", entry)] = (c, d, R.inter_conv(*geo, d["F"], d["W"], d["gOut"]),
                                   R.inter_abs_sums(*geo, d["F"], d["W"], d["gOut"], expanded=True))
    return _CACHE[("real", entry)]


def _rotations24():
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            m = np.zeros((3, 3))
            for r in range(3):
                m[r, perm[r]] = signs[r]
            if round(np.linalg.det(m)) == 1:
                out.append(m)
    assert len(out) == 24
    return np.stack(out)


def _ints(rng, shape, q):
    """Integers in [-q, q], no zeros (a zero operand would hide a slot), as float32."""
    v = rng.integers(1, q + 1, size=shape) * (1 - 2 * rng.integers(0, 2, size=shape))
    return v.astype(np.float32)


def _index_table(rng, c):
    """[b, p2, nn] indices into 0 .. p1 (p1 = shadow), about one slot in six shadow, the two clouds drawn independently.  Every
    ordinary row references point 1 of its cloud (the heaviest atomic target of the data gradient).  With six rows or more, special rows:
    cloud 0: shadow in the first and last slot / one point repeated / indices 0 and p1 - 1 only;
    cloud 1: all shadow / the ball query's cyclic padding (cnt distinct hits repeated: the data gradient's `mul` path)."""
    p1, nn = c.p1, c.nn
    idx = rng.integers(0, p1, size=(c.b, c.p2, nn))
    idx = np.where(rng.random(idx.shape) < 1 / 6, p1, idx)
    if nn >= 2:
        slot = rng.integers(0, nn, size=(c.b, c.p2))
        np.put_along_axis(idx, slot[..., None], 1, axis=2)
    if c.b * c.p2 >= 6:
        idx[0, 0, 0] = idx[0, 0, -1] = p1
        idx[0, 1, :] = np.where(np.arange(nn) % 2 == 0, 3, idx[0, 1, :])
        idx[0, 2, :] = np.where(np.arange(nn) % 2 == 0, 0, p1 - 1)
        idx[1, 0, :] = p1
        cnt = max(1, min(5, nn // 3))
        idx[1, 1, :] = (np.arange(nn) % cnt) + 1
    dead = (idx == p1).all(axis=(0, 1))                  # a slot that is shadow in every row would never be exercised
    idx[-1, -1, dead] = rng.integers(0, p1, size=int(dead.sum()))
    return idx.astype(np.int32)


def build_inter(c, seed=None):
    """The dyadic case: dict of float32 / int32 arrays at the C boundary, the float64 reference `ref`, the operand magnitude `q`
    (the largest of 3, 2, 1 whose sums of absolute values stay below 2^24 last-bit units = 2^20) and `bits` (those sums / 2^24).
    Deterministic in the case's name."""
    rng = np.random.default_rng(abs(hash_name(c.name)) if seed is None else seed)
    rot = _rotations24()
    anchors = rot[np.arange(c.na) % 24].astype(np.float32)
    eighth = lambda shape, m: (rng.integers(-m, m + 1, size=shape) / 8.0).astype(np.float32)
    kernels = eighth((c.ks, 3), 2)
    xyz, new_xyz = eighth((c.b, 3, c.p1), 2), eighth((c.b, 3, c.p2), 2)
    idx = _index_table(rng, c)
    shapes = dict(F=(c.b, c.p1, c.na, c.cin), W=(c.cout, c.cin * c.ks), gOut=(c.b, c.p2, c.na, c.cout))
    unit = {k: _ints(rng, s, 1) for k, s in shapes.items()}
    mag = {k: rng.integers(1, 4, size=s) for k, s in shapes.items()}
    geo = (xyz, new_xyz, idx, anchors, kernels, c.sigma)
    # every |term| grows at most with q^2: one evaluation at q = 1 picks q, the evaluation at that q is the proof
    want = tuple(OUTPUT[p] for p in c.passes)
    first = R.inter_abs_sums(*geo, unit["F"], unit["W"], unit["gOut"], want=want)
    bits1 = max(float(v.max()) for v in first.values()) * 16.0 / 2.0 ** 24               # w is a multiple of 1/16
    q = 3 if 9 * bits1 < 1.0 else 2 if 4 * bits1 < 1.0 else 1
    ops = {k: unit[k] * np.minimum(mag[k], q).astype(np.float32) for k in shapes}
    sums = first if q == 1 else R.inter_abs_sums(*geo, ops["F"], ops["W"], ops["gOut"], want=want)
    bits = {k: float(v.max()) * 16.0 / 2.0 ** 24 for k, v in sums.items()}
    assert max(bits.values()) < 1.0, (c, bits)
    ref = R.inter_conv(*geo, ops["F"], ops["W"], ops["gOut"], want=want)
    for k in ("w", "G") + want:
        assert np.array_equal(ref[k] * 16.0, np.round(ref[k] * 16.0)), (c, k)             # multiples of 1/16
    return dict(xyz=xyz, new_xyz=new_xyz, idx=idx, anchors=anchors, kernels=kernels, sigma=c.sigma, ref=ref, q=q, bits=bits,
                **ops)


def _bf16(v):
    """float32 values rounded to the nearest bf16 (ties to even), so that one operand serves the fp32 and the bf16 entries."""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def build_group(c):
    """A grouping case: the dyadic geometry of build_inter (the weights are then the same float in every form), features F and a
    grouped gradient dG of bf16-representable normal deviates, and the float64 G = group(F), dF = ungroup(dG)."""
    rng = np.random.default_rng(hash_name(c.name))
    anchors = _rotations24()[np.arange(c.na) % 24].astype(np.float32)
    eighth = lambda shape, m: (rng.integers(-m, m + 1, size=shape) / 8.0).astype(np.float32)
    kernels = eighth((c.ks, 3), 2)
    xyz, new_xyz = eighth((c.b, 3, c.p1), 2), eighth((c.b, 3, c.p2), 2)
    idx = _index_table(rng, c)
    F = _bf16(rng.standard_normal((c.b, c.p1, c.na, c.cin)))
    dG = _bf16(rng.standard_normal((c.b * c.p2 * c.na, c.cin * c.ks)))
    geo = (xyz, new_xyz, idx, anchors, kernels, c.sigma)
    return dict(xyz=xyz, new_xyz=new_xyz, idx=idx, anchors=anchors, kernels=kernels, sigma=c.sigma, F=F, dG=dG,
                G=R.inter_group(*geo, F), dF=R.inter_ungroup(*geo, dG, c.cin))


def build_inverse(c):
    """An index table [b, p2, nn] with indices up to p1 + 2 (p1 and beyond: shadow) and one point named by a whole row."""
    rng = np.random.default_rng(hash_name(c.name))
    idx = rng.integers(0, c.p1 + 3, size=(c.b, c.p2, c.nn)).astype(np.int32)
    idx[0, 0, :] = c.p1 - 1
    off, ent = R.inverse_list(idx, c.p1)
    return dict(idx=idx, off=off, ent=ent)


def build_intra(c):
    rng = np.random.default_rng(abs(hash_name(c.name)))
    idx = np.stack([rng.permutation(c.na) for _ in range(c.kn)], axis=1).astype(np.int32)
    shapes = dict(F=(c.b, c.p, c.na, c.cin), W=(c.cout, c.cin * c.kn), gOut=(c.b, c.p, c.na, c.cout))
    q = 3
    ops = {k: _ints(rng, s, q) for k, s in shapes.items()}
    ncol = c.b * c.p * c.na
    bits = q * q * max(c.cin * c.kn, c.cout * c.kn, ncol) / 2.0 ** 24                     # every |term| <= q^2
    assert bits < 1.0, c
    ref = R.intra_conv(ops["F"], ops["W"], idx, ops["gOut"])
    return dict(idx=idx, inv=R.inverse_intra_idx(idx), ref=ref, q=q, bits=bits, **ops)


def hash_name(name):
    """A seed from the case's name that does not depend on PYTHONHASHSEED."""
    h = 2166136261
    for ch in name.encode():
        h = ((h ^ ch) * 16777619) & 0xFFFFFFFF
    return h


def inter_case(c):
    if c not in _CACHE:
        _CACHE[c] = build_inter(c)
    return _CACHE[c]


def intra_case(c):
    if c not in _CACHE:
        _CACHE[c] = build_intra(c)
    return _CACHE[c]


def group_case(c):
    if c not in _CACHE:
        _CACHE[c] = build_group(c) if isinstance(c, GroupCase) else build_inverse(c)
    return _CACHE[c]
