"""Case tables of tests/test_gpu_gemm_exact.py, the exactness condition they stand on, and a Python restatement of the GEMM
dispatch tables (csrc/gemm.hip launch_nt_typed / nt_choose, csrc/gemm_x3.hip gemm_nt_x3_ok / x3_choose, csrc/gemm_tn.hip gemm_tn_tile /
gemm_tn_splits / tn_fast_ok / tn_plan) that says which kernel instance a case must reach.  tests/test_gemm_spec.py checks on the
CPU that every case is in the exact regime, that the restated split counts agree with the library's workspace queries, and that
the cases reach every instance listed in REACHABLE; the GPU file asserts per call that the library ran the predicted instance.

Exactness: integers in [-q, q] are exact in every piece format (bf16: 8 bits, fp16 high piece: 11 bits under any power-of-two
scale); with q^2 L < 2^24 for the contraction length L every product and every partial sum in ANY order is an integer below
2^24, hence exact in fp32.  Column statistics (sum of squares of 32 outputs): 32 (q^2 K)^2 < 2^24.

Nothing here needs a device."""
import re
from collections import namedtuple

NT_FORMS = ("native", "split", "f16x2", "bf16", "bf16f32")      # bf16: bf16 in / bf16 out; bf16f32: bf16 in / fp32 out
TN_MODES = ("native", "split", "f16x2", "bf16")
Q_NT, Q_TN, Q_STATS = 64, 8, 3
GEMM_MAX_PROB = 6


def e16_of(form):
    return 8 if form.startswith("bf16") else 4


# ------------------------------------------------------------------------------------------------ NT
# M, N, K; operand / output placement: ld* = leading dimension (0: dense), *0 = first column inside the wider tensor, *sh =
# elements the buffer is shifted from an aligned address; stats / amax: the epilogues; q: range of the integers
NtCase = namedtuple("NtCase", "M N K lda a0 ash ldb b0 bsh ldc c0 stats amax q", defaults=(0, 0, 0, 0, 0, 0, 0, 0, False, False, Q_NT))


def nt_lds(c):
    """(lda, ldb, ldc) as gemm.py hands them to the library: a one-row operand is passed with its width."""
    lda = c.lda or c.K
    ldb = c.ldb or c.K
    ldc = c.ldc or c.N
    return (c.K if c.M <= 1 else lda), (c.K if c.N <= 1 else ldb), (c.N if c.M <= 1 else ldc)


def nt_exact(c):
    assert c.q * c.q * c.K < 2 ** 24, c
    if c.stats:
        assert c.M % 32 == 0 and c.M > 0 and 32 * (c.q * c.q * c.K) ** 2 < 2 ** 24, c
    return True


def _nt_name(t, to, cfg):
    return "gemm_nt_kernel<%s,%s,%s>" % (t, to, ",".join(map(str, cfg)))


def _nt_native(form, chunk):
    """launch_nt_typed for one launch (<= 6 problems)."""
    e16 = e16_of(form)
    t = "float" if e16 == 4 else "bf16"
    to = "bf16" if form == "bf16" else "float"
    fast, half_k = True, False
    for c in chunk:
        lda, ldb, _ = nt_lds(c)
        if c.K % (4 * e16) or lda % e16 or ldb % e16 or (c.a0 + c.ash) % e16 or (c.b0 + c.bsh) % e16:
            fast = False
        if c.K % (8 * e16):
            half_k = True
    maxn, minn = max(c.N for c in chunk), min(c.N for c in chunk)
    if not fast:
        return "gemm_nt_generic_kernel<%s,%s>" % (t, to)
    if half_k:
        return _nt_name(t, to, (8, 1, 2, 1, 4, 2) if maxn <= 32 else ((8, 1, 2, 2, 4, 2) if maxn <= 64 else (4, 2, 2, 2, 4, 2)))
    if e16 == 4 and len(chunk) == 1 and maxn in (128, 256) and (chunk[0].M // 128) * (maxn // 128) >= 3840:
        return _nt_name(t, to, (2, 2, 2, 2, 8, 2))
    if e16 == 4 and len(chunk) > 1:
        return _nt_name(t, to, (4, 1, 2, 2, 8, 2) if maxn <= 320 and minn <= 64 else (2, 2, 2, 2, 8, 2))
    if maxn <= 32:
        return _nt_name(t, to, (8, 1, 2, 1, 8, 2))
    if maxn <= 64:
        return _nt_name(t, to, (8, 1, 2, 2, 8, 2))
    if minn >= 256:
        return _nt_name(t, to, (4, 2, 2, 4, 8, 2))
    return _nt_name(t, to, (4, 2, 2, 2, 8, 3) if e16 == 8 else (4, 2, 2, 2, 8, 2))


def nt_x3_ok(chunk):
    """gemm_nt_x3_ok: ldb and the alignment of Bt are NOT conditions (the weight split reads Bt element-wise)."""
    for c in chunk:
        lda, _, _ = nt_lds(c)
        if c.M < 1 or c.K < 32 or c.K % 32 or lda % 4 or (c.a0 + c.ash) % 4:
            return False
    return True


def _nt_x3(npl, chunk):
    maxn, minn = max(c.N for c in chunk), min(c.N for c in chunk)
    nstg64 = 2 if npl == 2 else 3
    name = lambda cfg: "gemm_nt_x3_kernel<%s,%d>" % (",".join(map(str, cfg)), npl)
    if len(chunk) > 1:
        if maxn <= 320 and minn <= 64:
            return name((4, 1, 2, 2, nstg64))
        return name((4, 2, 2, 4, 2)) if minn >= 256 else name((2, 2, 2, 2, 2))
    if maxn <= 32:
        return name((8, 1, 2, 1, 2))
    if maxn <= 64:
        return name((4, 1, 2, 2, nstg64))
    if npl == 2 and maxn <= 128:
        return name((2, 2, 2, 2, 2))
    if maxn <= 128 or maxn % 256 > 128 or (maxn % 256 and maxn < 512):
        return name((4, 2, 2, 2, 2))
    return name((4, 2, 2, 4, 2))


def nt_instance(form, cases):
    """The main kernel epn_last_kernel() names after a (grouped) NT call: that of the LAST launch (nt_entry launches six
    problems at a time; a launch whose problems all have M == 0 launches nothing)."""
    last = None
    for i0 in range(0, len(cases), GEMM_MAX_PROB):
        chunk = cases[i0:i0 + GEMM_MAX_PROB]
        if all(c.M == 0 for c in chunk):
            continue
        if form in ("split", "f16x2") and nt_x3_ok(chunk):
            last = _nt_x3(3 if form == "split" else 2, chunk)
        else:
            last = _nt_native(form, chunk)
    return last


def nt_block(inst):
    """(BM, BN) of an NT MFMA instance name; None for the generic kernel."""
    if "generic" in inst:
        return None
    a = inst[inst.index("<") + 1:-1].split(",")
    a = [int(v) for v in a if v.lstrip("-").isdigit()]
    return a[0] * a[2] * 32, a[1] * a[3] * 32


NT_N = (1, 31, 32, 33, 64, 65, 127, 128, 129, 255, 256, 257, 320, 576)
NT_K = {"native": (16, 48, 32, 64, 96), "split": (16, 48, 32, 64, 96), "f16x2": (16, 48, 32, 64, 96),
        "bf16": (32, 96, 64, 128, 192, 256), "bf16f32": (32, 96, 64, 128, 192, 256)}
NT_K_GENERIC = (1, 4, 20, 40)


def nt_single_cases(form):
    """Every (N, K) of the grids twice, the row counts {1, 31, 33, BM - 1, BM + 1, BM, 2 BM} of the instance the pair reaches
    dealt round robin PER INSTANCE (so every instance sees each of them), c_amax on every other case; then the generic K."""
    out, turn = [], {}
    for n in NT_N:
        for k in NT_K[form]:
            inst = nt_instance(form, [NtCase(64, n, k)])
            bm = nt_block(inst)[0]
            ms = (1, 31, 33, bm - 1, bm + 1, bm, 2 * bm)
            for _ in range(2):
                i = turn.get(inst, 0)
                turn[inst] = i + 1
                out.append(NtCase(ms[i % len(ms)], n, k, amax=bool(i & 1)))
    for j, k in enumerate(NT_K_GENERIC):
        for i, n in enumerate((1, 33, 130)):
            out.append(NtCase((1, 33, 257)[(i + j) % 3], n, k, amax=bool((i + j) & 1)))
    return out


def nt_layout_cases(form):
    """Strides and alignment on two shapes: A / Bt as column slices of wider tensors, outputs into column slices, leading
    dimensions that are no multiple of the 16-byte element count, operands one element past an aligned address."""
    out = []
    for m, n, k in ((300, 130, 64), (70, 40, 32), (257, 257, 96 if not form.startswith("bf16") else 128)):
        out += [NtCase(m, n, k, lda=k + 4, a0=4), NtCase(m, n, k, lda=k + 32), NtCase(m, n, k, lda=k + 32, a0=8, amax=True),
                NtCase(m, n, k, ldb=k + 4), NtCase(m, n, k, ldb=k + 32, b0=16), NtCase(m, n, k, ldc=n + 4, c0=2, amax=True),
                NtCase(m, n, k, ldc=n + 1, c0=1), NtCase(m, n, k, lda=k + 1), NtCase(m, n, k, lda=k + 2, a0=2),
                NtCase(m, n, k, ldb=k + 1, amax=True), NtCase(m, n, k, ldb=k + 2, b0=1), NtCase(m, n, k, lda=k + 4, ash=1),
                NtCase(m, n, k, ldb=k + 4, bsh=1), NtCase(m, n, k, lda=k + 32, a0=8, ldb=k + 8, b0=8, ldc=n + 4, c0=3)]
    return out


def nt_stats_cases(form):
    """col_stats (+ c_amax): M % 32 == 0 with a ragged last row tile, ragged N, both K-step widths, the generic kernel."""
    ks = (32, 64) if form.startswith("bf16") else (16, 32, 64)
    out = []
    for i, n in enumerate((1, 31, 33, 64, 65, 129, 256, 257, 320)):
        k = ks[i % len(ks)]
        bm = nt_block(nt_instance(form, [NtCase(64, n, k)]))[0]
        for m in (32, bm + 32, 2 * bm):
            out.append(NtCase(m, n, k, stats=True, amax=True, q=Q_STATS))
    out += [NtCase(96, 33, 20, stats=True, amax=True, q=Q_STATS), NtCase(64, 130, 40, stats=True, amax=True, q=Q_STATS),
            NtCase(160, 40, 32, lda=33, stats=True, amax=True, q=Q_STATS)]
    return out


MANY_TILE = NtCase(245760, 256, 32)         # native fp32 only: the smallest M with (M / 128) (N / 128) >= 3840


def _g(*mnk, **kw):
    return [NtCase(m, n, k, **kw) for m, n, k in mnk]


def nt_group_cases(form):
    """name -> (problems, per-problem flags 'a' = a_amax given, 'c' = c_amax, 's' = col_stats).  K ascends inside every group
    (the launcher sorts by K, longest first); the tile counts are no multiples of 8."""
    k1, k2, k3, k4 = (64, 128, 192, 256) if form.startswith("bf16") else (32, 64, 96, 128)
    hk = 32 if form.startswith("bf16") else 16              # a K only the half-K-step instances take
    ks = (32, 32, 64, 64, 64)                               # col_stats stay exact up to K = 64
    g = {
        "two_narrow": (_g((300, 64, k1), (513, 192, k2)), ("c", "a")),
        "five_spectral": (_g((70, 32, k1), (210, 96, k2), (200, 96, k2), (257, 128, k3), (330, 160, k4)), ("a", "", "c", "ac", "")),
        "six_m0_middle": (_g((130, 96, k1), (257, 128, k1), (0, 130, k2), (129, 200, k2), (300, 384, k3), (31, 100, k4)),
                          ("", "c", "c", "a", "", "ac")),
        "six_rest": (_g((130, 96, k1), (257, 128, k1), (1, 130, k2), (129, 200, k2), (300, 384, k3), (31, 100, k4)),
                     ("a", "c", "", "a", "c", "")),
        "three_wide": (_g((300, 256, k1), (257, 320, k2), (33, 257, k3)), ("", "ac", "")),
        "seven": (_g((70, 32, k1), (210, 96, k1), (200, 96, k2), (257, 128, k2), (330, 160, k3), (40, 64, k4), (513, 130, k2)),
                  ("", "c", "", "", "a", "", "c")),
        "thirteen": (_g(*[(30 + 41 * i, (24, 64, 130, 257, 96)[i % 5], (k1, k1, k2, k2, k3, k3)[i % 6]) for i in range(13)]),
                     tuple(("", "c", "a")[i % 3] for i in range(13))),
        "half_k_member": (_g((70, 32, hk), (210, 96, k1), (200, 96, k2), (257, 128, k3), (330, 160, k4)), ("", "c", "", "a", "")),
        "three_m0_narrow": (_g((300, 64, k1), (0, 96, k1), (513, 192, k2)), ("c", "", "a")),
        "stats_mixed": ([NtCase(m, n, k, q=Q_STATS, stats=s) for (m, n, s), k in
                         zip(((64, 32, True), (70, 96, False), (288, 96, True), (257, 33, False), (544, 160, True)), ks)],
                        ("sa", "c", "sc", "", "s")),
    }
    return g


def nt_all_instances(form):
    """Instances the module's NT cases of `form` are predicted to reach."""
    got = {nt_instance(form, [c]) for c in nt_single_cases(form) + nt_layout_cases(form) + nt_stats_cases(form)}
    got |= {nt_instance(form, probs) for probs, _ in nt_group_cases(form).values()}
    if form == "native":
        got.add(nt_instance(form, [MANY_TILE]))
    return got


# ------------------------------------------------------------------------------------------------ TN
TnCase = namedtuple("TnCase", "R N1 N2 ldx x0 xsh ldy y0 ysh ldc c0", defaults=(0, 0, 0, 0, 0, 0, 0, 0))
TN_MODE_ID = {"native": 0, "bf16": 1, "split": 2, "f16x2": 3}       # the `bf16` argument of the workspace queries
TN_F32_BR = {(32, 512): (1, 8, 1, 2, 32), (64, 64): (2, 2, 1, 1, 32), (64, 128): (2, 2, 1, 2, 32), (64, 256): (1, 8, 2, 1, 32),
             (64, 512): (1, 4, 2, 4, 16), (128, 64): (2, 2, 2, 1, 32), (128, 128): (2, 2, 2, 2, 32), (128, 256): (2, 4, 2, 2, 32),
             (128, 512): (1, 8, 4, 2, 32)}
TN_PLANES_BR = {(32, 512): (1, 8, 1, 2, 32), (64, 512): (1, 8, 2, 2, 16), (128, 256): (2, 4, 2, 2, 32), (128, 512): (1, 8, 4, 2, 16),
                (256, 256): (2, 4, 4, 2, 16)}
TN_BF16 = {(32, 256): (1, 4, 2, 4), (64, 256): (1, 4, 4, 4), (128, 256): (2, 2, 4, 8)}


def tn_exact(c):
    assert Q_TN * Q_TN * c.R < 2 ** 24 and c.R <= 131072 and max(c.N1, c.N2) <= 1280, c
    return True


def tn_lds(c):
    return ((c.ldx or c.N1) if c.R > 1 else c.N1), ((c.ldy or c.N2) if c.R > 1 else c.N2), ((c.ldc or c.N2) if c.N1 > 1 else c.N2)


def tn_fast_ok(mode, c):
    e16 = 8 if mode == "bf16" else 4
    ldx, ldy, _ = tn_lds(c)
    return (c.R > 0 and c.R % 32 == 0 and c.N1 >= e16 and c.N2 >= e16 and ldx % e16 == 0 and ldy % e16 == 0 and
            (c.x0 + c.xsh) % e16 == 0 and (c.y0 + c.ysh) % e16 == 0 and c.N1 % e16 == 0 and c.N2 % e16 == 0)


def tn_tile(dtype, n1, n2):
    """gemm_tn_tile; dtype 0 fp32, 1 bf16, 2 the split forms."""
    if dtype == 1:
        if n2 <= 128:
            bn2 = 32 if n2 <= 32 else (64 if n2 <= 64 else 128)
            bn1 = 32 if n1 <= 32 else (64 if n1 <= 64 else (128 if n1 <= 128 else 256))
            return (64 if bn2 == 32 and bn1 > 64 else bn1), bn2
        return (32 if n1 <= 32 else (64 if n1 <= 64 else 128)), 256
    if dtype == 2 and n2 >= 512:
        return (32, 512) if n1 <= 32 else ((64, 512) if n1 <= 64 else ((256, 256) if n1 >= 256 else (128, 512)))
    if n1 <= 32 and n2 > 128:
        return 32, 512
    bn2 = 512 if n2 >= 512 else (256 if n2 > 128 else (128 if n2 > 64 else 64))
    return (64 if n1 <= 64 else 128), bn2


def tn_splits(dtype, r, n1, n2):
    """gemm_tn_splits of the default build."""
    bn1, bn2 = tn_tile(dtype, n1, n2)
    tiles = -(-n1 // bn1) * -(-n2 // bn2)
    chunks = r // 32
    if dtype == 1 and n2 <= 128:
        return max(1, min(256 // tiles, max(chunks // 16, 1)))
    return max(1, min(512 // tiles, max(chunks // 32, 1), 512))


def _al256(n):
    return (n + 255) // 256 * 256


def tn_workspace(mode, c):
    """epn_gemm_tn_workspace_bytes restated from the split count: partial slabs + planes of X + the two maxima."""
    d = {"native": 0, "bf16": 1}.get(mode, 2)
    s = tn_splits(d, c.R, c.N1, c.N2)
    planes = _al256((4 if mode == "f16x2" else 6) * c.R * c.N1) if d == 2 and c.N2 >= 512 else 0
    return (_al256(s * c.N1 * c.N2 * 4) if s > 1 else 0) + planes + (256 if mode == "f16x2" else 0)


def tn_ring_kr(tm, tn):
    step_b = 32 * 2 * 16 * (2 * tm + 2 * tn)
    kr = 1
    while 2 * kr * step_b <= 32 * 1024 and 2 * kr * step_b * 4 <= 160 * 1024:
        kr *= 2
    return kr


def tn_instance(mode, cases):
    """The main kernel of a (grouped) TN call: tn_plan's tile and family, or the generic kernel."""
    if not all(tn_fast_ok(mode, c) for c in cases):
        return "gemm_tn_generic_kernel<%s>" % ("bf16" if mode == "bf16" else "float")
    x3 = {"split": 3, "f16x2": 2}.get(mode, 0)
    bf = 1 if mode == "bf16" else (2 if x3 else 0)
    nprob = len(cases)
    max1, min1 = max(c.N1 for c in cases), min(c.N1 for c in cases)
    min2 = min(c.N2 for c in cases)
    group_planes = 256 if x3 == 2 else 512
    bn1, bn2 = tn_tile(0 if nprob > 1 and bf == 2 else bf, max1, 256 if nprob > 1 and min2 < 256 else min2)
    if nprob > 1 and bf == 2 and min2 >= group_planes and min1 >= 256:
        bn1, bn2 = 256, 256
    if nprob > 1 and x3 == 2 and min2 < 256:
        bn1, bn2 = 128, 128
    if bf == 1:
        if (bn2 <= 128) if nprob == 1 else (bn1 == 128):
            tm, tn = bn1 // 32, bn2 // 32
            tail = (4, tn_ring_kr(tm, tn)) if bn2 <= 128 else (3, 1)
            return "gemm_tn_bf16_ring_kernel<2,2,%d,%d,%d,%d>" % ((tm, tn) + tail)
        return "gemm_tn_bf16_kernel<%s>" % ",".join(map(str, TN_BF16[(bn1, bn2)]))
    if x3 and (bn1, bn2) in TN_PLANES_BR and min2 >= (512 if nprob == 1 else group_planes):
        return "gemm_tn_x3_kernel<%s,%d>" % (",".join(map(str, TN_PLANES_BR[(bn1, bn2)])), x3)
    return "gemm_tn_f32_kernel<%s,%d>" % (",".join(map(str, TN_F32_BR[(bn1, bn2)])), x3)


TN_W1 = (24, 32, 40, 56, 64, 72, 120, 128, 136, 248, 256, 264)
TN_W2 = TN_W1 + (504, 512, 520)


def tn_width_cases():
    """R = 32 (one chunk, no split): every N1 x N2 one below, at and above the thresholds of gemm_tn_tile."""
    return [TnCase(32, a, b) for a in TN_W1 for b in TN_W2]


# rows: no fast path (1, 31, 33, 100); the first split (2048) and a last split that ends inside a stage (2080); an odd split
# count (3072 -> 3); > 16 slabs (17408 -> 17: the shared-quad reduction with 4 threads per quad; 66560 -> 65: 16 per quad)
TN_ROWS = (1, 31, 33, 100, 2048, 2080, 3072, 17408, 66560)
TN_ROW_SHAPES = ((64, 64), (32, 32), (128, 256), (40, 520), (264, 512), (136, 72))
TN_ROWS_BF16 = (8704, 33280)          # ring form: >= 16 rows steps per split -> 17 and 65 slabs at 64 x 64


def tn_row_cases(mode):
    out = [TnCase(r, a, b) for a, b in TN_ROW_SHAPES for r in TN_ROWS if r <= 17408 or a * b <= 64 * 64]
    if mode == "bf16":
        out += [TnCase(r, 64, 64) for r in TN_ROWS_BF16]
    return out


def tn_layout_cases():
    out = []
    for r, a, b in ((64, 64, 64), (2080, 136, 264), (96, 40, 520)):
        out += [TnCase(r, a, b, ldx=a + 8, x0=8), TnCase(r, a, b, ldx=a + 32), TnCase(r, a, b, ldy=b + 8, y0=8),
                TnCase(r, a, b, ldc=b + 4, c0=2), TnCase(r, a, b, ldc=b + 1, c0=1), TnCase(r, a, b, ldx=a + 1), TnCase(r, a, b, ldy=b + 2, y0=1),
                TnCase(r, a, b, ldx=a + 8, xsh=1), TnCase(r, a, b, ldy=b + 8, ysh=1), TnCase(r, a, b, ldx=a + 16, x0=8, ldy=b + 8, ldc=b + 12, c0=4)]
    # N1 / N2 that are no multiple of the 16-byte element count (fp32: 4, bf16: 8)
    out += [TnCase(64, 30, 64), TnCase(64, 64, 66), TnCase(2048, 36, 68), TnCase(64, 3, 5), TnCase(96, 132, 260)]
    return out


def _t(*rnn):
    return [TnCase(*v) for v in rnn]


TN_GROUPS = {
    "two_narrow": _t((64, 24, 40), (96, 64, 32)),
    "five_spectral": _t((64, 32, 32), (192, 96, 96), (160, 96, 96), (256, 128, 128), (320, 160, 160)),
    "six_thin": _t((32, 16, 256), (64, 32, 264), (96, 24, 512), (128, 32, 320), (160, 8, 256), (2080, 32, 256)),
    "two_256": _t((64, 256, 512), (96, 264, 520)),
    "two_128x512": _t((64, 128, 512), (96, 72, 520)),
    "two_64x512": _t((64, 64, 512), (32, 40, 520)),
    "two_128x256": _t((64, 128, 256), (2080, 136, 264)),
    "two_64x256": _t((64, 64, 256), (96, 40, 264)),
    "five_long": _t((2048, 64, 64), (4160, 72, 128), (96, 128, 136), (8192, 24, 32), (32, 200, 264)),
    "two_unaligned": _t((64, 30, 64), (100, 64, 64)),
}


def tn_all_instances(mode):
    got = {tn_instance(mode, [c]) for c in tn_width_cases() + tn_row_cases(mode) + tn_layout_cases()}
    return got | {tn_instance(mode, g) for g in TN_GROUPS.values()}


# ------------------------------------------------------------------------------------------------ instances of the default build
def _names(fmt, cfgs, *tails):
    return {fmt % (",".join(map(str, c + t))) for c in cfgs for t in tails}


_NT_HALF = ((8, 1, 2, 1, 4, 2), (8, 1, 2, 2, 4, 2), (4, 2, 2, 2, 4, 2))
_NT_FULL = ((8, 1, 2, 1, 8, 2), (8, 1, 2, 2, 8, 2), (4, 2, 2, 4, 8, 2))
_X3 = lambda npl: {"gemm_nt_x3_kernel<%s,%d>" % (",".join(map(str, c)), npl) for c in
                   ((8, 1, 2, 1, 2), (4, 1, 2, 2, 2 if npl == 2 else 3), (2, 2, 2, 2, 2), (4, 2, 2, 2, 2), (4, 2, 2, 4, 2))}
_NT_NATIVE = (_names("gemm_nt_kernel<float,float,%s>", _NT_HALF + _NT_FULL + ((4, 2, 2, 2, 8, 2), (2, 2, 2, 2, 8, 2), (4, 1, 2, 2, 8, 2)), ())
              | {"gemm_nt_generic_kernel<float,float>"})
# the fp32 kernels a split-form call falls back to: K % 32 != 0 (half-K-step instances), a group with one such member or with
# M == 0, lda % 4 / misaligned A (generic)
_NT_FALLBACK = _names("gemm_nt_kernel<float,float,%s>", _NT_HALF + ((4, 1, 2, 2, 8, 2), (2, 2, 2, 2, 8, 2)), ()) | {"gemm_nt_generic_kernel<float,float>"}


def _tn_f32(x3, tiles):
    return {"gemm_tn_f32_kernel<%s,%d>" % (",".join(map(str, TN_F32_BR[t])), x3) for t in tiles}


def _tn_planes(npl, tiles):
    return {"gemm_tn_x3_kernel<%s,%d>" % (",".join(map(str, TN_PLANES_BR[t])), npl) for t in tiles}


_TN_NARROW = ((32, 512), (64, 64), (64, 128), (64, 256), (128, 64), (128, 128), (128, 256))
# Instances the tables of the default build (no -DEPN_TUNING) reach through gemm.py's entry points, per form / mode.
# NOT reachable, although instantiated (CHANGELOG): gemm_tn_f32_kernel<1,4,2,4,16,X3> and <1,8,4,2,32,X3> for X3 = 3, 2 (a
# 512-column tile of the split forms always takes the planes kernel) and gemm_tn_x3_kernel<2,4,2,2,32,3> (the three-piece form
# pre-splits a group only from N2 >= 512, where the tile is 512 columns wide or 256 x 256).
REACHABLE = {
    ("nt", "native"): _NT_NATIVE,
    ("nt", "split"): _X3(3) | _NT_FALLBACK,
    ("nt", "f16x2"): _X3(2) | _NT_FALLBACK,
    ("nt", "bf16"): _names("gemm_nt_kernel<bf16,bf16,%s>", _NT_HALF + _NT_FULL + ((4, 2, 2, 2, 8, 3),), ()) | {"gemm_nt_generic_kernel<bf16,bf16>"},
    ("nt", "bf16f32"): _names("gemm_nt_kernel<bf16,float,%s>", _NT_HALF + _NT_FULL + ((4, 2, 2, 2, 8, 3),), ()) | {"gemm_nt_generic_kernel<bf16,float>"},
    ("tn", "native"): _tn_f32(0, TN_F32_BR) | {"gemm_tn_generic_kernel<float>"},
    ("tn", "split"): _tn_f32(3, _TN_NARROW) | _tn_planes(3, ((32, 512), (64, 512), (128, 512), (256, 256))) | {"gemm_tn_generic_kernel<float>"},
    ("tn", "f16x2"): _tn_f32(2, _TN_NARROW) | _tn_planes(2, TN_PLANES_BR) | {"gemm_tn_generic_kernel<float>"},
    ("tn", "bf16"): ({"gemm_tn_bf16_kernel<%s>" % ",".join(map(str, v)) for v in TN_BF16.values()}
                     | {"gemm_tn_bf16_ring_kernel<2,2,%d,%d,4,%d>" % (a, b, tn_ring_kr(a, b))
                        for a, b in ((1, 1), (2, 1), (1, 2), (2, 2), (4, 2), (8, 2), (1, 4), (2, 4), (4, 4), (8, 4))}
                     | {"gemm_tn_bf16_ring_kernel<2,2,4,8,3,1>", "gemm_tn_generic_kernel<bf16>"}),
}


def normalise(name):
    """epn_last_kernel()'s text -> the spelling of REACHABLE: no namespace, no blanks, `bf16` for `__bf16`.  The C++ demangler
    predates 'DF16b' (= __bf16), so instances with a bf16 template argument come back MANGLED; those are decoded here for what
    the GEMM templates use (integer, bool, float, double and bf16 arguments), as bench.py does for its report."""
    if isinstance(name, bytes):
        name = name.decode()
    m = re.search(r"_GLOBAL__N_1(\d+)", name) if name.startswith("_Z") else None
    if m is None and name.startswith("_ZN3epn"):
        m = re.match(r"_ZN3epn(\d+)", name)
    if m:
        n = int(m.group(1))
        base, rest = name[m.end():m.end() + n], name[m.end() + n:]
        args = []
        if rest.startswith("I"):
            for tok in re.finditer(r"Li(\d+)E|Lb([01])E|(DF16b)|(f)|(d)|(E)", rest[1:]):
                if tok.group(6):
                    break
                args.append(tok.group(1) or ("true" if tok.group(2) == "1" else "false" if tok.group(2) else None)
                            or ("bf16" if tok.group(3) else "float" if tok.group(4) else "double"))
        return base + ("<" + ",".join(args) + ">" if args else "")
    # ('DF16b' followed by 'f' -- bf16 operands, fp32 output -- is taken for another type by that demangler: 'bool _Accum')
    return name.replace(" ", "").replace("epn::", "").replace("__bf16", "bf16").replace("bool_Accum", "bf16,float")
