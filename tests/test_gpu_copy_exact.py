"""The kernels that only move data -- epn_cast, epn_cast_add_bf16, epn_transpose_cast (csrc/gemm.hip), epn_gather_rows,
epn_scatter_rows, epn_scatter_rows_add, epn_intra_group_*, epn_conv1x1_c1_* (csrc/glue.hip) -- through their plain C entries, held
to EXACT results: every output equals the numpy restatement of tests/copy_cases.py bit for bit.

1. Every output is a region of a sentinel-filled arena (tests/gemm_ref.py Arena) pre-filled with a value of its own: nothing around
   it may change, the return code and the name epn_last_kernel() reports are those of the restated launcher.  A refused call
   leaves the whole arena untouched.
2. Python surface: ops.CastFn, gemm.cast, gemm.transpose_cast, ops.gather_rows (kernel and torch fallback), ops._fold_grad_shared
   and ops.conv1x1 at cin = 1 against the same restatements, by `==`.
3. The one comparison that is not `==`: the weight gradient of the single-channel convolution on real-valued data, held to
   L 2^-24 sum|x dy| per column (test_conv1x1_c1_weight_gradient_within_its_chain_bound).
tests/test_copy_spec.py proves the restatements, the tables and the bound without a device."""
import ctypes

import numpy as np
import pytest
import torch

import copy_cases as C
import gemm_ref as R

pytestmark = pytest.mark.gpu
F32, BF16, I32 = torch.float32, torch.bfloat16, torch.int32
RECORDED = set()        # kernel names epn_last_kernel() reported
COUNT = {}              # family -> cases compared exactly
FILL = 7.0
_LIVE = []              # inputs of the call being prepared (kept alive until it has run)
DONE = {}               # (family, case) -> failures: every case of a table runs, and counts, once per session


def once(key, fn):
    if key not in DONE:
        bad = []
        fn(bad)
        DONE[key] = bad
    return list(DONE[key])


def _lib():
    from epn_pointcloud_amd import _lib
    return _lib, _lib.get_lib()


def _report(bad):
    assert not bad, f"{len(bad)} failure(s):\n" + "\n".join(bad[:40])


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _dev(a, gpu):
    """numpy -> device tensor: float32 as it is, uint16 as bfloat16, uint32 as int32 (bits kept)."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        t = torch.from_numpy(a.view(np.int16)).to(gpu).view(BF16)
    elif a.dtype == np.uint32:
        t = torch.from_numpy(a.view(np.int32)).to(gpu)
    else:
        t = torch.from_numpy(a).to(gpu)
    _LIVE.append(t)
    return t


def _host(t):
    """device tensor -> numpy in the representation of copy_cases: float32, uint16 bits of bfloat16, uint32 words of int32."""
    t = t.detach().contiguous()
    if t.dtype == BF16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    if t.dtype == I32:
        return t.cpu().numpy().view(np.uint32)
    return t.cpu().numpy()


def _shifted(a, gpu, shift):
    """A 1-D copy of `a` that starts `shift` elements past a 256-byte aligned address."""
    t = _dev(np.asarray(a).reshape(-1), gpu)
    flat = torch.zeros(t.numel() + shift + 64, dtype=t.dtype, device=gpu)
    assert flat.data_ptr() % 256 == 0
    v = flat[shift:shift + t.numel()]
    v.copy_(t)
    _LIVE.append(v)
    return v


def _words(a):
    """Any bit array as uint32 words along its last axis."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32)


def call(bad, what, entry, args, arenas, want_rc=0, kernel="", refused=False):
    """One call: return code, kernel name and the arenas' guard bands (a refused call: the arenas untouched)."""
    _l, lib = _lib()
    lib.epn_last_kernel()
    rc = getattr(lib, entry)(*args, _l.stream_of(arenas[0].flat))
    torch.cuda.synchronize()
    del _LIVE[:]
    name = C.normalise(lib.epn_last_kernel())
    if rc != want_rc:
        bad.append(f"{what}: {entry} returned {rc} ({lib.epn_strerror(rc).decode()}), expected {want_rc}")
    if name != kernel:
        bad.append(f"{what}: ran '{name}', the restated launcher says '{kernel}'")
    if name:
        RECORDED.add(name)
    for a in arenas:
        if refused:
            if not a.untouched():
                bad.append(f"{what}: a refused call wrote to its output")
        else:
            try:
                a.check(f"{what} [{name}]")
            except AssertionError as e:
                bad.append(str(e))
    return rc


def _arena(dtype, gpu, rows, cols, shift=0, fill=True):
    a = R.Arena(dtype, gpu, [(rows, cols, None, 0, shift)])
    if fill:
        a.t[0].fill_(FILL if dtype != I32 else C.FILL_WORD)
    return a


def _same(bad, what, got, want, nan_as_nan=False, family=None):
    got = np.asarray(got).reshape(np.shape(want))
    if not C.same_bits(got, want, nan_as_nan):
        ne = np.flatnonzero(got.reshape(-1) != np.asarray(want).reshape(-1))
        first = int(ne[0]) if ne.size else -1
        bad.append(f"{what}: {ne.size} of {got.size} elements differ, first at {first}: got {got.reshape(-1)[first]!r}, "
                   f"expected {np.asarray(want).reshape(-1)[first]!r}")
    elif family:
        COUNT[family] = COUNT.get(family, 0) + 1


_T = {"f32": F32, "bf16": BF16}


# ------------------------------------------------------------------------------------------------ casts
def run_cast(gpu, bad, what, src, want, s, d, src_shift=0, dst_shift=0, nan=False):
    st = _shifted(src, gpu, src_shift)
    n = st.numel()
    arena = _arena(_T[d], gpu, 1, n, dst_shift)
    rc, kernel = C.cast_launch(n, s, d, src_shift, dst_shift)
    for t, shift in ((st, src_shift), (arena.t[0], dst_shift)):
        assert (t.data_ptr() % 16 == 0) == ((shift * t.element_size()) % 16 == 0)
    call(bad, what, "epn_cast", (_ptr(st), _ptr(arena.t[0]), n, int(s == "bf16"), int(d == "bf16")), [arena], rc, kernel)
    _same(bad, what, _host(arena.t[0]), want, nan, "cast")


def run_cast_case(gpu, c):
    def run(bad):
        src, want = C.cast_data(c)
        run_cast(gpu, bad, c.name, src, want, c.src, c.dst, c.src_shift, c.dst_shift)
    return once(("cast", c.name), run)


@pytest.mark.parametrize("c", C.CAST_CASES, ids=lambda c: c.name)
def test_cast_exact(gpu, c):
    _report(run_cast_case(gpu, c))


def test_cast_special_values_to_bf16(gpu):
    """Ties above an even and an odd bf16 and their neighbours, the overflow threshold, subnormals, signed zeros, infinities and
    NaNs (a NaN stays a NaN; its payload is not pinned), through the vector body, the scalar tail and the scalar kernel."""
    bad = []
    for rot in C.SPECIAL_ROTATIONS:
        x, want = C.special_f32(rot)
        run_cast(gpu, bad, f"special rot {rot}", x, want, "f32", "bf16", nan=True)
        run_cast(gpu, bad, f"special rot {rot} scalar", x, want, "f32", "bf16", src_shift=1, nan=True)
    _report(bad)


def test_cast_every_bf16_pattern_to_f32(gpu):
    bad = []
    bits = C.all_bf16()
    run_cast(gpu, bad, "all bf16", bits, C.from_bf16_bits(bits), "bf16", "f32", nan=True)
    run_cast(gpu, bad, "all bf16 scalar", bits, C.from_bf16_bits(bits), "bf16", "f32", dst_shift=1, nan=True)
    _report(bad)


def test_cast_refusals(gpu):
    bad = []
    for c in C.CAST_REFUSALS:
        src = None if c.null else _shifted(np.zeros(8, np.float32 if c.src == "f32" else np.uint16), gpu, 0)
        arena = _arena(_T[c.dst], gpu, 1, 8, fill=False)
        rc, kernel = C.cast_launch(c.n, c.src, c.dst, null=c.null)
        call(bad, c.name, "epn_cast", (_ptr(src), _ptr(None if c.null else arena.t[0]), c.n, int(c.src == "bf16"), int(c.dst == "bf16")),
             [arena], rc, kernel, refused=True)
    _report(bad)


def run_cast_add(gpu, n):
    def run(bad):
        src, add, want = C.cast_add_data(n)
        arena = _arena(BF16, gpu, 1, n)
        call(bad, f"cast_add n{n}", "epn_cast_add_bf16", (_ptr(_dev(src, gpu)), _ptr(_dev(add, gpu)), _ptr(arena.t[0]), n), [arena],
             *C.cast_add_launch(n))
        _same(bad, f"cast_add n{n}", _host(arena.t[0]), want, family="cast_add")
    return once(("cast_add", n), run)


@pytest.mark.parametrize("n", C.N_LADDER)
def test_cast_add_exact(gpu, n):
    """bf16(src + float(add)): one fp32 add, one rounding -- on operands where bf16(src) + add rounds differently."""
    _report(run_cast_add(gpu, n))


def test_cast_add_refusals(gpu):
    bad = []
    src, add, _ = C.cast_add_data(16)
    for shifts in C.CAST_ADD_SHIFTS:
        s, a = _shifted(src, gpu, shifts[0]), _shifted(add, gpu, shifts[1])
        arena = _arena(BF16, gpu, 1, 16, shifts[2], fill=False)
        call(bad, f"cast_add shifts {shifts}", "epn_cast_add_bf16", (_ptr(s), _ptr(a), _ptr(arena.t[0]), 16), [arena],
             *C.cast_add_launch(16, shifts), refused=True)
    arena = _arena(BF16, gpu, 1, 16, fill=False)
    s, a = _dev(src, gpu), _dev(add, gpu)
    for what, args, n, null in (("null src", (None, a, arena.t[0]), 16, True), ("null add", (s, None, arena.t[0]), 16, True),
                                ("null dst", (s, a, None), 16, True), ("n = 0", (None, None, None), 0, True)):
        call(bad, f"cast_add {what}", "epn_cast_add_bf16", (*[_ptr(t) for t in args], n), [arena], *C.cast_add_launch(n, null=null),
             refused=True)
    _report(bad)


def run_transpose(gpu, pair):
    def run(bad):
        for rows, cols in C.TRANSPOSE_SHAPES:
            s, want = C.transpose_data(rows, cols, *pair)
            arena = _arena(_T[pair[1]], gpu, cols, rows)
            what = f"transpose {rows}x{cols} {pair}"
            call(bad, what, "epn_transpose_cast", (_ptr(_dev(s, gpu)), _ptr(arena.t[0]), rows, cols, int(pair[0] == "bf16"),
                                                   int(pair[1] == "bf16")), [arena], *C.transpose_launch(rows, cols, *pair))
            _same(bad, what, _host(arena.t[0]), want, family="transpose_cast")
    return once(("transpose", pair), run)


@pytest.mark.parametrize("pair", C.TRANSPOSE_PAIRS, ids="_".join)
def test_transpose_cast_exact(gpu, pair):
    bad = run_transpose(gpu, pair)
    src = _dev(np.zeros(64, np.float32), gpu)
    for rows, cols in C.TRANSPOSE_REFUSALS:
        arena = _arena(_T[pair[1]], gpu, 8, 8, fill=False)
        call(bad, f"transpose {rows}x{cols} refused", "epn_transpose_cast", (_ptr(src), _ptr(arena.t[0]), rows, cols, int(pair[0] == "bf16"),
                                                                             int(pair[1] == "bf16")), [arena],
             *C.transpose_launch(rows, cols, *pair), refused=True)
    _report(bad)


# ------------------------------------------------------------------------------------------------ rows
def run_rows(gpu, c):
    return once(("rows", c.name), lambda bad: _run_rows(gpu, c, bad))


def _run_rows(gpu, c, bad):
    """Gather, the plain scatter (distinct indices only) and the accumulating scatter in every tier of the case."""
    idx = C.rows_index(c)
    it = torch.from_numpy(idx).to(gpu)
    w = c.row_bytes // 4
    words = C.rows_words(c, c.p1)
    arena = _arena(I32, gpu, c.b * c.p2, w)
    call(bad, f"{c.name} gather", "epn_gather_rows", (_ptr(_dev(words, gpu)), _ptr(it), _ptr(arena.t[0]), c.b, c.p1, c.p2, c.row_bytes),
         [arena], *C.rows_launch("gather", c.b, c.p1, c.p2, c.row_bytes))
    _same(bad, f"{c.name} gather", _host(arena.t[0]), C.gather_rows(words, idx, fill=C.FILL_WORD).reshape(c.b * c.p2, w), family="gather_rows")
    if C.is_distinct(idx, c.p1):
        g = C.rows_words(c, c.p2)
        arena = _arena(I32, gpu, c.b * c.p1, w)
        call(bad, f"{c.name} scatter", "epn_scatter_rows", (_ptr(_dev(g, gpu)), _ptr(it), _ptr(arena.t[0]), c.b, c.p1, c.p2, c.row_bytes),
             [arena], *C.rows_launch("scatter", c.b, c.p1, c.p2, c.row_bytes))
        _same(bad, f"{c.name} scatter", _host(arena.t[0]), C.scatter_rows(g, idx, c.p1).reshape(c.b * c.p1, w), family="scatter_rows")
    if c.p2 <= C.ROWS_P2_MAX:
        for tier in C.tiers_of(c):
            bf = tier.endswith("bf16")
            g, _, want = C.rows_add_case(c, tier)
            arena = _arena(I32, gpu, c.b * c.p1, w)
            call(bad, f"{c.name} add {tier}", "epn_scatter_rows_add",
                 (_ptr(_dev(_words(g), gpu)), _ptr(it), _ptr(arena.t[0]), c.b, c.p1, c.p2, c.row_bytes, int(bf)), [arena],
                 *C.rows_launch("scatter_add", c.b, c.p1, c.p2, c.row_bytes, bf))
            _same(bad, f"{c.name} add {tier}", _host(arena.t[0]), _words(want).reshape(c.b * c.p1, w), family="scatter_rows_add")


@pytest.mark.parametrize("c", C.ROWS_CASES + C.ROWS_CASES_BEYOND, ids=lambda c: c.name)
def test_rows_exact(gpu, c):
    """Repeated indices receive the fp32 sum of their rows in ascending order from the first occurrence (bf16: one rounding);
    out-of-range indices are skipped -- the gather leaves that destination row as it was."""
    _report(run_rows(gpu, c))


def test_rows_refusals(gpu):
    bad = []
    buf = torch.zeros(1 << 16, dtype=I32, device=gpu)
    for entry, b, p1, p2, rb in C.ROWS_REFUSALS:
        for e in ((entry,) if entry else ("gather", "scatter", "scatter_add")):
            arena = _arena(I32, gpu, 64, 64, fill=False)
            args = (_ptr(buf), _ptr(buf), _ptr(arena.t[0]), b, p1, p2, rb) + ((0,) if e == "scatter_add" else ())
            call(bad, f"{e} b{b} p1 {p1} p2 {p2} row_bytes {rb}", {"gather": "epn_gather_rows", "scatter": "epn_scatter_rows",
                                                                     "scatter_add": "epn_scatter_rows_add"}[e], args, [arena],
                 *C.rows_launch(e, b, p1, p2, rb), refused=True)
    _report(bad)


# ------------------------------------------------------------------------------------------------ intra grouping
def run_intra(gpu):
    def run(bad):
        for c in C.INTRA_CASES:
            feats, table = C.intra_feats(c), C.intra_table(c)
            want = _words(C.intra_group(feats, table))
            arena = _arena(I32, gpu, *want.shape)
            call(bad, c.name, "epn_intra_group_bf16" if c.bf16 else "epn_intra_group_f32",
                 (_ptr(_dev(_words(feats), gpu)), _ptr(_dev(table, gpu)), _ptr(arena.t[0]), c.b, c.p, c.na, c.kn, c.c), [arena],
                 *C.intra_launch(c))
            _same(bad, c.name, _host(arena.t[0]), want, family="intra_group")
    return once("intra", run)


def test_intra_group_exact(gpu):
    bad = run_intra(gpu)
    buf = torch.zeros(4096, dtype=I32, device=gpu)
    for c in C.INTRA_REFUSALS:
        arena = _arena(I32, gpu, 64, 64, fill=False)
        call(bad, c.name, "epn_intra_group_bf16" if c.bf16 else "epn_intra_group_f32",
             (_ptr(buf), _ptr(buf), _ptr(arena.t[0]), c.b, c.p, c.na, c.kn, c.c), [arena], *C.intra_launch(c), refused=True)
    _report(bad)


# ------------------------------------------------------------------------------------------------ conv1x1, one input channel
def _c1_fwd(gpu, bad, what, x, w):
    rows, cout = x.size, w.size
    arena = _arena(F32, gpu, rows, cout)
    call(bad, what, "epn_conv1x1_c1_f32", (_ptr(_dev(x, gpu)), _ptr(_dev(w, gpu)), _ptr(arena.t[0]), rows, cout), [arena],
         *C.c1_launch("fwd", rows, cout))
    _same(bad, what, _host(arena.t[0]), C.c1_forward(x, w).reshape(rows, cout), family="conv1x1_c1 forward")


def _c1_bwd(gpu, bad, what, form, x, dy, cout):
    """-> the weight gradient (float32 numpy) of one of the two forms; the ws form gets exactly the bytes the launcher asks for."""
    rows = x.size
    arena = _arena(F32, gpu, 1, cout)
    args = (_ptr(_dev(x, gpu)), _ptr(_dev(dy, gpu)), _ptr(arena.t[0]), rows, cout)
    if form == "bwd_ws":
        nbytes = C.c1_workspace_bytes(rows, cout) if rows else 0
        ws = torch.empty(max(nbytes // 4, 4), dtype=F32, device=gpu)
        args += (_ptr(ws), nbytes)
    call(bad, what, "epn_conv1x1_c1_bwd_weight_ws_f32" if form == "bwd_ws" else "epn_conv1x1_c1_bwd_weight_f32", args, [arena],
         *C.c1_launch(form, rows, cout))
    return _host(arena.t[0]).reshape(cout)


def run_c1(gpu, rows, cout):
    def run(bad):
        x, w, dy = C.c1_ints(rows, cout)
        _c1_fwd(gpu, bad, f"fwd {rows}x{cout}", x, w)
        for form in ("bwd", "bwd_ws"):
            got = _c1_bwd(gpu, bad, f"{form} {rows}x{cout}", form, x, dy, cout)
            _same(bad, f"{form} {rows}x{cout}", got.astype(np.float64), C.c1_grad64(x, dy), family=f"conv1x1_c1 {form}")
    return once(("c1", rows, cout), run)


@pytest.mark.parametrize("rows,cout", C.C1_SHAPES, ids=lambda v: str(v))
def test_conv1x1_c1_exact(gpu, rows, cout):
    """Integers: y = x w as one multiply, and both forms of the weight gradient equal the float64 sum (zero-filled for no rows)."""
    _report(run_c1(gpu, rows, cout))


def test_conv1x1_c1_forward_full_mantissa_and_forward_only_widths(gpu):
    bad = []
    for rows, cout in C.C1_REAL:
        d = C.c1_real(rows, cout)
        _c1_fwd(gpu, bad, f"fwd real {rows}x{cout}", d["x"], np.ascontiguousarray(d["dy"][1 % rows]))
    for cout in C.C1_COUT_FWD_ONLY:
        x, w, dy = C.c1_ints(65, cout)
        _c1_fwd(gpu, bad, f"fwd 65x{cout}", x, w)
    _report(bad)


def test_conv1x1_c1_refusals(gpu):
    bad = []
    buf = torch.zeros(1 << 16, dtype=F32, device=gpu)
    entries = {"fwd": "epn_conv1x1_c1_f32", "bwd": "epn_conv1x1_c1_bwd_weight_f32", "bwd_ws": "epn_conv1x1_c1_bwd_weight_ws_f32"}
    for cout in C.C1_COUT_REFUSED + C.C1_COUT_FWD_ONLY:
        for e, entry in entries.items():
            if e == "fwd" and cout in C.C1_COUT_FWD_ONLY:
                continue
            arena = _arena(F32, gpu, 8, 2048, fill=False)
            args = (_ptr(buf), _ptr(buf), _ptr(arena.t[0]), 5, cout) + ((_ptr(buf), buf.numel() * 4) if e == "bwd_ws" else ())
            call(bad, f"{e} cout {cout}", entry, args, [arena], *C.c1_launch(e, 5, cout), refused=True)
    rows, cout = 65, 8
    x, w, dy = C.c1_ints(rows, cout)
    need = C.c1_workspace_bytes(rows, cout)
    ws = torch.empty(need // 4 + 8, dtype=F32, device=gpu)
    assert ws.data_ptr() % 16 == 0
    for kind, ptr, nbytes in (("short", ws.data_ptr(), need - 1), ("misaligned", ws.data_ptr() + 4, need), ("null", 0, need)):
        arena = _arena(F32, gpu, 1, cout, fill=False)
        call(bad, f"workspace {kind}", entries["bwd_ws"], (_ptr(_dev(x, gpu)), _ptr(_dev(dy, gpu)), _ptr(arena.t[0]), rows, cout,
                                                         ctypes.c_void_p(ptr), nbytes), [arena],
             *C.c1_launch("bwd_ws", rows, cout, kind), refused=True)
    _report(bad)


@pytest.mark.parametrize("shape", C.C1_REAL, ids=lambda s: f"{s[0]}x{s[1]}")
def test_conv1x1_c1_weight_gradient_within_its_chain_bound(gpu, shape):
    """Real-valued x and near-cancelling dy, both forms: per column |got - fp64| <= L 2^-24 sum|x dy|, L = ceil(rpb / rstep) + rstep
    + nb + 1 the longest chain of roundings (a row lane's sum, the block's lanes, the blocks, the products): L = 37, 37, 146,
    1139 for the shapes of C1_REAL.  The bound comes from the kernel's structure; an fp32 restatement of that order on the CPU
    uses 0.0166, 0.0795, 0.0068 and 0.0002 of it (tests/test_copy_spec.py), and a single lost row is outside it."""
    bad = []
    d = C.c1_real(*shape)
    for form in ("bwd", "bwd_ws"):
        got = _c1_bwd(gpu, bad, f"{form} real {shape}", form, d["x"], d["dy"], shape[1])
        ratio = C.c1_ratio(got, d)
        print(f"{form} {shape}: L = {d['L']}, |kernel - fp64| / (L 2^-24 sum|x dy|) = {ratio:.4f}")
        if not ratio <= 1.0:
            bad.append(f"{form} {shape}: |kernel - fp64| reaches {ratio:.4f} of the bound L = {d['L']}")
    _report(bad)


# ------------------------------------------------------------------------------------------------ 2. the Python surface
def test_python_casts(gpu):
    from epn_pointcloud_amd import gemm, ops
    x4 = R.full_mantissa((2, 8, 5, 3), 11, gpu)
    x2 = R.full_mantissa((37, 9), 12, gpu)
    for x in (x4, x2, x4.contiguous(memory_format=torch.channels_last)):
        y = ops.CastFn.apply(x, BF16)
        assert y.dtype == BF16 and y.shape == x.shape
        assert C.same_bits(_host(y), C.to_bf16_bits(x.cpu().numpy()))
        assert C.same_bits(_host(ops.CastFn.apply(y, F32)), C.from_bf16_bits(_host(y)))
    xg = x4.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(ops.CastFn.apply(xg, BF16), [xg], ops.CastFn.apply(x4, BF16))
    assert g.dtype == F32 and C.same_bits(_host(g), C.from_bf16_bits(C.to_bf16_bits(x4.cpu().numpy())))
    assert C.same_bits(_host(gemm.cast(x2, BF16)), C.to_bf16_bits(x2.cpu().numpy()))
    assert gemm.cast(x2, F32) is x2
    for dt in (F32, BF16):
        t = gemm.transpose_cast(x2, dt)
        want = np.ascontiguousarray(x2.cpu().numpy().T)
        assert t.shape == (9, 37) and C.same_bits(_host(t), want if dt == F32 else C.to_bf16_bits(want))


def test_python_fold_grad_shared_fused_branch(gpu):
    from epn_pointcloud_amd import _lib, ops
    src, add, want = C.cast_add_data(2 * 8 * 5 * 3)
    gf = _dev(src, gpu).view(2, 5, 3, 8).permute(0, 3, 1, 2)            # channels-last [b, c, p, a]
    gs = _dev(add, gpu).view(2, 5, 3, 8).permute(0, 3, 1, 2)
    _lib.get_lib().epn_last_kernel()
    out = ops._fold_grad_shared(gf, gs, BF16)
    assert C.normalise(_lib.get_lib().epn_last_kernel()) == "cast_kernel<float,__bf16,true>"
    assert out.dtype == BF16 and C.same_bits(_host(out.permute(0, 2, 3, 1)).reshape(-1), want)


@pytest.mark.parametrize("dt,p2", [(F32, 20), (BF16, 20), (F32, 8193)], ids=["f32_p2_20", "bf16_p2_20", "f32_p2_8193"])
def test_python_gather_rows(gpu, dt, p2):
    """ops.gather_rows forward and backward on integer data; p2 = 8193 is beyond the accumulating kernel and takes the torch
    composition, which must give the same sums (fp32: torch's own bf16 accumulation rounds after every add)."""
    from epn_pointcloud_amd import _lib, ops
    b, c, p1, a = 2, 4, 40, 2
    rng = np.random.default_rng(p2)
    idx = np.stack([rng.integers(0, p1, size=p2), np.concatenate([np.arange(min(p2, 12)), np.zeros(max(p2 - 12, 0), np.int64)])]).astype(np.int32)
    rows = rng.integers(-3, 4, size=(b, p1, a * c)).astype(np.float32)
    grow = rng.integers(-3, 4, size=(b, p2, a * c)).astype(np.float32)
    feats = torch.from_numpy(rows).to(gpu).view(b, p1, a, c).permute(0, 3, 1, 2).to(dt).requires_grad_(True)
    g = torch.from_numpy(grow).to(gpu).view(b, p2, a, c).permute(0, 3, 1, 2).to(dt)
    lib = _lib.get_lib()
    lib.epn_last_kernel()
    out = ops.gather_rows(feats, torch.from_numpy(idx).to(gpu))
    assert C.normalise(lib.epn_last_kernel()) == ("rows_gather_kernel" if p2 <= 8192 else "")
    (got,) = torch.autograd.grad(out, [feats], g)
    assert np.array_equal(out.detach().permute(0, 2, 3, 1).reshape(b, p2, a * c).float().cpu().numpy(), C.gather_rows(rows, idx))
    want = C.scatter_rows_add(grow, idx, p1)
    if dt == BF16:
        want = C.from_bf16_bits(C.to_bf16_bits(want))
    assert np.array_equal(got.permute(0, 2, 3, 1).reshape(b, p1, a * c).float().cpu().numpy(), want)


@pytest.mark.parametrize("cout", [12, 64])
def test_python_conv1x1_single_channel(gpu, cout):
    """cout 64 runs the outer-product kernels, cout 12 (accepted forward, refused backward) the torch product: both one multiply."""
    from epn_pointcloud_amd import _lib, ops
    b, p, a = 2, 5, 3
    x = R.full_mantissa((b, 1, p, a), 21, gpu)
    w = R.full_mantissa((cout, 1, 1, 1), 22, gpu).requires_grad_(True)
    lib = _lib.get_lib()
    lib.epn_last_kernel()
    y = ops.conv1x1(x, w)
    assert C.normalise(lib.epn_last_kernel()) == ("c1_outer_kernel" if cout == 64 else "")
    xr = x.permute(0, 2, 3, 1).reshape(-1).cpu().numpy()
    assert C.same_bits(y.detach().permute(0, 2, 3, 1).reshape(-1, cout).cpu().numpy(), C.c1_forward(xr, w.detach().reshape(-1).cpu().numpy()))
    xi, wi, dyi = C.c1_ints(b * p * a, cout)
    yi = ops.conv1x1(_dev(xi, gpu).view(b, p, a, 1).permute(0, 3, 1, 2), w)
    ran = []                # epn_last_kernel() is thread-local and the backward runs on autograd's thread: read it there
    hook = w.register_hook(lambda grad: ran.append(C.normalise(lib.epn_last_kernel())))
    (gw,) = torch.autograd.grad(yi, [w], _dev(dyi, gpu).view(b, p, a, cout).permute(0, 3, 1, 2))
    hook.remove()
    if cout == 64:
        assert ran == ["c1_outer_bwd_kernel<true>"], ran
    assert np.array_equal(gw.reshape(-1).double().cpu().numpy(), C.c1_grad64(xi, dyi))


# ------------------------------------------------------------------------------------------------ kernel coverage (last)
def test_every_copy_kernel_was_run(gpu):
    """The names epn_last_kernel() reported during this module are exactly copy_cases.REACHABLE_COPY.  (Cases of the tables
    deselected from the run are run now, through the same runners; a case runs and counts once per session.)"""
    bad = []
    for c in C.CAST_CASES:
        bad += run_cast_case(gpu, c)
    for n in C.N_LADDER:
        bad += run_cast_add(gpu, n)
    for pair in C.TRANSPOSE_PAIRS:
        bad += run_transpose(gpu, pair)
    for c in C.ROWS_CASES + C.ROWS_CASES_BEYOND:
        bad += run_rows(gpu, c)
    bad += run_intra(gpu)
    for rows, cout in C.C1_SHAPES:
        bad += run_c1(gpu, rows, cout)
    print("exact cases per family: " + ", ".join(f"{k} {v}" for k, v in sorted(COUNT.items())))
    assert RECORDED == C.REACHABLE_COPY, (f"never ran {sorted(C.REACHABLE_COPY - RECORDED)}; ran but not listed "
                                          f"{sorted(RECORDED - C.REACHABLE_COPY)}")
    _report(bad)
