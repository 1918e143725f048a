"""What tests/test_gpu_copy_exact.py stands on, proven without a device: the numpy restatements of tests/copy_cases.py agree with
the torch compositions they replace, the restated launch conditions reach every kernel and every refusal, and the tables catch
the mutants a loose test lets through (descending order, a rounding per add, a double-rounded cast_add, a dropped tail, a row
lost at position 256, a row lost from one block of the weight gradient)."""
import numpy as np
import pytest
import torch

import copy_cases as C

F32, U16, U32 = np.float32, np.uint16, np.uint32


def _bf16_tensor(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16)


def _bits_of(t):
    return t.contiguous().view(torch.int16).numpy().view(U16)


# ------------------------------------------------------------------------------------------------ conversions
def test_rounding_to_bf16_on_the_special_values_is_what_the_table_says_and_what_torch_does():
    for name, (f, b) in C.SPECIAL_F32.items():
        x = np.array([f], U32).view(F32)
        assert C.same_bits(C.to_bf16_bits(x), np.array([b], U16), nan_as_nan=True), name
        assert C.same_bits(_bits_of(torch.from_numpy(x).bfloat16()), np.array([b], U16), nan_as_nan=True), name
    tails = set()
    for rot in C.SPECIAL_ROTATIONS:
        x, want = C.special_f32(rot)
        assert C.same_bits(C.to_bf16_bits(x), want, nan_as_nan=True) and x.size % 4 == 3
        tails |= set(x[-3:].view(U32).tolist())
    assert tails == {v[0] for v in C.SPECIAL_F32.values()}              # every value passes through the scalar tail once
    finite = ~np.isnan(x)
    assert np.array_equal(np.signbit(C.from_bf16_bits(want))[finite], np.signbit(x)[finite])        # -0 stays -0
    # the table holds the edges: both kinds of tie, both neighbours of one, both sides of the overflow threshold
    names = set(C.SPECIAL_F32)
    assert {"tie_above_even", "tie_above_odd", "below_tie_even", "above_tie_even", "largest_that_stays_finite",
            "smallest_that_overflows", "neg_zero", "min_subnormal_f32", "pos_inf", "neg_inf", "quiet_nan"} <= names
    assert np.isinf(C.from_bf16_bits(C.to_bf16_bits(np.array([0x7F7F8000], U32).view(F32)))).all()
    assert np.isfinite(C.from_bf16_bits(C.to_bf16_bits(np.array([0x7F7F7FFF], U32).view(F32)))).all()


def test_widening_and_rounding_agree_with_torch_on_every_bf16_pattern():
    bits = C.all_bf16()
    wide = C.from_bf16_bits(bits)
    assert C.same_bits(_bf16_tensor(bits).float().numpy(), wide, nan_as_nan=True)
    assert np.array_equal(np.isnan(wide), ((bits & 0x7F80) == 0x7F80) & ((bits & 0x7F) != 0))
    # bf16 -> f32 -> bf16 is the identity on everything that is not a NaN, here and in torch
    back = C.to_bf16_bits(wide)
    ok = ~np.isnan(wide)
    assert np.array_equal(back[ok], bits[ok]) and np.isnan(C.from_bf16_bits(back[~ok])).all()
    assert np.array_equal(_bits_of(torch.from_numpy(wide).bfloat16())[ok], bits[ok])


@pytest.mark.parametrize("c", [c for c in C.CAST_CASES if c.n <= 2048], ids=lambda c: c.name)
def test_cast_cases_agree_with_torch(c):
    src, want = C.cast_data(c)
    if c.src == "f32":
        assert np.array_equal(_bits_of(torch.from_numpy(src).bfloat16()), want)
        assert c.n < 4 or not np.array_equal(C.from_bf16_bits(want), src)              # the inputs are not bf16 values already
    else:
        assert C.same_bits(_bf16_tensor(src).float().numpy(), want)
    if c.n % 4 and c.src_shift == c.dst_shift == 0:
        fill = U16(0x7FC5) if c.dst == "bf16" else np.array([0x7FC5A5A5], U32).view(F32)[0]
        assert not C.same_bits(C.drop_tail(want, fill), want)                           # a lost tail shows


def test_cast_table_reaches_both_kernels_both_loops_and_every_refusal():
    names, codes = set(), set()
    for c in C.CAST_CASES:
        rc, k = C.cast_launch(c.n, c.src, c.dst, c.src_shift, c.dst_shift, c.null)
        assert rc == 0 and k, c
        names.add(k)
    assert names == {n for n in C.REACHABLE_COPY if n.startswith(("cast_kernel", "cast_scalar")) and not n.endswith("true>")}
    for c in C.CAST_REFUSALS:
        rc, k = C.cast_launch(c.n, c.src, c.dst, c.src_shift, c.dst_shift, c.null)
        assert k == ""
        codes.add(rc)
    assert codes == {0, C.EPN_EINVAL, C.EPN_ENULL}
    assert C.cast_trips(C.N_VECTOR_WRAP, True) == 2 and C.cast_trips(C.N_VECTOR_WRAP - 8, True) == 1
    assert C.cast_trips(C.N_SCALAR_WRAP, False) == 2 and C.cast_trips(C.N_SCALAR_WRAP - 5, False) == 1
    assert max(C.cast_trips(n, True) for n in C.N_LADDER) == 1
    assert C.N_VECTOR_WRAP * 4 < 34e6                                                   # the largest allocation of the GPU file
    assert {n % 4 for n in C.N_LADDER} == {0, 1, 3} and len({c.name for c in C.CAST_CASES}) == len(C.CAST_CASES)


@pytest.mark.parametrize("n", C.N_LADDER)
def test_cast_add_is_one_add_and_one_rounding(n):
    src, add, want = C.cast_add_data(n)
    t = (torch.from_numpy(src) + _bf16_tensor(add).float()).bfloat16()
    assert np.array_equal(_bits_of(t), want)
    if n >= 3:
        for name, m in C.cast_add_mutants(src, add).items():
            assert not np.array_equal(m, want), name
        assert not np.array_equal(C.cast_add_mutants(src, add)["double_rounded"][:1], want[:1])     # the hand-made element
    if n % 4:
        assert not np.array_equal(C.drop_tail(want, U16(0x7FC5)), want)


def test_cast_add_refusals():
    assert C.cast_add_launch(0, null=True) == (0, "")
    assert C.cast_add_launch(5, null=True) == (C.EPN_ENULL, "")
    for s in C.CAST_ADD_SHIFTS:
        assert C.cast_add_launch(5, s) == (C.EPN_EINVAL, ""), s
    assert {tuple(bool(v) for v in s) for s in C.CAST_ADD_SHIFTS} >= {(True, False, False), (False, True, False), (False, False, True)}
    assert C.cast_add_launch(5) == (0, "cast_kernel<float,__bf16,true>")


@pytest.mark.parametrize("pair", C.TRANSPOSE_PAIRS, ids="_".join)
def test_transpose_cases_agree_with_torch(pair):
    names = set()
    for rows, cols in C.TRANSPOSE_SHAPES:
        s, want = C.transpose_data(rows, cols, *pair)
        t = torch.from_numpy(s) if pair[0] == "f32" else _bf16_tensor(s)
        t = t.t().contiguous().to(torch.float32 if pair[1] == "f32" else torch.bfloat16)
        got = t.numpy() if pair[1] == "f32" else _bits_of(t)
        assert C.same_bits(got, want), (rows, cols)
        names.add(C.transpose_launch(rows, cols, *pair)[1])
    assert names == {f"transpose_cast_kernel<{C._TYPE[pair[0]]},{C._TYPE[pair[1]]}>"}
    assert all(C.transpose_launch(r, c, *pair) == (C.EPN_EINVAL, "") for r, c in C.TRANSPOSE_REFUSALS)
    # both sides of the 32 x 32 tile on both axes, and a shape with a partial tile on each
    assert {(r % 32 != 0, c % 32 != 0) for r, c in C.TRANSPOSE_SHAPES} == {(True, True), (True, False), (False, True), (False, False)}


# ------------------------------------------------------------------------------------------------ rows
def _torch_gather(src, idx):
    ii = torch.from_numpy(idx.astype(np.int64))[:, :, None].expand(-1, -1, src.shape[2])
    return torch.gather(src, 1, ii)


_IN_RANGE = [c for c in C.ROWS_CASES + C.ROWS_CASES_BEYOND if c.p2 <= 512 or c.name in ("p2_8192_all_equal", "p2_8193")]


@pytest.mark.parametrize("c", _IN_RANGE, ids=lambda c: c.name)
def test_rows_restatements_agree_with_torch_gather_and_its_backward(c):
    """Integer data in float64: torch.gather and its autograd backward (which sums repeated indices) against the three
    restatements.  Out-of-range indices are skipped: torch sees them replaced by a row of zeros that is cut off again."""
    idx = C.rows_index(c)
    valid = (idx >= 0) & (idx < c.p1)
    safe = np.where(valid, idx, c.p1)                                   # row p1: an extra all-zero source row
    g, _, want = C.rows_add_case(c, "exact")
    src = torch.zeros(c.b, c.p1 + 1, g.shape[2], dtype=torch.float64, requires_grad=True)
    out = _torch_gather(src, safe)
    (back,) = torch.autograd.grad(out, [src], torch.from_numpy(g).double())
    assert np.array_equal(back[:, :c.p1].numpy(), want.astype(np.float64))
    gb, _, wantb = C.rows_add_case(c, "exact_bf16")
    srcb = torch.zeros(c.b, c.p1 + 1, gb.shape[2], dtype=torch.float64, requires_grad=True)
    (backb,) = torch.autograd.grad(_torch_gather(srcb, safe), [srcb], torch.from_numpy(C.from_bf16_bits(gb)).double())
    assert np.array_equal(C.from_bf16_bits(C.to_bf16_bits(backb[:, :c.p1].numpy().astype(F32))), C.from_bf16_bits(wantb))
    if C.is_distinct(idx, c.p1):
        assert np.array_equal(C.scatter_rows(g, idx, c.p1), want)
    words = C.rows_words(c, c.p1)
    got = C.gather_rows(words, idx, fill=C.FILL_WORD)
    ref = _torch_gather(torch.from_numpy(np.concatenate([words, np.full_like(words[:, :1], C.FILL_WORD)], 1).astype(np.int64)), safe)
    assert np.array_equal(got.astype(np.int64), ref.numpy())


def test_order_tiers_pin_the_order_and_the_single_rounding():
    """On every case of the order tiers the ascending fp32 sum differs from the descending one and from the float64 sum rounded
    once, and one bf16 rounding differs from a rounding per add: a kernel with another order cannot pass."""
    seen = 0
    for c in C.ROWS_CASES:
        if "order" not in C.tiers_of(c):
            continue
        seen += 1
        g, idx, want = C.rows_add_case(c, "order")
        assert not np.array_equal(C.scatter_rows_add(g, idx, c.p1, order="descending"), want), c.name
        assert not np.array_equal(C.scatter_rows_add(g, idx, c.p1, order="float64"), want), c.name
        gb, _, wantb = C.rows_add_case(c, "round_bf16")
        assert not np.array_equal(C.scatter_rows_add(gb, idx, c.p1, True, per_step=True), wantb), c.name
    assert seen >= 20


def test_a_row_lost_at_position_256_shows():
    hit = 0
    for c in C.ROWS_CASES:
        idx = C.rows_index(c)
        if c.p2 <= 256 or c.p2 > 512:
            continue
        q = int(idx[0, 256])
        if not 0 <= q < c.p1 or int((idx[0, :256] == q).sum()) == 0:
            continue
        hit += 1
        for tier in ("exact", "exact_bf16"):
            g, _, want = C.rows_add_case(c, tier)
            assert not np.array_equal(C.scatter_rows_add(g, idx, c.p1, tier.endswith("bf16"), lose_at=256), want), (c.name, tier)
    assert hit >= 4


def test_rows_tables_hold_the_edges():
    cases = C.ROWS_CASES
    assert len({c.name for c in cases}) == len(cases)
    assert {c.row_bytes for c in cases} >= {16, 48, 16 * 255, 16 * 256, 16 * 257, 15360}
    assert {c.p2 for c in cases} >= {0, 1, 255, 256, 257, 8192} and {c.p1 for c in cases} >= {1, 7, 300} and {c.b for c in cases} >= {1, 3}
    assert {c.pattern for c in cases} == set(C.PATTERNS) and any(c.oob for c in cases)
    pos = C.rows_index(next(c for c in cases if c.name == "positions_b3"))
    q = pos[0, 0]
    assert list(np.flatnonzero(pos[0] == q)) == [0, 255, 256, 300] and list(np.flatnonzero(pos[1] == pos[1, 1])) == [1, 256, 257]
    bd = next(c for c in cases if c.name == "boundary_p2_257")
    i = C.rows_index(bd)
    assert i[0, -1] == i[1, 0] and (i[0] == i[0, -1]).sum() == 1 and (i[1] == i[1, 0]).sum() == 1 and C.is_distinct(i, bd.p1)
    ba = next(c for c in cases if c.name == "boundary_absent_p2_257")
    i = C.rows_index(ba)
    assert (i[0] == i[0, -1]).sum() == 1 and not (i[1:] == i[0, -1]).any() and C.is_distinct(i, ba.p1)
    big = next(c for c in cases if c.name == "p2_8192_all_equal")       # ascending order held across all 32 strides of the scan
    assert "order" in C.tiers_of(big) and "round_bf16" in C.tiers_of(big)
    for c in cases:                                                     # a different pattern per cloud
        i = C.rows_index(c)
        if c.b > 1 and c.p2 > 1 and c.p1 > 1:
            assert not np.array_equal(i[0], i[1]), c.name
        if c.oob:
            assert (i == -1).any() and (i >= c.p1).any(), c.name
    names, codes = set(), set()
    for c in cases + C.ROWS_CASES_BEYOND:
        for entry in ("gather", "scatter", "scatter_add"):
            for bf in (False, True):
                rc, k = C.rows_launch(entry, c.b, c.p1, c.p2, c.row_bytes, bf)
                if c in C.ROWS_CASES_BEYOND:
                    assert rc == (C.EPN_EINVAL if entry == "scatter_add" else 0)
                else:
                    assert rc == 0 and (k != "") == (c.p2 > 0), c
                names.add(k)
    assert names - {""} == {n for n in C.REACHABLE_COPY if n.startswith("rows_")}
    for entry, b, p1, p2, rb in C.ROWS_REFUSALS:
        for e in ((entry,) if entry else ("gather", "scatter", "scatter_add")):
            assert C.rows_launch(e, b, p1, p2, rb) == (C.EPN_EINVAL, "")
    assert {r[4] for r in C.ROWS_REFUSALS} >= {8, 24} and any(r[0] == "scatter_add" and r[3] == 8193 for r in C.ROWS_REFUSALS)


# ------------------------------------------------------------------------------------------------ intra grouping
@pytest.mark.parametrize("c", C.INTRA_CASES, ids=lambda c: c.name)
def test_intra_group_restatement_is_index_select(c):
    feats, table = C.intra_feats(c), C.intra_table(c)
    t = torch.from_numpy(feats.astype(np.int64))
    ref = torch.stack([t.index_select(2, torch.from_numpy(table[:, k].astype(np.int64))) for k in range(c.kn)], dim=3)
    assert np.array_equal(C.intra_group(feats, table).astype(np.int64), ref.reshape(c.b * c.p * c.na, c.kn * c.c).numpy())
    assert C.intra_launch(c)[0] == 0


def test_intra_table_reaches_both_kernels_and_the_refusals():
    names = {C.intra_launch(c)[1] for c in C.INTRA_CASES}
    assert names == {"intra_group_kernel<f32x4>", "intra_group_kernel<float>"}
    assert {C.intra_launch(c)[1] for c in C.INTRA_CASES if c.bf16} == {"intra_group_kernel<f32x4>"}
    assert all(C.intra_launch(c) == (C.EPN_EINVAL, "") for c in C.INTRA_REFUSALS)
    assert {c.c for c in C.INTRA_REFUSALS if c.bf16} == {4, 12}
    assert {c.c for c in C.INTRA_CASES if not c.bf16} == {1, 3, 4, 5, 8, 64} and {c.c for c in C.INTRA_CASES if c.bf16} == {8, 16, 64}
    for kernel in names:                                                # every table kind and both p with both kernels
        mine = [c for c in C.INTRA_CASES if C.intra_launch(c)[1] == kernel]
        assert {c.table for c in mine} == {"identity", "permutation", "repeats"} and {c.p for c in mine} == {1, 3}
        assert {(c.na, c.kn) for c in mine} == {(1, 1), (12, 5), (60, 12)}


# ------------------------------------------------------------------------------------------------ conv1x1, one channel
@pytest.mark.parametrize("rows,cout", [(1, 4), (65, 8), (1000, 64), (65, 1024), (63, 12)])
def test_conv1x1_c1_restatements_agree_with_conv2d(rows, cout):
    x, w, dy = C.c1_ints(rows, cout)
    xt = torch.from_numpy(x).double().view(1, 1, rows, 1)
    wt = torch.from_numpy(w).double().view(cout, 1, 1, 1).requires_grad_(True)
    y = torch.nn.functional.conv2d(xt, wt)
    assert np.array_equal(y[0, :, :, 0].t().detach().numpy(), C.c1_forward(x, w).astype(np.float64))
    (gw,) = torch.autograd.grad(y, [wt], torch.from_numpy(dy).double().t().reshape(1, cout, rows, 1))
    assert np.array_equal(gw.reshape(cout).numpy(), C.c1_grad64(x, dy))
    if C.c1_accepts("bwd", cout):
        assert np.array_equal(C.c1_grad_fp32(x, dy).astype(np.float64), C.c1_grad64(x, dy))      # integers: any order
    # full-mantissa operands: one fp32 multiply is what float32 conv2d does too
    d = C.c1_real(rows, cout if cout != 12 else 8)
    wf = d["dy"][0]
    yf = torch.nn.functional.conv2d(torch.from_numpy(d["x"]).view(1, 1, rows, 1), torch.from_numpy(wf.copy()).view(-1, 1, 1, 1))
    assert np.array_equal(yf[0, :, :, 0].t().numpy(), C.c1_forward(d["x"], wf))


def test_conv1x1_c1_acceptance_is_one_table():
    """The forward entry, the two backward entries and ops.conv1x1's own branch: the Python surface takes the kernels exactly where
    all three C entries accept, for every cout in 1 .. 1100."""
    takes = C.conv1x1_c1_condition()
    for cout in range(1, 1101):
        fwd, bwd = C.c1_accepts("fwd", cout), C.c1_accepts("bwd", cout)
        assert C.c1_accepts("bwd_ws", cout) == bwd and (not bwd or fwd)
        assert takes(cout) == (fwd and bwd), cout
    assert all(C.c1_accepts("fwd", c) and C.c1_accepts("bwd", c) for c in C.C1_COUT)
    assert not any(C.c1_accepts("fwd", c) for c in C.C1_COUT_REFUSED)
    assert all(C.c1_accepts("fwd", c) and not C.c1_accepts("bwd", c) for c in C.C1_COUT_FWD_ONLY)


def test_conv1x1_c1_tables_hold_the_edges():
    assert {r for r, _ in C.C1_SHAPES} == set(C.C1_ROWS) and {c for _, c in C.C1_SHAPES} == set(C.C1_COUT)
    assert C.c1_plan(65535, 8)[2] == 1024 and C.c1_plan(65535, 8)[0] == 64          # the last shape of the 64-row blocks
    assert C.c1_plan(65536, 8) == (64, 128, 1024) and C.c1_plan(65537, 8) == (65, 128, 1009)
    assert C.c1_plan(1, 4) == (1, 256, 1) and C.c1_plan(65, 1024) == (33, 1, 2)
    names = {C.c1_launch(e, r, c)[1] for e in ("fwd", "bwd", "bwd_ws") for r, c in C.C1_SHAPES}
    assert names - {""} == {n for n in C.REACHABLE_COPY if n.startswith("c1_")}
    for ws in ("short", "misaligned", "null"):
        assert C.c1_launch("bwd_ws", 65, 8, ws) == (C.EPN_EWORKSPACE, "")
    assert C.c1_workspace_bytes(65537, 8) == 1009 * 8 * 4
    for s in C.C1_REAL:
        assert C.c1_chain(*s) == C.C1_REAL_L[s]
    assert max(max(r, 1) * c * 4 for r, c in C.C1_SHAPES) <= 5e6
    assert max(r * 9 for r in C.C1_ROWS) < 2 ** 24


@pytest.mark.parametrize("shape", C.C1_REAL, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_weight_gradient_bound_holds_for_the_order_and_catches_a_lost_row(shape):
    """|fp32 in the kernels' order - fp64| <= L 2^-24 sum|x dy| per column with room to spare (C1_REAL_CPU_RATIO_MAX), and the same
    sum with the largest row of a column left out of its block is outside it."""
    d = C.c1_real(*shape)
    ratio = C.c1_ratio(C.c1_grad_fp32(d["x"], d["dy"]), d)
    print(f"{shape}: L = {d['L']}, |fp32 - fp64| / (L 2^-24 S) = {ratio:.4f}")
    assert ratio <= C.C1_REAL_CPU_RATIO_MAX < 1.0
    r = int(np.argmax(np.abs(d["x"] * d["dy"][:, 0])))
    rpb = C.c1_plan(*shape)[0]
    assert C.c1_ratio(C.c1_grad_fp32(d["x"], d["dy"], drop=(r // rpb, r % rpb)), d) > 1.0
    # near-cancelling columns: the sum is far below the sum of absolute terms
    assert np.median(np.abs(d["g64"]) / d["S"]) < 0.01


# ------------------------------------------------------------------------------------------------ names
def test_every_kernel_name_is_predicted_and_spelled_as_the_library_reports_it():
    predicted = set()
    for c in C.CAST_CASES:
        predicted.add(C.cast_launch(c.n, c.src, c.dst, c.src_shift, c.dst_shift)[1])
    predicted.add(C.cast_add_launch(5)[1])
    predicted |= {C.transpose_launch(3, 3, *p)[1] for p in C.TRANSPOSE_PAIRS}
    predicted |= {C.rows_launch(e, 2, 7, 5, 16, bf)[1] for e in ("gather", "scatter", "scatter_add") for bf in (False, True)}
    predicted |= {C.intra_launch(c)[1] for c in C.INTRA_CASES}
    predicted |= {C.c1_launch(e, 65, 8)[1] for e in ("fwd", "bwd", "bwd_ws")}
    assert predicted == C.REACHABLE_COPY
    # the two spellings epn_last_kernel() can return: demangled, or mangled where the C++ runtime does not know the bf16 type
    assert C.normalise(b"epn::cast_kernel<float, __bf16, false>") == "cast_kernel<float,__bf16,false>"
    assert C.normalise(b"_ZN3epn12_GLOBAL__N_111cast_kernelIfDF16bLb1EEEvPKT_PT0_mPKS5_") == "cast_kernel<float,__bf16,true>"
    assert C.normalise(b"_ZN3epn12_GLOBAL__N_118cast_scalar_kernelIDF16bfEEvPKT_PT0_m") == "cast_scalar_kernel<__bf16,float>"
    assert C.normalise(b"_ZN3epn12_GLOBAL__N_121transpose_cast_kernelIDF16bDF16bEEvPKT_PT0_ii") == "transpose_cast_kernel<__bf16,__bf16>"
    assert C.normalise(b"epn::intra_group_kernel<float __vector(4)>") == "intra_group_kernel<f32x4>"
    assert C.normalise(b"epn::cast_kernel<bool _Accum, false>") == "cast_kernel<__bf16,float,false>"
    assert C.normalise(b"epn::cast_kernel<float, bool _Accum, bool, E>") == "cast_kernel<float,__bf16,true>"
    assert not set(C._MISREAD) & C.REACHABLE_COPY and set(C._MISREAD.values()) <= C.REACHABLE_COPY
    assert C.normalise(b"epn::rows_scatter_add_kernel<true>") == "rows_scatter_add_kernel<true>"
