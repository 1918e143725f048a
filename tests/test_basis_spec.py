"""Without a device: the exactness arguments of tests/test_gpu_basis_exact.py, case by case (tests/basis_cases.py), and the
margins of its real-data tier.

For every transform case the float64 result must be representable as the family stores it (bf16: after the one rounding the
reference applies), the integer sets must satisfy sum |M||x| < 2^24, and the numpy emulations of the three families
(basis_ref.emulate: sequential fp32; three bf16 planes with the six kept products; hi + lo of M) must reproduce sets P, I, S and
X with `==` -- if an emulation that keeps what the kernels keep cannot, the sets do not pin what they claim to.  Dropping one kept
product or the low plane from the emulation must break `==` on the set that is said to see it."""
import numpy as np
import pytest

import basis_cases as C
import basis_ref as B
import gemm_ref as R

F32, F64 = np.float32, np.float64
SPEC_SHAPES = [s for s in C.TRANSFORM_SHAPES if s.pts in (1, 2, 17)]


@pytest.mark.parametrize("s", C.TRANSFORM_SHAPES, ids=C.sid)
@pytest.mark.parametrize("family", B.FAMILIES)
def test_sets_are_exact_and_emulated(family, s):
    """Every transform case: representable results, the integer bound, the float64 restatement; the emulation of the family's
    arithmetic (the costly part) at the shapes of 1, 2 and 17 points."""
    for kind in C.SETS[family]:
        M, x, ref = C.operands(family, kind, s.na, s.c, s.pts)
        assert np.array_equal(ref.astype(F32).astype(F64), ref), f"{kind}: the float64 result is not a float32"
        if family == "bf16":
            assert np.array_equal(R.bf16_rne(x), x) and (kind != "P" or np.array_equal(B.stored(ref, family).astype(F64), ref))
        if kind == "I":
            assert np.abs(M).max() <= 1000 and np.abs(x).max() <= 250 and s.na * 1000 * 250 < 2 ** 24      # structural
            assert B.abs_budget(M, x).max() < 2.0 ** 24
        if kind in ("P", "X"):
            assert np.array_equal(B.transform(M, x), ref)
        if s in SPEC_SHAPES:
            got = B.emulate(family, M, x)
            assert np.array_equal(got, B.stored(ref, family)), f"{family} {kind}: the emulation differs from the exact result"


def test_sets_see_the_planes(monkeypatch):
    """x3 without am bm fails X; without ah bl fails P (a lost low piece of the input); bf16 without the low plane of M fails S
    (the paired columns) and I."""
    na, c, pts = 60, 32, 2
    M, x, ref = C.operands("x3", "X", na, c, pts)
    monkeypatch.setattr(B, "X3_KEPT", tuple(t for t in B.X3_KEPT if t != (1, 1)))
    assert not np.array_equal(B.emulate("x3", M, x), ref.astype(F32))
    monkeypatch.setattr(B, "X3_KEPT", ((2, 0), (1, 1), (0, 1), (1, 0), (0, 0)))
    M, x, ref = C.operands("x3", "P", na, c, pts)
    assert not np.array_equal(B.emulate("x3", M, x), ref.astype(F32))
    monkeypatch.undo()
    for kind in ("S", "I"):
        M, x, ref = C.operands("bf16", kind, na, c, pts)
        hi_only = B.transform(R.bf16_rne(M), x)
        assert not np.array_equal(B.stored(hi_only, "bf16"), B.stored(ref, "bf16")), kind
    M, x, ref = C.operands("x3", "S", na, c, pts)
    h, m, _ = R.split3(M)
    assert not np.array_equal(B.transform(h.astype(F64) + m, x).astype(F32), ref.astype(F32))


@pytest.mark.parametrize("s", SPEC_SHAPES[::3] + C.STATS_SHAPES, ids=C.sid)
def test_layouts_are_bijections_and_statistics_exact(s):
    blk = C.blocks(s.na)
    assert blk.shape == (s.na, 2) and blk[-1, 0] + blk[-1, 1] == s.na
    x = np.arange(s.pts * s.na * s.c, dtype=F64).reshape(s.pts, s.na, s.c)
    for spec in (0, 1):
        idx = B.layout_index(spec, blk, s.pts, s.c)
        assert np.array_equal(B.from_flat(B.to_flat(x, idx, check=True), idx), x)
    # every block a dense row-major [pts d][d c] matrix: element (pt d + i, j c + ch) of block `base` is row base + i d + j
    sp = B.spectral_index(blk, s.pts, s.c)
    for f in range(s.na):
        base, d = int(blk[f, 0]), B.dim_of(int(blk[f, 1]))
        i, j = divmod(f - base, d)
        pt = s.pts - 1
        assert sp[pt, f, 3] == base * s.pts * s.c + (pt * d + i) * (d * s.c) + j * s.c + 3
    for family in B.FAMILIES:
        M, xx, ref = C.operands(family, "Is", s.na, s.c, s.pts)
        st = B.point_stats(B.stored(ref, family))
        assert np.abs(st).max() < 2.0 ** 24 and np.array_equal(st, np.round(st))
        assert np.array_equal(B.stored(ref, family).astype(F64), ref)


def test_bf16_statistics_case_rounds():
    M, x, ref = C.stats_over_256()
    st = B.stored(ref, "bf16").astype(F64)
    assert np.abs(ref).max() > 256 and not np.array_equal(st, ref)
    assert not np.array_equal(B.point_stats(st), B.point_stats(ref))
    assert (st * st).sum(1).max() < 2.0 ** 24 and np.array_equal(B.emulate("bf16", M, x), st.astype(F32))


def test_dispatch_restatement():
    """so3_basis_any: SMALL = below 2 GiB, fewer than 2^24 points, na c 4 < 2^24; pair mode = c == 32 under the first two."""
    assert C.is_small("f32", 60, 64, 1000) and C.is_small("bf16", 60, 64, 140000) and not C.is_small("f32", 60, 64, 140000)
    assert not C.is_small("bf16", 60, 64, 280000) and not C.is_small("f32", 4, 32, 1 << 24)
    for na, c, pts in C.BIG_SHAPES:
        assert na * c * 4 >= 1 << 24 and (na - 4) * c * 4 < 1 << 25 and c % 32 == 0
        for f in B.FAMILIES:
            assert not C.is_small(f, na, c, pts) and C.instance(f, na, c, pts).endswith("false,false>")
    assert not C.is_small("f32", 60, 69920, 1) and C.is_small("f32", 60, 69888, 1)
    assert C.is_pair("x3", 60, 32, 15) and not C.is_pair("x3", 60, 64, 15)
    assert C.phantom_lanes("x3", 60, 32, 15) and not C.phantom_lanes("x3", 60, 32, 16) and C.phantom_lanes("x3", 60, 96, 16)
    assert C.phantom_lanes("x3", 60, 69920, 3) and not C.phantom_lanes("x3", 64, 65536, 2)
    assert len(C.BASIS_INSTANCES) == 12 and len(C.REACHABLE) == 17
    assert C.instance("f32", 60, 64, 3, True) == "so3_basis_kernel<float,true,true>"
    assert C.instance("bf16", 64, 65536, 2) == "so3_basis_bf16_kernel<false,false>"
    for s in C.TRANSFORM_SHAPES:
        assert all(C.is_small(f, s.na, s.c, s.pts) for f in B.FAMILIES)
    # every value of every parameter, and every width and count with all four directions at na = 60
    for c in (32, 64, 96, 128):
        assert {(s.in_spec, s.out_spec) for s in C.TRANSFORM_SHAPES if s.c == c and s.na == 60} == set(C.DIRECTIONS)
    for pts in (1, 2, 15, 16, 17, 33, 65):
        assert len({(s.in_spec, s.out_spec) for s in C.TRANSFORM_SHAPES if s.pts == pts and s.na == 60}) == 4


@pytest.mark.parametrize("family", B.FAMILIES)
def test_exact_frozen_case(family):
    M, x, stats, gamma, slope, ref = C.exact_frozen(family, 12, 64, 3)
    mean, rstd = B.norm_params(stats, 1, 3, 12, 0.0, frozen=True)
    assert np.array_equal(rstd, np.ones_like(rstd))
    y, n, _ = B.norm_on_load(x, mean, rstd, gamma, None, slope, 3)
    assert np.array_equal(n.astype(F32).astype(F64), n), "the normalised values are not exact in fp32"
    assert np.array_equal(B.transform(M, B.stored(y, family)), ref)


@pytest.mark.parametrize("s,groups", C.DSTATS_SHAPES, ids=lambda v: C.sid(v) if isinstance(v, tuple) else str(v))
@pytest.mark.parametrize("family", B.FAMILIES)
def test_dstats_inputs_keep_clear_of_the_kink(family, s, groups):
    d = C.dstats_inputs(family, s, groups)
    assert d["left"] == 0
    dy, ds, tol, n, k2 = C.dstats_ref(family, s, groups, d)
    assert np.abs(n).min() >= 0.5 * C.DSTATS_TAU, "a pre-activation within the margin of zero"
    assert (n > 0).any() and (n < 0).any()
    assert np.array_equal(ds[..., 0].astype(F32).astype(F64), ds[..., 0]) and np.abs(4 * ds[..., 0]).max() < 2.0 ** 24
    assert np.array_equal(B.stored(dy, family).astype(F64), dy)
    # every group has its own nonzero mean: the mean term and the group select of sb_point_dstats carry weight
    mean, rstd = B.norm_params(d["sums"], groups, d["ppg"], s.na, d["eps"])
    assert k2.min() > 0.05 and k2.max() < 8.0
    for a in range(groups):
        for b in range(a + 1, groups):
            assert np.median(np.abs(mean[a] - mean[b]) * np.minimum(rstd[a], rstd[b])) > 0.25, "two groups share their means"
    # ... so that the statistics of ANOTHER group, or no mean at all, leave the tolerance by orders of magnitude
    gi = np.arange(s.pts) // d["ppg"] if groups > 1 else np.zeros(s.pts, dtype=np.int64)
    for wrong_mean, wrong_rstd in ([(np.zeros_like(mean), rstd)] + ([(np.roll(mean, 1, 0), np.roll(rstd, 1, 0))] if groups > 1 else [])):
        _, nw, xw = B.norm_on_load(d["x"], wrong_mean, wrong_rstd, d["gamma"], d["beta"], C.DSTATS_SLOPE, d["ppg"])
        dw, _, _ = B.dstats(dy, nw, xw, C.DSTATS_SLOPE)
        assert (np.abs(dw[..., 1] - ds[..., 1]) > 1000.0 * tol).mean() > 0.9


@pytest.mark.parametrize("w", C.WEIGHT_CASES + C.WEIGHT_CASES_BF16[-1:], ids=C.wid)
def test_weight_cases(w):
    blk = B.blocks_of(w.dims)
    assert blk.shape[0] == w.na and max(w.dims) <= 7
    for tr in (False, True):
        idx = B.weight_index(blk, w.cin, w.cout, tr)
        assert np.array_equal(np.sort(idx.reshape(-1)), np.arange(w.na * w.cin * w.cout))
    if w.cin * w.cout > 70000:
        return
    for kind in ("I", "S"):
        W, Rm = C.weight_operands(w, kind)
        ref = B.spectral_weights(W, Rm)
        assert np.array_equal(ref.astype(F32).astype(F64), ref)
        g, Rg = C.weight_grad_operands(w, kind)
        gw = B.spectral_weights_bwd(g, Rg)
        assert np.array_equal(gw.astype(F32).astype(F64), gw)
    assert C.weight_slices(5, 7) == 12 and C.weight_slices(256, 256) == 6 and C.weight_slices(512, 512) == 4
    assert {max(x.dims) for x in C.WEIGHT_CASES} >= {5, 6, 7}


def test_real_data_margins():
    """m_family of the real-data tier, measured on the emulations over the very inputs the GPU test uses (printed: CHANGELOG
    quotes them).  The GPU test allows twice these."""
    for family in B.FAMILIES:
        m = C.m_family(family)
        print(f"m_family[{family}] = {m:.3f}")
        assert 0.0 < m < 64.0
    # what the tier is for: the emulation of x3 without its smallest kept term leaves the margin
    c = C.real_case("x3", 64, "fwd")
    keep = tuple(t for t in B.X3_KEPT if t != (1, 1))
    acc = B._partials(np.zeros(c["ref"].shape, F32), R.split3(c["M"]), R.split3(c["x"]), keep, 60)
    assert (np.abs(acc - c["ref"]) / (B.U24 * c["S"])).max() > 2.0 * C.m_family("x3")
