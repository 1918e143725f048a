"""What tests/test_gpu_ungroup_cloud_exact.py relies on, pinned without a device: every case of tests/cloud_cases.py meets the
conditions under which the cloud-resident grouping transpose must equal float64 by `==` (weights that are multiples of 1/16,
weight times multiplicity within bf16's 8 bits, partial and destination sums below 2^24 last-bit units), is not vacuous and holds
the special rows; the restated dispatch agrees with the library's host-side answers, maps every case to the instance its comment
claims and covers REACHABLE_CLOUD and every edge value; CLOUD_REAL_M is what the emulation of the documented arithmetic gives.
No device is needed, but the built library is: test_dispatch_restatement_against_the_library asks its host-side entries (as
tests/test_conv_spec.py does), so build() comes first."""
import ctypes
import math

import numpy as np
import pytest

import cloud_cases as K
import conv_cases as C
import conv_ref as R

RUN = [c for c in K.CLOUD_CASES if c.name not in K.REFUSED]


# ------------------------------------------------------------------------------------------------ exactness, not vacuous
@pytest.mark.parametrize("c", RUN, ids=lambda c: c.name)
def test_cloud_case_is_exact_and_not_vacuous(c):
    d = K.cloud_case(c)                                                   # (build_cloud asserts the conditions themselves)
    assert max(d["bits"].values()) < 1.0 and d["q"] in (1, 2, 3)
    dG = d["dG"]
    assert np.abs(dG).min() >= 1 and np.abs(dG).max() <= d["q"] and np.array_equal(dG, np.round(dG)) and K.fits_bf16(dG)
    assert np.array_equal(d["add"], np.round(d["add"])) and np.abs(d["add"]).max() <= 4 and K.fits_bf16(d["add"])
    for k in ("xyz", "new_xyz", "kernels"):
        assert np.array_equal(d[k] * 8, np.round(d[k] * 8)) and np.abs(d[k]).max() <= 0.25
    assert math.log2(c.sigma) == round(math.log2(c.sigma))
    for a in d["anchors"]:
        assert np.array_equal(np.abs(a).sum(0), [1, 1, 1]) and np.array_equal(np.abs(a).sum(1), [1, 1, 1]) and round(np.linalg.det(a)) == 1
    # the proof once more, from the arrays alone, and for the operand with `add`
    geo = (d["xyz"], d["new_xyz"], d["idx"], d["anchors"], d["kernels"], c.sigma)
    ref, bits = K.prove_exact(c, geo, dG, d["add"])
    assert np.array_equal(ref, d["ref"]) and bits == d["bits"]
    tot = ref + d["add"]
    assert np.array_equal(tot, tot.astype(np.float32)) and np.abs(tot).max() * 16 < 2 ** 24
    # the same weights in fp32, direct and expanded, fused or not (what the S-MFMA of the kernel evaluates)
    from test_conv_spec import _w_fp32
    w = R.inter_weights(*geo)[0]
    for fused in (False, True):
        assert np.array_equal(_w_fp32(d, fused, True).astype(np.float64), w), (c.name, fused)
    # not vacuous
    assert np.any(ref != 0) and (w > 0).any()
    if c.b * c.p2 >= 6:
        assert 0.05 <= (w > 0).mean() <= 0.95, (w > 0).mean()
        assert (w.max(axis=(0, 1, 2, 4)) > 0).all(), "a kernel-point slot never contributes"
        assert (w.max(axis=(0, 1, 2, 3)) > 0).all(), "a neighbour slot never contributes"
    m = K.slot_multiplicity(d["idx"], c.p1)
    idx = d["idx"]
    for kind, (bb, pp) in d["special"].items():
        row = idx[bb, pp]
        if kind == "one_point":
            assert len(set(row.tolist())) == 1 and m[bb, pp, 0] == c.nn and not m[bb, pp, 1:].any()
            assert R.inter_weights(*geo)[0][bb, pp].max() > 0
        elif kind == "cyclic_ragged":
            cnt = len(set(row.tolist()))
            assert c.nn % cnt and m[bb, pp, :cnt].max() - m[bb, pp, :cnt].min() == 1 and m[bb, pp].sum() == c.nn
        elif kind == "cyclic_breaks":
            assert row[:4].tolist() == [1, 2, 1, 3] and m[bb, pp].max() == 1
        elif kind == "duplicates":
            assert row.tolist() == [3, 5] + [3] * (c.nn - 2) and m[bb, pp].min() == 1 and K.duplicate_rows(idx, c.p1)[bb, pp]
        elif kind == "cyclic_inner":
            assert K.row_period(row) == 5 and m[bb, pp, :5].min() >= 2 and not m[bb, pp, 5:].any() and K.duplicate_rows(idx, c.p1)[bb, pp]
        elif kind == "negative":
            assert row[-1] == -1 and m[bb, pp, -1] == 0
        else:
            assert row[-1] == 2 ** 30 and (row == c.p1 + 1).any() == (c.nn > 1) and m[bb, pp, -1] == 0
    if c.b > 1 and c.p2 >= 1:
        assert not np.array_equal(idx[0], idx[1])


def test_special_rows_reach_every_neighbour_tile_count():
    """Every kind of special row exists at NT = 1, 2 and 4 (the last slot of such a row lies in the last neighbour tile), and the
    rows of conv_cases._index_table are still there."""
    seen = {}
    for c in RUN:
        d = K.cloud_case(c)
        for kind in d["special"]:
            seen.setdefault(kind, set()).add(K._nt(c.nn))
        if c.b * c.p2 >= 6 and c.b >= 2:
            idx = d["idx"]
            assert (idx[1, 0] == c.p1).all() and idx[0, 0, 0] == c.p1 and idx[0, 0, -1] == c.p1
            assert set(idx[0, 2].tolist()) <= {0, c.p1 - 1}
    assert seen == {kind: {1, 2, 4} for kind in K.SPECIAL_KINDS}, seen


def test_slot_multiplicity_restates_the_table_kernel():
    m = lambda row, p1=6: K.slot_multiplicity(np.array([[row]]), p1)[0, 0].tolist()
    assert m([1, 2, 3, 1, 2, 3, 1]) == [3, 2, 2, 0, 0, 0, 0]
    assert m([4, 4, 4, 4]) == [4, 0, 0, 0]
    assert m([1, 2, 1, 3]) == [1, 1, 1, 1]
    assert m([3, 5, 3, 3, 3]) == [1, 1, 1, 1, 1]
    assert m([6, 6, 6]) == [0, 0, 0] and m([-1, 2, 7]) == [0, 1, 0]
    assert m([6, 1, 6, 1, 6]) == [0, 2, 0, 0, 0]
    d = lambda row: bool(K.duplicate_rows(np.array([[row]]), 6)[0, 0])
    assert d([3, 5, 3, 3]) and d([1, 2, 2, 4]) and not d([1, 2, 1, 2]) and not d([0, 1, 2, 3]) and not d([6, 6, 1, 2])
    # a cyclic row whose period names a point twice: folded, and its kept slots still meet in one accumulator
    assert m([1, 2, 2, 1, 2, 2, 1]) == [3, 2, 2, 0, 0, 0, 0] and d([1, 2, 2, 1, 2, 2, 1]) and not d([1, 6, 6, 1, 6, 6])
    row = ([1] + [2] * 31) * 2
    assert K.row_period(row) == 32 and m(row) == [2] * 32 + [0] * 32 and d(row)
    row = [1] + [2] * 62 + [1]
    assert K.row_period(row) == 63 and m(row) == [2] + [1] * 62 + [0] and d(row)


# ------------------------------------------------------------------------------------------------ dispatch restatement
def _desc(c, keep):
    from epn_pointcloud_amd import _lib
    d = _lib.InterDesc()
    d.xyz = d.new_xyz = d.ball_idx = d.anchors = d.kernels = keep.ctypes.data
    d.dense_w, d.sigma = None, c.sigma
    d.b, d.p1, d.p2, d.nn, d.na, d.ks, d.cin, d.cout = c.b, c.p1, c.p2, c.nn, c.na, c.ks, c.cin, 16
    return d


def test_dispatch_restatement_against_the_library():
    """epn_inter_ungroup_cloud_ok and the workspace size (at least the offsets, the neighbourhood table and the scalars; 0 for a
    refused shape) on a grid of shapes around every limit, and on every case."""
    from epn_pointcloud_amd import _lib
    lib = _lib.get_lib()
    keep = np.zeros(16, np.float32)
    probes = [K.CloudCase("probe", nn, ks, cin, na, 2, p2, p1)
              for nn in (1, 16, 33, 64, 65) for ks in (4, 12, 18, 32, 36) for cin in (8, 16, 48, 128) for na in (1, 60)
              for p2 in (0, 3, 4096, 4097) for p1 in (1, 6, 1275, 1276)]
    yes = 0
    for c in probes + K.CLOUD_CASES:
        d = _desc(c, keep)
        assert bool(lib.epn_inter_ungroup_cloud_ok(ctypes.byref(d))) == K.cloud_ok(c), c
        need = int(lib.epn_inter_ungroup_cloud_workspace_bytes(ctypes.byref(d)))
        if K.cloud_ok(c):
            yes += 1
            assert need > K.workspace_extra_bytes(c) and need % 4 == 0, (c, need)          # (+ the rotated-kernel tables in front)
        else:
            assert need == 0, c
    assert 100 < yes < len(probes)
    for c in K.CLOUD_CASES:
        assert K.cloud_ok(c) == (c.name not in K.REFUSED), c


def test_cases_map_to_the_claimed_instances_and_cover_the_reachable_set():
    assert len(K.REACHABLE_CLOUD) == 38 and len(K.UNREACHABLE_CLOUD) == 10 and not K.REACHABLE_CLOUD & set(K.UNREACHABLE_CLOUD)
    assert len({c.name for c in K.CLOUD_CASES}) == len(K.CLOUD_CASES)
    by = {c.name: c for c in K.CLOUD_CASES}
    for name, (f32, bf16) in K.INSTANCES.items():
        assert (K.cloud_instance(by[name], 0), K.cloud_instance(by[name], 1)) == (f32, bf16), name
    seen = {K.cloud_instance(c, t) for c in RUN for t in (0, 1)}
    assert seen == K.REACHABLE_CLOUD, (sorted(K.REACHABLE_CLOUD - seen), sorted(seen - K.REACHABLE_CLOUD))
    # an unreachable instance would need more channels per workgroup than the cap of its (NT, type) allows at ANY cin
    for nn in (16, 32, 64):
        for t in (0, 1):
            widest = max(K.channels_per_wg(K.CloudCase("probe", nn, 24, cin, 1), t) for cin in range(16, 1025, 16))
            assert widest == K._cap(nn, t)
            for nl in (1, 2, 4, 8):
                assert (K._name(K._nt(nn), 2, t, nl) in K.REACHABLE_CLOUD) == (16 * nl <= widest)


def test_cases_hold_every_edge_value():
    run = RUN
    assert {c.nn for c in run} >= {1, 15, 16, 17, 32, 33, 64} and {c.ks for c in run} >= {4, 12, 16, 20, 24, 28, 32}
    for nn in (16, 32, 64):
        assert {c.cin for c in run if c.nn == nn and c.p1 == 6} >= {16, 32, 48, 64, 96, 128, 256}
    assert {c.p2 for c in run} >= {1, 15, 16, 17, 33} and {c.b * c.p2 for c in run} >= {1, 7, 8, 9, 31, 32, 33}
    assert {c.na for c in run} == {1, 2, 3, 4, 5}
    # several channel blocks per grid row, in both types
    assert any(c.cin // K.channels_per_wg(c, 0) >= 4 for c in run) and any(c.cin // K.channels_per_wg(c, 1) >= 2 for c in run)
    # the LDS edge: the widest workgroup that fits changes exactly between the two p1 of a pair, 16 -> refused at the last
    lds = lambda p1, cr: (p1 + K.UC_DUMMY) * cr * 8 + 16
    for cr, p1 in ((128, 155), (64, 315), (32, 635), (16, 1275)):
        assert lds(p1, cr) <= K.UC_LDS_MAX < lds(p1 + 1, cr)
        pair = [(c, d) for c in K.CLOUD_CASES for d in K.CLOUD_CASES
                if c.name.startswith("lds_") and c.cin == cr and c.p1 == p1 and d == c._replace(name=d.name, p1=p1 + 1)]
        assert pair, (cr, p1)
        assert any(K.channels_per_wg(c, t) == cr and K.channels_per_wg(d, t) == (cr // 2 if cr > 16 else 0)
                   for c, d in pair for t in (0, 1)), (cr, p1)
    by = {c.name: c for c in K.CLOUD_CASES}
    for name in K.SCALE_CASES:
        assert name in by
    assert [K._nt(by[n].nn) for n in K.SCALE_CASES] == [1, 2, 4]
    for name, nn2 in K.INVARIANCE_CASES:
        assert K._nt(by[name].nn) != K._nt(nn2) and K.cloud_ok(by[name]._replace(nn=nn2))


def test_slot_permutation_keeps_the_multiset_and_the_cyclic_rows():
    for name, _ in K.INVARIANCE_CASES:
        c = next(c for c in RUN if c.name == name)
        d = K.cloud_case(c)
        idx2 = K.permute_slots(d["idx"], np.random.default_rng(5))
        assert not np.array_equal(idx2, d["idx"])
        assert np.array_equal(np.sort(idx2, axis=2), np.sort(d["idx"], axis=2))
        m1, m2 = K.slot_multiplicity(d["idx"], c.p1), K.slot_multiplicity(idx2, c.p1)
        assert np.array_equal(m1.max(axis=2), m2.max(axis=2)) and m1.max() > 1
        ref2 = K.prove_exact(c, (d["xyz"], d["new_xyz"], idx2, d["anchors"], d["kernels"], c.sigma), d["dG"])[0]
        assert np.array_equal(ref2, d["ref"])


def test_normalise_reads_the_cloud_kernels_names():
    n = C.normalise
    assert n(b"epn::inter_ungroup_cloud_kernel<1, 1, float, 16, 1>") == K._name(1, 1, 0, 1)
    for nt in (1, 2, 4):
        for kt in (1, 2):
            for nl in (1, 2, 4, 8):
                mangled = f"_ZN3epn12_GLOBAL__N_126inter_ungroup_cloud_kernelILi{nt}ELi{kt}EDF16bLi16ELi{nl}EEEvNS0_6UcArgsE"
                assert n(mangled.encode()) == K._name(nt, kt, 1, nl)


# ------------------------------------------------------------------------------------------------ scale, extreme, wrap
def test_extreme_and_wrap_cases_are_what_they_claim():
    c, geo, dG, ref = K.extreme_case()
    assert K.cloud_ok(c) and np.abs(dG).min() == np.abs(dG).max() == K.AMAX_TOP and K.fits_bf16(dG)
    # one contribution: multiplicity 64 x 32 kernel points x amax at the scale uc_scale picks (2^(50 - 11) per unit of 2^0)
    assert 64 * 32 * float(K.AMAX_TOP) * 2.0 ** 39 < 2.0 ** 50 and 64 * 32 * float(K.AMAX_TOP) * 2.0 ** 39 > 2.0 ** 50 * (1 - 2.0 ** -7)
    assert (K.wrap_crossing("plain"), K.wrap_crossing("period")) == (131, 266)
    for kind, (row, point, slots, mult, other) in K.WRAP_ROWS.items():
        p2 = K.wrap_crossing(kind)
        for q in (p2 - 1, p2):
            c, geo, dG, ref = K.wrap_case(kind, q)
            assert K.cloud_ok(c) and (c.nn, c.ks, c.cin, c.na, c.p1, c.b) == (64, 32, 16, 1, 6, 1)
            # no single contribution reaches 2^50 units at the scale the folded multiplicity alone gives, their sum crosses 2^63
            scale = 2.0 ** (50 - math.ceil(math.log2(mult * 32)))
            assert mult * 32 * float(K.AMAX_TOP) * scale < 2.0 ** 50
            assert (ref[0, point, 0, 0] * scale >= 2.0 ** 63) == (q == p2)
    # with nn reported for such a row the unit is 2^(50 - 11) per 2^0 and the sum stays below 2^62 up to p2 = 4096
    assert 4096 * 64 * 32 * float(K.AMAX_TOP) * 2.0 ** 39 < 2.0 ** 62


# ------------------------------------------------------------------------------------------------ CLOUD_REAL_M
def geo_of(d):
    return d["xyz"], d["new_xyz"], d["idx"], d["anchors"], d["kernels"], d["sigma"]


def test_real_geometry_bound_comes_from_the_emulation():
    """The numpy emulation of the documented arithmetic (fp32 weights in the expanded form the S-MFMA evaluates, bf16-rounded
    for the bf16 instances; fp32 products; exact sum; one rounding to the output type) against float64 on the real geometries,
    element by element in units of 2^-24 S: CLOUD_REAL_M is twice the worst ratio, rounded up to a power of two."""
    worst = {"f32": 0.0, "bf16": 0.0}
    for entry in C.REAL_INTER:
        c, d, ref, S = K.real_cloud_reference(entry)
        assert K.cloud_ok(c) and (S > 0).mean() > 0.5
        w32 = K.weights_fp32(d)
        assert np.abs(w32 - R.inter_weights(*geo_of(d))[0]).max() < 1e-4
        for t, bf16 in (("f32", 0), ("bf16", 1)):
            got = K.emulate_cloud(c, d, w32, bf16)
            ratio = float((np.abs(got - ref) / (2.0 ** -24 * S + 1e-300)).max())
            print(f"emulation, {c.name} {t}: worst |emulation - fp64| / (2^-24 S) = {ratio:.4f}")
            worst[t] = max(worst[t], ratio)
    for t in worst:
        assert K.CLOUD_REAL_M[t] == 2.0 ** math.ceil(math.log2(2 * worst[t])), (t, worst[t], K.CLOUD_REAL_M[t])
