"""What tests/test_gpu_conv_exact.py relies on, pinned without a device: the dyadic cases of tests/conv_cases.py are exact in
fp32 in every evaluation order, have headroom, are not vacuous; the float64 restatement of tests/conv_ref.py agrees with the fp32
oracle and the golden file; the dispatch restatement agrees with the library's host-side answers and covers every instance and
every edge value -- of the fused passes and, for tests/test_gpu_group_dispatch.py, of the grouping entries; REAL_M is what the
oracle's own error gives."""
import math

import numpy as np
import pytest
import torch

import conv_cases as C
import conv_ref as R
from conftest import golden

f32 = np.float32


# ------------------------------------------------------------------------------------------------ order independence
def _fma(a, b, c):
    """round32(a b + c) with one rounding: the product of two floats is exact in float64, and so is the sum at these sizes."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def _mul_add(a, b, c):
    return ((a * b).astype(f32) + c).astype(f32)


def _w_fp32(d, fused, expanded):
    """w[b, p, a, k, n] in float32, direct (1 - |g - R kappa|^2 / sigma) or expanded (alpha_n + beta_k + g . r) form, products
    and sums rounded after every operation (fused: a b + c rounded once)."""
    ma = _fma if fused else _mul_add
    g, valid, safe = R.inter_gather(d["xyz"], d["new_xyz"], d["idx"])
    g = g.astype(f32)                                                         # xyz - new_xyz: one float32 subtraction
    assert np.array_equal(g.astype(np.float64), R.inter_gather(d["xyz"], d["new_xyz"], d["idx"])[0])
    A, K = d["anchors"], d["kernels"]
    zero = np.zeros((A.shape[0], K.shape[0]), f32)
    rk = np.stack([ma(A[:, None, i, 2], K[None, :, 2], ma(A[:, None, i, 1], K[None, :, 1], ma(A[:, None, i, 0], K[None, :, 0], zero)))
                   for i in range(3)], -1)                                    # [a, k, 3]
    sinv = f32(1.0) / f32(d["sigma"])
    G = g[:, :, None, None, :, :]
    if not expanded:
        diff = (G - rk[None, None, :, :, None, :]).astype(f32)
        d2 = ma(diff[..., 2], diff[..., 2], ma(diff[..., 1], diff[..., 1], (diff[..., 0] * diff[..., 0]).astype(f32)))
        s = (f32(1.0) - (d2 * sinv).astype(f32)).astype(f32)
    else:
        g2 = ma(g[..., 2], g[..., 2], ma(g[..., 1], g[..., 1], (g[..., 0] * g[..., 0]).astype(f32)))
        alpha = (f32(1.0) - (g2 * sinv).astype(f32)).astype(f32)[:, :, None, None, :]
        r = (f32(2.0) * sinv * rk).astype(f32)
        r2 = ma(rk[..., 2], rk[..., 2], ma(rk[..., 1], rk[..., 1], (rk[..., 0] * rk[..., 0]).astype(f32)))
        beta = (-(r2 * sinv)).astype(f32)[None, None, :, :, None]
        R_ = r[None, None, :, :, None, :]
        s = beta
        for i in range(3):
            s = ma(np.broadcast_to(G[..., i], np.broadcast_shapes(G[..., i].shape, R_[..., i].shape)),
                   np.broadcast_to(R_[..., i], np.broadcast_shapes(G[..., i].shape, R_[..., i].shape)), s)
        s = (s + alpha).astype(f32)
    return np.maximum(s, f32(0.0)) * valid[:, :, None, None, :]


@pytest.mark.parametrize("c", C.INTER_CASES, ids=lambda c: c.name)
def test_weights_are_the_same_float_in_every_form(c):
    d = C.inter_case(c)
    w64 = d["ref"]["w"]
    for fused in (False, True):
        for expanded in (False, True):
            assert np.array_equal(_w_fp32(d, fused, expanded).astype(np.float64), w64), (c.name, fused, expanded)


# ------------------------------------------------------------------------------------------------ headroom, not vacuous
@pytest.mark.parametrize("c", C.INTER_CASES, ids=lambda c: c.name)
def test_inter_case_has_headroom_and_is_not_vacuous(c):
    d = C.inter_case(c)
    assert set(d["bits"]) == {C.OUTPUT[p] for p in c.passes} and max(d["bits"].values()) < 1.0
    q = d["q"]
    # the kernels' intermediates: G = sum_n w F, dG = sum_o W dOut, T = sum_k w dG, in units of 1/16
    assert 16 * c.nn * q < 2 ** 24 and c.cout * q * q < 2 ** 24 and 16 * c.ks * c.cout * q * q < 2 ** 24
    for k in ("F", "W", "gOut"):
        assert np.abs(d[k]).min() >= 1 and np.abs(d[k]).max() <= q and np.array_equal(d[k], np.round(d[k]))
    for k in ("xyz", "new_xyz", "kernels"):
        assert np.array_equal(d[k] * 8, np.round(d[k] * 8)) and np.abs(d[k]).max() <= 1.0
    assert math.log2(d["sigma"]) == round(math.log2(d["sigma"]))
    for a in d["anchors"]:
        assert np.array_equal(np.abs(a).sum(0), [1, 1, 1]) and np.array_equal(np.abs(a).sum(1), [1, 1, 1]) and round(np.linalg.det(a)) == 1
    w = d["ref"]["w"]
    assert 0.10 <= (w > 0).mean() <= 0.90, (w > 0).mean()
    assert (w.max(axis=(0, 1, 2, 4)) > 0).all(), "a kernel-point slot never contributes"
    assert (w.max(axis=(0, 1, 2, 3)) > 0).all(), "a neighbour slot never contributes"
    for p in c.passes:
        assert np.any(d["ref"][C.OUTPUT[p]] != 0)
    if c.b > 1:
        assert not np.array_equal(d["idx"][0], d["idx"][1])
    if c.b * c.p2 >= 6:
        p1 = d["xyz"].shape[2]
        assert (d["idx"][1, 0] == p1).all() and d["idx"][0, 0, 0] == p1 and d["idx"][0, 0, -1] == p1
        assert set(d["idx"][0, 2].tolist()) <= {0, p1 - 1}


@pytest.mark.parametrize("c", C.INTRA_CASES, ids=lambda c: c.name)
def test_intra_case_has_headroom_and_is_not_vacuous(c):
    d = C.intra_case(c)
    assert d["bits"] < 1.0
    for k in ("out", "dF", "dW"):
        assert np.any(d["ref"][k] != 0) and np.array_equal(d["ref"][k], np.round(d["ref"][k])) and np.abs(d["ref"][k]).max() < 2 ** 24
    from epn_pointcloud_amd.vgtk.so3conv import functional as L
    if c.na == 60 and c.kn <= 12:
        assert not np.array_equal(d["idx"], np.asarray(L.get_intra_idx())[:, :c.kn])
    assert np.array_equal(d["inv"][d["idx"][:, 0], 0], np.arange(c.na))


# ------------------------------------------------------------------------------------------------ anchored to existing code
def test_restatement_agrees_with_the_fp32_oracle():
    from oracle import so3conv_ref as O
    g = torch.Generator().manual_seed(11)
    b, p1, na, ks, nn, cin, cout, sigma = 2, 9, 7, 8, 5, 3, 4, 0.3
    xyz = torch.rand(b, 3, p1, generator=g) - 0.5
    anchors = torch.linalg.qr(torch.randn(na, 3, 3, generator=g))[0]
    kernels = 0.3 * torch.randn(ks, 3, generator=g)
    idx = torch.randint(0, p1 + 1, (b, p1, nn), generator=g)
    feats = torch.randn(b, cin, p1, na, generator=g, requires_grad=True)
    W = torch.randn(cout, cin * ks, generator=g, requires_grad=True)
    grouped = O.group_nd(O.add_shadow_point(xyz), idx.int()) - xyz.unsqueeze(3)
    w = O.inter_weights(grouped, anchors, kernels, sigma)
    out = O.basic_conv(W, O.inter_feat_grouping(idx, w, O.add_shadow_feature(feats)))
    gy = torch.randn(out.shape, generator=g)
    dF, dW = torch.autograd.grad(out, [feats, W], gy)
    cl = lambda t: t.detach().permute(0, 2, 3, 1).contiguous().numpy()
    ref = R.inter_conv(xyz.numpy(), xyz.numpy(), idx.numpy(), anchors.numpy(), kernels.numpy(), sigma, cl(feats), W.detach().numpy(), cl(gy))
    S = R.inter_abs_sums(xyz.numpy(), xyz.numpy(), idx.numpy(), anchors.numpy(), kernels.numpy(), sigma, cl(feats), W.detach().numpy(),
                         cl(gy), expanded=True)
    # (the oracle's shadow point sits at 1e4: its weight is relu(1 - 1e8 / sigma) = 0, the restatement's zero shadow row)
    assert np.abs(w.numpy() - ref["w"]).max() <= 16 * 2.0 ** -24 * (1 + 3 / sigma)
    for got, key in ((cl(out), "out"), (cl(dF), "dF"), (dW.numpy(), "dW")):
        assert (np.abs(got - ref[key]) <= 16 * 2.0 ** -24 * S[key] + 1e-30).all(), key
    idx2 = torch.stack([torch.randperm(na, generator=g) for _ in range(4)], 1)
    W2 = torch.randn(cout, cin * 4, generator=g, requires_grad=True)
    o2 = O.intra_so3conv(feats, W2, idx2)
    dF2, dW2 = torch.autograd.grad(o2, [feats, W2], gy)
    r2 = R.intra_conv(cl(feats), W2.detach().numpy(), idx2.numpy(), cl(gy))
    for got, key in ((cl(o2), "out"), (cl(dF2), "dF"), (dW2.numpy(), "dW")):
        assert np.abs(got - r2[key]).max() <= 1e-5 * np.abs(r2[key]).max(), key


def test_restatement_agrees_with_the_golden_file():
    g = golden("inter_module_s1_lazy.npz")
    cl = lambda t: np.ascontiguousarray(np.transpose(t, (0, 2, 3, 1)))
    ref = R.inter_conv(g["xyz"], g["new_xyz"], g["inter_idx"], g["anchors"], g["kernels"], np.float32(0.08), cl(g["feats"]), g["W"],
                       cl(g["gy"]))
    for got, key in ((cl(g["out"]), "out"), (cl(g["dF"]), "dF"), (g["dW"], "dW")):
        assert np.abs(got - ref[key]).max() <= 2e-5 * np.abs(ref[key]).max(), key


# ------------------------------------------------------------------------------------------------ dispatch restatement
def test_dispatch_restatement_against_the_library():
    from epn_pointcloud_amd import _lib
    lib = _lib.get_lib()
    keep = np.zeros(16, np.float32)
    seen = 0
    for nn in (1, 16, 128, 129):
        for ks in (4, 12, 16, 18, 24, 30, 32, 36):
            for cin in (8, 16, 48, 256, 272):
                for cout in (8, 16, 80, 256, 272):
                    c = C.InterCase("probe", nn, ks, cin, cout, 60, 2, 3)
                    d = _lib.InterDesc()
                    d.xyz = d.new_xyz = d.ball_idx = d.anchors = d.kernels = keep.ctypes.data
                    d.dense_w, d.sigma = None, 0.25
                    d.b, d.p1, d.p2, d.nn, d.na, d.ks, d.cin, d.cout = 2, 6, 3, nn, 60, ks, cin, cout
                    assert bool(lib.epn_inter_is_fused(d)) == C.inter_is_fused(c), c
                    seen += C.inter_is_fused(c)
    assert seen > 50
    for cin in (8, 16, 48, 256, 272):
        for cout in (8, 16, 80, 256, 272):
            c = C.IntraCase("probe", 12, cin, cout, 60)
            assert bool(lib.epn_intra_is_fused(60, 12, cin, cout)) == C.intra_is_fused(c), c
    for c in C.INTER_CASES:
        assert C.inter_is_fused(c)
    for c in C.INTRA_CASES + C.REAL_INTRA:
        assert C.intra_is_fused(c)


def test_cases_reach_every_instance_and_every_edge_value():
    sizes = {("inter", "fwd"): 18, ("inter", "bwd_data"): 18, ("inter", "bwd_weight"): 14, ("intra", "fwd"): 1,
             ("intra", "bwd_data"): 1, ("intra", "bwd_weight"): 3}
    for key, want in C.REACHABLE.items():
        assert len(want) == sizes[key]                                        # no instance listed twice, none forgotten
    for p in C.PASSES:
        cases = [c for c in C.INTER_CASES if p in c.passes]
        assert {C.inter_instance(c, p) for c in cases} == C.REACHABLE[("inter", p)]
        assert {C.intra_instance(c, p) for c in C.INTRA_CASES} == C.REACHABLE[("intra", p)]
        assert {c.nn for c in cases} >= {1, 15, 16, 17, 32, 33, 64, 65, 128}
        assert {c.ks for c in cases} >= {4, 12, 16, 20, 24, 28, 32}
        assert {c.cout for c in cases} >= {16, 32, 48, 64, 80, 128, 256}
        assert {c.cin for c in cases} >= {16, 32, 48, 256}
        assert {c.na for c in cases} >= {60, 12, 16, 24}
        assert {c.b * c.p2 * c.na for c in cases} >= {63, 64, 65, 127, 128, 129} and any(c.p2 == 1 for c in cases)
    assert {c.kn for c in C.INTRA_CASES} >= {1, 4, 5, 12, 13} and {c.na for c in C.INTRA_CASES} == {60, 12}
    assert {c.cin for c in C.INTRA_CASES} | {c.cout for c in C.INTRA_CASES} >= {16, 48, 64, 128, 256}
    assert any(c.p == 1 for c in C.INTRA_CASES) and all((c.b * c.p * c.na) % 64 for c in C.INTRA_CASES)
    # the weight gradients that walk more than one column tile per workgroup, with a short last workgroup
    by = {c.name: c for c in C.INTER_CASES}
    assert C.inter_weight_grad_plan(by["dw_tiles8"]) == (17, 2, 9) and "weight8" in C.inter_instance(by["dw_tiles8"], "bwd_weight")
    assert C.inter_weight_grad_plan(by["dw_tiles4"]) == (35, 2, 18) and "weight_kernel" in C.inter_instance(by["dw_tiles4"], "bwd_weight")
    pt = next(c for c in C.INTRA_CASES if c.name == "kn4_256_256_pt_points")
    assert C.intra_instance(pt, "bwd_weight") == "intra_bwd_weight_pt_kernel" and C.intra_point_tile_plan(pt) == (39, 2, 20)
    k28 = by["k28_n33_192"]
    assert C.inter_instance(k28, "fwd") == "inter_fwd_kernel<4,2>"
    gs = 4 * 16 * (16 * k28.ks + 4) * 4                                      # the forward's grouped-feature tiles, bytes
    assert gs + k28.cout * (64 + 4) * 4 > 160 * 1024 >= gs + k28.cout * (32 + 4) * 4      # wk = 64 (56 KB budget) did not fit
    for name in ("kn13_128_128_v4_tiles", "kn13_48_128_tiles", "kn1_256_256_v4_tiles"):
        tiles, per = C.intra_weight_grad_plan(next(c for c in C.INTRA_CASES if c.name == name))
        assert per > 1 and tiles % per != 0, (name, tiles, per)


def _group_calls(c):
    """(family, restated instance or None) of the eight calls tests/test_gpu_group_dispatch.py makes for a grouping case."""
    for bf16 in (0, 1):
        for packed in (0, 1):
            yield "group", C.group_instance(c, bf16, packed)
        yield "ungroup", C.ungroup_instance(c, bf16)
        yield "ungroup_det", C.ungroup_det_instance(c, bf16)


def test_group_cases_reach_every_instance_and_every_edge_value():
    sizes = dict(group=16 + 24, ungroup=16 + 44, ungroup_det=16 + 24, inverse_list=2)
    for key, want in sizes.items():
        assert len(C.REACHABLE_GROUPING[key]) == want                                  # no instance listed twice, none forgotten
    seen = {key: set() for key in sizes}
    for c in C.GROUP_CASES:
        for key, name in _group_calls(c):
            assert name is None or name in C.REACHABLE_GROUPING[key], (c, name)
            seen[key].add(name)
    seen["inverse_list"] = {C.inverse_list_instance(c) for c in C.INV_CASES}
    for key in sizes:
        assert seen[key] - {None} == C.REACHABLE_GROUPING[key], (key, C.REACHABLE_GROUPING[key] ^ (seen[key] - {None}))
    # the refusals: the packed order where the wide kernel does not serve, the deterministic entry below 16 anchors
    assert None in seen["group"] and None in seen["ungroup_det"] and None not in seen["ungroup"]
    assert len({c.name for c in C.GROUP_CASES}) == len(C.GROUP_CASES)
    assert {c.nn for c in C.GROUP_CASES} >= {16, 17, 32, 33, 64, 65, 128} and {c.ks for c in C.GROUP_CASES} == {12, 24}
    assert {c.cin for c in C.GROUP_CASES} == {16, 32, 64} and {c.na for c in C.GROUP_CASES} == {60, 12}
    assert {c.p2 for c in C.GROUP_CASES} >= {16, 8, 4, 3} and all(c.b == 2 for c in C.GROUP_CASES)
    # both scatters and both fallbacks, two and four chunks per step, every group size
    plans = {C.ungroup_plan(c) for c in C.GROUP_CASES}
    assert plans >= {None} | {(gp, 1) for gp in (16, 8, 4, 2)} | {(8, 2), (8, 4), (16, 4)}
    # the 32-channel K = 32 case whose p2 16 divides is moved to groups of 8: the one pair the two-chunk form is never asked for
    assert any(C.ungroup_group_points(c) == 16 and C.ungroup_plan(c) == (8, 2) for c in C.GROUP_CASES)
    assert (16, 2) not in plans
    ent = {c.p2 * c.nn for c in C.INV_CASES}
    assert {C.INV_LDS_ENT, C.INV_LDS_ENT + 128} <= ent and {C.INV_LDS_P1, C.INV_LDS_P1 + 1} <= {c.p1 for c in C.INV_CASES}


def test_normalise_reads_the_names_the_runtime_leaves_mangled():
    n = C.normalise
    assert n(b"epn::inter_group_kernel<1, 2, float>") == "inter_group_kernel<1,2,float>"
    assert n(b"_ZN3epn12_GLOBAL__N_118inter_group_kernelILi1ELi1EDF16bEEvNS0_9InterArgsE") == "inter_group_kernel<1,1,__bf16>"
    assert n(b"_ZN3epn12_GLOBAL__N_127inter_ungroup_shared_kernelILi2ELi1EDF16bLi16ELi1ELb0ELi4ELi1EEEvNS0_9InterArgsEPKiPh") \
        == "inter_ungroup_shared_kernel<2,1,__bf16,16,1,false,4,1>"
    assert n(b"_ZN3epn12_GLOBAL__N_127inter_ungroup_shared_kernelILi1ELi1EfLi8ELi2ELb1ELi1ELi1EEEvNS0_9InterArgsEPKiPh") \
        == "inter_ungroup_shared_kernel<1,1,float,8,2,true,1,1>"
    assert n(b"_ZN3epn12_GLOBAL__N_119inverse_list_kernelEPKiiiPiS3_") == "inverse_list_kernel"
    assert n(b"epn::inter_ungroup_shared_kernel<8, 1, bool _Accum, int, EL, int, E, false, 1, 1>") \
        == "inter_ungroup_shared_kernel<8,1,__bf16,2,1,false,1,1>"
    assert sum("__bf16,2,1," in name for fam in C.REACHABLE_GROUPING.values() for name in fam) == 4       # <8, 1 | 2, .., false | true>
    with pytest.raises(ValueError):
        n(b"_ZN3epn12_GLOBAL__N_118inter_group_kernelILi1ELi1EdEEvNS0_9InterArgsE")


def test_group_cases_stay_within_what_the_entries_accept():
    from epn_pointcloud_amd import _lib
    lib = _lib.get_lib()
    keep = np.zeros(16, np.float32)
    for c in C.GROUP_CASES:
        assert C.group_is_mfma(c) and 1 <= c.p2 <= C.MORTON_MAX and 1 <= c.p1 <= C.USH_TAB, c
        d = _lib.InterDesc()
        d.xyz = d.new_xyz = d.ball_idx = d.anchors = d.kernels = keep.ctypes.data
        d.dense_w, d.sigma = None, c.sigma
        d.b, d.p1, d.p2, d.nn, d.na, d.ks, d.cin, d.cout = c.b, c.p1, c.p2, c.nn, c.na, c.ks, c.cin, 16
        assert bool(lib.epn_inter_group_packed_ok(d)) == C.group_packed_ok(c), c
        if C.group_packed_ok(c):
            pos = np.empty(c.cin * c.ks, np.int32)
            assert lib.epn_inter_packed_position(c.cin, c.ks, pos.ctypes.data) == 0
            assert np.array_equal(pos, C.packed_position(c.cin, c.ks)), c
    for c in C.INV_CASES:
        assert c.b >= 1 and c.p1 >= 1 and c.p2 >= 0 and c.nn >= 1 and c.p2 * c.nn < 2 ** 20


# ------------------------------------------------------------------------------------------------ REAL_M from the oracle
def test_real_geometry_bound_comes_from_the_oracle():
    """The fp32 CPU oracle (direct form) against float64 on the real-geometry cases, element by element in units of 2^-24 S:
    REAL_M is twice the worst ratio, rounded up to a power of two."""
    from oracle import so3conv_ref as O
    worst = 0.0
    for entry in C.REAL_INTER:
        c, d, ref, S = C.real_inter_reference(entry)
        T = torch.from_numpy
        feats = T(d["F"]).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        W = T(d["W"]).clone().requires_grad_(True)
        xyz, new_xyz, idx = T(d["xyz"]), T(d["new_xyz"]), T(d["idx"])
        grouped = O.group_nd(O.add_shadow_point(xyz), idx) - new_xyz.unsqueeze(3)
        w = O.inter_weights(grouped, T(d["anchors"]), T(d["kernels"]), d["sigma"])
        out = O.basic_conv(W, O.inter_feat_grouping(idx, w, O.add_shadow_feature(feats)))
        dF, dW = torch.autograd.grad(out, [feats, W], T(d["gOut"]).permute(0, 3, 1, 2).contiguous())
        cl = lambda t: t.detach().permute(0, 2, 3, 1).numpy()
        for got, key in ((cl(out), "out"), (cl(dF), "dF"), (dW.numpy(), "dW")):
            ratio = float((np.abs(got - ref[key]) / (2.0 ** -24 * S[key] + 1e-300)).max())
            print(f"fp32 oracle, {c.name} {key}: worst |oracle - fp64| / (2^-24 S) = {ratio:.4f}")
            worst = max(worst, ratio)
    assert C.REAL_M == 2.0 ** math.ceil(math.log2(2 * worst)), (worst, C.REAL_M)
