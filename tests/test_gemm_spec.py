"""The GEMM tests' own footing, without a device: every case of tests/gemm_cases.py is in the exact-integer regime, the restated
dispatch tables reach every instance of gemm_cases.REACHABLE and agree with the library's host-only workspace queries, the
numpy emulations of the operand splits (tests/gemm_ref.py) meet what csrc/gemm.h says of them, and gemm.py's wrappers refuse
what they can refuse before a device is involved."""
import numpy as np
import pytest
import torch

import gemm_cases as G
import gemm_ref as R
from epn_pointcloud_amd import _lib, gemm


@pytest.mark.parametrize("form", G.NT_FORMS)
def test_nt_cases_stay_in_the_exact_regime(form):
    cases = G.nt_single_cases(form) + G.nt_layout_cases(form) + G.nt_stats_cases(form) + [G.MANY_TILE]
    for probs, flags in G.nt_group_cases(form).values():
        assert len(probs) == len(flags)
        for i0 in range(0, len(probs), G.GEMM_MAX_PROB):                  # ascending per launch: the launcher's sort has work to do
            chunk = probs[i0:i0 + G.GEMM_MAX_PROB]
            assert all(a.K <= b.K for a, b in zip(chunk, chunk[1:])) and (len(chunk) == 1 or chunk[0].K < chunk[-1].K)
        cases += [c._replace(stats="s" in f) for c, f in zip(probs, flags)]
    assert all(G.nt_exact(c) for c in cases)
    assert max(c.M for c in cases if c != G.MANY_TILE) <= 131072 and max(c.N for c in cases) <= 1280
    e16 = G.e16_of(form)
    assert any(c.lda % e16 for c in cases) and any(c.ldb % e16 for c in cases) and any(c.ash for c in cases) and any(c.bsh for c in cases)
    assert any(c.lda and not c.lda % e16 for c in cases) and any(c.ldb and not c.ldb % e16 for c in cases)
    assert {4, 1} <= {c.ldc - c.N for c in cases if c.ldc}


@pytest.mark.parametrize("form", G.NT_FORMS)
def test_nt_cases_reach_every_instance_at_every_row_count(form):
    assert G.nt_all_instances(form) == G.REACHABLE[("nt", form)]
    rows = {}
    for c in G.nt_single_cases(form):
        inst = G.nt_instance(form, [c])
        if G.nt_block(inst):
            rows.setdefault(inst, set()).add(c.M)
    for inst, ms in rows.items():
        bm = G.nt_block(inst)[0]
        assert {1, 31, 33, bm - 1, bm + 1, bm} <= ms, (inst, sorted(ms))
    if not form.startswith("bf16"):       # the split forms' fallbacks: K in {16, 48} and an odd lda / a misaligned A
        assert {16, 48} <= {c.K for c in G.nt_single_cases(form)}
    else:                                 # the three-stage ring with 1 .. 4 K steps
        ring = [c.K // 64 for c in G.nt_single_cases(form) if G.nt_instance(form, [c]).endswith("8,3>")]
        assert {1, 2, 3, 4} <= set(ring)
    groups = G.nt_group_cases(form)
    assert {len(p) for p, _ in groups.values()} >= {2, 5, 6, 7, 13}
    assert any(c.M == 0 for c in groups["six_m0_middle"][0][1:-1])
    for probs, _ in groups.values():      # tile counts of the grouped launches: not all multiples of 8 (the padding has work to do)
        blk = G.nt_block(G.nt_instance(form, probs[:G.GEMM_MAX_PROB]))
        if blk and len(probs) > 1:
            assert any((-(-c.M // blk[0]) * -(-c.N // blk[1])) % 8 for c in probs[:G.GEMM_MAX_PROB - 1])
    if form == "native":
        assert (G.MANY_TILE.M // 128) * (G.MANY_TILE.N // 128) == 3840
        assert G.nt_instance(form, [G.MANY_TILE._replace(M=G.MANY_TILE.M - 128)]) != G.nt_instance(form, [G.MANY_TILE])


@pytest.mark.parametrize("mode", G.TN_MODES)
def test_tn_cases_plan_and_exact_regime(mode):
    """The restated split counts against epn_gemm_tn_workspace_bytes for every single-problem case; the split counts the row cases
    are there for; every reachable instance."""
    lib = _lib.get_lib()
    cases = G.tn_width_cases() + G.tn_row_cases(mode) + G.tn_layout_cases()
    for c in cases:
        assert G.tn_exact(c)
        assert int(lib.epn_gemm_tn_workspace_bytes(G.TN_MODE_ID[mode], c.R, c.N1, c.N2)) == G.tn_workspace(mode, c), c
    assert all(G.tn_exact(c) for g in G.TN_GROUPS.values() for c in g)
    assert {len(g) for g in G.TN_GROUPS.values()} >= {2, 5, 6}
    d = {"native": 0, "bf16": 1}.get(mode, 2)
    want = {2048: 2, 2080: 2, 3072: 3, 17408: 17, 66560: 65} if mode != "bf16" else {8704: 17, 33280: 65}
    for r, s in want.items():
        assert G.tn_splits(d, r, 64, 64) == s
    assert G.tn_splits(d, 32, 64, 64) == 1
    assert not any(G.tn_fast_ok(mode, G.TnCase(r, 64, 64)) for r in (1, 31, 33, 100))
    assert G.tn_all_instances(mode) == G.REACHABLE[("tn", mode)]


def test_unreachable_instances_are_the_documented_ones():
    """Instances the tables of csrc/gemm_tn.hip instantiate but no entry point reaches (named in CHANGELOG.md)."""
    every = {"gemm_tn_f32_kernel<%s,%d>" % (",".join(map(str, v)), x3) for v in G.TN_F32_BR.values() for x3 in (3, 2)}
    every |= {"gemm_tn_x3_kernel<%s,%d>" % (",".join(map(str, v)), npl) for v in G.TN_PLANES_BR.values() for npl in (3, 2)}
    reach = G.REACHABLE[("tn", "split")] | G.REACHABLE[("tn", "f16x2")]
    assert every - reach == {"gemm_tn_f32_kernel<1,4,2,4,16,3>", "gemm_tn_f32_kernel<1,4,2,4,16,2>", "gemm_tn_f32_kernel<1,8,4,2,32,3>",
                             "gemm_tn_f32_kernel<1,8,4,2,32,2>", "gemm_tn_x3_kernel<2,4,2,2,32,3>"}


def test_kernel_names_are_read_demangled_or_not():
    """epn_last_kernel() demangles what the C++ demangler knows; a bf16 template argument ('DF16b') leaves the name mangled."""
    n = G.normalise
    assert n(b"epn::gemm_nt_x3_kernel<4, 1, 2, 2, 3, 3>") == "gemm_nt_x3_kernel<4,1,2,2,3,3>"
    assert n("epn::gemm_nt_kernel<float, float, 8, 1, 2, 1, 4, 2>") == "gemm_nt_kernel<float,float,8,1,2,1,4,2>"
    assert n("epn::gemm_tn_generic_kernel<__bf16>") == "gemm_tn_generic_kernel<bf16>"
    assert n("_ZN3epn12_GLOBAL__N_114gemm_nt_kernelIDF16bDF16bLi8ELi1ELi2ELi2ELi4ELi2EEEvNS_11GemmNtBatchE") == "gemm_nt_kernel<bf16,bf16,8,1,2,2,4,2>"
    assert n("_ZN3epn12_GLOBAL__N_114gemm_nt_kernelIDF16bfLi4ELi2ELi2ELi2ELi8ELi3EEEvNS_11GemmNtBatchE") == "gemm_nt_kernel<bf16,float,4,2,2,2,8,3>"
    assert n("_ZN3epn12_GLOBAL__N_122gemm_nt_generic_kernelIDF16bfEEvPKT_S4_PT0_xiixxx") == "gemm_nt_generic_kernel<bf16,float>"
    assert n("_ZN3epn12_GLOBAL__N_122gemm_tn_generic_kernelIDF16bEEvPKT_S4_Pfxiixxx") == "gemm_tn_generic_kernel<bf16>"
    assert n("epn::gemm_nt_kernel<bool _Accum, 4, 2, 2, 2, 8, 3>") == "gemm_nt_kernel<bf16,float,4,2,2,2,8,3>"
    every = set().union(*G.REACHABLE.values())
    assert all(n(v) == v for v in every)


def _values(n, seed):
    """n float32 values over 60 binades, a third of them within a few ulps of a power of two."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * np.exp2(rng.integers(-30, 31, n))).astype(np.float32)
    near = np.exp2(rng.integers(-30, 31, n // 3)).astype(np.float32)
    near = near.view(np.uint32) + rng.integers(-3, 4, n // 3).astype(np.int64)
    x[: n // 3] = near.astype(np.uint32).view(np.float32) * rng.choice([-1.0, 1.0], n // 3).astype(np.float32)
    return x


def test_split3_emulation_is_lossless():
    """x = h + m + l exactly, every piece a bf16, and l + m, then + h (the order of x3_terms) exact in float32."""
    x = _values(100000, 1)
    h, m, l = R.split3(x)
    for p in (h, m, l):
        assert np.array_equal(R.bf16_rne(p), p)
    assert np.array_equal(h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64), x.astype(np.float64))
    lm = (l + m).astype(np.float32)
    assert np.array_equal(lm.astype(np.float64), l.astype(np.float64) + m.astype(np.float64))
    assert np.array_equal((lm + h).astype(np.float32), x)
    assert np.array_equal(R.bf16_rne(np.float32([1.00390625, 1.01171875, -1.00390625])), np.float32([1.0, 1.015625, -1.0]))     # ties to even


def test_f2_split_emulation_meets_the_stated_bound():
    """|x - (h + l) / s| <= max(|x| 2^-22, max|x| 2^-39) with s = f2_scale_of(max|x|); s puts the maximum into [2^14, 2^15);
    over-reported maxima keep the bound relative to what was reported."""
    x = _values(100000, 2)
    for over in (1.0, 2.0, 1024.0):
        amax = np.float32(np.abs(x).max() * over)
        s = R.f2_scale_of(amax)
        assert 2.0 ** 14 <= float(amax) * float(s) < 2.0 ** 15
        h, l = R.f2_split(x, s)
        assert np.isfinite(h.astype(np.float64)).all()
        err = np.abs((h.astype(np.float64) + l.astype(np.float64)) / float(s) - x.astype(np.float64))
        assert (err <= R.f2_bound(x, amax)).all()
    assert float(R.f2_scale_of(np.float32(0.0))) == 2.0 ** 127 == float(R.f2_scale_of(np.float32(1e-40)))
    ints = np.arange(-64, 65).astype(np.float32)               # integers: exact in the high piece under any scale in range
    for over in (1.0, 2.0, 1024.0):
        h, l = R.f2_split(ints, R.f2_scale_of(np.float32(64.0 * over)))
        assert not l.any() and np.array_equal(h.astype(np.float32) / R.f2_scale_of(np.float32(64.0 * over)), ints)


def test_input_builders():
    a = R.ints((33, 17), 64, 3)
    assert a.abs().max() == 64 and (a == a.round()).all() and (a[0] == 64).all()
    assert torch.equal(a.to(torch.bfloat16).float(), a)
    m, k, v = R.selection_rows(50, 24, 1)
    assert ((m != 0).sum(1) == 1).all() and torch.equal(m[torch.arange(50), k], v) and (torch.frexp(v)[0].abs() == 0.5).all()
    m, r, v = R.selection_cols(50, 24, 1)
    assert ((m != 0).sum(0) == 1).all() and ((m != 0).sum(1) <= 1).all() and torch.equal(m[r, torch.arange(24)], v)
    s = R.row_scales(320)
    assert s.min() == 2.0 ** -20 and s.max() == 2.0 ** 20 and len(set(s.tolist())) == 41
    f = R.full_mantissa((64, 64), 5)
    assert (f.abs() >= 1).all() and (f.abs() < 2).all()
    ar = R.Arena(torch.float32, "cpu", [(5, 7, 11, 2, 0), (0, 3, None, 0, 0), (4, 4, None, 0, 1)])
    assert ar.untouched()
    ar.t[0].fill_(1.0), ar.t[2].fill_(2.0)
    ar.check()
    ar.bodies[0][2, 9] = 0.0                                   # a guard column
    with pytest.raises(AssertionError, match="outside"):
        ar.check()
    p = R.place(a, 20, 2, 1)
    assert torch.equal(p, a) and p.stride() == (20, 1) and p.storage_offset() == 3


def test_wrappers_refuse_before_any_device_work():
    """gemm.py looks at .is_cuda first: host tensors are refused by every wrapper with an error, not a crash; the mode switch
    takes only its three names."""
    with pytest.raises(ValueError):
        gemm.set_fp32_mode("fp64")
    assert gemm.FP32_MODE in gemm.FP32_MODES
    a, b = torch.zeros(8, 32), torch.zeros(8, 32)
    for call in (lambda: gemm.gemm_nt(a, b), lambda: gemm.gemm_nt_grouped([(a, b, None)]), lambda: gemm.gemm_tn(a, b),
                 lambda: gemm.gemm_tn_grouped([(a, b)])):
        with pytest.raises(RuntimeError, match="CUDA"):
            call()
    with pytest.raises(TypeError, match="CUDA"):
        gemm.absmax(a)
    with pytest.raises(ValueError, match="amax"):
        gemm._use_amax(torch.zeros(1))
    lib = _lib.get_lib()
    assert lib.epn_gemm_nt_f16x2_workspace_bytes(0, None) == 0 and lib.epn_gemm_nt_split_workspace_bytes(0, None) == 0
    probs = (_lib.GemmNtProblem * 7)()
    for p in probs:
        p.N, p.K = 40, 32
    # seven problems = two launches: a 256-byte block of maxima per launch, planes [2][N][K] fp16 and N row maxima per problem
    assert lib.epn_gemm_nt_f16x2_workspace_bytes(7, probs) == 2 * 256 + 7 * (4 * 40 * 32 + 256)
    assert lib.epn_gemm_nt_split_workspace_bytes(7, probs) == 7 * 6 * 40 * 32
