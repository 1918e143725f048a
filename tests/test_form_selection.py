"""Which form does a layer take?  ops.select_inter_fwd / select_inter_bwd_data / select_intra on a table: every layer of the
three benchmarked schedules at the benchmark's batch sizes and dtypes, times the values of the switches the code honours,
plus the boundary cases the rules name.  The expectations are written out from the rules as documented (INTEGRATION.md
"Run-time switches") and as the launch traces of tools/launch_trace.py show them; library predicates are
stubbed with what the library answers for these shapes (it takes every cin % 16 == 0 layer of the schedules)."""
import pytest
import torch

from epn_pointcloud_amd import ops, schedule as S

F32, BF16 = torch.float32, torch.bfloat16
GB = 2 ** 30
DEVICE = 288 * GB                                          # MI355X
NETS = {"cls": (S.cls_so3net_schedule(1024), 32, 1024, F32), "reg": (S.reg_so3net_schedule(1024), 64, 1024, BF16),
        "inv": (S.inv_so3net_schedule(2048), 64, 2048, BF16)}


def yes():
    return True


def never():
    raise AssertionError("this predicate is not part of the rule that decides here")


def layers():
    """(net, index, layer, points after the layer's stride, feature dtype of the net)"""
    for net, (sched, batch, points, dtype) in NETS.items():
        p = points
        for i, l in enumerate(sched):
            p //= l.stride
            yield net, i, l, batch * p * 60 * l.cin * 24 * 4, dtype


def fwd(l, dtype, g_bytes, mode="auto", fp32_mode="f16x2", share=True, requires_grad=True, switch="1", dense=False, cuda=True,
        device=DEVICE, onchip=yes):
    dtype = F32 if l.cin == 1 else dtype                  # the occupancy features of the first layer are fp32 in every network
    return ops.select_inter_fwd(l.cin, dtype, dense, cuda, mode, fp32_mode, share, requires_grad, switch if share else None,
                                g_bytes, lambda: device, onchip)


@pytest.mark.parametrize("mode", ["auto", "split", "fused", "onchip"])
@pytest.mark.parametrize("fp32_mode", ["f16x2", "split", "native"])
def test_inter_forward_of_the_schedules(mode, fp32_mode):
    for net, i, l, g_bytes, dtype in layers():
        got = fwd(l, dtype, g_bytes, mode, fp32_mode)
        if l.cin == 1:
            want = ("fused", False)                        # the first layer: only the fused kernels take cin = 1
        elif mode in ("auto", "split"):
            want = ("split_shared", False)                 # a block's convolution: the skip branch's gradient is folded in
        elif mode == "onchip" and not (dtype == F32 and fp32_mode == "native"):
            want = ("onchip", False)
        elif dtype == BF16:
            want = ("split", False)                        # bf16 has no fused kernels
        else:
            want = ("fused", False)                        # EPN_INTER_MODE=fused; =onchip under the exact-f32 switch
        assert got == want, (net, i, mode, fp32_mode, got)
        # the same layer outside a block, with a frozen trunk, and with the fold switched off
        plain = fwd(l, dtype, g_bytes, mode, fp32_mode, share=False)
        assert plain == (("split", False) if want[0] == "split_shared" else want), (net, i, mode, plain)
        assert fwd(l, dtype, g_bytes, mode, fp32_mode, switch="0") == plain
        frozen = fwd(l, dtype, g_bytes, mode, fp32_mode, requires_grad=False)
        assert frozen == (("split_stats", False) if want[0] == "split_shared" else want), (net, i, mode, frozen)


def test_inter_forward_boundaries():
    L = S.Layer
    l64 = L(64, 64, 1, 0.2, 0.02, 16, True, 0)
    assert fwd(L(1, 64, 2, 0.2, 0.02, 32, False, 0), F32, 1, share=False) == ("fused", False)
    assert fwd(L(24, 64, 1, 0.2, 0.02, 16, True, 0), F32, 1) == ("fused", False)            # cin not a multiple of 16
    assert fwd(L(24, 64, 1, 0.2, 0.02, 16, True, 0), BF16, 1) == ("fused", True)            # ... bf16: fp32 kernels after a cast
    assert fwd(L(24, 64, 1, 0.2, 0.02, 16, True, 0), BF16, 1, mode="onchip", onchip=never) == ("fused", True)
    for mode in ("auto", "split", "onchip"):
        assert fwd(l64, F32, 1, mode=mode, dense=True, onchip=never) == ("fused", False)   # dense inter_w
    assert fwd(l64, BF16, 1, dense=True) == ("fused", True)
    # an eighth of the device: auto mode, fp32 features only; EPN_INTER_MODE=split and bf16 features are not limited
    assert fwd(l64, F32, DEVICE // 8) == ("split_shared", False)
    assert fwd(l64, F32, DEVICE // 8 + 1) == ("fused", False)
    assert fwd(l64, F32, DEVICE // 8, share=False) == ("split", False)
    assert fwd(l64, F32, DEVICE // 8 + 1, share=False) == ("fused", False)
    assert fwd(l64, F32, DEVICE // 8 + 1, mode="split") == ("split_shared", False)
    assert fwd(l64, BF16, DEVICE // 8 + 1) == ("split_shared", False)
    assert fwd(l64, F32, 3 * GB, device=16 * GB) == ("fused", False)                       # a small-memory part
    # a non-CUDA input: nothing asks for the device; the split Function itself rejects it
    cpu = dict(cuda=False, device=None, onchip=never)
    assert fwd(l64, F32, 1, **cpu) == ("split", False)
    assert fwd(l64, F32, 1, mode="onchip", **cpu) == ("fused", False)
    assert fwd(l64, torch.float64, 1, **cpu) == ("split", True)
    # the on-chip kernel declines a layer: the forms that write no grouped tensor either (fp32), the split form (bf16)
    assert fwd(l64, F32, 1, mode="onchip", onchip=lambda: False) == ("fused", False)
    assert fwd(l64, BF16, 1, mode="onchip", onchip=lambda: False) == ("split", False)
    assert fwd(l64, F32, 1, mode="fused", onchip=never) == ("fused", False)


def bwd(dtype, nn, cin=64, na=60, lazy=True, mode="auto", det=False, f16x2=True, cloud=yes, onchip=yes, fused=yes, write=yes):
    return ops.select_inter_bwd_data(dtype, nn, cin, na, lazy, mode, det, f16x2 and dtype == F32, cloud, onchip, fused, write)


@pytest.mark.parametrize("mode", ["auto", "cloud", "split", "onchip", "fused"])
@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("fp32_mode", ["f16x2", "split", "native"])
def test_inter_data_gradient_of_the_schedules(mode, det, fp32_mode):
    for net, i, l, _g, dtype in layers():
        if l.cin == 1:
            continue                                       # the first layer runs the fused Function: no split backward
        for dt in {dtype, F32}:                            # (the rotation network is also traced in fp32: K = 64)
            for shared in (True, False):                   # is there a private fp32 gradient of a shared input to write into?
                got = bwd(dt, l.nn, l.cin, mode=mode, det=det, f16x2=fp32_mode == "f16x2", write=lambda: shared)
                onto = shared and dt == F32 and not det
                if mode == "cloud" or (det and mode == "auto"):
                    want = ("cloud", False)
                elif det:
                    want = ("slab", False)                 # an explicit form in deterministic mode: the atomic-free transpose
                elif mode == "auto":
                    want = ("cloud", False) if dt == BF16 or l.nn <= 32 else ("scatter", onto)
                elif mode == "onchip" and dt == F32 and fp32_mode == "f16x2":
                    want = ("onchip", onto)
                elif mode == "fused" and dt == F32:
                    want = ("fused", False)
                else:
                    want = ("scatter", onto)
                assert got == want, (net, i, dt, mode, det, fp32_mode, shared, got)


def test_inter_data_gradient_boundaries():
    no = lambda: False                                     # noqa: E731
    assert bwd(F32, 32) == ("cloud", False) and bwd(F32, 64) == ("scatter", True)           # K = 32 vs 64 in fp32
    assert bwd(BF16, 64, write=never) == ("cloud", False)
    assert bwd(F32, 64, det=True, write=never) == ("cloud", False)
    # the cloud kernel declines (or dense inter_w: the library is not asked): scatter; deterministic: the slab reduction
    assert bwd(F32, 16, cloud=no) == ("scatter", True) and bwd(F32, 16, mode="cloud", cloud=no) == ("scatter", True)
    assert bwd(BF16, 16, cloud=no, write=never) == ("scatter", False)
    assert bwd(F32, 16, det=True, cloud=no, write=never) == ("slab", False)
    assert bwd(BF16, 16, det=True, cloud=no, write=never) == ("slab", False)
    assert bwd(F32, 16, na=12, det=True, cloud=no, write=never) == ("scatter", False)       # the slab kernels want na >= 16
    assert bwd(F32, 16, lazy=False, cloud=never) == ("scatter", True)
    assert bwd(F32, 16, lazy=False, det=True, cloud=never, write=never) == ("scatter", False)
    assert bwd(F32, 16, lazy=False, mode="onchip", cloud=never, onchip=never) == ("scatter", True)
    # explicit forms never ask the cloud predicate; a shared gradient somebody else can see is added afterwards
    assert bwd(F32, 16, mode="split", cloud=never, write=no) == ("scatter", False)
    assert bwd(F32, 16, mode="onchip", cloud=never, onchip=no) == ("scatter", True)
    assert bwd(F32, 16, mode="onchip", cloud=never, f16x2=False, onchip=never) == ("scatter", True)
    assert bwd(F32, 16, mode="fused", cloud=never, write=never) == ("fused", False)
    assert bwd(F32, 16, mode="fused", cloud=never, fused=no, write=never) == ("scatter", False)
    assert bwd(BF16, 16, mode="fused", cloud=never, fused=never, write=never) == ("scatter", False)
    assert bwd(BF16, 16, mode="onchip", cloud=never, onchip=never, write=never) == ("scatter", False)


@pytest.mark.parametrize("mode", ["auto", "spectral", "split", "fused"])
def test_intra_of_the_schedules(mode):
    for net, i, l, _g, dtype in layers():
        got = ops.select_intra(l.cout, l.cout, 12, True, mode, yes, dtype == BF16)
        if mode in ("auto", "spectral"):
            want = "spectral"                              # every width of the three schedules is a multiple of 32
        else:
            want = "split" if mode == "split" or dtype == BF16 else "fused"    # bf16 has no fused kernels
        assert got == want, (net, i, mode, got)


def test_intra_boundaries():
    no = lambda: False                                     # noqa: E731
    sel = ops.select_intra
    assert sel(64, 64, 12, True, "auto", no) == "split"                  # the table is no regular group action
    assert sel(64, 64, 12, False, "auto", never) == "split"              # non-CUDA
    assert sel(64, 64, 1, True, "auto", never) == "split"                # a single neighbour (1x1 convolution)
    assert sel(48, 64, 12, True, "auto", never) == "split"               # multiples of 16, not of 32
    assert sel(48, 64, 12, True, "fused", never) == "fused"
    assert sel(24, 64, 12, True, "auto", never) == "fused"               # not a multiple of 16: fp32 fused ...
    assert sel(24, 64, 12, True, "auto", never, True) == "split"         # ... bf16: multiples of 8 take the split form
    assert sel(20, 64, 12, True, "auto", never, True) == "fused"         # ... odd widths: fp32 kernels between two casts
    assert sel(20, 64, 12, True, "split", never) == "split"


def test_the_public_predicates_use_the_same_selection(monkeypatch):
    idx = torch.zeros(60, 12, dtype=torch.int32)
    asked = []
    monkeypatch.setattr(ops, "spectral_basis", lambda t: asked.append(t) or object())
    for mode, want in (("auto", True), ("spectral", True), ("split", False), ("fused", False)):
        monkeypatch.setenv("EPN_INTRA_MODE", mode)
        assert ops.intra_takes_spectral(64, 64, idx) is want
        assert ops.intra_takes_spectral(64, 48, idx) is False and ops.intra_takes_spectral(64, 64, idx, is_cuda=False) is False
    assert len(asked) == 2                                 # the table is looked at only where everything else holds
    assert ops.inter_mode.__doc__.count("onchip") and "select_inter_fwd" in ops.inter_mode.__doc__
