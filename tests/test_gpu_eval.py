"""-m gpu: eval()-mode inference on the HIP glue -- BatchNorm2d with frozen (running) statistics inside the norm kernels
(ops.norm_act_eval / norm_act_pair_eval / the pre_eval route of the intra convolution, csrc/glue.hip + csrc/so3_basis.hip), the
routing of the blocks (schedule.select_glue "eval") and the three networks in eval() under torch.no_grad().

References are the stock torch modules in eval mode (torch.nn.BatchNorm2d inside SPConvNets/utils/base_so3conv.py:168-212 /
:87-126 / :358-448) and the goldens of tests/golden/."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden, unit_ball_cloud
from test_gpu_dropout import _bf16_ulp, _block_case, _close_except_kinks
from test_gpu_models import close
from test_models_cpu import fill_state_dict, product_model

pytestmark = pytest.mark.gpu
T = torch.from_numpy
STOCK_NORM_OPS = ("batch_norm", "instance_norm", "dropout", "native_layer_norm")


def _stock_norm_ops(prof):
    aten = {e.key for e in prof.key_averages()}
    assert any(k.startswith("aten::") for k in aten)
    return sorted(k for k in aten if k.startswith("aten::") and any(s in k for s in STOCK_NORM_OPS))


@functools.lru_cache(maxsize=None)
def _frozen_case(shape, bf16, mean30):
    """(x, residual, BatchNorm2d in eval mode, conv_bias) of a case, made once and never written to.
    running_var uniform in [0.01, 2]; gamma = +-[0.5, 1.5] (both signs: with slope 0 half of the channels stay alive whatever the
    mean); beta in [-0.5, 0.5]; conv_bias = +-[0.05, 0.25], never 0.  running_mean = 0.3 * randn clipped to +-0.9, or 30
    everywhere with running_var = 0.01 (mean^2 / var = 9e4: statistics emulated as (sum x, sum x^2) lose var to 0.6 %).
    Why these magnitudes: the tolerance is 2e-6 * max(1, |want|) and the fp32 reference rounds x + bias before it subtracts the
    mean.  Where |want| <= 1 the input sits within ~0.15 of the mean, so |x + b| < 1.2 and that rounding is <= 6e-8, times
    rstd * |gamma| <= 15: 0.9e-6; the kernel's own mean - bias (|.| < 1.2) adds as much at most -- together inside 2e-6.  Where
    |want| > 1 every error is relative (a few 6e-8 roundings and a 1-ulp rsqrt).  In the mean = 30 case x stays ordinary, so
    |x + b - 30| ~ 30 and nothing cancels on either side."""
    b, c, p, a = shape
    gen = torch.Generator().manual_seed(c + 7 * p + (1000 if mean30 else 0))
    dt = torch.bfloat16 if bf16 else torch.float32
    mk = lambda s, o: (torch.randn(b, c, p, a, generator=gen) * s + o).to(dt).cuda().contiguous(memory_format=torch.channels_last)
    x, r = mk(2.0, 0.5), mk(1.0, 0.0)
    sign = lambda: torch.randint(0, 2, (c,), generator=gen).float() * 2 - 1
    norm = torch.nn.BatchNorm2d(c)
    with torch.no_grad():
        norm.weight.copy_((torch.rand(c, generator=gen) + 0.5) * sign())
        norm.bias.copy_(torch.rand(c, generator=gen) - 0.5)
        if mean30:
            norm.running_mean.fill_(30.0)
            norm.running_var.fill_(0.01)
        else:
            norm.running_mean.copy_((torch.randn(c, generator=gen) * 0.3).clamp_(-0.9, 0.9))
            norm.running_var.copy_(torch.rand(c, generator=gen) * 1.99 + 0.01)
        norm.num_batches_tracked.fill_(3)
    bias = ((torch.rand(c, generator=gen) * 0.2 + 0.05) * sign()).cuda()
    return x, r, norm.cuda().eval(), bias


@pytest.mark.parametrize("mean30", [False, True])
@pytest.mark.parametrize("slope", [0.01, 0.0])
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("shape", [(2, 8, 5, 60), (1, 64, 3, 60), (2, 256, 3, 60)])
def test_frozen_pass_is_the_eval_mode_module(gpu, shape, bf16, res, slope, mean30):
    """ops.norm_act_eval == leaky_relu(batch_norm(x + conv_bias, running statistics), slope) (+ residual) in fp32, at the tolerance
    of test_gpu_dropout.py::test_forward_is_the_masked_scaled_norm_act: 2e-6 * max(1, |want|), and for bf16 one bf16 ulp of the
    unrounded reference where that is larger.  The module's buffers are read, never written."""
    from epn_pointcloud_amd import ops
    x, r, norm, bias = _frozen_case(shape, bf16, mean30)
    r = r if res else None
    before = [t.clone() for t in (norm.running_mean, norm.running_var, norm.num_batches_tracked)]
    with torch.no_grad():
        y = ops.norm_act_eval(x, norm, residual=r, slope=slope, conv_bias=bias)
        want = F.leaky_relu(F.batch_norm(x.float() + bias.view(1, -1, 1, 1), norm.running_mean, norm.running_var, norm.weight,
                                         norm.bias, False, 0.0, norm.eps), slope)
        if res:
            want = want + r.float()
    assert y.dtype == x.dtype and y.is_contiguous(memory_format=torch.channels_last)
    assert getattr(y, "_epn_amax", None) is None          # no max|y| tag: the consumer scans
    err = (y.float() - want).abs()
    tol = 2e-6 * want.abs().clamp_min(1.0)
    if bf16:
        tol = torch.maximum(_bf16_ulp(want), tol)
    worst = (err / tol).max().item()
    print(f"shape={shape} bf16={bf16} res={res} slope={slope} mean30={mean30}: max err / tolerance = {worst:.3f}")
    assert worst <= 1.0
    assert (want != 0).float().mean().item() > 0.25       # the case is not an all-zero relu
    for u, v in zip(before, (norm.running_mean, norm.running_var, norm.num_batches_tracked)):
        assert torch.equal(u, v)


def test_eval_wrappers_are_forward_only(gpu):
    from epn_pointcloud_amd import ops
    x, _, norm, bias = _frozen_case((2, 8, 5, 60), False, False)
    with pytest.raises(RuntimeError, match="forward only"):
        ops.norm_act_eval(x.clone().requires_grad_(True), norm)
    with pytest.raises(RuntimeError, match="forward only"):
        ops.norm_act_eval(x, norm)                                   # the norm's own parameters require grad
    with pytest.raises(TypeError):
        with torch.no_grad():
            ops.norm_act_eval(x, torch.nn.InstanceNorm2d(8, affine=True).cuda().eval())
    assert ops.norm_eval_kind(norm) == "frozen"
    assert ops.norm_eval_kind(torch.nn.InstanceNorm2d(8)) == "batch"
    assert ops.norm_eval_kind(torch.nn.BatchNorm2d(8, track_running_stats=False)) == "batch"
    assert ops.norm_eval_kind(torch.nn.InstanceNorm2d(8, track_running_stats=True)) is None
    assert ops.norm_eval_kind(torch.nn.GroupNorm(2, 8)) is None


def _randomise_running_stats(module, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                c = m.num_features
                m.running_mean.copy_((torch.randn(c, generator=gen) * 0.3).to(m.running_mean.device))
                m.running_var.copy_((torch.rand(c, generator=gen) + 0.5).to(m.running_var.device))
                m.num_batches_tracked.fill_(5)
                m.weight.copy_((torch.rand(c, generator=gen) + 0.5).to(m.weight.device))
                m.bias.copy_((torch.rand(c, generator=gen) - 0.5).to(m.bias.device))


@pytest.mark.parametrize("rate", [0.0, 0.25])
@pytest.mark.parametrize("kind", ["separable_bn_strided", "separable_in", "inter_block_12"])
def test_blocks_stay_on_hip_in_eval(gpu, vgtk_alias, monkeypatch, kind, rate):
    """A block in eval() under no_grad runs its glue on the HIP norm passes -- no batch-norm, instance-norm, dropout or
    layer-norm ATen operator, a frozen kernel where the block has BatchNorm2d -- and computes what the stock modules compute
    (< 1e-3 absolute, the TOL of test_gpu_conv.py::test_fused_block_matches_stock_block), with or without a dropout module;
    buffers and the dropout generator are untouched.  EPN_FUSED_EVAL=0 (A/B mode): the stock path, same values."""
    from epn_pointcloud_amd import ops
    import vgtk.spconv as zptk
    TOL = 1e-3
    l, norm, kanchor, stock_cls, hip_cls = _block_case(gpu, kind)
    rng = np.random.default_rng(5)
    xyz = T(unit_ball_cloud(rng, 2, 256)).to(gpu)
    torch.manual_seed(9)
    a = stock_cls(l, kanchor, norm, rate).to(gpu)
    _randomise_running_stats(a, 11)
    b = hip_cls(l, kanchor, norm, rate).to(gpu)
    b.load_state_dict(a.state_dict())
    a.eval(), b.eval()
    na = (b.conv if kind == "inter_block_12" else b.inter_conv.conv).anchors.shape[0]
    feats = torch.randn(2, l.cin, 256, na, device=gpu)
    buffers = {n: t.clone() for n, t in b.named_buffers()}
    drop_state = ops.dropout_state(gpu).clone()

    ops.profile_begin()
    try:
        with torch.no_grad(), torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
            yb = b(zptk.SphericalPointCloud(xyz, feats, None))[3].feats
            torch.cuda.synchronize()
    finally:
        rec = ops.profile_end()
    assert not _stock_norm_ops(prof), _stock_norm_ops(prof)       # (the part that fails without the eval route)
    kernels = sorted({r[5] for r in rec})
    if norm == "BatchNorm2d":
        assert any("frozen" in k for k in kernels), kernels
    for n, t in b.named_buffers():
        assert torch.equal(t, buffers[n]), n
    assert torch.equal(ops.dropout_state(gpu), drop_state)

    monkeypatch.setenv("EPN_AB", "1")
    monkeypatch.setenv("EPN_FUSED_EVAL", "0")
    with torch.no_grad(), torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
        ya = a(zptk.SphericalPointCloud(xyz, feats, None))[3].feats
        yc = b(zptk.SphericalPointCloud(xyz, feats, None))[3].feats
    assert _stock_norm_ops(prof)                                  # the switch took the stock modules
    print(f"{kind} rate={rate}: max |hip - stock| = {(ya - yb).abs().max().item():.3e}, kernels: {kernels}")
    assert (ya - yb).abs().max().item() < TOL
    assert (ya - yc).abs().max().item() < TOL
    assert torch.equal(ops.dropout_state(gpu), drop_state)


def test_eval_with_grad_enabled_is_the_stock_route(gpu, vgtk_alias):
    """eval() with grad enabled (fine-tuning with frozen BatchNorm): the frozen passes have no backward, the block keeps the stock
    modules -- gradients exist and equal the stock class's at the tolerances of the block test above."""
    import vgtk.spconv as zptk
    l, norm, kanchor, stock_cls, hip_cls = _block_case(gpu, "separable_bn_strided")
    rng = np.random.default_rng(5)
    xyz = T(unit_ball_cloud(rng, 2, 256)).to(gpu)
    torch.manual_seed(9)
    a = stock_cls(l, kanchor, norm, 0.0).to(gpu)
    _randomise_running_stats(a, 11)
    b = hip_cls(l, kanchor, norm, 0.0).to(gpu)
    b.load_state_dict(a.state_dict())
    a.eval(), b.eval()
    feats = torch.randn(2, l.cin, 256, 60, device=gpu)
    fa, fb = feats.clone().requires_grad_(True), feats.clone().requires_grad_(True)
    gy = torch.randn(2, l.cout, 128, 60, device=gpu)
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
        yb = b(zptk.SphericalPointCloud(xyz, fb, None))[3].feats
    assert any("batch_norm" in k for k in _stock_norm_ops(prof))
    ya = a(zptk.SphericalPointCloud(xyz, fa, None))[3].feats
    gb = torch.autograd.grad(yb, [fb] + list(b.parameters()), gy)
    ga = torch.autograd.grad(ya, [fa] + list(a.parameters()), gy)
    assert (ya - yb).abs().max().item() < 1e-3
    for (n, _), u, v in zip([("feats", None)] + list(a.named_parameters()), ga, gb):
        assert v is not None and _close_except_kinks(v, u, 1e-3, 1e-4), n


def test_cls_network_in_eval_vs_reference_golden(gpu):
    g = golden("model_cls_tiny.npz")
    m = fill_state_dict(product_model("cls")).to(gpu).eval()
    with torch.no_grad(), torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
        logits_eval, _ = m(T(g["pts"]).to(gpu))
    assert close(logits_eval, g["logits_eval"])
    # every BatchNorm2d of the network (backbone blocks, the head's mlp) ran frozen on HIP: the one batch_norm operator left is
    # the head's BatchNorm1d on its [b, c, a] tensor, which stays on torch (models.ClsOutBlockPointnet)
    ev = [e for e in prof.key_averages() if e.key == "aten::batch_norm"]
    assert len(ev) == 1 and ev[0].count == 1, [(e.key, e.count) for e in prof.key_averages() if "norm" in e.key]
    assert not [k for k in _stock_norm_ops(prof) if "batch_norm" not in k]


def test_reg_and_inv_networks_in_eval_vs_reference_goldens(gpu):
    """InstanceNorm2d(affine=False) without running statistics everywhere: eval arithmetic is train arithmetic, so the outputs
    meet the goldens (and tolerances) of the train-mode tests -- on the HIP glue, no instance_norm operator."""
    g = golden("model_reg_tiny.npz")
    m = fill_state_dict(product_model("reg")).to(gpu).eval()
    with torch.no_grad(), torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
        conf, quats = m(T(g["pairs"]).to(gpu))
    assert not _stock_norm_ops(prof), _stock_norm_ops(prof)
    assert close(conf, g["confidence"], 3e-3)
    assert close(quats, g["quats"])
    g = golden("model_inv_tiny.npz")
    m = fill_state_dict(product_model("inv")).to(gpu).eval()
    with torch.no_grad(), torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
        desc, attn = m(T(g["pts"]).to(gpu))
    assert not _stock_norm_ops(prof), _stock_norm_ops(prof)
    assert close(desc, g["descriptor"])
    assert close(attn[:, :, ::8], g["attention_sub"])


def test_graph_replay_follows_the_running_statistics(gpu):
    """norm_act_eval captured in a graph (a single chain on one stream): the statistics are read through the module's buffers
    by a kernel inside the graph, so a replay after an in-place change of running_mean computes with the new mean."""
    from epn_pointcloud_amd import ops
    b, c, p, a = 2, 64, 9, 60
    gen = torch.Generator().manual_seed(17)
    x = (torch.randn(b, c, p, a, generator=gen) * 2 + 0.5).to(gpu)
    norm = torch.nn.BatchNorm2d(c).to(gpu).eval()
    with torch.no_grad():
        norm.running_mean.copy_(torch.randn(c, generator=gen).to(gpu) * 0.3)
        norm.running_var.copy_(torch.rand(c, generator=gen).to(gpu) + 0.5)
    bias = (torch.rand(c, generator=gen) * 0.2 + 0.05).to(gpu)

    def ref():
        return F.leaky_relu(F.batch_norm(x + bias.view(1, -1, 1, 1), norm.running_mean, norm.running_var, norm.weight, norm.bias,
                                         False, 0.0, norm.eps))

    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ops.norm_act_eval(x, norm, conv_bias=bias)         # warm-up: allocations exist before capture
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = ops.norm_act_eval(x, norm, conv_bias=bias)
        graph.replay()
        torch.cuda.synchronize()
        y0, want0 = y.clone(), ref()
        norm.running_mean.add_(1.5)
        graph.replay()
        torch.cuda.synchronize()
        y1, want1 = y.clone(), ref()
    # the tolerance of the frozen-pass test: rstd * gamma <= 1.5 here, so the roundings of x + b and mean - b (|.| < 8: 5e-7)
    # stay inside it although the shifted mean is no longer small
    tol = lambda w: 2e-6 * w.abs().clamp_min(1.0)
    assert ((y0 - want0).abs() <= tol(want0)).all()
    assert ((y1 - want1).abs() <= tol(want1)).all()
    assert (y1 - y0).abs().max().item() > 0.5                  # and the two replays differ by the shift of the mean


def test_frozen_entry_points_reject_bad_arguments(gpu):
    """The C entries' own checks, as tests/test_gpu_models.py::test_pointnet_rejects_bad_arguments makes them: c % 4 != 0 (or
    c / 4 not dividing 256) is EPN_EINVAL (-1), a NULL stats / output pointer EPN_ENULL (-3)."""
    from epn_pointcloud_amd import _lib
    lib = _lib.get_lib()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    x = torch.zeros(2 * 60 * 24, device=gpu)
    y = torch.zeros_like(x)
    st = torch.ones(24, 2, device=gpu)
    for fn in (lib.epn_norm_act_frozen_fwd_f32, lib.epn_norm_act_frozen_fwd_bf16):
        assert fn(vp(x), 120, 6, vp(st), None, None, None, 1e-5, 0.01, vp(y), None) == -1      # c % 4
        assert fn(vp(x), 120, 24, vp(st), None, None, None, 1e-5, 0.01, vp(y), None) == -1     # 256 % (c / 4)
        assert fn(vp(x), 120, 8, None, None, None, None, 1e-5, 0.01, vp(y), None) == -3
        assert fn(vp(x), 120, 8, vp(st), None, None, None, 1e-5, 0.01, None, None) == -3
        assert fn(vp(x), 120, 8, vp(st), None, None, None, 1e-5, 0.01, vp(y), None) == 0
    assert lib.epn_bn_frozen_stats_f32(vp(st), vp(st), None, 0, vp(y), None) == -1
    assert lib.epn_bn_frozen_stats_f32(vp(st), None, None, 8, vp(y), None) == -3
    assert lib.epn_bn_frozen_stats_f32(vp(st), vp(st), None, 8, None, None) == -3
    sa, sb = _lib.NormPairSide(), _lib.NormPairFrozenSide()
    sa.sums, sa.eps, sa.instance = vp(st), 1e-5, 1
    sb.stats, sb.eps, sb.frozen = vp(st), 1e-5, 1
    pair = lambda c, a_, b_, out: lib.epn_norm_act_pair_frozen_fwd(vp(x), vp(x), 2, 60, c, a_, b_, 0.01, out, 0, None)
    assert pair(6, ctypes.byref(sa), ctypes.byref(sb), vp(y)) == -1
    assert pair(8, ctypes.byref(sa), None, vp(y)) == -3
    assert pair(8, ctypes.byref(sa), ctypes.byref(sb), None) == -3
    sb.stats = None
    assert pair(8, ctypes.byref(sa), ctypes.byref(sb), vp(y)) == -3
    # norm on load: the transform's own sizes (c % 32), NULL statistics / output
    M = torch.eye(60, device=gpu)
    blk = torch.zeros(60, 2, dtype=torch.int32, device=gpu)
    xin = torch.zeros(2 * 60 * 32, device=gpu)
    for fn in (lib.epn_so3_basis_norm_frozen_f32, lib.epn_so3_basis_norm_frozen_split_f32, lib.epn_so3_basis_norm_frozen_bf16):
        assert fn(vp(xin), vp(M), vp(blk), 2, 60, 24, 0, vp(xin), vp(st), None, None, 1e-5, 0.01, None) == -1
        assert fn(vp(xin), vp(M), vp(blk), 2, 60, 32, 0, vp(xin), None, None, None, 1e-5, 0.01, None) == -3
        assert fn(vp(xin), vp(M), vp(blk), 2, 60, 32, 0, None, vp(st), None, None, 1e-5, 0.01, None) == -3
    torch.cuda.synchronize()
