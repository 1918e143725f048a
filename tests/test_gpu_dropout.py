"""-m gpu: dropout inside the HIP norm passes (ops.norm_act(..., dropout=rate), csrc/glue.hip) -- the nn.Dropout that follows
norm + leaky_relu in every block of the reference (SPConvNets/utils/base_so3conv.py:58-59 / 124-125).

The mask is specified apart from the kernels (include/epn_so3conv.h; tests/philox_ref.py restates it in numpy), so every
comparison below is against a mask the test can name: bit for bit against the restatement, then the forward / backward values
against the stock torch modules driven with that same mask."""
import copy
import functools

import numpy as np
import pytest
import torch

import philox_ref as P
from conftest import unit_ball_cloud

pytestmark = pytest.mark.gpu
T = torch.from_numpy
RATE = 0.3
SEEDS = ((20240613, 0), ((7 << 32) + 12345, (1 << 33) + 5))     # (seed, call); the second: both above 2^32
SHAPE3 = (3, 37, 60)                                            # b, p, a of the kernel cases: 6660 rows, no multiple of any row step


def _close_except_kinks(a, b, tol, max_frac):
    """tests/test_gpu_conv.py's comparison: leaky_relu's kink lets a vanishing fraction of elements take the other sub-gradient."""
    err = (a - b).abs()
    bad = (err > tol * max(1.0, b.abs().max().item())).float().mean().item()
    return bad <= max_frac


def _norm(c, instance, gpu):
    norm = (torch.nn.InstanceNorm2d(c, affine=False) if instance else torch.nn.BatchNorm2d(c)).to(gpu).train()
    if not instance:
        gen = torch.Generator().manual_seed(c)
        with torch.no_grad():
            norm.weight.copy_(torch.rand(c, generator=gen) + 0.5)
            norm.bias.copy_(torch.rand(c, generator=gen) - 0.5)
    return norm


@functools.lru_cache(maxsize=None)
def _inputs(c, bf16):
    """(x, residual, dy) of a case, made once and shared by the forward and the backward test (never written to)."""
    gen = torch.Generator().manual_seed(1000 + c)
    b, p, a = SHAPE3
    dt = torch.bfloat16 if bf16 else torch.float32
    mk = lambda s, o: (torch.randn(b, c, p, a, generator=gen) * s + o).to(dt).cuda().contiguous(memory_format=torch.channels_last)
    return mk(2.0, 0.5), mk(1.0, 0.0), mk(1.0, 0.0)


def _bf16_ulp(v):
    """Spacing of bfloat16 at |v| (8 significand bits), elementwise; the smallest normal's for tiny values."""
    return torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126))) - 7)


@pytest.mark.parametrize("shape", [(2, 8, 5, 60), (1, 64, 3, 60)])
@pytest.mark.parametrize("rate", [0.1, 0.5])
@pytest.mark.parametrize("seed,call", SEEDS)
def test_mask_kernel_is_the_specification(gpu, shape, rate, seed, call):
    """ops.dropout_mask == the numpy restatement, bit for bit; a seed or call above 2^32 catches a truncated key / counter."""
    from epn_pointcloud_amd import ops
    st = torch.tensor([seed, call], dtype=torch.int64, device=gpu)
    m = ops.dropout_mask(*shape, rate, st)
    assert m.dtype == torch.bool and tuple(m.shape) == shape and m.is_contiguous(memory_format=torch.channels_last)
    want = P.keep_mask(*shape, rate, seed, call)
    assert np.array_equal(m.cpu().numpy(), want)
    assert torch.equal(ops.dropout_mask(*shape, rate, (seed, call)), m)       # (seed, call) as plain ints


def test_rates_outside_the_open_interval_raise(gpu):
    from epn_pointcloud_amd import ops
    x = _inputs(8, False)[0]
    norm = _norm(8, True, gpu)
    for bad in (1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            ops.norm_act(x, norm, dropout=bad)
        with pytest.raises(ValueError):
            ops.dropout_mask(1, 8, 2, 60, bad, (1, 0))
    with pytest.raises(ValueError):
        ops.dropout_mask(1, 8, 2, 60, 0.0, (1, 0))


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("instance", [False, True])
@pytest.mark.parametrize("c", [8, 64, 256])
def test_forward_is_the_masked_scaled_norm_act(gpu, c, instance, res, bf16):
    """y == where(m, ref / (1 - p), 0) + residual with m = ops.dropout_mask for the state before the call and
    ref = ops.norm_act without dropout; `call` advances by exactly 1; running statistics are those of a dropout-free call.
    c / 4 = 2, 16, 64 channel lanes of a 256-thread block.  fp32: 2e-6 * max(1, |.|) (scale and product round once each; the
    residual add may be contracted into an fma).  bf16: one bf16 ulp against the UNROUNDED reference, i.e. ops.norm_act on
    the same bf16 values held in fp32 -- the bf16 output of the dropout-free call is already rounded once, and scaling that
    by 1 / (1 - p) = 1.43 before the second rounding can leave up to 0.5 + 0.71 ulp between two correct results.  Where the
    residual cancels the masked value the fp32 bound is the floor: the bf16 kernels compute in fp32 and round once."""
    from epn_pointcloud_amd import ops
    x, r, _ = _inputs(c, bf16)
    r = r if res else None
    b, p, a = SHAPE3
    norm, plain = _norm(c, instance, gpu), _norm(c, instance, gpu)
    ops.seed_dropout(SEEDS[1][0], gpu)
    before = ops.dropout_state(gpu).clone()
    y = ops.norm_act(x, norm, residual=r, dropout=RATE)
    after = ops.dropout_state(gpu).clone()
    assert after.tolist() == [before[0].item(), before[1].item() + 1]
    assert y.dtype == x.dtype and y.is_contiguous(memory_format=torch.channels_last)
    assert getattr(y, "_epn_amax", None) is None          # no max|y| tag: the undropped tensor's maximum would be too small
    same_dtype = ops.norm_act(x, plain)
    ref = ops.norm_act(x.float(), _norm(c, instance, gpu)) if bf16 else same_dtype
    m = ops.dropout_mask(b, c, p, a, RATE, before)
    want = torch.where(m, ref / (1 - RATE), torch.zeros_like(ref)) + (r.float() if res else 0)
    err = (y.float() - want).abs()
    tol = 2e-6 * want.abs().clamp_min(1.0)
    if bf16:
        tol = torch.maximum(_bf16_ulp(want), tol)
    worst = (err / tol).max().item()
    print(f"c={c} instance={instance} res={res} bf16={bf16}: max err / tolerance = {worst:.3f}")
    assert worst <= 1.0
    if not res:
        assert torch.equal(y == 0, ~m)                    # dropped elements are exact zeros, kept ones are not
    if not instance:
        assert torch.equal(norm.running_mean, plain.running_mean) and torch.equal(norm.running_var, plain.running_var)
        assert norm.num_batches_tracked.item() == 1


def test_mask_statistics(gpu):
    """Kept fraction overall and per channel, and the agreement of two consecutive calls, each within 5 sigma of its binomial
    (tests/philox_ref.mask_statistics_failures); the seed is fixed and tests/test_dropout_cpu.py shows that the specification
    itself meets these bounds for it, so a failure here is the kernel's.  Re-seeding reproduces the first mask bit for bit."""
    from epn_pointcloud_amd import ops
    b, c, p, a = P.STAT_SHAPE
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(b, c, p, a, generator=gen).to(gpu)
    norm = _norm(c, True, gpu)

    def draw():
        return (ops.norm_act(x, norm, dropout=P.STAT_RATE) != 0).cpu().numpy()

    ops.seed_dropout(P.STAT_SEED, gpu)
    k = [draw(), draw()]
    assert not P.mask_statistics_failures(lambda call: k[call], P.STAT_SHAPE, P.STAT_RATE)
    ops.seed_dropout(P.STAT_SEED, gpu)
    assert np.array_equal(draw(), k[0])
    assert np.array_equal(k[0], P.keep_mask(b, c, p, a, P.STAT_RATE, P.STAT_SEED, 0))


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("instance", [False, True])
@pytest.mark.parametrize("c", [8, 64, 256])
def test_backward_vs_torch_autograd(gpu, c, instance, res, bf16):
    """dx, dresidual, dgamma, dbeta against torch autograd of m * leaky_relu(norm(x)) / (1 - p) + r on the stock modules (fp32),
    m from ops.dropout_mask: tolerance and kink allowance of test_gpu_conv.py::test_norm_act_kernels_vs_torch (fp32: 1e-3,
    1e-5 of the elements) and of that file's pair test for bf16 (5e-2, 2e-3).  The residual's gradient is dy itself."""
    from epn_pointcloud_amd import ops
    x0, r0, gy = _inputs(c, bf16)
    b, p, a = SHAPE3
    norm = _norm(c, instance, gpu)
    ref_norm = copy.deepcopy(norm)
    x = x0.clone().requires_grad_(True)
    r = r0.clone().requires_grad_(True) if res else None
    ops.seed_dropout(SEEDS[0][0], gpu)
    before = ops.dropout_state(gpu).clone()
    y = ops.norm_act(x, norm, residual=r, dropout=RATE)
    ins = [x] + ([r] if res else []) + list(norm.parameters())
    g = torch.autograd.grad(y, ins, gy)

    m = ops.dropout_mask(b, c, p, a, RATE, before)
    xr = x0.float().clone().requires_grad_(True)
    rr = r0.float().clone().requires_grad_(True) if res else None
    y_ref = torch.nn.functional.leaky_relu(ref_norm(xr)) * m / (1 - RATE) + (rr if res else 0)
    g_ref = torch.autograd.grad(y_ref, [xr] + ([rr] if res else []) + list(ref_norm.parameters()), gy.float())
    tol, frac = (5e-2, 2e-3) if bf16 else (1e-3, 1e-5)
    names = ["dx"] + (["dresidual"] if res else []) + [n for n, _ in norm.named_parameters()]
    for n, u, v in zip(names, g, g_ref):
        assert u.shape == v.shape
        assert _close_except_kinks(u.float(), v, tol, frac), n
    if res:
        assert torch.equal(g[1], gy)


class _MaskDropout(torch.nn.Module):
    """Stand-in for a stock block's nn.Dropout that applies the masks the HIP block draws: ops.dropout_mask for consecutive
    calls from a given (seed, call), scaled by 1 / (1 - p)."""

    def __init__(self, rate, state):
        super().__init__()
        self.p, self.seed, self.call = rate, int(state[0]), int(state[1])     # .p: as nn.Dropout

    def forward(self, t):
        from epn_pointcloud_amd import ops
        m = ops.dropout_mask(*t.shape, self.p, (self.seed, self.call))
        self.call += 1
        return t * m / (1 - self.p)


def _block_case(gpu, kind):
    from epn_pointcloud_amd import schedule as S
    if kind == "separable_bn_strided":
        return S.Layer(16, 32, 2, 0.4, 0.08, 16, False), "BatchNorm2d", 60, S.SeparableBlock, S.FusedSeparableBlock
    if kind == "separable_in":
        return S.Layer(32, 32, 1, 0.4, 0.08, 16, True), None, 60, S.SeparableBlock, S.FusedSeparableBlock
    return S.Layer(16, 32, 2, 0.4, 0.08, 16, False), "BatchNorm2d", 12, S.InterBlock, S.InterBlock


@pytest.mark.parametrize("kind", ["separable_bn_strided", "separable_in", "inter_block_12"])
def test_blocks_with_dropout_stay_on_hip(gpu, vgtk_alias, monkeypatch, kind):
    """A block with dropout_rate = 0.25 runs its glue on the dropout norm kernels -- no batch-norm, instance-norm or dropout
    ATen operator -- and computes what the stock-module block computes when its nn.Dropout is replaced by the same masks:
    outputs, input gradient, every parameter gradient and the running statistics, at the tolerance and kink allowance of
    test_gpu_conv.py::test_fused_block_matches_stock_block.  EPN_FUSED_DROPOUT=0 (A/B mode) takes the stock path and runs."""
    from epn_pointcloud_amd import ops
    import vgtk.spconv as zptk
    TOL, rate = 1e-3, 0.25
    l, norm, kanchor, stock_cls, hip_cls = _block_case(gpu, kind)
    rng = np.random.default_rng(5)
    xyz = T(unit_ball_cloud(rng, 2, 256)).to(gpu)
    torch.manual_seed(9)
    a = stock_cls(l, kanchor, norm, rate).to(gpu).train()
    b = hip_cls(l, kanchor, norm, rate).to(gpu).train()
    b.load_state_dict(a.state_dict())
    # (kanchor = 12 selects the block TYPE in the builders; the anchor set itself is the full one unless kanchor is 1, 20 or 40,
    # vgtk/vgtk/so3conv/functional.py:281-289 -- the features carry the convolution's own anchor count)
    na = (b.conv if kind == "inter_block_12" else b.inter_conv.conv).anchors.shape[0]
    feats = torch.randn(2, l.cin, 256, na, device=gpu)
    fa, fb = feats.clone().requires_grad_(True), feats.clone().requires_grad_(True)
    gy = torch.randn(2, l.cout, 256 // l.stride, na, device=gpu)

    ops.seed_dropout(SEEDS[1][0], gpu)
    before = ops.dropout_state(gpu).clone()
    ops.profile_begin()
    try:
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
            yb = b(zptk.SphericalPointCloud(xyz, fb, None))[3].feats
            gb = torch.autograd.grad(yb, [fb] + list(b.parameters()), gy)
            torch.cuda.synchronize()
    finally:
        rec = ops.profile_end()
    kernels = [r[5] for r in rec]
    for k in ("norm_act_dropout_fwd_kernel", "norm_act_dropout_bwd_reduce_kernel", "norm_act_dropout_bwd_apply_kernel"):
        assert any(k in name for name in kernels), (k, sorted(set(kernels)))
    aten = {e.key for e in prof.key_averages()}
    assert any(k.startswith("aten::") for k in aten)
    stock_ops = sorted(k for k in aten if k.startswith("aten::")
                       and ("batch_norm" in k or "instance_norm" in k or "dropout" in k or "bernoulli" in k))
    assert not stock_ops, stock_ops
    n_drop = 1 if kind == "inter_block_12" else 2
    assert ops.dropout_state(gpu).tolist() == [before[0].item(), before[1].item() + n_drop]

    # the stock modules with the same masks (InterBlock: the stock path of the same class, selected by the A/B switch)
    monkeypatch.setenv("EPN_AB", "1")
    monkeypatch.setenv("EPN_FUSED_DROPOUT", "0")
    a.dropout = _MaskDropout(rate, before)
    ya = a(zptk.SphericalPointCloud(xyz, fa, None))[3].feats
    ga = torch.autograd.grad(ya, [fa] + list(a.parameters()), gy)
    assert a.dropout.call == before[1].item() + n_drop
    assert (ya - yb).abs().max().item() < TOL
    for (n, _), u, v in zip([("feats", None)] + list(a.named_parameters()), ga, gb):
        assert _close_except_kinks(v, u, TOL, 1e-4), n
    for (n, u), (_, v) in zip(a.named_buffers(), b.named_buffers()):
        if "running" in n:
            assert torch.allclose(u, v, atol=1e-4), n

    # EPN_FUSED_DROPOUT=0: the HIP block class itself falls back to the stock modules (nn.Dropout) and runs
    calls = ops.dropout_state(gpu).clone()
    yc = b(zptk.SphericalPointCloud(xyz, feats, None))[3].feats
    assert torch.isfinite(yc).all() and (yc == 0).float().mean().item() < 0.5
    assert torch.equal(ops.dropout_state(gpu), calls)     # the HIP generator was not used


def test_graph_replay_draws_fresh_masks(gpu):
    """One forward + backward captured in a graph (a single chain on one stream), replayed twice: the two outputs are dropped
    where ops.dropout_mask says for calls n and n + 1 -- the state is read through its pointer, nothing of it is baked into the
    launches -- and each replay's backward used the mask of its OWN forward: its dx matches torch autograd through the stock
    modules with that replay's mask (tolerance of test_backward_vs_torch_autograd) and not with the other replay's.
    (dx is NOT zero where the output was dropped: a normalisation's input gradient carries the mean terms
    -rstd * (mean(dn) + xhat * mean(dn * xhat)) at every element, so the comparison is made on values.)"""
    from epn_pointcloud_amd import ops
    b, c, p, a = 2, 64, 9, 60
    gen = torch.Generator().manual_seed(17)
    x = (torch.randn(b, c, p, a, generator=gen) * 2 + 0.5).to(gpu).requires_grad_(True)
    gy = torch.randn(b, c, p, a, generator=gen).to(gpu)
    norm = _norm(c, False, gpu)

    def step():
        y = ops.norm_act(x, norm, dropout=RATE)
        (dx,) = torch.autograd.grad(y, [x], gy)
        return y, dx

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                            # warm-up: allocations and the generator state exist before capture
    torch.cuda.current_stream().wait_stream(side)
    ops.seed_dropout(SEEDS[1][0], gpu)
    before = ops.dropout_state(gpu).clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y, dx = step()
    assert torch.equal(ops.dropout_state(gpu), before)    # capturing launches nothing
    outs = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        outs.append((y.detach().clone(), dx.clone()))
    seed, call = before.tolist()
    assert ops.dropout_state(gpu).tolist() == [seed, call + 2]
    masks = [ops.dropout_mask(b, c, p, a, RATE, (seed, call + k)) for k in range(2)]
    assert not torch.equal(outs[0][0] == 0, outs[1][0] == 0)
    refs = []
    for k in range(2):
        assert torch.equal(outs[k][0] == 0, ~masks[k])
        xr = x.detach().clone().requires_grad_(True)
        ref_norm = copy.deepcopy(norm)
        y_ref = torch.nn.functional.leaky_relu(ref_norm(xr)) * masks[k] / (1 - RATE)
        refs.append(torch.autograd.grad(y_ref, [xr], gy)[0])
    for k in range(2):
        assert _close_except_kinks(outs[k][1], refs[k], 1e-3, 1e-5)
        assert not _close_except_kinks(outs[k][1], refs[1 - k], 1e-3, 1e-2)
