"""The norm glue without a device: the float64 restatement tests/norm_ref.py against torch's own modules in double (it has to be
right before tests/test_gpu_norm_fp64.py uses it as a judge), the two input builders on every case of that file, the floor of
the fp32 one-pass variance, and the host-only plan of the launchers (workspace queries, argument checks).

The floor (norm_ref.one_pass_fp32: float32 roundings of the EXACT sums, var = fl(fl(s2 / n) - fl(m m))), relative error of var
over 64 channels x 4096 rows, channel means kappa x std (max over the channels / root mean square):
    kappa   0: 6.6e-08 / 3.1e-08        kappa  10: 1.8e-05 / 6.6e-06
    kappa   1: 2.2e-07 / 7.6e-08        kappa 300: 1.1e-02 / 5.7e-03     ("0.6 % of var at mean 30, var 0.01")
i.e. about 2^-24 (1 + kappa^2), which no fp32 kernel of this form can beat."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import norm_ref as R
import norm_cases as G
from epn_pointcloud_amd import _lib, ops

F64 = torch.float64
EINVAL = -1


def _module(kind, c, affine, momentum, seed):
    torch.manual_seed(seed)
    m = (torch.nn.InstanceNorm2d(c, affine=False) if kind == "instance" else torch.nn.BatchNorm2d(c, affine=affine, momentum=momentum))
    m = m.double()
    if kind == "batch":
        with torch.no_grad():
            m.running_mean.normal_(); m.running_var.uniform_(0.5, 2.0)
            if affine:
                m.weight.uniform_(-1.5, 1.5); m.bias.uniform_(-0.5, 0.5)
    return m


@pytest.mark.parametrize("momentum", (0.1, None))
@pytest.mark.parametrize("kind,affine", (("batch", True), ("batch", False), ("instance", False)))
def test_norm_ref_matches_torch_double(kind, affine, momentum):
    """norm_act_ref / grads / running_update_ref against nn.BatchNorm2d and nn.InstanceNorm2d in double: training forward with a
    residual, autograd gradients, two running updates (momentum 0.1 and None), then the eval forward on the running statistics."""
    shape, slope = (3, 5, 7, 4), 0.2
    mod = _module(kind, 5, affine, momentum, 1)
    torch.manual_seed(2)
    rm, rv, nb = ((mod.running_mean.clone(), mod.running_var.clone(), 0) if kind == "batch" else (None, None, 0))
    for step in range(2):
        x = (torch.randn(shape, dtype=F64) * 2 + 0.7).requires_grad_(True)
        r = torch.randn(shape, dtype=F64, requires_grad=True)
        dy = torch.randn(shape, dtype=F64)
        params = [mod.weight, mod.bias] if affine else []
        y_t = torch.nn.functional.leaky_relu(mod(x), slope) + r
        g_t = torch.autograd.grad(y_t, [x, r] + params, dy)
        xr, rr = x.detach().clone().requires_grad_(True), r.detach().clone().requires_grad_(True)
        gm = mod.weight.detach().clone().requires_grad_(True) if affine else None
        bt = mod.bias.detach().clone().requires_grad_(True) if affine else None
        out = R.norm_act_ref(xr, kind, gm, bt, mod.eps, slope, rr)
        g_r = R.grads(out.y, [xr, rr, gm, bt], dy)
        assert torch.allclose(out.y, y_t, rtol=1e-12, atol=1e-12)
        for u, v in zip([t for t in g_r if t is not None], g_t):
            assert torch.allclose(u, v, rtol=1e-10, atol=1e-12)
        # dsums is what the two-pass backward is built from: dx = rstd (dn - mean(dn) - xhat mean(dn xhat))
        groups, rows = G.groups_rows(kind, shape)
        ds = R.dsums_ref(out, dy, kind, gm, slope).reshape((groups, 5, 1, 1, 2) if kind == "instance" else (1, 5, 1, 1, 2))
        dn = dy * torch.where(out.n > 0, torch.ones_like(dy), torch.full_like(dy, slope)) * (gm.reshape(1, -1, 1, 1) if affine else 1.0)
        rstd = 1.0 / torch.sqrt(out.var + mod.eps)
        dx = rstd * (dn - ds[..., 0] / rows - out.xhat * ds[..., 1] / rows)
        assert torch.allclose(dx, g_t[0], rtol=1e-10, atol=1e-12)
        if kind == "batch":
            rm, rv, nb = R.running_update_ref(out.sums[0], rows, None, rm, rv, nb, momentum)
            assert torch.allclose(rm, mod.running_mean, rtol=1e-12, atol=1e-14)
            assert torch.allclose(rv, mod.running_var, rtol=1e-12, atol=1e-14)
            assert nb == int(mod.num_batches_tracked) == step + 1
    if kind == "batch":
        ev = copy.deepcopy(mod).eval()
        x = torch.randn(shape, dtype=F64)
        bias = torch.randn(5, dtype=F64)
        want = torch.nn.functional.leaky_relu(ev(x + bias.reshape(1, -1, 1, 1)), slope)
        out = R.norm_act_ref(x, "frozen", ev.weight if affine else None, ev.bias if affine else None, ev.eps, slope,
                             conv_bias=bias, frozen_stats=(ev.running_mean, ev.running_var))
        assert torch.allclose(out.y, want.detach(), rtol=1e-12, atol=1e-12)


def test_norm_ref_conv_bias_mask_and_pair():
    """The remaining arguments: a conv_bias the training kinds cancel (y unchanged, sums those of x), the mask before the residual,
    the pair form as the sum of its two sides."""
    torch.manual_seed(3)
    shape = (2, 4, 6, 5)
    x, r = torch.randn(shape, dtype=F64), torch.randn(shape, dtype=F64)
    bias = torch.randn(4, dtype=F64)
    a = R.norm_act_ref(x, "batch", conv_bias=bias)
    b = R.norm_act_ref(x, "batch")
    assert torch.allclose(a.y, b.y, rtol=1e-12, atol=1e-13) and torch.equal(a.sums, b.sums)
    assert torch.allclose(b.sums[0, :, 0], x.sum((0, 2, 3))) and torch.allclose(b.sums[0, :, 1], (x * x).sum((0, 2, 3)))
    mask = torch.rand(shape) < 0.75
    m = R.norm_act_ref(x, "instance", residual=r, mask=mask, rate=0.25)
    plain = R.norm_act_ref(x, "instance")
    assert torch.allclose(m.y, plain.y * mask / 0.75 + r)
    assert m.sums.shape == (2, 4, 2)
    pr = R.norm_act_pair_ref(x, r, "instance", "batch")
    assert torch.allclose(pr.y, plain.y + R.norm_act_ref(r, "batch").y)


def test_exact_inputs_keep_every_sum_below_2_24():
    """For every shape of the GPU file: integer x in [-3, 3], sum x^2 per group and channel below 2^24 (so is |sum x|); dy is an
    integer times a power of two; both are exact in bf16."""
    for kind, shape in G.SINGLE:
        groups, rows = G.groups_rows(kind, shape)
        x, dy = R.exact_inputs(shape, seed=shape[1] + rows)
        assert bool((x == x.round()).all()) and float(x.abs().max()) <= 3 and 9 * rows < 2 ** 24
        sums = R.stats(x, kind)[2]
        assert sums.shape == (groups, shape[1], 2) and float(sums.abs().max()) < 2 ** 24
        for t in (x, dy):
            assert torch.equal(t, t.float().bfloat16().to(F64))


@pytest.mark.parametrize("c", G.WIDTHS)
def test_real_inputs_leave_nothing_near_the_kink(c):
    """For every (shape, kappa, dtype) of the GPU file's accuracy test: zero elements whose float64 pre-activation lies within
    tau = 4 x the forward tolerance, the values are exact in the dtype, and the channel statistics are what kappa asks for."""
    for kind, shape in [s for s in G.SINGLE if s[1][1] == c]:
        groups, rows = G.groups_rows(kind, shape)
        for dtype in G.DTYPES:
            for kappa in G.KAPPAS:
                affine = kind == "batch"
                x, left, gamma, beta, _, P, _ = G.single_inputs(kind, shape, dtype, kappa, G.single_seed(shape, kappa), affine)
                assert left == 0, (kind, shape, dtype, kappa)
                assert P <= 300
                assert torch.equal(x, x.float().to(dtype).to(F64))
                if rows > 1:
                    o = R.norm_act_ref(x, kind, gamma, beta, G.EPS)
                    tau = G.tau_fn(P, rows, gamma, dtype == torch.bfloat16)(o)
                    assert bool((o.n.abs() >= tau).all())
                if rows >= 4096 and dtype == torch.float32:
                    k = (o.mean / o.var.sqrt()).flatten()
                    assert float((k - kappa).abs().max()) < 0.1 * (1 + kappa)


@pytest.mark.parametrize("side_b", G.PAIR_SIDES, ids=lambda s: f"{s[0]}-{'affine' if s[1] else 'plain'}")
def test_pair_inputs_leave_nothing_near_the_kink(side_b):
    for shape in G.PAIR:
        for dtype in G.DTYPES:
            _, la, _, lb = G.pair_inputs(shape, side_b, dtype)
            assert la == 0 and lb == 0, (shape, dtype)


def test_frozen_inputs_leave_nothing_near_the_kink():
    """The frozen forward (every batch shape, with and without conv_bias) and the frozen pair side: nothing within tau of T(0)."""
    for kind, shape in [s for s in G.SINGLE if s[0] == "batch"]:
        for dtype in G.DTYPES:
            for use_bias in (False, True):
                x, left, gamma, beta, _, _, _, fs, P = G.frozen_inputs(shape, dtype, use_bias)
                assert left == 0, (shape, dtype, use_bias)
                o = R.norm_act_ref(x, "frozen", gamma, beta, G.EPS, frozen_stats=fs)
                tau = G.tau_fn(P, shape[0] * shape[2] * shape[3], gamma, dtype == torch.bfloat16, frozen=True)(o)
                assert bool((o.n.abs() >= tau).all()) and torch.equal(x, x.float().to(dtype).to(F64))
                assert float((o.xhat.abs()).max()) < 8
    for shape in G.PAIR:
        for dtype in G.DTYPES:
            for affine_b in (True, False):
                assert G.pair_frozen_inputs(shape, affine_b, dtype)[1] == 0


def test_forms_inputs_leave_nothing_near_the_kink():
    """The option runs of test_forms_vs_fp64 that move the statistics or the parameters: conv_bias, no affine pair."""
    for kind, shape in G.FORMS:
        seed = shape[1] + shape[2]
        for dtype in G.DTYPES:
            for s, kw in ((seed, {}), (seed + 3, dict(conv_bias=True))):
                assert G.single_inputs(kind, shape, dtype, 1, s, kind == "batch", **kw)[1] == 0
            if kind == "batch":
                assert G.single_inputs(kind, shape, dtype, 1, seed + 5, False)[1] == 0


def test_one_pass_floor():
    """The floors in this module's docstring and DESIGN 4, measured from the restatement alone; the kappa = 300 value is DESIGN
    3.4's "0.6 %" within a factor of 2; and every forward bound 4 T(kappa) of the GPU file is at least 2 x the floor's effect on y
    (half its relative error of var), for the smallest P of any case."""
    pmin = min(R.roundings(*G.groups_rows(k, s), s[1]) for k, s in G.SINGLE)
    pmax = max(R.roundings(*G.groups_rows(k, s), s[1]) for k, s in G.SINGLE)
    assert pmax <= 300
    got = {}
    for kappa in (0, 1, 10, 300):
        x, _ = R.real_inputs((1, 64, 4096, 1), kappa, 0, 0.0)
        x = x[0, :, :, 0].T.numpy()
        got[kappa] = (R.one_pass_floor(x, "max"), R.one_pass_floor(x, "rms"))
        bound = 4 * pmin * R.U * (1 + kappa ** 2)
        print(f"kappa {kappa}: floor max {got[kappa][0]:.2e} rms {got[kappa][1]:.2e}; y bound / floor effect: "
              f"{bound / (0.5 * got[kappa][0]):.0f} (P = {pmin}) .. {bound * pmax / pmin / (0.5 * got[kappa][0]):.0f} (P = {pmax})")
        assert bound >= 2 * 0.5 * got[kappa][0]
        assert 0.25 * R.U * (1 + kappa ** 2) < got[kappa][1] < got[kappa][0] < 4 * R.U * (1 + kappa ** 2)
    assert 0.003 <= got[300][1] <= 0.012
    # DESIGN's own operating point: mean 30, var 0.01
    g = torch.Generator().manual_seed(0)
    x = (30.0 + 0.1 * torch.randn(4096, 64, generator=g, dtype=F64)).float().to(F64).numpy()
    assert 0.003 <= R.one_pass_floor(x, "rms") <= 0.012
    # one_pass_fp32 is what it says: exact sums, three float32 roundings
    m, v = R.one_pass_fp32(x)
    s1, s2 = np.float32(x.sum(0)), np.float32((x * x).sum(0))
    assert m.dtype == np.float32 and np.array_equal(m, s1 / np.float32(4096))
    assert np.array_equal(v, np.float32(s2 / np.float32(4096)) - np.float32(m * m))


# ---- the host-only plan ---------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def test_supported_widths_are_the_launcher_s():
    """epn_norm_workspace_bytes(1, 64, c) != 0 exactly where ops.norm_act_supported(c): c / 4 a power of two up to 256."""
    lib = _lib.get_lib()
    want = {4 << k for k in range(9)}
    for c in range(1, 2050):
        ok = lib.epn_norm_workspace_bytes(1, 64, c) != 0
        assert ok == bool(ops.norm_act_supported(c)) == (c in want), c


@pytest.mark.parametrize("groups", (1, 3, 16, 1024, 1025))
def test_norm_workspace_is_the_block_plan(groups):
    """bytes = groups x blocks x c x 8 with blocks = ceil(rows / max(64, ceil(rows / ceil(1024 / groups)))): about 1024 blocks in
    total, never fewer than 64 rows each (make_norm; include/epn_so3conv.h); norm_ref.geometry restates the same rule."""
    lib = _lib.get_lib()
    for rows in (1, 64, 65, 4096, 4100, 65536, 65537):
        for c in (4, 64, 1024):
            blocks = _cdiv(rows, max(64, _cdiv(rows, _cdiv(1024, groups))))
            assert lib.epn_norm_workspace_bytes(groups, rows, c) == groups * blocks * c * 8, (groups, rows, c)
            assert R.geometry(groups, rows, c)[:2] == (max(64, _cdiv(rows, _cdiv(1024, groups))), blocks)
            assert lib.epn_norm_pair_workspace_bytes(groups, rows, c) == 2 * groups * blocks * c * 8
    assert R.geometry(16, 4100, 64) == (65, 64, 16) and 4100 - 63 * 65 == 5
    assert R.geometry(1, 257, 4) == (64, 5, 256) and R.geometry(1, 257, 1024)[2] == 1


def test_stats_finish_workspace_switches_at_2048_blocks():
    lib = _lib.get_lib()
    for groups in (1, 3):
        for c in (1, 7, 1024):
            for blocks in (1, 16, 2047, 2048):
                assert lib.epn_stats_finish_workspace_bytes(groups, blocks, c) == 0
            for blocks in (2049, 2304, 2305, 4097, 30720):
                assert lib.epn_stats_finish_workspace_bytes(groups, blocks, c) == groups * _cdiv(blocks, 256) * c * 8


def test_argument_checks_need_no_device():
    """Widths and group counts the launchers refuse return EPN_EINVAL before any pointer is looked at or any runtime call made."""
    lib = _lib.get_lib()
    z, sz = None, ctypes.c_size_t(0)
    for groups, c in ((1, 12), (1, 48), (1, 96), (1, 2048), (65536, 64)):
        assert lib.epn_norm_workspace_bytes(groups, 64, c) == 0
        assert lib.epn_chan_stats_f32(z, groups, 64, c, z, z, sz, z) == EINVAL
        assert lib.epn_chan_stats_bf16(z, groups, 64, c, z, z, sz, z) == EINVAL
        assert lib.epn_norm_act_fwd_f32(z, groups, 64, c, z, z, z, z, 1e-5, 0.01, z, z) == EINVAL
        assert lib.epn_norm_act_bwd_reduce_f32(z, z, groups, 64, c, z, z, z, 1e-5, 0.01, z, z, z, z, sz, z) == EINVAL
        assert lib.epn_norm_act_bwd_apply_f32(z, z, groups, 64, c, z, z, z, z, 1e-5, 0.01, z, z) == EINVAL
        amax = ctypes.c_float(0.0)      # a non-NULL dx_amax (checked first); never written before the refusal
        assert lib.epn_norm_act_bwd_apply_amax_f32(z, z, groups, 64, c, z, z, z, z, 1e-5, 0.01, z, ctypes.byref(amax), z) == EINVAL
        if groups == 1:
            assert lib.epn_norm_act_frozen_fwd_f32(z, 64, c, z, z, z, z, 1e-5, 0.01, z, z) == EINVAL
        sd = _lib.NormPairSide()
        assert lib.epn_norm_act_pair_fwd(z, z, groups, 64, c, ctypes.byref(sd), ctypes.byref(sd), 0.01, z, 0, z) == EINVAL
    assert lib.epn_norm_bwd_finish(z, 1, 0, 64, z, z, z, z, z, sz, z) == EINVAL
    assert lib.epn_norm_bwd_finish(z, 65536, 1, 64, z, z, z, z, z, sz, z) == EINVAL
    assert lib.epn_stats_finish(z, 65536, 1, 64, z, z, sz, z) == EINVAL
    assert lib.epn_stats_finish(z, 1, 1, 0, z, z, sz, z) == EINVAL
    assert lib.epn_bn_running_update_f32(z, 1.0, z, z, z, z, 0.1, 1025, z) == EINVAL
    assert lib.epn_bn_running_update_f32(z, 0.0, z, z, z, z, 0.1, 4, z) == EINVAL
