"""-m gpu: the norm glue of csrc/glue.hip (chan_stats, the norm_act / norm_act2 passes in their plain, dropout, frozen and amax
forms, the finishing kernels, bn_running_update) against the float64 restatement tests/norm_ref.py, at the smallest shapes at
which each path of the launch geometry runs.  Nothing is excused: the inputs are built so that no element sits near the
leaky_relu kink (norm_ref.real_inputs; tests/test_norm_spec.py checks that on the CPU), and every element is compared.

Geometry (norm_ref.geometry restates make_norm): a block is c/4 channel lanes x rstep = 256 / (c/4) row lanes and owns
rows_per_block = max(64, ceil(rows / ceil(1024 / groups))) rows.  c = 4: one lane, rstep 256, an LDS fold of 255 terms;
c = 1024: rstep 1, no fold, a per-thread chain of rows_per_block terms.  rows 1, 63: fewer rows than rstep / one short block;
65, 257: a last block of one row; [16, c, 205, 20] instance: rows_per_block 65, 64 blocks per cloud, last block 5 rows.

Tolerances.  u = 2^-24.  P = norm_ref.roundings(...) bounds the fp32 roundings between an element and a finished sum (chain +
fold + finishing kernel + 4; at most 300 for the shapes here: c = 4 has 1 + 255 + 26 + 4).  A sum of P roundings of
non-negative-magnitude terms is off by at most P u sum|t|, so with k2 = mean^2 / (var + eps) of the group and channel (the
reference's own numbers; kappa^2 by construction):
    T = P u (1 + k2)          T(0) = P u for the frozen forms, which subtract no sums
    |d mean| / std <= P u (1 + kappa) <= 1.21 T;   |d var| / var <= P u [(1 + k2) + 2 kappa (1 + kappa)] <= 4 T   (s2 / n - m^2:
    the error of s2, twice mean times the error of the mean);  |d rstd| / rstd <= 2 T;  so |d xhat| <= 2 T (1 + |xhat|) to first
    order.  y = leaky(gamma xhat + beta) has |leaky'| <= 1:  |d y| <= 2 T |gamma| (1 + |xhat|), doubled for the second-order
    terms and the rounding of 1 / rows and rsqrt -> the constant 4; the final operations round relative to |y|: 2^-22 |y|.
    dx = rstd (dn - m1 - xhat m2): rstd is off by 2 T, xhat by 2 T (1 + |xhat|), m1 and m2 by T(0) max|dn| and by the xhat error
    inside m2; with |xhat| up to ~4 these add to at most ~8 T max|dx| -> the constant 8, against the tensor's maximum.  The same
    bound is kept for dgamma, dbeta, dresidual: for the two sums it is TIGHTER than the worst case, which is relative to
    sum|d xhat|, not to the cancelled sum.  The operands of the final subtraction dn - m1 - xhat m2 are each rounded to fp32
    before it, which leaves 4 u rstd max(|dn|, |m1|, |xhat m2|): nothing next to 8 T max|dx| unless dx cancels to zero, as it does
    for a group of one row; the bound carries that term.
    dsums (the reduce pass on its own, norm_ref.dsums_ref) per group and channel: a sum of P roundings of the terms d and d xhat,
    with xhat off by 2 T (1 + |xhat|):  |d dsums| <= |gamma| (P u + 2 T) sum|d| (1 + |xhat|) <= 3 T |gamma| sum|d| (1 + |xhat|),
    held at 4 T for the second-order terms as for y.  This one IS the worst case, relative to sum|d|, so it holds per entry.
    running_mean: the store rounds once (2^-22 |rm|, with margin); the mean is a sum of P roundings, off by at most
    P u mean|x| <= P u (|mean| + std), weighted by the momentum m.  (An expression proportional to |mean| alone, such as
    T |mean|, cannot bound it: it vanishes with the mean, the rounding error of a sum of values of size std does not.
    P u (|mean| + std) is below T |mean| = P u (1 + kappa^2) |mean| from kappa = 1 upwards.)
    running_var: 2^-22 |rv| + m n / (n - 1) 2 T (var + mean^2)   (|d var| <= 4 T var is 2 T (var + mean^2) at kappa = 1 and
    below it elsewhere up to the factor 2 the constant carries).
bf16 tensors: the reference is fed the bf16-rounded inputs; a stored bf16 y / dx is compared with the unrounded float64 value
with 2^-8 |ref| on top (one rounding to 8 significant bits).
The bracket against one_pass_fp32 (test_norm_spec.test_one_pass_floor prints it): the floor has 3 roundings and exact sums, the
bound P + 3 in the worst case, so the y bound is 8 P / 3 ~ 50 ... 800 times the floor's effect -- ABOVE the 32 x of a
measurement-like bound by design: P is a worst case over every accumulation order a kernel may use, and is what lets the bound
stand under a change of that order.  The lower side (bound >= 2 x floor) holds and is asserted there.  The documented cost
itself is held to the floor, not to P: at kappa = 300 the kernel's implied variance must be within 4 x the floor (below).
kappa = 300: T(300) = P u 90 001 is 0.2 .. 0.3 at c = 64, so 4 T (1 + |xhat|) exceeds |y| itself: the T(300) bounds on y and the
gradients are asserted but carry NO information there, and tau = 4 x tolerance exceeds the range of n, so no input can keep
clear of the kink; that case runs with slope = 1, where the kink vanishes.  The binding check at kappa = 300 is the variance
ratio against the floor."""
import ctypes

import pytest
import torch

import norm_ref as R
from norm_cases import (DTYPES, EPS, F64, FORMS, K300, KAPPAS, PAIR, PAIR_SIDES, SINGLE, U, _id, affine_params, finish_cases,
                        frozen_inputs, fwd_tol, groups_rows, pair_frozen_inputs, pair_inputs, single_inputs, single_seed, t_of)

pytestmark = pytest.mark.gpu

pytestmark = pytest.mark.gpu
def to_dev(t64, dtype, dev):
    return t64.to(torch.float32).to(dtype).to(dev).contiguous(memory_format=torch.channels_last)


def close(name, got, ref, tol):
    err = (got.detach().to(F64) - ref.detach()).abs()
    tol = torch.as_tensor(tol, dtype=F64, device=err.device).expand_as(err)
    bad = ~(err <= tol)
    assert not bool(bad.any()), (f"{name}: {int(bad.sum())} of {bad.numel()} elements beyond the bound, worst error / bound "
                                 f"{float((err / tol.clamp_min(1e-300)).max()):.3g}, worst error {float(err.max()):.3g}")


def close_max(name, got, ref, T, bf16=False, operands=0.0):
    """max error <= 8 T max|ref| + 4 u `operands` (+ 2^-8 |ref| per element of a tensor stored in bf16).  operands: the largest
    magnitude that enters the final subtraction dn - m1 - xhat m2, times rstd (module docstring)."""
    ref = ref.detach()
    tol = 8.0 * float(T) * float(ref.abs().max()) + 4.0 * U * float(operands) + (2.0 ** -8 * ref.abs() if bf16 else 0.0)
    close(name, got, ref, tol)


def _grads(y, inputs, dy):
    live = [t for t in inputs if t is not None]
    g = list(torch.autograd.grad(y, live, dy, allow_unused=True))
    return [g.pop(0) if t is not None else None for t in inputs]


def make_norm(kind, c, gamma, beta, dev, momentum=0.1, affine=None):
    if kind == "instance":
        return torch.nn.InstanceNorm2d(c, affine=False).to(dev).train()
    m = torch.nn.BatchNorm2d(c, affine=gamma is not None, momentum=momentum).to(dev).train()
    if gamma is not None:
        with torch.no_grad():
            m.weight.copy_(gamma.float()); m.bias.copy_(beta.float())
    return m


def run_single(dev, kind, shape, dtype, kappa, seed, *, affine=None, slope=0.01, residual=False, conv_bias=False, dropout=0.0,
               momentum=0.1, nudge=True):
    """One norm_act forward + backward on real inputs against float64: y, dx, dresidual, dgamma, dbeta, dconv_bias, the running
    statistics.  Returns what the callers look at further."""
    from epn_pointcloud_amd import ops
    b, c, p, a = shape
    groups, rows = groups_rows(kind, shape)
    bf = dtype == torch.bfloat16
    affine = (kind == "batch") if affine is None else affine
    x64, left, gamma, beta, bias, P, g = single_inputs(kind, shape, dtype, kappa, seed, affine, conv_bias, nudge, dev)
    assert left == 0
    x64 = x64.cpu()
    dy64 = R._round(torch.randn(shape, generator=g, dtype=F64), dtype)
    r64 = R._round(torch.randn(shape, generator=g, dtype=F64), dtype) if residual else None
    # kernels
    norm = make_norm(kind, c, gamma, beta, dev, momentum)
    x = to_dev(x64, dtype, dev).requires_grad_(True)
    r = to_dev(r64, dtype, dev).requires_grad_(True) if residual else None
    cb = bias.float().to(dev).requires_grad_(True) if conv_bias else None
    mask, rate = None, 0.0
    if dropout:
        state = ops.dropout_state(dev).clone()
        rate = dropout
    y = ops.norm_act(x, norm, residual=r, slope=slope, conv_bias=cb, dropout=dropout)
    if dropout:
        mask = ops.dropout_mask(b, c, p, a, dropout, state)
        assert int(ops.dropout_state(dev)[1]) == int(state[1]) + 1
    ins = [x, r, norm.weight if affine else None, norm.bias if affine else None, cb]
    got = _grads(y, ins, to_dev(dy64, dtype, dev))
    if rows == 1 and not residual and not dropout:
        # one row per group: mean = x and xhat = 0 on both sides without a rounding, n = beta exactly
        nb = (beta.float() if affine else torch.zeros(c)).to(dev)
        want = torch.where(nb > 0, nb, nb * slope).to(dtype).reshape(1, c, 1, 1).expand(b, c, p, a)
        assert torch.equal(y.detach(), want)
    # float64
    xr = x64.to(dev).requires_grad_(True)
    rr = r64.to(dev).requires_grad_(True) if residual else None
    gr = gamma.to(dev).requires_grad_(True) if affine else None
    br = beta.to(dev).requires_grad_(True) if affine else None
    cr = bias.to(dev).requires_grad_(True) if conv_bias else None
    out = R.norm_act_ref(xr, kind, gr, br, EPS, slope, rr, mask, rate, cr)
    ref = R.grads(out.y, [xr, rr, gr, br, None], dy64.to(dev))
    out = R.NormOut(*(t.detach() for t in out))
    T = t_of(out, P, rows)
    Tm = float(T.max())
    scale = 1.0 / (1.0 - rate)
    close("y", y, out.y, fwd_tol(out, T, gamma.to(dev) if affine else None, bf, scale))
    gmax = float(gamma.abs().max()) if affine else 1.0
    ops_dx = float(dy64.abs().max()) * gmax * scale * float((out.var + EPS).rsqrt().max()) * (1.0 + float(out.xhat.abs().max()))
    close_max("dx", got[0], ref[0], Tm * scale, bf, ops_dx)
    if residual:
        close_max("dresidual", got[1], ref[1], Tm, bf)
    if affine:
        close_max("dgamma", got[2], ref[2], Tm * scale)
        close_max("dbeta", got[3], ref[3], Tm * scale)
    if conv_bias:
        assert got[4] is not None and bool((got[4] == 0).all()), "dconv_bias is exactly 0"
    # the reduce pass on its own (with the mask of the forward's (seed, call) when there is one)
    xc, dyc = x.detach(), to_dev(dy64, dtype, dev)
    g32, b32 = (gamma.float().to(dev), beta.float().to(dev)) if affine else (None, None)
    dsums, _, _ = ops._norm_bwd_reduce(xc, dyc, ops._chan_stats(xc, groups, rows, c), g32, b32, groups, rows, c, EPS, slope,
                                       drop=(rate, state) if dropout else None)
    dref = R.dsums_ref(out, dy64.to(dev), kind, gamma.to(dev) if affine else None, slope, mask, rate)
    d = dy64.to(dev).abs() * (mask.to(F64) * scale if dropout else 1.0)
    dims = (2, 3) if kind == "instance" else (0, 2, 3)
    budget = (d * (1.0 + out.xhat.abs())).sum(dims).reshape(groups, c, 1) * (gamma.abs().to(dev).reshape(1, c, 1) if affine else 1.0)
    close("dsums", dsums, dref, 4.0 * T.reshape(groups, c, 1) * budget)
    if kind == "batch":
        rm, rv, nb = R.running_update_ref(out.sums[0].cpu(), rows, bias, torch.zeros(c), torch.ones(c), 0, momentum)
        m = momentum if momentum is not None else 1.0
        mean, var = out.sums[0, :, 0].cpu() / rows, out.var.reshape(-1).cpu()
        Tc = T.reshape(-1).cpu()
        Pu = P * U
        close("running_mean", norm.running_mean.cpu(), rm, 2.0 ** -22 * rm.abs() + m * Pu * (mean.abs() + var.sqrt()))
        close("running_var", norm.running_var.cpu(), rv,
              2.0 ** -22 * rv.abs() + m * 2.0 * Tc * (var + mean * mean) * rows / max(rows - 1, 1))
        assert int(norm.num_batches_tracked) == nb == 1
    return dict(x64=x64, y=y, out=out, norm=norm, bias=bias, gamma=gamma, beta=beta, P=P)


# ---- a. exact structure ---------------------------------------------------------------------------------------------
GUARD = 64
SENT = 12345.0


class Guarded:
    """A device buffer of n elements poisoned with NaN, followed by GUARD cells holding a sentinel."""

    def __init__(self, n, dev, dtype=torch.float32):
        self.n = n
        self.buf = torch.full((n + GUARD,), float("nan"), dtype=dtype, device=dev)
        self.buf[n:] = SENT if dtype != torch.bfloat16 else 2.0
        self.sent = self.buf[n:].clone()

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr())

    def data(self):
        return self.buf[:self.n]

    def check(self, name):
        assert torch.equal(self.buf[self.n:], self.sent), f"{name}: cells after the end of the buffer were written"
        assert not bool(torch.isnan(self.data()).any()), f"{name}: {int(torch.isnan(self.data()).sum())} cells never written"
        return self.data()


def _workspace(nbytes, dev):
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    return ws, ctypes.c_void_p(ws.data_ptr() if nbytes else 0), ctypes.c_size_t(nbytes)


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
@pytest.mark.parametrize("case", SINGLE, ids=_id)
def test_exact_sums_and_written_ranges(gpu, case, dtype):
    """Integer inputs: every partial sum is exact in fp32 in any order, so (sum x, sum x^2) from chan_stats + stats_finish EQUAL
    the float64 sums -- through NormActFn and through the C ABI.  The four passes write every cell of sums, y, dsums, dgamma,
    dbeta, dx (poisoned with NaN before the call) and nothing after their ends.  The VALUES of y, dsums and the gradients are
    compared on inputs built clear of the kink (run_single), not here."""
    from epn_pointcloud_amd import _lib, ops
    kind, shape = case
    b, c, p, a = shape
    groups, rows = groups_rows(kind, shape)
    lib, sfx = _lib.get_lib(), "bf16" if dtype == torch.bfloat16 else "f32"
    x64, dy64 = R.exact_inputs(shape, seed=c + rows)
    want = R.stats(x64, kind)[2]
    x, dy = to_dev(x64, dtype, gpu), to_dev(dy64, dtype, gpu)
    with torch.no_grad():
        y0, sums0 = ops.NormActFn.apply(x, None, None, None, None, kind == "instance", EPS, 0.01)
    assert torch.equal(sums0.cpu().to(F64), want)
    gamma, beta = (t.float().to(gpu) for t in affine_params(c, 3))
    n = x.numel()
    sums, dsums = Guarded(groups * c * 2, gpu), Guarded(groups * c * 2, gpu)
    dg, db = Guarded(c, gpu), Guarded(c, gpu)
    y, dx = Guarded(n, gpu, dtype), Guarded(n, gpu, dtype)
    ws, wsp, wsn = _workspace(lib.epn_norm_workspace_bytes(groups, rows, c), gpu)
    st = _lib.stream_of(x)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(getattr(lib, "epn_chan_stats_" + sfx)(vp(x), groups, rows, c, sums.ptr, wsp, wsn, st), "chan_stats")
    _lib.check(getattr(lib, "epn_norm_act_fwd_" + sfx)(vp(x), groups, rows, c, sums.ptr, vp(gamma), vp(beta), None, EPS, 0.01, y.ptr,
                                                       st), "fwd")
    _lib.check(getattr(lib, "epn_norm_act_bwd_reduce_" + sfx)(vp(x), vp(dy), groups, rows, c, sums.ptr, vp(gamma), vp(beta), EPS, 0.01,
                                                              dsums.ptr, dg.ptr, db.ptr, wsp, wsn, st), "bwd_reduce")
    _lib.check(getattr(lib, "epn_norm_act_bwd_apply_" + sfx)(vp(x), vp(dy), groups, rows, c, sums.ptr, dsums.ptr, vp(gamma), vp(beta),
                                                             EPS, 0.01, dx.ptr, st), "bwd_apply")
    torch.cuda.synchronize()
    assert torch.equal(sums.check("sums").cpu().to(F64).reshape(groups, c, 2), want)
    for name, gb in (("y", y), ("dsums", dsums), ("dgamma", dg), ("dbeta", db), ("dx", dx)):
        gb.check(name)


def _partials(g, nb, c, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, (g, nb, c, 2), generator=gen).float()


@pytest.mark.parametrize("case", finish_cases((1, 7, 20, 1024)), ids=_id)
def test_stats_finish_exact(gpu, case):
    """epn_stats_finish on integer partials: sums[g][e] = sum_b part[g][b][e] exactly, across the 16 / 128-block strides of the
    one-level kernel, the 2048-block switch to two levels and the 256-block boundaries behind it; any c >= 1 (the e < c2
    guards)."""
    from epn_pointcloud_amd import _lib
    g, nb, c = case
    lib = _lib.get_lib()
    part = _partials(g, nb, c, 11 * nb + c)
    want = part.to(F64).sum(1)
    nbytes = lib.epn_stats_finish_workspace_bytes(g, nb, c)
    assert nbytes == (g * -(-nb // 256) * c * 8 if nb > 2048 else 0)
    ws = Guarded(nbytes // 4, gpu)
    sums = Guarded(g * c * 2, gpu)
    pd = part.to(gpu)
    _lib.check(lib.epn_stats_finish(pd.data_ptr(), g, nb, c, sums.ptr, ws.ptr if nbytes else None, nbytes, _lib.stream_of(pd)),
               "stats_finish")
    torch.cuda.synchronize()
    assert torch.equal(sums.check("sums").cpu().to(F64).reshape(g, c, 2), want)
    ws.check("workspace")


@pytest.mark.parametrize("with_gamma", (True, False), ids=("gamma", "nogamma"))
@pytest.mark.parametrize("case", finish_cases((4, 20, 1024)), ids=_id)
def test_bwd_finish_exact(gpu, case, with_gamma):
    """epn_norm_bwd_finish on integer partials, gamma in {+-1/2, +-1, +-2, 3} (exact products): dsums = gamma (sa, sb) per group,
    dgamma = sum_g sb, dbeta = sum_g sa exactly; one group stores, three groups add atomically onto the memset."""
    from epn_pointcloud_amd import _lib
    g, nb, c = case
    lib = _lib.get_lib()
    part = _partials(g, nb, c, 13 * nb + c)
    tot = part.to(F64).sum(1)
    gen = torch.Generator().manual_seed(c)
    gamma = torch.tensor([0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 3.0])[torch.randint(0, 7, (c,), generator=gen)] if with_gamma else None
    want = tot * (gamma.to(F64).reshape(1, c, 1) if with_gamma else 1.0)
    nbytes = lib.epn_stats_finish_workspace_bytes(g, nb, c)
    ws = Guarded(nbytes // 4, gpu)
    dsums, dg, db = Guarded(g * c * 2, gpu), Guarded(c, gpu), Guarded(c, gpu)
    pd, gd = part.to(gpu), gamma.to(gpu) if with_gamma else None
    _lib.check(lib.epn_norm_bwd_finish(pd.data_ptr(), g, nb, c, gd.data_ptr() if with_gamma else None, dsums.ptr, dg.ptr, db.ptr,
                                       ws.ptr if nbytes else None, nbytes, _lib.stream_of(pd)), "norm_bwd_finish")
    torch.cuda.synchronize()
    assert torch.equal(dsums.check("dsums").cpu().to(F64).reshape(g, c, 2), want)
    assert torch.equal(dg.check("dgamma").cpu().to(F64), tot[:, :, 1].sum(0))
    assert torch.equal(db.check("dbeta").cpu().to(F64), tot[:, :, 0].sum(0))
    ws.check("workspace")


# ---- b. real-valued accuracy ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
@pytest.mark.parametrize("case", SINGLE, ids=_id)
def test_norm_act_vs_fp64(gpu, case, dtype):
    """ops.norm_act, forward and backward, at kappa = 0, 1, 10: every element of y within 4 T |gamma| (1 + |xhat|) + 2^-22 |y|,
    gradients within 8 T of their maximum, running statistics within their bound (module docstring)."""
    kind, shape = case
    for kappa in KAPPAS:
        run_single(gpu, kind, shape, dtype, kappa, single_seed(shape, kappa))


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
@pytest.mark.parametrize("case", [s for s in SINGLE if s[0] == "batch"], ids=_id)
def test_frozen_forward_vs_fp64(gpu, case, dtype):
    """ops.norm_act_eval on running statistics of mean 30, var 0.01 (k2 = 90 000): the bound is T(0), with no kappa^2 term -- what
    the FROZEN flag exists for.  With and without a conv_bias (it moves the mean the pass subtracts: the reference is fed the
    float32 difference the pass reads)."""
    from epn_pointcloud_amd import ops
    _, shape = case
    b, c, p, a = shape
    rows, bf = b * p * a, dtype == torch.bfloat16
    for use_bias in (False, True):
        x64, left, gamma, beta, rm, rv, bias, fs, P = frozen_inputs(shape, dtype, use_bias, gpu)
        assert left == 0
        x64 = x64.cpu()
        norm = make_norm("batch", c, gamma, beta, gpu).eval()
        with torch.no_grad():
            norm.running_mean.copy_(rm); norm.running_var.copy_(rv)
            y = ops.norm_act_eval(to_dev(x64, dtype, gpu), norm, conv_bias=bias.to(gpu) if use_bias else None)
        out = R.norm_act_ref(x64, "frozen", gamma, beta, EPS, frozen_stats=fs)
        close("y", y.cpu(), out.y, fwd_tol(out, t_of(out, P, rows, frozen=True), gamma, bf))
        assert torch.equal(norm.running_mean.cpu(), rm) and int(norm.num_batches_tracked) == 0


@pytest.mark.parametrize("case", K300, ids=_id)
def test_training_form_at_kappa_300(gpu, case):
    """mean = 300 std: the documented cost of var = s2 / rows - mean^2 in fp32.  THE test here is the variance the
    kernel implies -- rstd recovered from y = (x - mean) rstd by least squares in float64 -- within 4 x the one_pass_fp32 floor
    of the same inputs.  The T(300) bounds that run_single asserts on the way exceed |y| and carry no information (module
    docstring); slope 1, no affine pair, nothing to nudge."""
    kind, shape = case
    res = run_single(gpu, kind, shape, torch.float32, 300, seed=300, affine=False, slope=1.0, nudge=False)
    out, y = res["out"], res["y"].detach().cpu().to(F64)
    d = (2, 3) if kind == "instance" else (0, 2, 3)
    xc = res["x64"] - out.mean.cpu()
    rstd = (y * xc).sum(d) / (xc * xc).sum(d)
    var_k = 1.0 / (rstd * rstd) - EPS
    var = out.var.cpu().reshape(var_k.shape)
    err = float(((var_k - var).abs() / var).max())
    b, c, p, a = shape
    xs = res["x64"].permute(0, 2, 3, 1).reshape((b, p * a, c) if kind == "instance" else (1, b * p * a, c))
    floor = max(R.one_pass_floor(xg.numpy()) for xg in xs)
    print(f"kappa 300 {kind} {shape}: implied variance off by {err:.3e}, one-pass floor {floor:.3e}, ratio {err / floor:.2f}")
    assert err <= 4.0 * floor, (err, floor)


# ---- c. forms that share the bodies -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
@pytest.mark.parametrize("case", FORMS, ids=_id)
def test_forms_vs_fp64(gpu, case, dtype):
    """The options of the single-tensor passes: residual, slope 0.2 and 1, conv_bias (gradient exactly 0, the running mean moves
    by it), BatchNorm without affine parameters, dropout 0.25 (mask from epn_dropout_mask_u8 for the saved (seed, call), applied
    before the residual), momentum None."""
    kind, shape = case
    seed = shape[1] + shape[2]
    run_single(gpu, kind, shape, dtype, 1, seed, residual=True)
    run_single(gpu, kind, shape, dtype, 1, seed + 1, slope=0.2)
    run_single(gpu, kind, shape, dtype, 10, seed + 2, slope=1.0, nudge=False)
    run_single(gpu, kind, shape, dtype, 1, seed + 3, conv_bias=True)
    run_single(gpu, kind, shape, dtype, 1, seed + 4, dropout=0.25, residual=True)
    if kind == "batch":
        run_single(gpu, kind, shape, dtype, 1, seed + 5, affine=False)
        run_single(gpu, kind, shape, dtype, 0, seed + 6, momentum=None)


def _side(sums, gamma, beta, instance):
    from epn_pointcloud_amd import _lib
    sd = _lib.NormPairSide()
    sd.sums, sd.gamma, sd.beta = _lib.dev_ptr(sums, "sums"), _lib.dev_ptr(gamma, "gamma"), _lib.dev_ptr(beta, "beta")
    sd.eps, sd.instance = EPS, int(instance)
    return sd


@pytest.mark.parametrize("case", FORMS, ids=_id)
def test_amax_forms(gpu, case):
    """The _amax entry points: the tensor is the one the plain entry writes, bit for bit, and amax = max|stored tensor|; the
    maximum is a by-product of the fp32 kernels only, so bf16 = 1 is refused."""
    from epn_pointcloud_amd import _lib, ops
    kind, shape = case
    b, c, p, a = shape
    groups, rows = groups_rows(kind, shape)
    lib = _lib.get_lib()
    g = torch.Generator().manual_seed(c + rows)
    x = to_dev(torch.randn(shape, generator=g, dtype=F64) * 2 + 0.5, torch.float32, gpu)
    xb = to_dev(torch.randn(shape, generator=g, dtype=F64) - 0.2, torch.float32, gpu)
    dy = to_dev(torch.randn(shape, generator=g, dtype=F64), torch.float32, gpu)
    gamma, beta = (t.float().to(gpu) for t in affine_params(c, 9))
    sums, sums_b = ops._chan_stats(x, groups, rows, c), ops._chan_stats(xb, b, p * a, c)
    dsums, _, _ = ops._norm_bwd_reduce(x, dy, sums, gamma, beta, groups, rows, c, EPS, 0.01)
    st = _lib.stream_of(x)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    amax = torch.full((1,), float("nan"), device=gpu)
    dx0, dx1 = torch.empty_like(x), torch.empty_like(x)
    common = (vp(x), vp(dy), groups, rows, c, vp(sums), vp(dsums), vp(gamma), vp(beta), EPS, 0.01)
    _lib.check(lib.epn_norm_act_bwd_apply_f32(*common, vp(dx0), st), "bwd_apply")
    _lib.check(lib.epn_norm_act_bwd_apply_amax_f32(*common, vp(dx1), vp(amax), st), "bwd_apply_amax")
    assert torch.equal(dx0, dx1) and float(amax) == float(dx0.abs().max())
    # pair form: side a = x with the single form's kind and affine pair, side b = xb instance
    sa, sb = _side(sums, gamma, beta, kind == "instance"), _side(sums_b, None, None, True)
    rows_c = p * a
    y0, y1 = torch.empty_like(x), torch.empty_like(x)
    head = (vp(x), vp(xb), b, rows_c, c, ctypes.byref(sa), ctypes.byref(sb), 0.01)
    _lib.check(lib.epn_norm_act_pair_fwd(*head, vp(y0), 0, st), "pair_fwd")
    amax.fill_(float("nan"))
    _lib.check(lib.epn_norm_act_pair_fwd_amax(*head, vp(y1), 0, vp(amax), st), "pair_fwd_amax")
    assert torch.equal(y0, y1) and float(amax) == float(y0.abs().max())
    assert lib.epn_norm_act_pair_fwd_amax(*head, vp(y1), 1, vp(amax), st) == -1, "bf16 = 1: EPN_EINVAL"
    dsa, dsb = torch.empty_like(sums), torch.empty_like(sums_b)
    dga, dba = torch.empty(c, device=gpu), torch.empty(c, device=gpu)
    ws, wsp, wsn = _workspace(lib.epn_norm_pair_workspace_bytes(b, rows_c, c), gpu)
    bh = (vp(x), vp(xb), vp(dy), b, rows_c, c, ctypes.byref(sa), ctypes.byref(sb), 0.01)
    _lib.check(lib.epn_norm_act_pair_bwd_reduce(*bh, vp(dsa), vp(dga), vp(dba), vp(dsb), None, None, wsp, wsn, 0, st), "pair_bwd_reduce")
    da0, db0, da1, db1 = (torch.empty_like(x) for _ in range(4))
    _lib.check(lib.epn_norm_act_pair_bwd_apply(*bh, vp(dsa), vp(dsb), vp(da0), vp(db0), 0, st), "pair_bwd_apply")
    amax.fill_(float("nan"))
    _lib.check(lib.epn_norm_act_pair_bwd_apply_amax(*bh, vp(dsa), vp(dsb), vp(da1), vp(db1), 0, vp(amax), st), "pair_bwd_apply_amax")
    assert torch.equal(da0, da1) and torch.equal(db0, db1) and float(amax) == float(db0.abs().max())
    assert lib.epn_norm_act_pair_bwd_apply_amax(*bh, vp(dsa), vp(dsb), vp(da1), vp(db1), 1, vp(amax), st) == -1, "bf16 = 1: EPN_EINVAL"


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16"))
@pytest.mark.parametrize("side_b", PAIR_SIDES, ids=lambda s: f"{s[0]}-{'affine' if s[1] else 'plain'}")
@pytest.mark.parametrize("shape", PAIR, ids=_id)
def test_pair_vs_fp64(gpu, shape, side_b, dtype):
    """ops.norm_act_pair on 16 clouds: side a InstanceNorm, side b instance or batch (a batch side folds 16 x blocks partials),
    with or without affine parameters (an affine instance side accumulates dgamma / dbeta over the clouds atomically).  y within
    the sum of the two sides' bounds, both input gradients and side b's parameter gradients within 8 T of their maximum, side
    b's running statistics; then the frozen side b of norm_act_pair_eval within T(0) on statistics of mean 30, var 0.01."""
    from epn_pointcloud_amd import ops
    kind_b, affine_b = side_b
    b, c, p, a = shape
    rows = p * a
    bf = dtype == torch.bfloat16
    ga, rb = groups_rows("instance", shape), groups_rows(kind_b, shape)
    Pa = R.roundings(*ga, c)
    Pb = R.roundings(*rb, c, fold=1) if kind_b == "instance" else R.roundings(b, rows, c, fold=b)
    gamma, beta = affine_params(c, 21) if affine_b else (None, None)
    xa64, la, xb64, lb = pair_inputs(shape, side_b, dtype, gpu)
    assert la == 0 and lb == 0
    xa64, xb64 = xa64.cpu(), xb64.cpu()
    g = torch.Generator().manual_seed(5)
    dy64 = R._round(torch.randn(shape, generator=g, dtype=F64), dtype)
    na = torch.nn.InstanceNorm2d(c, affine=False).to(gpu).train()
    if kind_b == "batch":
        nb = make_norm("batch", c, gamma, beta, gpu)
    else:
        nb = torch.nn.InstanceNorm2d(c, affine=affine_b).to(gpu).train()
        if affine_b:
            with torch.no_grad():
                nb.weight.copy_(gamma.float()); nb.bias.copy_(beta.float())
    xa, xb = to_dev(xa64, dtype, gpu).requires_grad_(True), to_dev(xb64, dtype, gpu).requires_grad_(True)
    y = ops.norm_act_pair(xa, na, xb, nb)
    got = _grads(y, [xa, xb, nb.weight if affine_b else None, nb.bias if affine_b else None], to_dev(dy64, dtype, gpu))
    ra, rbx = xa64.to(gpu).requires_grad_(True), xb64.to(gpu).requires_grad_(True)
    gr = gamma.to(gpu).requires_grad_(True) if affine_b else None
    br = beta.to(gpu).requires_grad_(True) if affine_b else None
    o = R.norm_act_pair_ref(ra, rbx, "instance", kind_b, None, None, gr, br, EPS, EPS, 0.01)
    ref = R.grads(o.y, [ra, rbx, gr, br], dy64.to(gpu))
    oa, ob = (R.NormOut(*(t.detach() for t in s)) for s in (o.a, o.b))
    Ta, Tb = t_of(oa, Pa, rows), t_of(ob, Pb, rb[1])
    tol = fwd_tol(oa, Ta, None, False, y=o.y.detach() * 0) + fwd_tol(ob, Tb, gamma.to(gpu) if affine_b else None, bf, y=o.y.detach())
    close("y", y, o.y, tol)
    dmax = float(dy64.abs().max())
    opa = dmax * float((oa.var + EPS).rsqrt().max()) * (1.0 + float(oa.xhat.abs().max()))
    opb = dmax * (float(gamma.abs().max()) if affine_b else 1.0) * float((ob.var + EPS).rsqrt().max()) * (1.0 + float(ob.xhat.abs().max()))
    close_max("dxa", got[0], ref[0], float(Ta.max()), bf, opa)
    close_max("dxb", got[1], ref[1], float(Tb.max()), bf, opb)
    if affine_b:
        close_max("dgamma_b", got[2], ref[2], float(Tb.max()))
        close_max("dbeta_b", got[3], ref[3], float(Tb.max()))
    if kind_b == "batch":
        n = b * rows
        rm, rv, _ = R.running_update_ref(ob.sums[0].cpu(), n, None, torch.zeros(c), torch.ones(c), 0, 0.1)
        mean, var, Tc = ob.sums[0, :, 0].cpu() / n, ob.var.reshape(-1).cpu(), Tb.reshape(-1).cpu()
        close("running_mean", nb.running_mean.cpu(), rm, 2.0 ** -22 * rm.abs() + 0.1 * Pb * U * (mean.abs() + var.sqrt()))
        close("running_var", nb.running_var.cpu(), rv, 2.0 ** -22 * rv.abs() + 0.1 * 2.0 * Tc * (var + mean * mean) * n / (n - 1))
        # eval mode: side b frozen on statistics of mean 30, var 0.01; x_b drawn around them, clear of side b's kink
        xf64, lf, gm, _, rm32, rv32, fs, Pf = pair_frozen_inputs(shape, affine_b, dtype, gpu)
        assert lf == 0
        xf64 = xf64.cpu()
        of = R.norm_act_ref(xf64, "frozen", gm, beta, EPS, frozen_stats=fs)
        nb.eval()
        with torch.no_grad():
            nb.running_mean.copy_(rm32); nb.running_var.copy_(rv32)
            ye = ops.norm_act_pair_eval(xa.detach(), na.eval(), to_dev(xf64, dtype, gpu), nb)
        want = oa.y.cpu() + of.y
        tole = fwd_tol(oa, Ta, None, False, y=want.to(gpu) * 0).cpu() + fwd_tol(of, t_of(of, Pf, n, frozen=True), gm, bf, y=want)
        close("y eval", ye.cpu(), want, tole)


# ---- d. epn_bn_running_update_f32 directly ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 2, 6660))
@pytest.mark.parametrize("with_bias", (False, True), ids=("nobias", "bias"))
@pytest.mark.parametrize("momentum", (0.1, None), ids=("m0.1", "mNone"))
@pytest.mark.parametrize("c", (1, 3, 1024))
def test_bn_running_update_vs_ref(gpu, c, momentum, with_bias, n):
    """Two consecutive updates against running_update_ref: unbiased variance with the max(n - 1, 1) clamp, the conv_bias added to
    the mean, num_batches_tracked + 1 per call, the cumulative average weighted by the NEW count.  The kernel divides, squares,
    subtracts and rescales in fp32: T = 4 u (1 + mean^2 / var) in the bounds of the module docstring."""
    from epn_pointcloud_amd import _lib
    lib = _lib.get_lib()
    g = torch.Generator().manual_seed(c + n)
    rm, rv, nb = torch.randn(c, generator=g).float(), (0.5 + torch.rand(c, generator=g)).float(), 5
    rm_d, rv_d, nb_d = Guarded(c, gpu), Guarded(c, gpu), torch.tensor([nb], dtype=torch.int64, device=gpu)
    rm_d.data().copy_(rm); rv_d.data().copy_(rv)
    bias = torch.randn(c, generator=g).float() if with_bias else None
    bias_d = bias.to(gpu) if with_bias else None
    rm_r, rv_r = rm.to(F64), rv.to(F64)
    acc_m = acc_v = 0.0          # the first call's error stays in the buffers, weighted by 1 - m
    for call in range(2):
        mean = 2.0 * torch.randn(c, generator=g, dtype=F64)
        var = 0.1 + 1.9 * torch.rand(c, generator=g, dtype=F64) if n > 1 else torch.zeros(c, dtype=F64)
        sums = torch.stack((n * mean, n * (var + mean * mean)), 1).float()
        sd = sums.to(gpu)
        _lib.check(lib.epn_bn_running_update_f32(sd.data_ptr(), float(n), bias_d.data_ptr() if with_bias else None, rm_d.ptr, rv_d.ptr,
                                                 nb_d.data_ptr(), momentum if momentum is not None else -1.0, c, _lib.stream_of(sd)),
                   "bn_running_update")
        rm_r, rv_r, nb = R.running_update_ref(sums.to(F64), n, bias.to(F64) if with_bias else None, rm_r, rv_r, nb, momentum)
        assert int(nb_d) == nb == 6 + call
        m = momentum if momentum is not None else 1.0 / nb
        s64 = sums.to(F64)
        mu, ex2 = s64[:, 0] / n, s64[:, 1] / n
        T = 4.0 * U
        tol_m = 2.0 ** -22 * rm_r.abs() + m * T * (mu.abs() + (bias.to(F64).abs() if with_bias else 0.0))
        tol_v = 2.0 ** -22 * rv_r.abs() + m * 2.0 * T * ex2 * n / max(n - 1, 1)
        acc_m, acc_v = tol_m + (1.0 - m) * acc_m, tol_v + (1.0 - m) * acc_v
        close("running_mean", rm_d.check("running_mean").cpu(), rm_r, acc_m)
        close("running_var", rv_d.check("running_var").cpu(), rv_r, acc_v)
