"""float64 restatement of the block glue (include/epn_so3conv.h "Normalisation + leaky_relu"), independent of the
kernels: plain torch in double, the backward passes through autograd.  Tensors are logical [b, c, p, a].

    batch    : one statistics group, rows = b*p*a        (BatchNorm2d, training arithmetic)
    instance : one group per cloud,  rows = p*a          (InstanceNorm2d(affine=False))
    frozen   : (mean, var) = (running_mean - conv_bias, running_var) as they are (eval-mode BatchNorm2d)
    xhat = (x - mean) / sqrt(var + eps)     var biased
    n    = xhat * gamma + beta              the pre-activation
    y    = leaky(n, slope) * mask / (1 - rate) + residual          the mask comes BEFORE the residual
    sums[g][c] = (sum x, sum x^2) over the group's rows
    dsums[g][c] = gamma * (sum d, sum d * xhat),  d = dy * mask / (1 - rate) * leaky'(n)   (the reduce pass on its own)

Also here: BatchNorm's running update, the fp32 one-pass variance floor, and the two input builders of the GPU tests."""
from collections import namedtuple

import numpy as np
import torch

F64 = torch.float64
NormOut = namedtuple("NormOut", "y xhat n sums mean var")
PairOut = namedtuple("PairOut", "y a b")


def _dims(kind):
    return (2, 3) if kind == "instance" else (0, 2, 3)


def _chan(v):
    return None if v is None else v.to(F64).reshape(1, -1, 1, 1)


def leaky(n, slope):
    return torch.where(n > 0, n, n * slope)


def stats(x, kind, frozen_stats=None, conv_bias=None):
    """(mean, var, sums): broadcastable mean / biased var of the kind, sums f64[groups][c][2] of x as it is stored."""
    x = x.to(F64)
    d = _dims(kind if kind != "frozen" else "batch")
    s1, s2 = x.sum(d, keepdim=True), (x * x).sum(d, keepdim=True)
    sums = torch.stack((s1, s2), -1).reshape(-1, x.shape[1], 2).detach()
    if kind == "frozen":
        rm, rv = frozen_stats
        mean = _chan(rm) - (_chan(conv_bias) if conv_bias is not None else 0.0)
        return mean, _chan(rv), sums
    mean = x.mean(d, keepdim=True)
    var = ((x - mean) ** 2).mean(d, keepdim=True)
    return mean, var, sums


def norm_act_ref(x, kind, gamma=None, beta=None, eps=1e-5, slope=0.01, residual=None, mask=None, rate=0.0, conv_bias=None,
                 frozen_stats=None):
    """-> NormOut(y, xhat, n, sums, mean, var).  conv_bias is the bias of the producing convolution that was NOT added to x:
    the training kinds see x + conv_bias (their mean cancels it), the frozen kind subtracts it from the running mean."""
    x = x.to(F64)
    if kind != "frozen" and conv_bias is not None:
        xe = x + _chan(conv_bias)
        mean, var, _ = stats(xe, kind)
        sums = stats(x, kind)[2]
    else:
        xe = x
        mean, var, sums = stats(x, kind, frozen_stats, conv_bias)
    xhat = (xe - mean) / torch.sqrt(var + eps)
    n = xhat
    if gamma is not None:
        n = n * _chan(gamma)
    if beta is not None:
        n = n + _chan(beta)
    y = leaky(n, slope)
    if mask is not None:
        y = y * mask.to(F64) / (1.0 - rate)
    if residual is not None:
        y = y + residual.to(F64)
    return NormOut(y, xhat, n, sums, mean, var)


def norm_act_pair_ref(xa, xb, kind_a, kind_b, gamma_a=None, beta_a=None, gamma_b=None, beta_b=None, eps_a=1e-5, eps_b=1e-5,
                      slope=0.01, conv_bias_b=None, frozen_stats_b=None):
    """leaky(norm_a(xa)) + leaky(norm_b(xb)) -> PairOut(y, NormOut of side a, NormOut of side b)."""
    a = norm_act_ref(xa, kind_a, gamma_a, beta_a, eps_a, slope)
    b = norm_act_ref(xb, kind_b, gamma_b, beta_b, eps_b, slope, conv_bias=conv_bias_b, frozen_stats=frozen_stats_b)
    return PairOut(a.y + b.y, a, b)


def dsums_ref(out, dy, kind, gamma=None, slope=0.01, mask=None, rate=0.0):
    """f64[groups][c][2] = gamma * (sum d, sum d * xhat) of one norm: what the reduce pass hands to the apply pass."""
    d = dy.to(F64)
    if mask is not None:
        d = d * mask.to(F64) / (1.0 - rate)
    n = out.n.detach()
    d = d * torch.where(n > 0, torch.ones_like(n), torch.full_like(n, slope))
    dm = _dims(kind)
    g = _chan(gamma) if gamma is not None else 1.0
    s = torch.stack(((d.sum(dm, keepdim=True) * g), ((d * out.xhat.detach()).sum(dm, keepdim=True) * g)), -1)
    return s.reshape(-1, dy.shape[1], 2)


def grads(y, inputs, dy):
    """Autograd gradients of the restatement: one tensor per entry of `inputs` (None entries stay None)."""
    live = [t for t in inputs if t is not None]
    g = list(torch.autograd.grad(y, live, dy.to(F64), allow_unused=True))
    return [g.pop(0) if t is not None else None for t in inputs]


def running_update_ref(sums, n, conv_bias, rm, rv, nb, momentum):
    """BatchNorm's training-mode update from sums f64[c][2] of n values per channel -> (running_mean, running_var,
    num_batches_tracked).  Unbiased variance with the max(n - 1, 1) clamp; momentum None: cumulative average, weight
    1 / (nb + 1) (the count after this batch)."""
    sums = torch.as_tensor(sums, dtype=F64)
    mean = sums[:, 0] / n
    var = (sums[:, 1] / n - mean * mean).clamp_min(0.0) * (n / max(n - 1, 1))
    if conv_bias is not None:
        mean = mean + torch.as_tensor(conv_bias, dtype=F64)
    nb = int(nb) + 1
    m = float(momentum) if momentum is not None else 1.0 / nb
    rm, rv = torch.as_tensor(rm, dtype=F64), torch.as_tensor(rv, dtype=F64)
    return rm + m * (mean - rm), rv + m * (var - rv), nb


def one_pass_fp32(x):
    """The floor of every fp32 one-pass variance: x f64[rows, c] -> (mean, var) as float32 arrays with
    var = fl(fl(s2 / n) - fl(m * m)), m = fl(s1 / n), where s1, s2 are the float32 ROUNDINGS OF THE EXACT sums: no summation
    error at all, only the three roundings no kernel of this form avoids."""
    x = np.asarray(x, dtype=np.float64)
    n = np.float32(x.shape[0])
    s1 = x.sum(0).astype(np.float32)
    s2 = (x * x).sum(0).astype(np.float32)
    m = (s1 / n).astype(np.float32)
    var = ((s2 / n).astype(np.float32) - (m * m).astype(np.float32)).astype(np.float32)
    return m, var


def one_pass_floor(x, stat="max"):
    """Relative error of one_pass_fp32's variance against the float64 variance of x f64[rows, c]: the largest over the
    channels (stat="max") or their root mean square (stat="rms")."""
    x = np.asarray(x, dtype=np.float64)
    var = x.var(0)
    e = np.abs(one_pass_fp32(x)[1].astype(np.float64) - var) / var
    return float(e.max() if stat == "max" else np.sqrt((e * e).mean()))


# ---- the launch geometry, restated (csrc/glue.hip make_norm; include/epn_so3conv.h epn_norm_workspace_bytes) -------------
U = 2.0 ** -24          # unit roundoff of fp32


def _cdiv(a, b):
    return -(-a // b)


def geometry(groups, rows, c):
    """(rows_per_block, blocks per group, rstep) of a norm pass: about 1024 blocks in total, at least 64 rows each; a block is
    c/4 channel lanes x rstep = 256 / (c/4) row lanes."""
    rpb = max(64, _cdiv(rows, _cdiv(1024, groups)))
    return rpb, _cdiv(rows, rpb), 256 // (c // 4)


def roundings(groups, rows, c, fold=1):
    """P: an upper bound on the fp32 roundings between an element and a finished sum.  The per-thread chain
    ceil(rows_per_block / rstep), the LDS fold rstep - 1, the finishing kernel over nb = fold * blocks partials (a strided
    chain of at most ceil(nb / 128) + 7 adds, 3 for its register tree, 15 for its LDS fold; nb > 2048 goes through 256-block
    pre-sums first: 16 + 3 + 3 more), and 4 for the product, 1 / rows, the scaling and the subtraction."""
    rpb, blocks, rstep = geometry(groups, rows, c)
    nb = fold * blocks
    pre = 0
    if nb > 2048:
        pre, nb = 22, _cdiv(nb, 256)
    return _cdiv(min(rpb, rows), rstep) + (rstep - 1) + pre + min(nb, _cdiv(nb, 128) + 10) + 15 + 4


# ---- input builders -------------------------------------------------------------------------------------------------
def _round(t, dtype):
    """float64 tensor holding values that `dtype` represents exactly."""
    return t.to(torch.float32).to(dtype).to(F64)


def exact_inputs(shape, seed):
    """(x, dy) float64 [b, c, p, a]: x integers in [-3, 3], dy integers in [-3, 3] times a power of two in [1/4, 4].
    Every partial sum of x, x^2 over fewer than 2^24 / 9 rows is an integer below 2^24: exact in fp32 in any order, and the
    values are exact in bf16."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, shape, generator=g).to(F64)
    dy = torch.randint(-3, 4, shape, generator=g).to(F64) * 2.0 ** torch.randint(-2, 3, shape, generator=g).to(F64)
    return x, dy


def _ulp(v, dtype):
    bits = 7 if dtype == torch.bfloat16 else 23
    return 2.0 ** (torch.floor(torch.log2(v.abs().clamp_min(1e-30))) - bits)


def real_inputs(shape, kappa, seed, tau, kind="batch", gamma=None, beta=None, eps=1e-5, dtype=torch.float32, conv_bias=None,
                frozen_stats=None, max_iter=30, device=None):
    """(x, count): x float64 [b, c, p, a] of values `dtype` represents exactly; channel ch is N(kappa * std_ch, std_ch^2) with
    std_ch spread log-uniformly over [0.3, 3] (kind "frozen": N(mean, var) of the frozen statistics).  Elements whose float64 pre-activation (norm_act_ref with the given kind and
    parameters) satisfies |n| < tau (a number, or a function of the NormOut giving a broadcastable tensor) are moved to |n| = 2 tau on their own side (rounded away from the kink in `dtype`); the
    statistics move with them, so this repeats until none is left.  count = elements with |n| < tau at the end: must be 0.
    A group of one row has xhat = 0 identically and nothing to move: it is not counted, the caller treats it as exact."""
    b, c, p, a = shape
    g = torch.Generator().manual_seed(seed)
    std = 0.3 * 10.0 ** torch.linspace(0.0, 1.0, c, dtype=F64)[torch.randperm(c, generator=g)]
    x = torch.randn(shape, generator=g, dtype=F64) * std.reshape(1, c, 1, 1) + (kappa * std).reshape(1, c, 1, 1)
    if kind == "frozen":        # drawn around the statistics the pass normalises with (kappa is not used)
        fm = _chan(frozen_stats[0]) - (_chan(conv_bias) if conv_bias is not None else 0.0)
        x = fm + _chan(frozen_stats[1]).sqrt() * torch.randn(shape, generator=g, dtype=F64)
    x = _round(x, dtype)
    if device is not None:      # the values are drawn on the host (one generator), the loop below may run anywhere
        x = x.to(device)
        gamma, beta, conv_bias = (t.to(device) if t is not None else None for t in (gamma, beta, conv_bias))
        frozen_stats = tuple(t.to(device) for t in frozen_stats) if frozen_stats is not None else None
    rows = p * a if kind == "instance" else b * p * a
    if (rows == 1 and kind != "frozen") or (not callable(tau) and tau <= 0):
        return x, 0
    gm = _chan(gamma) if gamma is not None else torch.ones(1, c, 1, 1, dtype=F64, device=x.device)
    bt = _chan(beta) if beta is not None else torch.zeros(1, c, 1, 1, dtype=F64, device=x.device)
    shift = _chan(conv_bias) if conv_bias is not None and kind != "frozen" else 0.0
    for _ in range(max_iter):
        o = norm_act_ref(x, kind, gamma, beta, eps, conv_bias=conv_bias, frozen_stats=frozen_stats)
        t = torch.as_tensor(tau(o) if callable(tau) else tau, dtype=F64, device=x.device)
        near = o.n.abs() < t
        count = int(near.sum())
        if count == 0:
            return x, 0
        side = torch.where(o.n >= 0, 1.0, -1.0).to(F64)
        rstd = 1.0 / torch.sqrt(o.var + eps)
        target = o.mean - shift + (side * 2.0 * t - bt) / (gm * rstd)         # x at which n = +-2 tau
        away = side * torch.sign(gm)                                           # direction of x that leaves the kink
        xr = _round(target, dtype)
        xr = torch.where((xr - target) * away < 0, xr + away * _ulp(xr, dtype), xr)
        x = torch.where(near, _round(xr, dtype), x)
    return x, count
