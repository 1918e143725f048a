"""Case tables, input builders and the tolerance model shared by tests/test_gpu_norm_fp64.py (which runs them on the device) and
tests/test_norm_spec.py (which checks on the CPU that the builders leave no element near the leaky_relu kink).  Nothing here
needs a device or the library.  The derivation of the bounds is in the docstring of tests/test_gpu_norm_fp64.py."""
import torch

import norm_ref as R

F64 = torch.float64
U = R.U
EPS = 1e-5
WIDTHS = (4, 16, 64, 1024)
ROWS = (1, 63, 64, 65, 255, 256, 257)
DTYPES = (torch.float32, torch.bfloat16)
KAPPAS = (0, 1, 10)


def single_cases(widths=WIDTHS, rows=ROWS, extra=True):
    """(kind, [b, c, p, a]): instance with 2 clouds and batch with 1 at every rows-per-group, batch over 3 clouds, and the
    16-cloud instance case (4100 rows per cloud up to c = 64, 257 at c = 1024: tensors stay under 20 MB)."""
    out = []
    for c in widths:
        for r in rows:
            out += [("instance", (2, c, r, 1)), ("batch", (1, c, r, 1))]
        if extra:
            out += [("batch", (3, c, 21, 1)), ("batch", (3, c, 17, 5)), ("batch", (3, c, 19, 5))]
            out.append(("instance", (16, c, 205, 20) if c <= 64 else (16, c, 257, 1)))
    return out


SINGLE = single_cases()
FORMS = single_cases((4, 1024), (65, 257), extra=False)
PAIR = [(16, c, r, 1) for c in (4, 1024) for r in (65, 257)]
K300 = [("batch", (3, 64, 17, 5)), ("instance", (2, 64, 257, 1))]
_id = lambda v: f"{v[0]}-{'x'.join(map(str, v[1]))}" if isinstance(v[0], str) else "x".join(map(str, v))


def groups_rows(kind, shape):
    b, c, p, a = shape
    return (b, p * a) if kind == "instance" else (1, b * p * a)


def affine_params(c, seed):
    """gamma of either sign in 0.5 .. 1.5, beta of either sign in 0.1 .. 0.5, as float32 values held in float64."""
    g = torch.Generator().manual_seed(seed)
    sg = torch.where(torch.rand(c, generator=g) < 0.25, -1.0, 1.0)
    gamma = ((0.5 + torch.rand(c, generator=g)) * sg).float().to(F64)
    beta = ((0.1 + 0.4 * torch.rand(c, generator=g)) * torch.where(torch.rand(c, generator=g) < 0.5, -1.0, 1.0)).float().to(F64)
    return gamma, beta


def t_of(out, P, rows, eps=EPS, frozen=False):
    """T per group and channel, broadcastable against [b, c, p, a]: P u (1 + k2), k2 from the sums the kernel sees."""
    if frozen:
        return torch.full_like(out.var, P * U)
    s1 = out.sums[..., 0] / rows
    k2 = (s1 * s1).reshape(-1, out.sums.shape[1], 1, 1) / (out.var + eps)
    return P * U * (1.0 + k2)


def fwd_tol(out, T, gamma, bf16, scale=1.0, y=None):
    g = gamma.abs().reshape(1, -1, 1, 1) if gamma is not None else 1.0
    y = out.y if y is None else y
    return 4.0 * T * g * (1.0 + out.xhat.abs()) * scale + (2.0 ** -22 + (2.0 ** -8 if bf16 else 0.0)) * y.abs()


def tau_fn(P, rows, gamma, bf16, frozen=False, eps=EPS):
    """tau = 4 x the forward tolerance of the element; |y| <= |n| < tau near the kink, so the |y| terms q |y| of the tolerance are
    covered by dividing by 1 - 4 q."""
    q = 2.0 ** -22 + (2.0 ** -8 if bf16 else 0.0)
    g = gamma.abs().reshape(1, -1, 1, 1) if gamma is not None else 1.0

    def tau(o):
        return 4.0 * (4.0 * t_of(o, P, rows, eps, frozen) * g * (1.0 + o.xhat.abs())) / (1.0 - 4.0 * q)
    return tau


def single_seed(shape, kappa):
    return shape[1] + 3 * shape[2] + kappa


def single_inputs(kind, shape, dtype, kappa, seed, affine, conv_bias=False, nudge=True, device=None):
    """The inputs of one run_single: (x float64, elements left within tau, gamma, beta, conv_bias, P, the generator for the rest).
    tests/test_norm_spec.py builds the same on the CPU and checks that nothing is left."""
    c = shape[1]
    groups, rows = groups_rows(kind, shape)
    gamma, beta = affine_params(c, seed + 7) if affine else (None, None)
    g = torch.Generator().manual_seed(seed + 13)
    bias = torch.randn(c, generator=g).float().to(F64) if conv_bias else None
    P = R.roundings(groups, rows, c)
    tau = tau_fn(P, rows, gamma.to(device) if affine and device is not None else gamma, dtype == torch.bfloat16)
    x64, left = R.real_inputs(shape, kappa, seed, tau if nudge else 0.0, kind, gamma, beta, EPS, dtype, conv_bias=bias, device=device)
    return x64, left, gamma, beta, bias, P, g


PAIR_SIDES = (("instance", False), ("instance", True), ("batch", True), ("batch", False))


def pair_inputs(shape, side_b, dtype, device=None):
    """(xa, left a, xb, left b) of test_pair_vs_fp64: side a at kappa 1, a batch side b at kappa 10, an instance one at 0."""
    kind_b, affine_b = side_b
    b, c, p, a = shape
    rows, bf = p * a, dtype == torch.bfloat16
    rb = groups_rows(kind_b, shape)
    Pa = R.roundings(b, rows, c)
    Pb = Pa if kind_b == "instance" else R.roundings(b, rows, c, fold=b)
    gamma, beta = affine_params(c, 21) if affine_b else (None, None)
    gd = gamma.to(device) if affine_b and device is not None else gamma
    xa64, la = R.real_inputs(shape, 1, 31 + c, tau_fn(Pa, rows, None, bf), "instance", dtype=dtype, device=device)
    xb64, lb = R.real_inputs(shape, 10 if kind_b == "batch" else 0, 32 + c, tau_fn(Pb, rb[1], gd, bf), kind_b, gamma, beta, EPS,
                             dtype, device=device)
    return xa64, la, xb64, lb


def frozen_stats(c, seed, use_bias):
    """Running statistics of mean 30, var 0.01 per channel (float32 values), an optional conv_bias, and the (mean, var) the frozen
    pass reads: fl32(running_mean - conv_bias), running_var."""
    g = torch.Generator().manual_seed(seed)
    rm = (30.0 + torch.randn(c, generator=g)).float()
    rv = (0.01 * (0.5 + torch.rand(c, generator=g))).float()
    bias = torch.randn(c, generator=g).float() if use_bias else None
    eff = (rm - bias) if use_bias else rm
    return rm, rv, bias, (eff.to(F64), rv.to(F64))


def frozen_inputs(shape, dtype, use_bias, device=None):
    """Inputs of test_frozen_forward_vs_fp64: (x, left, gamma, beta, rm, rv, bias, frozen statistics, P); tau from T(0)."""
    b, c, p, a = shape
    rows = b * p * a
    P = R.roundings(1, rows, c)
    gamma, beta = affine_params(c, 5 + c)
    rm, rv, bias, fs = frozen_stats(c, 17 + rows, use_bias)
    gd = gamma.to(device) if device is not None else gamma
    x, left = R.real_inputs(shape, 0, 19 + rows, tau_fn(P, rows, gd, dtype == torch.bfloat16, frozen=True), "frozen", gamma, beta, EPS,
                            dtype, frozen_stats=fs, device=device)
    return x, left, gamma, beta, rm, rv, bias, fs, P


def pair_frozen_inputs(shape, affine_b, dtype, device=None):
    """Side b of the eval-mode pair form: (x, left, gamma, beta, rm, rv, frozen statistics, P)."""
    b, c, p, a = shape
    n = b * p * a
    P = R.roundings(b, p * a, c, fold=b)
    gamma, beta = affine_params(c, 21) if affine_b else (None, None)
    rm, rv, _, fs = frozen_stats(c, 77, False)
    gd = gamma.to(device) if affine_b and device is not None else gamma
    x, left = R.real_inputs(shape, 0, 78 + c, tau_fn(P, n, gd, dtype == torch.bfloat16, frozen=True), "frozen", gamma, beta, EPS, dtype,
                            frozen_stats=fs, device=device)
    return x, left, gamma, beta, rm, rv, fs, P


FINISH_BLOCKS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 2048, 2049, 2304, 2305, 4097)


def finish_cases(widths):
    """(groups, blocks, c): every threshold at the narrow widths; c = 1024 at the thresholds of the one-level kernel and, with one
    group, on both sides of the switch to two levels (buffers stay under 20 MB)."""
    out = []
    for g in (1, 3):
        for nb in FINISH_BLOCKS:
            for c in widths:
                if c == 1024 and not (nb <= 129 or (g == 1 and nb in (2048, 2049))):
                    continue
                out.append((g, nb, c))
    return out
