"""The library's GEMMs (csrc/gemm.hip, gemm_x3.hip, gemm_tn.hip behind epn_pointcloud_amd/gemm.py) held to EXACT results at the
edges of every tile instance -- compared with `==`, not with a tolerance relative to the largest output.

1. Integer operands in [-q, q] with q^2 L < 2^24 (tests/gemm_cases.py): every product and partial sum is exact in fp32 in any
   order, so native fp32, the lossless 3 x bf16 form, the two-piece fp16 form and bf16-in / fp32-out must equal
   A.double() @ B.double().T bit for bit, and bf16-out that result rounded once.  Operands and outputs live in poisoned
   buffers (tests/gemm_ref.py Arena / place): after every call each element outside C must still hold the sentinel.  After
   every call epn_last_kernel() must name the instance the restated dispatch tables predict; the last test compares the union
   with gemm_cases.REACHABLE.
2. Real operands where integers are blind: selection matrices (one +-2^e per row against full-mantissa values: native and the
   3 x bf16 form must return the selected value bit for bit -- "no input bit is dropped" --, the two-piece form within the bound
   its header states, |entry| max(|x| 2^-22, rowmax 2^-39)), per-row powers of two (pins b_amax[n] to its row), power-of-two
   invariance incl. all-zero operands, over-reported maxima.
3. The workspace contracts of the C entry points: exactly the reported size inside a poisoned buffer, and one byte less.

The only tolerance in this file is the two-piece bound of (2.), taken from csrc/gemm.h, not from a run."""
import ctypes
from contextlib import contextmanager

import pytest
import torch

import gemm_cases as G
import gemm_ref as R

pytestmark = pytest.mark.gpu
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
EWORKSPACE = -2
RECORDED = {}          # ("nt" / "tn", form) -> instance names epn_last_kernel() reported
DONE = {}              # (part, form) -> failures of that part (each part runs once per session)


def _in_dtype(form):
    return BF16 if form.startswith("bf16") else F32


def _out_dtype(form):
    return BF16 if form == "bf16" else F32


@contextmanager
def _fp32_form(form):
    from epn_pointcloud_amd import gemm
    old = gemm.FP32_MODE
    if not form.startswith("bf16"):
        gemm.set_fp32_mode(form)
    try:
        yield gemm
    finally:
        gemm.set_fp32_mode(old)


def _last_kernel():
    from epn_pointcloud_amd import _lib
    return G.normalise(_lib.get_lib().epn_last_kernel())


def _scalar(v, gpu):
    return torch.tensor([float(v)], dtype=F32, device=gpu)


# ------------------------------------------------------------------------------------------------ NT runner
def run_nt(gpu, form, cases, flags=None, seed=0):
    """One (grouped) NT call on integer operands; returns the list of what went wrong (empty: all exact)."""
    bad = []
    dt, odt = _in_dtype(form), _out_dtype(form)
    flags = flags or tuple(("c" if c.amax else "") + ("s" if c.stats else "") for c in cases)
    for c in cases:
        G.nt_exact(c)
    As = [R.place(R.ints((c.M, c.K), c.q, seed + 2 * i + c.M, gpu, dt), c.lda or None, c.a0, c.ash) for i, c in enumerate(cases)]
    Bs = [R.place(R.ints((c.N, c.K), c.q, seed + 2 * i + 1 + c.N, gpu, dt), c.ldb or None, c.b0, c.bsh) for i, c in enumerate(cases)]
    arena = R.Arena(odt, gpu, [(c.M, c.N, c.ldc or None, c.c0, 0) for c in cases])
    sarena = R.Arena(F32, gpu, [((c.M // 32) if "s" in f else 0, c.N * 2, None, 0, 0) for c, f in zip(cases, flags)])
    stats = [sarena.t[i].view(c.M // 32, c.N, 2) if "s" in f else None for i, (c, f) in enumerate(zip(cases, flags))]
    camax = [torch.zeros(1, dtype=F32, device=gpu) if "c" in f else None for f in flags]
    aamax = [A.float().abs().max().reshape(1) if "a" in f and A.numel() else None for A, f in zip(As, flags)]
    with _fp32_form(form) as gemm:
        _last_kernel()
        gemm.gemm_nt_grouped([(A, B, C) for A, B, C in zip(As, Bs, arena.t)], out_dtype=odt, col_stats=stats, a_amax=aamax,
                             c_amax=camax)
        name = _last_kernel()
    RECORDED.setdefault(("nt", form), set()).add(name)
    want_name = G.nt_instance(form, list(cases))
    if name != want_name:
        bad.append(f"{form} {cases}: ran {name}, the dispatch tables say {want_name}")
    for i, (c, A, B, C) in enumerate(zip(cases, As, Bs, arena.t)):
        ref = (A.double() @ B.double().t()).to(odt)
        if not torch.equal(C, ref):
            d = (C.double() - ref.double()).abs()
            bad.append(f"{form} {c} [{name}]: {int((d > 0).sum())} of {d.numel()} outputs differ, max |diff| {d.max().item():g} "
                       f"first at {tuple(torch.nonzero(d > 0)[0].tolist())}")
        if camax[i] is not None:
            want = C.float().abs().max().item() if C.numel() else 0.0
            if camax[i].item() != want:
                bad.append(f"{form} {c} [{name}]: c_amax {camax[i].item()} != max|C| {want}")
        if stats[i] is not None:
            blocks = C.double().reshape(c.M // 32, 32, c.N)
            want = torch.stack((blocks.sum(1), (blocks * blocks).sum(1)), -1)
            if not torch.equal(stats[i].double(), want):
                bad.append(f"{form} {c} [{name}]: col_stats differ in {int((stats[i].double() != want).sum())} entries")
    try:
        arena.check(f"{form} {cases} [{name}]")
        sarena.check(f"{form} {cases} [{name}] col_stats")
    except AssertionError as e:
        bad.append(str(e))
    return bad


def _nt_part(gpu, part, form):
    if (part, form) not in DONE:
        bad = []
        if part == "nt_single":
            for i, c in enumerate(G.nt_single_cases(form)):
                bad += run_nt(gpu, form, [c], seed=i)
        elif part == "nt_layout":
            for i, c in enumerate(G.nt_layout_cases(form)):
                bad += run_nt(gpu, form, [c], seed=1000 + i)
        elif part == "nt_stats":
            for i, c in enumerate(G.nt_stats_cases(form)):
                bad += run_nt(gpu, form, [c], seed=2000 + i)
        elif part == "nt_groups":
            for i, (name, (probs, flags)) in enumerate(G.nt_group_cases(form).items()):
                bad += [f"group {name}: {b}" for b in run_nt(gpu, form, probs, flags, seed=3000 + 50 * i)]
        DONE[(part, form)] = bad
    return DONE[(part, form)]


def _report(bad):
    assert not bad, f"{len(bad)} failure(s):\n" + "\n".join(bad[:40])


@pytest.mark.parametrize("form", G.NT_FORMS)
def test_nt_every_instance_full_and_ragged_tiles(gpu, form):
    """Every (N, K) of the grids at the row counts {1, 31, 33, BM - 1, BM + 1, BM, 2 BM} of the instance it reaches, the K steps
    1 .. 4 of the bf16 three-stage ring, the K no fast path takes, K in {16, 48} where the split forms fall back; c_amax on
    every other case."""
    _report(_nt_part(gpu, "nt_single", form))


@pytest.mark.parametrize("form", G.NT_FORMS)
def test_nt_strides_alignment_and_guard_bands(gpu, form):
    _report(_nt_part(gpu, "nt_layout", form))


@pytest.mark.parametrize("form", G.NT_FORMS)
def test_nt_epilogue_col_stats_and_c_amax_exact(gpu, form):
    """q = 3, K <= 64: the 32-row block sums and sums of squares are integers below 2^24 -- the partials must EQUAL the fp64
    sums of the stored tensor (ragged last row tile, ragged N, the generic kernel's passes over C, bf16 output)."""
    _report(_nt_part(gpu, "nt_stats", form))


@pytest.mark.parametrize("form", G.NT_FORMS)
def test_nt_grouped_launches(gpu, form):
    """2, 3, 5, 6, 7 and 13 problems, K ascending (the launcher re-sorts), tile counts that are no multiples of 8, M == 0 in the
    middle, the grouped routes of each form, a member that takes the whole group off the split forms, mixed None / given
    col_stats, c_amax and a_amax."""
    _report(_nt_part(gpu, "nt_groups", form))


def test_nt_many_tile_route(gpu):
    """fp32, one problem, N = 256, M = 245760, K = 32: (M / 128) (N / 128) = 3840, the 128 x 128 tiles the benchmark runs on."""
    if ("nt_many", "native") not in DONE:
        DONE[("nt_many", "native")] = run_nt(gpu, "native", [G.MANY_TILE], seed=7)
    _report(DONE[("nt_many", "native")])


# ------------------------------------------------------------------------------------------------ TN runner
def run_tn(gpu, mode, cases, grouped=False, seed=0, over=None):
    """One TN call (or one grouped call) on integers in [-8, 8], run twice; over: factor by which x_amax / y_amax over-report."""
    bad = []
    dt = BF16 if mode == "bf16" else F32
    for c in cases:
        G.tn_exact(c)
    Xs = [R.place(R.ints((c.R, c.N1), G.Q_TN, seed + 2 * i + c.R, gpu, dt), c.ldx or None, c.x0, c.xsh) for i, c in enumerate(cases)]
    Ys = [R.place(R.ints((c.R, c.N2), G.Q_TN, seed + 2 * i + 1 + c.N2, gpu, dt), c.ldy or None, c.y0, c.ysh) for i, c in enumerate(cases)]
    arena = R.Arena(F32, gpu, [(c.N1, c.N2, c.ldc or None, c.c0, 0) for c in cases])
    xa = [_scalar(G.Q_TN * over, gpu) for _ in cases] if over else None
    ya = [_scalar(G.Q_TN * over, gpu) for _ in cases] if over else None
    first = []
    with _fp32_form(mode) as gemm:
        for rep in range(2):
            _last_kernel()
            if grouped:
                gemm.gemm_tn_grouped(list(zip(Xs, Ys)), outs_into=arena.t, x_amax=xa, y_amax=ya)
            else:
                gemm.gemm_tn(Xs[0], Ys[0], out=arena.t[0], x_amax=xa and xa[0], y_amax=ya and ya[0],
                             fp32_mode=None if mode == "bf16" else mode)
            name = _last_kernel()
            if rep == 0:
                first = [C.clone() for C in arena.t]
    RECORDED.setdefault(("tn", mode), set()).add(name)
    want_name = G.tn_instance(mode, list(cases))
    if name != want_name:
        bad.append(f"{mode} {cases}: ran {name}, the plan says {want_name}")
    for c, X, Y, C, C0 in zip(cases, Xs, Ys, arena.t, first):
        ref = (X.double().t() @ Y.double()).float()
        if not torch.equal(C, ref):
            d = (C.double() - ref.double()).abs()
            bad.append(f"{mode} {c} [{name}]: {int((d > 0).sum())} of {d.numel()} outputs differ, max |diff| {d.max().item():g} "
                       f"first at {tuple(torch.nonzero(d > 0)[0].tolist())}")
        if not torch.equal(C, C0):
            bad.append(f"{mode} {c} [{name}]: the second call differs from the first")
    try:
        arena.check(f"{mode} {cases} [{name}]")
    except AssertionError as e:
        bad.append(str(e))
    return bad


def _tn_part(gpu, part, mode):
    if (part, mode) not in DONE:
        bad = []
        if part == "tn_widths":
            for i, c in enumerate(G.tn_width_cases()):
                bad += run_tn(gpu, mode, [c], seed=i)
        elif part == "tn_rows":
            for i, c in enumerate(G.tn_row_cases(mode)):
                bad += run_tn(gpu, mode, [c], seed=500 + i)
        elif part == "tn_layout":
            for i, c in enumerate(G.tn_layout_cases()):
                bad += run_tn(gpu, mode, [c], seed=900 + i)
        elif part == "tn_groups":
            for i, (name, probs) in enumerate(G.TN_GROUPS.items()):
                bad += [f"group {name}: {b}" for b in run_tn(gpu, mode, probs, grouped=True, seed=1200 + 20 * i)]
        DONE[(part, mode)] = bad
    return DONE[(part, mode)]


@pytest.mark.parametrize("mode", G.TN_MODES)
def test_tn_every_tile_choice(gpu, mode):
    """R = 32; N1 x N2 one below, at and above every threshold of gemm_tn_tile: each (bn1, bn2) per mode, the bf16 ring form
    (N2 <= 128), the pre-split planes form (N2 >= 512)."""
    _report(_tn_part(gpu, "tn_widths", mode))


@pytest.mark.parametrize("mode", G.TN_MODES)
def test_tn_rows_splits_and_reductions(gpu, mode):
    """R without a fast path (1, 31, 33, 100), the first split (2048), a last split that ends inside a stage (2080), an odd split
    count (3), 17 and 65 partial slabs (the shared-quad reductions); the split counts are pinned against the workspace queries in
    tests/test_gemm_spec.py."""
    _report(_tn_part(gpu, "tn_rows", mode))


@pytest.mark.parametrize("mode", G.TN_MODES)
def test_tn_strides_alignment_and_guard_bands(gpu, mode):
    _report(_tn_part(gpu, "tn_layout", mode))


@pytest.mark.parametrize("mode", G.TN_MODES)
def test_tn_grouped_launches(gpu, mode):
    """2, 5 and 6 problems of unequal R and widths into regions of ONE poisoned buffer, every call repeated bitwise."""
    _report(_tn_part(gpu, "tn_groups", mode))


# ------------------------------------------------------------------------------------------------ 2. structured real operands
FP32_FORMS = ("native", "split", "f16x2")
F2_WORST = {}          # worst observed error / bound of the two-piece form per test (printed: DESIGN 4 quotes it)


def _within_f2(C, want64, entry, x64, xmax, key):
    """|C - want| <= |entry| max(|x| 2^-22, xmax 2^-39); want = entry * x exactly (float64)."""
    bound = entry.abs() * torch.maximum(x64.abs() * 2.0 ** -22, xmax * 2.0 ** -39)
    ratio = ((C.double() - want64).abs() / bound).max().item()
    F2_WORST[key] = max(F2_WORST.get(key, 0.0), ratio)
    print(f"two-piece form, {key}: worst |error| / bound = {ratio:.4f}")
    return ratio <= 1.0


@pytest.mark.parametrize("form", FP32_FORMS)
@pytest.mark.parametrize("M,N,K", [(300, 130, 96), (33, 320, 32), (513, 64, 64), (257, 256, 48)])
def test_nt_selection_matrices(gpu, form, M, N, K):
    """A selects (one +-2^e per row), B full-mantissa: C[m, n] = +-2^e B[n, k(m)]; then the roles swapped."""
    with _fp32_form(form) as gemm:
        A, k, v = R.selection_rows(M, K, M + K, gpu)
        B = R.full_mantissa((N, K), N + K, gpu)
        C = gemm.gemm_nt(A, B)
        want = v.double()[:, None] * B.double()[:, k].t()
        if form == "f16x2" and K % 32 == 0:
            rowmax = B.double().abs().amax(1)[None, :].expand(M, N)
            assert _within_f2(C, want, v.double()[:, None], B.double()[:, k].t(), rowmax, "NT, A selects")
        else:
            assert torch.equal(C.double(), want)
        Bs, k, v = R.selection_rows(N, K, 3 * N + K, gpu)
        Af = R.full_mantissa((M, K), 5 * M + K, gpu)
        C = gemm.gemm_nt(Af, Bs)
        want = Af.double()[:, k] * v.double()[None, :]
        if form == "f16x2" and K % 32 == 0:
            amax = Af.double().abs().max()
            assert _within_f2(C, want, v.double()[None, :], Af.double()[:, k], amax, "NT, B selects")
        else:
            assert torch.equal(C.double(), want)


@pytest.mark.parametrize("mode", FP32_FORMS)
@pytest.mark.parametrize("R_,N1,N2", [(2080, 64, 136), (96, 72, 520), (3072, 264, 512), (100, 40, 24)])
def test_tn_selection_matrices(gpu, mode, R_, N1, N2):
    """X selects (one +-2^e per column, in distinct rows): C[n1, :] = +-2^e Y[r(n1), :] through every split and reduction."""
    from epn_pointcloud_amd import gemm
    X, r, v = R.selection_cols(R_, N1, R_ + N1, gpu)
    Y = R.full_mantissa((R_, N2), R_ + N2, gpu)
    C = gemm.gemm_tn(X, Y, fp32_mode=mode)
    want = v.double()[:, None] * Y.double()[r, :]
    if mode == "f16x2" and R_ % 32 == 0:
        assert _within_f2(C, want, v.double()[:, None], Y.double()[r, :], Y.double().abs().max(), "TN, X selects")
    else:
        assert torch.equal(C.double(), want)


@pytest.mark.parametrize("form", ("native", "split"))
def test_twelve_bit_products_are_exact(gpu, form):
    """Selection entries and values of twelve significant bits: every product has at most 24 and is exact in fp32, and both
    operands have a non-zero middle bf16 piece -- the m x m term of the three-piece forms (weight 2^-16) must be there."""
    with _fp32_form(form) as gemm:
        for M, N, K in ((300, 130, 96), (33, 320, 32)):
            A, k, v = R.selection_rows(M, K, M + K, gpu)
            A = A * R.twelve_bit((M, 1), M, gpu)
            B = R.twelve_bit((N, K), N + K, gpu)
            assert torch.equal(gemm.gemm_nt(A, B).double(), A.double() @ B.double().t())
        for R_, N1, N2 in ((2080, 64, 136), (96, 72, 520), (3072, 264, 512), (64, 40, 264)):
            X, r, v = R.selection_cols(R_, N1, R_ + N1, gpu)
            X = X * R.twelve_bit((1, N1), N1, gpu)
            Y = R.twelve_bit((R_, N2), R_ + N2, gpu)
            assert torch.equal(gemm.gemm_tn(X, Y, fp32_mode=form).double(), X.double().t() @ Y.double()), (R_, N1, N2)
        Xs = [R.selection_cols(c.R, c.N1, 7 + c.R, gpu)[0] * R.twelve_bit((1, c.N1), c.N1, gpu) for c in G.TN_GROUPS["five_spectral"]]
        Ys = [R.twelve_bit((c.R, c.N2), 9 + c.R, gpu) for c in G.TN_GROUPS["five_spectral"]]
        for X, Y, C in zip(Xs, Ys, gemm.gemm_tn_grouped(list(zip(Xs, Ys)))):
            assert torch.equal(C.double(), X.double().t() @ Y.double())


@pytest.mark.parametrize("form", G.NT_FORMS)
@pytest.mark.parametrize("N", [129, 320])
def test_nt_row_scales_stay_with_their_rows(gpu, form, N):
    """Integer B whose row n carries 2^((7 n mod 41) - 20): every form stays exact, so the per-row scale of the two-piece weight
    split (b_amax[n], rowmax) is applied to ITS row across tile and wave boundaries."""
    dt, odt = _in_dtype(form), _out_dtype(form)
    M, K = 257, 64
    A = R.ints((M, K), G.Q_NT, N, gpu, dt)
    B = (R.ints((N, K), G.Q_NT, N + 1, gpu).double() * R.row_scales(N, gpu).double()[:, None]).to(dt)
    with _fp32_form(form) as gemm:
        C = gemm.gemm_nt(A, B, out_dtype=odt)
    assert torch.equal(C, (A.double() @ B.double().t()).to(odt))


@pytest.mark.parametrize("form", FP32_FORMS)
def test_power_of_two_invariance_and_zero_operands(gpu, form):
    """gemm(A 2^p, B 2^q) == gemm(A, B) 2^(p + q) bitwise; all-zero operands give exact zeros and leave the overflow counter at 0
    (the e < 14 clamp of f2_scale_of)."""
    with _fp32_form(form) as gemm:
        A = R.full_mantissa((257, 96), 1, gpu)
        B = R.full_mantissa((130, 96), 2, gpu)
        X = R.full_mantissa((2080, 72), 3, gpu)
        Y = R.full_mantissa((2080, 136), 4, gpu)
        two = lambda t, e: t * (2.0 ** e)          # (an exact scalar: the device's ldexp goes through pow)
        C0, D0 = gemm.gemm_nt(A, B), gemm.gemm_tn(X, Y, fp32_mode=form)
        for p, q in ((-100, 60), (-20, 20), (20, -20), (100, -60), (40, 40)):
            assert torch.equal(gemm.gemm_nt(two(A, p), two(B, q)), two(C0, p + q)), (p, q)
            assert torch.equal(gemm.gemm_tn(two(X, p), two(Y, q), fp32_mode=form), two(D0, p + q)), (p, q)
        for a, b in ((torch.zeros_like(A), B), (A, torch.zeros_like(B))):
            assert bool((gemm.gemm_nt(a, b) == 0).all().item())
        for x, y in ((torch.zeros_like(X), Y), (X, torch.zeros_like(Y))):
            assert bool((gemm.gemm_tn(x, y, fp32_mode=form) == 0).all().item())
        assert gemm.f16x2_overflow_count() == 0


@pytest.mark.parametrize("over", [1, 2, 1024])
def test_over_reported_maxima_stay_exact(gpu, over):
    """a_amax / x_amax / y_amax at 1, 2 and 1024 times the true maximum, integers in [-8, 8]: low bits may go, correctness not."""
    with _fp32_form("f16x2") as gemm:
        for M, N, K in ((300, 130, 64), (33, 40, 32)):
            A, B = R.ints((M, K), 8, M, gpu), R.ints((N, K), 8, N, gpu)
            C = gemm.gemm_nt(A, B, a_amax=_scalar(8 * over, gpu))
            assert torch.equal(C.double(), A.double() @ B.double().t())
    bad = []
    for c in (G.TnCase(2080, 64, 136), G.TnCase(64, 72, 520)):
        bad += run_tn(gpu, "f16x2", [c], over=over)
    bad += run_tn(gpu, "f16x2", G.TN_GROUPS["five_spectral"], grouped=True, over=over)
    _report(bad)


def test_wrappers_refuse_what_they_do_not_take(gpu):
    """The refusals of gemm.py that need device tensors to be reached (the wrappers look at .is_cuda first)."""
    from epn_pointcloud_amd import gemm
    f = lambda *s, dt=F32: torch.zeros(*s, dtype=dt, device=gpu)
    with pytest.raises(ValueError, match="K mismatch"):
        gemm.gemm_nt(f(8, 32), f(8, 64))
    with pytest.raises(TypeError, match="mixed"):
        gemm.gemm_nt(f(8, 32), f(8, 32, dt=BF16))
    with pytest.raises(TypeError, match="float32 or bfloat16"):
        gemm.gemm_nt(f(8, 32, dt=torch.float16), f(8, 32, dt=torch.float16))
    with pytest.raises(ValueError, match="2-D"):
        gemm.gemm_nt(f(32), f(8, 32))
    for out in (f(8, 9), f(8, 8, dt=BF16)):
        with pytest.raises(ValueError, match="output"):
            gemm.gemm_nt(f(8, 32), f(8, 32), out=out)
    with pytest.raises(ValueError, match="output"):
        gemm.gemm_nt(f(8, 32), f(8, 32), out=f(8, 16)[:, ::2])
    for part in (f(1, 8, 2), f(2, 8, 3), f(2, 8, 2, dt=BF16), f(2, 16, 2)[:, ::2]):
        with pytest.raises(ValueError, match="col_stats"):
            gemm.gemm_nt_grouped([(f(64, 32), f(8, 32), None)], col_stats=[part])
    with pytest.raises(ValueError, match="col_stats"):
        gemm.gemm_nt_grouped([(f(48, 32), f(8, 32), None)], col_stats=[f(1, 8, 2)])
    for am in (f(2), f(1, dt=BF16), torch.zeros(1)):
        with pytest.raises(ValueError, match="amax"):
            gemm.gemm_nt_grouped([(f(64, 32), f(8, 32), None)], c_amax=[am])
    with pytest.raises(ValueError, match="row mismatch"):
        gemm.gemm_tn(f(32, 8), f(64, 8))
    with pytest.raises(TypeError, match="mixed"):
        gemm.gemm_tn(f(32, 8), f(32, 8, dt=BF16))
    for out in (f(8, 9), f(8, 8, dt=BF16), f(8, 16)[:, ::2]):
        with pytest.raises(ValueError, match="output"):
            gemm.gemm_tn(f(32, 8), f(32, 8), out=out)
    with pytest.raises(ValueError, match="contiguous"):
        gemm.gemm_tn_grouped([(f(32, 8), f(32, 8))], outs_into=[f(8, 12)[:, :8]])
    with pytest.raises(ValueError, match="row mismatch"):
        gemm.gemm_tn_grouped([(f(32, 8), f(64, 8))])


# ------------------------------------------------------------------------------------------------ 3. workspace contracts (C ABI)
def _ws(gpu, nbytes):
    """A workspace of exactly nbytes inside a poisoned byte buffer (16-byte aligned)."""
    return R.guarded(1, nbytes, torch.uint8, gpu)


def _tn_call(lib, mode, X, Y, C, ws_ptr, ws_bytes, st):
    a = (X.data_ptr(), X.stride(0), Y.data_ptr(), Y.stride(0), C.data_ptr(), C.stride(0), X.shape[0], X.shape[1], Y.shape[1])
    if mode == "f16x2":
        return lib.epn_gemm_tn_f16x2_f32(*a, None, None, ws_ptr, ws_bytes, st)
    fn = {"native": lib.epn_gemm_tn_f32, "split": lib.epn_gemm_tn_split_f32, "bf16": lib.epn_gemm_tn_bf16}[mode]
    return fn(*a, ws_ptr, ws_bytes, st)


@pytest.mark.parametrize("mode", G.TN_MODES)
@pytest.mark.parametrize("R_,N1,N2", [(3072, 64, 64), (64, 64, 512), (2080, 264, 520)], ids=["three_splits", "planes", "splits_planes"])
def test_tn_entry_workspace_contract(gpu, mode, R_, N1, N2):
    from epn_pointcloud_amd import _lib
    lib = _lib.get_lib()
    dt = BF16 if mode == "bf16" else F32
    X, Y = R.ints((R_, N1), 8, 1, gpu, dt), R.ints((R_, N2), 8, 2, gpu, dt)
    need = int(lib.epn_gemm_tn_workspace_bytes(G.TN_MODE_ID[mode], R_, N1, N2))
    assert need == G.tn_workspace(mode, G.TnCase(R_, N1, N2))
    st = _lib.stream_of(X)
    ca, C = R.guarded(N1, N2, F32, gpu)
    wa, ws = _ws(gpu, need)
    assert _tn_call(lib, mode, X, Y, C, ws.data_ptr() if need else None, need, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(C.double(), X.double().t() @ Y.double())
    ca.check("C"), wa.check("workspace")
    if need:
        ca2, C2 = R.guarded(N1, N2, F32, gpu)
        assert _tn_call(lib, mode, X, Y, C2, ws.data_ptr(), need - 1, st) == EWORKSPACE
        assert _tn_call(lib, mode, X, Y, C2, None, need, st) == EWORKSPACE
        torch.cuda.synchronize()
        assert ca2.untouched()


@pytest.mark.parametrize("mode", G.TN_MODES)
@pytest.mark.parametrize("group", ["five_long", "two_256"])
def test_tn_grouped_entry_workspace_contract(gpu, mode, group):
    from epn_pointcloud_amd import _lib
    lib = _lib.get_lib()
    dt = BF16 if mode == "bf16" else F32
    cases = G.TN_GROUPS[group]
    Xs = [R.ints((c.R, c.N1), 8, 3 + i, gpu, dt) for i, c in enumerate(cases)]
    Ys = [R.ints((c.R, c.N2), 8, 30 + i, gpu, dt) for i, c in enumerate(cases)]

    def problems(outs):
        arr = (_lib.GemmTnProblem * len(cases))()
        for p, c, X, Y, C in zip(arr, cases, Xs, Ys, outs):
            p.X, p.Y, p.C, p.R, p.N1, p.N2, p.ldx, p.ldy, p.ldc = X.data_ptr(), Y.data_ptr(), C.data_ptr(), c.R, c.N1, c.N2, c.N1, c.N2, c.N2
        return arr

    def call(arr, ws_ptr, nbytes):
        if mode == "f16x2":
            return lib.epn_gemm_tn_grouped_f16x2(len(cases), arr, None, None, ws_ptr, nbytes, _lib.stream_of(Xs[0]))
        return lib.epn_gemm_tn_grouped(G.TN_MODE_ID[mode], len(cases), arr, ws_ptr, nbytes, _lib.stream_of(Xs[0]))

    ca = R.Arena(F32, gpu, [(c.N1, c.N2, None, 0, 0) for c in cases])
    arr = problems(ca.t)
    need = int(lib.epn_gemm_tn_grouped_workspace_bytes(G.TN_MODE_ID[mode], len(cases), arr))
    assert need > 0 or (group == "two_256" and mode in ("native", "bf16"))      # (one chunk each, nothing pre-split: no workspace)
    wa, ws = _ws(gpu, need)
    assert call(arr, ws.data_ptr() if need else None, need) == 0
    torch.cuda.synchronize()
    for X, Y, C in zip(Xs, Ys, ca.t):
        assert torch.equal(C.double(), X.double().t() @ Y.double())
    ca.check("C"), wa.check("workspace")
    if need:
        ca2 = R.Arena(F32, gpu, [(c.N1, c.N2, None, 0, 0) for c in cases])
        assert call(problems(ca2.t), ws.data_ptr(), need - 1) == EWORKSPACE
        torch.cuda.synchronize()
        assert ca2.untouched()


@pytest.mark.parametrize("nprob", [1, 7])
def test_nt_f16x2_entry_workspace_contract(gpu, nprob):
    """epn_gemm_nt_f16x2_f32 with exactly epn_gemm_nt_f16x2_workspace_bytes (7 problems: two launches, two carvings), and one
    byte less: EPN_EWORKSPACE, C untouched (this entry has no fallback for a short workspace)."""
    from epn_pointcloud_amd import _lib
    lib = _lib.get_lib()
    cases = [G.NtCase(70 + 31 * i, (40, 130, 257)[i % 3], (32, 64, 96)[i % 3]) for i in range(nprob)]
    As = [R.ints((c.M, c.K), 64, i, gpu) for i, c in enumerate(cases)]
    Bs = [R.ints((c.N, c.K), 64, 20 + i, gpu) for i, c in enumerate(cases)]

    def problems(outs):
        arr = (_lib.GemmNtProblem * nprob)()
        for p, c, A, B, C in zip(arr, cases, As, Bs, outs):
            p.A, p.Bt, p.C, p.M, p.N, p.K, p.lda, p.ldb, p.ldc = A.data_ptr(), B.data_ptr(), C.data_ptr(), c.M, c.N, c.K, c.K, c.K, c.N
        return arr

    ca = R.Arena(F32, gpu, [(c.M, c.N, None, 0, 0) for c in cases])
    arr = problems(ca.t)
    need = int(lib.epn_gemm_nt_f16x2_workspace_bytes(nprob, arr))
    assert need > 0
    wa, ws = _ws(gpu, need)
    st = _lib.stream_of(As[0])
    assert lib.epn_gemm_nt_f16x2_f32(nprob, arr, None, ws.data_ptr(), need, st) == 0
    torch.cuda.synchronize()
    assert "gemm_nt_x3_kernel" in _last_kernel()
    for A, B, C in zip(As, Bs, ca.t):
        assert torch.equal(C.double(), A.double() @ B.double().t())
    ca.check("C"), wa.check("workspace")
    if nprob == 1:
        ca2 = R.Arena(F32, gpu, [(c.M, c.N, None, 0, 0) for c in cases])
        assert lib.epn_gemm_nt_f16x2_f32(nprob, problems(ca2.t), None, ws.data_ptr(), need - 1, st) == EWORKSPACE
        torch.cuda.synchronize()
        assert ca2.untouched()


# ------------------------------------------------------------------------------------------------ instance coverage (last)
def test_every_reachable_instance_was_run(gpu):
    """The union of the instances epn_last_kernel() named during this module's cases equals gemm_cases.REACHABLE per form: a
    dispatch branch nobody reaches, or a new instance nobody lists, fails here.  (Parts deselected from the run are run now.)"""
    bad = []
    for form in G.NT_FORMS:
        for part in ("nt_single", "nt_layout", "nt_stats", "nt_groups"):
            bad += _nt_part(gpu, part, form)
    if ("nt_many", "native") not in DONE:
        DONE[("nt_many", "native")] = run_nt(gpu, "native", [G.MANY_TILE], seed=7)
    for mode in G.TN_MODES:
        for part in ("tn_widths", "tn_rows", "tn_layout", "tn_groups"):
            bad += _tn_part(gpu, part, mode)
    for key, want in G.REACHABLE.items():
        got = RECORDED.get(key, set())
        assert got == want, f"{key}: never ran {sorted(want - got)}; ran but not listed {sorted(got - want)}"
    _report(bad)
