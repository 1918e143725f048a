"""The Adam step on the GPU (csrc/adam_step.hip behind optim.FlatAdam) against the numpy fp64 restatement of its specification
(tests/adam_ref.py), and against torch.optim.Adam.

Tolerance.  The kernel computes in fp64 and rounds every stored value once, so a float output is compared with the restatement's
value rounded to fp32 and may differ from it by ONE fp32 ulp of that value (the `one_ulp` rule of test_gpu_cls_loss.py): the two
fp64 values differ by the order of the sum of squares and by the pow / sqrt / division implementations, of order 1e-16 relative
(1e-10 for the norm of a million elements) -- far below half an fp32 ulp, but enough to straddle a rounding boundary.  NaN and inf
are expected exactly where the restatement has them; integers are exact.  Against torch in fp64 the bound is the one derived in
test_adam_spec.py: 2^-22 max(|p|, |p'|).

A finite gradient whose sum of squares overflows to inf in fp64 cannot arise from fp32 inputs: fewer than 2^40 squares, each
below 2^256, stay below 2^296, far inside fp64's 2^1024.  No test is built for it.

Measured on an MI355X when this file was written: every float output of every case equalled the restatement's value rounded to
fp32 bit for bit (largest error 0 ulp, exact in 100 % of the elements; each test prints both figures).  Against torch in fp64 the
largest distance was 0.23 of the bound on the synthetic state (torch's own fp32 step: 0.28) and 0.72 on the tiny network."""
import numpy as np
import pytest
import torch

import adam_ref as R
from test_adam_spec import P_BOUND

pytestmark = pytest.mark.gpu

SPAN = R.SPAN


def H(t):
    return t.detach().cpu().numpy()


def close(got, ref, what):
    """|got - fp32(ref)| <= ulp(fp32(ref)) elementwise; NaN and inf exactly where fp32(ref) has them; prints the largest error."""
    got = np.asarray(H(got) if isinstance(got, torch.Tensor) else got)
    with np.errstate(over="ignore", invalid="ignore"):
        ref32 = np.asarray(ref, dtype=np.float64).astype(np.float32)
    assert got.shape == ref32.shape, (what, got.shape, ref32.shape)
    special = ~np.isfinite(ref32)
    same_special = np.array_equal(np.isnan(got), np.isnan(ref32)) and np.array_equal(got[special & ~np.isnan(ref32)],
                                                                                      ref32[special & ~np.isnan(ref32)])
    err = np.abs(got[~special].astype(np.float64) - ref32[~special].astype(np.float64))
    ulp = np.spacing(np.abs(ref32[~special])).astype(np.float64)
    print(f"{what}: largest err {float((err / ulp).max()) if err.size else 0:.3f} ulp, exact in "
          f"{float((err == 0).mean()) if err.size else 1:.4f} of {err.size}")
    return bool(same_special and np.isfinite(got[~special]).all() and (err <= ulp).all())


class Rig:
    """FlatAdam over parameters of the given lengths next to the restatement's state.  A length given as ('slice', L) is a
    parameter that is the [1:] slice of a tensor of L + 1 elements: its address is 4 bytes off a 16-byte boundary."""

    def __init__(self, gpu, lengths, p, m=None, v=None, counters=(0, 0), **kw):
        from epn_pointcloud_amd import optim
        self.gpu = gpu
        self.lengths = [x[1] if isinstance(x, tuple) else x for x in lengths]
        self.off = R.offsets(self.lengths)
        self.ref = R.State(p, m, v, counters)
        self.params, self.bases = [], []
        for spec, a, b in zip(lengths, self.off[:-1], self.off[1:]):
            chunk = torch.from_numpy(self.ref.p[a:b].copy()).to(gpu)
            if isinstance(spec, tuple):
                base = torch.zeros(b - a + 1, device=gpu)
                base[1:] = chunk
                self.bases.append(base)
                chunk = base[1:].detach()
                assert chunk.data_ptr() % 16 == 4 and chunk.is_contiguous()
            self.params.append(chunk.requires_grad_())
        self.hyper = dict(lr=kw.pop("lr", 1e-3), beta1=kw.get("betas", (0.9, 0.999))[0], beta2=kw.get("betas", (0.9, 0.999))[1],
                          eps=kw.get("eps", 1e-8), weight_decay=kw.get("weight_decay", 0.0), max_norm=kw.get("max_norm"),
                          grad_scale=1.0 / kw.get("world", 1))
        self.opt = optim.FlatAdam(self.params, lr=self.hyper["lr"], **kw)
        if m is not None:
            self.opt.exp_avg.copy_(torch.from_numpy(self.ref.m))
        if v is not None:
            self.opt.exp_avg_sq.copy_(torch.from_numpy(self.ref.v))
        self.opt.counters.copy_(torch.tensor(self.ref.counters, dtype=torch.int32))
        assert self.opt.n == self.off[-1]

    def set_grad(self, g):
        self.opt.grad_buckets.flat.copy_(torch.from_numpy(np.ascontiguousarray(g, dtype=np.float32)))

    def step(self, g):
        """One step of both with gradient g -> the restatement's info."""
        self.set_grad(g)
        self.opt.step()
        h = dict(self.hyper)
        return R.step(self.ref, g, h.pop("lr"), **h)

    def device_state(self):
        torch.cuda.synchronize()
        return (np.concatenate([H(p).ravel() for p in self.params]), H(self.opt.exp_avg), H(self.opt.exp_avg_sq),
                H(self.opt.last_info()), self.opt.counters.tolist())

    def agrees(self, info, what):
        p, m, v, dinfo, counters = self.device_state()
        ok = close(p, self.ref.p, what + " p") and close(m, self.ref.m, what + " m") and close(v, self.ref.v, what + " v")
        ok = ok and close(dinfo, info, what + " info")
        return ok and counters == self.ref.counters


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def data(n, seed, steps=10):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n).astype(np.float32), [(0.1 * rng.standard_normal(n)).astype(np.float32) for _ in range(steps)]


# ----------------------------------------------------------------------------------------------- layouts
LAYOUTS = {
    "one": [1], "three": [3], "four_five": [4, 5], "one_to_eight": list(range(1, 9)),
    "span_minus_1": [SPAN - 1], "span": [SPAN], "span_plus_1": [SPAN + 1], "two_spans_split_inside": [SPAN - 2, 7, SPAN - 5],
    "odd_offset_70001": [5, 70001], "sliced_parameter": [8, ("slice", 2 * SPAN + 3), 6],
}


@pytest.mark.parametrize("name", LAYOUTS)
def test_layouts_follow_the_restatement_for_ten_steps(gpu, name):
    """p, exp_avg, exp_avg_sq, info and the counters after steps 1, 2, 3 and 10, with weight decay and clipping switched on so
    that every term of the update is live.  The layouts put segment boundaries at every position inside a quad, one element
    below, at and above the chunk a workgroup iteration covers, a long segment at an odd flat offset (the flat buffers are
    read 16 bytes wide, its parameter element by element) and a parameter whose own address is off the 16-byte grid."""
    lengths = LAYOUTS[name]
    n = sum(x[1] if isinstance(x, tuple) else x for x in lengths)
    p, grads = data(n, 100 + n)
    rig = Rig(gpu, lengths, p, lr=1e-2, weight_decay=0.01, max_norm=0.5 * float(np.sqrt(n) * 0.1))
    for k, g in enumerate(grads, 1):
        info = rig.step(g)
        if k in (1, 2, 3, 10):
            assert rig.agrees(info, f"{name} step {k}")
    assert rig.opt.counters.tolist() == [10, 0]
    if rig.bases:
        assert float(rig.bases[0][0]) == 0.0                     # the element in front of the sliced parameter is untouched


def test_more_than_one_chunk_per_workgroup(gpu):
    """Beyond 2048 chunks a workgroup owns several: n = 2^21 + 2051 gives two chunks each, in three segments whose boundaries
    fall inside a workgroup's range.  Two steps."""
    lengths = [(1 << 20) + 1, 3, (1 << 20) + 2047]
    p, grads = data(sum(lengths), 7, steps=2)
    rig = Rig(gpu, lengths, p, max_norm=1.0)
    for k, g in enumerate(grads, 1):
        assert rig.agrees(rig.step(g), f"two chunks per workgroup, step {k}")


# ----------------------------------------------------------------------------------------------- values
def test_zero_gradients_leave_the_parameters_bitwise(gpu):
    p, _ = data(2 * SPAN + 3, 3)
    p[:4] = [0.0, -0.0, 1e-42, -3e-39]                           # zeros of both signs and subnormals keep their bits too
    rig = Rig(gpu, [SPAN + 1, SPAN + 2], p)
    info = rig.step(np.zeros_like(p))
    got = rig.device_state()
    assert np.array_equal(bits(got[0]), bits(p)) and not got[1].any() and not got[2].any()
    assert got[4] == [1, 0] and got[3].tolist() == [0.0, 1.0, float(np.float32(1e-3)), 0.0] and info[0] == 0.0


@pytest.mark.parametrize("mag", (1e18, 1e20, 1e-30, 1e-41), ids=("1e18", "1e20_square_overflows_fp32", "1e-30", "subnormal"))
def test_extreme_gradient_magnitudes(gpu, mag):
    """|g| = 1e18: g^2 = 1e36 is still an fp32 number.  1e20: (1 - beta2) g^2 = 1e37 fits but the second step's does not... the
    restatement decides; where v' = inf the update is 0.  1e-30: g^2 underflows fp32 entirely.  1e-41: g itself is subnormal.
    Three steps each, both signs, p among them subnormal."""
    n = SPAN + 9
    rng = np.random.default_rng(5)
    p = rng.standard_normal(n).astype(np.float32)
    p[::7] = np.float32(2e-40)
    rig = Rig(gpu, [3, n - 3], p)
    for k in range(3):
        g = (np.float32(mag) * (10.0 ** k) * np.sign(rng.standard_normal(n))).astype(np.float32)
        assert np.isfinite(g).all()
        assert rig.agrees(rig.step(g), f"|g| = {mag:g} x 1e{k}")
    if mag == 1e20:
        assert np.isinf(rig.ref.v).all()                          # the case the issue names did occur
    if mag < 1:
        assert (rig.ref.v == 0).all() and (rig.ref.m != 0).all()


def test_an_update_that_cancels_the_parameter(gpu):
    """p = fl32(update): p' is the rounding residue, some 2^-25 of p, and still within one ulp OF ITSELF."""
    n = SPAN + 5
    _, grads = data(n, 9, steps=1)
    probe = R.State(np.zeros(n, dtype=np.float32))
    R.step(probe, grads[0], 1e-3)
    p = -probe.p
    rig = Rig(gpu, [n], p)
    assert rig.agrees(rig.step(grads[0]), "cancelling update")
    assert (np.abs(rig.ref.p) <= 2.0 ** -23 * np.abs(p)).all() and (rig.ref.p != 0).any()


def test_large_step_count(gpu):
    """t = 100001: beta1^t underflows to 0 and 1 - beta2^t rounds to 1 in fp64; t = 2^31 - 1 is the last count an int32 holds."""
    n = 77
    p, grads = data(n, 13, steps=2)
    rng = np.random.default_rng(14)
    m, v = (0.05 * rng.standard_normal(n)).astype(np.float32), (0.01 * rng.random(n)).astype(np.float32)
    for t0 in (100000, 2 ** 31 - 2):
        rig = Rig(gpu, [n], p, m, v, counters=(t0, 4))
        assert rig.agrees(rig.step(grads[0]), f"t = {t0 + 1}")
        assert rig.opt.counters.tolist() == [t0 + 1, 4]


# ----------------------------------------------------------------------------------------------- skip
@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf), ids=("nan", "inf", "minus_inf"))
def test_a_non_finite_gradient_skips_the_step(gpu, bad):
    lengths = [5, 70001, 3]
    n = sum(lengths)
    p, grads = data(n, 21, steps=4)
    rig = Rig(gpu, lengths, p, max_norm=1.0, weight_decay=0.01)
    for k, pos in enumerate((0, n - 1, 5 + 33333)):
        before = rig.device_state()
        g = grads[k].copy()
        g[pos] = bad
        info = rig.step(g)
        after = rig.device_state()
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(before[:3], after[:3])), pos
        assert after[4] == [before[4][0], before[4][1] + 1] == rig.ref.counters
        assert after[3][3] == 1.0 and info[3] == 1.0 and close(after[3], info, f"skip at {pos} info")
        if k == 0:                                               # the next clean step is the first: t = 1
            assert rig.ref.counters[0] == 0
            assert rig.agrees(rig.step(grads[3]), "clean step after a skip")
            assert rig.opt.counters.tolist() == [1, 1]
    assert rig.opt.counters.tolist() == [1, 3]


# ----------------------------------------------------------------------------------------------- clip, scale
@pytest.mark.parametrize("rel", (0.5, 1.0, 2.0, None, 0, np.inf), ids=("below", "equal", "above", "none", "zero", "inf"))
def test_clipping(gpu, rel):
    n = 3 * SPAN + 1
    p, grads = data(n, 31, steps=2)
    norm = float(np.sqrt((grads[0].astype(np.float64) ** 2).sum()))
    max_norm = rel * norm if rel not in (None, 0, np.inf) else rel
    rig = Rig(gpu, [n - 2, 2], p, max_norm=max_norm)
    info = rig.step(grads[0])
    assert rig.agrees(info, f"max_norm {rel} x norm")
    assert (info[1] < 1.0) == (rel in (0.5, 1.0))
    assert rig.agrees(rig.step(grads[1]), f"max_norm {rel} x norm, second step")


def test_world_of_four_reads_a_quarter_of_the_gradient(gpu):
    """grad_scale = 1 / world inside the kernel, compared with the restatement's (s c) g -- not with bit equality to dividing
    first: s g rounds differently in fp64 than an fp32 division would have."""
    n = SPAN + 77
    p, grads = data(n, 41, steps=3)
    rig = Rig(gpu, [70, n - 70], p, world=4, max_norm=0.2, weight_decay=0.02)
    assert rig.opt.grad_scale == 0.25
    for k, g in enumerate(grads, 1):
        info = rig.step(4 * g)
        assert rig.agrees(info, f"world 4 step {k}")
    quarter = R.State(p)
    infos = [R.step(quarter, g, 1e-3, max_norm=0.2, weight_decay=0.02) for g in grads]
    assert close(rig.device_state()[0], quarter.p, "against dividing first") and abs(infos[-1][0] - info[0]) <= 1e-12 * info[0]


# ----------------------------------------------------------------------------------------------- graph, repeatability
def test_step_replays_from_a_captured_graph(gpu):
    """step() captured with torch.cuda.graph on one stream, replayed three times; between replays the gradient buffer is rewritten
    in place and the rate changes through vgtk.LearningRateScheduler.  Bitwise equal to the same three steps run eagerly."""
    from epn_pointcloud_amd.vgtk.utils import LearningRateScheduler
    lengths = [5, 70001, 3]
    n = sum(lengths)
    p, grads = data(n, 51, steps=3)
    kw = dict(lr=1e-2, max_norm=1.0, weight_decay=0.01)
    eager, captured = Rig(gpu, lengths, p, **kw), Rig(gpu, lengths, p, **kw)
    s_e = LearningRateScheduler(eager.opt, 1e-2, "exp_decay", 1, decay_rate=0.5)
    s_c = LearningRateScheduler(captured.opt, 1e-2, "exp_decay", 1, decay_rate=0.5)
    for g in grads:
        eager.step(g)
        s_e.step()
    want = eager.device_state()
    graph = torch.cuda.CUDAGraph()
    captured.set_grad(grads[0])
    versions = [q._version for q in captured.params]
    with torch.cuda.graph(graph):
        captured.opt.step()
    torch.cuda.synchronize()
    assert captured.opt.counters.tolist() == [0, 0]               # a capture runs nothing
    assert all(q._version > v for q, v in zip(captured.params, versions))
    for k, g in enumerate(grads):
        captured.set_grad(g)
        graph.replay()
        s_c.step()
        torch.cuda.synchronize()
        assert captured.opt.counters.tolist() == [k + 1, 0]
    got = captured.device_state()
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got[:4], want[:4])) and got[4] == want[4] == [3, 0]
    assert got[3][2] == np.float32(1e-2 * 0.25)                   # the third step read the rate of the second scheduler call


def test_two_runs_are_bitwise_equal(gpu):
    lengths = [5, 70001]
    p, grads = data(sum(lengths), 61, steps=3)
    runs = []
    for _ in range(2):
        rig = Rig(gpu, lengths, p, max_norm=0.3)
        for g in grads:
            rig.step(g)
        runs.append(rig.device_state())
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(runs[0][:4], runs[1][:4])) and runs[0][4] == runs[1][4]


# ----------------------------------------------------------------------------------------------- torch on the device
LR = 2.0 ** -10      # the kernel reads its rate as a float32: a rate that IS one, so that torch in fp64 steps with the same number
                     # (1e-3 is not: fl32(1e-3) lies 0.8 2^-24 away, which the derived bound has no room for)


def torch_step(ps, gs, dtype, sd=None, max_norm=None, **kw):
    """One torch.optim.Adam step (after clip_grad_norm_ when max_norm is given) on copies of ps in `dtype` with gradients gs and
    the state of `sd` -> the new parameters and the optimiser."""
    qs = [torch.nn.Parameter(p.detach().to(dtype).clone()) for p in ps]
    opt = torch.optim.Adam(qs, **kw)
    if sd is not None:
        opt.load_state_dict({k: v for k, v in sd.items() if k != "steps_skipped"})
    for q, g in zip(qs, gs):
        q.grad = g.detach().to(dtype).clone()
    if max_norm is not None:
        torch.nn.utils.clip_grad_norm_(qs, max_norm)
    opt.step()
    return [q.detach() for q in qs], opt


def within_bound(old, new, ref, what):
    worst = 0.0
    for o, n_, r in zip(old, new, ref):
        scale = torch.maximum(o.detach().double().abs(), r.double().abs())
        err = (n_.detach().double() - r.double()).abs()
        if not bool((err <= P_BOUND * scale).all()):
            print(f"{what}: beyond the bound")
            return False
        worst = max(worst, float((err / scale.clamp_min(1e-300)).max()))
    print(f"{what}: largest distance {worst / P_BOUND:.3f} of the 2^-22 bound")
    return True


def test_against_torch_adam_on_the_device(gpu):
    from epn_pointcloud_amd import optim
    shapes = [(33, 7), (129,), (5, 5, 5), (1,)]
    gen = torch.Generator(device="cpu").manual_seed(5)
    start = [torch.randn(*s, generator=gen).to(gpu) for s in shapes]
    gs = [0.1 * torch.randn(*s, generator=gen).to(gpu) for s in shapes]
    kw = dict(lr=LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    ps = [s.clone().requires_grad_() for s in start]
    opt = optim.FlatAdam(ps, **kw)
    for v, g in zip(opt.grad_buckets.views, gs):
        v.copy_(g)
    opt.step()
    ref, _ = torch_step(start, gs, torch.float64, **kw)
    assert within_bound(start, ps, ref, "FlatAdam against torch fp64")
    t32, _ = torch_step(start, gs, torch.float32, **kw)
    within_bound(start, t32, ref, "torch's own fp32 step against torch fp64 (printed, not asserted)")


# ----------------------------------------------------------------------------------------------- network level
def test_network_step(gpu):
    """The tiny classification network of test_gpu_cls_loss.py: one forward and backward, the same gradients to FlatAdam and to
    torch.optim.Adam in fp64, every parameter within the bound; the version contract; a second forward; state dicts both ways."""
    from epn_pointcloud_amd import gemm, optim
    from epn_pointcloud_amd.vgtk import AttentionCrossEntropyLoss
    from test_gpu_cls_loss import _clouds, _tiny_cls
    net = _tiny_cls(gpu).train()
    params = [p for p in net.parameters() if p.requires_grad]
    kw = dict(lr=LR, weight_decay=1e-4, max_norm=10.0)
    opt = optim.FlatAdam(params, **kw)
    crit = AttentionCrossEntropyLoss("default", 0.5).to(gpu)
    pc, label, rlabel = _clouds(gpu, 4, 31)

    def backward():
        opt.zero_grad()
        logits, att = net(pc)
        crit(logits, label, att, rlabel)[0].backward()
        assert all(p.grad.data_ptr() == v.data_ptr() for p, v in zip(params, opt.grad_buckets.views))
        return [p.grad.clone() for p in params]

    gs = backward()
    assert all(torch.isfinite(g).all() for g in gs) and any(torch.count_nonzero(g) > 0 for g in gs)
    start = [p.detach().clone() for p in params]
    for p in params:
        gemm.absmax_cached(p)
    assert all(gemm.amax_tag(p) is not None for p in params)
    versions = [p._version for p in params]
    opt.step()
    assert all(gemm.amax_tag(p) is None and p._version > v for p, v in zip(params, versions))
    info = H(opt.last_info())
    assert info[3] == 0.0 and opt.counters.tolist() == [1, 0]
    print(f"network: gradient norm {info[0]:.4g}, clip factor {info[1]:.4g}")
    ref, _ = torch_step(start, gs, torch.float64, **kw)
    assert within_bound(start, params, ref, "network, step 1")
    logits, att = net(pc)
    assert torch.isfinite(logits).all() and torch.isfinite(att).all()
    # FlatAdam's state into torch: the same second step
    sd = opt.state_dict()
    gs = backward()
    start = [p.detach().clone() for p in params]
    opt.step()
    ref, _ = torch_step(start, gs, torch.float64, sd=sd, **kw)
    assert within_bound(start, params, ref, "network, step 2 from FlatAdam's state dict in torch")
    # torch's fp32 state into FlatAdam and into torch fp64: the same third step
    start = [p.detach().clone() for p in params]
    _, t32 = torch_step(start, gs, torch.float32, sd=opt.state_dict(), **kw)
    sd32 = t32.state_dict()
    opt.load_state_dict(sd32)
    assert opt.counters.tolist() == [3, 0]
    gs = backward()
    opt.step()
    ref, _ = torch_step(start, gs, torch.float64, sd=sd32, **kw)
    assert within_bound(start, params, ref, "network, step 4 from torch's state dict in FlatAdam")
    assert opt.counters.tolist() == [4, 0]
