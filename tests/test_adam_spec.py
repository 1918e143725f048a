"""The Adam step's specification on the CPU: the restatement (tests/adam_ref.py) against torch.optim.Adam in fp64, the C ABI's
binding and refusals (decided before any HIP runtime call, so they need no GPU), and what optim.FlatAdam does on the host.

Bound against torch in fp64 (also used on the device by test_gpu_adam.py).  torch.optim.Adam in fp64 rounds nothing to fp32; the
step of the specification rounds m', v' and p' once each.  m' and v' therefore agree with torch's within one fp32 ulp (half an ulp
from the rounding; one is allowed).  For p': the roundings of m' and v' put a relative error of at most 2^-24 + 2^-25 = 1.5 2^-24
on the update u = p - p' (m' enters linearly, v' through a square root), |u| <= |p| + |p'| <= 2 max(|p|, |p'|), and the final
rounding adds half an ulp of p', at most 2^-24 |p'|: together at most (3 + 1) 2^-24 max(|p|, |p'|) = 2^-22 max(|p|, |p'|)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import adam_ref as R
from conftest import ROOT

EINVAL, EWORKSPACE, ENULL = -1, -2, -3
P_BOUND = 2.0 ** -22


def torch_adam64(p, g, m, v, steps, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=None):
    """One step of torch.optim.Adam in fp64 on the CPU from the given state -> (p', m', v') as fp64 arrays."""
    q = torch.nn.Parameter(torch.from_numpy(np.asarray(p, dtype=np.float64).copy()))
    opt = torch.optim.Adam([q], lr=float(np.float32(lr)), betas=betas, eps=eps, weight_decay=weight_decay)
    opt.state[q] = {"step": torch.tensor(float(steps)), "exp_avg": torch.from_numpy(np.asarray(m, dtype=np.float64).copy()),
                    "exp_avg_sq": torch.from_numpy(np.asarray(v, dtype=np.float64).copy())}
    q.grad = torch.from_numpy(np.asarray(g, dtype=np.float64).copy())
    if max_norm is not None:
        torch.nn.utils.clip_grad_norm_([q], max_norm)
    opt.step()
    st = opt.state[q]
    return q.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


def random_state(n, seed, steps=3):
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(np.float32)
    g = (0.1 * rng.standard_normal(n)).astype(np.float32)
    m = (0.05 * rng.standard_normal(n)).astype(np.float32)
    v = (0.01 * rng.random(n)).astype(np.float32)
    return R.State(p, m, v, (steps, 0)), g


def within_bound(p_old, p_new, m_new, v_new, ref, what):
    """p' within 2^-22 max(|p|, |p'|) and m', v' within one fp32 ulp of torch's fp64 step; prints the largest ratios."""
    rp, rm, rv = ref
    scale = np.maximum(np.abs(p_old.astype(np.float64)), np.abs(rp))
    ep = np.abs(p_new.astype(np.float64) - rp) / np.where(scale > 0, scale, 1.0)
    em = np.abs(m_new.astype(np.float64) - rm) / np.spacing(np.abs(rm).astype(np.float32)).astype(np.float64)
    ev = np.abs(v_new.astype(np.float64) - rv) / np.spacing(np.abs(rv).astype(np.float32)).astype(np.float64)
    print(f"{what}: p' off by {ep.max() / P_BOUND:.3f} of the 2^-22 bound, m' by {em.max():.3f} ulp, v' by {ev.max():.3f} ulp")
    return bool((ep <= P_BOUND).all() and (em <= 1.0).all() and (ev <= 1.0).all())


# ------------------------------------------------------------------------------------------- the restatement against torch
@pytest.mark.parametrize("weight_decay", (0.0, 0.01))
@pytest.mark.parametrize("steps", (0, 3))
def test_restatement_equals_torch_adam_in_fp64(weight_decay, steps):
    st, g = random_state(4099, 11 + steps, steps)
    old = st.copy()
    info = R.step(st, g, 1e-3, weight_decay=weight_decay)
    assert info[3] == 0.0 and info[1] == 1.0 and st.counters == [steps + 1, 0]
    ref = torch_adam64(old.p, g, old.m, old.v, steps, 1e-3, weight_decay=weight_decay)
    assert within_bound(old.p, st.p, st.m, st.v, ref, f"wd {weight_decay} t {steps + 1}")


@pytest.mark.parametrize("factor", (0.5, 2.0), ids=("norm_above_max", "norm_below_max"))
def test_restatement_clips_like_clip_grad_norm(factor):
    st, g = random_state(1531, 23)
    old = st.copy()
    norm = float(np.sqrt((g.astype(np.float64) ** 2).sum()))
    info = R.step(st, g, 2e-3, max_norm=factor * norm)
    assert abs(info[0] - norm) <= 1e-12 * norm
    assert (info[1] < 1.0) == (factor < 1.0) and (factor < 1.0 or info[1] == 1.0)
    ref = torch_adam64(old.p, g, old.m, old.v, 3, 2e-3, max_norm=factor * norm)
    assert within_bound(old.p, st.p, st.m, st.v, ref, f"max_norm {factor} x norm")


def test_restatement_skips_and_counts():
    st, g = random_state(37, 5)
    old = st.copy()
    for bad in (np.nan, np.inf, -np.inf):
        h = g.copy()
        h[7] = bad
        info = R.step(st, h, 1e-3, max_norm=1.0)
        assert info[3] == 1.0 and not np.isfinite(info[0])
    assert st.counters == [3, 3]
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in ((st.p, old.p), (st.m, old.m), (st.v, old.v)))
    assert R.clip_factor(np.inf, 1.0) == 0.0 and R.clip_factor(np.nan, 1.0) == 1.0
    assert all(R.clip_factor(10.0, off) == 1.0 for off in (None, 0, 0.0, -1.0, np.inf))


# ------------------------------------------------------------------------------------------- the binding
NAMES = ("epn_adam_workspace_bytes", "epn_adam_check_plan", "epn_adam_step_f32")


def test_header_library_and_binding_agree():
    from epn_pointcloud_amd import _lib
    with open(os.path.join(ROOT, "include", "epn_so3conv.h")) as f:
        header = f.read()
    lib = _lib.get_lib()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTS and hasattr(raw, name) and callable(getattr(lib, name))
    assert re.search(r"#define\s+EPN_ADAM_SPAN\s+1024\b", header)
    from epn_pointcloud_amd import optim
    assert optim.SPAN == R.SPAN == 1024
    assert len(lib._cdll.epn_adam_step_f32.argtypes) == 19 and lib._cdll.epn_adam_workspace_bytes.restype is ctypes.c_size_t
    import epn_pointcloud_amd
    assert epn_pointcloud_amd.FlatAdam is optim.FlatAdam


# ------------------------------------------------------------------------------------------- refusals
def _plan(ptrs, offs):
    return (ctypes.c_uint64 * len(ptrs))(*ptrs), (ctypes.c_longlong * len(offs))(*offs)


def test_check_plan_refusals():
    from epn_pointcloud_amd import _lib
    f = _lib.get_lib().epn_adam_check_plan
    ok_p, ok_o = [4096, 8192, 12292], [0, 3, 4, 9]
    assert f(*_plan(ok_p, ok_o), 3, 9) == 0
    assert f(*_plan(ok_p, ok_o), 0, 9) == EINVAL                                  # nseg below 1
    assert f(*_plan(ok_p, ok_o), 65537, 9) == EINVAL                              # nseg above 65536 (decided before the tables are read)
    assert f(*_plan(ok_p, [1, 3, 4, 9]), 3, 9) == EINVAL                          # seg_off[0] != 0
    assert f(*_plan(ok_p, [0, 3, 3, 9]), 3, 9) == EINVAL                          # not strictly increasing
    assert f(*_plan(ok_p, [0, 4, 3, 9]), 3, 9) == EINVAL
    assert f(*_plan(ok_p, ok_o), 3, 10) == EINVAL                                 # seg_off[nseg] != n
    assert f(*_plan(ok_p, [0, 0, 0, 0]), 3, 0) == EINVAL                          # n below 1
    assert f(*_plan(ok_p, [0, 3, 4, 1 << 40]), 3, 1 << 40) == EINVAL              # n = 2^40
    assert f(*_plan(ok_p, [0, 3, 4, (1 << 40) - 1]), 3, (1 << 40) - 1) == 0
    assert f(*_plan([4096, 0, 12292], ok_o), 3, 9) == EINVAL                      # a zero address
    assert f(*_plan([4096, 8194, 12292], ok_o), 3, 9) == EINVAL                   # an address off the 4-byte grid
    assert f(None, _plan(ok_p, ok_o)[1], 3, 9) == ENULL and f(_plan(ok_p, ok_o)[0], None, 3, 9) == ENULL
    n = 65536
    assert f(*_plan([4096 + 4 * i for i in range(n)], list(range(n + 1))), n, n) == 0


def _step_args(**over):
    """Arguments of epn_adam_step_f32 that pass every host check (never-dereferenced addresses), with overrides by name."""
    a = dict(seg_param=4096, seg_off=8192, nseg=3, n=9, grad=4096, exp_avg=4096, exp_avg_sq=4096, lr=4096, beta1=0.9, beta2=0.999,
             eps=1e-8, weight_decay=0.0, grad_scale=1.0, max_norm=0.0, counters=4096, info=4096, workspace=4096,
             workspace_bytes=1 << 20, stream=None)
    a.update(over)
    return list(a.values())


def test_step_refusals_in_their_order():
    """Each refusal alone, then each class against the classes behind it: sizes and hyper-parameters, then pointers, then the
    workspace.  Every call here is refused on the host: nothing is launched and no pointer is followed."""
    from epn_pointcloud_amd import _lib
    lib = _lib.get_lib()
    f = lib.epn_adam_step_f32
    need = int(lib.epn_adam_workspace_bytes(9))
    nan, inf = float("nan"), float("inf")
    invalid = [dict(nseg=0), dict(nseg=65537), dict(n=0), dict(n=-1), dict(n=1 << 40), dict(nseg=10, n=9),
               dict(beta1=-0.1), dict(beta1=1.0), dict(beta1=nan), dict(beta2=-0.1), dict(beta2=1.0), dict(beta2=nan),
               dict(eps=0.0), dict(eps=-1e-8), dict(eps=nan), dict(eps=inf),
               dict(weight_decay=-1.0), dict(weight_decay=nan), dict(weight_decay=inf),
               dict(grad_scale=-1.0), dict(grad_scale=nan), dict(grad_scale=inf), dict(max_norm=nan)]
    pointers = ("seg_param", "seg_off", "grad", "exp_avg", "exp_avg_sq", "lr", "counters", "info")
    small = [dict(workspace=None), dict(workspace_bytes=need - 1), dict(workspace_bytes=0)]
    for bad in invalid:
        assert f(*_step_args(**bad)) == EINVAL, bad
        assert f(*_step_args(**bad, grad=None)) == EINVAL, bad                       # a size wins over a pointer
        assert f(*_step_args(**bad, workspace=None)) == EINVAL, bad                  # ... and over the workspace
    for name in pointers:
        assert f(*_step_args(**{name: None})) == ENULL, name
        for ws in small:
            assert f(*_step_args(**{name: None}, **ws)) == ENULL, (name, ws)          # a pointer wins over the workspace
    for ws in small:
        assert f(*_step_args(**ws)) == EWORKSPACE, ws
    assert f(*_step_args(workspace=4100)) == EWORKSPACE                               # off the 8-byte grid
    # what is NOT refused on these grounds: the edges of the ranges (they fall through to the workspace refusal used as a probe)
    for fine in (dict(beta1=0.0, beta2=0.0), dict(weight_decay=0.0, grad_scale=0.0), dict(max_norm=inf), dict(max_norm=-1.0),
                 dict(n=(1 << 40) - 1), dict(nseg=65536, n=65536), dict(nseg=1, n=1)):
        assert f(*_step_args(**fine, workspace=None)) == EWORKSPACE, fine


def test_workspace_bytes_is_positive_and_monotone():
    from epn_pointcloud_amd import _lib
    f = _lib.get_lib().epn_adam_workspace_bytes
    sizes = [1, 2, 1023, 1024, 1025, 70001, 1 << 21, (1 << 21) + 1, 7_800_000, 1 << 30, (1 << 40) - 1]
    got = [int(f(n)) for n in sizes]
    assert all(g > 0 for g in got) and all(a <= b for a, b in zip(got, got[1:])), got


# ------------------------------------------------------------------------------------------- FlatAdam on the host
def _params(shapes, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in shapes]


def test_flat_adam_builds_its_tables_on_cpu_parameters():
    from epn_pointcloud_amd import dp, optim
    ps = _params([(3, 5), (7,), (1,), (2, 2, 2)])
    opt = optim.FlatAdam(ps, lr=3e-4, weight_decay=0.01, max_norm=5.0, world=4)
    assert opt.n == 31 and opt.offsets == [0, 15, 22, 23, 31] and opt.grad_scale == 0.25
    addr, off = opt.table()
    assert addr.dtype == off.dtype == torch.int64
    assert addr.tolist() == [p.data_ptr() for p in ps] and off.tolist() == opt.offsets
    assert opt.exp_avg.shape == opt.exp_avg_sq.shape == (31,) and opt.counters.tolist() == [0, 0]
    assert opt.counters.dtype == torch.int32 and opt.last_info().shape == (4,) and opt.last_info().dtype == torch.float32
    # its own GradBuckets: the accumulate form, the gradients are views of the flat buffer at the same offsets
    gb = opt.grad_buckets
    assert isinstance(gb, dp.GradBuckets) and gb.collect == "accumulate" and not gb.hooks and gb.world == 1
    assert all(p.grad.data_ptr() == gb.flat.data_ptr() + 4 * o for p, o in zip(ps, opt.offsets))
    g = opt.param_groups[0]
    assert len(opt.param_groups) == 1 and g["lr"] == 3e-4 and g["betas"] == (0.9, 0.999) and g["eps"] == 1e-8
    assert g["weight_decay"] == 0.01 and g["params"] == [0, 1, 2, 3]
    with pytest.raises(TypeError):
        opt.step()
    with pytest.raises(NotImplementedError):
        optim.FlatAdam(ps, amsgrad=True)
    with pytest.raises(ValueError):
        optim.FlatAdam([])
    with pytest.raises(TypeError):
        optim.FlatAdam([torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))])
    with pytest.raises(ValueError):
        optim.FlatAdam([ps[0], ps[0]])
    d = optim.FlatAdam(_params([(2,)]))
    dg = d.param_groups[0]
    assert (dg["lr"], dg["betas"], dg["eps"], dg["weight_decay"]) == (1e-3, (0.9, 0.999), 1e-8, 0.0) and d.max_norm == 0.0


def test_flat_adam_refuses_grad_buckets_in_another_order():
    from epn_pointcloud_amd import dp, optim
    ps = _params([(3,), (4,), (5,)])
    gb = dp.GradBuckets([[ps[2]], [ps[0], ps[1]]], world=2, hooks=False)
    with pytest.raises(ValueError):
        optim.FlatAdam(ps, grad_buckets=gb, world=2)
    with pytest.raises(ValueError):
        optim.FlatAdam(ps[:2], grad_buckets=gb, world=2)
    opt = optim.FlatAdam(gb.params, grad_buckets=gb, world=2)
    assert opt.grad_buckets is gb and opt.grad_scale == 0.5 and opt.offsets == [0, 5, 8, 12]


def test_state_dict_interchanges_with_torch_adam():
    from epn_pointcloud_amd import optim
    shapes = [(3, 5), (7,), (2, 2)]
    ps, qs = _params(shapes, 1), _params(shapes, 1)
    ta = torch.optim.Adam(qs, lr=2e-3, betas=(0.8, 0.99), eps=1e-7, weight_decay=0.02)
    for k in range(2):
        for q in qs:
            q.grad = torch.full_like(q, 0.1 * (k + 1))
        ta.step()
    want = ta.state_dict()
    # torch -> FlatAdam
    fa = optim.FlatAdam(ps)
    fa.load_state_dict(want)
    assert fa.counters.tolist() == [2, 0]
    g = fa.param_groups[0]
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"]) == (2e-3, (0.8, 0.99), 1e-7, 0.02)
    assert float(fa.lr_tensor()[0]) == float(np.float32(2e-3))
    for i, q in enumerate(qs):
        a, b = fa.offsets[i], fa.offsets[i + 1]
        assert torch.equal(fa.exp_avg[a:b].view_as(q), ta.state[q]["exp_avg"])
        assert torch.equal(fa.exp_avg_sq[a:b].view_as(q), ta.state[q]["exp_avg_sq"])
    # FlatAdam -> torch: keys and shapes are torch's, the extra key is ignored by torch
    fa.counters[1] = 5
    got = fa.state_dict()
    assert set(got) == {"state", "param_groups", "steps_skipped"} and got["steps_skipped"] == 5
    assert set(got["param_groups"][0]) == set(want["param_groups"][0]) and got["param_groups"][0]["params"] == [0, 1, 2]
    assert set(got["state"]) == set(want["state"])
    for i in got["state"]:
        assert set(got["state"][i]) == {"step", "exp_avg", "exp_avg_sq"} == set(want["state"][i])
        assert float(got["state"][i]["step"]) == 2.0
        for k in ("exp_avg", "exp_avg_sq"):
            assert got["state"][i][k].shape == want["state"][i][k].shape and torch.equal(got["state"][i][k], want["state"][i][k])
    tb = torch.optim.Adam(_params(shapes, 1), lr=1.0)
    tb.load_state_dict(got)
    back = tb.state_dict()
    assert back["param_groups"][0]["lr"] == 2e-3 and back["param_groups"][0]["betas"] == (0.8, 0.99)
    assert all(float(back["state"][i]["step"]) == 2.0 and torch.equal(back["state"][i]["exp_avg"], want["state"][i]["exp_avg"])
               for i in back["state"])
    # and round again into a fresh FlatAdam, the skipped count with it
    fb = optim.FlatAdam(_params(shapes, 1))
    fb.load_state_dict(got)
    assert fb.counters.tolist() == [2, 5] and torch.equal(fb.exp_avg, fa.exp_avg) and torch.equal(fb.exp_avg_sq, fa.exp_avg_sq)
    # a fresh torch optimiser has no state: zeros and step 0
    fb.load_state_dict(torch.optim.Adam(_params(shapes, 1)).state_dict())
    assert fb.counters.tolist() == [0, 0] and not fb.exp_avg.any() and not fb.exp_avg_sq.any()
    with pytest.raises(ValueError):
        fb.load_state_dict(torch.optim.Adam(_params(shapes[:2], 1)).state_dict())


def test_learning_rate_scheduler_writes_the_device_scalar(capsys):
    from epn_pointcloud_amd import optim
    from epn_pointcloud_amd.vgtk.utils import LearningRateScheduler
    opt = optim.FlatAdam(_params([(4,)]), lr=1e-2)
    sched = LearningRateScheduler(opt, 1e-2, "exp_decay", 2, decay_rate=0.5)
    assert float(opt.lr_tensor()[0]) == float(np.float32(1e-2))
    seen = []
    for _ in range(4):
        sched.step()
        seen.append((opt.param_groups[0]["lr"], float(opt.lr_tensor()[0])))
    assert [s[0] for s in seen] == [1e-2, 5e-3, 5e-3, 2.5e-3]
    assert all(dev == float(np.float32(host)) for host, dev in seen)
    opt.param_groups[0].update(lr=7e-4)
    assert opt.param_groups[0]["lr"] == 7e-4 and float(opt.lr_tensor()[0]) == float(np.float32(7e-4))


def test_finish_average_false_leaves_the_sum(tmp_path):
    """A one-rank gloo group and a GradBuckets told it is one of four ranks: the all-reduce over one rank changes nothing, so the
    default finish() leaves flat / 4 and finish(average=False) leaves flat."""
    import torch.distributed as dist
    from epn_pointcloud_amd import dp
    assert not dist.is_initialized()
    dist.init_process_group("gloo", init_method="file://" + str(tmp_path / "rendezvous"), rank=0, world_size=1)
    try:
        ps = _params([(3,), (5,)])
        gb = dp.GradBuckets([ps], world=4, hooks=False)
        fill = torch.arange(1.0, 9.0)
        gb.flat.copy_(fill)
        assert gb.finish() == 1 and torch.equal(gb.flat, fill / 4)
        gb.flat.copy_(fill)
        assert gb.finish(average=False) == 1 and torch.equal(gb.flat, fill)
        gb.flat.copy_(fill)
        assert gb.finish(one_collective=True, average=False) == 1 and torch.equal(gb.flat, fill)
        gb.flat.copy_(fill)
        assert gb.finish(one_collective=True, average=True) == 1 and torch.equal(gb.flat, fill / 4)
    finally:
        dist.destroy_process_group()
