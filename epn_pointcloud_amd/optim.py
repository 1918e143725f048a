"""The optimiser of the three trainers on the device: Adam over every parameter in two launches (csrc/adam_step.hip,
epn_adam_step_f32).

The reference trains with `optim.Adam(model.parameters(), lr=init_lr)` driven by `vgtk.LearningRateScheduler`
(vgtk/vgtk/app/trainer.py:162-168).  `FlatAdam` has torch.optim.Adam's defaults and state-dict layout, and adds what a captured
step needs: the rate, the step count and the decision to skip a step with a non-finite gradient live on the device, the
gradient norm and its clipping are part of the step, and the 1/world average of `dp.GradBuckets` is folded in.

    buckets = dp.GradBuckets(dp.stage_buckets(model), world, hooks=False)
    opt = FlatAdam(buckets.params, lr=1e-3, max_norm=10.0, grad_buckets=buckets, world=world)
    sched = vgtk.LearningRateScheduler(opt, 1e-3, 'exp_decay', 20000, decay_rate=0.7)
    ...
    buckets.zero(); loss.backward(); buckets.finish(average=False); opt.step(); sched.step()
"""
import ctypes

import torch

from . import _lib, dp

SPAN = 1024          # the chunk length the C header states: the flat index space is cut into chunks of this many elements, whole chunks per workgroup


class _Group(dict):
    """A param group whose 'lr' lives on the device as well: assigning it fills the device scalar (no synchronisation); reading
    it returns the value last assigned on the host."""

    def __init__(self, owner, items):
        super().__init__(items)
        self._owner = owner

    def __setitem__(self, key, value):
        if key == "lr":
            value = float(value)
            self._owner._lr_dev.fill_(value)
        super().__setitem__(key, value)

    def update(self, *args, **kwargs):
        for k, v in dict(*args, **kwargs).items():
            self[k] = v


def _torch_group_keys(lr, betas, eps, weight_decay):
    """The keys and defaults of a torch.optim.Adam param group in the installed torch, so that state dicts interchange."""
    probe = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
    return {k: v for k, v in probe.param_groups[0].items() if k != "params"}


class FlatAdam:
    """Adam (torch.optim.Adam's rule and defaults; no amsgrad) over the float32 parameters of one device, in the order given.

    max_norm: clip the global gradient norm like torch's clip_grad_norm_ (None, 0 or inf: off).  grad_buckets: a
    dp.GradBuckets over the same parameters in the same order, whose flat buffer is the gradient (with None one is built in the
    accumulate form: `p.grad` are views of it).  world: the gradient is read as grad / world, so call
    `grad_buckets.finish(average=False)`.

    step() launches on the current stream, never synchronises and returns nothing; it can be captured with torch.cuda.graph.  A
    step whose gradient holds a non-finite element changes nothing but `counters[1]` and `last_info()`.  `counters` is the device
    int32 pair (steps_applied, steps_skipped); `last_info()` the device float32 quadruple (gradient norm, clip factor, rate as
    read, skipped)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=None, grad_buckets=None,
                 world=1, amsgrad=False):
        if amsgrad:
            raise NotImplementedError("FlatAdam has no amsgrad form")
        params = list(params)
        if not params:
            raise ValueError("no parameters")
        for i, p in enumerate(params):
            if not isinstance(p, torch.Tensor):
                raise TypeError(f"parameter {i} must be a torch tensor, got {type(p).__name__}")
            if p.dtype != torch.float32:
                raise TypeError(f"parameter {i} must be float32, got {p.dtype}")
            if not p.is_contiguous() or p.numel() == 0:
                raise ValueError(f"parameter {i} must be contiguous and non-empty, got shape {tuple(p.shape)}, stride {p.stride()}")
            if not p.requires_grad:
                raise ValueError(f"parameter {i} does not require a gradient: pass the trainable parameters")
        if len({id(p) for p in params}) != len(params):
            raise ValueError("a parameter is given twice")
        _lib.same_device(*params)
        lr, eps, weight_decay, world = float(lr), float(eps), float(weight_decay), int(world)
        betas = (float(betas[0]), float(betas[1]))
        if not lr >= 0.0:
            raise ValueError(f"invalid learning rate {lr}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"betas must lie in [0, 1), got {betas}")
        if not 0.0 < eps < float("inf"):
            raise ValueError(f"eps must be positive and finite, got {eps}")
        if not 0.0 <= weight_decay < float("inf"):
            raise ValueError(f"weight_decay must be finite and >= 0, got {weight_decay}")
        if world < 1:
            raise ValueError(f"world must be >= 1, got {world}")
        self.max_norm = 0.0 if max_norm is None else float(max_norm)
        if self.max_norm != self.max_norm:
            raise ValueError("max_norm is NaN")
        self.params, self.world, self.grad_scale = params, world, 1.0 / world
        self._own_buckets = grad_buckets is None
        if grad_buckets is None:
            grad_buckets = dp.GradBuckets([params], world=1, hooks=False)
        elif len(grad_buckets.params) != len(params) or any(a is not b for a, b in zip(grad_buckets.params, params)):
            raise ValueError("grad_buckets holds other parameters, or the same in another order: its flat buffer is read with "
                             "this optimiser's offsets (pass grad_buckets.params)")
        self.grad_buckets = grad_buckets
        dev = params[0].device
        self.n = sum(p.numel() for p in params)
        self.exp_avg = torch.zeros(self.n, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(self.n, dtype=torch.float32, device=dev)
        self._lr_dev = torch.full((1,), lr, dtype=torch.float32, device=dev)
        self.counters = torch.zeros(2, dtype=torch.int32, device=dev)
        self._info = torch.zeros(4, dtype=torch.float32, device=dev)
        offs = [0]
        for p in params:
            offs.append(offs[-1] + p.numel())
        self.offsets = offs
        self._seg_off = torch.tensor(offs, dtype=torch.int64, device=dev)
        self._seg_param = torch.zeros(len(params), dtype=torch.int64, device=dev)      # addresses; the kernel reads them as u64
        self._ptrs = None
        self._write_table()
        self._workspace = torch.zeros(int(_lib.get_lib().epn_adam_workspace_bytes(self.n)), dtype=torch.uint8, device=dev)
        self.param_groups = [_Group(self, dict(_torch_group_keys(lr, betas, eps, weight_decay), params=list(range(len(params)))))]

    # the tables -----------------------------------------------------------------------------------------------------------
    def _write_table(self):
        """Validate (epn_adam_check_plan, on host copies) and upload the parameters' addresses."""
        ptrs = [p.data_ptr() for p in self.params]
        nseg = len(ptrs)
        host_p = (ctypes.c_uint64 * nseg)(*ptrs)
        host_o = (ctypes.c_longlong * (nseg + 1))(*self.offsets)
        rc = _lib.get_lib().epn_adam_check_plan(host_p, host_o, nseg, self.n)
        if rc != 0:
            raise ValueError(f"the parameters do not make a valid plan (code {rc}): 1..65536 parameters, fewer than 2^40 elements, "
                             "every address 4-byte aligned")
        self._seg_param.copy_(torch.tensor(ptrs, dtype=torch.int64))
        self._ptrs = ptrs

    def table(self):
        """(addresses, offsets) as the kernel reads them: two int64 tensors on the parameters' device."""
        return self._seg_param, self._seg_off

    # the step -------------------------------------------------------------------------------------------------------------
    def zero_grad(self, set_to_none=False):
        """Start of a step: the flat gradient buffer is zeroed (the gradients stay views of it)."""
        self.grad_buckets.zero()

    def _eager_checks(self):
        """What a replayed graph cannot do and an eager step can: follow a parameter that was re-allocated, and bring a
        gradient that autograd put elsewhere into the flat buffer this optimiser built itself."""
        if any(p.data_ptr() != q for p, q in zip(self.params, self._ptrs)):
            self._write_table()
        if self._own_buckets:
            for p, v in zip(self.params, self.grad_buckets.views):
                g = p.grad
                if g is None:
                    v.zero_()
                elif g.data_ptr() != v.data_ptr():
                    v.copy_(g)
                p.grad = v

    def step(self):
        if not self.params[0].is_cuda:
            raise TypeError("FlatAdam.step() runs on the device: the parameters are on the CPU (there is no host form)")
        if not torch.cuda.is_current_stream_capturing():
            self._eager_checks()
        g = self.param_groups[0]
        lib = _lib.get_lib()
        ws = self._workspace
        rc = lib.epn_adam_step_f32(_lib.dev_ptr(self._seg_param, "seg_param", torch.int64),
                                   _lib.dev_ptr(self._seg_off, "seg_off", torch.int64), len(self.params), self.n,
                                   _lib.dev_ptr(self.grad_buckets.flat, "grad"), _lib.dev_ptr(self.exp_avg, "exp_avg"),
                                   _lib.dev_ptr(self.exp_avg_sq, "exp_avg_sq"), _lib.dev_ptr(self._lr_dev, "lr"),
                                   g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], self.grad_scale, self.max_norm,
                                   _lib.dev_ptr(self.counters, "counters", torch.int32), _lib.dev_ptr(self._info, "info"),
                                   _lib.dev_ptr(ws, "workspace", torch.uint8), ws.numel(), _lib.stream_of(self.exp_avg))
        _lib.check(rc, "epn_adam_step_f32")
        from . import gemm
        for p in self.params:
            gemm.mark_written(p)            # raw-pointer writes: bump the version, drop every cached maximum

    def last_info(self):
        """Device float32 [4] of the last step: (gradient norm, clip factor, rate as read, 1 if the step was skipped)."""
        return self._info

    def lr_tensor(self):
        """The device scalar the kernel reads its rate from (written by `param_groups[0]['lr'] = ...`)."""
        return self._lr_dev

    # state ----------------------------------------------------------------------------------------------------------------
    def state_dict(self):
        """torch.optim.Adam's layout: state[i] = {step, exp_avg, exp_avg_sq}, param_groups with torch's keys; `steps_skipped` as
        an extra top-level key.  Reads the counters: synchronises."""
        applied, skipped = (int(x) for x in self.counters.tolist())
        state = {}
        for i, p in enumerate(self.params):
            a, b = self.offsets[i], self.offsets[i + 1]
            state[i] = {"step": torch.tensor(float(applied)), "exp_avg": self.exp_avg[a:b].view_as(p).clone(),
                        "exp_avg_sq": self.exp_avg_sq[a:b].view_as(p).clone()}
        return {"state": state, "param_groups": [dict(self.param_groups[0])], "steps_skipped": skipped}

    def load_state_dict(self, sd):
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self.params):
            raise ValueError(f"the state dict holds {len(groups)} groups of {[len(g['params']) for g in groups]} parameters; "
                             f"this optimiser has one group of {len(self.params)}")
        grp = groups[0]
        if grp.get("amsgrad") or grp.get("maximize"):
            raise NotImplementedError("FlatAdam has no amsgrad or maximize form")
        state = sd["state"]
        steps = set()
        for i, (pid, p) in enumerate(zip(grp["params"], self.params)):
            st = state.get(pid)
            a, b = self.offsets[i], self.offsets[i + 1]
            if st is None:                                 # torch keeps no state for a parameter that never had a gradient
                self.exp_avg[a:b].zero_()
                self.exp_avg_sq[a:b].zero_()
                continue
            if tuple(st["exp_avg"].shape) != tuple(p.shape) or tuple(st["exp_avg_sq"].shape) != tuple(p.shape):
                raise ValueError(f"state of parameter {i} has shape {tuple(st['exp_avg'].shape)}, the parameter {tuple(p.shape)}")
            self.exp_avg[a:b].view_as(p).copy_(st["exp_avg"])
            self.exp_avg_sq[a:b].view_as(p).copy_(st["exp_avg_sq"])
            steps.add(int(float(st["step"])))
        if len(steps) > 1:
            raise ValueError(f"the parameters' step counts differ ({sorted(steps)}): one flat update has one count")
        self.counters.copy_(torch.tensor([steps.pop() if steps else 0, int(sd.get("steps_skipped", 0))], dtype=torch.int32))
        g = self.param_groups[0]
        g["betas"] = (float(grp["betas"][0]), float(grp["betas"][1]))
        g["eps"], g["weight_decay"] = float(grp["eps"]), float(grp["weight_decay"])
        g["lr"] = float(grp["lr"])
