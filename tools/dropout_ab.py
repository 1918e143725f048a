#!/usr/bin/env python3
"""What dropout costs a training step, and what the generator costs the norm passes.  One process, eager steps:

  (a) dropout_rate = 0
  (b) dropout_rate = 0.2 on the stock modules (EPN_FUSED_DROPOUT=0: every block with dropout leaves the HIP glue)
  (c) dropout_rate = 0.2 with the masks drawn inside the HIP norm passes (the default)

for the classification network (fp32, B = 32, N = 1024) and the rotation network (bf16 features, B = 64 clouds), 5 warm-up and
20 timed steps each; then the six dropout kernel instances next to their plain twins on one block-sized tensor (per-launch
times from HIP events around each library call, ops.profile_begin).  `python tools/dropout_ab.py [cls|reg|kernels ...]`.
Every step runs under a time limit: a step that hangs ends the process with a traceback."""
import faulthandler
import os
import statistics
import sys
import time

os.environ["EPN_AB"] = "1"            # A/B mode: EPN_FUSED_DROPOUT is read on every block call

import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epn_pointcloud_amd import models as M, ops, schedule as S  # noqa: E402

STEP_LIMIT_S, WARMUP, STEPS, RATE = 60, 5, 20, 0.2
dev = torch.device("cuda", 0)


def limited(fn):
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        faulthandler.cancel_dump_traceback_later()


def time_model(name, rate, fused):
    os.environ["EPN_FUSED_DROPOUT"] = "1" if fused else "0"
    torch.manual_seed(0)
    ops.seed_dropout(0, dev)
    if name == "cls":
        model = M.build_cls(1024, dropout_rate=rate).to(dev).train()
        pts = S.synthetic_clouds(32, 1024, dev)
        labels = torch.arange(32, device=dev) % 40
        loss = lambda: torch.nn.functional.cross_entropy(model(pts)[0], labels)
    else:
        model = S.set_feature_dtype(M.build_reg(1024, dropout_rate=rate).to(dev).train(), torch.bfloat16)
        pts = S.synthetic_clouds(64, 1024, dev).view(32, 2, 1024, 3)

        def loss():
            conf, rot = model(pts)
            return conf.square().mean() + rot.square().mean()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)

    def step():
        opt.zero_grad(set_to_none=True)
        loss().backward()
        opt.step()

    for _ in range(WARMUP):
        limited(step)
    times = []
    for _ in range(STEPS):
        t0 = time.perf_counter()
        limited(step)
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times)


def models(name):
    rows = [("a  dropout 0", 0.0, True), ("b  dropout 0.2, stock modules", RATE, False), ("c  dropout 0.2, HIP norm passes", RATE, True)]
    base = None
    for label, rate, fused in rows:
        med, best = time_model(name, rate, fused)
        base = med if base is None else base
        print(f"{name}  {label:34s} median {med:8.2f} ms/step  min {best:8.2f}  ({med / base:5.3f} x a)", flush=True)
    os.environ["EPN_FUSED_DROPOUT"] = "1"


def kernels():
    """Per-launch time of norm_act_{fwd,bwd_reduce,bwd_apply}_kernel<T> and of their dropout forms on [32, 64, 512, 60] (the
    classification network's first stage), BatchNorm2d with affine parameters, a residual in the forward."""
    for dt in (torch.float32, torch.bfloat16):
        x = torch.randn(32, 64, 512, 60, device=dev).to(dt).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        r = torch.randn_like(x)
        gy = torch.randn_like(x)
        norm = torch.nn.BatchNorm2d(64).to(dev).train()
        per = {}
        for rate in (0.0, RATE):
            def once():
                y = ops.norm_act(x, norm, residual=r, dropout=rate)
                torch.autograd.grad(y, [x] + list(norm.parameters()), gy)
            for _ in range(3):
                limited(once)
            ops.profile_begin()
            try:
                for _ in range(10):
                    limited(once)
            finally:
                rec = ops.profile_end()
            for kind, _key, _flops, e0, e1, kernel in rec:
                if "norm_act" in kernel:
                    per.setdefault(kernel, []).append(e0.elapsed_time(e1) * 1e3)
        gb = x.numel() * x.element_size() / 1e9
        for base in ("fwd", "bwd_reduce", "bwd_apply"):
            plain = [v for k, v in per.items() if f"norm_act_{base}_kernel" in k]
            drop = [v for k, v in per.items() if f"norm_act_dropout_{base}_kernel" in k]
            if not plain or not drop:
                print(f"{dt} {base}: kernels seen: {sorted(per)}")
                continue
            p, d = statistics.median(plain[0]), statistics.median(drop[0])
            print(f"{str(dt)[6:]:9s} norm_act_{base:11s} plain {p:8.1f} us   dropout {d:8.1f} us   ({d / p:5.3f} x; tensor {gb:.3f} GB)",
                  flush=True)


if __name__ == "__main__":
    what = sys.argv[1:] or ["kernels", "cls", "reg"]
    for w in what:
        kernels() if w == "kernels" else models(w)
