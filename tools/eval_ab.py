#!/usr/bin/env python3
"""What an eval() forward costs, and what the frozen-statistics kernels cost next to their training twins.

  (a) model.eval() under no_grad with EPN_FUSED_EVAL=0: every block's glue on the stock torch modules (the earlier behaviour)
  (b) model.eval() under no_grad, the default: the glue on the forward-only HIP passes (frozen BatchNorm statistics)
  (c) model.train() under no_grad: the train-mode forward (the arithmetic of bench.py's configs.cls_fwd), for scale

for the classification network (fp32, B = 32, N = 1024) and the rotation network (bf16 features, 64 clouds): ONE fresh process
per variant, started one after the other (this parent never opens the GPU), 5 warm-up and 20 timed eager forwards each, median
and minimum.  Then, in one more process, the frozen kernel instances next to their twins on one block-sized tensor (per-launch
times from HIP events around each library call, ops.profile_begin).  `python tools/eval_ab.py [cls|reg|kernels ...]`.
The claim to check: (b) < (a), and (b) <= (c) within the +-2 % spread between boxes -- (b) reduces no statistics for its BatchNorm
sides and saves nothing for a backward.  Every forward runs under a time limit: one that hangs ends its process with a traceback."""
import faulthandler
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_LIMIT_S, WARMUP, STEPS = 60, 5, 20
VARIANTS = (("a", "eval(), stock modules (EPN_FUSED_EVAL=0)"), ("b", "eval(), HIP glue (default)"), ("c", "train-mode forward"))


def limited(fn):
    import torch
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    try:
        out = fn()
        torch.cuda.synchronize()
        return out
    finally:
        faulthandler.cancel_dump_traceback_later()


def child_model(name, variant):
    os.environ["EPN_AB"] = "1"
    os.environ["EPN_FUSED_EVAL"] = "0" if variant == "a" else "1"
    import torch
    sys.path.insert(0, ROOT)
    from epn_pointcloud_amd import models as M, schedule as S
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    if name == "cls":
        model = M.build_cls(1024).to(dev)
        pts = S.synthetic_clouds(32, 1024, dev)
        clouds = 32
    else:
        model = S.set_feature_dtype(M.build_reg(1024).to(dev), torch.bfloat16)
        pts = S.synthetic_clouds(64, 1024, dev).view(32, 2, 1024, 3)
        clouds = 64
    model = model.train() if variant == "c" else model.eval()

    def fwd():
        with torch.no_grad():
            return model(pts)

    for _ in range(WARMUP):
        limited(fwd)
    times = []
    for _ in range(STEPS):
        t0 = time.perf_counter()
        limited(fwd)
        times.append((time.perf_counter() - t0) * 1e3)
    med, best = statistics.median(times), min(times)
    print(f"RESULT {name} {variant} {med:.3f} {best:.3f} {clouds / med * 1e3:.1f}", flush=True)


def child_kernels():
    """norm_act_fwd / norm_act2_fwd / the norm-on-load basis change on [32, 64, 512, 60] (the classification network's first
    stage), BatchNorm2d with affine parameters: the training instance (statistics reduced first; only the apply kernel is
    compared) next to the frozen one."""
    os.environ["EPN_AB"] = "1"
    import torch
    sys.path.insert(0, ROOT)
    from epn_pointcloud_amd import ops
    from epn_pointcloud_amd.vgtk import so3conv as sptk
    dev = torch.device("cuda", 0)
    intra = sptk.IntraSO3Conv(64, 64).to(dev)
    for dt in (torch.float32, torch.bfloat16):
        x = torch.randn(32, 64, 512, 60, device=dev).to(dt).contiguous(memory_format=torch.channels_last)
        r = torch.randn_like(x)
        bn = torch.nn.BatchNorm2d(64).to(dev)
        inorm = torch.nn.InstanceNorm2d(64).to(dev)
        per = {}
        for frozen in (False, True):
            def once():
                with torch.no_grad():
                    if frozen:
                        ops.norm_act_eval(x, bn, residual=r)
                        ops.norm_act_pair_eval(x, inorm, r, bn)
                        ops.intra_so3conv(x, intra.basic_conv.W, intra._idx32(), pre_norm=bn, pre_eval=True)
                    else:
                        ops.norm_act(x, bn, residual=r)
                        ops.norm_act_pair(x, inorm, r, bn)
                        ops.intra_so3conv(x, intra.basic_conv.W, intra._idx32(), pre_norm=bn)
            bn.train(not frozen)
            for _ in range(3):
                limited(once)
            ops.profile_begin()
            try:
                for _ in range(10):
                    limited(once)
            finally:
                rec = ops.profile_end()
            for kind, _key, _flops, e0, e1, kernel in rec:
                if "norm_act" in kernel or "so3_basis" in kernel:
                    per.setdefault((frozen, kernel), []).append(e0.elapsed_time(e1) * 1e3)
        gb = x.numel() * x.element_size() / 1e9
        for (frozen, kernel), v in sorted(per.items(), key=lambda kv: (kv[0][1], kv[0][0])):
            print(f"{str(dt)[6:]:9s} {'eval ' if frozen else 'train'} {kernel:60s} median {statistics.median(v):8.1f} us  "
                  f"({len(v)} launches; tensor {gb:.3f} GB)", flush=True)


def run_child(*args):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", *args], capture_output=True, text=True,
                         timeout=STEP_LIMIT_S * (WARMUP + STEPS))
    if out.returncode != 0:
        sys.stderr.write(out.stdout + out.stderr)
        raise SystemExit(f"child {' '.join(args)} ended with status {out.returncode}: nothing more is started")
    return out.stdout


def models(name):
    base = {}
    for variant, label in VARIANTS:
        line = [l for l in run_child(name, variant).splitlines() if l.startswith("RESULT")][-1].split()
        med, best, rate = float(line[3]), float(line[4]), float(line[5])
        base[variant] = med
        print(f"{name}  {variant}  {label:42s} median {med:8.2f} ms  min {best:8.2f}  {rate:8.1f} clouds/s  "
              f"({med / base['a']:5.3f} x a)", flush=True)
    print(f"{name}  b / a = {base['b'] / base['a']:.3f}   b / c = {base['b'] / base['c']:.3f}", flush=True)


if __name__ == "__main__":
    if sys.argv[1:2] == ["--child"]:
        child_kernels() if sys.argv[2] == "kernels" else child_model(sys.argv[2], sys.argv[3])
    else:
        for w in sys.argv[1:] or ["kernels", "cls", "reg"]:
            print(run_child("kernels"), end="", flush=True) if w == "kernels" else models(w)
