#!/usr/bin/env python3
"""Which form did every layer take?  One eager step (forward, backward, optimiser; or the forward alone) of each configuration
below under ops.profile_begin() / profile_end(), written as one text file per configuration: a line `kind key flops kernel` per
recorded launch, in launch order.  Two trees that select the same forms, launch the same kernels in the same order and
report the same flop counts produce identical files:

    python tools/launch_trace.py --out A        # in one tree
    python tools/launch_trace.py --out B        # in the other
    diff -r A B

The configurations cover every selection rule of ops.select_inter_fwd / select_inter_bwd_data / select_intra that a
switch can move.  Each one runs in a fresh child process (EPN_GEMM_FP32 and EPN_AB are read at import); --jobs children
run side by side, and nothing more is started once a child has failed."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (model, dtype, forward_only, environment[, {"dropout_rate": rate} | {"eval": True}])
CONFIGS = {}
for _m in ("f16x2", "split", "native"):
    CONFIGS[f"cls_f32_gemm_{_m}"] = ("cls", "f32", False, {"EPN_GEMM_FP32": _m})
CONFIGS["reg_bf16"] = ("reg", "bf16", False, {})
CONFIGS["inv_bf16"] = ("inv", "bf16", False, {})
CONFIGS["reg_f32"] = ("reg", "f32", False, {})                     # K = 64 layers: the atomic scatter
CONFIGS["cls_f32_deterministic"] = ("cls", "f32", False, {"EPN_DETERMINISTIC": "1"})
for _m in ("fused", "split", "onchip"):
    CONFIGS[f"cls_f32_inter_{_m}"] = ("cls", "f32", False, {"EPN_INTER_MODE": _m})
for _m in ("cloud", "split", "onchip", "fused"):
    CONFIGS[f"cls_f32_bwd_{_m}"] = ("cls", "f32", False, {"EPN_INTER_BWD_DATA": _m})
    CONFIGS[f"reg_bf16_bwd_{_m}"] = ("reg", "bf16", False, {"EPN_INTER_BWD_DATA": _m})
CONFIGS["cls_f32_no_shared_grad"] = ("cls", "f32", False, {"EPN_AB": "1", "EPN_SHARE_INPUT_GRAD": "0"})
CONFIGS["cls_f32_forward"] = ("cls", "f32", True, {})
CONFIGS["reg_bf16_forward"] = ("reg", "bf16", True, {})
CONFIGS["cls_f32_dropout"] = ("cls", "f32", False, {}, {"dropout_rate": 0.2})
CONFIGS["cls_f32_eval"] = ("cls", "f32", True, {}, {"eval": True})              # eval() under no_grad: the forward-only glue
CONFIGS["reg_bf16_eval"] = ("reg", "bf16", True, {}, {"eval": True})


def run_one(name, out, batch):
    import torch
    sys.path.insert(0, ROOT)
    from epn_pointcloud_amd import models as M, ops, schedule as S
    model_name, dtype, forward_only, _env, *extra = CONFIGS[name]
    extra = extra[0] if extra else {}
    drop = extra.get("dropout_rate", 0.0)
    dev = torch.device("cuda", 0)
    points = 2048 if model_name == "inv" else 1024
    batch = batch or (32 if model_name == "cls" else 64)
    layers = {"cls": S.cls_so3net_schedule, "reg": S.reg_so3net_schedule, "inv": S.inv_so3net_schedule}[model_name](points)
    torch.manual_seed(2913)
    if model_name == "cls":
        model = M.ClsSO3ConvModel(layers, out_mlps=(256,), pooling="attention", dropout_rate=drop)
    elif model_name == "reg":
        model = M.RegSO3ConvModel(layers, dropout_rate=drop)
    else:
        model = M.InvSO3ConvModel(layers, dropout_rate=drop)
    model = S.set_feature_dtype(model.to(dev).train(not extra.get("eval")), torch.float32 if dtype == "f32" else torch.bfloat16)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    pts = S.synthetic_clouds(batch, points, dev, seed=2913, scale=0.4 if model_name == "inv" else 1.0)
    labels = torch.arange(batch, device=dev) % 40
    if model_name == "reg":
        pts = pts.view(batch // 2, 2, points, 3)

    def step():
        out_ = model(pts)
        if model_name == "cls":
            loss = torch.nn.functional.cross_entropy(out_[0], labels)
        elif model_name == "inv":
            loss = (out_[0] @ out_[0].t()).square().mean()
        else:
            loss = out_[0].square().mean() + out_[1].square().mean()
        if not forward_only:
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()

    with torch.set_grad_enabled(not forward_only):
        step()                                   # first step: tables, caches, the one-off calibration
        torch.cuda.synchronize()
        ops.profile_begin()
        step()
        rec = ops.profile_end()
    torch.cuda.synchronize()
    with open(os.path.join(out, name + ".txt"), "w") as fh:
        for kind, key, flops, _e0, _e1, kernel in rec:
            fh.write(f"{kind} {key} {flops!r} {kernel}\n")
    print(f"{name}: {len(rec)} records", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", required=True, help="directory of the trace files")
    ap.add_argument("--batch", type=int, default=0, help="clouds per step (default: 32 for cls, 64 for reg / inv)")
    ap.add_argument("--jobs", type=int, default=4, help="child processes side by side")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per configuration")
    ap.add_argument("--only", default="", help="run this one configuration in this process")
    ap.add_argument("names", nargs="*", help="configurations (default: all)")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.only:
        return run_one(a.only, a.out, a.batch)
    todo = list(a.names or CONFIGS)
    switches = {k for cfg in CONFIGS.values() for k in cfg[3]}
    running, failed = [], []
    while (todo and not failed) or running:
        while todo and not failed and len(running) < a.jobs:
            name = todo.pop(0)
            env = {k: v for k, v in os.environ.items() if k not in switches}      # a configuration sets all it differs by
            env.update(CONFIGS[name][3])
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--out", a.out,
                   "--batch", str(a.batch), "--only", name]
            running.append((name, subprocess.Popen(cmd, env=env)))
        name, proc = running.pop(0)
        if proc.wait() != 0:
            failed.append((name, proc.returncode))
    if failed:
        sys.exit(f"failed (nothing further was started): {failed}; not run: {todo}")


if __name__ == "__main__":
    main()
