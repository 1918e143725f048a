"""bench.py's reporting half without a GPU: the one stdout line stays under the driver's capture window (< 3000 bytes: round
3's 35 KB line was cut and could not be parsed), kernels are priced against the roof that bounds them (HBM for GEMMs that stream
the grouped features, the bf16 matrix pipe -- with 6x the algorithmic flops -- for the split fp32 kernels), and the short kernel
names decode the mangled template instances rocprofv3 prints for __bf16 kernels."""
import json
import os
import sys

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _key(b=64, p1=512, p2=512, nn=32, na=60, ks=24, cin=64, cout=64):
    return (b, p1, p2, nn, na, ks, cin, cout)


def canned_records(dtype):
    """A step's worth of records as ops.profile_end() returns them, with float milliseconds in place of event pairs."""
    bf = dtype == "bf16"
    k = _key() if bf else _key(b=32, p1=128, p2=128, cin=256, cout=256)      # fp32: the 256-channel layers (MFMA-bound)
    cols = k[0] * k[2] * k[4]
    fl_gemm = 2.0 * cols * k[7] * k[6] * k[5]
    nt = ("_ZN3epn12_GLOBAL__N_114gemm_nt_kernelIDF16bDF16bLi4ELi2ELi2ELi4ELi8ELi2EEEvNS_11GemmNtBatchE" if bf
          else "epn::gemm_nt_x3_kernel<4, 2, 2, 4, 2>")
    tn = "epn::gemm_tn_bf16_kernel<2, 2, 4, 8>" if bf else "epn::gemm_tn_x3_kernel<2, 4, 4, 2, 16>"
    grp = ("_ZN3epn12_GLOBAL__N_123inter_group_wide_kernelILi2ELi2EDF16bLi4EEEvNS0_9InterArgsE" if bf
           else "_ZN3epn12_GLOBAL__N_123inter_group_wide_kernelILi1ELi2EfLi4EEEvNS0_9InterArgsE")
    ung = "_ZN3epn12_GLOBAL__N_127inter_ungroup_shared_kernelILi4ELi2EDF16bLi8ELi1ELb0ELi2ELi1EEEvNS0_9InterArgsEPKiPh"
    recs = []
    for _ in range(7):
        recs += [("inter_group", k, 2.0 * cols * k[6] * k[5] * k[3], 1.0, None, grp),
                 ("inter_gemm", k, fl_gemm, 0.6 if bf else 1.2, None, nt),
                 ("inter_gemm_dw", k, fl_gemm, 1.3, None, tn),
                 ("inter_gemm_dg", k, fl_gemm, 0.6 if bf else 1.2, None, nt),
                 ("inter_ungroup", k, 0.0, 1.2, None, ung),
                 ("so3_basis", ("so3_basis", k[0] * k[2], 64), 2.0 * k[0] * k[2] * 3600 * 64, 0.09, None,
                  "epn::so3_basis_bf16_kernel"),
                 ("norm_act_fwd", (), 0.0, 0.05, None, "_ZN3epn12_GLOBAL__N_120norm_act2_fwd_kernelIDF16bEEvNS0_9NormArgs2E"),
                 ("fps", (), 0.0, 0.27, None, "fps_wave_kernel<4, 4>")]
    return recs


def full_output():
    r32, d32 = bench.roofline_of(canned_records("f32"), 1, "f32", None, True)
    r16, d16 = bench.roofline_of(canned_records("bf16"), 1, "bf16", None, True)
    wl = ("ModelNet40 cls (cls_so3net_pn: 7 separable SO3 blocks + ClsOutBlockPointnet), B=32/GPU N=1024 K=32/16 A=60 fp32 "
          "(contractions: lossless 3xbf16 split, fp32 accumulate), fwd+bwd+Adam")
    cfg = {"workload": wl, "global_batch": 32, "launch": "hipgraph", "hbm_peak_gb": 35.2,
           "fp32_gemm": "split", "parallelism": "dp1"}
    base = {"metric": "point-clouds/sec fwd+bwd, ModelNet40 N=1024 A=60", "value": 396.923, "unit": "point-clouds/s",
            "n_gpus": 1, "steps": 20, "warmup": 5, "ms_per_step": 80.621, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic", "config": cfg, "roofline": r32}
    out = dict(base, f16x2_overflow=0)
    out["native_fp32_mfma"] = {"value": 314.439, "unit": "point-clouds/s", "ms_per_step": 101.769, "steps": 20, "note": "x" * 200}
    out["index_kernels"] = {"fps": {"n": 1024, "m": 512, "us_per_launch": 269.8, "us_per_cloud": 8.43, "GB/s": 1.7, "bound": "l"},
                            "ball_query": {"queries": 512, "support": 1024, "K": 32, "us_per_launch": 16.3, "us_per_cloud": 0.51,
                                           "GB/s": 164.4}}
    step = {"algorithmic_tflops": 163.1, "frac_fp32_matrix": 1.037, "frac_bf16_pipe_x6": 0.391, "algorithmic_gb": 19.3,
            "hbm_gb": 250.3, "hbm_over_algorithmic": 13.0}
    out["roofline"] = dict(r32, step=step)
    other = {"dominant_mfma_kernel": {"kernel": "gemm_tn_f32_kernel<2,2,1,1,32,true>", "achieved": 116.0, "unit": "TFLOP/s",
                                      "frac": 0.0465, "traffic": None, "avg_launch_ms": 0.1}}
    out["configs"] = {n: dict(base, dtype="bf16", roofline=dict(r16, traffic=1652000000, step=step, **other), vs_cpu_forward=1819.3)
                      for n in ("cls_fwd", "reg_bf16", "inv_bf16")}
    out["configs"]["cls_fwd"]["roofline"] = dict(r16, step={"algorithmic_tflops": 157.0}, **other)     # forward: no PMC pass
    out["configs"]["cls_dp_rank"] = dict(base, roofline=dict(r32, step=step), overhead_ms=0.412, vs_headline=0.9947,
                                         collect="pack+1 all-reduce", predicted_eff_8gpu=0.9876, allreduce_ms=0.061,
                                         no_comm_ms=80.2, wire="ASSUMED 100 GB/s busbw",
                                         dp={"ms_per_step_local": 80.6, "allreduce_ms": 0.061, "allreduce_mb": 29.9,
                                             "allreduce_per_step": 1, "bus_gbps": None, "no_comm_ms_per_step_local": 80.2,
                                             "eff_vs_rank_program": 0.995},
                                         assumes="t1/(t_rank+wire); wire 0.60 ms = 31.3 MB ring all-reduce, 8 GPUs, 100 GB/s busbw "
                                                 "+ 0.05 ms (ASSUMED, unmeasured), no overlap")
    out["cpu_baseline"] = {"value": 0.3734, "unit": "point-clouds/s", "cores": 16, "kind": "port", "samples": 2,
                           "forward_only_value": 0.6078, "all_samples_s": [10.7, 10.9],
                           "sweep": {"one_cloud_forward_s_by_threads": {"16": 1.52, "64": 2.31, "256": 7.9}},
                           "sample": "4 clouds fwd+bwd x2, median 10.7 s (fwd 6.6); oracle/backbone_ref.py; threads = best of sweep_s; "
                                     "256/256 host CPUs usable"}
    return out, {"headline": d32, "configs": {"reg_bf16": d16}}


def test_one_line_report_fits_the_driver_window():
    out, detail = full_output()
    line = bench.compact_line(out)
    text = json.dumps(line)
    assert len(text) < bench.LINE_LIMIT <= 3000, len(text)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "configs", "detail"):
        assert k in line, k
    assert set(line["roofline"]) <= {"bound", "kernel", "achieved", "peak", "unit", "frac", "algorithmic_fp32_tflops",
                                     "vs_fp32_mfma_peak", "traffic", "launches", "avg_launch_ms",
                                     "algorithmic_bytes_per_launch", "dominant_memory_bound_kernel", "dominant_mfma_kernel",
                                     "step"}
    # what the STEP achieves is readable off the line (review item 5): TF/s, both fractions, GB per step and its ratio
    assert set(line["roofline"]["step"]) >= {"algorithmic_tflops", "frac_fp32_matrix", "frac_bf16_pipe_x6", "hbm_gb",
                                             "hbm_over_algorithmic"}
    dpr = line["configs"]["cls_dp_rank"]
    assert dpr["overhead_ms"] == 0.412 and dpr["predicted_eff_8gpu"] == 0.9876 and "ASSUMED" in dpr["wire"]
    assert dpr["allreduce_ms"] == 0.061 and dpr["no_comm_ms"] == 80.2 and "assumes" not in dpr     # (long form: detail file)
    assert line["f16x2_overflow"] == 0
    assert line["configs"]["reg_bf16"]["traffic"] == 1652000000
    assert line["cpu_baseline"]["samples"] == 2 and "all_samples_s" not in line["cpu_baseline"]
    assert all("other_roof" in c for n, c in line["configs"].items() if n != "cls_dp_rank")      # nothing had to be trimmed
    assert all(set(c) <= {"value", "ms_per_step", "steps", "dtype", "workload", "bound", "frac", "kernel", "other_roof",
                          "vs_cpu_forward", "traffic", "step", "overhead_ms", "vs_headline", "predicted_eff_8gpu", "wire",
                          "collect", "allreduce_ms", "no_comm_ms"} for c in line["configs"].values())
    assert "per_kernel" in detail["headline"] and len(detail["headline"]["per_kernel"]) >= 6


def test_a_multi_rank_line_explains_itself():
    """world > 1: the line carries per-rank step times, the collective phase and its bus bandwidth, and the efficiency against
    the comm-free rank program timed in the same run (review item 7) -- and still fits the window."""
    out, _ = full_output()
    for k in ("configs", "cpu_baseline", "native_fp32_mfma", "index_kernels"):
        out.pop(k, None)                                   # single-rank extras
    out.update(n_gpus=8, value=3100.5)
    out["dp"] = {"ms_per_step_local": 81.9, "allreduce_ms": 0.71, "allreduce_mb": 29.9, "allreduce_per_step": 1, "bus_gbps": 77.2,
                 "no_comm_ms_per_step_local": 80.9, "per_rank_ms_per_step": [81.7, 82.5], "per_rank_no_comm_ms": [80.4, 81.3],
                 "per_rank_allreduce_ms": [0.55, 1.4], "eff_vs_rank_program": 0.9855}
    line = json.loads(bench.fit_line(bench.compact_line(out)))
    assert line["dp"]["per_rank_ms_per_step"] == [81.7, 82.5] and line["dp"]["bus_gbps"] == 77.2
    assert line["dp"]["eff_vs_rank_program"] == 0.9855 and line["n_gpus"] == 8


def test_emit_writes_the_detail_file_and_one_stdout_line(tmp_path, capsys, monkeypatch):
    out, detail = full_output()
    monkeypatch.setattr(bench, "DETAIL_FILE", str(tmp_path / "bench_detail.json"))
    bench.emit(out, detail)
    cap = capsys.readouterr()
    lines = cap.out.strip().splitlines()
    assert len(lines) == 1 and json.loads(lines[0])["value"] == out["value"]
    full = json.load(open(tmp_path / "bench_detail.json"))
    assert full["detail"]["headline"]["per_kernel"] and full["cpu_baseline"]["all_samples_s"] == [10.7, 10.9]
    assert "[bench] detail:" in cap.err


def test_kernels_are_priced_against_the_roof_that_bounds_them():
    r32, _ = bench.roofline_of(canned_records("f32"), 1, "f32", None, True)
    # split fp32 GEMM: the bf16 matrix pipe with the flops it executes (6 x algorithmic)
    k = _key(b=32, p1=128, p2=128, cin=256, cout=256)
    fl = 7 * 2.0 * k[0] * k[2] * k[4] * k[7] * k[6] * k[5] * 2         # forward + data-gradient GEMMs of 7 layers
    assert r32["bound"] == "mfma" and r32["peak"] == 2500.0 and r32["kernel"] == "gemm_nt_x3_kernel<4,2,2,4,2>"
    assert abs(r32["achieved"] - 6 * fl / (14 * 1.2e-3) / 1e12) < 0.1 and abs(r32["algorithmic_fp32_tflops"] * 6 - r32["achieved"]) < 0.1
    assert r32["dominant_memory_bound_kernel"]["unit"] == "GB/s"
    r16, d16 = bench.roofline_of(canned_records("bf16"), 1, "bf16", None, True)
    # bf16: cin ks = 1536, cout = 64 -> 3.2 KB per column against 197 kflop: HBM-bound by 5x
    assert r16["bound"] == "hbm" and r16["kernel"] == "gemm_tn_bf16_kernel<2,2,4,8>"
    k = _key()
    cols = k[0] * k[2] * k[4]
    want = cols * (1536 + 64) * 2 / 1.3e-3 / 1e9
    assert abs(r16["achieved"] - want) < 1.0 and abs(r16["frac"] - want / 8000.0) < 1e-3
    assert r16["algorithmic_bytes_per_launch"] == cols * 1600 * 2
    nt = [v for n, v in d16["per_kernel"].items() if "gemm_nt_kernel" in n][0]
    assert nt["bound"] == "hbm" and nt["kernel"] == "gemm_nt_kernel<bf16,bf16,4,2,2,4,8,2>"


def test_short_kernel_names():
    s = bench.short_kernel
    assert s("_ZN3epn12_GLOBAL__N_127inter_ungroup_shared_kernelILi4ELi2EDF16bLi8ELi1ELb0ELi2ELi1EEEvNS0_9InterArgsEPKiPh") \
        == "inter_ungroup_shared_kernel<4,2,bf16,8,1,false,2,1>"
    assert s("_ZN3epn22inter_pack_cols_kernelIDF16bLb0EEEvPKfPT_iii") == "inter_pack_cols_kernel<bf16,false>"
    assert s("epn::gemm_nt_x3_kernel<4, 2, 2, 4, 2>") == "gemm_nt_x3_kernel<4,2,2,4,2>"
    assert s("void epn::(anonymous namespace)::gemm_tn_bf16_kernel<2, 2, 4, 8>(epn::GemmTnBatch)") == "gemm_tn_bf16_kernel<2,2,4,8>"
    assert s("_ZN3epn12_GLOBAL__N_120norm_act2_fwd_kernelIDF16bEEvNS0_9NormArgs2E") == "norm_act2_fwd_kernel<bf16>"
    assert s("_ZN3epn12_GLOBAL__N_123inter_group_wide_kernelILi1ELi2EfLi4EEEvNS0_9InterArgsE") == "inter_group_wide_kernel<1,2,float,4>"


def test_algorithmic_bytes_of_the_gemm_families():
    k = _key(b=32, p1=512, p2=512, nn=16, cin=64, cout=64)
    cols = 32 * 512 * 60
    assert bench.algo_bytes("inter_gemm", k, 4) == cols * (1536 + 64) * 4
    assert bench.algo_bytes("inter_gemm_dw", k, 2) == cols * (1536 + 64) * 2
    assert bench.algo_bytes("intra_gemm", ("spectral", 16384, 64, 128), 4) == 16384 * 60 * 192 * 4
    assert bench.algo_bytes("conv1x1_gemm", ("nt", 1000, 64, 32), 4) == 1000 * 96 * 4
    assert bench.algo_bytes("inter_group", k, 4) == (32 * 512 * 60 * 64 + cols * 1536) * 4
    assert bench.algo_bytes("norm_act_fwd", (), 4) == 0


def test_an_oversized_line_is_trimmed_not_printed():
    out, _ = full_output()
    out["config"]["workload"] = out["config"]["workload"] + " " + "x" * 900
    for c in out["configs"].values():
        c["config"] = dict(c["config"], workload=out["config"]["workload"])
    text = bench.fit_line(bench.compact_line(out))
    line = json.loads(text)
    assert len(text) < bench.LINE_LIMIT and "roofline" in line and "cpu_baseline" in line and line["value"] == out["value"]


def test_dumped_outputs_stay_under_the_limit_and_sample_the_same_elements(tmp_path):
    """--dump-outputs: loss, network outputs (tuples and point clouds flattened to named leaves), gradients and parameters as
    float32 (float64 kept), at most 64 MB in all; an array over its share is a seeded sample -- the same elements every run."""
    import numpy as np
    import torch

    class Cloud:
        def __init__(self, xyz, feats):
            self.xyz, self.feats = xyz, feats

    big = torch.nn.Parameter(torch.arange(9 * 2 ** 20, dtype=torch.float32))
    small = torch.nn.Parameter(torch.ones(3, dtype=torch.float64))
    big.grad = -big.detach()
    out = (torch.ones(2, 4, dtype=torch.bfloat16), Cloud(torch.zeros(1, 3, 5), torch.full((1, 2, 5, 60), 2.0, dtype=torch.float64)))
    arrays = bench.step_outputs(torch.tensor(0.5), out, [big, small], with_grads=True)
    assert set(arrays) == {"loss", "output_0", "output_1_xyz", "output_1_feats", "grads", "params"}
    assert arrays["output_0"].dtype == np.float32 and arrays["output_1_feats"].dtype == np.float64
    assert arrays["grads"].size == 9 * 2 ** 20 + 3 and not arrays["grads"][-3:].any()       # no gradient: zeros
    runs = []
    for d in ("a", "b"):
        bench.write_outputs(arrays, str(tmp_path / d))
        runs.append({f.name: np.load(f) for f in (tmp_path / d).iterdir()})
        assert sum(f.stat().st_size for f in (tmp_path / d).iterdir()) <= 64e6
    a, b = runs
    assert set(a) == {n + ".npy" for n in arrays} and a["loss.npy"] == np.float32(0.5)
    assert a["params.npy"].size < arrays["params"].size and np.array_equal(a["params.npy"], b["params.npy"])
    g, p = a["grads.npy"], a["params.npy"]
    assert np.all((g == -p) | (g == 0))                      # same length, same elements: gradient and parameter side by side
    assert np.all(np.diff(p[p > 1.5]) > 0)                   # sampled in element order
    assert np.array_equal(a["output_1_feats.npy"], arrays["output_1_feats"])                  # small arrays: whole
