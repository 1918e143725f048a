"""The grouping entries of the split convolution -- epn_inter_group_{f32,bf16}, epn_inter_group_packed_{f32,bf16},
epn_inter_ungroup_{f32,bf16}, epn_inter_ungroup_det_{f32,bf16} and epn_inter_inverse_list -- held to the instance their launchers
must choose.  For every case of conv_cases.GROUP_CASES / INV_CASES (the smallest shapes on both sides of every edge of the choice)
each call must return the restated code, epn_last_kernel() must name the restated instance, and the result must agree with the
float64 restatement of tests/conv_ref.py (inter_weights, the gather for G, its transpose for dF).  G is filled with NaN and dF
with 7 before the call: a tile that was not launched cannot pass.  The last test compares the union of the names with
conv_cases.REACHABLE_GROUPING.

Tolerances are the ones these entries already have: TOL of tests/test_gpu_conv.py for fp32 (absolute), BF16_TOL of
tests/test_gpu_bf16.py times the reference's largest magnitude for bf16.  They are not the point: a missing tile or a wrong chunk
count is an error of order one."""
import ctypes

import numpy as np
import pytest
import torch

import conv_cases as C

pytestmark = pytest.mark.gpu
TOL = 1e-3             # tests/test_gpu_conv.py
BF16_TOL = 2e-2        # tests/test_gpu_bf16.py
RECORDED = {}          # family -> instance names epn_last_kernel() reported
DONE = {}              # case -> failures (each case runs once per session)


def _lib():
    from epn_pointcloud_amd import _lib
    return _lib, _lib.get_lib()


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _report(bad):
    assert not bad, f"{len(bad)} failure(s):\n" + "\n".join(bad[:40])


def _judge(bad, what, family, rc, name, want, got=None, ref=None, bf16=0):
    """Return code, instance name and result of one call against the restatement (want None: the entry refuses the shape)."""
    _l, lib = _lib()
    if want is None:
        if rc != C.EPN_EINVAL:
            bad.append(f"{what}: returned {rc}, the restatement says EPN_EINVAL")
        return
    RECORDED.setdefault(family, set()).add(name)
    if rc != 0:
        bad.append(f"{what}: the entry returned {rc} ({lib.epn_strerror(rc).decode()})")
    if name != want:
        bad.append(f"{what}: ran {name}, the restated dispatch says {want}")
    if got is not None:
        got = got.detach().float().cpu().double().numpy().reshape(ref.shape)
        tol = BF16_TOL * np.abs(ref).max() if bf16 else TOL
        err = np.abs(got - ref)
        print(f"{what} [{name}]: max |got - fp64| = {np.nanmax(err):.3g} (bound {tol:.3g}), NaN {int(np.isnan(got).sum())}")
        if not (err < tol).all():
            bad.append(f"{what} [{name}]: {int((~(err < tol)).sum())} of {err.size} elements off by more than {tol:g} "
                       f"(NaN: {int(np.isnan(got).sum())}), max |diff| {np.nanmax(err):g}")


def run_group(gpu, c):
    if c in DONE:
        return DONE[c]
    _l, lib = _lib()
    d = C.group_case(c)
    t = {k: _dev(d[k], gpu) for k in ("xyz", "new_xyz", "idx", "anchors", "kernels", "F", "dG")}
    desc = _l.InterDesc()
    desc.xyz, desc.new_xyz, desc.ball_idx = t["xyz"].data_ptr(), t["new_xyz"].data_ptr(), t["idx"].data_ptr()
    desc.anchors, desc.kernels, desc.dense_w, desc.sigma = t["anchors"].data_ptr(), t["kernels"].data_ptr(), None, c.sigma
    desc.b, desc.p1, desc.p2, desc.nn, desc.na, desc.ks, desc.cin, desc.cout = c.b, c.p1, c.p2, c.nn, c.na, c.ks, c.cin, 16
    need = int(lib.epn_inter_group_workspace_bytes(ctypes.byref(desc)))
    ws = torch.zeros(need, dtype=torch.uint8, device=gpu)
    st = _l.stream_of(ws)
    tail = (ws.data_ptr(), need, st)
    rows, cols = c.b * c.p2 * c.na, c.cin * c.ks
    pos = torch.from_numpy(C.packed_position(c.cin, c.ks)).to(gpu) if c.cin % 32 == 0 else None
    # the inverse neighbour list of the deterministic entry (its own kernels are judged by the INV_CASES)
    off = torch.empty((c.b, c.p1 + 1), dtype=torch.int32, device=gpu)
    ent = torch.full((c.b, c.p2 * c.nn), -1, dtype=torch.int32, device=gpu)
    bad = []
    rc = lib.epn_inter_inverse_list(t["idx"].data_ptr(), c.b, c.p1, c.p2, c.nn, off.data_ptr(), ent.data_ptr(), st)
    if rc != 0:
        bad.append(f"{c.name}: epn_inter_inverse_list returned {rc}")
    for bf16 in (0, 1):
        dt = torch.bfloat16 if bf16 else torch.float32
        sfx = "bf16" if bf16 else "f32"
        F, dG = t["F"].to(dt), t["dG"].to(dt)
        for packed in (0, 1):
            G = torch.full((rows, cols), float("nan"), dtype=dt, device=gpu)
            entry = getattr(lib, f"epn_inter_group{'_packed' if packed else ''}_{sfx}")
            lib.epn_last_kernel()
            rc = entry(ctypes.byref(desc), F.data_ptr(), G.data_ptr(), *tail)
            torch.cuda.synchronize()
            name = C.normalise(lib.epn_last_kernel())
            want = C.group_instance(c, bf16, packed)
            if packed and want is not None:
                G = G[:, pos]                                                  # packed[:, pos[q]] = plain[:, q]
            _judge(bad, f"{c.name} group{'_packed' if packed else ''}_{sfx}", "group", rc, name, want, G, d["G"], bf16)
        dF = torch.full((c.b, c.p1, c.na, c.cin), 7.0, dtype=torch.float32, device=gpu)       # fp32 whatever dG is
        lib.epn_last_kernel()
        rc = getattr(lib, f"epn_inter_ungroup_{sfx}")(ctypes.byref(desc), dG.data_ptr(), dF.data_ptr(), *tail)
        torch.cuda.synchronize()
        name = C.normalise(lib.epn_last_kernel())
        _judge(bad, f"{c.name} ungroup_{sfx}", "ungroup", rc, name, C.ungroup_instance(c, bf16), dF, d["dF"], bf16)
        # slab [b][p2][nn][na][cin] of dG's type, and behind it (256-byte aligned) one mark per slot: the pre-reduced form
        slab_need = c.b * c.p2 * c.nn * c.na * c.cin * (2 if bf16 else 4)
        slab_bytes = ((slab_need + 255) & ~255) + c.b * c.p2 * c.nn
        slab = torch.zeros(slab_bytes, dtype=torch.uint8, device=gpu)
        dF = torch.full((c.b, c.p1, c.na, c.cin), 7.0, dtype=dt, device=gpu)
        lib.epn_last_kernel()
        rc = getattr(lib, f"epn_inter_ungroup_det_{sfx}")(ctypes.byref(desc), dG.data_ptr(), dF.data_ptr(), off.data_ptr(),
                                                          ent.data_ptr(), slab.data_ptr(), slab_bytes, *tail)
        torch.cuda.synchronize()
        name = C.normalise(lib.epn_last_kernel())
        _judge(bad, f"{c.name} ungroup_det_{sfx}", "ungroup_det", rc, name, C.ungroup_det_instance(c, bf16), dF, d["dF"], bf16)
    DONE[c] = bad
    return bad


def run_inverse(gpu, c):
    if c in DONE:
        return DONE[c]
    _l, lib = _lib()
    d = C.group_case(c)
    idx = _dev(d["idx"], gpu)
    off = torch.full((c.b, c.p1 + 1), -7, dtype=torch.int32, device=gpu)
    ent = torch.full((c.b, c.p2 * c.nn), -1, dtype=torch.int32, device=gpu)
    bad = []
    lib.epn_last_kernel()
    rc = lib.epn_inter_inverse_list(idx.data_ptr(), c.b, c.p1, c.p2, c.nn, off.data_ptr(), ent.data_ptr(), _l.stream_of(idx))
    torch.cuda.synchronize()
    name = C.normalise(lib.epn_last_kernel())
    _judge(bad, f"inverse list {c.name}", "inverse_list", rc, name, C.inverse_list_instance(c))
    if not np.array_equal(off.cpu().numpy(), d["off"]):
        bad.append(f"inverse list {c.name} [{name}]: the offsets differ")
    n_ent = d["off"][:, -1]
    for bb in range(c.b):
        if not np.array_equal(ent[bb, :n_ent[bb]].cpu().numpy(), d["ent"][bb, :n_ent[bb]]):
            bad.append(f"inverse list {c.name} [{name}]: the entries of cloud {bb} differ")
    DONE[c] = bad
    return bad


@pytest.mark.parametrize("c", C.GROUP_CASES, ids=lambda c: c.name)
def test_grouping_entries_run_the_restated_instance(gpu, c):
    """Return code, instance name and result (against float64) of the eight grouping calls of a case."""
    _report(run_group(gpu, c))


@pytest.mark.parametrize("c", C.INV_CASES, ids=lambda c: c.name)
def test_inverse_list_runs_the_restated_kernel(gpu, c):
    _report(run_inverse(gpu, c))


def test_every_reachable_grouping_instance_was_run(gpu):
    """The union of the names seen equals conv_cases.REACHABLE_GROUPING per family: a branch nobody reaches, an entry of the launchers'
    tables the restatement does not know, or a case that drifted to a neighbouring instance fails here.  (Cases deselected from
    the run are run now.)"""
    bad = []
    for c in C.GROUP_CASES:
        bad += run_group(gpu, c)
    for c in C.INV_CASES:
        bad += run_inverse(gpu, c)
    _report(bad)
    for family in ("group", "ungroup", "ungroup_det", "inverse_list"):
        assert RECORDED.get(family, set()) == C.REACHABLE_GROUPING[family], (family, RECORDED.get(family, set()) ^ C.REACHABLE_GROUPING[family])
