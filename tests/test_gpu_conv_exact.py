"""The fused inter / intra SO(3) convolution kernels (csrc/inter_mfma.hip, csrc/intra_mfma.hip) through the plain C entries
epn_{inter,intra}_so3conv_{fwd,bwd_data,bwd_weight}_f32, held to EXACT results at the edges of every kernel instance.

1. Exact tier (tests/conv_cases.py): dyadic geometry and integer operands, so that every output equals the float64 restatement
   of tests/conv_ref.py by `==` whatever the summation or atomic order.  Outputs and workspace are regions of sentinel-filled
   buffers (tests/gemm_ref.py Arena): nothing around them may change; the outputs are pre-filled with 7.0, because the header says
   the gradients are zero-filled / overwritten by the call.  After every call epn_last_kernel() must name the instance the
   restated dispatch predicts, and the last test compares the union with conv_cases.REACHABLE.
2. Invariances: permuted neighbour slots, appended shadow slots (nn across an NT boundary and across the 8-wave limit), features
   scaled by a power of two.
3. Real-geometry tier: icosahedral anchors, the shipped kernel points, unit-ball clouds, radius / sigma of the first and of a
   K = 64 layer: |kernel - fp64| <= REAL_M 2^-24 S element by element (S: sum of absolute values of the expanded form's terms).
   REAL_M comes from the CPU fp32 oracle (tests/test_conv_spec.py), never from the kernels.  The intra kernels have no
   geometry; what integers cannot see there -- a narrowed operand -- is tested with selecting operands against full-mantissa
   values, again by `==`.

fp32 MFMA operands: all six fused kernels feed v_mfma_f32_16x16x4_f32 with full fp32 values (mfma4 in inter_device.h and
intra_mfma.hip; no operand is narrowed), so no instance is held to anything weaker than `==`."""
import numpy as np
import pytest
import torch

import conv_cases as C
import conv_ref as CR
import gemm_ref as R

pytestmark = pytest.mark.gpu
F32 = torch.float32
RECORDED = {}          # ("inter" / "intra", pass) -> instance names epn_last_kernel() reported
DONE = {}              # case -> failures (each case runs once per session)
REAL_WORST = {}        # pass -> worst |kernel - fp64| / (2^-24 S) of the real-geometry tier (printed: CHANGELOG quotes it)


def _lib():
    from epn_pointcloud_amd import _lib
    return _lib, _lib.get_lib()


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _report(bad):
    assert not bad, f"{len(bad)} failure(s):\n" + "\n".join(bad[:40])


def _compare(got, ref, what):
    got = got.detach().cpu().double().numpy().reshape(ref.shape)
    if np.array_equal(got, ref):
        return []
    d = np.abs(got - ref)
    return [f"{what}: {int((d > 0).sum())} of {d.size} elements differ (NaN: {int(np.isnan(got).sum())}), max |diff| "
            f"{np.nanmax(d):g}, first at {tuple(int(i) for i in np.argwhere(~(d == 0))[0])}"]


# ------------------------------------------------------------------------------------------------ inter runner
class InterDevice:
    """Device copies of one case's geometry and operands, and its descriptor."""

    def __init__(self, gpu, c, d):
        _l, lib = _lib()
        self.c, self.gpu = c, gpu
        self.t = {k: _dev(d[k], gpu) for k in ("xyz", "new_xyz", "idx", "anchors", "kernels", "F", "W", "gOut")}
        desc = _l.InterDesc()
        desc.xyz, desc.new_xyz, desc.ball_idx = self.t["xyz"].data_ptr(), self.t["new_xyz"].data_ptr(), self.t["idx"].data_ptr()
        desc.anchors, desc.kernels, desc.dense_w, desc.sigma = self.t["anchors"].data_ptr(), self.t["kernels"].data_ptr(), None, d["sigma"]
        desc.b, desc.p1, desc.p2, desc.nn, desc.na = c.b, d["xyz"].shape[2], c.p2, d["idx"].shape[2], c.na
        desc.ks, desc.cin, desc.cout = c.ks, c.cin, c.cout
        self.desc, self.p1 = desc, d["xyz"].shape[2]
        self.need = int(lib.epn_inter_workspace_bytes(desc))

    def run(self, which, guard=True):
        """One call; returns (output tensor, instance name, failures of the guard bands and of the return code)."""
        _l, lib = _lib()
        c, t, bad = self.c, self.t, []
        rows, cols = {"fwd": (c.b * c.p2 * c.na, c.cout), "bwd_data": (c.b * self.p1 * c.na, c.cin),
                      "bwd_weight": (c.cout, c.cin * c.ks)}[which]
        arena, out = R.guarded(rows, cols, F32, self.gpu)
        out.fill_(7.0)
        wa, ws = R.guarded(1, self.need, torch.uint8, self.gpu)
        st = _l.stream_of(out)
        lib.epn_last_kernel()
        tail = (ws.data_ptr(), self.need, st)
        if which == "fwd":
            rc = lib.epn_inter_so3conv_fwd_f32(self.desc, t["F"].data_ptr(), t["W"].data_ptr(), out.data_ptr(), *tail)
        elif which == "bwd_data":
            rc = lib.epn_inter_so3conv_bwd_data_f32(self.desc, t["gOut"].data_ptr(), t["W"].data_ptr(), out.data_ptr(), *tail)
        else:
            rc = lib.epn_inter_so3conv_bwd_weight_f32(self.desc, t["F"].data_ptr(), t["gOut"].data_ptr(), out.data_ptr(), *tail)
        torch.cuda.synchronize()
        name = C.normalise(lib.epn_last_kernel())
        if rc != 0:
            bad.append(f"{c.name} {which}: the entry returned {rc} ({lib.epn_strerror(rc).decode()})")
        if guard:
            for a, what in ((arena, "output"), (wa, "workspace")):
                try:
                    a.check(f"{c.name} {which} [{name}] {what}")
                except AssertionError as e:
                    bad.append(str(e))
        return out, name, bad


def run_inter(gpu, c):
    if c not in DONE:
        d = C.inter_case(c)
        dev = InterDevice(gpu, c, d)
        bad = []
        for which in c.passes:
            out, name, b = dev.run(which)
            bad += b
            RECORDED.setdefault(("inter", which), set()).add(name)
            want = C.inter_instance(c, which)
            if name != want:
                bad.append(f"{c.name} {which}: ran {name}, the restated dispatch says {want}")
            bad += _compare(out, d["ref"][C.OUTPUT[which]], f"{c.name} {which} [{name}] (q = {d['q']})")
        DONE[c] = bad
    return DONE[c]


@pytest.mark.parametrize("c", C.INTER_CASES, ids=lambda c: c.name)
def test_inter_exact(gpu, c):
    """out, dF and dW of the dyadic case equal float64 by `==`, inside guard bands, from the predicted instance."""
    _report(run_inter(gpu, c))


# ------------------------------------------------------------------------------------------------ intra runner
def intra_call(gpu, c, d, which, F=None):
    _l, lib = _lib()
    bad = []
    t = {k: _dev(d[k], gpu) for k in ("idx", "inv", "F", "W", "gOut")}
    if F is not None:
        t["F"] = F
    need = int(lib.epn_intra_workspace_bytes(c.na, c.kn, c.cin, c.cout))
    rows, cols = {"fwd": (c.b * c.p * c.na, c.cout), "bwd_data": (c.b * c.p * c.na, c.cin),
                  "bwd_weight": (c.cout, c.cin * c.kn)}[which]
    arena, out = R.guarded(rows, cols, F32, gpu)
    out.fill_(7.0)
    wa, ws = R.guarded(1, need, torch.uint8, gpu)
    st = _l.stream_of(out)
    shape = (c.b, c.p, c.na, c.kn, c.cin, c.cout)
    lib.epn_last_kernel()
    if which == "fwd":
        rc = lib.epn_intra_so3conv_fwd_f32(t["F"].data_ptr(), t["idx"].data_ptr(), t["W"].data_ptr(), *shape, out.data_ptr(),
                                           ws.data_ptr(), need, st)
    elif which == "bwd_data":
        rc = lib.epn_intra_so3conv_bwd_data_f32(t["gOut"].data_ptr(), t["idx"].data_ptr(), t["inv"].data_ptr(), t["W"].data_ptr(),
                                                *shape, out.data_ptr(), ws.data_ptr(), need, st)
    else:
        rc = lib.epn_intra_so3conv_bwd_weight_f32(t["F"].data_ptr(), t["gOut"].data_ptr(), t["idx"].data_ptr(), *shape,
                                                  out.data_ptr(), st)
    torch.cuda.synchronize()
    name = C.normalise(lib.epn_last_kernel())
    if rc != 0:
        bad.append(f"{c.name} {which}: the entry returned {rc} ({lib.epn_strerror(rc).decode()})")
    for a, what in ((arena, "output"), (wa, "workspace")):
        try:
            a.check(f"{c.name} {which} [{name}] {what}")
        except AssertionError as e:
            bad.append(str(e))
    return out, name, bad


def run_intra(gpu, c):
    if c not in DONE:
        d = C.intra_case(c)
        bad = []
        for which in C.PASSES:
            out, name, b = intra_call(gpu, c, d, which)
            bad += b
            RECORDED.setdefault(("intra", which), set()).add(name)
            want = C.intra_instance(c, which)
            if name != want:
                bad.append(f"{c.name} {which}: ran {name}, the restated dispatch says {want}")
            bad += _compare(out, d["ref"][C.OUTPUT[which]], f"{c.name} {which} [{name}]")
        DONE[c] = bad
    return DONE[c]


@pytest.mark.parametrize("c", C.INTRA_CASES, ids=lambda c: c.name)
def test_intra_exact(gpu, c):
    """Integer operands, intra_idx columns that are random permutations (not the icosahedral table), the inverse table built as
    epn_pointcloud_amd.ops builds it: out, dF, dW equal float64 by `==`."""
    _report(run_intra(gpu, c))


# ------------------------------------------------------------------------------------------------ 2. invariances
def _by_name(name):
    return next(c for c in C.INTER_CASES if c.name == name)


@pytest.mark.parametrize("name", ["k24_n15_32", "k24_n33_64", "k12_n17", "k32_n17", "k24_n128_48_a12"])
def test_inter_slot_permutation_is_bitwise_invisible(gpu, name):
    """The neighbour slots of every row permuted (another order of the same multiset): out and dW bitwise equal, dF as well."""
    c = _by_name(name)
    d = dict(C.inter_case(c))
    base = InterDevice(gpu, c, d)
    rng = np.random.default_rng(5)
    d["idx"] = np.ascontiguousarray(rng.permuted(d["idx"], axis=2))
    perm = InterDevice(gpu, c, d)
    bad = []
    for which in c.passes:
        a, _, b1 = base.run(which)
        b_, _, b2 = perm.run(which)
        bad += b1 + b2
        if not torch.equal(a, b_):
            bad.append(f"{name} {which}: {int((a != b_).sum())} elements change under a permutation of the neighbour slots")
    _report(bad)


@pytest.mark.parametrize("name,nn2", [("k24_n15_32", 17), ("k24_n32_80", 33), ("k12_n17", 33), ("k24_n64_32_c127", 65),
                                      ("k32_n16", 40), ("k16_n16", 128)])
def test_inter_appended_shadow_slots_change_nothing(gpu, name, nn2):
    """nn raised across an NT boundary (and out of the 8-wave kernels) by shadow entries behind every row: another instance, the
    same bits."""
    c = _by_name(name)
    d = dict(C.inter_case(c))
    base = InterDevice(gpu, c, d)
    p1 = d["xyz"].shape[2]
    d["idx"] = np.ascontiguousarray(np.concatenate([d["idx"], np.full((c.b, c.p2, nn2 - c.nn), p1, np.int32)], axis=2))
    c2 = c._replace(nn=nn2)
    wide = InterDevice(gpu, c2, d)
    bad = []
    for which in c.passes:
        a, n1, b1 = base.run(which)
        b_, n2, b2 = wide.run(which)
        bad += b1 + b2
        if n2 != C.inter_instance(c2, which) or n1 == n2:
            bad.append(f"{name} {which}: nn = {c.nn} ran {n1}, nn = {nn2} ran {n2} (expected {C.inter_instance(c2, which)})")
        if not torch.equal(a, b_):
            bad.append(f"{name} {which}: {int((a != b_).sum())} elements change when shadow slots are appended ({n1} -> {n2})")
    _report(bad)


# ------------------------------------------------------------------------------------------------ 3. real geometry
@pytest.mark.parametrize("entry", C.REAL_INTER, ids=lambda e: e[0])
def test_inter_real_geometry_within_the_oracles_error(gpu, entry):
    """No element excluded (w is continuous at the clamp); F scaled by 2^5 scales out bitwise."""
    c, d, ref, S = C.real_inter_reference(entry)
    dev = InterDevice(gpu, c, d)
    bad = []
    for which in C.PASSES:
        out, name, b = dev.run(which)
        bad += b
        if name != C.inter_instance(c, which):
            bad.append(f"{c.name} {which}: ran {name}, expected {C.inter_instance(c, which)}")
        key = C.OUTPUT[which]
        got = out.cpu().double().numpy().reshape(ref[key].shape)
        ratio = float((np.abs(got - ref[key]) / (2.0 ** -24 * S[key] + 1e-300)).max())
        REAL_WORST[("inter", which)] = max(REAL_WORST.get(("inter", which), 0.0), ratio)
        print(f"real geometry, {c.name} {which} [{name}]: worst |kernel - fp64| / (2^-24 S) = {ratio:.4f} (REAL_M = {C.REAL_M})")
        if not ratio <= C.REAL_M:
            bad.append(f"{c.name} {which} [{name}]: |kernel - fp64| reaches {ratio:.4f} x 2^-24 S, allowed {C.REAL_M}")
    out1, _, b1 = dev.run("fwd", guard=False)
    dev.t["F"] = dev.t["F"] * 32.0
    out2, _, b2 = dev.run("fwd", guard=False)
    bad += b1 + b2
    if not torch.equal(out2, out1 * 32.0):
        bad.append(f"{c.name}: out(32 F) != 32 out(F) in {int((out2 != out1 * 32.0).sum())} elements")
    _report(bad)


@pytest.mark.parametrize("c", C.REAL_INTRA, ids=lambda c: c.name)
def test_intra_no_operand_bit_is_dropped(gpu, c):
    """What integers cannot see in the intra kernels: a narrowed operand.  One operand selects (a single +-2^e per output element's
    contraction, every other term an exact zero), the other holds full-mantissa values sign (1 + u): every output is +-2^e times
    ONE input value and must equal it bit for bit -- `==` against float64, no tolerance.  Forward: W has one entry per row o;
    data gradient: W has one entry per input channel c; weight gradient: dOut has one entry per output channel, in distinct
    columns.  The icosahedral table (kn = 13: its first column once more).  Then out(F / 8) == out(F) / 8 bitwise."""
    from epn_pointcloud_amd.vgtk.so3conv import functional as L
    tab = np.asarray(L.get_intra_idx(), dtype=np.int32)
    idx = np.ascontiguousarray(tab[:, :c.kn] if c.kn <= 12 else np.concatenate([tab, tab[:, :c.kn - 12]], axis=1))
    seed = C.hash_name(c.name) % 10000
    ncol, ck = c.b * c.p * c.na, c.cin * c.kn
    full = lambda shape, k: R.full_mantissa(shape, seed + k).numpy()
    zeros = lambda *shape: np.zeros(shape, np.float32)
    rng = np.random.default_rng(seed)
    Wc = zeros(c.cout, c.cin, c.kn)                                         # one entry per input channel
    Wc[rng.integers(0, c.cout, c.cin), np.arange(c.cin), rng.integers(0, c.kn, c.cin)] = R.selection_rows(c.cin, 1, seed + 7)[2].numpy()
    ops = {"fwd": dict(F=full((c.b, c.p, c.na, c.cin), 1), W=R.selection_rows(c.cout, ck, seed + 2)[0].numpy(),
                       gOut=zeros(c.b, c.p, c.na, c.cout)),
           "bwd_data": dict(F=zeros(c.b, c.p, c.na, c.cin), W=Wc.reshape(c.cout, ck), gOut=full((c.b, c.p, c.na, c.cout), 3)),
           "bwd_weight": dict(F=full((c.b, c.p, c.na, c.cin), 4), W=zeros(c.cout, ck),
                              gOut=R.selection_cols(ncol, c.cout, seed + 5)[0].numpy().reshape(c.b, c.p, c.na, c.cout))}
    bad = []
    for which in C.PASSES:
        d = dict(idx=idx, inv=CR.inverse_intra_idx(idx), **ops[which])
        ref = CR.intra_conv(d["F"], d["W"], idx, d["gOut"])[C.OUTPUT[which]]
        assert np.any(ref != 0) and np.array_equal(ref, ref.astype(np.float32))
        out, name, b = intra_call(gpu, c, d, which)
        bad += b
        if name != C.intra_instance(c, which):
            bad.append(f"{c.name} {which}: ran {name}, expected {C.intra_instance(c, which)}")
        bad += _compare(out, ref, f"{c.name} {which} [{name}], selecting operand")
    d = dict(idx=idx, inv=CR.inverse_intra_idx(idx), F=full((c.b, c.p, c.na, c.cin), 8), W=full((c.cout, ck), 9),
             gOut=zeros(c.b, c.p, c.na, c.cout))
    out1, _, b1 = intra_call(gpu, c, d, "fwd")
    out2, _, b2 = intra_call(gpu, c, d, "fwd", F=_dev(d["F"], gpu) * 0.125)
    bad += b1 + b2
    if not torch.equal(out2, out1 * 0.125):
        bad.append(f"{c.name}: out(F / 8) != out(F) / 8")
    _report(bad)


# ------------------------------------------------------------------------------------------------ instance coverage (last)
def test_every_reachable_conv_instance_was_run(gpu):
    """The union of the instances epn_last_kernel() named during the exact cases equals conv_cases.REACHABLE per pass: a dispatch
    branch nobody reaches, or a new instance nobody lists, fails here.  (Cases deselected from the run are run now.)"""
    bad = []
    for c in C.INTER_CASES:
        bad += run_inter(gpu, c)
    for c in C.INTRA_CASES:
        bad += run_intra(gpu, c)
    for key, want in C.REACHABLE.items():
        got = RECORDED.get(key, set())
        assert got == want, f"{key}: never ran {sorted(want - got)}; ran but not listed {sorted(got - want)}"
    _report(bad)
