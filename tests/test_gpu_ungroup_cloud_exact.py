"""-m gpu: the cloud-resident grouping transpose (csrc/inter_ungroup_cloud.hip) through its C entries
epn_inter_ungroup_cloud_{f32,bf16}, held to EXACT results at the edges of every kernel instance.  The kernel's contract is "every
contribution rounded once to the unit, the sum exact, one rounding to the output type": every comparison of tiers 1 - 5 is `==`.

1. Exact tier (tests/cloud_cases.py, proofs in tests/test_cloud_spec.py): dyadic geometry, integer dG and add.  Every case runs
   fp32, bf16 -> bf16 and bf16 -> fp32, plain and with `add` (a separate tensor, and the output itself).  Output and workspace are
   regions of sentinel-filled arenas (tests/gemm_ref.py), the output pre-filled with 7.0; after every call epn_last_kernel() must
   name the restated instance and epn_inter_ungroup_cloud_range_count(1) must read 0.  A refused shape returns EPN_EINVAL and
   writes nothing; p2 = 0 gives zeros, or add.
2. Maximum and scale: the true max|dG|, NULL (the entry's own pass) and a maximum overstated by 2^6 give the same bits; dG scaled
   by 2^-20 and 2^10 scales the result bitwise; the bound's extreme inside the contract is exact and silent.
3. Invariances: permuted neighbour slots and appended shadow slots (another instance) leave every bit.
4. Rows whose kept slots name one point many times (not cyclic, or cyclic with such a period), on both sides of the point count where the 64-bit sum would wrap
   if such a row reported multiplicity 1: the float64 sum rounded once, or a loud NaN -- never a wrapped value.
5. Real-geometry tier: |kernel - fp64| <= CLOUD_REAL_M 2^-24 S element by element, the constant from the emulation of the
   documented arithmetic (tests/test_cloud_spec.py), never from the kernel.
The last test compares the union of the recorded instance names with cloud_cases.REACHABLE_CLOUD."""
import ctypes

import numpy as np
import pytest
import torch

import cloud_cases as K
import conv_cases as C
import gemm_ref as R
from test_gpu_conv_exact import _compare, _dev, _lib, _report

pytestmark = pytest.mark.gpu
RECORDED = set()       # instance names epn_last_kernel() reported
DONE = {}              # case -> failures (each case runs once per session)
REAL_WORST = {}        # type -> worst |kernel - fp64| / (2^-24 S) of the real-geometry tier (printed: CHANGELOG quotes it)
FORMS = {"f32": (torch.float32, torch.float32), "bf16": (torch.bfloat16, torch.bfloat16), "bf16_f32": (torch.bfloat16, torch.float32)}


class CloudDevice:
    """Device copies of one case's geometry, its descriptor, and calls of the entries inside guard bands."""

    def __init__(self, gpu, c, d):
        _l, lib = _lib()
        self.c, self.gpu = c, gpu
        self.t = {k: _dev(d[k], gpu) for k in ("xyz", "new_xyz", "idx", "anchors", "kernels")}
        desc = _l.InterDesc()
        desc.xyz, desc.new_xyz, desc.ball_idx = self.t["xyz"].data_ptr(), self.t["new_xyz"].data_ptr(), self.t["idx"].data_ptr()
        desc.anchors, desc.kernels, desc.dense_w, desc.sigma = self.t["anchors"].data_ptr(), self.t["kernels"].data_ptr(), None, float(d["sigma"])
        desc.b, desc.p1, desc.p2, desc.nn, desc.na, desc.ks, desc.cin, desc.cout = c.b, c.p1, c.p2, c.nn, c.na, c.ks, c.cin, 16
        self.desc = desc
        self.ok = int(lib.epn_inter_ungroup_cloud_ok(ctypes.byref(desc)))
        self.need = int(lib.epn_inter_ungroup_cloud_workspace_bytes(ctypes.byref(desc)))

    def call(self, form, dG, amax="true", add=None, alias=False, silent=True):
        """One call.  dG: float32 array (bf16-representable); amax: "true", None (NULL) or a float; add: float32 array or None;
        alias: add IS the output.  Returns (output, instance name, range count, failures of code, guards and counter)."""
        _l, lib = _lib()
        c, bad = self.c, []
        din, dout = FORMS[form]
        g = _dev(dG, self.gpu).to(din)
        arena, out = R.guarded(c.b * c.p1 * c.na, c.cin, dout, self.gpu)
        out.fill_(7.0)
        a = None
        if add is not None:
            a = _dev(add, self.gpu).to(dout).reshape(out.shape)
            if alias:
                out.copy_(a)
                a = out
            else:
                a = a.contiguous()
        wa, ws = R.guarded(1, max(self.need, 256), torch.uint8, self.gpu)
        am = None
        if amax is not None:
            am = torch.tensor([float(np.abs(dG).max()) if amax == "true" else float(amax)], dtype=torch.float32, device=self.gpu)
        lib.epn_inter_ungroup_cloud_range_count(1)
        lib.epn_last_kernel()
        args = [ctypes.byref(self.desc), g.data_ptr(), None if am is None else am.data_ptr(), out.data_ptr(), None if a is None else a.data_ptr()]
        tail = (ws.data_ptr(), self.need, _l.stream_of(out))
        if form == "f32":
            rc = lib.epn_inter_ungroup_cloud_f32(*args, *tail)
        else:
            rc = lib.epn_inter_ungroup_cloud_bf16(*args, 1 if form == "bf16_f32" else 0, *tail)
        torch.cuda.synchronize()
        name = C.normalise(lib.epn_last_kernel())
        count = int(lib.epn_inter_ungroup_cloud_range_count(1))
        what = f"{c.name} {form}{' + add' if add is not None else ''}{' (in place)' if alias else ''} [{name}]"
        if rc != (0 if self.ok else K.EPN_EINVAL):
            bad.append(f"{what}: the entry returned {rc} ({lib.epn_strerror(rc).decode()})")
        if silent and count != 0:
            bad.append(f"{what}: the range counter reads {count}")
        for ar, region in ((arena, "output"), (wa, "workspace")):
            try:
                ar.check(f"{what} {region}")
            except AssertionError as e:
                bad.append(str(e))
        self.wa = wa
        return out, name, count, bad


def _judge(dev, form, dG, ref, bad, add=None, alias=False, record=True, **kw):
    """A call whose result must equal float64 (+ add) rounded once to the output type, from the restated instance."""
    out, name, _, b = dev.call(form, dG, add=add, alias=alias, **kw)
    bad += b
    want = K.cloud_instance(dev.c, form != "f32")
    if record:
        RECORDED.add(name)
    if name != want:
        bad.append(f"{dev.c.name} {form}: ran {name}, the restated dispatch says {want}")
    exp = K.expected(ref, add, form == "bf16").astype(np.float64)
    bad += _compare(out.float(), exp, f"{dev.c.name} {form}{' + add' if add is not None else ''}{' (in place)' if alias else ''} [{name}]")
    return out


def run_cloud(gpu, c):
    if c in DONE:
        return DONE[c]
    _l, lib = _lib()
    bad = []
    if c.name in K.REFUSED:
        # beyond the LDS: _ok 0, no workspace, EPN_EINVAL, nothing written
        rng = np.random.default_rng(K.hash_name(c.name))
        anchors, kernels, xyz, new_xyz = K._geometry(c, rng)
        d = dict(xyz=xyz, new_xyz=new_xyz, idx=K._index_table(rng, c), anchors=anchors, kernels=kernels, sigma=c.sigma)
        dev = CloudDevice(gpu, c, d)
        if dev.ok != 0 or dev.need != 0:
            bad.append(f"{c.name}: _ok = {dev.ok}, _workspace_bytes = {dev.need}; the restatement refuses the shape")
        dG = np.ones((c.b * c.p2 * c.na, c.cin * c.ks), np.float32)
        for form in FORMS:
            out, name, count, b = dev.call(form, dG)
            bad += b
            if name or not bool((out == 7.0).all().item()) or not dev.wa.untouched():
                bad.append(f"{c.name} {form}: a refused call launched {name!r} or wrote to the output or the workspace")
    else:
        d = K.cloud_case(c)
        dev = CloudDevice(gpu, c, d)
        if dev.ok != 1 or dev.need <= K.workspace_extra_bytes(c):
            bad.append(f"{c.name}: _ok = {dev.ok}, _workspace_bytes = {dev.need}")
        for form in FORMS:
            _judge(dev, form, d["dG"], d["ref"], bad)
            _judge(dev, form, d["dG"], d["ref"], bad, add=d["add"])
            if form != "bf16_f32":
                _judge(dev, form, d["dG"], d["ref"], bad, add=d["add"], alias=True)
    DONE[c] = bad
    return bad


@pytest.mark.parametrize("c", K.CLOUD_CASES, ids=lambda c: c.name)
def test_cloud_exact(gpu, c):
    """dF of the dyadic case equals float64 by `==` in every form, inside guard bands, from the predicted instance, the range
    counter at 0; a shape beyond the LDS is refused."""
    _report(run_cloud(gpu, c))


def test_no_output_points(gpu):
    """p2 = 0: zeros, or add (a separate tensor is copied, the output itself is left as it is); nothing around is written."""
    c = K.by_name("nn17")
    d = dict(K.cloud_case(c))
    c0 = c._replace(name="p2_0", p2=0)
    d["new_xyz"], d["idx"] = np.zeros((c.b, 3, 1), np.float32), np.zeros((c.b, 1, c.nn), np.int32)      # (pointers that are not NULL)
    dev = CloudDevice(gpu, c0, d)
    assert K.cloud_ok(c0) and dev.ok == 1
    dG = np.ones((1, c.cin * c.ks), np.float32)
    zero = np.zeros_like(d["ref"])
    bad = []
    for form in FORMS:
        for add, alias in ((None, False), (d["add"], False), (d["add"], True)):
            out, name, _, b = dev.call(form, dG, add=add, alias=alias)
            bad += b
            bad += _compare(out.float(), K.expected(zero, add, form == "bf16").astype(np.float64), f"p2 = 0 {form} add {add is not None} alias {alias}")
    _report(bad)


# ------------------------------------------------------------------------------------------------ 2. maximum and scale
@pytest.mark.parametrize("name", K.SCALE_CASES)
def test_reported_maximum_and_scale_leave_the_bits(gpu, name):
    """The true max|dG|, NULL and 2^6 x the maximum: the same bits (the unit only has to be fine enough, and it is by 2^19 and
    more).  dG 2^-20 and dG 2^10: the result scaled, bit for bit."""
    c = K.by_name(name)
    d = K.cloud_case(c)
    dev = CloudDevice(gpu, c, d)
    bad = []
    top = float(np.abs(d["dG"]).max())
    for form in FORMS:
        base = _judge(dev, form, d["dG"], d["ref"], bad)
        for amax in (None, top * 64.0):
            out = _judge(dev, form, d["dG"], d["ref"], bad, amax=amax)
            if not torch.equal(out, base):
                bad.append(f"{name} {form}: dg_amax = {amax} changes {int((out != base).sum())} elements")
        for s in (2.0 ** -20, 2.0 ** 10):
            for amax in ("true", None):
                out = _judge(dev, form, d["dG"] * np.float32(s), d["ref"] * s, bad, amax=amax)
                if not torch.equal(out.float(), base.float() * s):
                    bad.append(f"{name} {form}: dF({s} dG) != {s} dF(dG), dg_amax {amax}")
    _report(bad)


def test_extreme_of_the_bound_inside_the_contract(gpu):
    """Multiplicity 64 x 32 coinciding kernel points x |dG| = amax just below a power of two: every contribution is 2^50 (1 - 2^-8)
    units.  Exact, and the range counter stays at 0 (call() checks it), with the true maximum and with the entry's own."""
    c, geo, dG, ref = K.extreme_case()
    dev = CloudDevice(gpu, c, dict(zip(("xyz", "new_xyz", "idx", "anchors", "kernels", "sigma"), geo)))
    bad = []
    for form in FORMS:
        for amax in ("true", None):
            _judge(dev, form, dG, ref, bad, amax=amax)
    _report(bad)


# ------------------------------------------------------------------------------------------------ 3. invariances
@pytest.mark.parametrize("name,nn2", K.INVARIANCE_CASES)
def test_slot_order_and_shadow_slots_are_bitwise_invisible(gpu, name, nn2):
    """Every row's slots in another order (cyclic rows stay cyclic), then shadow slots appended across an NT boundary: another
    instance, the same bits."""
    c = K.by_name(name)
    d = dict(K.cloud_case(c))
    base = CloudDevice(gpu, c, d)
    d1 = dict(d, idx=K.permute_slots(d["idx"], np.random.default_rng(5)))
    assert not np.array_equal(d1["idx"], d["idx"])
    perm = CloudDevice(gpu, c, d1)
    c2 = c._replace(name=f"{name}_to_{nn2}", nn=nn2)
    d2 = dict(d, idx=np.ascontiguousarray(np.concatenate([d["idx"], np.full((c.b, c.p2, nn2 - c.nn), c.p1, np.int32)], axis=2)))
    wide = CloudDevice(gpu, c2, d2)
    bad = []
    for form in FORMS:
        a = _judge(base, form, d["dG"], d["ref"], bad)
        b1 = _judge(perm, form, d["dG"], d["ref"], bad)
        b2 = _judge(wide, form, d["dG"], d["ref"], bad)
        if K.cloud_instance(c2, form != "f32") == K.cloud_instance(c, form != "f32"):
            bad.append(f"{name} {form}: nn = {nn2} does not change the instance")
        for other, what in ((b1, "a permutation of the neighbour slots"), (b2, f"shadow slots up to nn = {nn2}")):
            if not torch.equal(a, other):
                bad.append(f"{name} {form}: {int((a != other).sum())} elements change under {what}")
    _report(bad)


# ------------------------------------------------------------------------------------------------ 4. duplicates among kept slots
@pytest.mark.parametrize("side", ["below", "at"])
@pytest.mark.parametrize("kind", list(K.WRAP_ROWS))
def test_duplicate_rows_never_wrap_the_accumulator(gpu, kind, side):
    """Every row names one point in many of the slots the table kernel keeps -- "plain": [3, 5, 3, 3, ...], 63 slots on point 3
    without being cyclic; "period": ([1] + [2] * 31) * 2, cyclic and folded to 32 slots of multiplicity 2, 31 of them on point 2
    -- with w = 1 and dG = +amax, at p2 just below and at the point count where the slots of 2^50 (1 - 2^-8) units that the folded
    multiplicity alone would allow cross 2^63 (131 and 266).  The table kernel reports nn as the multiplicity of such a row
    (CHANGELOG), so that the sum of a destination stays below 2^62: the result is the float64 sum rounded once.  A loud NaN with
    the counter raised would also honour the contract; a wrapped value does not."""
    p2 = K.wrap_crossing(kind) - (1 if side == "below" else 0)
    c, geo, dG, ref = K.wrap_case(kind, p2)
    point = K.WRAP_ROWS[kind][1]
    dev = CloudDevice(gpu, c, dict(zip(("xyz", "new_xyz", "idx", "anchors", "kernels", "sigma"), geo)))
    bad = []
    for form in FORMS:
        for amax in ("true", None):
            out, name, count, b = dev.call(form, dG, amax=amax, silent=False)
            bad += b
            got = out.float().cpu().double().numpy().reshape(ref.shape)
            exp = K.expected(ref, None, form == "bf16").astype(np.float64)
            print(f"{c.name} {form} dg_amax {amax} [{name}]: dF[point {point}] = {got[0, point, 0, 0]!r}, float64 {ref[0, point, 0, 0]!r}, range counter {count}")
            if count > 0:
                if not (np.isnan(got).any() and np.array_equal(got[~np.isnan(got)], exp[~np.isnan(got)])):
                    bad.append(f"{c.name} {form}: range counter {count} without NaN rows")
            else:
                bad += _compare(out.float(), exp, f"{c.name} {form} dg_amax {amax} [{name}]")
    _report(bad)


# ------------------------------------------------------------------------------------------------ 5. real geometry
@pytest.mark.parametrize("entry", C.REAL_INTER, ids=lambda e: e[0])
def test_real_geometry_within_the_documented_arithmetic(gpu, entry):
    c, d, ref, S = K.real_cloud_reference(entry)
    dev = CloudDevice(gpu, c, d)
    bad = []
    for t, form in (("f32", "f32"), ("bf16", "bf16")):
        out, name, _, b = dev.call(form, d["dG"])
        bad += b
        if name != K.cloud_instance(c, form != "f32"):
            bad.append(f"{c.name} {form}: ran {name}, expected {K.cloud_instance(c, form != 'f32')}")
        got = out.float().cpu().double().numpy().reshape(ref.shape)
        ratio = float((np.abs(got - ref) / (2.0 ** -24 * S + 1e-300)).max())
        REAL_WORST[t] = max(REAL_WORST.get(t, 0.0), ratio)
        print(f"real geometry, {c.name} {form} [{name}]: worst |kernel - fp64| / (2^-24 S) = {ratio:.4f} (CLOUD_REAL_M = {K.CLOUD_REAL_M[t]})")
        if not ratio <= K.CLOUD_REAL_M[t]:
            bad.append(f"{c.name} {form} [{name}]: |kernel - fp64| reaches {ratio:.4f} x 2^-24 S, allowed {K.CLOUD_REAL_M[t]}")
    _report(bad)


# ------------------------------------------------------------------------------------------------ instance coverage (last)
def test_every_reachable_cloud_instance_was_run(gpu):
    """The union of the instances epn_last_kernel() named equals cloud_cases.REACHABLE_CLOUD.  (Cases deselected from the run are
    run now.)"""
    bad = []
    for c in K.CLOUD_CASES:
        bad += run_cloud(gpu, c)
    got = RECORDED - {""}
    assert got == K.REACHABLE_CLOUD, f"never ran {sorted(K.REACHABLE_CLOUD - got)}; ran but not listed {sorted(got - K.REACHABLE_CLOUD)}"
    _report(bad)
