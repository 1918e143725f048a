"""The PointNet head (csrc/pointnet.hip) through its plain C entries, held to EXACT results: values, arg-max indices and every
gradient equal the float64 restatement of tests/pointnet_ref.py by `==` on the cases of tests/pointnet_cases.py.

1. Exact tier: integer operands and dyadic geometry (any summation or atomic order gives the same floats).  Every output is a
   region of a sentinel-filled arena (tests/gemm_ref.py Arena) pre-filled with 7.0: nothing around it may change, the return code
   is 0 and epn_last_kernel() names the kernel the restated dispatch predicts.  The backward entries get the forward's own
   arg-max and synthetic routing tables.
2. Tie tier: exact copies of a point inside one MFMA lane group, across lane groups, 16-tiles, the 32- and 64-point tiles and the
   8-row unroll of the max kernel, and a cloud of identical points: the smaller index wins, in arg and in dF.
3. Special values: two NaNs, NaN after +inf, +inf twice, all -inf, +-0 ties.
4. Ops tier: ops.pointnet_so3conv in its GEMM-composed and its fused form, fp32 and bf16 features, equal to the restatement
   (hence to each other) bit for bit; the default dispatch on both sides of its thresholds.
5. Real-geometry tier: |kernel - fp64| <= REAL_M 2^-24 S element by element; REAL_M comes from the CPU
   (tests/test_pointnet_spec.py), never from a kernel."""
import ctypes

import numpy as np
import pytest
import torch

import gemm_ref as R
import pointnet_cases as C
import pointnet_ref as P

pytestmark = pytest.mark.gpu
F32, I32 = torch.float32, torch.int32
RECORDED = set()       # kernel names epn_last_kernel() reported during the exact cases
DONE = {}              # (entry, case) -> failures (each case runs once per session)


def _lib():
    from epn_pointcloud_amd import _lib
    return _lib, _lib.get_lib()


def _dev(a, gpu):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _report(bad):
    assert not bad, f"{len(bad)} failure(s):\n" + "\n".join(bad[:40])


def _compare(got, ref, what, signs=False):
    got = got.detach().cpu().double().numpy().reshape(ref.shape)
    if np.array_equal(got, ref, equal_nan=True) and (not signs or np.array_equal(np.signbit(got), np.signbit(ref))):
        return []
    d = np.abs(got - ref)
    ne = ~((got == ref) | (np.isnan(got) & np.isnan(ref)))
    return [f"{what}: {int(ne.sum())} of {d.size} elements differ (NaN: {int(np.isnan(got).sum())}), max |diff| "
            f"{np.nanmax(np.where(ne, d, 0)):g}, first at {tuple(int(i) for i in np.argwhere(ne)[0]) if ne.any() else 'a zero sign'}: "
            f"got {got[ne][:1]}, expected {ref[ne][:1]}"]


class Call:
    """One call of an entry: float32 outputs as regions of one arena pre-filled with 7.0, the int32 arg-max in another."""

    def __init__(self, gpu, what, shapes, int_shape=None):
        self.what, self.bad = what, []
        self.arena = R.Arena(F32, gpu, [(r, c, None, 0, 0) for r, c in shapes])
        for t in self.arena.t:
            t.fill_(7.0)
        self.t = self.arena.t
        self.iarena = self.arg = None
        if int_shape is not None:
            self.iarena, self.arg = R.guarded(*int_shape, I32, gpu)
            self.arg.fill_(7)

    def run(self, entry, *args, want_rc=0, kernel=None, record=True):
        _l, lib = _lib()
        lib.epn_last_kernel()
        rc = getattr(lib, entry)(*args, _l.stream_of(self.arena.flat))
        torch.cuda.synchronize()
        name = C.normalise(lib.epn_last_kernel())
        if rc != want_rc:
            self.bad.append(f"{self.what}: {entry} returned {rc} ({lib.epn_strerror(rc).decode()}), expected {want_rc}")
        if kernel is not None:
            if record and name:
                RECORDED.add(name)
            if name != kernel:
                self.bad.append(f"{self.what}: ran '{name}', the restated dispatch says '{kernel}'")
        for a in (self.arena, self.iarena):
            if a is not None:
                try:
                    a.check(f"{self.what} [{name}]")
                except AssertionError as e:
                    self.bad.append(str(e))
        return self

    def untouched(self, *tensors):
        for t in tensors:
            if not bool((t == 7).all().item()):
                self.bad.append(f"{self.what}: an output that must not be written was written")


def _inputs(gpu, d):
    return {k: _dev(d[k], gpu) for k in ("F", "xyz", "anchors", "W", "bias", "gout", "arg")}


def call_fwd(gpu, c, t, what, record=True, b=None):
    b = c.b if b is None else b
    k = Call(gpu, what, [(c.b * c.a, c.co), (c.b, 3)], (c.b * c.a, c.co))
    k.run("epn_pointnet_so3conv_fwd_f32", _ptr(t["F"]), _ptr(t["xyz"]), _ptr(t["anchors"]), _ptr(t["W"]), _ptr(t["bias"]),
          _ptr(k.t[0]), _ptr(k.arg), _ptr(k.t[1]), b, c.p, c.a, c.c, c.co, kernel=C.fwd_kernel(c.c) if b else "", record=record)
    return k


def call_max(gpu, c, t, Z, what, record=True, b=None):
    b = c.b if b is None else b
    k = Call(gpu, what, [(c.b * c.a, c.co), (c.b, 3)], (c.b * c.a, c.co))
    k.run("epn_pointnet_max_f32", _ptr(Z), _ptr(t["xyz"]), _ptr(t["anchors"]), _ptr(t["W"]), _ptr(t["bias"]), _ptr(k.t[0]),
          _ptr(k.arg), _ptr(k.t[1]), b, c.p, c.a, c.c, c.co, kernel=C.KERNEL["max"] if b else "", record=record)
    return k


def call_bwd_data(gpu, c, t, what, arg=None, record=True, b=None):
    b = c.b if b is None else b
    k = Call(gpu, what, [(c.b * c.p * c.a, c.c)])
    k.run("epn_pointnet_so3conv_bwd_data_f32", _ptr(t["gout"]), _ptr(t["arg"] if arg is None else arg), _ptr(t["W"]), _ptr(k.t[0]),
          b, c.p, c.a, c.c, c.co, kernel=C.KERNEL["bwd_data"] if b else "", record=record)
    return k


def call_bwd_weight(gpu, c, t, centre, what, arg=None, record=True, b=None, bias=True):
    b = c.b if b is None else b
    k = Call(gpu, what, [(c.co, c.c + 3), (1, c.co)])
    k.run("epn_pointnet_so3conv_bwd_weight_f32", _ptr(t["gout"]), _ptr(t["arg"] if arg is None else arg), _ptr(t["F"]), _ptr(t["xyz"]),
          _ptr(t["anchors"]), _ptr(centre), _ptr(k.t[0]), _ptr(k.t[1] if bias else None), b, c.p, c.a, c.c, c.co,
          kernel=C.KERNEL["bwd_weight"] if b else "", record=record)
    return k


def call_bwd_coord(gpu, c, t, centre, what, record=True, b=None, bias=True):
    b = c.b if b is None else b
    k = Call(gpu, what, [(c.co, c.c + 3), (1, c.co)])
    k.run("epn_pointnet_bwd_coord_f32", _ptr(t["gout"]), _ptr(t["arg"]), _ptr(t["xyz"]), _ptr(t["anchors"]), _ptr(centre),
          _ptr(k.t[0]), _ptr(k.t[1] if bias else None), b, c.p, c.a, c.c, c.co, kernel=C.KERNEL["bwd_coord"], record=record)
    return k


# ------------------------------------------------------------------------------------------------ 1. / 2. exact and tie tiers
def run_fused(gpu, c):
    """Forward, then both fused gradients through the restatement's arg-max (which the forward's must equal)."""
    if ("fused", c) not in DONE:
        d = C.case(c)
        r, t = d["ref"], _inputs(gpu, d)
        k = call_fwd(gpu, c, t, f"{c.name} fwd")
        bad = k.bad + _compare(k.t[0], r["out"], f"{c.name} out") + _compare(k.arg, r["arg_fwd"].astype(np.float64), f"{c.name} arg")
        bad += _compare(k.t[1], r["centre"], f"{c.name} centre")
        ctr = k.t[1].clone() if not bad else _dev(r["centre"].astype(np.float32), gpu)
        # the gradients through the KERNEL's arg-max tensor where it is right (the restatement's otherwise: one report per bug)
        arg = k.arg.clone() if not bad else t["arg"]
        g = call_bwd_data(gpu, c, t, f"{c.name} bwd_data", arg)
        bad += g.bad + _compare(g.t[0], r["dF"], f"{c.name} dF")
        w = call_bwd_weight(gpu, c, t, ctr, f"{c.name} bwd_weight", arg, bias=c.bias)
        if not c.bias:
            w.untouched(w.t[1])
        bad += w.bad + _compare(w.t[0], r["dW"], f"{c.name} dW")
        if c.bias:
            bad += _compare(w.t[1], r["dbias"], f"{c.name} dbias")
        DONE[("fused", c)] = bad
    return DONE[("fused", c)]


def run_max(gpu, c):
    if ("max", c) not in DONE:
        d = C.case(c)
        r, t = d["ref"], _inputs(gpu, d)
        out, arg, ctr = P.max_of(r["Z"], d["xyz"], d["anchors"], d["W"], d["bias"], c.c)
        assert np.array_equal(out, r["out"]) and np.array_equal(arg, r["arg_fwd"])
        k = call_max(gpu, c, t, _dev(r["Z"].astype(np.float32), gpu), f"{c.name} max")
        DONE[("max", c)] = (k.bad + _compare(k.t[0], out, f"{c.name} max out") + _compare(k.arg, arg.astype(np.float64), f"{c.name} max arg")
                            + _compare(k.t[1], ctr, f"{c.name} max centre"))
    return DONE[("max", c)]


def run_bwd_data(gpu, c):
    if ("bwd_data", c) not in DONE:
        d = C.case(c)
        k = call_bwd_data(gpu, c, _inputs(gpu, d), f"{c.name} (routing {c.routing})")
        DONE[("bwd_data", c)] = k.bad + _compare(k.t[0], d["ref"]["dF"], f"{c.name} dF")
    return DONE[("bwd_data", c)]


def run_bwd_weight(gpu, c):
    if ("bwd_weight", c) not in DONE:
        d = C.case(c)
        r = d["ref"]
        k = call_bwd_weight(gpu, c, _inputs(gpu, d), _dev(r["centre"].astype(np.float32), gpu), f"{c.name} (routing {c.routing})",
                            bias=c.bias)
        if not c.bias:
            k.untouched(k.t[1])
        bad = k.bad + _compare(k.t[0], r["dW"], f"{c.name} dW")
        if c.bias:
            bad += _compare(k.t[1], r["dbias"], f"{c.name} dbias")
        DONE[("bwd_weight", c)] = bad
    return DONE[("bwd_weight", c)]


def run_bwd_coord(gpu, c):
    if ("bwd_coord", c) not in DONE:
        d = C.case(c)
        r = d["ref"]
        k = call_bwd_coord(gpu, c, _inputs(gpu, d), _dev(r["centre"].astype(np.float32), gpu), f"{c.name}", bias=c.bias)
        k.untouched(k.t[0][:, :c.c], *(() if c.bias else (k.t[1],)))          # the GEMM's columns keep their 7.0
        bad = k.bad + _compare(k.t[0][:, c.c:], r["dW"][:, c.c:], f"{c.name} dW[:, c:]")
        if c.bias:
            bad += _compare(k.t[1], r["dbias"], f"{c.name} dbias")
        DONE[("bwd_coord", c)] = bad
    return DONE[("bwd_coord", c)]


def run_dz(gpu, c):
    if ("dz", c) not in DONE:
        d = C.build_dz(c)
        g, arg = _dev(d["gout"], gpu), _dev(d["arg"], gpu)
        rows = c.b * c.p * c.a
        k = Call(gpu, f"{c.name} f32", [(rows, c.co)])
        k.run("epn_pointnet_dz_f32", _ptr(g), _ptr(arg), _ptr(k.t[0]), c.b, c.p, c.a, c.co, kernel=C.KERNEL["dz_f32"])
        bad = k.bad + _compare(k.t[0], d["f32"], f"{c.name} dZ f32")
        arena, dz = R.guarded(rows, c.co, torch.bfloat16, gpu)
        dz.fill_(7.0)
        _l, lib = _lib()
        lib.epn_last_kernel()
        rc = lib.epn_pointnet_dz_bf16(_ptr(g), _ptr(arg), _ptr(dz), c.b, c.p, c.a, c.co, _l.stream_of(dz))
        torch.cuda.synchronize()
        name = C.normalise(lib.epn_last_kernel())
        RECORDED.add(name)
        if rc != 0 or name != C.KERNEL["dz_bf16"]:
            bad.append(f"{c.name} bf16: rc {rc}, ran '{name}'")
        try:
            arena.check(f"{c.name} dZ bf16")
        except AssertionError as e:
            bad.append(str(e))
        bad += _compare(dz.float(), d["bf16"], f"{c.name} dZ bf16 (round to nearest even, bit for bit)")
        DONE[("dz", c)] = bad
    return DONE[("dz", c)]


_id = lambda c: c.name


@pytest.mark.parametrize("c", C.FWD_CASES, ids=_id)
def test_fused_forward_and_gradients_exact(gpu, c):
    """out, arg, centre, dF, dW, dbias equal float64 by `==`, inside guard bands, from the predicted kernel."""
    _report(run_fused(gpu, c))


@pytest.mark.parametrize("c", C.TIE_CASES, ids=_id)
def test_ties_go_to_the_first_point(gpu, c):
    """Exact copies of a point: the fused forward kernel of the case's width, and the max kernel fed the exact Z, name the smaller
    index; dF through that arg-max equals the restatement."""
    _report(run_fused(gpu, c) + run_max(gpu, c))


@pytest.mark.parametrize("c", C.MAX_CASES, ids=_id)
def test_max_kernel_exact(gpu, c):
    _report(run_max(gpu, c))


@pytest.mark.parametrize("c", C.BWD_DATA_CASES, ids=_id)
def test_bwd_data_exact(gpu, c):
    _report(run_bwd_data(gpu, c))


@pytest.mark.parametrize("c", C.BWD_WEIGHT_CASES, ids=_id)
def test_bwd_weight_exact(gpu, c):
    _report(run_bwd_weight(gpu, c))


@pytest.mark.parametrize("c", C.BWD_COORD_CASES, ids=_id)
def test_bwd_coord_exact(gpu, c):
    """The three coordinate columns and dbias; the first c columns of dW belong to a GEMM and keep their 7.0."""
    _report(run_bwd_coord(gpu, c))


@pytest.mark.parametrize("c", C.DZ_CASES, ids=_id)
def test_dz_exact(gpu, c):
    """fp32: a copy or a zero; bf16: round to nearest even, bit for bit against gemm_ref.bf16_rne."""
    _report(run_dz(gpu, c))


def test_dz_refuses_misaligned_pointers_and_odd_widths(gpu):
    _l, lib = _lib()
    c = C.DZ_CASES[0]
    rows = c.b * c.p * c.a
    g = torch.zeros(rows * c.co + 8, device=gpu)
    arg = torch.zeros(rows * c.co + 8, dtype=I32, device=gpu)
    bad = []
    for entry, dt in (("epn_pointnet_dz_f32", F32), ("epn_pointnet_dz_bf16", torch.bfloat16)):
        arena, dz = R.guarded(rows + 1, c.co, dt, gpu)
        off = lambda t, n: ctypes.c_void_p(t.data_ptr() + 4 * n)
        for what, args in (("grad_out + 4 bytes", (off(g, 1), _ptr(arg), _ptr(dz), c.b, c.p, c.a, c.co)),
                           ("argmax + 4 bytes", (_ptr(g), off(arg, 1), _ptr(dz), c.b, c.p, c.a, c.co)),
                           ("dZ + 4 bytes", (_ptr(g), _ptr(arg), off(dz, 1), c.b, c.p, c.a, c.co)),
                           ("co = 12", (_ptr(g), _ptr(arg), _ptr(dz), c.b, c.p, c.a, 12)),
                           ("co = 4", (_ptr(g), _ptr(arg), _ptr(dz), c.b, c.p, c.a, 4))):
            rc = getattr(lib, entry)(*args, _l.stream_of(dz))
            torch.cuda.synchronize()
            if rc != C.EPN_EINVAL:
                bad.append(f"{entry}, {what}: returned {rc}, expected EPN_EINVAL")
            if not arena.untouched():
                bad.append(f"{entry}, {what}: the refused call wrote")
    _report(bad)


def test_empty_batch(gpu):
    """b = 0: every entry returns 0 and writes nothing; the weight gradient zero-fills dW and dbias, the coordinate gradient
    writes zeros into its three columns and dbias."""
    c = C.PnCase("empty", 1, **C.EMPTY_SHAPE)
    d = C.case(c)
    t = _inputs(gpu, d)
    ctr = _dev(d["ref"]["centre"].astype(np.float32), gpu)
    bad = []
    k = call_fwd(gpu, c, t, "fwd, b = 0", record=False, b=0)
    k.untouched(*k.t, k.arg)
    bad += k.bad
    k = call_max(gpu, c, t, _dev(d["ref"]["Z"].astype(np.float32), gpu), "max, b = 0", record=False, b=0)
    k.untouched(*k.t, k.arg)
    bad += k.bad
    k = call_bwd_data(gpu, c, t, "bwd_data, b = 0", record=False, b=0)
    k.untouched(*k.t)
    bad += k.bad
    k = call_bwd_weight(gpu, c, t, ctr, "bwd_weight, b = 0", record=False, b=0)
    bad += k.bad + _compare(k.t[0], np.zeros((c.co, c.c + 3)), "bwd_weight, b = 0: dW") + _compare(k.t[1], np.zeros((1, c.co)), "dbias")
    k = call_bwd_coord(gpu, c, t, ctr, "bwd_coord, b = 0", record=False, b=0)
    k.untouched(k.t[0][:, :c.c])
    bad += k.bad + _compare(k.t[0][:, c.c:], np.zeros((c.co, 3)), "bwd_coord, b = 0: dW[:, c:]") + _compare(k.t[1], np.zeros((1, c.co)), "dbias")
    # ... and with every data pointer NULL, as a caller with an empty batch has them
    _l, lib = _lib()
    z = ctypes.c_void_p(0)
    k = Call(gpu, "bwd_coord, b = 0, NULL inputs", [(c.co, c.c + 3), (1, c.co)])
    k.run("epn_pointnet_bwd_coord_f32", z, z, z, z, z, _ptr(k.t[0]), _ptr(k.t[1]), 0, c.p, c.a, c.c, c.co)
    bad += k.bad + _compare(k.t[0][:, c.c:], np.zeros((c.co, 3)), "bwd_coord, NULL inputs: dW[:, c:]")
    for entry in ("epn_pointnet_dz_f32", "epn_pointnet_dz_bf16"):
        k = Call(gpu, f"{entry}, b = 0", [(8, c.co)])
        k.run(entry, _ptr(t["gout"]), _ptr(t["arg"]), _ptr(k.t[0]), 0, c.p, c.a, c.co)
        k.untouched(*k.t)
        bad += k.bad
    _report(bad)


# ------------------------------------------------------------------------------------------------ 3. special values
@pytest.mark.parametrize("c", [C.TIE_CASES[0], C.TIE_CASES[6]], ids=_id)
def test_two_nan_features_first_one_wins(gpu, c):
    """NaN features at two points of one (cloud, anchor) row, placed as the tie pairs: that whole row of `out` is NaN and its
    arg-max the FIRST NaN's point; every other row is bit-identical to the clean run."""
    d = C.case(c)
    t = _inputs(gpu, d)
    clean = call_fwd(gpu, c, t, f"{c.name} clean", record=False)
    bad = list(clean.bad)
    for pair in C.SPECIAL_PAIRS:
        F, (bb, ai) = C.nan_features(c, pair)
        k = call_fwd(gpu, c, dict(t, F=_dev(F, gpu)), f"{c.name} NaN at {pair}", record=False)
        bad += k.bad
        row = bb * c.a + ai
        out, arg = k.t[0].cpu().numpy(), k.arg.cpu().numpy()
        if not np.isnan(out[row]).all():
            bad.append(f"{c.name} NaN at {pair}: {int((~np.isnan(out[row])).sum())} of {c.co} outputs of the row are not NaN")
        if not np.all(arg[row] == pair[0]):
            bad.append(f"{c.name} NaN at {pair}: arg-max {sorted(set(arg[row].tolist()))}, expected the first NaN's point {pair[0]}")
        keep = np.arange(c.b * c.a) != row
        if not (np.array_equal(out[keep].view(np.int32), clean.t[0].cpu().numpy()[keep].view(np.int32))
                and np.array_equal(arg[keep], clean.arg.cpu().numpy()[keep])):
            bad.append(f"{c.name} NaN at {pair}: rows without a NaN changed")
    _report(bad)


@pytest.mark.parametrize("pattern", list(C.SPECIAL_PATTERNS) + ["all_neg_inf"])
def test_max_kernel_special_values(gpu, pattern):
    """Z written directly (zero coordinate weights, no bias): the restatement, which tests/test_pointnet_spec.py holds to torch.max."""
    co = 8
    c = C.PnCase("special", 1, C.TIE_P, 1, 16, co, False)
    W = torch.zeros(co, c.c + 3, device=gpu)
    xyz = _dev(C.case(C.PnCase("special_xyz", 1, C.TIE_P, 1, 16, co, False))["xyz"], gpu)
    t = dict(xyz=xyz, anchors=None, W=W, bias=None)
    bad = []
    for pair in C.SPECIAL_PAIRS:
        Z = C.special_Z(pattern, pair, co)
        out, arg = P.max_first(Z.astype(np.float64) + 0.0, axis=1)               # + 0.0: the kernel adds its zero bias
        k = call_max(gpu, c, t, _dev(Z, gpu), f"{pattern} at {pair}", record=False)
        bad += k.bad + _compare(k.t[0], out, f"{pattern} at {pair}: out", signs=True)
        bad += _compare(k.arg, arg.astype(np.float64), f"{pattern} at {pair}: arg")
    _report(bad)


# ------------------------------------------------------------------------------------------------ 4. ops tier
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("form", ["gemm", "fused"])
@pytest.mark.parametrize("c", C.OPS_CASES, ids=_id)
def test_ops_forms_equal_the_restatement(gpu, monkeypatch, c, form, dtype):
    """ops.pointnet_so3conv in the GEMM-composed and in the fused form, fp32 and bf16 features (the integer operands are
    bf16 values): y, dF, dW, dB equal the restatement by `==` -- so the two forms agree bit for bit."""
    from epn_pointcloud_amd import ops
    monkeypatch.setenv("EPN_POINTNET", form)
    d = C.case(c)
    r = d["ref"]
    dt = torch.bfloat16 if dtype == "bf16" else F32
    assert np.array_equal(R.bf16_rne(d["F"]), d["F"]) and np.abs(r["dF"]).max() <= 256
    feats = _dev(d["F"], gpu).to(dt).permute(0, 3, 1, 2).requires_grad_(True)        # [b, c, p, a], channels-last memory
    W = _dev(d["W"], gpu).reshape(c.co, c.c + 3, 1, 1).requires_grad_(True)
    bias = _dev(d["bias"], gpu).requires_grad_(True) if c.bias else None
    spy = []
    for cls in (ops.PointnetSO3ConvGemmFn, ops.PointnetSO3ConvFn):
        real = cls.apply
        monkeypatch.setattr(cls, "apply", staticmethod(lambda *a, _r=real, _n=cls.__name__: (spy.append(_n), _r(*a))[1]))
    y = ops.pointnet_so3conv(feats, _dev(d["xyz"], gpu), _dev(d["anchors"], gpu), W, bias)
    assert spy == ["PointnetSO3ConvGemmFn" if form == "gemm" else "PointnetSO3ConvFn"], spy
    y.backward(_dev(d["gout"], gpu).permute(0, 2, 1))
    torch.cuda.synchronize()
    bad = _compare(y.permute(0, 2, 1), r["out"], f"{c.name} {form} {dtype} y")
    bad += _compare(feats.grad.permute(0, 2, 3, 1), r["dF"], f"{c.name} {form} {dtype} dF")
    bad += _compare(W.grad.reshape(c.co, c.c + 3), r["dW"], f"{c.name} {form} {dtype} dW")
    if c.bias:
        bad += _compare(bias.grad, r["dbias"], f"{c.name} {form} {dtype} dB")
    assert feats.grad.dtype == dt and y.dtype == F32
    _report(bad)


@pytest.mark.parametrize("b,c,p,a,co,want", [(1, 16, 16383, 1, 8, "fused"), (1, 16, 16384, 1, 8, "gemm"), (2, 16, 8192, 1, 8, "gemm"),
                                             (1, 24, 16384, 1, 8, "fused"), (1, 16, 16384, 1, 12, "fused"),
                                             (1, 32, 2048, 8, 16, "gemm"), (1, 32, 2047, 8, 16, "fused")])
def test_default_dispatch_thresholds(gpu, monkeypatch, b, c, p, a, co, want):
    """No A/B switch set: the GEMM-composed form from 16384 feature rows with c % 16 == 0 and co % 8 == 0, the fused one otherwise."""
    from epn_pointcloud_amd import ops
    monkeypatch.delenv("EPN_POINTNET", raising=False)
    spy = []
    monkeypatch.setattr(ops.PointnetSO3ConvGemmFn, "apply", staticmethod(lambda *args: spy.append("gemm")))
    monkeypatch.setattr(ops.PointnetSO3ConvFn, "apply", staticmethod(lambda *args: spy.append("fused")))
    for dt in (F32, torch.bfloat16):
        feats = torch.zeros(b, p, a, c, device=gpu, dtype=dt).permute(0, 3, 1, 2)
        ops.pointnet_so3conv(feats, torch.zeros(b, 3, p, device=gpu), torch.zeros(a, 3, 3, device=gpu),
                             torch.zeros(co, c + 3, 1, 1, device=gpu), None)
    assert spy == [want, want], (spy, want)


# ------------------------------------------------------------------------------------------------ 5. real geometry
@pytest.mark.parametrize("shape", C.REAL_SHAPES, ids=lambda s: "b{}_c{}_co{}_p{}_a{}".format(*s))
def test_real_geometry_within_the_oracles_error(gpu, shape):
    """|out - fp64| <= REAL_M 2^-24 S element by element (S: the column's largest per-point sum of absolute terms); the arg-max
    may differ from float64's only where the float64 value at the kernel's point is within that bound of the float64 maximum,
    and in at most 1 column of 1000; the gradients against the restatement through the kernel's own arg-max and centre."""
    b, cc, co, p, a = shape
    c = C.PnCase("real", b, p, a, cc, co)
    d = C.real_case(shape)
    t = {k: _dev(d[k], gpu) for k in ("F", "xyz", "anchors", "W", "bias", "gout")}
    eps, bad, worst = 2.0 ** -24, [], {}

    def hold(what, got, ref, S):
        got = got.cpu().double().numpy().reshape(ref.shape)
        ratio = float((np.abs(got - ref) / (eps * np.where(S > 0, S, 1.0))).max())
        worst[what] = ratio
        if not (ratio <= C.REAL_M and np.all((got == ref) | (S > 0))):
            bad.append(f"{what}: |kernel - fp64| reaches {ratio:.4f} x 2^-24 S, allowed {C.REAL_M}")

    k = call_fwd(gpu, c, t, f"real {shape} fwd", record=False)
    bad += k.bad
    arg = k.arg.cpu().numpy().reshape(b, a, co)
    if arg.min() < 0 or arg.max() >= p:
        _report(bad + [f"arg-max out of range: {arg.min()} .. {arg.max()}"])
    S = P.magnitudes(d["F"], d["xyz"], d["anchors"], d["W"], d["bias"], d["gout"], arg)
    hold("out", k.t[0], d["out64"], S["out"])
    differ = arg != d["arg64"]
    at_kernel = np.take_along_axis(d["z64"], arg[:, None].astype(np.int64), axis=1)[:, 0]
    if not np.all(d["out64"] - at_kernel <= C.REAL_M * eps * S["out"]):
        bad.append(f"arg-max: {int((d['out64'] - at_kernel > C.REAL_M * eps * S['out']).sum())} columns name a point whose float64 value "
                   "is below the float64 maximum by more than the bound")
    if differ.mean() > 1e-3:
        bad.append(f"arg-max: {int(differ.sum())} of {differ.size} columns differ from float64 (allowed: 1 in 1000)")
    ctr = k.t[1].clone()
    hold("centre", ctr, P.centre_of(d["xyz"]), np.abs(d["xyz"].astype(np.float64)).mean(axis=2))
    t["arg"] = k.arg.clone()
    g = call_bwd_data(gpu, c, t, f"real {shape} bwd_data", record=False)
    bad += g.bad
    hold("dF", g.t[0], P.bwd_data(d["gout"], arg, d["W"], p), S["dF"])
    w = call_bwd_weight(gpu, c, t, ctr, f"real {shape} bwd_weight", record=False)
    bad += w.bad
    dW, db = P.bwd_weight(d["gout"], arg, d["F"], d["xyz"], d["anchors"], ctr.cpu().double().numpy())
    hold("dW", w.t[0], dW, S["dW"])
    hold("dbias", w.t[1], db, S["dbias"])
    print(f"real geometry {shape} [{C.fwd_kernel(cc)}]: worst |kernel - fp64| / (2^-24 S) per pass: "
          + ", ".join(f"{n} {v:.4f}" for n, v in worst.items()) + f"; arg-max differs in {int(differ.sum())} of {differ.size} columns "
          f"(REAL_M = {C.REAL_M})")
    _report(bad)


# ------------------------------------------------------------------------------------------------ kernel coverage (last)
def test_every_kernel_of_the_head_was_run(gpu):
    """The union of the names epn_last_kernel() reported during the exact cases equals pointnet_cases.REACHABLE_POINTNET: every
    kernel of the head section of pointnet.hip, no other.  (Cases deselected from the run are run now.)"""
    bad = []
    for c in C.FWD_CASES + C.TIE_CASES:
        bad += run_fused(gpu, c)
    for c in C.TIE_CASES + C.MAX_CASES:
        bad += run_max(gpu, c)
    for table, run in ((C.BWD_DATA_CASES, run_bwd_data), (C.BWD_WEIGHT_CASES, run_bwd_weight), (C.BWD_COORD_CASES, run_bwd_coord),
                       (C.DZ_CASES, run_dz)):
        for c in table:
            bad += run(gpu, c)
    assert RECORDED == C.REACHABLE_POINTNET, (f"never ran {sorted(C.REACHABLE_POINTNET - RECORDED)}; ran but not listed "
                                              f"{sorted(RECORDED - C.REACHABLE_POINTNET)}")
    _report(bad)
