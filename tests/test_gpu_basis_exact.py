"""-m gpu: csrc/so3_basis.hip -- the change of anchor basis in its three arithmetic families (fp32 MFMA, three bf16 planes for
fp32 storage, hi + lo bf16 for bf16 storage), each in its 32-bit and its 64-bit addressed form, with the optional norm on load,
per-point statistics, backward partials of the norm and producer-side maximum, and the three spectral-weight kernels -- through
the plain C entries, held to EXACT results (tests/basis_ref.py restates everything in float64, tests/basis_cases.py holds the
cases and the restated dispatch, tests/test_basis_spec.py proves the exactness arguments without a device).

Every call: inputs, outputs, statistics and the maximum live in sentinel-filled arenas (gemm_ref.Arena) whose guard bands are
checked afterwards -- the 32-bit forms rely on the buffer bounds check to drop the stores of rows >= na and of lanes without
channels, and the guards are what sees a store that was not dropped; outputs are pre-filled with 7.0; epn_last_kernel() must name
the instance the restated dispatch predicts, and the last test compares the union with basis_cases.REACHABLE.

Tiers.  1. exact transform: sets P, I, S, X of basis_cases at the smallest shapes that reach each edge, `==`.  The 64-bit forms
are reached with na c 4 >= 2^24 (50 MB), not with 2 GiB tensors.  2. extras: statistics and maximum with `==`; norm on load
against the unfolded route (the glue's forward entry, then the plain entry) with `==`; the norm's backward partials: dy and sum d
with `==`, sum d xhat within a counted number of roundings (basis_cases.dstats_ref).  3. real data: the shipped U / U^T on normal inputs, |kernel - fp64| <= 2
m_family 2^-24 S element by element, m_family measured on the emulations (never on the kernels)."""
import numpy as np
import pytest
import torch

import basis_cases as C
import basis_ref as B
import gemm_ref as R

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
TDT = {"f32": torch.float32, "x3": torch.float32, "bf16": torch.bfloat16}
SUFFIX = {"f32": "f32", "x3": "split_f32", "bf16": "bf16"}
RECORDED = set()
REAL_WORST = {}


def _lib():
    from epn_pointcloud_amd import _lib
    return _lib, _lib.get_lib()


def _report(bad):
    assert not bad, f"{len(bad)} failure(s):\n" + "\n".join(bad[:40])


def _np(t):
    return t.detach().float().cpu().numpy()


def _dev(a, gpu, dtype=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu).to(dtype).contiguous()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _filled(n, dtype, gpu, value=None, fill=7.0):
    """A region of n elements in an arena of its own, holding `value` (a flat array) or the pre-fill."""
    arena, t = R.guarded(1, n, dtype, gpu)
    if value is None:
        t.fill_(fill)
    else:
        t.copy_(torch.from_numpy(np.ascontiguousarray(value)).reshape(1, n).to(gpu).to(dtype))
    return arena, t


def _compare(got, ref, what):
    ref = np.asarray(ref, F64)
    got = np.asarray(got, F64).reshape(ref.shape)
    if np.array_equal(got, ref):
        return []
    d = np.abs(got - ref)
    return [f"{what}: {int((~(d == 0)).sum())} of {d.size} elements differ (NaN: {int(np.isnan(got).sum())}), max |diff| "
            f"{np.nanmax(d):g}, first at {tuple(int(i) for i in np.argwhere(~(d == 0))[0])}"]


def basis_call(gpu, family, s, M, x, mode="plain", frozen=False, norm=None, x_cl=None, expect_rc=0, index=None):
    """One call of the `mode` entry of `family` on logical x [pts][na][c].  norm: dict(sums | stats, groups, ppg, gamma, beta, eps,
    slope).  -> dict(out f32[pts][na][c] logical, stats f32[pts][c][2] | None, amax float32 | None, bad, arenas)."""
    _l, lib = _lib()
    dt, n, bad = TDT[family], s.pts * s.na * s.c, []
    blk = C.blocks(s.na)
    iidx = index[0] if index else B.layout_index(s.in_spec, blk, s.pts, s.c)
    oidx = index[1] if index else B.layout_index(s.out_spec, blk, s.pts, s.c)
    ain, tin = _filled(n, dt, gpu, B.to_flat(np.asarray(x, F32), iidx))
    aout, tout = _filled(n, dt, gpu)
    arenas = [(ain, "input"), (aout, "output")]
    dM, dblk = _dev(M, gpu), torch.from_numpy(blk).to(gpu)
    head = (tin.data_ptr(), dM.data_ptr(), dblk.data_ptr(), s.pts, s.na, s.c)
    st = _l.stream_of(tout)
    tstats = tamax = None
    if mode in ("stats", "dstats"):
        a, tstats = _filled(s.pts * s.c * 2, torch.float32, gpu)
        arenas.append((a, "point statistics"))
    if mode in ("amax", "norm_amax"):
        a, tamax = _filled(1, torch.float32, gpu)
        arenas.append((a, "amax"))
    keep = []
    if norm is not None:
        keep = [_dev(norm.get("sums", norm.get("stats")), gpu), _dev(norm.get("gamma"), gpu), _dev(norm.get("beta"), gpu)]
        ntail = ((_ptr(keep[0]),) + (() if frozen else (norm["groups"], norm["ppg"])) + (_ptr(keep[1]), _ptr(keep[2]), norm["eps"], norm["slope"]))
    lib.epn_last_kernel()
    sfx = SUFFIX[family]
    if mode == "plain":
        rc = getattr(lib, "epn_so3_basis_" + sfx)(*head, s.in_spec, s.out_spec, tout.data_ptr(), st)
    elif mode == "stats":
        rc = getattr(lib, "epn_so3_basis_stats_" + sfx)(*head, s.in_spec, s.out_spec, tout.data_ptr(), tstats.data_ptr(), st)
    elif mode == "amax":
        rc = lib.epn_so3_basis_amax_split_f32(*head, s.in_spec, s.out_spec, tout.data_ptr(), tamax.data_ptr(), st)
    elif mode == "norm":
        rc = getattr(lib, "epn_so3_basis_norm_" + ("frozen_" if frozen else "") + sfx)(*head, s.out_spec, tout.data_ptr(), *ntail, st)
    elif mode == "norm_amax":
        rc = lib.epn_so3_basis_norm_amax_split_f32(*head, s.out_spec, tout.data_ptr(), *ntail, tamax.data_ptr(), st)
    else:
        assert mode == "dstats"
        ax, tx = _filled(n, dt, gpu, B.to_flat(np.asarray(x_cl, F32), B.plain_index(s.pts, s.na, s.c)))
        arenas.append((ax, "x_cl"))
        rc = getattr(lib, "epn_so3_basis_dstats_" + sfx)(*head, tout.data_ptr(), tx.data_ptr(), *ntail, tstats.data_ptr(), st)
    torch.cuda.synchronize()
    name = C.normalise(lib.epn_last_kernel())
    what = f"{family} {mode}{' frozen' if frozen else ''} {C.sid(s)} [{name}]"
    if rc != expect_rc:
        bad.append(f"{what}: the entry returned {rc}, expected {expect_rc}")
    if expect_rc == 0:
        RECORDED.add(name)
        want = C.instance(family, s.na, s.c, s.pts, frozen)
        if name != want:
            bad.append(f"{what}: the restated dispatch says {want}")
    elif name:
        bad.append(f"{what}: a refused call launched a kernel")
    for a, w in arenas:
        try:
            a.check(f"{what} {w}")
        except AssertionError as e:
            bad.append(str(e))
    return dict(out=B.from_flat(_np(tout), oidx), stats=None if tstats is None else _np(tstats).reshape(s.pts, s.c, 2),
                amax=None if tamax is None else _np(tamax).reshape(-1)[0], bad=bad, what=what, tout=tout, arenas=arenas)


# ------------------------------------------------------------------------------------------------ 1. the transform
@pytest.mark.parametrize("s", C.TRANSFORM_SHAPES, ids=C.sid)
def test_transform_exact(gpu, s):
    """Sets P, I, S (and X for the split form) in all three families: the stored output equals float64 by `==`."""
    bad = []
    for family in B.FAMILIES:
        for kind in C.SETS[family]:
            M, x, ref = C.operands(family, kind, s.na, s.c, s.pts)
            r = basis_call(gpu, family, s, M, x)
            bad += r["bad"] + _compare(r["out"], B.stored(ref, family), f"{r['what']} set {kind}")
    _report(bad)


@pytest.mark.parametrize("big", (0, 1), ids=lambda i: "a%d_c%d_p%d" % C.BIG_SHAPES[i])
@pytest.mark.parametrize("family", B.FAMILIES)
def test_64bit_forms_exact(gpu, family, big):
    """na c 4 >= 2^24: the 64-bit-address instance of every family, the whole tensor by `==` (set P), two directions per shape;
    on the first shape (padding rows, a half-empty last block) also the frozen norm on load in its exact form."""
    na, c, pts = C.BIG_SHAPES[big]
    blk, bad = C.blocks(na), []
    idx = {sp: B.layout_index(sp, blk, pts, c) for sp in (0, 1)}
    M, x, ref = C.operands(family, "P", na, c, pts)
    for i, o in (((0, 0), (1, 1)), ((0, 1), (1, 0)))[big]:
        s = C.Shape(na, c, pts, i, o)
        r = basis_call(gpu, family, s, M, x, index=(idx[i], idx[o]))
        bad += r["bad"] + _compare(r["out"], B.stored(ref, family), r["what"])
        del r
    if big == 0:
        M, x, stats, gamma, slope, ref = C.exact_frozen(family, na, c, pts)
        s = C.Shape(na, c, pts, 0, 1)
        r = basis_call(gpu, family, s, M, x, mode="norm", frozen=True, index=(idx[0], idx[1]),
                       norm=dict(stats=stats, gamma=gamma, beta=None, eps=0.0, slope=slope))
        bad += r["bad"] + _compare(r["out"], ref, r["what"])
    _report(bad)


# ------------------------------------------------------------------------------------------------ 2. the extras
@pytest.mark.parametrize("s", C.STATS_SHAPES, ids=C.sid)
def test_point_stats_exact(gpu, s):
    """Small integers: point_stats = (sum, sum of squares) over a point's stored outputs equals float64 by `==`."""
    bad = []
    for family in B.FAMILIES:
        M, x, ref = C.operands(family, "Is", s.na, s.c, s.pts)
        r = basis_call(gpu, family, s, M, x, mode="stats")
        st = B.stored(ref, family)
        bad += r["bad"] + _compare(r["out"], st, r["what"]) + _compare(r["stats"], B.point_stats(st), r["what"] + " point_stats")
    _report(bad)


def test_point_stats_of_the_rounded_bf16_values(gpu):
    """Integer outputs above 256 are rounded by the bf16 store: the statistics are those of the ROUNDED values."""
    M, x, ref = C.stats_over_256()
    s = C.Shape(M.shape[0], x.shape[2], x.shape[0], 0, 0)
    r = basis_call(gpu, "bf16", s, M, x, mode="stats")
    st = B.stored(ref, "bf16")
    _report(r["bad"] + _compare(r["out"], st, r["what"]) + _compare(r["stats"], B.point_stats(st), r["what"] + " point_stats"))


@pytest.mark.parametrize("family", B.FAMILIES)
def test_point_stats_refuses_the_spectral_output(gpu, family):
    s = C.Shape(60, 64, 2, 0, 1)
    M, x, _ = C.operands(family, "Is", s.na, s.c, s.pts)
    r = basis_call(gpu, family, s, M, x, mode="stats", expect_rc=C.EPN_EINVAL)
    assert bool((r["tout"] == 7.0).all()) and bool((torch.from_numpy(r["stats"]) == 7.0).all())
    _report(r["bad"])


def _amax_bits(v):
    return int(np.asarray(v, F32).reshape(1).view(np.uint32)[0])


@pytest.mark.parametrize("s", C.AMAX_SHAPES, ids=C.sid)
def test_amax_is_the_maximum_of_the_stored_output(gpu, s):
    """epn_so3_basis_amax_split_f32 on set P: out by `==`, and *amax is bit for bit max |stored out|."""
    M, x, ref = C.operands("x3", "P", s.na, s.c, s.pts)
    r = basis_call(gpu, "x3", s, M, x, mode="amax")
    bad = r["bad"] + _compare(r["out"], ref, r["what"])
    if _amax_bits(r["amax"]) != _amax_bits(B.amax(r["out"])):
        bad.append(f"{r['what']}: amax {r['amax']!r}, max |stored out| {B.amax(r['out'])!r}")
    _report(bad)


@pytest.mark.parametrize("s", C.AMAX_SHAPES, ids=C.sid)
def test_norm_amax_ignores_lanes_without_channels(gpu, s):
    """epn_so3_basis_norm_amax_split_f32, twice.  (a) Statistics of mean 10, variance 0.01: a lane without channels (the second
    point of an odd count at c = 32, lanes x >= 8 of a half-empty last block) normalises its zero rows to leaky(-100) = -25,
    five times any stored output.  (b) The genuine sums of normal inputs with gamma and beta.  In both *amax must be bit for bit
    max |stored out|, and `out` (+- the normalised inputs: set P's matrix) lies within the forward bound of the norm glue of the
    float64 norm (_norm_reference) -- which is also norm on load at c = 96 and on the 64-bit path, widths the unfolded route
    does not take."""
    assert C.phantom_lanes("x3", s.na, s.c, s.pts) == (s.c != 64), "all shapes but the c = 64 one have lanes without channels"
    M, _, _ = C.operands("x3", "P", s.na, s.c, s.pts)
    rng = np.random.default_rng(C._seed(s.na, s.c, s.pts, 9))
    rows = float(s.pts * s.na)
    xa = (10.0 + 0.1 * rng.standard_normal((s.pts, s.na, s.c))).astype(F32)
    na = dict(sums=np.broadcast_to(np.array([10.0 * rows, 100.01 * rows], F32), (1, s.c, 2)), groups=1, ppg=s.pts, gamma=None,
              beta=None, eps=1e-5, slope=0.25)
    xb, sums, gamma, beta = C.norm_inputs("x3", s, 1, True, seed=7)
    nb = dict(sums=sums, groups=1, ppg=s.pts, gamma=gamma, beta=beta, eps=1e-5, slope=0.01)
    bad = []
    for tag, x, norm in (("mean 10", xa, na), ("genuine sums", xb, nb)):
        r = basis_call(gpu, "x3", s, M, x, mode="norm_amax", norm=norm)
        bad += r["bad"]
        top = B.amax(r["out"])
        if tag == "mean 10":
            assert 0.5 < float(top) < 12.5, "the stored outputs are normalised values of a few units"
        if _amax_bits(r["amax"]) != _amax_bits(top):
            bad.append(f"{r['what']} ({tag}): amax {r['amax']!r}, max |stored out| {top!r}")
        ref, tol = _norm_reference("x3", s, M, x, norm, False)
        err = np.abs(r["out"].astype(F64) - ref)
        if not np.all(err <= tol):
            bad.append(f"{r['what']} ({tag}): {int((err > tol).sum())} of {err.size} stored outputs beyond the forward bound, worst "
                       f"error / bound {(err / tol).max():.3g}")
    _report(bad)


def _unfolded(gpu, family, s, M, x, norm, frozen):
    """The glue's norm-activation forward entry on x (plain layout), then the plain basis entry: the logical output."""
    _l, lib = _lib()
    dt, n = TDT[family], s.pts * s.na * s.c
    ain, tin = _filled(n, dt, gpu, B.to_flat(x, B.plain_index(s.pts, s.na, s.c)))
    ay, ty = _filled(n, dt, gpu)
    stat, ga, be = _dev(norm.get("sums", norm.get("stats")), gpu), _dev(norm.get("gamma"), gpu), _dev(norm.get("beta"), gpu)
    t = "bf16" if family == "bf16" else "f32"
    st = _l.stream_of(ty)
    if frozen:
        rc = getattr(lib, "epn_norm_act_frozen_fwd_" + t)(tin.data_ptr(), s.pts * s.na, s.c, stat.data_ptr(), _ptr(ga), _ptr(be), None,
                                                          norm["eps"], norm["slope"], ty.data_ptr(), st)
    else:
        rc = getattr(lib, "epn_norm_act_fwd_" + t)(tin.data_ptr(), norm["groups"], norm["ppg"] * s.na, s.c, stat.data_ptr(), _ptr(ga),
                                                   _ptr(be), None, norm["eps"], norm["slope"], ty.data_ptr(), st)
    torch.cuda.synchronize()
    lib.epn_last_kernel()
    assert rc == 0, f"the norm entry returned {rc}"
    ay.check("unfolded norm output")
    y = B.from_flat(_np(ty), B.plain_index(s.pts, s.na, s.c))
    return basis_call(gpu, family, s, M, y), y


def _norm_reference(family, s, M, x, norm, frozen):
    """(out f64, tolerance) of norm on load, the statistics restated in float64 from the sums / stats the kernel is given
    (basis_ref.norm_params): the forward bound of tests/test_gpu_norm_fp64.py, 4 T |gamma| (1 + |xhat|) + (2^-22 [+ 2^-8 with
    bf16 storage]) |y| with T = P u (1 + mean^2 / (var + eps)) and P = norm_ref.roundings (frozen: T = P u), carried through the
    signed permutation."""
    import norm_ref as N
    groups, ppg = norm["groups"], norm["ppg"]
    P = N.roundings(groups, ppg * s.na, min(s.c, 1024))      # the glue's geometry ends at c = 1024: wider takes its count
    mean, rstd = B.norm_params(norm.get("sums", norm.get("stats")), groups, ppg, s.na, norm["eps"], frozen)
    T = np.full(mean.shape, P * B.U24) if frozen else P * B.U24 * (1.0 + mean * mean * rstd * rstd)
    y, _, xhat = B.norm_on_load(x, mean, rstd, norm["gamma"], norm["beta"], norm["slope"], ppg)
    g = np.arange(s.pts) // ppg if groups > 1 else np.zeros(s.pts, dtype=np.int64)
    ga = np.abs(np.asarray(norm["gamma"], F64)) if norm["gamma"] is not None else 1.0
    tol = 4.0 * T[g][:, None, :] * ga * (1.0 + np.abs(xhat)) + (2.0 ** -22 + (2.0 ** -8 if family == "bf16" else 0.0)) * np.abs(y)
    if np.abs(M).sum(1).max() == 1.0:          # a signed permutation: carried through by indexing
        perm, sign = np.argmax(np.abs(M), 1), M[np.arange(M.shape[0]), np.argmax(np.abs(M), 1)].astype(F64)
        return y[:, perm, :] * sign[None, :, None], tol[:, perm, :]
    return B.transform(M, y), B.transform(np.abs(M), tol)


@pytest.mark.parametrize("s,groups", C.NORM_SHAPES, ids=lambda v: C.sid(v) if isinstance(v, tuple) else f"g{v}")
@pytest.mark.parametrize("family", B.FAMILIES)
def test_norm_on_load_and_the_unfolded_route(gpu, family, s, groups):
    """epn_so3_basis_norm_* and _norm_frozen_* on set P's matrix (outputs are +- the normalised inputs) against the unfolded
    route -- epn_norm_act_fwd_* / _frozen_fwd_*, then the plain entry -- from the same sums / stats, gamma, beta (present and
    NULL), eps and slope.  groups = 3 with an odd pts_per_group at c = 32: a pair task straddles two groups.
    FINDING (CHANGELOG has the figures): the kernel comment claimed the two routes agree to the last bit.  They do with frozen
    statistics (all families) and with bf16 storage, and are held to `==` there.  With batch / instance statistics and fp32
    storage a few ulp separate them in some elements.  The per-element expression is the one that agrees in the frozen form, so
    the presumed cause is mean / var / rstd = f(s1, s2, 1 / rows), compiled separately in the two kernels (not verified in the
    ISA).  BOTH routes are held to the float64 norm within the forward bound of tests/test_gpu_norm_fp64.py (_norm_reference)
    for every combination, as every norm kernel of the library is."""
    M, _, _ = C.operands(family, "P", s.na, s.c, s.pts)
    bad = []
    for frozen in (False, True):
        for affine in (True, False):
            x, sums, gamma, beta = C.norm_inputs(family, s, 1 if frozen else groups, affine, seed=int(frozen))
            norm = dict(gamma=gamma, beta=beta, eps=1e-5, slope=0.01, groups=1 if frozen else groups,
                        ppg=s.pts if frozen else s.pts // groups)
            norm["stats" if frozen else "sums"] = C.frozen_stats(s.c, 3) if frozen else sums
            r = basis_call(gpu, family, s, M, x, mode="norm", frozen=frozen, norm=norm)
            u, _ = _unfolded(gpu, family, s, M, x, norm, frozen)
            bad += r["bad"] + u["bad"]
            ref, tol = _norm_reference(family, s, M, x, norm, frozen)
            for route, got in (("folded", r["out"]), ("unfolded", u["out"])):
                err = np.abs(got.astype(F64) - ref)
                if not np.all(err <= tol):
                    bad.append(f"{r['what']} affine={affine} {route}: {int((err > tol).sum())} of {err.size} elements beyond the "
                               f"forward bound, worst error / bound {(err / tol).max():.3g}")
            differ = int((r["out"] != u["out"]).sum())
            print(f"{r['what']} affine={affine}: {differ} of {r['out'].size} elements differ between the routes, max "
                  f"{np.abs(r['out'].astype(F64) - u['out']).max():g}")
            if family == "bf16" or frozen:
                bad += _compare(r["out"], u["out"], f"{r['what']} affine={affine} against the unfolded route")
    _report(bad)


@pytest.mark.parametrize("s,groups", C.DSTATS_SHAPES, ids=lambda v: C.sid(v) if isinstance(v, tuple) else f"g{v}")
@pytest.mark.parametrize("family", B.FAMILIES)
def test_dstats(gpu, family, s, groups):
    """epn_so3_basis_dstats_*: dy = (signed permutation) . gradient by `==`; point_dstats[..][0] = sum d by `==` (integer
    gradients, slope 1/4: every sum is exact; no pre-activation within DSTATS_TAU of zero, test_basis_spec); point_dstats[..][1] =
    sum d xhat within 2^-24 [(DSTATS_K + 3.5 k2) sum |d xhat| + 2 sqrt(k2) sum |d|], k2 = mean^2 / (var + eps) -- the count is
    derived in basis_cases.dstats_ref.  x comes from norm_ref.real_inputs with the genuine batch / instance sums of every group,
    whose means are nonzero and differ from group to group (kappa 1, -1/2, 2): the mean, its channel and the group select of
    sb_point_dstats (a pair task straddles two groups at c = 32) all carry weight."""
    d = C.dstats_inputs(family, s, groups)
    dy, ds, tol, _, k2 = C.dstats_ref(family, s, groups, d)
    norm = dict(sums=d["sums"], groups=groups, ppg=d["ppg"], gamma=d["gamma"], beta=d["beta"], eps=d["eps"], slope=C.DSTATS_SLOPE)
    r = basis_call(gpu, family, s, d["M"], d["g"], mode="dstats", norm=norm, x_cl=d["x"])
    bad = r["bad"] + _compare(r["out"], dy, r["what"] + " dy") + _compare(r["stats"][..., 0], ds[..., 0], r["what"] + " sum d")
    err = np.abs(r["stats"][..., 1].astype(F64) - ds[..., 1])
    print(f"{r['what']}: worst |sum d xhat - fp64| / tolerance = {(err / tol).max():.3f} (k2 up to {k2.max():.2f})")
    if not np.all(err <= tol):
        bad.append(f"{r['what']} sum d xhat: {int((err > tol).sum())} of {err.size} beyond the tolerance, worst error / tolerance "
                   f"{(err / tol).max():.3g}")
    _report(bad)


@pytest.mark.parametrize("family", B.FAMILIES)
def test_dstats_refused_beyond_the_32bit_forms(gpu, family):
    """na c 4 >= 2^24 takes the 64-bit kernels, which have no dstats: EPN_EINVAL, point_dstats and out untouched."""
    s = C.Shape(64, 65536, 1, 1, 0)
    M, perm, sign = C.signed_perm(s.na, 3)
    x = np.ones((s.pts, s.na, s.c), F32)
    norm = dict(sums=np.broadcast_to(np.array([0.0, 64.0], F32), (1, s.c, 2)), groups=1, ppg=1, gamma=None, beta=None, eps=1e-5, slope=0.25)
    r = basis_call(gpu, family, s, M, x, mode="dstats", norm=norm, x_cl=x, expect_rc=C.EPN_EINVAL)
    bad = r["bad"]
    if not bool((torch.from_numpy(r["stats"]) == 7.0).all()):
        bad.append(f"{r['what']}: point_dstats was written by a refused call")
    if not bool((r["tout"] == 7.0).all()):
        bad.append(f"{r['what']}: out was written by a refused call")
    _report(bad)


# ------------------------------------------------------------------------------------------------ 3. real data
@pytest.mark.parametrize("c,direction", C.REAL_CASES, ids=lambda v: str(v))
def test_real_data_within_the_oracle_margin(gpu, c, direction):
    """Shipped U / U^T, normal inputs, 33 points: |kernel - fp64| <= 2 m_family 2^-24 S per element (bf16: + the half ulp of the
    one store rounding, 2^-8 of the value).  m_family: basis_cases.m_family, measured on the emulations."""
    bad = []
    for family in B.FAMILIES:
        k = C.real_case(family, c, direction)
        m = C.m_family(family)
        r = basis_call(gpu, family, k["shape"], k["M"], k["x"])
        err = np.abs(r["out"].astype(F64) - k["ref"])
        tol = 2.0 * m * B.U24 * k["S"]
        store = 2.0 ** -8 * (np.abs(k["ref"]) + tol) if family == "bf16" else 0.0
        ratio = float((np.maximum(err - store, 0.0) / (B.U24 * k["S"])).max())
        REAL_WORST[family] = max(REAL_WORST.get(family, 0.0), ratio)
        print(f"{r['what']}: worst |kernel - fp64| / (2^-24 S) = {ratio:.3f} (oracle {m:.3f}, allowed {2 * m:.3f})")
        bad += r["bad"]
        if not np.all(err <= tol + store):
            bad.append(f"{r['what']}: {int((err > tol + store).sum())} of {err.size} elements beyond the margin, worst ratio {ratio:.3f}")
    _report(bad)


# ------------------------------------------------------------------------------------------------ spectral weights
def _weights_call(gpu, w, W, Rm, bf):
    _l, lib = _lib()
    blk = B.blocks_of(w.dims)
    n, dt, bad = w.na * w.cin * w.cout, torch.bfloat16 if bf else torch.float32, []
    dW, dR, dblk = _dev(W, gpu), _dev(Rm, gpu), torch.from_numpy(blk).to(gpu)
    outs = {k: _filled(n, dt, gpu) for k in w.which}
    st = _l.stream_of(dW)
    lib.epn_last_kernel()
    fn = lib.epn_spectral_weights_bf16 if bf else lib.epn_spectral_weights_f32
    rc = fn(dW.data_ptr(), dR.data_ptr(), dblk.data_ptr(), w.cout, w.cin, w.kn, w.na, _ptr(outs["w"][1]) if "w" in outs else None,
            _ptr(outs["t"][1]) if "t" in outs else None, st)
    torch.cuda.synchronize()
    name = C.normalise(lib.epn_last_kernel())
    RECORDED.add(name)
    want = "spectral_weights_kernel<%s,%s>" % ("true" if "t" in outs else "false", "bf16" if bf else "float")
    what = f"{C.wid(w)} {'bf16' if bf else 'f32'} [{name}]"
    if rc != 0 or name != want:
        bad.append(f"{what}: returned {rc}, expected instance {want}")
    ref = B.spectral_weights(W, Rm).astype(F32)
    ref = R.bf16_rne(ref) if bf else ref
    for k, (a, t) in outs.items():
        try:
            a.check(f"{what} {k}")
        except AssertionError as e:
            bad.append(str(e))
        bad += _compare(B.from_flat(_np(t), B.weight_index(blk, w.cin, w.cout, k == "t")), ref, f"{what} layout {k}")
    return bad


@pytest.mark.parametrize("w", C.WEIGHT_CASES, ids=C.wid)
def test_spectral_weights_f32_exact(gpu, w):
    """What and its transposed layout, integers and a one-hot W against full-mantissa R, by `==`; and the transpose
    epn_spectral_weights_bwd_f32 on integer and one-hot gradients."""
    _l, lib = _lib()
    bad, blk = [], B.blocks_of(w.dims)
    for kind in ("I", "S"):
        bad += _weights_call(gpu, w, *C.weight_operands(w, kind), bf=False)
        g, Rm = C.weight_grad_operands(w, kind)
        ag, tg = _filled(g.size, torch.float32, gpu, B.to_flat(g, B.weight_index(blk, w.cin, w.cout, False)))
        aw, tw = _filled(w.cout * w.cin * w.kn, torch.float32, gpu)
        dR, dblk = _dev(Rm, gpu), torch.from_numpy(blk).to(gpu)
        lib.epn_last_kernel()
        rc = lib.epn_spectral_weights_bwd_f32(tg.data_ptr(), dR.data_ptr(), dblk.data_ptr(), w.cout, w.cin, w.kn, w.na, tw.data_ptr(),
                                              _l.stream_of(tw))
        torch.cuda.synchronize()
        name = C.normalise(lib.epn_last_kernel())
        RECORDED.add(name)
        what = f"{C.wid(w)} bwd set {kind} [{name}]"
        if rc != 0 or name != "spectral_weights_bwd_kernel":
            bad.append(f"{what}: returned {rc}")
        for a in (ag, aw):
            try:
                a.check(what)
            except AssertionError as e:
                bad.append(str(e))
        bad += _compare(_np(tw), B.spectral_weights_bwd(g, Rm), what)
    _report(bad)


@pytest.mark.parametrize("w", C.WEIGHT_CASES_BF16, ids=C.wid)
def test_spectral_weights_bf16_exact(gpu, w):
    """The bf16 operand copies: the float64 value rounded once."""
    bad = []
    for kind in ("I", "S"):
        bad += _weights_call(gpu, w, *C.weight_operands(w, kind), bf=True)
    _report(bad)


# ------------------------------------------------------------------------------------------------ last: coverage
def test_every_reachable_instance_ran(gpu):
    """The union of the instance names epn_last_kernel() reported in this module is the REACHABLE set: all twelve basis
    instances (family x addressing x frozen) and the five spectral-weight instances.  (Runs last; needs the whole module.)"""
    assert RECORDED, "this test judges the whole module: run it with the module's other tests, in one process"
    print("worst real-data ratios:", {k: round(v, 3) for k, v in REAL_WORST.items()})
    assert RECORDED == C.REACHABLE, f"missing: {sorted(C.REACHABLE - RECORDED)}, unexpected: {sorted(RECORDED - C.REACHABLE)}"
