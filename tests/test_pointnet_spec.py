"""What the exact tests of the PointNet head (tests/test_gpu_pointnet_exact.py) stand on, checked without a device:
the float64 restatement (tests/pointnet_ref.py) against the torch oracle and against torch.max, the builders' proofs for every
case of tests/pointnet_cases.py, the restated dispatch, mutants of the restatement that the tables must catch, and the CPU
measurement behind REAL_M."""
import math

import numpy as np
import pytest
import torch

import pointnet_cases as C
import pointnet_ref as P
from gemm_ref import bf16_rne

ALL_FUSED = C.FWD_CASES + C.TIE_CASES
ALL_TABLES = ALL_FUSED + C.MAX_CASES + C.BWD_DATA_CASES + C.BWD_WEIGHT_CASES + C.BWD_COORD_CASES


# ------------------------------------------------------------------------------------------------ restatement vs oracle
@pytest.mark.parametrize("b,p,a,c,co,bias", [(2, 9, 3, 5, 7, True), (1, 17, 1, 4, 3, True), (3, 6, 12, 16, 9, False)])
def test_restatement_against_the_torch_oracle(b, p, a, c, co, bias):
    """Values and, through autograd in float64, every gradient (random floats: no ties)."""
    from oracle import so3conv_ref as O
    rng = np.random.default_rng(b * 100 + p)
    F = rng.standard_normal((b, p, a, c))
    xyz = rng.standard_normal((b, 3, p))
    q, _ = np.linalg.qr(rng.standard_normal((a, 3, 3)))
    anchors = None if a == 1 else q
    W, bs, gout = rng.standard_normal((co, c + 3)), (rng.standard_normal(co) if bias else None), rng.standard_normal((b, a, co))
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).double().requires_grad_(True)
    Ft, Wt = t(F.transpose(0, 3, 1, 2)), t(W)
    bt = t(bs) if bias else None
    y = O.pointnet_so3conv(torch.from_numpy(xyz), Ft, None if a == 1 else torch.from_numpy(anchors), Wt, bt)     # [b, co, a]
    y.backward(torch.from_numpy(gout.transpose(0, 2, 1)))
    out, arg, ctr = P.forward(F, xyz, anchors, W, bs)
    close = lambda got, want: np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-13)
    close(out, y.detach().numpy().transpose(0, 2, 1))
    close(P.bwd_data(gout, arg, W, p), Ft.grad.numpy().transpose(0, 2, 3, 1))
    dW, db = P.bwd_weight(gout, arg, F, xyz, anchors, ctr)
    close(dW, Wt.grad.numpy())
    dWx, db2 = P.bwd_coord(gout, arg, xyz, anchors, ctr)
    close(dWx, Wt.grad.numpy()[:, c:])
    close(db, gout.sum(axis=(0, 1)))
    close(db2, db)
    if bias:
        close(db, bt.grad.numpy())
    close(P.dz(gout, arg, p).sum(axis=1), gout)


def _same(got, want):
    """Equal including NaN positions and the sign of zeros."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.array_equal(got, want, equal_nan=True) and np.array_equal(np.signbit(got), np.signbit(want))


@pytest.mark.parametrize("pattern", list(C.SPECIAL_PATTERNS) + ["all_neg_inf"])
def test_restatement_against_torch_max_on_special_values(pattern):
    expect_first = {"two_nans": 0, "nan_after_inf": 1, "nan_before_inf": 0, "inf_twice": 0, "neg_zero_first": 0, "pos_zero_first": 0}
    for pair in C.SPECIAL_PAIRS:
        Z = C.special_Z(pattern, pair).astype(np.float64)
        out, arg = P.max_first(Z, axis=1)
        tv, ti = torch.from_numpy(Z).max(dim=1)
        assert _same(out, tv.numpy()) and np.array_equal(arg, ti.numpy()), (pattern, pair)
        if pattern == "all_neg_inf":
            assert np.all(arg == 0) and np.all(out == -np.inf)
        else:
            assert np.all(arg[..., :-1] == pair[expect_first[pattern]]), (pattern, pair)


def test_nan_features_make_the_whole_row_nan():
    for c in (C.TIE_CASES[0], C.TIE_CASES[6]):
        for pair in C.SPECIAL_PAIRS:
            F, (bb, ai) = C.nan_features(c, pair)
            d = C.case(c)
            out, arg, _ = P.forward(F, d["xyz"], d["anchors"], d["W"], d["bias"])
            assert np.isnan(out[bb, ai]).all() and np.all(arg[bb, ai] == pair[0])
            keep = np.ones(out.shape[:2], bool)
            keep[bb, ai] = False
            assert np.array_equal(out[keep], d["ref"]["out"][keep]) and np.array_equal(arg[keep], d["ref"]["arg_fwd"][keep])


# ------------------------------------------------------------------------------------------------ builders, dispatch
@pytest.mark.parametrize("c", ALL_TABLES, ids=lambda c: c.name)
def test_builder_proves_its_case(c):
    d = C.case(c)                                   # build() asserts
    assert max(d["ref"]["bits"].values()) < 1.0
    for k in ("F", "xyz", "W", "gout"):
        assert d[k].dtype == np.float32
    assert d["arg"].dtype == np.int32 and d["arg"].min() >= 0 and d["arg"].max() < c.p
    assert c.b <= 3
    assert np.array_equal(d["ref"]["Z"], d["ref"]["Z"].astype(np.float32))


def test_dz_cases():
    for c in C.DZ_CASES:
        d = C.build_dz(c)
        assert c.co % 8 == 0 and d["f32"].shape == (c.b, c.p, c.a, c.co)
        assert np.array_equal(d["f32"].sum(axis=1), d["gout"].astype(np.float64))
        assert not np.array_equal(d["bf16"], d["f32"])
    assert sorted(c.b * c.p * c.a * c.co // 8 for c in C.DZ_CASES) == [255, 255, 256, 256, 257, 258, 258]
    # ties to even, both directions
    assert bf16_rne(np.float32(1 + 2.0 ** -8)) == 1.0 and bf16_rne(np.float32(1 + 3 * 2.0 ** -8)) == np.float32(1 + 2.0 ** -6)


def test_names_are_unique_and_the_restated_dispatch_covers_every_case():
    names = [c.name for c in ALL_TABLES] + [c.name for c in C.DZ_CASES]
    assert len(names) == len(set(names))
    ran = {C.fwd_kernel(c.c) for c in ALL_FUSED}
    assert ran == {"pointnet_fwd_mfma_kernel", "pointnet_fwd_kernel"}
    assert ran | set(C.KERNEL.values()) == C.REACHABLE_POINTNET and len(C.REACHABLE_POINTNET) == 8
    for c in ALL_FUSED:
        assert (C.fwd_kernel(c.c) == "pointnet_fwd_mfma_kernel") == (c.c % 16 == 0)
    for c in C.OPS_CASES:
        assert c.c % 16 == 0 and c.co % 8 == 0
    assert len(C.OPS_CASES) >= 10 and any(c.ties for c in C.OPS_CASES)


def test_the_tables_hold_the_edges_the_kernels_have():
    """The sets the exact tests are meant to cover, restated from the kernels' constants."""
    f = lambda pred, key: {getattr(c, key) for c in C.FWD_CASES if pred(c)}
    valu, mfma = (lambda c: c.c % 16 != 0), (lambda c: c.c % 16 == 0)
    assert f(valu, "c") >= {1, 4, 63, 65, 70} and f(valu, "p") >= {1, 31, 32, 33, 65} and f(valu, "co") >= {1, 127, 128, 129}
    assert f(valu, "a") >= {1, 2} and {c.bias for c in C.FWD_CASES if valu(c)} == {True, False}
    assert f(mfma, "c") >= {16, 48, 64, 80, 144} and f(mfma, "p") >= {1, 3, 4, 15, 16, 17, 63, 64, 65, 129}
    assert f(mfma, "co") >= {1, 15, 17, 31, 33, 127, 128, 129, 257} and f(mfma, "a") >= {1, 2, 60}
    assert {c.co for c in C.MAX_CASES} >= {8, 248, 256, 264} and {c.p for c in C.MAX_CASES} >= {1, 7, 8, 9, 63, 64, 65, 72, 129}
    assert {c.co for c in C.BWD_DATA_CASES} >= {1, 3, 4, 5, 7, 9} and {c.c for c in C.BWD_DATA_CASES} >= {1, 127, 128, 129}
    assert {c.p for c in C.BWD_DATA_CASES} >= {1, 63, 64, 65, 130}
    assert {c.routing for c in C.BWD_DATA_CASES} >= {"fwd", "random", 0, -1, 63, 64}
    assert {c.b * c.a for c in C.BWD_WEIGHT_CASES} >= {1, 7, 8, 9, 15, 16, 17, 33, 128, 131}
    assert {c.c for c in C.BWD_WEIGHT_CASES} >= {1, 253, 254, 256} and {c.co for c in C.BWD_WEIGHT_CASES} >= {1, 3}
    assert any(not c.bias for c in C.BWD_WEIGHT_CASES) and any(not c.bias for c in C.BWD_COORD_CASES)
    assert any(C.weight_slices(c.b * c.a)[2] > 0 for c in C.BWD_WEIGHT_CASES)
    assert {c.b * c.a for c in C.BWD_COORD_CASES} >= {1, 255, 256, 257, 513}
    for (i, j), (k, l) in C.PLACES.values():
        assert i < j < C.TIE_P and k < l < C.TIE_P
    g = lambda i: (i // 16, (i % 16) // 4)                  # (16-tile, lane group)
    (i, j), _ = C.PLACES["same_lane_group"]
    assert g(i) == g(j)
    (i, j), _ = C.PLACES["other_lane_group"]
    assert g(i)[0] == g(j)[0] and g(i)[1] != g(j)[1]
    (i, j), _ = C.PLACES["other_tile16"]
    assert g(i)[0] != g(j)[0] and g(i)[1] == g(j)[1] and i // 64 == j // 64
    for key, tile in (("across_tile32", 32), ("across_tile64", 64), ("across_unroll8", 8)):
        for i, j in C.PLACES[key]:
            assert i // tile != j // tile


# ------------------------------------------------------------------------------------------------ mutants
def _first_in(z, sel):
    """(value, index) of the first maximum of z[b][p][a][co] over the points sel (NaN-aware); no point: (-inf, 0)."""
    if not sel.any():
        return np.full(z[:, 0].shape, -np.inf), np.zeros(z[:, 0].shape, np.int64)
    idx = np.flatnonzero(sel)
    v, k = P.max_first(z[:, idx], axis=1)
    return v, idx[k]


def lane_group_max(z, tie="smaller"):
    """pointnet_fwd_mfma_kernel's order: a sequential scan per lane group j = (p % 16) // 4, then the butterfly (j ^ 1, j ^ 2).
    tie: "smaller" (the kernel) | "larger" (mutant) | "ge" (mutant: the other lane wins whenever its value is >=)."""
    pts = np.arange(z.shape[1])
    groups = [_first_in(z, (pts % 16) // 4 == j) for j in range(4)]

    def comb(x, y):
        (xv, xi), (yv, yi) = x, y
        xn, yn = np.isnan(xv), np.isnan(yv)
        if tie == "ge":
            take = yv >= xv
        else:
            less = yi < xi if tie == "smaller" else yi > xi
            take = np.where(xn | yn, yn & (~xn | (yi < xi)), (yv > xv) | ((yv == xv) & less))
        return np.where(take, yv, xv), np.where(take, yi, xi)

    return comb(comb(groups[0], groups[1]), comb(groups[2], groups[3]))[1].astype(np.int32)


def _arg_last(z):
    return (z.shape[1] - 1 - P.max_first(z[:, ::-1], axis=1)[1]).astype(np.int32)


def _arg_nan_ignored(z):
    return P.max_first(np.where(np.isnan(z), -np.inf, z), axis=1)[1]


def _arg_second_nan(z):
    nan = np.isnan(z)
    first = nan.argmax(axis=1)
    rest = nan.copy()
    np.put_along_axis(rest, first[:, None], False, axis=1)
    return np.where(rest.any(axis=1), rest.argmax(axis=1), P.max_first(z, axis=1)[1]).astype(np.int32)


def _forward_inputs():
    """(name, embedding z, restatement's arg-max) of every forward case, tie case and special-value pattern."""
    for c in ALL_FUSED:
        d = C.case(c)
        yield c.name, P.embed(d["F"], d["xyz"], d["anchors"], d["W"], d["bias"]), d["ref"]["arg_fwd"]
    for c in (C.TIE_CASES[0], C.TIE_CASES[6]):
        d = C.case(c)
        for pair in C.SPECIAL_PAIRS:
            z = P.embed(C.nan_features(c, pair)[0], d["xyz"], d["anchors"], d["W"], d["bias"])
            yield f"{c.name} NaN {pair}", z, P.max_first(z, axis=1)[1]
    for pattern in list(C.SPECIAL_PATTERNS) + ["all_neg_inf"]:
        for pair in C.SPECIAL_PAIRS:
            z = C.special_Z(pattern, pair).astype(np.float64)
            yield f"{pattern} {pair}", z, P.max_first(z, axis=1)[1]


def _chunk_read_as_full(c):
    """Forward mutant: the last 64-channel chunk read as a full one -- W's row runs on into its coordinate columns and the next
    row, the feature row into the next row (zeros behind the buffers)."""
    d = C.case(c)
    cf = (c.c + 63) // 64 * 64
    Wf = np.concatenate([d["W"].astype(np.float64).reshape(-1), np.zeros(cf)])
    Ff = np.concatenate([d["F"].astype(np.float64).reshape(-1), np.zeros(cf)])
    W2 = np.stack([Wf[o * (c.c + 3):o * (c.c + 3) + cf] for o in range(c.co)])
    F2 = np.stack([Ff[r * c.c:r * c.c + cf] for r in range(c.b * c.p * c.a)]).reshape(c.b, c.p, c.a, cf)
    z = F2 @ W2.T + (P.embed(d["F"], d["xyz"], d["anchors"], d["W"], d["bias"]) - d["ref"]["Z"])
    return P.max_first(z, axis=1)


def _dF_tail_skipped(c):
    d = C.case(c)
    g = d["gout"].copy()
    g[..., c.co - c.co % 4:] = 0
    return P.bwd_data(g, d["arg"], d["W"], c.p)


def _dW_empty_slices_twice(c):
    """An empty slice (q0 >= b a) walks the last `per` pairs once more."""
    d = C.case(c)
    nba = c.b * c.a
    _, per, empty = C.weight_slices(nba)
    g = d["gout"].astype(np.float64).reshape(nba, c.co).copy()
    g[max(0, nba - per):] *= 1 + empty
    return P.bwd_weight(g.reshape(c.b, c.a, c.co), d["arg"], d["F"], d["xyz"], d["anchors"], d["ref"]["centre"])[0]


def _bf16_truncate(x):
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) & 0xFFFF0000).view(np.float32)


def test_lane_group_emulation_is_the_restatement():
    for name, z, arg in _forward_inputs():
        assert np.array_equal(lane_group_max(z), arg), name


ARG_MUTANTS = {
    "last maximum wins": _arg_last,
    "a cross-group tie goes to the larger index": lambda z: lane_group_max(z, "larger"),
    "NaN is ignored": _arg_nan_ignored,
    "the second NaN wins": _arg_second_nan,
    "an empty lane group contributes (-inf, 0) with >=": lambda z: lane_group_max(z, "ge"),
}


@pytest.mark.parametrize("mutant", list(ARG_MUTANTS))
def test_the_tables_catch_argmax_mutants(mutant):
    caught = [name for name, z, arg in _forward_inputs() if not np.array_equal(ARG_MUTANTS[mutant](z), arg)]
    print(f"{mutant}: caught by {len(caught)} inputs, e.g. {caught[:4]}")
    assert caught, f"no case of the tables notices the mutant '{mutant}': a case is missing"


def test_the_tie_cases_catch_their_own_mutants():
    """Every tie case, not just some case: the last-maximum mutant moves its arg-max; the cross-lane-group case is what catches
    the larger-index combine apart from cases that tie by chance."""
    for c in C.TIE_CASES:
        d = C.case(c)
        z = P.embed(d["F"], d["xyz"], d["anchors"], d["W"], d["bias"])
        assert not np.array_equal(_arg_last(z), d["ref"]["arg_fwd"]), c.name
        # ... and the gradient moves with it
        assert not np.array_equal(P.bwd_data(d["gout"], _arg_last(z), d["W"], c.p), d["ref"]["dF"]), c.name
    for name in ("tie_mfma_other_lane_group", "tie_mfma_identical_cloud"):
        d = C.case(next(c for c in C.TIE_CASES if c.name == name))
        z = P.embed(d["F"], d["xyz"], d["anchors"], d["W"], d["bias"])
        assert not np.array_equal(lane_group_max(z, "larger"), d["ref"]["arg_fwd"]), name
    # p in 1 .. 3: three lane groups are empty; with ">=" they would win a column of -inf ... which has arg 0 either way, so
    # that mutant is visible only through ties across groups (above) -- stated here so that nobody looks for a missing case
    z = np.full((1, 3, 1, 4), -np.inf)
    assert np.array_equal(lane_group_max(z, "ge"), P.max_first(z, axis=1)[1])


def test_the_tables_catch_the_structural_mutants():
    partial = [c for c in ALL_FUSED if c.c % 64]
    assert any(not (np.array_equal(_chunk_read_as_full(c)[0], C.case(c)["ref"]["out"])) for c in partial if c.c % 16 == 0), \
        "partial channel chunk read as a full one: no MFMA case notices"
    assert any(not (np.array_equal(_chunk_read_as_full(c)[0], C.case(c)["ref"]["out"])) for c in partial if c.c % 16), \
        "partial channel chunk read as a full one: no VALU case notices"
    tails = [c for c in C.BWD_DATA_CASES if c.co % 4]
    assert tails and all(not np.array_equal(_dF_tail_skipped(c), C.case(c)["ref"]["dF"]) for c in tails), "co % 4 tail skipped"
    empties = [c for c in C.BWD_WEIGHT_CASES if C.weight_slices(c.b * c.a)[2]]
    assert empties and all(not np.array_equal(_dW_empty_slices_twice(c), C.case(c)["ref"]["dW"]) for c in empties), \
        "empty weight-gradient slices counted twice"
    for c in C.DZ_CASES:
        d = C.build_dz(c)
        trunc = P.dz(_bf16_truncate(d["gout"]), d["arg"], c.p)
        assert not np.array_equal(trunc, d["bf16"]), f"{c.name}: dz truncating where it should round goes unnoticed"


# ------------------------------------------------------------------------------------------------ REAL_M
def _ordered_sum(term, groups):
    """fp32: every group summed sequentially from its first term, the group sums added in order."""
    total = None
    for grp in groups:
        s = term(grp[0])
        for k in grp[1:]:
            s = s + term(k)
        total = s if total is None else total + s
    assert total.dtype == np.float32
    return total


def _orders(ids, tail, rng):
    """Summation orders over the term ids `ids` followed (or preceded) by `tail`."""
    ids, tail = list(ids), list(tail)
    blocks = lambda n: [ids[i:i + n] for i in range(0, len(ids), n)]
    out = {"sequential, tail last": [[k] for k in ids + tail], "sequential, tail first": [[k] for k in tail + ids],
           "blocks of 4": ([tail] if tail else []) + blocks(4), "chunks of 64": blocks(64) + ([tail] if tail else [])}
    for i in range(2):
        out[f"random permutation {i}"] = [[k] for k in rng.permutation(ids + tail)]
    return out


def f32_centre_ext(d):
    """The kernels' centre (sequential fp32 mean) and rotated coordinates in fp32."""
    xyz, R = d["xyz"], d["anchors"]
    ctr = (np.cumsum(xyz, axis=2, dtype=np.float32)[:, :, -1] / np.float32(xyz.shape[2])).astype(np.float32)
    v = (xyz - ctr[:, :, None]).transpose(0, 2, 1)                                       # [b][p][3]
    e = np.stack([(R[None, None, :, 0, i] * v[:, :, None, 0] + R[None, None, :, 1, i] * v[:, :, None, 1])
                  + R[None, None, :, 2, i] * v[:, :, None, 2] for i in range(3)], axis=-1)
    assert e.dtype == np.float32
    return ctr, e


def measure_real_ratio(shape):
    """Worst |fp32 - fp64| / (2^-24 S) per pass over the summation orders, on the real-tier inputs of one shape."""
    d = C.real_case(shape)
    b, c, co, p, a = shape
    rng = np.random.default_rng(7)
    F, W, bias, g, arg = d["F"], d["W"], d["bias"], d["gout"], d["arg64"]
    ctr, e = f32_centre_ext(d)
    S = P.magnitudes(F, d["xyz"], d["anchors"], W, bias, g, arg)
    worst = {}

    def note(what, got, ref, s):
        assert np.all((got == ref) | (s > 0))
        r = float((np.abs(got.astype(np.float64) - ref) / (2.0 ** -24 * np.where(s > 0, s, 1.0))).max())
        worst[what] = max(worst.get(what, 0.0), r)

    def fwd_term(k):
        if k < c:
            return F[..., k, None] * W[:, k]
        if k < c + 3:
            return e[..., k - c, None] * W[:, k]
        return np.broadcast_to(bias, (b, p, a, co)).astype(np.float32)

    for name, groups in _orders(range(c), range(c, c + 4), rng).items():
        note("out", _ordered_sum(fwd_term, groups).max(axis=1), d["out64"], S["out"])
    dZ = P.dz(g, arg, p).astype(np.float32)
    ref_dF = P.bwd_data(g, arg, W, p)
    for name, groups in _orders(range(co), (), rng).items():
        note("dF", _ordered_sum(lambda o: dZ[..., o, None] * W[o, :c], groups), ref_dF, S["dF"])
    G = np.concatenate([P._gather(F, arg), P._gather(e, arg)], axis=-1).reshape(b * a, co, c + 3)      # fp32
    g2 = g.reshape(b * a, co)
    ref_dW, ref_db = P.bwd_weight(g, arg, F, d["xyz"], d["anchors"], ctr)
    for name, groups in _orders(range(b * a), (), rng).items():
        note("dW", _ordered_sum(lambda q: g2[q, :, None] * G[q], groups), ref_dW, S["dW"])
        note("dbias", _ordered_sum(lambda q: g2[q], groups), ref_db, S["dbias"])
    return worst


def test_real_m_is_twice_the_cpu_fp32_oracles_worst_ratio():
    worst = {}
    for shape in C.REAL_SHAPES:
        for k, v in measure_real_ratio(shape).items():
            worst[k] = max(worst.get(k, 0.0), v)
    top = max(worst.values())
    print("worst |fp32 - fp64| / (2^-24 S) of the CPU restatement per pass:", {k: round(v, 4) for k, v in worst.items()})
    assert abs(top - C.REAL_RATIO_MEASURED) < 5e-3, f"measured {top:.4f}, pointnet_cases.py records {C.REAL_RATIO_MEASURED}"
    assert C.REAL_M == max(1, math.ceil(2 * top)), (top, C.REAL_M)
    assert C.REAL_M <= min(s[1] for s in C.REAL_SHAPES) + 5
