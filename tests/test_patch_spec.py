"""Patch extraction without a GPU: the entry point exists at every layer, its argument checks run before any HIP runtime call,
and the specification (tests/patch_ref.py, the numpy restatement of include/epn_so3conv.h: epn_radius_patches_f32) has the
properties it claims: the n_sample smallest (key, i) pairs, ties to the lowest index, rows independent of how the keypoints
are split over calls, and a uniform subset."""
import ctypes
import math

import numpy as np
import pytest

import patch_ref as P

EINVAL = -1


def test_symbol_resolves_and_is_bound_at_every_layer(vgtk_alias):
    from epn_pointcloud_amd import _lib, models
    from epn_pointcloud_amd.vgtk.cuda import grouping
    assert "epn_radius_patches_f32" in _lib.EXPORTS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "epn_radius_patches_f32")
    assert callable(grouping.radius_patches)
    import vgtk.pc
    assert callable(vgtk.pc.radius_patches) and vgtk.pc.radius_patches is vgtk_alias.pc.radius_patches
    assert callable(models.InvSO3ConvModel.describe)


_OK = dict(pc=16, n=100, kpts=16, k=1, kpt_row0=0, radius=0.4, n_sample=64, seed=0, key_bits=32, center=0, scale=1.0, idx=16,
           counts=16, patches=16)          # pointers: non-NULL and never dereferenced (every call below is refused, or k = 0)


def _call(**over):
    from epn_pointcloud_amd import _lib
    a = dict(_OK, **over)
    vp = lambda v: ctypes.c_void_p(v) if v else None
    return _lib.get_lib().epn_radius_patches_f32(vp(a["pc"]), a["n"], vp(a["kpts"]), a["k"], a["kpt_row0"], a["radius"], a["n_sample"],
                                                 a["seed"], a["key_bits"], a["center"], a["scale"], vp(a["idx"]), vp(a["counts"]),
                                                 vp(a["patches"]), None)


@pytest.mark.parametrize("bad", [dict(n=0), dict(n=-5), dict(k=-1), dict(n_sample=0), dict(n_sample=8193), dict(key_bits=0),
                                 dict(key_bits=33), dict(radius=0.0), dict(radius=-0.4), dict(radius=float("nan")),
                                 dict(radius=float("inf")), dict(pc=0), dict(kpts=0), dict(idx=0), dict(counts=0),
                                 dict(patches=0)], ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_bad_arguments_are_refused_before_any_runtime_call(bad):
    assert _call(**bad) == EINVAL


def test_no_keypoints_is_success_and_launches_nothing():
    assert _call(k=0) == 0
    assert _call(k=0, pc=0, kpts=0, idx=0, counts=0, patches=0) == 0
    assert _call(k=0, n_sample=0) == EINVAL          # the other checks still hold


def _brute_subset(members, Q, n_sample, seed, key_bits):
    pairs = sorted((int(P.keys([i], Q, seed, key_bits)[0]), int(i)) for i in members)
    return sorted(i for _, i in pairs[:n_sample])


@pytest.mark.parametrize("count,n_sample", [(16, 16), (17, 16), (300, 64), (129, 128), (40, 1)])
def test_selected_set_is_the_smallest_key_index_pairs(count, n_sample):
    rng = np.random.default_rng(count)
    members = np.sort(rng.choice(5000, count, replace=False))
    for Q, seed in ((0, 0), (3, 2913), (2 ** 33 + 5, 2 ** 63 + 11)):
        row = P.select(members, Q, n_sample, seed)
        assert row.tolist() == _brute_subset(members, Q, n_sample, seed, 32)
        assert (np.diff(row) > 0).all() if n_sample > 1 else True


def test_four_key_bits_resolve_ties_to_the_lowest_index():
    members = np.arange(3, 903, 3)                     # 300 members, 16 distinct keys: ~19 per key
    Q, seed = 7, 99
    k = P.keys(members, Q, seed, 4)
    assert k.max() < 16
    partial = 0
    for n_sample in range(40, 60):                     # a bucket holds ~19: most of these cut one in the middle
        row = P.select(members, Q, n_sample, seed, key_bits=4)
        assert row.tolist() == _brute_subset(members, Q, n_sample, seed, 4)
        chosen = np.isin(members, row)
        T = k[chosen].max()
        assert chosen[k < T].all() and not chosen[k > T].any()
        ties = chosen[k == T]                          # in ascending index: a taken prefix, then none
        t = int(ties.sum())
        assert 0 < t <= ties.size and ties[:t].all() and not ties[t:].any()
        partial += t < ties.size
    assert partial >= 15


def test_fewer_members_than_samples_are_kept_and_repeated():
    members = np.array([4, 9, 10, 77, 300])
    row = P.select(members, 5, 32, 1)
    assert row[:5].tolist() == members.tolist() and np.isin(row[5:], members).all()
    assert len(set(row[5:].tolist())) > 1
    assert (P.select(members[:1], 5, 32, 1) == -1).all() and (P.select(members[:0], 5, 32, 1) == -1).all()


def test_rows_do_not_depend_on_how_the_keypoints_are_split():
    rng = np.random.default_rng(4)
    pc = rng.uniform(-1, 1, (600, 3)).astype(np.float32)
    kpts = pc[rng.choice(600, 10, replace=False)]
    whole = P.radius_patches(pc, kpts, 0.5, 24, seed=6, center=1, scale=2.0)
    a = P.radius_patches(pc, kpts[:4], 0.5, 24, seed=6, kpt_row0=0, center=1, scale=2.0)
    b = P.radius_patches(pc, kpts[4:], 0.5, 24, seed=6, kpt_row0=4, center=1, scale=2.0)
    assert whole[1].min() <= 24 <= whole[1].max()      # both branches of the selection are in play
    for w, x, y in zip(whole, a, b):
        assert np.array_equal(w, np.concatenate((x, y)))
    wrong = P.radius_patches(pc, kpts[4:], 0.5, 24, seed=6, kpt_row0=0, center=1, scale=2.0)
    assert not np.array_equal(wrong[0], b[0])          # the row number is part of the key


def test_the_subset_is_uniform():
    """count = 64, n_sample = 16, 200 seeds: every point's inclusion frequency within 5 sigma of 16 / 64."""
    members = np.arange(64)
    hits = np.zeros(64)
    for seed in range(200):
        hits[P.select(members, 11, 16, seed)] += 1
    sigma = math.sqrt(0.25 * 0.75 / 200)
    assert np.abs(hits / 200 - 0.25).max() <= 5 * sigma, (hits / 200).tolist()


def test_build_inv_records_the_patch_configuration_outside_the_state_dict():
    import torch
    from epn_pointcloud_amd import models as M
    m = M.build_inv(input_num=1024, search_radius=0.3, width_div=8)
    assert m.search_radius == pytest.approx(0.3) and m.input_num == 1024
    keys = list(m.state_dict().keys())
    bare = M.build_inv(input_num=1024, search_radius=0.3, width_div=8)
    del bare.search_radius, bare.input_num
    assert list(bare.state_dict().keys()) == keys
    names = [n for n, _ in m.named_buffers()] + [n for n, _ in m.named_parameters()]
    assert not any("search_radius" in n or "input_num" in n for n in names + keys)
    with pytest.raises(RuntimeError, match="eval"):
        m.train().describe(torch.zeros(4, 3), torch.zeros(1, 3))
