"""The dropout mask's specification (include/epn_so3conv.h "dropout inside the norm passes"), restated in numpy
(tests/philox_ref.py) and checked without a GPU: the published Philox4x32-10 known-answer vectors, the element -> (counter,
word) mapping, and that the seed the GPU statistics test fixes satisfies that test's bounds in the restatement itself -- so
on the GPU those bounds are conditions on the kernel, not on luck."""
import math

import numpy as np
import pytest

import philox_ref as P

# Random123 kat_vectors, philox4x32 10 rounds
KAT = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    got = " ".join("%08x" % int(w[0]) for w in P.philox4x32_10(counter, key))
    assert got == want


def test_philox_is_vectorised_consistently():
    """An array of counters gives, per entry, what the scalar call gives."""
    c0 = np.array([0, 0xFFFFFFFF, 0x243F6A88, 7], dtype=np.uint64)
    words = P.philox4x32_10([c0, 5, 6, 7], (11, 13))
    for i, c in enumerate(c0):
        one = P.philox4x32_10([int(c), 5, 6, 7], (11, 13))
        assert [int(w[i]) for w in words] == [int(w[0]) for w in one]


def test_mask_layout_and_threshold():
    """Element e takes word e & 3 of the call with counter e >> 2; 64-bit seed and call fill both halves of key / counter;
    the logical [b, c, p, a] view is the channels-last order."""
    seed, call, rate = (5 << 32) | 9, (3 << 32) | 2, 0.1
    assert P.threshold(0.1) == 429496729 and P.threshold(0.5) == 1 << 31
    flat = P.keep_mask_flat(64, rate, seed, call)
    for e in (0, 1, 2, 3, 4, 37, 63):
        w = P.philox4x32_10([e >> 2, 0, 2, 3], (9, 5))[e & 3][0]
        assert bool(flat[e]) == (int(w) >= P.threshold(rate))
    m = P.keep_mask(2, 8, 2, 2, rate, seed, call)
    assert m.shape == (2, 8, 2, 2)
    for (bi, ch, pi, ai) in ((0, 0, 0, 0), (1, 3, 1, 0), (1, 7, 1, 1), (0, 5, 0, 1)):
        assert m[bi, ch, pi, ai] == flat[((bi * 2 + pi) * 2 + ai) * 8 + ch]
    # a seed or call truncated to 32 bits gives another mask
    big = P.keep_mask_flat(4096, 0.5, seed, call)
    assert (big != P.keep_mask_flat(4096, 0.5, seed & 0xFFFFFFFF, call)).any()
    assert (big != P.keep_mask_flat(4096, 0.5, seed, call & 0xFFFFFFFF)).any()


def test_fixed_seed_of_the_gpu_statistics_test_meets_its_bounds():
    failures = P.mask_statistics_failures(
        lambda call: P.keep_mask(*P.STAT_SHAPE, P.STAT_RATE, P.STAT_SEED, call), P.STAT_SHAPE, P.STAT_RATE)
    assert not failures, failures


def test_statistics_bounds_reject_a_biased_mask():
    """The bounds are not vacuous: a mask drawn at another rate, or repeated between calls, fails them."""
    rng = np.random.default_rng(0)
    b, c, p, a = P.STAT_SHAPE
    biased = lambda call: rng.random((b, c, p, a)) >= P.STAT_RATE + 0.01
    assert P.mask_statistics_failures(biased, P.STAT_SHAPE, P.STAT_RATE)
    same = P.keep_mask(*P.STAT_SHAPE, P.STAT_RATE, P.STAT_SEED, 0)
    assert P.mask_statistics_failures(lambda call: same, P.STAT_SHAPE, P.STAT_RATE)
    assert math.isclose(P.STAT_RATE, 0.3)


# ---- the host side of the feature, as far as it goes without a GPU (each of these fails on a tree without the dropout kernels)

def test_dropout_entry_points_are_declared_exported_and_validate_on_the_host():
    """The eight new C entry points are in the header, the library and the binding; a rate outside (0, 1) or a missing state is
    refused on the host, before anything is launched."""
    import ctypes
    from epn_pointcloud_amd import _lib
    names = [f"epn_norm_act_dropout_{k}_{t}" for k in ("fwd", "bwd_reduce", "bwd_apply") for t in ("f32", "bf16")]
    names += ["epn_dropout_mask_u8", "epn_dropout_state_next"]
    header = open(_lib.os.path.join(_lib.os.path.dirname(_lib._PKG), "include", "epn_so3conv.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert n in _lib.EXPORTS and n + "(" in header and hasattr(raw, n), n
    lib = _lib.get_lib()
    EINVAL, ENULL = -1, -3
    state = (ctypes.c_longlong * 2)(1, 0)          # never dereferenced by these calls
    sp = ctypes.cast(state, ctypes.c_void_p)
    for bad in (0.0, 1.0, -0.5, 2.0, float("nan")):
        assert lib.epn_dropout_mask_u8(None, 0, bad, sp, None) == EINVAL
    assert lib.epn_dropout_mask_u8(None, 0, 0.5, None, None) == ENULL
    assert lib.epn_dropout_mask_u8(None, 0, 0.5, sp, None) == 0         # nothing to write
    assert lib.epn_dropout_mask_u8(None, -1, 0.5, sp, None) == EINVAL
    assert lib.epn_dropout_state_next(None, None, None) == ENULL
    # the norm entry points check the rate first as well (groups = 0: nothing to do once the arguments are accepted)
    assert lib.epn_norm_act_dropout_fwd_f32(None, 0, 0, 8, None, None, None, None, 1e-5, 0.01, 1.0, sp, None, None) == EINVAL
    assert lib.epn_norm_act_dropout_fwd_f32(None, 0, 0, 8, None, None, None, None, 1e-5, 0.01, 0.5, None, None, None) == ENULL
    assert lib.epn_norm_act_dropout_fwd_f32(None, 0, 0, 8, None, None, None, None, 1e-5, 0.01, 0.5, sp, None, None) == 0


def test_norm_act_takes_dropout_as_a_keyword_and_checks_the_rate():
    """`dropout` is keyword-only: the positional defaults of ops.norm_act (residual, slope, conv_bias) are what they were.  A rate
    outside [0, 1) raises ValueError before any tensor is touched."""
    import inspect
    import torch
    from epn_pointcloud_amd import ops
    sig = inspect.signature(ops.norm_act).parameters
    assert sig["dropout"].kind is inspect.Parameter.KEYWORD_ONLY and sig["dropout"].default == 0.0
    assert ops.norm_act.__defaults__ == (None, 0.01, None)
    x, norm = torch.zeros(1, 8, 2, 60), torch.nn.InstanceNorm2d(8)
    for bad in (1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            ops.norm_act(x, norm, dropout=bad)
        with pytest.raises(ValueError):
            ops.dropout_mask(1, 8, 2, 60, bad, (1, 0))
    with pytest.raises(RuntimeError):               # a valid rate goes on to the HIP path: no CPU fall-back
        ops.norm_act(x, norm, dropout=0.5)
    assert ops._as_int64(2 ** 64 - 1) == -1 and ops._as_int64(2 ** 63) == -2 ** 63 and ops._as_int64(5) == 5


def test_blocks_choose_the_hip_dropout_path(monkeypatch):
    """schedule._hip_dropout_rate: 0.0 without dropout, the rate for 0 < rate < 1, None (stock modules) for rate 1 and under the
    A/B switch EPN_FUSED_DROPOUT=0, which defaults to 1."""
    import torch
    from epn_pointcloud_amd import _ab, schedule as S
    assert _ab.AB_DEFAULTS["EPN_FUSED_DROPOUT"] == "1"
    monkeypatch.setenv("EPN_AB", "1")
    monkeypatch.delenv("EPN_FUSED_DROPOUT", raising=False)
    assert S._hip_dropout_rate(None) == 0.0
    assert S._hip_dropout_rate(torch.nn.Dropout(0.25)) == 0.25
    assert S._hip_dropout_rate(torch.nn.Dropout(1.0)) is None
    monkeypatch.setenv("EPN_FUSED_DROPOUT", "0")
    assert S._hip_dropout_rate(torch.nn.Dropout(0.25)) is None
    assert S._hip_dropout_rate(None) == 0.0
