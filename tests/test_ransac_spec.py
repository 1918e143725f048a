"""Pairwise registration without a GPU: the entry points exist at every layer, every argument refusal is decided on the host
before any HIP runtime call, the workspace query follows its formula, the specification's numpy restatement
(tests/ransac_ref.py) recovers a planted transform, and the host-side error measures are right on hand-made transforms."""
import ctypes

import numpy as np
import pytest

import ransac_ref as R
from test_match_spec import _BAD_SCENE, _FRAG, _PAIRS, _TGT, _DEV, _arr, _dev, _ids, _ptr

EINVAL, EWORKSPACE, ENULL = -1, -2, -3
SYMBOLS = ("epn_ransac_register_workspace_bytes", "epn_ransac_register_f64")
NAMES = ("register_scene", "register_fragment_pair", "registration_errors", "registration_recall", "RegistrationResult")


def test_symbols_resolve_and_are_bound_at_every_layer():
    import epn_pointcloud_amd
    from epn_pointcloud_amd import _lib, matching
    from epn_pointcloud_amd.vgtk.cuda import grouping
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in _lib.EXPORTS
        assert hasattr(cdll, name)
    assert callable(grouping.ransac_register)
    for name in NAMES:
        assert getattr(epn_pointcloud_amd, name) is getattr(matching, name)
    assert matching.RegistrationResult._fields == ("T", "n_match", "n_inlier", "rmse", "margin", "best_h")
    assert _lib.get_lib().epn_abi_version() == 3


def _ws(n):
    return (24 * n + 7) // 8 * 8 + 4 * 32768


def test_workspace_query_is_24_bytes_per_tgt_row_and_the_pair_counts():
    from epn_pointcloud_amd import _lib
    q = _lib.get_lib().epn_ransac_register_workspace_bytes
    for n in (0, 1, 2, 3, 580, 10 ** 6, 2 ** 33 + 3):
        assert q(n) == _ws(n) and q(n) % 8 == 0
    assert q(-1) == 0


# The valid scene of tests/test_match_spec.py: F = 3 fragments of 4, 0 and 6 rows, P = 2 pairs.  Device pointers are non-NULL
# and never dereferenced: every call below is refused, or has nothing to launch.
def _reg(**over):
    from epn_pointcloud_amd import _lib
    a = dict(kp=_DEV, R=10, F=3, frag=_FRAG, frag_d=_DEV, P=2, pairs=_PAIRS, pairs_d=_DEV, tgt=_TGT, tgt_d=_DEV, msrc=_DEV, tau=0.05,
             H=64, seed=7, pair0=0, min_margin=1e-2, ws=_DEV, ws_bytes=_ws(10), T=_DEV, best_h=_DEV, hyp_count=_DEV, n_inlier=_DEV,
             rmse=_DEV, margin=_DEV)
    a.update(over)
    frag, pairs, tgt = _arr(a["frag"], np.int64), _arr(a["pairs"], np.int32), _arr(a["tgt"], np.int64)
    return _lib.get_lib().epn_ransac_register_f64(_dev(a["kp"]), a["R"], a["F"], _ptr(frag), _dev(a["frag_d"]), a["P"], _ptr(pairs),
                                                  _dev(a["pairs_d"]), _ptr(tgt), _dev(a["tgt_d"]), _dev(a["msrc"]), a["tau"], a["H"],
                                                  a["seed"], a["pair0"], a["min_margin"], _dev(a["ws"]), a["ws_bytes"], _dev(a["T"]),
                                                  _dev(a["best_h"]), _dev(a["hyp_count"]), _dev(a["n_inlier"]), _dev(a["rmse"]),
                                                  _dev(a["margin"]), None)


# the scene-table refusals of the matching entries, without the rows about out_off (this entry does not take that table)
_SCENE = [(bad, code) for bad, code in _BAD_SCENE if not ({"out", "out_d", "nn_idx"} & set(bad))]
_NAN, _INF = float("nan"), float("inf")


@pytest.mark.parametrize("bad,code", _SCENE + [
    (dict(H=0), EINVAL), (dict(H=-1), EINVAL), (dict(H=65537), EINVAL),
    (dict(tau=_NAN), EINVAL), (dict(tau=0.0), EINVAL), (dict(tau=-0.05), EINVAL), (dict(tau=_INF), EINVAL),
    (dict(min_margin=-1e-3), EINVAL), (dict(min_margin=1.0), EINVAL), (dict(min_margin=_NAN), EINVAL), (dict(pair0=-1), EINVAL),
    (dict(tgt=[0, 6, 11]), EINVAL), (dict(tgt=[0, 4, 10]), EINVAL), (dict(tgt=None), ENULL), (dict(tgt_d=0), ENULL),
    (dict(kp=0), ENULL), (dict(msrc=0), ENULL), (dict(T=0), ENULL), (dict(best_h=0), ENULL), (dict(hyp_count=0), ENULL),
    (dict(n_inlier=0), ENULL), (dict(rmse=0), ENULL), (dict(margin=0), ENULL),
    (dict(ws=0), EWORKSPACE), (dict(ws_bytes=_ws(10) - 1), EWORKSPACE)], ids=_ids)
def test_ransac_register_refuses_bad_arguments_before_any_runtime_call(bad, code):
    assert len(_SCENE) == 15
    assert _reg(**bad) == code


def test_the_range_ends_are_accepted_and_nothing_to_do_launches_nothing():
    none = dict(P=0, pairs=None, pairs_d=0, tgt=[0], kp=0, msrc=0, ws=0, ws_bytes=0, T=0, best_h=0, hyp_count=0, n_inlier=0, rmse=0,
                margin=0)
    assert _reg(**none) == 0
    for ok in (dict(H=1), dict(H=65536), dict(min_margin=0.0), dict(min_margin=0.999), dict(seed=2 ** 64 - 1), dict(pair0=2 ** 40)):
        assert _reg(**none, **ok) == 0
    assert _reg(**none, H=0) == EINVAL and _reg(**none, tau=_NAN) == EINVAL          # the other checks still hold


def test_the_restatement_recovers_a_planted_transform_at_30_percent_inliers():
    case = R.planted_case(share=0.3, H=1024)
    ref = case["ref"]
    rre, rte = R.registration_errors(ref["T"][0], case["gt"][0])
    assert rre < 1.0 and rte < 0.02
    assert 0.25 * ref["n_corr"][0] <= ref["n_inlier"][0] <= 0.35 * ref["n_corr"][0] and ref["rmse"][0] < 2.0 * R.NOISE
    T = ref["T"][0]
    assert np.abs(T[:3, :3].T @ T[:3, :3] - np.eye(3)).max() <= 1e-14 and np.array_equal(T[3], [0, 0, 0, 1])


def test_the_restatement_on_degenerate_pairs():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 3))
    failed = R.register_pair(x, x, 0.05, 16, 0, 0, 1e-2)                                 # two matches: every hypothesis rejected
    assert failed["best_h"] == -1 and (failed["hyp_count"] == -1).all() and np.array_equal(failed["T"], np.eye(4))
    assert failed["n_inlier"] == 0 and failed["rmse"] == np.inf and failed["margin"] == 0.0
    line = np.outer(np.arange(6.0), [1.0, 2.0, -1.0])                                    # collinear: margin 0, all rejected
    assert (R.register_pair(line, line, 0.05, 64, 0, 0, 1e-2)["hyp_count"] == -1).all()
    idx = R.draws(3, 4096, 5, 9)                                                         # M = 3: 6 of 27 draws are distinct
    distinct = (idx[:, 0] != idx[:, 1]) & (idx[:, 0] != idx[:, 2]) & (idx[:, 1] != idx[:, 2])
    assert abs(distinct.mean() - 6 / 27) < 5 * np.sqrt(6 / 27 * 21 / 27 / 4096) and idx.min() == 0 and idx.max() == 2
    assert not np.array_equal(R.draws(600, 8, 0, 9), R.draws(600, 8, 1, 9))              # the pair is a counter word


def test_registration_errors_on_hand_made_transforms():
    from epn_pointcloud_amd import matching
    I = np.eye(4)
    turn = np.eye(4)
    turn[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]                                    # 90 degrees about z
    shift = np.eye(4)
    shift[:3, 3] = [0.3, -0.4, 1.2]
    both = turn @ shift
    rre, rte = matching.registration_errors(np.stack([I, turn, shift, both, both]), np.stack([I, I, I, I, both]))
    assert np.allclose(rre, [0, 90, 0, 90, 0], atol=1e-12) and np.allclose(rte, [0, 0, 1.3, np.linalg.norm(both[:3, 3]), 0], atol=1e-12)
    one = matching.registration_errors(turn, I)
    assert one[0].shape == (1,) and abs(one[0][0] - 90) < 1e-12
    assert matching.registration_recall(np.stack([I, turn, shift, both]), np.stack([I] * 4)) == 0.25
    assert matching.registration_recall(np.stack([I, turn, shift]), np.stack([I] * 3), rre_deg=91.0, rte=1.31) == 1.0
    assert matching.registration_recall(np.zeros((0, 4, 4)), np.zeros((0, 4, 4))) == 0.0
    with pytest.raises(ValueError):
        matching.registration_errors(np.stack([I, I]), I)
    assert R.registration_errors(both, I) == pytest.approx((90.0, float(np.linalg.norm(both[:3, 3]))))
