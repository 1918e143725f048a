"""Descriptor matching without a GPU: the entry points exist at every layer, every argument refusal is decided on the host
before any HIP runtime call, the workspace query follows its formula, and the specification's numpy restatement
(tests/match_ref.py) agrees with what the reference runs -- sklearn's KDTree for the neighbours, and the golden fixture
(tests/golden/match_pair.npz, the reference's evaluate_fragment_pair on one synthetic pair) for the inlier step."""
import ctypes

import numpy as np
import pytest

import match_ref as R
from conftest import golden

EINVAL, EWORKSPACE, ENULL = -1, -2, -3
SYMBOLS = ("epn_nn_match_workspace_bytes", "epn_nn_match_f32", "epn_match_inliers_f64")


def test_symbols_resolve_and_are_bound_at_every_layer():
    import epn_pointcloud_amd
    from epn_pointcloud_amd import _lib, matching
    from epn_pointcloud_amd.vgtk.cuda import grouping
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in _lib.EXPORTS
        assert hasattr(cdll, name)
    assert callable(grouping.nn_match) and callable(grouping.match_inliers)
    for name in ("match_descriptors", "evaluate_fragment_pair", "evaluate_scene"):
        assert getattr(epn_pointcloud_amd, name) is getattr(matching, name)
    assert _lib.get_lib().epn_abi_version() == 3


def test_workspace_query_is_eight_bytes_per_output_row():
    from epn_pointcloud_amd import _lib
    q = _lib.get_lib().epn_nn_match_workspace_bytes
    for n in (0, 1, 2, 580, 10 ** 6, 2 ** 33 + 3):
        assert q(n) == 8 * n
    assert q(-1) == 0


# A valid scene: F = 3 fragments of 4, 0 and 6 rows, P = 2 pairs.  Device pointers are non-NULL and never dereferenced: every
# call below is refused, or has nothing to launch.
_FRAG = [0, 4, 4, 10]
_PAIRS = [[0, 2], [2, 0]]
_OUT = [0, 10, 20]
_TGT = [0, 6, 10]
_DEV = 64


def _arr(x, dt):
    return None if x is None else np.ascontiguousarray(np.asarray(x, dtype=dt))


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _dev(v):
    return ctypes.c_void_p(v) if v else None


def _nn(**over):
    from epn_pointcloud_amd import _lib
    a = dict(feats=_DEV, R=10, C=64, valid=0, F=3, frag=_FRAG, frag_d=_DEV, P=2, pairs=_PAIRS, pairs_d=_DEV, out=_OUT, out_d=_DEV,
             ws=_DEV, ws_bytes=8 * 20, nn_idx=_DEV, nn_d2=_DEV)
    a.update(over)
    frag, pairs, out = _arr(a["frag"], np.int64), _arr(a["pairs"], np.int32), _arr(a["out"], np.int64)
    return _lib.get_lib().epn_nn_match_f32(_dev(a["feats"]), a["R"], a["C"], _dev(a["valid"]), a["F"], _ptr(frag), _dev(a["frag_d"]),
                                           a["P"], _ptr(pairs), _dev(a["pairs_d"]), _ptr(out), _dev(a["out_d"]), _dev(a["ws"]),
                                           a["ws_bytes"], _dev(a["nn_idx"]), _dev(a["nn_d2"]), None)


def _inl(**over):
    from epn_pointcloud_amd import _lib
    a = dict(kp=_DEV, R=10, F=3, frag=_FRAG, frag_d=_DEV, P=2, pairs=_PAIRS, pairs_d=_DEV, out=_OUT, out_d=_DEV, tgt=_TGT, tgt_d=_DEV,
             nn_idx=_DEV, gt=_DEV, tau1=0.1, msrc=_DEV, mdist=_DEV, n_match=_DEV, n_inlier=_DEV)
    a.update(over)
    frag, pairs, out, tgt = (_arr(a["frag"], np.int64), _arr(a["pairs"], np.int32), _arr(a["out"], np.int64),
                             _arr(a["tgt"], np.int64))
    return _lib.get_lib().epn_match_inliers_f64(_dev(a["kp"]), a["R"], a["F"], _ptr(frag), _dev(a["frag_d"]), a["P"], _ptr(pairs),
                                                _dev(a["pairs_d"]), _ptr(out), _dev(a["out_d"]), _ptr(tgt), _dev(a["tgt_d"]),
                                                _dev(a["nn_idx"]), _dev(a["gt"]), a["tau1"], _dev(a["msrc"]), _dev(a["mdist"]),
                                                _dev(a["n_match"]), _dev(a["n_inlier"]), None)


_BAD_SCENE = [
    (dict(R=-1), EINVAL), (dict(R=11), EINVAL), (dict(F=0), EINVAL), (dict(P=-1), EINVAL), (dict(P=32768), EINVAL),
    (dict(frag=[1, 4, 4, 10]), EINVAL), (dict(frag=[0, 5, 4, 10]), EINVAL), (dict(frag=[0, 4, 4, 9]), EINVAL),
    (dict(pairs=[[0, 3], [2, 0]]), EINVAL), (dict(pairs=[[-1, 2], [2, 0]]), EINVAL), (dict(pairs=[[0, 2], [2, 2]]), EINVAL),
    (dict(out=[0, 10, 21]), EINVAL), (dict(out=[1, 10, 20]), EINVAL), (dict(out=[0, 6, 20]), EINVAL),
    (dict(frag=None), ENULL), (dict(pairs=None), ENULL), (dict(out=None), ENULL),
    (dict(frag_d=0), ENULL), (dict(pairs_d=0), ENULL), (dict(out_d=0), ENULL), (dict(nn_idx=0), ENULL),
]
_ids = lambda v: "-".join(f"{k}={x}" for k, x in v.items()).replace(" ", "") if isinstance(v, dict) else str(v)


@pytest.mark.parametrize("bad,code", _BAD_SCENE + [
    (dict(C=0), EINVAL), (dict(C=129), EINVAL), (dict(feats=0), ENULL), (dict(nn_d2=0), ENULL),
    (dict(ws=0), EWORKSPACE), (dict(ws_bytes=8 * 20 - 1), EWORKSPACE)], ids=_ids)
def test_nn_match_refuses_bad_arguments_before_any_runtime_call(bad, code):
    assert _nn(**bad) == code


@pytest.mark.parametrize("bad,code", _BAD_SCENE + [
    (dict(tau1=float("nan")), EINVAL), (dict(tgt=[0, 6, 11]), EINVAL), (dict(tgt=[0, 4, 10]), EINVAL), (dict(tgt=None), ENULL),
    (dict(tgt_d=0), ENULL), (dict(kp=0), ENULL), (dict(gt=0), ENULL), (dict(msrc=0), ENULL), (dict(mdist=0), ENULL),
    (dict(n_match=0), ENULL), (dict(n_inlier=0), ENULL)], ids=_ids)
def test_match_inliers_refuses_bad_arguments_before_any_runtime_call(bad, code):
    assert _inl(**bad) == code


def test_nothing_to_do_is_success_and_launches_nothing():
    none = dict(P=0, pairs=None, pairs_d=0, out=[0], tgt=[0])
    assert _nn(**{k: v for k, v in none.items() if k != "tgt"}, feats=0, ws=0, ws_bytes=0, nn_idx=0, nn_d2=0) == 0
    assert _inl(**none, kp=0, nn_idx=0, gt=0, msrc=0, mdist=0, n_match=0, n_inlier=0) == 0
    empty = dict(R=0, F=2, frag=[0, 0, 0], P=1, pairs=[[0, 1]], out=[0, 0])           # a pair of empty fragments
    assert _nn(**empty, feats=0, ws=0, ws_bytes=0, nn_idx=0, nn_d2=0) == 0
    assert _nn(P=0, pairs=None, out=[0], C=0) == EINVAL                              # the other checks still hold


@pytest.mark.parametrize("sizes,C,seed", [((300, 280), 64, 1), ((65, 257), 32, 2), ((1000, 1000), 64, 3)])
def test_match_ref_agrees_with_the_kdtree_the_reference_uses(sizes, C, seed):
    """evaluation_3dmatch.py:77-84 restated: KDTree(tgt).query(src, k=1) and the reverse.  sklearn measures in fp64 on the same
    float32 rows, from the differences, as match_ref does: the same row and the same distance."""
    KDTree = pytest.importorskip("sklearn.neighbors").KDTree
    feats, off = R.unit_scene(sizes, C, seed)
    a, b = feats[off[0]:off[1]], feats[off[1]:off[2]]
    for q, t in ((a, b), (b, a)):
        idx, d2, _ = R.nearest(q, t)
        dist, nn = KDTree(t).query(q, k=1)
        assert np.array_equal(nn.squeeze(1), idx)
        assert np.allclose(dist.squeeze(1) ** 2, d2, rtol=1e-12, atol=1e-300)


def test_match_ref_inlier_step_against_the_golden_pair():
    g = golden("match_pair.npz")
    n_inlier, ratio, matches, dist = R.evaluate_fragment_pair(g["src_kp"], g["tgt_kp"], g["src_feats"], g["tgt_feats"], g["gt"],
                                                              float(g["tau1"]))
    assert n_inlier == int(g["n_inlier"]) and matches.shape[0] == int(g["n_match"])
    assert ratio == float(g["inlier_ratio"])
    assert np.array_equal(matches[dist < float(g["tau1"])], g["inlier_pairs"])
    n = g["tgt_feats"].shape[0]
    assert 0.3 * n <= matches.shape[0] <= 0.8 * n and 0 < n_inlier < matches.shape[0]       # the fixture discriminates
    assert (np.abs(dist - float(g["tau1"])) > 1e-6 * float(g["tau1"])).all()


def test_masks_and_nan_rows_in_the_specification():
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal((6, 4)).astype(np.float32), rng.standard_normal((5, 4)).astype(np.float32)
    b[2] = np.nan
    a[3] = np.nan
    bv = np.array([1, 1, 1, 0, 1], bool)
    av = np.array([1, 0, 1, 1, 1, 1], bool)
    idx, d2, _ = R.nearest(a, b, av, bv)
    assert idx[1] == -1 and idx[3] == -1 and np.isinf(d2[[1, 3]]).all()
    assert not np.isin(idx, (2, 3)).any() and (idx[[0, 2, 4, 5]] >= 0).all()
    idx, _, _ = R.nearest(a, b, None, np.zeros(5, bool))
    assert (idx == -1).all()
    b[:] = b[0]                                            # all candidates tie: the lowest admissible index
    b[2] = np.nan
    assert (R.nearest(a[:1], b, None, np.array([0, 1, 1, 1, 1], bool))[0] == 1).all()
