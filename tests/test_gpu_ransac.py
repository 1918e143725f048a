"""Pairwise registration on the GPU (csrc/ransac_register.hip through vgtk.cuda.grouping.ransac_register and
epn_pointcloud_amd.matching.register_scene) against tests/ransac_ref.py, the numpy restatement of the specification (draws
through philox_ref, fits through numpy's SVD).

Shapes: one scene of six pairs with M_p = 0, 2, 3, 65, 257, 600 correspondences (an empty pair and a two-match pair between
live ones; the least that can succeed; one past a wave; one past the 256-correspondence LDS tile; more than two tiles) at
H = 1, 257 (one past a 256-hypothesis workgroup) and 1024.
Exact: hyp_count (every entry, the -1 of a rejected hypothesis included), best_h and n_inlier equal the restatement's.  That is
legitimate because every case builder asserts on the CPU that no decision sits within 1e-9 of its threshold (ransac_ref's
docstring), and two fp64 evaluations of a three-point fit with margin >= 1e-2 differ by far less.
Tolerance: T, rmse and margin within 1e-9 absolute.  From |dR| <= 2 |dC| / (s1 margin) with |dC| / s1 <= 4 (n + 3) u rho for two
evaluations (tests/test_ransac_host.py) and |dt| <= 3 |dR| |ybar| + (n + 4) u (|xbar| + 3 |ybar|): with n <= 600, rho <= 10 and
margin >= 1e-2 that is |dR| <= 5.4e-10 and, for |ybar| <= 0.28, the same 1e-9 for t.  The builders do not rely on those round
figures: they evaluate this bound for every pair that succeeds (ransac_ref.fit_bound) and assert it is at most 1e-9, next to
coordinates <= 10 and refit margins >= 1e-2."""
import numpy as np
import pytest
import torch

import ransac_ref as R

pytestmark = pytest.mark.gpu
T_ = torch.from_numpy
TOL = R.T_TOL


def run(gpu, case, match_src=None, H=None, seed=None, pair0=0, pairs=None, kp=None, frag_off=None, tgt_off=None):
    from epn_pointcloud_amd.vgtk.cuda import grouping
    ms = case["match_src"] if match_src is None else match_src
    out = grouping.ransac_register(T_(case["kp"] if kp is None else kp).to(gpu), case["frag_off"] if frag_off is None else frag_off,
                                   case["pairs"] if pairs is None else pairs, T_(ms).to(gpu),
                                   case["tgt_off"] if tgt_off is None else tgt_off, R.TAU, case["H"] if H is None else H,
                                   case["seed"] if seed is None else seed, R.MIN_MARGIN, pair0=pair0)
    keys = ("T", "best_h", "hyp_count", "n_inlier", "rmse", "margin")
    return {k: v.cpu().numpy() for k, v in zip(keys, out)}


def check(got, ref, pairs=None):
    """Every output of the entry against the restatement's, for the listed pairs (default: all)."""
    P = ref["best_h"].shape[0]
    for p in range(P) if pairs is None else pairs:
        assert np.array_equal(got["hyp_count"][p], ref["hyp_count"][p]), p
        assert got["best_h"][p] == ref["best_h"][p] and got["n_inlier"][p] == ref["n_inlier"][p], p
        T = got["T"][p]
        assert np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0])
        assert np.abs(T[:3, :3].T @ T[:3, :3] - np.eye(3)).max() <= 1e-12 and np.linalg.det(T[:3, :3]) > 0
        if ref["best_h"][p] < 0:                              # a failed pair: the defined record, exactly
            assert np.array_equal(T, np.eye(4)) and got["n_inlier"][p] == 0 and got["rmse"][p] == np.inf and got["margin"][p] == 0.0
        else:
            assert ref["margin"][p] >= R.MIN_REFIT_MARGIN
            assert np.abs(T - ref["T"][p]).max() <= TOL, (p, np.abs(T - ref["T"][p]).max())
            assert abs(got["rmse"][p] - ref["rmse"][p]) <= TOL and abs(got["margin"][p] - ref["margin"][p]) <= TOL, p


@pytest.mark.parametrize("H", R.H_SET)
def test_six_pairs_from_empty_to_three_tiles(gpu, H):
    case = R.six_pair_case(H)
    got = run(gpu, case)
    assert got["hyp_count"].shape == (6, H) and got["T"].shape == (6, 4, 4)
    check(got, case["ref"])
    assert (got["hyp_count"][:2] == -1).all() and (got["best_h"][:2] == -1).all()       # M = 0 and M = 2 fail
    assert got["best_h"][2] >= 0 and got["n_inlier"][2] == 3                            # M = 3 succeeds
    if H > 1:
        assert (got["best_h"][3:] >= 0).all()
        for p in range(3, 6):                                 # and what succeeded found the planted motion
            rre, rte = R.registration_errors(got["T"][p], case["gt"][p])
            assert rre < 1.0 and rte < 0.02


def test_ties_go_to_the_lowest_hypothesis(gpu):
    case = R.tie_case()
    got = run(gpu, case)
    check(got, case["ref"])
    for p in range(2):
        c = got["hyp_count"][p]
        assert (c == c.max()).sum() >= 2 and got["best_h"][p] == np.flatnonzero(c == c.max())[0]


def test_a_pair_without_inliers_between_live_pairs(gpu):
    case = R.outlier_case()
    got = run(gpu, case)
    check(got, case["ref"])
    assert np.isfinite(got["T"]).all() and not np.isnan(got["rmse"]).any() and not np.isnan(got["margin"]).any()


def test_out_of_range_match_rows_are_dropped_and_touch_no_other_pair(gpu):
    case = R.six_pair_case(257)
    clean = run(gpu, case)
    ms = case["match_src"].copy()
    off, fo = case["tgt_off"], case["frag_off"]
    rows = off[4] + np.flatnonzero(ms[off[4]:off[5]] >= 0)[[0, 7, 100, 256]]            # pair 4 (M = 257): four of its matches
    n_src = int(fo[2 * 4 + 1] - fo[2 * 4])
    ms[rows] = [n_src, n_src + 5, 2 ** 31 - 1, 10 ** 6]
    ref = R.register(case["kp"], fo, case["pairs"], ms, off, R.TAU, 257, case["seed"], R.MIN_MARGIN)
    assert ref["n_corr"][4] == 253 and not R.check_conditions(ref, (2, 3, 4, 5))
    got = run(gpu, case, match_src=ms)
    check(got, ref)
    assert not np.array_equal(got["hyp_count"][4], clean["hyp_count"][4])               # the rows did take part before
    for k in got:
        for p in (0, 1, 2, 3, 5):
            assert got[k][p].tobytes() == clean[k][p].tobytes(), (k, p)


def test_two_runs_are_bitwise_equal(gpu):
    case = R.six_pair_case(1024)
    a, b = run(gpu, case), run(gpu, case)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_a_pair_alone_equals_the_pair_in_its_batch(gpu):
    """Pair p of a call draws with the counter word pair0 + p: the pair alone, called with pair0 = p, is the same computation."""
    case = R.six_pair_case(257)
    batch = run(gpu, case)
    fo, off = case["frag_off"], case["tgt_off"]
    for p in range(6):
        kp = np.ascontiguousarray(case["kp"][fo[2 * p]:fo[2 * p + 2]])
        one = run(gpu, case, match_src=np.ascontiguousarray(case["match_src"][off[p]:off[p + 1]]), pair0=p, pairs=[[0, 1]], kp=kp,
                  frag_off=fo[2 * p:2 * p + 3] - fo[2 * p], tgt_off=off[p:p + 2] - off[p])
        for k in batch:
            assert one[k][0].tobytes() == batch[k][p].tobytes(), (k, p)
    other = run(gpu, case, pair0=1)                           # and the counter word does enter the draw
    assert not np.array_equal(other["hyp_count"][5], batch["hyp_count"][5])


def test_describe_then_register_end_to_end(gpu):
    """Plumbing: two overlapping fragments of one cloud -> describe() -> register_scene runs without ground truth, returns a
    rotation for every pair, and equals the restatement run on the same match_src."""
    from epn_pointcloud_amd import matching, models as M
    from epn_pointcloud_amd.vgtk.cuda import grouping
    from test_models_cpu import fill_state_dict
    rng = np.random.default_rng(8)
    cloud = rng.uniform(-1, 1, (4000, 3)).astype(np.float32)
    src_pc, tgt_pc = cloud[:3000], cloud[1000:]               # the middle 2000 points are shared; the true motion is the identity
    rows = rng.choice(np.arange(1000, 3000), 12, replace=False)
    src_kp, tgt_kp = cloud[rows].copy(), cloud[rows[::-1]].copy()
    src_kp[4] = 9.0                                           # far outside: describe() marks them invalid
    tgt_kp[7] = -9.0
    m = fill_state_dict(M.build_inv(input_num=1024, search_radius=0.8, width_div=2)).to(gpu).eval()
    dev = lambda x: T_(x).to(gpu)
    sd, sv = m.describe(dev(src_pc), dev(src_kp), batch=4, seed=3)
    td, tv = m.describe(dev(tgt_pc), dev(tgt_kp), batch=4, seed=3)
    kps, feats, valids, pairs = [dev(src_kp), dev(tgt_kp)], [sd, td], [sv, tv], [[0, 1], [1, 0]]
    H, seed = 256, 5
    res = matching.register_scene(kps, feats, valids, pairs, tau=0.05, hypotheses=H, seed=seed, min_margin=1e-2)
    assert isinstance(res, matching.RegistrationResult) and res.T.shape == (2, 4, 4)
    for T in res.T:
        assert np.abs(T[:3, :3].T @ T[:3, :3] - np.eye(3)).max() <= 1e-12 and np.array_equal(T[3], [0, 0, 0, 1])
    # the restatement on the same match_src
    frag_off = np.array([0, 12, 24], np.int64)
    all_kps, all_feats, valid = torch.cat(kps), torch.cat(feats), torch.cat([sv, tv]).to(torch.uint8)
    nn_idx, _, _ = grouping.nn_match(all_feats, frag_off, pairs, valid)
    match_src, _, n_match, _, tgt_off = grouping.match_inliers(all_kps, frag_off, pairs, nn_idx, np.tile(np.eye(4), (2, 1, 1)), 0.0)
    ref = R.register(all_kps.cpu().numpy(), frag_off, np.asarray(pairs), match_src.cpu().numpy(), tgt_off.numpy(), 0.05, H, seed, 1e-2)
    assert np.array_equal(res.n_match, n_match.cpu().numpy()) and np.array_equal(res.n_match, ref["n_corr"])
    assert np.array_equal(res.best_h, ref["best_h"]) and np.array_equal(res.n_inlier, ref["n_inlier"])
    for p in range(2):
        if ref["best_h"][p] >= 0 and ref["margin"][p] >= R.MIN_REFIT_MARGIN:
            assert np.abs(res.T[p] - ref["T"][p]).max() <= TOL and abs(res.rmse[p] - ref["rmse"][p]) <= TOL
            assert abs(res.margin[p] - ref["margin"][p]) <= TOL
    one = matching.register_fragment_pair(kps[0], kps[1], sd, td, tau=0.05, hypotheses=H, seed=seed, src_valid=sv, tgt_valid=tv)
    assert one[0].tobytes() == res.T[0].tobytes() and one[1:] == (int(res.n_match[0]), int(res.n_inlier[0]), float(res.rmse[0]),
                                                                  float(res.margin[0]), int(res.best_h[0]))
