"""Descriptor matching on the GPU (csrc/desc_match.hip through vgtk.cuda.grouping and epn_pointcloud_amd.matching) against
tests/match_ref.py, the numpy restatement of the specification (fp64 distances, first-minimum ties, masks).

Shapes: (n_src, n_tgt) from one row to more than one query tile (256 rows) and three target segments (512 rows), every C
that takes another kernel instance (8, 32, 64, 128 wide) or a padded width (1, 5).
Exact cases: descriptors on the grid of multiples of 2^-8 in [-1, 1]; every d2 is then a multiple of 2^-16, below 2^8 on these
inputs (asserted), and exact in fp32 in any summation order -- indices and distances must equal the reference bit for bit,
ties (duplicated rows, also across a segment boundary) included.
Generic unit rows: with j the kernel's choice, j* the fp64 arg-min and gamma = (C + 3) 2^-23 (each difference and square
carries three roundings and the sum C - 1, all on non-negative terms: first order (C + 3) 2^-24, doubled for the higher
orders): d64(i,j) <= d64(i,j*) (1 + gamma) / (1 - gamma) and |nn_d2 - d64(i,j)| <= gamma d64(i,j) for every row, and j == j*
wherever the fp64 runner-up gap exceeds 2 gamma."""
import functools

import numpy as np
import pytest
import torch

import match_ref as R
from conftest import golden

pytestmark = pytest.mark.gpu
T = torch.from_numpy

SIZES = [(1, 1), (63, 65), (256, 257), (300, 280), (700, 1300)]
CHANNELS = [1, 5, 32, 64, 128]
FOUR = (300, 65, 700, 280)                                    # F = 4 fragments of unequal sizes
FIVE = [[0, 1], [1, 0], [2, 0], [3, 2], [1, 3]]               # fragment 0 is src and tgt; (0, 1) in both orders


@functools.lru_cache(maxsize=None)
def exact_case(sizes, C):
    feats, off = R.quantised_scene(sizes, C, seed=100 * sizes[0] + C)
    pairs = FIVE if len(sizes) == 4 else [[0, 1]]
    return feats, off, pairs, R.nn_match(feats, off, pairs)


@functools.lru_cache(maxsize=None)
def unit_case(sizes, C):
    feats, off = R.unit_scene(sizes, C, seed=7 * sizes[0] + C)
    return feats, off


def on_grid(feats):
    """Unit-scene descriptors moved onto the 2^-8 grid: the neighbour structure of the noisy copies with exact arithmetic."""
    return (np.round(feats.astype(np.float64) * 256.0) / 256.0).astype(np.float32)


def run_nn(gpu, feats, off, pairs, valid=None):
    from epn_pointcloud_amd.vgtk.cuda import grouping
    v = None if valid is None else T(valid.astype(np.uint8)).to(gpu)
    idx, d2, out_off = grouping.nn_match(T(feats).to(gpu), off, pairs, v)
    return idx.cpu().numpy(), d2.cpu().numpy(), out_off.numpy()


@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("sizes", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_exact_distances_match_bit_for_bit(gpu, sizes, C):
    feats, off, pairs, (ref_idx, ref_d2, ref_off) = exact_case(sizes, C)
    idx, d2, out_off = run_nn(gpu, feats, off, pairs)
    assert ref_d2.max() < 256.0 and np.array_equal(ref_d2.astype(np.float32).astype(np.float64), ref_d2)   # lossless in fp32
    assert np.array_equal(out_off, ref_off)
    assert np.array_equal(idx, ref_idx)
    assert d2.tobytes() == ref_d2.astype(np.float32).tobytes()
    if min(sizes) > 2:                                      # the duplicated rows were in play: a zero distance, lowest index
        assert (ref_d2 == 0).any()


@pytest.mark.parametrize("C", [5, 64])
def test_exact_scene_of_four_fragments_and_five_pairs(gpu, C):
    feats, off, pairs, (ref_idx, ref_d2, ref_off) = exact_case(FOUR, C)
    idx, d2, out_off = run_nn(gpu, feats, off, pairs)
    assert np.array_equal(out_off, ref_off) and np.array_equal(idx, ref_idx)
    assert d2.tobytes() == ref_d2.astype(np.float32).tobytes()
    n0, n1 = FOUR[0], FOUR[1]                               # (0, 1) and (1, 0): the same neighbours, blocks swapped
    assert np.array_equal(idx[:n0], idx[ref_off[1] + n1:ref_off[2]]) and np.array_equal(idx[n0:ref_off[1]], idx[ref_off[1]:ref_off[1] + n1])


def _check_generic(idx, d2, q, t, C):
    """The docstring's properties for the rows of q against the rows of t; no row is left out."""
    gamma = (C + 3) * 2.0 ** -23
    D = R.d2_matrix(q, t)
    star = np.argmin(D, axis=1)
    rows = np.arange(q.shape[0])
    assert (idx >= 0).all() and (idx < t.shape[0]).all()
    chosen, best = D[rows, idx], D[rows, star]
    assert (chosen <= best * (1 + gamma) / (1 - gamma)).all()
    assert (np.abs(d2.astype(np.float64) - chosen) <= gamma * chosen).all()
    if t.shape[0] > 1:
        runner_up = np.partition(D, 1, axis=1)[:, 1]
        clear = (runner_up - best) > 2 * gamma * best
        assert np.array_equal(idx[clear], star[clear])
        assert C == 1 or clear.mean() > 0.9                 # C = 1: unit rows are +-1 and every distance ties
    return gamma


@pytest.mark.parametrize("sizes,C", [((300, 280), 64), ((65, 257), 32), ((700, 1300), 64), ((256, 257), 1), ((256, 257), 5),
                                     ((256, 257), 128), ((1, 1), 64)], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_generic_unit_descriptors_within_the_derived_bound(gpu, sizes, C):
    feats, off = unit_case(sizes, C)
    idx, d2, out_off = run_nn(gpu, feats, off, [[0, 1]])
    a, b = feats[:off[1]], feats[off[1]:]
    _check_generic(idx[:sizes[0]], d2[:sizes[0]], a, b, C)
    _check_generic(idx[sizes[0]:], d2[sizes[0]:], b, a, C)


def test_masks_and_nan_rows(gpu):
    feats, off = unit_case(FOUR, 32)
    feats = on_grid(feats)                                  # exact distances: the indices must equal the reference's
    rng = np.random.default_rng(9)
    valid = rng.random(feats.shape[0]) > 0.3
    valid[off[1]:off[2]] = False                            # fragment 1: every row invalid
    feats[~valid] = 0.0                                     # what describe() hands over
    nan_rows = off[2] + np.array([0, 5, 511, 512, 699])     # fragment 2: NaN rows, marked valid
    feats[nan_rows] = np.nan
    valid[nan_rows] = True
    ref_idx, ref_d2, ref_off = R.nn_match(feats, off, FIVE, valid)
    idx, d2, out_off = run_nn(gpu, feats, off, FIVE, valid)
    assert np.array_equal(idx, ref_idx)
    assert np.array_equal(np.isinf(d2), idx < 0) and (d2[idx < 0] > 0).all()
    for p, (s, t) in enumerate(FIVE):
        ns, nt = FOUR[s], FOUR[t]
        blocks = ((idx[ref_off[p]:ref_off[p] + ns], s, t), (idx[ref_off[p] + ns:ref_off[p + 1]], t, s))
        for got, fq, fc in blocks:
            vq, vc = valid[off[fq]:off[fq + 1]], valid[off[fc]:off[fc + 1]]
            nan_q = np.isnan(feats[off[fq]:off[fq + 1]]).any(axis=1)
            nan_c = np.isnan(feats[off[fc]:off[fc + 1]]).any(axis=1)
            assert (got[~vq] == -1).all() and (got[nan_q] == -1).all()
            hit = got[got >= 0]
            assert vc[hit].all() and not nan_c[hit].any()
            if fc == 1:
                assert (got == -1).all()
            elif fq != 1:
                assert (got[vq & ~nan_q] >= 0).all()


def _scene_inputs(gpu, C=32):
    feats, off = unit_case(FOUR, C)
    feats = on_grid(feats)                                  # exact distances: the matches must equal the reference's
    rng = np.random.default_rng(21)
    kp = rng.uniform(0, 2, (feats.shape[0], 3)).astype(np.float32)
    gts = []
    for _ in FIVE:
        q, _r = np.linalg.qr(rng.standard_normal((3, 3)))
        g = np.eye(4)
        g[:3, :3], g[:3, 3] = q * np.sign(np.linalg.det(q)), rng.uniform(-0.2, 0.2, 3)
        gts.append(g)
    frag = lambda x: [T(np.ascontiguousarray(x[off[f]:off[f + 1]])).to(gpu) for f in range(4)]
    return feats, off, kp, np.stack(gts), frag


def test_inliers_equal_the_reference_per_pair_and_batching_changes_nothing(gpu):
    from epn_pointcloud_amd import matching
    feats, off, kp, gts, frag = _scene_inputs(gpu)
    tau1 = 1.0                                              # random keypoints in a 2 m box: both outcomes occur
    for _ in range(20):                                     # keep every matched distance off the tau1 boundary (fp64, CPU)
        refs = [R.evaluate_fragment_pair(kp[off[s]:off[s + 1]], kp[off[t]:off[t + 1]], feats[off[s]:off[s + 1]],
                                         feats[off[t]:off[t + 1]], gts[p], tau1) for p, (s, t) in enumerate(FIVE)]
        if all((np.abs(r[3] - tau1) > 1e-6 * tau1).all() for r in refs):
            break
        tau1 *= 1.001
    kps, fs = frag(kp), frag(feats)
    scene = matching.evaluate_scene(kps, fs, None, FIVE, gts, tau1=tau1)
    again = matching.evaluate_scene(kps, fs, None, FIVE, gts, tau1=tau1)
    assert scene.n_match.sum() > 0 and 0 < scene.n_inlier.sum() < scene.n_match.sum()
    for p, (s, t) in enumerate(FIVE):
        n_inlier, ratio, matches, dist = refs[p]
        assert (int(scene.n_inlier[p]), int(scene.n_match[p])) == (n_inlier, matches.shape[0])
        assert scene.inlier_ratio[p] == ratio
        assert np.array_equal(scene.matches[p], matches)
        assert np.allclose(scene.distances[p], dist, rtol=1e-12, atol=0.0)
        one = matching.evaluate_fragment_pair(kps[s], kps[t], fs[s], fs[t], gts[p], tau1=tau1)
        assert one[0] == n_inlier and one[1] == ratio
        assert one[2].tobytes() == scene.matches[p].tobytes() and one[3].tobytes() == scene.distances[p].tobytes()
        assert again.matches[p].tobytes() == scene.matches[p].tobytes()
        assert again.distances[p].tobytes() == scene.distances[p].tobytes()
    assert again.n_inlier.tobytes() == scene.n_inlier.tobytes() and again.n_match.tobytes() == scene.n_match.tobytes()
    assert scene.recall == [(tau, 100.0 * float(np.mean(scene.inlier_ratio > tau))) for tau in (0.05, 0.1, 0.2)]


def test_two_runs_of_the_nearest_neighbour_call_are_bitwise_equal(gpu):
    feats, off = unit_case((700, 1300), 64)
    a, b = run_nn(gpu, feats, off, [[0, 1], [1, 0]]), run_nn(gpu, feats, off, [[0, 1], [1, 0]])
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_golden_pair_of_the_reference(gpu):
    from epn_pointcloud_amd import matching
    g = golden("match_pair.npz")
    dev = lambda k: T(g[k]).to(gpu)
    tau1 = float(g["tau1"])
    n_inlier, ratio, matches, dist = matching.evaluate_fragment_pair(dev("src_kp"), dev("tgt_kp"), dev("src_feats"), dev("tgt_feats"),
                                                                     g["gt"], tau1=tau1)
    assert n_inlier == int(g["n_inlier"]) and matches.shape[0] == int(g["n_match"]) and ratio == float(g["inlier_ratio"])
    assert np.array_equal(matches[dist < tau1], g["inlier_pairs"])
    ref = R.evaluate_fragment_pair(g["src_kp"], g["tgt_kp"], g["src_feats"], g["tgt_feats"], g["gt"], tau1)
    assert np.array_equal(matches, ref[2]) and np.allclose(dist, ref[3], rtol=1e-12, atol=0.0)
    s2t, t2s, mutual = matching.match_descriptors(dev("src_feats"), dev("tgt_feats"))
    assert np.array_equal(np.flatnonzero(mutual.cpu().numpy()), matches[:, 1])
    assert np.array_equal(t2s.cpu().numpy()[matches[:, 1]], matches[:, 0])
    assert np.array_equal(s2t.cpu().numpy()[matches[:, 0]], matches[:, 1])


def test_describe_then_match_end_to_end(gpu):
    """Plumbing only: two overlapping fragments of one cloud -> describe() -> evaluate_fragment_pair equals match_ref on the
    same descriptors; rows describe() marked invalid are absent from the matches."""
    from epn_pointcloud_amd import matching, models as M
    from test_models_cpu import fill_state_dict
    rng = np.random.default_rng(8)
    cloud = rng.uniform(-1, 1, (4000, 3)).astype(np.float32)
    src_pc, tgt_pc = cloud[:3000], cloud[1000:]             # the middle 2000 points are shared; gt is the identity
    rows = rng.choice(np.arange(1000, 3000), 12, replace=False)
    src_kp, tgt_kp = cloud[rows].copy(), cloud[rows[::-1]].copy()
    src_kp[4] = 9.0                                         # far outside: describe() marks them invalid
    tgt_kp[7] = -9.0
    m = fill_state_dict(M.build_inv(input_num=1024, search_radius=0.8, width_div=2)).to(gpu).eval()
    dev = lambda x: T(x).to(gpu)
    sd, sv = m.describe(dev(src_pc), dev(src_kp), batch=4, seed=3)
    td, tv = m.describe(dev(tgt_pc), dev(tgt_kp), batch=4, seed=3)
    assert sv.tolist() == [i != 4 for i in range(12)] and tv.tolist() == [i != 7 for i in range(12)]
    got = matching.evaluate_fragment_pair(dev(src_kp), dev(tgt_kp), sd, td, np.eye(4), tau1=0.1, src_valid=sv, tgt_valid=tv)
    ref = R.evaluate_fragment_pair(src_kp, tgt_kp, sd.cpu().numpy(), td.cpu().numpy(), np.eye(4), 0.1, sv.cpu().numpy(),
                                   tv.cpu().numpy())
    assert got[0] == ref[0] and got[1] == ref[1] and np.array_equal(got[2], ref[2])
    assert np.allclose(got[3], ref[3], rtol=1e-12, atol=0.0)
    assert got[2].shape[0] > 0 and 4 not in got[2][:, 0] and 7 not in got[2][:, 1]
