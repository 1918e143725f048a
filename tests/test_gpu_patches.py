"""Patch extraction on the GPU (csrc/patch_extract.hip through vgtk.cuda.grouping / vgtk.pc / InvSO3ConvModel.describe) against
tests/patch_ref.py, the numpy restatement of the specification: idx and counts exactly equal, patches bitwise equal.

Inputs: points uniform in [-1, 1]^3 from a fixed seed.  Set membership must not hang on a rounding: before use, every point
with | |p - q| - r | < 1e-3 r for some keypoint q (fp64, on the CPU) is moved inward by 2e-3 r along the ray from q, until no
such pair is left.  The fp32 rounding of d2 at these magnitudes is about 1e-6 and the margin in d2 about 2e-3 r^2, so nothing
is left out of the comparison.  The keypoints of a scene sit on the diagonal from outside the cube to its centre, at the
places where the ball holds exactly 0, 1, 2, n_sample - 1, n_sample, n_sample + 1 and 8 n_sample points (those that n
allows), the remaining ones are cloud points (d = 0)."""
import functools

import numpy as np
import pytest
import torch

import patch_ref as P

pytestmark = pytest.mark.gpu
T = torch.from_numpy


def _dist(pc64, q):
    return np.sqrt(((pc64 - q[None, :]) ** 2).sum(axis=1))


def _move_off_the_boundary(pc, kpts_of, r):
    """float32 cloud with no (keypoint, point) pair within 1e-3 r of the sphere; kpts_of(pc) -> float64 [k, 3]."""
    for _ in range(50):
        moved = False
        for q in kpts_of(pc):
            p64 = pc.astype(np.float64)
            d = _dist(p64, q)
            near = np.abs(d - r) < 1e-3 * r
            if near.any():
                moved = True
                p64[near] = q + (p64[near] - q) * ((d[near] - 2e-3 * r) / d[near])[:, None]
                pc = p64.astype(np.float32)
        if not moved:
            return pc
    raise AssertionError("boundary pairs remain")


def _place(pc, c0, m, r_eff):
    """Point on the segment c0 -> origin, just past the place where the ball of radius r_eff first holds m points."""
    p64 = pc.astype(np.float64)
    f = lambda t: int((_dist(p64, c0 * (1.0 - t)) < r_eff).sum())
    lo, hi = 0.0, 1.0
    assert f(lo) < m <= f(hi), (m, f(lo), f(hi))
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if f(mid) < m else (lo, mid)
    return c0 * (1.0 - hi)


@functools.lru_cache(maxsize=None)
def scene(n, k, n_sample, seed=0, duplicates=False):
    """-> (pc float32 [n,3], kpts float32 [k,3], radius, targets): see the module docstring."""
    rng = np.random.default_rng(1000 * n + 10 * k + seed)
    if duplicates:
        half = rng.uniform(-1, 1, (n // 2, 3)).astype(np.float32)
        pc = np.concatenate((half, half, half[:n - 2 * (n // 2)]))[rng.permutation(n)]
    else:
        pc = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    targets = [] if duplicates else sorted({m for m in (1, 2, n_sample - 1, n_sample, n_sample + 1, 8 * n_sample) if 1 <= m <= n})
    targets = targets[-1:] if k == 1 else targets[:k - 1]       # a lone keypoint takes the largest count, not the empty ball
    from_origin = np.sort(_dist(pc.astype(np.float64), np.zeros(3)))
    want = max(targets + [min(n, 2 * n_sample)])
    r = float(max(1.02 * from_origin[min(n, int(1.05 * want) + 2) - 1], 0.05))
    c0 = np.full(3, 1.0 + r + 0.1)                         # outside every ball: the keypoint with count 0
    cloud_rows = rng.choice(n, max(k - 1 - len(targets), 0), replace=n < k)
    placed = [_place(pc, c0, m, r * (1 + 1e-3)) for m in targets]

    def kpts_of(cloud):
        rows = ([c0] if k > 1 or not placed else []) + placed + [cloud[i].astype(np.float64) for i in cloud_rows]
        return np.stack(rows[:k])

    for _ in range(10):
        pc = _move_off_the_boundary(pc, kpts_of, r)
        got = [int((_dist(pc.astype(np.float64), q) <= r).sum()) for q in placed]
        off = [j for j, (g, m) in enumerate(zip(got, targets)) if g != m]
        if not off:
            break
        for j in off:
            placed[j] = _place(pc, c0, targets[j], r * (1 + 1e-3))
    else:
        raise AssertionError(f"counts {got} do not reach {targets}")
    kpts = kpts_of(pc).astype(np.float32)
    # the float32 keypoints are what the kernel sees: the margin holds for them too
    for q in kpts.astype(np.float64):
        assert not (np.abs(_dist(pc.astype(np.float64), q) - r) < 0.9e-3 * r).any()
    if duplicates:
        assert len(np.unique(pc, axis=0)) <= n // 2 + 1
    return pc, kpts, r, tuple(targets if k == 1 else [0] + targets)


@functools.lru_cache(maxsize=None)
def reference(key, seed, key_bits, center, scale):
    pc, kpts, r, _ = scene(*key)
    return P.radius_patches(pc, kpts, r, key[2], seed=seed, key_bits=key_bits, center=center, scale=scale)


def run(gpu, pc, kpts, r, n_sample, **kw):
    from epn_pointcloud_amd.vgtk.cuda import grouping
    idx, counts, patches = grouping.radius_patches(T(pc).to(gpu), T(kpts).to(gpu), r, n_sample, **kw)
    return idx.cpu().numpy(), counts.cpu().numpy(), patches.cpu().numpy()


def same(got, want):
    """idx and counts equal, patches bitwise equal; rows with count <= 1 are -1 and zeros."""
    assert np.array_equal(got[1], want[1]), (got[1].tolist(), want[1].tolist())
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32))
    empty = got[1] <= 1
    assert (got[0][empty] == -1).all() and (got[2][empty].view(np.uint32) == 0).all()
    assert (got[0][~empty] >= 0).all()


CASES = [(1, 1, 1), (1, 7, 64), (63, 1, 64), (63, 7, 64), (63, 7, 1), (1000, 7, 64), (1000, 7, 100), (1000, 64, 1),
         (20000, 7, 1), (20000, 7, 100), (20000, 64, 64), (20000, 64, 2048)]


@pytest.mark.parametrize("n,k,n_sample", CASES)
def test_patches_match_the_specification(gpu, n, k, n_sample):
    pc, kpts, r, targets = scene(n, k, n_sample)
    want = reference((n, k, n_sample), 2913, 32, 0, 1.0)
    assert set(targets) <= set(want[1].tolist()), (targets, want[1].tolist())
    got = run(gpu, pc, kpts, r, n_sample, seed=2913)
    same(got, want)
    filled = got[1] > 1                                 # center = 0, scale = 1: bit copies of the fragment's points
    assert np.array_equal(got[2][filled].view(np.uint32), pc[got[0][filled]].view(np.uint32))


def test_four_key_bits_tie_rule(gpu):
    """16 distinct keys over thousands of in-radius points: the threshold bucket holds hundreds of ties, of which the lowest
    indices are taken (the `t` counter of the emit pass)."""
    pc, kpts, r, _ = scene(20000, 7, 100)
    want = reference((20000, 7, 100), 5, 4, 0, 1.0)
    assert want[1].max() > 700
    same(run(gpu, pc, kpts, r, 100, seed=5, key_bits=4), want)
    pc, kpts, r, _ = scene(20000, 64, 2048)
    same(run(gpu, pc, kpts, r, 2048, seed=5, key_bits=4), reference((20000, 64, 2048), 5, 4, 0, 1.0))


def test_keypoints_that_are_cloud_points(gpu):
    pc, kpts, r, targets = scene(1000, 64, 1)           # rows past the placed ones are cloud points: d = 0 is inside
    rows = np.nonzero((kpts[:, None, :] == pc[None, :, :]).all(axis=2).any(axis=1))[0]
    assert len(rows) >= 50
    got = run(gpu, pc, kpts, r, 1, seed=1)
    assert (got[1][rows] >= 1).all()
    same(got, reference((1000, 64, 1), 1, 32, 0, 1.0))


def test_duplicate_points(gpu):
    pc, kpts, r, _ = scene(1000, 7, 64, 0, True)
    want = reference((1000, 7, 64, 0, True), 3, 32, 0, 1.0)
    assert want[1].max() > 64
    same(run(gpu, pc, kpts, r, 64, seed=3), want)


def test_centred_and_scaled_patches(gpu):
    pc, kpts, r, _ = scene(1000, 7, 100)
    same(run(gpu, pc, kpts, r, 100, seed=9, center=True, scale=2.5), reference((1000, 7, 100), 9, 32, 1, 2.5))


def test_two_runs_give_identical_bytes(gpu):
    pc, kpts, r, _ = scene(20000, 64, 64)
    a, b = run(gpu, pc, kpts, r, 64, seed=77), run(gpu, pc, kpts, r, 64, seed=77)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert not np.array_equal(a[0], run(gpu, pc, kpts, r, 64, seed=78)[0])


def test_split_calls_give_the_same_rows(gpu):
    from epn_pointcloud_amd.vgtk import pc as pctk
    pc, kpts, r, _ = scene(20000, 64, 64)
    whole = run(gpu, pc, kpts, r, 64, seed=4)
    lo, hi = run(gpu, pc, kpts[:32], r, 64, seed=4, kpt_row0=0), run(gpu, pc, kpts[32:], r, 64, seed=4, kpt_row0=32)
    for w, x, y in zip(whole, lo, hi):
        assert np.array_equal(w, np.concatenate((x, y)))
    patches, idx, counts = pctk.radius_patches(T(pc).to(gpu), T(kpts).to(gpu), r, 64, seed=4, rows_per_call=24)
    assert np.array_equal(idx.cpu().numpy(), whole[0]) and np.array_equal(counts.cpu().numpy(), whole[1])
    assert np.array_equal(patches.cpu().numpy().view(np.uint32), whole[2].view(np.uint32))


def test_integer_keypoints_equal_their_coordinates(gpu):
    from epn_pointcloud_amd.vgtk import pc as pctk
    pc, _, r, _ = scene(1000, 7, 64)
    rows = torch.tensor([0, 17, 999, 17, 500])
    cloud = T(pc).to(gpu)
    by_row = pctk.radius_patches(cloud, rows.to(gpu), r, 64, seed=2, center=True)
    by_xyz = pctk.radius_patches(cloud, cloud[rows.to(gpu)], r, 64, seed=2, center=True)
    by_int32 = pctk.radius_patches(cloud, rows.int().to(gpu), r, 64, seed=2, center=True)
    for a, b, c in zip(by_row, by_xyz, by_int32):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert (by_row[2] >= 1).all()
    with pytest.raises(RuntimeError):
        pctk.radius_patches(T(pc), rows, r, 64)         # host tensors: there is no CPU path


def test_side_stream_matches_the_default_stream(gpu):
    pc, kpts, r, _ = scene(1000, 7, 100)
    want = run(gpu, pc, kpts, r, 100, seed=6)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        got = run(gpu, pc, kpts, r, 100, seed=6)
    torch.cuda.current_stream(gpu).wait_stream(side)
    for x, y in zip(got, want):
        assert x.tobytes() == y.tobytes()


def test_describe(gpu):
    """k = 10 keypoints of a 4000-point fragment, batch = 4 (the last batch is partial), one keypoint far outside: its row is
    invalid and zero; every other descriptor equals the model's own forward on that patch alone -- in a batch of 4 copies, and
    in a batch padded with zero patches as describe() pads -- within the descriptor head's tolerance of
    tests/test_gpu_models.py (InstanceNorm: the rows of a batch are independent), and has unit norm."""
    from epn_pointcloud_amd import models as M
    from epn_pointcloud_amd.vgtk import pc as pctk
    from test_models_cpu import TOL, fill_state_dict
    rng = np.random.default_rng(8)
    cloud = T(rng.uniform(-1, 1, (4000, 3)).astype(np.float32)).to(gpu)
    kpts = cloud[T(rng.choice(4000, 10, replace=False)).to(gpu)].clone()
    kpts[6] = torch.tensor([9.0, 9.0, 9.0], device=gpu)
    m = fill_state_dict(M.build_inv(input_num=1024, search_radius=0.8, width_div=2)).to(gpu)
    with pytest.raises(RuntimeError):
        m.train().describe(cloud, kpts, batch=4)
    m.eval()
    desc, valid = m.describe(cloud, kpts, batch=4, seed=3)
    assert desc.shape == (10, 32) and desc.dtype == torch.float32 and valid.dtype == torch.bool
    assert valid.tolist() == [i != 6 for i in range(10)]
    assert (desc[6] == 0).all()
    assert torch.isfinite(desc).all()
    assert (desc[valid].norm(dim=1) - 1).abs().max().item() < 1e-4
    patches, _, counts = pctk.radius_patches(cloud, kpts, 0.8, 1024, seed=3)
    assert counts.min().item() == 0 and counts.max().item() > 1024 > counts[valid].min().item()    # both resampling branches
    with torch.no_grad():
        for i in torch.nonzero(valid).flatten().tolist():
            copies = m(patches[i:i + 1].expand(4, -1, -1).contiguous())[0][0]
            padded = m(torch.cat((patches[i:i + 1], patches.new_zeros(3, 1024, 3))))[0][0]
            assert (desc[i] - copies).abs().max().item() <= TOL, i
            assert (desc[i] - padded).abs().max().item() <= TOL, i
    again, _ = m.describe(cloud, kpts[:6], batch=64)     # one partial batch; the seed is describe's default
    assert again.shape == (6, 32) and (again.norm(dim=1) - 1).abs().max().item() < 1e-4
