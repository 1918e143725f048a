"""ICP refinement on the device (csrc/icp_refine.hip; include/epn_so3conv.h: epn_icp_refine_f32) against the
restatement tests/icp_ref.py.

The exact comparison is made step by step: for every iteration k of a device run the restatement is stepped once from the
DEVICE's own T_k bits (taken out of the trace), so a last-bit difference in T cannot move a correspondence between the two.
Correspondences, counts and the integer sums are then bitwise equal (for iterations other than the last they come from
single-iteration device calls started at T_k), T_{k+1} and the rmse are within T_TOL, and a max_iter = K run is bitwise equal to
K chained max_iter = 1 runs.  The case builders assert on the CPU that no decision of their reference run sits on a rounding error
(icp_ref.check_conditions)."""
import functools
import math

import numpy as np
import pytest

import grid_nn_ref as G
import icp_ref as I

pytestmark = pytest.mark.gpu

ACC_GROUPS = 1024            # the header's cap on icp_accumulate's workgroups, four source points each


def _dev(x, gpu, dtype=None):
    import torch
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(gpu)


class Target:
    """A target cloud on the device: its PointGrid (with the valid mask) and its normals."""

    def __init__(self, gpu, tgt, max_radius, normals=None, valid=None):
        from epn_pointcloud_amd.correspondence import PointGrid
        self.gpu, self.n = gpu, len(tgt)
        self.grid = PointGrid(_dev(np.asarray(tgt, dtype=np.float32).reshape(-1, 3), gpu), max_radius, valid=_dev(valid, gpu))
        self.normals = _dev(normals, gpu)

    def refine(self, src, T_init, max_dist, max_iter, rel=1e-6, plane=None, host=True):
        from epn_pointcloud_amd.vgtk.cuda import grouping
        import torch
        plane = self.normals is not None if plane is None else plane
        out = grouping.icp_refine(self.grid._workspace, self.n, _dev(np.asarray(src, dtype=np.float32).reshape(-1, 3), self.gpu),
                                  _dev(np.asarray(T_init, dtype=np.float64), self.gpu), max_dist,
                                  tgt_normals=self.normals if plane else None, max_iter=max_iter, rel_fitness=rel, rel_rmse=rel,
                                  return_sums=True, return_nn=True)
        if not host:
            return out
        T, trace, iterations, status, sums, nn_idx = (t.cpu().numpy() for t in out)
        return dict(T=T, trace=trace, iterations=int(iterations[0]), status=int(status[0]), sums=[int(v) for v in sums], nn_idx=nn_idx)


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))


def check_steps(target, case, dev, max_iter, rel=1e-6):
    """Every live iteration of the device run `dev` against the restatement stepped from the device's own T_k.  Every case that
    comes here was built by icp_ref.checked_run, which asserts the conditions of the exact comparison on the CPU."""
    assert case.get("checked") == max_iter, "the case did not pass check_conditions for this many iterations"
    tgt, src, plane = case["tgt"], np.asarray(case["src"], dtype=np.float32).reshape(-1, 3), case.get("normals") is not None
    m = len(src)
    T_k = np.array(case["T_init"], dtype=np.float64).reshape(4, 4).copy()
    T_k[3] = (0, 0, 0, 1)
    pf = pr = 0.0
    iterations = status = 0
    for k in range(max_iter):
        q, nn_idx, d2, S = I.iterate_from(tgt, src, T_k, case["max_dist"], case.get("normals"), case.get("valid"))
        one = target.refine(src, T_k, case["max_dist"], 1, rel=rel, plane=plane)            # the device's iteration from T_k
        assert np.array_equal(one["nn_idx"], nn_idx), f"iteration {k}: correspondences"
        assert one["sums"] == S, f"iteration {k}: sums"
        flags, T_next, rec, pf, pr, info = I.step(plane, S, m, k, rel, rel, pf, pr, T_k)
        got = dev["trace"][k]
        assert got[16] == rec[16] and got[17] == rec[17] and got[19] == rec[19], f"iteration {k}: count, ssd, flags"
        assert abs(got[18] - rec[18]) <= I.T_TOL, f"iteration {k}: rmse"
        assert np.abs(got[:16].reshape(4, 4) - T_next).max() <= I.T_TOL, f"iteration {k}: T"
        pr = got[18]                                                                       # the device's own value from here on
        status |= flags
        iterations += flags == 0
        if flags:
            for later in range(k + 1, max_iter):
                assert _same(dev["trace"][later], dev["trace"][k]), f"record {later} after the stop at {k}"
            assert _same(dev["T"], got[:16].reshape(4, 4)) and _same(got[:16].reshape(4, 4)[:3], T_k[:3])
            assert dev["sums"] == S and np.array_equal(dev["nn_idx"], nn_idx)
            break
        T_k = got[:16].reshape(4, 4).copy()
    else:
        assert dev["sums"] == S and np.array_equal(dev["nn_idx"], nn_idx)                   # the last iteration's
        assert _same(dev["T"], T_k)
    assert dev["iterations"] == iterations and dev["status"] == status
    return iterations, status


# ------------------------------------------------------------------------------------------------ cases
ANCHOR = np.float32(-0.04)   # one stray target point at (ANCHOR, ANCHOR, ANCHOR) fixes the grid's per-axis minimum
CLUMPS = ((300, 6, 8), (65, 12, 8))   # (records, cell index on x, on y) of the clumps on the z = 0 plane, in cell 1 on z


def _surface_case(seed, n, m, plane, valid_share=None, clumps=False, alter=None):
    """A noisy room corner as the target, m of its points moved by a small rigid motion and noise as the source.
    clumps: the target gets a stray point at the anchor, so that cell k of an axis is centred at ANCHOR + k * edge, and CLUMPS
    are placed within 0.2 edge of their cells' centres; the corner's own points that fall into those cells are taken out, so
    the cells hold exactly 300 and 65 records.  alter: a variation applied before the conditions are checked --
    ("nonfinite",): three source rows become NaN / inf; ("count", c): twelve source rows, all but the first c out of reach;
    ("parallel",): every normal (0, 0, 1)."""
    rng = np.random.default_rng(seed)
    tgt, nrm = I.corner_scene(rng, max(n // 3, 1), noise=0.002)
    tgt, nrm = tgt[:n], nrm[:n]
    if clumps:
        E = float(G.cell_edge(0.05))
        parts, normals = [np.full((1, 3), ANCHOR, dtype=np.float32)], [np.array([[0, 0, 1]], dtype=np.float32)]
        for size, kx, ky in CLUMPS:
            centre = np.array([float(ANCHOR) + kx * E, float(ANCHOR) + ky * E, 0.0])
            parts.append((centre + rng.uniform(-0.2, 0.2, (size, 3)) * [E, E, 0.05 * E]).astype(np.float32))
            normals.append(np.tile(np.array([[0, 0, 1]], dtype=np.float32), (size, 1)))
        own = []
        for c in parts[1:]:
            idx = G.cell_indices(np.concatenate((parts[0], c)), 0.05)[1][1:]      # with the anchor in, as in the whole target
            assert (idx == idx[0]).all()
            own.append(tuple(idx[0].tolist()))
        _, cells, _ = G.cell_indices(np.concatenate((parts[0], tgt)), 0.05)
        keep = np.array([tuple(c) not in own for c in cells[1:].tolist()])
        tgt, nrm = np.concatenate(parts + [tgt[keep]]), np.concatenate(normals + [nrm[keep]])
        n = len(tgt)
    pick = rng.integers(0, max(n, 1), m) if n else np.zeros(m, dtype=np.int64)
    truth = I.rigid(0.008 * rng.standard_normal(3), 0.005 * rng.standard_normal(3))
    inv = np.linalg.inv(truth)
    base = tgt[pick].astype(np.float64) if n else rng.uniform(0, 1, (m, 3))
    src = ((base + 0.001 * rng.standard_normal((m, 3))) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    if alter == ("nonfinite",):
        src[3], src[77, 1], src[500, 2] = np.nan, np.inf, -np.inf
    elif alter is not None and alter[0] == "count":
        src = src[:12].copy()
        src[alter[1]:] += np.float32(5.0)
    case = dict(tgt=tgt, src=src, T_init=np.eye(4), max_dist=0.05, truth=truth)
    if plane:
        case["normals"] = nrm
        if alter == ("parallel",):
            case["normals"] = np.tile(np.array([[0, 0, 1]], dtype=np.float32), (n, 1))
    if valid_share is not None:
        case["valid"] = (rng.random(n) < valid_share).astype(np.uint8)
    return case


def _search(make, what, max_iter):
    case, ref = I.checked_run(make, what, max_iter)
    return dict(case, checked=max_iter), ref


@functools.lru_cache(maxsize=None)
def _checked(n, m, plane, max_iter, valid_share=None, clumps=False, alter=None):
    return _search(lambda seed: _surface_case(seed, n, m, plane, valid_share, clumps, alter),
                   f"surface n={n} m={m} plane={plane} alter={alter}", max_iter)


def _fixed(case, what, max_iter):
    """A case with nothing to search: it must meet the conditions as it stands."""
    return _search(lambda seed: case, what, max_iter)[0]


@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
@pytest.mark.parametrize("m", [1, 3, 4, 5, 4 * ACC_GROUPS + 1])
def test_source_sizes_step_by_step(gpu, m, plane):
    """m = one wave-group short of, exactly and one past a workgroup, and just past four times the workgroup cap, where the
    stride loop wraps once, for one workgroup only.  (m = 1, 3: too few pairs for a fit, by contract.)"""
    K = 3
    case, ref = _checked(1500, m, plane, K)
    target = Target(gpu, case["tgt"], 0.05, case.get("normals"))
    dev = target.refine(case["src"], case["T_init"], case["max_dist"], K)
    iterations, status = check_steps(target, case, dev, K)
    assert (iterations, status) == (ref["iterations"], ref["status"])
    if m < (6 if plane else 3):
        assert status == I.FEW and iterations == 0


@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
def test_cells_of_1_65_and_300_records(gpu, plane):
    """No mask: the cells hold exactly 300 and 65 records (one past a wave's pass of 64), and some cell holds one."""
    K = 3
    case, ref = _checked(1500, 600, plane, K, None, True)
    _, cells, flags = G.cell_indices(case["tgt"], 0.05)
    uniq, counts = np.unique(cells, axis=0, return_counts=True)
    occupancy = {tuple(c): k for c, k in zip(uniq.tolist(), counts.tolist())}
    assert flags == 0 and [occupancy[(kx, ky, 1)] for _, kx, ky in CLUMPS] == [300, 65] and 1 in counts
    target = Target(gpu, case["tgt"], 0.05, case.get("normals"))
    dev = target.refine(case["src"], case["T_init"], case["max_dist"], K)
    check_steps(target, case, dev, K)
    mates = dev["nn_idx"][dev["nn_idx"] >= 0]
    assert ((mates >= 1) & (mates <= 300)).sum() > 20 and ((mates > 300) & (mates <= 365)).sum() > 5   # the clumps are searched


@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
def test_a_masked_target(gpu, plane):
    K = 3
    case, ref = _checked(1500, 600, plane, K, 0.8)
    target = Target(gpu, case["tgt"], 0.05, case.get("normals"), case["valid"])
    dev = target.refine(case["src"], case["T_init"], case["max_dist"], K)
    check_steps(target, case, dev, K)
    live = dev["nn_idx"][dev["nn_idx"] >= 0]
    assert live.size and case["valid"][live].all()                     # a masked point is never a mate


def test_m_zero_and_max_iter_zero(gpu):
    case, _ = _checked(1500, 5, False, 3)
    target = Target(gpu, case["tgt"], 0.05)
    T0 = I.rigid([0.1, 0.2, 0.3], [1, 2, 3])
    for src, K in ((np.zeros((0, 3), np.float32), 4), (case["src"], 0)):
        dev = target.refine(src, T0, 0.05, K)
        assert _same(dev["T"], T0) and dev["iterations"] == 0 and dev["status"] == 0
        assert dev["trace"].shape == (K, 20) and all(_same(r[:16].reshape(4, 4), T0) and not r[16:].any() for r in dev["trace"])
        assert dev["sums"] == [0] * 32 and (dev["nn_idx"] == -1).all()


@pytest.mark.parametrize("n", [0, 1])
def test_tiny_targets(gpu, n):
    tgt = np.array([[0.5, 0.25, 0.125]], dtype=np.float32)[:n]
    src = (np.array([[0.5, 0.25, 0.125]]) + 0.01 * np.random.default_rng(0).standard_normal((7, 3))).astype(np.float32)
    case = dict(tgt=tgt, src=src, T_init=np.eye(4), max_dist=0.1)
    target = Target(gpu, tgt, 0.1)
    dev = target.refine(src, np.eye(4), 0.1, 2)
    if n == 0:
        assert dev["status"] == I.FEW and dev["iterations"] == 0 and (dev["nn_idx"] == -1).all() and dev["sums"] == [0] * 32
        assert _same(dev["T"], np.eye(4)) and _same(dev["trace"][1], dev["trace"][0])
    else:                                                             # seven pairs with one point: the integer half only
        q, nn_idx, d2, S = I.iterate_from(tgt, src, np.eye(4), 0.1)
        assert (nn_idx == 0).all() and np.array_equal(dev["nn_idx"], nn_idx) and dev["trace"][0, 16] == 7
        assert target.refine(src, np.eye(4), 0.1, 1)["sums"] == S


def test_nothing_within_max_dist_and_non_finite_source_rows(gpu):
    case, _ = _checked(1500, 5, False, 3)
    target = Target(gpu, case["tgt"], 0.05)
    far = case["src"] + np.float32(10.0)
    dev = target.refine(far, np.eye(4), 0.05, 2)
    assert dev["status"] == I.FEW and (dev["nn_idx"] == -1).all() and dev["trace"][0, 16] == 0 and dev["trace"][0, 18] == 0
    bad, ref = _checked(1500, 600, False, 3, None, False, ("nonfinite",))
    target = Target(gpu, bad["tgt"], 0.05)
    dev = target.refine(bad["src"], np.eye(4), 0.05, 3)
    assert (dev["nn_idx"][[3, 77, 500]] == -1).all()
    check_steps(target, bad, dev, 3)


@pytest.mark.parametrize("plane,count", [(False, 2), (False, 3), (True, 5), (True, 6)])
def test_counts_at_the_minimum(gpu, plane, count):
    """`count` source points next to the target, the others out of reach; the seed is searched with the variation in place, so
    a fit from three or six pairs is one whose conditioning and bound pass check_conditions."""
    small, ref = _checked(1500, 600, plane, 2, None, False, ("count", count))
    target = Target(gpu, small["tgt"], 0.05, small.get("normals"))
    dev = target.refine(small["src"], np.eye(4), 0.05, 2)
    assert dev["trace"][0, 16] == count
    _, status = check_steps(target, small, dev, 2)
    assert bool(status & I.FEW) == (count < (6 if plane else 3))
    if not status & I.FEW:
        assert dev["iterations"] >= 1                                  # the fit from exactly enough pairs was made


def test_all_normals_parallel_is_singular(gpu):
    flat, ref = _checked(1500, 600, True, 3, None, False, ("parallel",))
    target = Target(gpu, flat["tgt"], 0.05, flat["normals"])
    dev = target.refine(flat["src"], np.eye(4), 0.05, 3)
    assert check_steps(target, flat, dev, 3) == (0, I.SINGULAR)
    assert _same(dev["T"], np.eye(4))


def test_lattice_ties_go_to_the_lowest_row(gpu):
    """Every target point twice (rows i and i + n): the mate is always the lower row; source points midway between lattice
    points are at exactly equal fp32 distances from several."""
    ax = np.arange(-2, 3) * 0.25
    lat = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    tgt = np.concatenate((lat, lat))
    src = np.concatenate((lat + np.float32(0.125), lat[:40] + np.array([0.125, 0, 0], dtype=np.float32)))
    case = _fixed(dict(tgt=tgt, src=src, T_init=np.eye(4), max_dist=0.25), "lattice ties", 1)
    target = Target(gpu, tgt, 0.25)
    dev = target.refine(src, np.eye(4), 0.25, 1)
    check_steps(target, case, dev, 1)
    assert (dev["nn_idx"] >= 0).all() and (dev["nn_idx"] < len(lat)).all()


def test_range_flag_one_quantum_inside_and_outside(gpu):
    # one pair at the edge of the range, forty around the origin: the centroids stay small, so the bound of the fit stays below T_TOL
    tgt = np.concatenate(([[63.9, 0, 0]], np.random.default_rng(3).uniform(-1, 1, (40, 3)))).astype(np.float32)
    inside, outside = np.float32(64.0), np.nextafter(np.float32(64.0), np.float32(np.inf))
    target = Target(gpu, tgt, 0.5)
    for x, flagged in ((inside, False), (outside, True)):
        src = tgt + np.float32([0, 0, 0.01])
        src[0] = (x, 0, 0)
        case = _fixed(dict(tgt=tgt, src=src, T_init=np.eye(4), max_dist=0.5), f"range pair at {x}", 2)
        dev = target.refine(src, np.eye(4), 0.5, 2)
        _, status = check_steps(target, case, dev, 2)
        assert bool(status & I.RANGE) == flagged and (dev["sums"][30] == 1) == flagged
    from epn_pointcloud_amd import refine_registration
    with pytest.raises(ValueError, match="bit 3"):
        refine_registration(_dev(src, gpu), target.grid, np.eye(4), 0.5)


@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
def test_early_stop_chained_runs_repeat_and_graph(gpu, plane):
    """A run that converges before max_iter: the later records and T unchanged, iterations right (check_steps); K iterations in
    one call bitwise equal to K chained one-iteration calls (with the stop test off: it compares successive iterations); two
    runs bitwise equal; one captured and replayed graph bitwise equal to the eager run."""
    import torch
    K = 12
    case, ref = _checked(1500, 600, plane, K)
    assert ref["status"] == I.CONVERGED and 0 < ref["iterations"] < K - 1
    target = Target(gpu, case["tgt"], 0.05, case.get("normals"))
    dev = target.refine(case["src"], np.eye(4), 0.05, K)
    assert check_steps(target, case, dev, K) == (ref["iterations"], I.CONVERGED)
    again = target.refine(case["src"], np.eye(4), 0.05, K)
    assert all(_same(dev[k], again[k]) for k in ("T", "trace", "nn_idx")) and dev["sums"] == again["sums"]
    assert (again["iterations"], again["status"]) == (dev["iterations"], dev["status"])
    whole = target.refine(case["src"], np.eye(4), 0.05, 4, rel=0.0)
    T = np.eye(4)
    for k in range(4):
        one = target.refine(case["src"], T, 0.05, 1, rel=0.0)
        assert _same(one["trace"][0], whole["trace"][k])
        T = one["T"]
    assert _same(T, whole["T"]) and whole["iterations"] == 4 and whole["status"] == 0
    stream, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        target.refine(case["src"], np.eye(4), 0.05, K, host=False)
        torch.cuda.synchronize()
        src, T0 = _dev(case["src"], gpu), _dev(np.eye(4), gpu)
        from epn_pointcloud_amd.vgtk.cuda import grouping
        with torch.cuda.graph(graph, stream=stream):                   # one stream, one linear chain
            out = grouping.icp_refine(target.grid._workspace, target.n, src, T0, 0.05, tgt_normals=target.normals, max_iter=K,
                                      return_sums=True, return_nn=True)
        for t in out:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
    assert _same(out[0].cpu().numpy(), dev["T"]) and _same(out[1].cpu().numpy(), dev["trace"])
    assert int(out[2][0]) == dev["iterations"] and int(out[3][0]) == dev["status"] and [int(v) for v in out[4].cpu()] == dev["sums"]
    assert np.array_equal(out[5].cpu().numpy(), dev["nn_idx"])


SIGMA = 0.002


@functools.lru_cache(maxsize=None)
def _planted(plane):
    """A sphere cap plus a box corner, 2000 points; the source is the same surface samples under the inverse of a planted motion
    with isotropic noise SIGMA; T_init is the truth off by about 3 degrees and 2 cm."""
    def make(seed):
        rng = np.random.default_rng(100 + seed)
        tgt, nrm = I.cap_and_corner(rng, 2000, noise=0.0)
        truth = I.rigid(rng.standard_normal(3) * 0.3, rng.uniform(-0.2, 0.2, 3))
        inv = np.linalg.inv(truth)
        src = ((tgt.astype(np.float64) + SIGMA * rng.standard_normal(tgt.shape)) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
        axis = rng.standard_normal(3)
        T_init = I.rigid(axis / np.linalg.norm(axis) * math.radians(3.0), [0.012, -0.012, 0.01]) @ truth
        case = dict(tgt=tgt, src=src, T_init=T_init, max_dist=0.1, truth=truth)
        if plane:
            case["normals"] = nrm
        return case
    return _search(make, f"planted pair plane={plane}", 30)


@pytest.mark.parametrize("plane", [False, True], ids=["point", "plane"])
def test_planted_pair_end_to_end(gpu, plane):
    """refine_registration improves on T_init, equals the restatement step by step, and the RESTATEMENT meets the ground truth
    within the planted noise: the least-squares estimate from N = 2000 pairs with noise SIGMA per coordinate has a standard
    deviation of about SIGMA / sqrt(N) in translation; the bounds SIGMA (translation) and SIGMA / 0.5 rad (rotation, the
    scene's half extent being 0.5) are more than twenty of those, and are not tuned to the device."""
    from epn_pointcloud_amd import refine_registration, registration_errors
    case, ref = _planted(plane)
    rre_ref, rte_ref = registration_errors(ref["T"], case["truth"])
    assert rte_ref[0] <= SIGMA and rre_ref[0] <= math.degrees(SIGMA / 0.5)                # on the CPU, on the restatement
    target = Target(gpu, case["tgt"], 0.1, case.get("normals"))
    res = refine_registration(_dev(case["src"], gpu), target.grid, case["T_init"], 0.1, tgt_normals=target.normals)
    rre0, rte0 = registration_errors(case["T_init"], case["truth"])
    rre, rte = registration_errors(res.T, case["truth"])
    assert rre[0] < rre0[0] and rte[0] < rte0[0]
    dev = target.refine(case["src"], case["T_init"], 0.1, 30)
    assert _same(dev["T"], res.T) and _same(dev["trace"], res.trace) and res.iterations == dev["iterations"]
    assert check_steps(target, case, dev, 30) == (ref["iterations"], ref["status"])
    live = dev["trace"][min(dev["iterations"], 29)]
    assert res.fitness == live[16] / len(case["src"]) and res.inlier_rmse == live[18] and res.status == I.CONVERGED


def test_refine_scene_equals_per_pair_calls(gpu):
    from epn_pointcloud_amd import refine_registration, refine_scene
    from epn_pointcloud_amd.matching import _invert_rigid
    rng = np.random.default_rng(9)
    world, nrm = I.cap_and_corner(rng, 900, noise=0.001)
    poses = [np.eye(4), I.rigid([0.1, -0.2, 0.05], [0.1, 0.0, -0.1]), I.rigid([-0.2, 0.1, 0.1], [0.0, 0.2, 0.1])]
    clouds = [_dev((world.astype(np.float64) @ np.linalg.inv(P)[:3, :3].T + np.linalg.inv(P)[:3, 3]).astype(np.float32), gpu)
              for P in poses]
    pairs = [[0, 1], [0, 2], [1, 2]]
    off = I.rigid([0.01, 0.02, -0.01], [0.005, -0.004, 0.003])
    T_init = np.stack([np.linalg.inv(poses[i]) @ poses[j] @ off for i, j in pairs])       # tgt into src, a little off
    for normals in (None, 0.1):
        T, results = refine_scene(clouds, pairs, T_init, 0.05, normals=normals, max_iter=10)
        for p, (i, j) in enumerate(pairs):
            from epn_pointcloud_amd.correspondence import PointGrid
            grid = PointGrid(clouds[j], 0.05 if normals is None else 0.1)
            n = None if normals is None else grid.normals(radius=0.1, max_nn=30).normals
            r = refine_registration(clouds[i], grid, _invert_rigid(T_init[p]), 0.05, tgt_normals=n, max_iter=10)
            assert _same(r.T, results[p].T) and _same(r.trace, results[p].trace) and _same(T[p], _invert_rigid(r.T))
            assert np.abs(T[p] - np.linalg.inv(poses[i]) @ poses[j]).max() < np.abs(T_init[p] - np.linalg.inv(poses[i]) @ poses[j]).max()
