"""The plane fit of the normals kernel (csrc/plane_fit.h: covariance from the fixed-point moments, cyclic Jacobi on the 3 x 3,
the sign rules) and the patch frame, compiled for the host with the address and undefined-behaviour sanitizers
(tools/plane_fit_host.cpp, a program of its own) and compared with the numpy restatement (tests/normals_ref.py: eigh).

This is where the constant of the one tolerance comes from.  Per component, before any rounding to fp32,

    |n - n_eigh| <= c 2^-52 lam2 / (lam1 - lam0)        |lam - lam_eigh| <= c 2^-52 max|lam|

and the test prints the worst ratio c over 10^5 random neighbourhoods and the degenerate cases of the GPU tests.  The constant
the tests use, normals_ref.C_JACOBI = 82, is 8 x the worst ratio observed (2.23 on the normals, 10.22 on the eigenvalues: 8 x
10.22 = 81.7); the margin covers another, equally valid rounding order on the device.  Here the host build is held to the
constant itself."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import normals_ref as N


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler is needed (the oracle build needs one too)"
    exe = str(tmp_path_factory.mktemp("plane") / "plane_fit_host")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tools", "plane_fit_host.cpp"), "-o", exe])
    return exe


def _run(exe, lines, width):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    res = np.array([[float(v) for v in line.split()] for line in out.stdout.strip().split("\n")])
    assert res.shape == (len(lines), width)
    return res


def _fit_lines(moms, used, q, view):
    v = [0.0, 0.0, 0.0] if view is None else [float(x) for x in view]
    return ["fit %d 1.0 %r %r %r %d %r %r %r " % (u, float(qq[0]), float(qq[1]), float(qq[2]), view is not None, *v)
            + " ".join(str(int(x)) for x in mom) for mom, u, qq in zip(moms, used, q)]


def random_moments(rng, groups, k):
    """`groups` neighbourhoods of k points each: a disc of random radius in a random plane, thickened by noise of a random
    level from 0 to isotropic, its centre off the query -- all inside the unit ball, in the units of the radius.  -> int64
    [groups, 9]"""
    normal = rng.standard_normal((groups, 1, 3))
    normal /= np.linalg.norm(normal, axis=2, keepdims=True)
    p = rng.standard_normal((groups, k, 3))
    p -= (p * normal).sum(axis=2, keepdims=True) * normal * (1.0 - 10.0 ** rng.uniform(-6, 0, (groups, 1, 1)))
    p *= rng.uniform(0.05, 0.5, (groups, 1, 1)) / np.abs(p).max(axis=(1, 2), keepdims=True)
    t = p + rng.uniform(-0.4, 0.4, (groups, 1, 3))
    assert np.abs(t).max() < 1.0
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    S = np.rint(t * N.FIX).astype(np.int64).sum(axis=1)
    M = np.stack([np.rint((t[:, :, i] * t[:, :, j]) * N.FIX).astype(np.int64).sum(axis=1) for i, j in pairs], axis=1)
    return np.concatenate((S, M), axis=1)


def test_builtin_records(host_program):
    out = subprocess.run([host_program], input="", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [[float(v) for v in line.split()] for line in out.stdout.strip().split("\n")]
    assert rows[0][:7] == [0, 0, 0, 1, 0, 0.25, 0.25]               # the square in z = 0: normal +z without a view
    assert rows[1][0] == 0 and rows[1][3] == -1 and rows[1][9] == -1         # the view below the plane turns it
    assert rows[2] == [1, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0]       # two neighbours: the fallback, bit 0


def test_plane_fit_against_eigh_and_the_constant_of_the_tolerance(host_program):
    rng = np.random.default_rng(0)
    moms, used = [], []
    for k, groups in ((3, 20000), (4, 15000), (5, 10000), (8, 15000), (16, 15000), (30, 20000), (100, 5000)):
        moms.append(random_moments(rng, groups, k))
        used += [k] * groups
    moms = np.concatenate(moms)
    assert moms.shape[0] == 100_000
    q = rng.uniform(-1, 1, (moms.shape[0], 3)).astype(np.float32)
    worst_n = worst_l = 0.0
    compared = 0
    for view in (None, np.float32([0.3, -2.0, 0.7])):
        got = _run(host_program, _fit_lines(moms, used, q, view), 13)
        for i in range(moms.shape[0]) if view is None else range(0, moms.shape[0], 10):
            n, lam, flags = N.plane_fit(moms[i], used[i], q[i], view)
            assert int(got[i, 0]) == flags or abs((lam[1] - lam[0]) - N.GAP_MIN) < 1e-15
            scale = np.abs(lam).max()
            worst_l = max(worst_l, np.abs(got[i, 4:7] - lam).max() / (2.0 ** -52 * scale))
            assert abs(np.linalg.norm(got[i, 1:4]) - 1.0) <= 2.0 ** -51
            if not flags & N.FLAG_GAP:
                ratio = np.abs(got[i, 1:4] - n).max() / (2.0 ** -52 * lam[2] / (lam[1] - lam[0]))
                worst_n = max(worst_n, ratio)
                compared += 1
                # the rounded outputs: fp32 of the fp64 ones
                assert np.array_equal(got[i, 7:10].astype(np.float32), got[i, 1:4].astype(np.float32))
    print(f"worst ratio over {compared} fits: normal {worst_n:.3f}, eigenvalues {worst_l:.3f}; C_JACOBI = {N.C_JACOBI}")
    assert compared > 100_000
    assert worst_n <= N.C_JACOBI and worst_l <= N.C_JACOBI


def test_degenerate_moments(host_program):
    """Points, lines, exact lattice planes and all-zero moments: finite unit normals, ascending eigenvalues, the flags."""
    t = {"point": np.tile([[0.25, -0.5, 0.125]], (5, 1)), "line": np.outer(np.arange(-3, 4) / 8.0, [1.0, 1.0, 0.0]),
         "z=0": np.array([[x / 4.0, y / 4.0, 0.0] for x in (-1, 0, 1) for y in (-1, 0, 1)]),
         "x=y": np.array([[x / 4.0, x / 4.0, z / 4.0] for x in (-1, 0, 1) for z in (-1, 0, 1)]),
         "three": np.array([[0.5, 0, 0], [0, 0.5, 0], [0, 0, 0.5]])}
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    moms = [np.concatenate((np.rint(v * N.FIX).astype(np.int64).sum(axis=0),
                            [np.rint((v[:, i] * v[:, j]) * N.FIX).astype(np.int64).sum() for i, j in pairs])) for v in t.values()]
    got = _run(host_program, _fit_lines(moms, [v.shape[0] for v in t.values()], np.zeros((len(t), 3)), None), 13)
    res = dict(zip(t, got))
    assert np.isfinite(got).all() and (np.diff(got[:, 4:7], axis=1) >= 0).all()
    assert int(res["point"][0]) == N.FLAG_GAP and int(res["line"][0]) == N.FLAG_GAP
    assert int(res["z=0"][0]) == 0 and res["z=0"][1:4].tolist() == [0, 0, 1] and res["z=0"][4] == 0
    s = np.sqrt(0.5)
    assert int(res["x=y"][0]) == 0 and np.abs(res["x=y"][1:4] - [s, -s, 0]).max() <= 2.0 ** -52 and abs(res["x=y"][4]) <= 2.0 ** -52
    assert int(res["three"][0]) == 0 and np.abs(res["three"][1:4] - np.sqrt(1 / 3.0)).max() <= 2.0 ** -51


def test_patch_frame_and_rotation(host_program):
    rng = np.random.default_rng(1)
    normals = np.vstack((rng.standard_normal((200, 3)), [[0, -1, 0], [0, 1, 0], [0, -3.5, 0], [0, 0, 0], [1e-3, 0, 0]])).astype(np.float32)
    rows = rng.uniform(-1, 1, normals.shape).astype(np.float32)
    rows[3] = 0
    got = _run(host_program, ["frame " + " ".join(repr(float(v)) for v in np.concatenate((n, p))) for n, p in zip(normals, rows)], 12)
    out, axis = N.orient_patches(rows[:, None, :], normals)
    assert np.isfinite(got).all()
    assert np.array_equal(got[:, :9].astype(np.float32).view(np.uint32), axis.reshape(-1, 9).view(np.uint32))
    assert np.array_equal(got[:, 9:].astype(np.float32).view(np.uint32), out[:, 0].view(np.uint32))
    assert (axis[200:203, :, :2] == 0).all()                        # parallel to up: x and y collapse, as upstream
