"""The projection onto SO(3) of the rotation kernels (csrc/rotation_math.h: Horn's 4 x 4 matrix, a fixed number of Jacobi sweeps),
compiled for the host with the address and undefined-behaviour sanitizers (tools/so3_project_host.cpp) and compared with
numpy's SVD at every conditioning, which the GPU tests (margin >= 1e-3, one opposed pair, zero weights) do not reach.

Bounds: R is a rotation to 1e-14 whatever the input; it attains the optimum, tr(R^T C) within 1e-12 max(1, |C|) of the SVD
solution's (unique or not); margin within 1e-12; and where the solution is unique to fp64, |R - R_svd| * margin <= 1e-13: the
projection's condition number is 2 / (s1 margin), both solvers are backward stable to a few ulps of s1."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import rotation_ref as Rf


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler is needed (the oracle build needs one too)"
    exe = str(tmp_path_factory.mktemp("rot") / "so3_project_host")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tools", "so3_project_host.cpp"), "-o", exe])
    return exe


def _run(exe, mats, xs=()):
    text = "\n".join(" ".join(repr(float(v)) for v in C.ravel()) for C in mats)
    text += "\nacos\n" + " ".join(repr(float(x)) for x in xs) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [[float(v) for v in line.split()] for line in out.stdout.strip().split("\n")]
    res = np.array(rows[:len(mats)])
    return res[:, :9].reshape(-1, 3, 3), res[:, 9], np.array([r[0] for r in rows[len(mats):]])


def _matrices():
    rng = np.random.default_rng(0)
    mats = [rng.standard_normal((3, 3)) for _ in range(2000)]
    mats += [Rf.random_rotations(rng, 1)[0] * rng.uniform(0.1, 3) for _ in range(50)]
    mats += [np.outer(rng.standard_normal(3), rng.standard_normal(3)) for _ in range(20)]            # rank 1
    U, V = Rf.random_rotations(rng, 40), Rf.random_rotations(rng, 40)
    for i, m in enumerate(np.logspace(-12, -1, 40)):                                              # margins 1e-12 .. 0.1
        mats.append(U[i] @ np.diag([1.0, 0.5 + m / 2, (0.5 - m / 2) * (-1) ** i * -1]) @ V[i].T)
    mats += [np.diag([0, 0, 2.0]), np.zeros((3, 3)), np.eye(3), -np.eye(3), np.diag([1, -1, -1.0]), np.diag([1e-30, 0, 0]),
             np.diag([1e30, 1e30, -1e30]), 1e-30 * rng.standard_normal((3, 3)), 1e30 * rng.standard_normal((3, 3))]
    return mats


def test_projection_against_svd_at_every_conditioning(host_program):
    mats = _matrices()
    R, margin, _ = _run(host_program, mats)
    seen = []
    for C, Rg, mg in zip(mats, R, margin):
        want, m = Rf.project(C)
        assert np.abs(Rg.T @ Rg - np.eye(3)).max() <= 1e-14 and np.linalg.det(Rg) > 0
        assert abs(np.trace(Rg.T @ C) - np.trace(want.T @ C)) <= 1e-12 * max(1.0, np.abs(C).max())
        assert abs(mg - m) <= 1e-12
        if m >= 1e-9:
            assert np.abs(Rg - want).max() * m <= 1e-13, (C, m)
        seen.append(m)
    seen = np.array(seen)
    assert (seen == 0).any() and ((seen > 0) & (seen < 1e-9)).any() and ((seen > 1e-9) & (seen < 1e-3)).any() and (seen > 1).any()
    zero = [i for i, C in enumerate(mats) if not C.any()]
    assert len(zero) == 1 and np.array_equal(R[zero[0]], np.eye(3)) and margin[zero[0]] == 0     # C = 0: R = I exactly


def test_acos_safe_of_the_kernels_against_the_restatement(host_program):
    one = np.float32(1)
    x = np.array([-1.0, -1.0 + 5e-5, 0.0, 1.0 - 5e-5, 1.0, float(np.nextafter(one, one * 2)), float(np.nextafter(-one, -one * 2)),
                  1.0 - 1e-4, -(1.0 - 1e-4), 0.3, -0.7, 1.5, -1.5])
    _, _, got = _run(host_program, [np.eye(3)], x)
    assert np.abs(got - Rf.acos_safe(x)).max() <= 1e-14
