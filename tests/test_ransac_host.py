"""The rigid fit of the registration kernels (csrc/rigid_fit.h: centroids, cross-covariance, the projection of
csrc/rotation_math.h, t = xbar - R ybar), compiled for the host with the address and undefined-behaviour sanitizers
(tools/rigid_fit_host.cpp, a program of its own) and compared with the numpy SVD fit of tests/ransac_ref.py on three-point and
many-point sets, coincident and collinear samples, coordinates from 1e-3 to 1e3 and sets far from the origin.

Bounds ("Conditioning"): R is a rotation to 1e-14 whatever the input; margin within 1e-12; and where the answer
is unique to fp64 (margin >= 1e-9), |R - R_svd| margin <= 1e-13 kappa with

    kappa = 1 + 4 (n + 3) u rho / 1e-13,   u = 2^-53,   rho = sum_m |x_m - xbar| |y_m - ybar| / s1.

The projection moves by at most 2 |dC| / (s1 margin) under a perturbation dC of C.  An error of a computed centroid shifts
every x_m - xbar alike and meets sum_m (y_m - ybar) = 0, so it enters only at second order; what is left per evaluation is the
rounding of the two differences and the product of each term and of the n - 1 additions, |dC| <= (n + 3) u sum_m |x_m - xbar|
|y_m - ybar|; two evaluations (this one and numpy's) double it.  The 1 is the projection's own 1e-13 of
tests/test_rotation_host.py.  t is held to 3 sqrt(3) max|R - R_svd| |ybar| + (n + 4) u (|xbar| + sqrt(3) |ybar|) + 1e-13 max(|xbar|, |ybar|)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import ransac_ref as Rr

U = 2.0 ** -53


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler is needed (the oracle build needs one too)"
    exe = str(tmp_path_factory.mktemp("fit") / "rigid_fit_host")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tools", "rigid_fit_host.cpp"), "-o", exe])
    return exe


def _run(exe, sets):
    lines = []
    for x, y in sets:
        lines.append(str(x.shape[0]))
        lines += [" ".join(repr(float(v)) for v in np.concatenate((a, b))) for a, b in zip(x, y)]
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    res = np.array([[float(v) for v in line.split()] for line in out.stdout.strip().split("\n")])
    assert res.shape == (len(sets), 14)
    return res[:, :9].reshape(-1, 3, 3), res[:, 9:12], res[:, 12], res[:, 13]


def _sets():
    """-> [(x [n,3], y [n,3], kind)]"""
    rng = np.random.default_rng(0)
    sets = []
    for i in range(600):                                                # three points, a noisy rigid motion, three scales
        T, s = Rr.random_rigid(rng), (1e-3, 1.0, 1e3)[i % 3]
        y = rng.uniform(-2, 2, (3, 3))
        x = y @ T[:3, :3].T + T[:3, 3] + 0.01 * rng.standard_normal((3, 3))
        sets.append((s * x, s * y, "three"))
    for i, n in enumerate([4, 5, 17, 64, 65, 257, 600] * 6):            # many points; every third set has 30 % outliers
        T, s = Rr.random_rigid(rng), (1e-3, 1.0, 1e3)[i % 3]
        y = rng.uniform(-2, 2, (n, 3))
        x = y @ T[:3, :3].T + T[:3, 3] + 0.01 * rng.standard_normal((n, 3))
        if i % 3 == 2:
            bad = rng.random(n) < 0.3
            x[bad] = rng.uniform(-2, 2, (int(bad.sum()), 3))
        sets.append((s * x, s * y, "many"))
    for n in (3, 50):                                                   # far from the origin: centroids at 1e3, spread 1
        T = Rr.random_rigid(rng)
        y = rng.uniform(-0.5, 0.5, (n, 3)) + 1e3
        sets.append((y @ T[:3, :3].T + T[:3, 3], y, "far"))
    for _ in range(20):                                                 # unrelated triples: any margin
        sets.append((rng.standard_normal((3, 3)), rng.standard_normal((3, 3)), "noise"))
    for _ in range(20):                                                 # collinear on both sides
        a, b, c, d = rng.standard_normal((4, 3))
        k = np.array([0.0, 1.0, 2.5])[:, None]
        sets.append((a + k * b, c + k * d, "collinear"))
    for _ in range(10):                                                 # two of the three coincide; all three coincide
        x, y = rng.standard_normal((3, 3)), rng.standard_normal((3, 3))
        x[1], y[1] = x[0], y[0]
        sets.append((x.copy(), y.copy(), "coincident"))
        x[2], y[2] = x[0], y[0]
        sets.append((x.copy(), y.copy(), "point"))
    sets.append((rng.standard_normal((1, 3)), rng.standard_normal((1, 3)), "point"))
    for m in np.logspace(-4, -0.5, 15):                                 # nearly collinear triples: margin ~ m^2, 1e-8 .. 0.1
        y = np.array([[0, 0, 0], [1.0, 0, 0], [0.5, m, 0]]) @ Rr.random_rigid(rng)[:3, :3].T
        T = Rr.random_rigid(rng)
        sets.append((y @ T[:3, :3].T + T[:3, 3], y, "thin"))
    return sets


def test_rigid_fit_against_the_svd_fit(host_program):
    sets = _sets()
    R, t, margin, sq = _run(host_program, [(x, y) for x, y, _ in sets])
    compared = {}
    for (x, y, kind), Rg, tg, mg, sg in zip(sets, R, t, margin, sq):
        n = x.shape[0]
        Rw, tw, mw = (v[0] for v in Rr.fit(x[None], y[None]))
        assert np.abs(Rg.T @ Rg - np.eye(3)).max() <= 1e-14 and np.linalg.det(Rg) > 0, kind
        assert abs(mg - mw) <= 1e-12, (kind, mg, mw)
        xb, yb = x.mean(axis=0), y.mean(axis=0)
        scale = max(np.abs(xb).max(), np.abs(yb).max(), np.abs(x - xb).max(), np.abs(y - yb).max())
        if kind in ("collinear", "coincident", "point"):
            assert mg <= 1e-12, (kind, mg)
        if mw >= 1e-9:
            s1 = np.linalg.svd((x - xb).T @ (y - yb), compute_uv=False)[0]
            rho = (np.linalg.norm(x - xb, axis=1) * np.linalg.norm(y - yb, axis=1)).sum() / s1
            kappa = 1.0 + 4.0 * (n + 3) * U * rho / 1e-13
            dR = np.abs(Rg - Rw).max()
            assert dR * mw <= 1e-13 * kappa, (kind, n, dR, mw, kappa)
            t_bound = (3.0 * dR * np.sqrt(3.0) * np.linalg.norm(yb) + (n + 4) * U * (np.linalg.norm(xb) + np.sqrt(3.0) * np.linalg.norm(yb))
                       + 1e-13 * scale)
            assert np.abs(tg - tw).max() <= t_bound, (kind, n, np.abs(tg - tw).max(), t_bound)
            want = Rr.distances2(Rw[None], tw[None], x, y).sum()
            assert abs(sg - want) <= 1e-9 * (want + scale * scale), (kind, sg, want)       # sq_residual measures what it says
            compared[kind] = compared.get(kind, 0) + 1
            compared["kappa"] = max(compared.get("kappa", 0.0), kappa)
    assert compared["three"] >= 500 and compared["many"] == 42 and compared["far"] == 2 and compared["thin"] == 15
    assert 2.0 < compared["kappa"] < 100.0                              # the many-point sets are what the constant is about
    assert (margin[[k == "thin" for _, _, k in sets]] < 1e-6).any()     # the conditioning was exercised
