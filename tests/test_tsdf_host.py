"""The per-sample arithmetic of the TSDF fusion kernels (csrc/tsdf_math.h: depth value, back-projection, unit index, projection
and update, crossing) compiled for the host with the address and undefined-behaviour sanitizers (tools/tsdf_host.cpp, a program
of its own) and compared bit for bit with the numpy restatement (tests/tsdf_ref.py).  The built-in edge table (zeros, signed tiny
and huge values, infinities, NaN through every function) must run clean under the sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import tsdf_ref as T

K = (585.0, 577.5, 19.5, 14.25)
VL, ST = 3.0 / 512, 0.04


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler is needed (the oracle build needs one too)"
    exe = str(tmp_path_factory.mktemp("tsdf") / "tsdf_host")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tools", "tsdf_host.cpp"), "-o", exe])
    return exe


def _run(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [[float(v) for v in line.split()] for line in out.stdout.strip().split("\n")]
    assert len(rows) == len(lines)
    return rows


def _r(v):
    return " ".join(repr(float(x)) for x in np.ravel(v))


def _pose(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    T4 = np.eye(4)
    T4[:3, :3] = q * np.sign(np.linalg.det(q))
    T4[:3, 3] = rng.uniform(-1, 1, 3)
    return T4


def test_edge_table_runs_clean(host_program):
    out = subprocess.run([host_program], input="", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ["edges", str(21 * 21 * 12), "1"]


def test_depth_values_at_the_truncation(host_program):
    raws = [0, 1, 999, 1000, 5999, 6000, 6001, 65535]
    got = _run(host_program, [f"depth {r} 1000 6.0" for r in raws] + ["depth 6000 999.5 6.0", "depth 3 7 6.0"])
    want = T.depth_values(np.array(raws, np.uint16), 1000.0, 6.0).tolist() + T.depth_values(np.array([6000], np.uint16), 999.5, 6.0).tolist() \
        + T.depth_values(np.array([3], np.uint16), 7.0, 6.0).tolist()
    assert [np.float32(g[0]) for g in got] == [np.float32(w) for w in want]
    assert want[5] == 6.0 and want[6] == 0.0 and want[0] == 0.0        # at depth_trunc: kept; just above: no measurement


def test_samples_and_unit_spans(host_program):
    rng = np.random.default_rng(0)
    lines, want = [], []
    for _ in range(300):
        u, v, raw = int(rng.integers(0, 40)), int(rng.integers(0, 30)), int(rng.integers(1, 6000))
        T4 = _pose(rng)
        lines.append(f"sample {u} {v} {raw} 1000 6.0 {_r(K)} {ST!r} {16 * VL!r} {_r(T4[:3])}")
        d = T.depth_values(np.array([raw], np.uint16), 1000.0, 6.0)
        p = T.transform(T4, T.back_project(np.float64(u), np.float64(v), d, K))[0]
        lo, hi = np.floor((p - ST) / (16 * VL)), np.floor((p + ST) / (16 * VL))
        want.append([float(d[0]), *p, lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]])
    got = _run(host_program, lines)
    assert np.array_equal(np.array(got)[:, 1:], np.array(want)[:, 1:])           # %.17g round-trips a double
    assert np.array_equal(np.array(got)[:, 0].astype(np.float32), np.array(want)[:, 0].astype(np.float32))
    assert (np.array(want)[:, 4:] < 0).any()                                     # negative coordinates: floor, not truncation


def test_voxel_projection(host_program):
    rng = np.random.default_rng(1)
    lines, want = [], []
    for _ in range(300):
        unit, idx = rng.integers(-6, 7, 3), rng.integers(0, 16, 3)
        T4 = np.linalg.inv(_pose(rng))
        lines.append(f"voxel {_r(unit)} {_r(idx)} {VL!r} {_r(K)} 40 30 {_r(T4[:3])}")
        p = ((16 * unit + idx).astype(np.float64) + 0.5) * VL
        c = T.transform(T4, p[None])[0]
        fx, fy, cx, cy = K
        uf, vf = ((c[0] * fx) / c[2] + cx) + 0.5, ((c[1] * fy) / c[2] + cy) + 0.5
        vis = bool(c[2] > 0 and 0 <= uf < 40 and 0 <= vf < 30)
        want.append([*p, *c, int(vis), int(uf) if vis else -1, int(vf) if vis else -1])
    assert np.array_equal(np.array(_run(host_program, lines)), np.array(want))


def test_observation_update_and_crossing(host_program):
    rng = np.random.default_rng(2)
    fx, fy, cx, cy = K
    lines, want = [], []
    for i in range(400):
        raw, pu, pv = int(rng.integers(0, 3000)), int(rng.integers(0, 40)), int(rng.integers(0, 30))
        z = raw / 1000.0 + rng.uniform(-0.08, 0.08) if i % 4 else raw / 1000.0 / 1.0000001
        tsdf, w = np.float32(rng.uniform(-1, 1)), int(rng.integers(0, 64))
        lines.append(f"observe {raw} 1000 6.0 {z!r} {pu} {pv} {_r(K)} {ST!r} {float(tsdf)!r} {w}")
        d = T.depth_values(np.array([raw], np.uint16), 1000.0, 6.0)[0]
        a, b = (pu - cx) / fx, (pv - cy) / fy
        sdf = (np.float64(d) - z) * np.sqrt((a * a + b * b) + 1.0)
        seen = bool(d != 0 and sdf > -ST)
        t = np.float32(min(1.0, sdf / ST)) if seen else np.float32(0)
        new = (tsdf * np.float32(w) + t) / (np.float32(w) + np.float32(1)) if seen else tsdf
        assert new.dtype == np.float32
        want.append([int(seen), t, new, w + seen])
    got = np.array(_run(host_program, lines))
    assert np.array_equal(got.astype(np.float32).view(np.uint32), np.array(want, dtype=np.float32).view(np.uint32))
    assert 0 < got[:, 0].sum() < len(lines) and (got[:, 1] == 1).any()          # both outcomes, and the clamp at 1

    def cross_want(f0, w0, f1, w1, p0):
        f0, f1 = np.float32(f0), np.float32(f1)
        c = bool(np.float64(f0) * np.float64(f1) < 0)
        r0, r1 = abs(np.float64(f0)), abs(np.float64(f1))
        return [w0 != 0 and -T.BAND <= f0 < T.BAND, w1 != 0 and -T.BAND <= f1 < T.BAND, c,
                np.float32((p0 * r1 + (p0 + VL) * r0) / (r0 + r1)) if c else 0]

    cases = [(rng.uniform(-1.05, 1.05), int(rng.integers(0, 3)), rng.uniform(-1.05, 1.05), int(rng.integers(0, 3)), rng.uniform(-3, 3))
             for _ in range(300)]
    # a product that underflows in fp32 still crosses; a zero does not; the band is closed below and open above
    cases += [(1e-30, 1, -1e-30, 1, 0.5), (0.0, 1, -0.5, 1, 0.5), (-0.98, 1, 0.98, 1, 0.5), (0.97999, 0, -0.5, 1, -0.25)]
    lines = [f"cross {float(np.float32(f0))!r} {w0} {float(np.float32(f1))!r} {w1} {p0!r} {VL!r}" for f0, w0, f1, w1, p0 in cases]
    want = [cross_want(*c) for c in cases]
    assert want[300][:3] == [True, True, True] and want[301][2] is False and want[302][:2] == [True, False]
    got = np.array(_run(host_program, lines))
    assert np.array_equal(got.astype(np.float32).view(np.uint32), np.array(want, dtype=np.float32).view(np.uint32))
