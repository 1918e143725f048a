"""The arithmetic of the FPFH kernels (csrc/fpfh_math.h: pair features, bins, the fixed-point weighting) compiled for the host
with the address and undefined-behaviour sanitizers (tools/fpfh_host.cpp, a program of its own) and compared with the numpy
restatement (tests/fpfh_ref.py).

Bins are compared on pairs that are not edge pairs (no value within 2^-30 of a bin border: there this host's atan2 and numpy's
may round apart); the test prints the smallest edge distance it saw.  The fixed-point terms and the final fp32 values are
sums, quotients and products that both sides round alike: they are compared exactly."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import fpfh_ref as F


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler is needed (the oracle build needs one too)"
    exe = str(tmp_path_factory.mktemp("fpfh") / "fpfh_host")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tools", "fpfh_host.cpp"), "-o", exe])
    return exe


def _run(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = out.stdout.strip().split("\n")
    assert len(rows) == len(lines)
    return rows


def _pair_lines(pi, ni, pk, nk):
    rows = np.concatenate((pi, ni, pk, nk), axis=1).astype(np.float64)
    return ["pair " + " ".join(repr(float(v)) for v in row) for row in rows]


def test_builtin_records(host_program):
    out = subprocess.run([host_program], input="", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [[float(v) for v in line.split()] for line in out.stdout.strip().split("\n")]
    # f = (0, 0, 0) three ways: every value mid-bin; (11 pi) / (2 pi) rounds to the double below 5.5
    assert rows == [[5, 5, 5, (11.0 * np.pi) / (2.0 * np.pi), 5.5, 5.5]] * 3


def test_bins_on_random_pairs(host_program):
    rng = np.random.default_rng(0)
    n = 100_000
    pi, pk = (rng.uniform(-1, 1, (n, 3)).astype(np.float32) for _ in range(2))
    ni, nk = F.unit_normals(rng, n), F.unit_normals(rng, n)
    nk[::7] = ni[::7]                                               # equal normals: f1 = atan2(0, 1)
    pk[::11, 2] = pi[::11, 2]
    h, edge = F.pair_bins(pi, ni, pk, nk)
    got = np.array([[float(v) for v in row.split()] for row in _run(host_program, _pair_lines(pi, ni, pk, nk))])
    t = F.bin_values(F.pair_features(pi, ni, pk, nk))
    sure = (edge >= F.EDGE).all(axis=1)
    print(f"smallest edge distance over {n} pairs: {edge.min():.3e}; {int((~sure).sum())} edge pairs left out")
    assert sure.sum() >= n - 10
    assert np.array_equal(got[sure, :3].astype(np.int64), h[sure])
    assert np.array_equal(got[:, 4:6], t[:, 1:])                    # no libm call in f2 and f3: the same bits
    assert np.abs(got[:, 3] - t[:, 0]).max() <= 2.0 ** -48          # atan2: an ulp or two of a value below 11
    assert len(set(map(tuple, h[sure]))) > 300                      # the pairs spread over the bins


def test_special_pairs(host_program):
    z, x = [0, 0, 1], [1, 0, 0]
    cases = [([0, 0, 0], z, [0, 0, 0], x),                          # len == 0
             ([0, 0, 0], z, [0, 0, 0.5], x),                        # d parallel to n1 (|a1| = 1: no swap): |v| == 0
             ([0, 0, 0], x, [0, 0, 0.5], z),                        # the swap: |a1| = 0 < |a2| = 1, then |v| == 0 again
             ([0, 0, 0], z, [0.5, 0, 0], [-0.0, -0.0, -1]),         # w . n2 = -0, n1 . n2 = -1: atan2(+0, -1) = +pi, the top bin
             ([0, 0, 0], [np.nan, 0, 1], [0.5, 0, 0], z),           # a non-finite normal
             ([0, 0, 0], [0, 0, 1e30], [0.5, 0, 0.25], [0, 0, -1e30])]   # f3 far outside [-1, 1]: clamped as a double
    arrs = [np.array([c[j] for c in cases], np.float32) for j in range(4)]
    got = np.array([[float(v) for v in row.split()] for row in _run(host_program, _pair_lines(*arrs))])
    h, _ = F.pair_bins(*arrs)
    assert np.array_equal(got[:, :3].astype(np.int64), h)
    assert h[:3].tolist() == [[5, 5, 5]] * 3 and h[4].tolist() == [5, 5, 5]
    assert h[3].tolist() == [10, 5, 5]
    assert h[5, 2] in (0, 10)


def test_fixed_point_terms_and_values_bitwise(host_program):
    rng = np.random.default_rng(1)
    m = 20_000
    used = rng.integers(1, 400, m)
    c = (rng.random(m) * (used + 1)).astype(np.int64).clip(0, used)
    d2k = rng.uniform(1e-6, 1.0, m).astype(np.float32)
    d2min = (d2k * rng.uniform(0, 1, m).astype(np.float32)).astype(np.float32)
    d2min[::5] = d2k[::5]
    d2min = np.maximum(d2min, np.float32(1e-30))
    want = np.rint(((d2min.astype(np.float64) / d2k.astype(np.float64)) * (c / used.astype(np.float64))) * F.FIX).astype(np.int64)
    lines = ["term %r %r %d %d" % (float(a), float(b), cc, u) for a, b, cc, u in zip(d2min, d2k, c, used)]
    got = np.array([int(r) for r in _run(host_program, lines)], np.int64)
    assert np.array_equal(got, want)
    assert want.max() <= 2 ** 40 and want.min() >= 0
    # whole neighbourhoods: A = sums of such terms, G = a group's total
    A = rng.integers(0, 2 ** 40, (m, 11)) * rng.integers(1, 2 ** 20, (m, 1))
    A[::9] = 0
    G = A.sum(axis=1)
    j = rng.integers(0, 11, m)
    Aj = A[np.arange(m), j]
    with np.errstate(invalid="ignore", divide="ignore"):
        nb = np.where(G != 0, (100.0 * Aj.astype(np.float64)) / G.astype(np.float64), 0.0)
    val = (nb + (100.0 * c.astype(np.float64)) / used.astype(np.float64)).astype(np.float32)
    lines = ["value %d %d %d %d" % (a, g, cc, u) for a, g, cc, u in zip(Aj, G, c, used)]
    got = np.array([float(r) for r in _run(host_program, lines)], np.float64).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), val.view(np.uint32))


def test_neighbourhood_rows_from_host_terms(host_program):
    """A whole random cloud: the restatement's weighted sums rebuilt from the host program's terms, and its rows from the
    host program's values."""
    c = F.case_dense(seed=77, n=150)
    want = F.point_fpfh(c["points"], c["normals"], c["radius"])
    i, k, d2 = want["pairs"]
    pos = d2 > 0
    i, k, d2 = i[pos], k[pos], d2[pos]
    d2min = np.full(150, np.inf, np.float32)
    np.minimum.at(d2min, i, d2)
    lines = ["term %r %r %d %d" % (float(d2min[a]), float(d), int(want["spfh"][b, j]), int(want["count"][b]))
             for a, b, d in zip(i, k, d2) for j in (0, 16, 32)]
    terms = np.array([int(r) for r in _run(host_program, lines)], np.int64).reshape(-1, 3)
    for col, j in enumerate((0, 16, 32)):
        A = np.zeros(150, np.int64)
        np.add.at(A, i, terms[:, col])
        assert np.array_equal(A, want["A"][:, j])
    G = np.repeat(want["A"].reshape(150, 3, 11).sum(axis=2), 11, axis=1)
    rows = np.nonzero(want["flags"] == 0)[0]
    lines = ["value %d %d %d %d" % (want["A"][r, j], G[r, j], want["spfh"][r, j], want["count"][r]) for r in rows for j in range(33)]
    got = np.array([float(r) for r in _run(host_program, lines)], np.float64).astype(np.float32).reshape(-1, 33)
    assert np.array_equal(got.view(np.uint32), want["fpfh"][rows].view(np.uint32))
