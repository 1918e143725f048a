"""The arithmetic of the ICP stage (csrc/icp_math.h: the pair's fixed-point terms, the transform's fma chain, the point-to-point
and point-to-plane solves, the Cayley map, the composition, the stop test and the failure flags), compiled for the host with the
address and undefined-behaviour sanitizers (tools/icp_host.cpp, a program of its own) and compared with the restatement
tests/icp_ref.py: integers and the fma chain exactly, a transform within T_TOL where the restatement's own bound (solve_bound)
allows it, and over an edge table -- zero sums, a rank-deficient J^T J, counts exactly 3 / 6 and one short, huge and tiny scales."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import icp_ref as I


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a C++ compiler is needed (the oracle build needs one too)"
    exe = str(tmp_path_factory.mktemp("icp") / "icp_host")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tools", "icp_host.cpp"), "-o", exe])
    return exe


def _ask(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = out.stdout.strip().split("\n")
    assert len(rows) == len(lines)
    return [r.split() for r in rows]


def _fmt(vals):
    return " ".join(repr(float(v)) for v in np.asarray(vals, dtype=np.float64).reshape(-1))


def _step_line(plane, m, it, rel_f, rel_r, pf, pr, T, S):
    return f"step {int(plane)} {m} {it} {_fmt([rel_f, rel_r, pf, pr])} {_fmt(T)} " + " ".join(str(int(s)) for s in S)


def _pairs(rng, k, scale=1.0):
    p = (scale * rng.uniform(-1, 1, (k, 3))).astype(np.float32)
    q = (p + 0.02 * scale * rng.standard_normal((k, 3))).astype(np.float32)
    n = I.unit_normals(rng.standard_normal((k, 3)))
    return p, q, n


def _sums(p, q, n, plane):
    return I.accumulate(p, q, np.arange(len(p), dtype=np.int32), n if plane else None)


def test_terms_and_transform_are_exact(host_program):
    rng = np.random.default_rng(1)
    p, q, n = _pairs(rng, 40, 3.0)
    q[5, 0], p[6, 1], n[7] = 64.00001, -65.0, (1.0000001, 0, 0)                    # out of range: q, p, the normal
    lines = [f"terms {pl} {_fmt(p[i])} {_fmt(q[i])} {_fmt(n[i])}" for pl in (0, 1) for i in range(40)]
    got = _ask(host_program, lines)
    for pl in (0, 1):
        for i in range(40):
            S = _sums(p[i:i + 1], q[i:i + 1], n[i:i + 1], pl)
            row = [int(v) for v in got[40 * pl + i]]
            assert row[0] == S[30] and (row[0] == 1) == (i in (5, 6) or (pl == 1 and i == 7))
            assert row[1:] == [0 if e == 30 else S[e] for e in range(32)], (pl, i)
    Ts = [I.rigid(rng.standard_normal(3), rng.standard_normal(3)) for _ in range(20)]
    s = rng.uniform(-4, 4, (20, 3)).astype(np.float32)
    got = _ask(host_program, [f"transform {_fmt(T[:3])} {_fmt(x)}" for T, x in zip(Ts, s)])
    for T, x, row in zip(Ts, s, got):
        assert np.array_equal(np.array([float(v) for v in row], dtype=np.float32), I.transform(T, x[None])[0])


def test_cayley_matches_the_restatement_bit_for_bit(host_program):
    rng = np.random.default_rng(2)
    ws = [rng.standard_normal(3) * s for s in (1e-9, 1e-3, 0.3, 1.0, 50.0) for _ in range(10)] + [np.zeros(3)]
    got = _ask(host_program, ["cayley " + _fmt(w) for w in ws])
    for w, row in zip(ws, got):
        assert np.array_equal(np.array([float(v) for v in row]).reshape(3, 3), I.cayley([float(v) for v in w]))


def _compare(host_program, cases):
    """cases: [(plane, m, it, rel_f, rel_r, pf, pr, T, S)] -> the rows, each compared with the restatement's step"""
    got = _ask(host_program, [_step_line(*c) for c in cases])
    seen = {}
    for c, row in zip(cases, got):
        plane, m, it, rel_f, rel_r, pf, pr, T, S = c
        flags, T2, rec, fit, rmse, info = I.step(plane, S, m, it, rel_f, rel_r, pf, pr, T)
        v = [float(x) for x in row]
        if int(v[0]) != flags:
            # only a solve whose conditioning sits at the threshold may be judged differently by two correct evaluations
            assert {int(v[0]), flags} == {0, I.SINGULAR} and not plane and abs(info["conditioning"] - I.MARGIN_MIN) < 1e-9, c
            continue
        assert v[1] == fit and abs(v[2] - rmse) <= 1e-15 * max(rmse, 1.0)
        assert v[3 + 16] == rec[16] and v[3 + 17] == rec[17] and v[3 + 19] == rec[19]
        Tg = np.array(v[3:19]).reshape(4, 4)
        assert np.array_equal(Tg[3], [0, 0, 0, 1])
        if flags:
            assert np.array_equal(Tg[:3], np.asarray(T, dtype=np.float64).reshape(4, 4)[:3])     # left as it was
        elif info["bound"] <= I.T_TOL:
            assert np.abs(Tg - T2).max() <= I.T_TOL, (c, np.abs(Tg - T2).max())
            assert np.abs(Tg[:3, :3] @ Tg[:3, :3].T - np.eye(3)).max() <= 1e-12
            seen["held"] = seen.get("held", 0) + 1
        seen[flags] = seen.get(flags, 0) + 1
    return seen


def test_steps_against_the_restatement(host_program):
    rng = np.random.default_rng(3)
    cases = []
    for i in range(120):
        plane, k = i % 2 == 1, int(rng.integers(20, 400))
        p, q, n = _pairs(rng, k, (0.1, 1.0, 10.0)[i % 3])
        T = I.rigid(0.2 * rng.standard_normal(3), rng.standard_normal(3))
        cases.append((plane, k + int(rng.integers(0, 50)), i % 4, 1e-6, 1e-6, 0.5, 0.01, T, _sums(p, q, n, plane)))
    seen = _compare(host_program, cases)
    assert seen.get("held", 0) >= 100 and seen.get(0, 0) >= 100


def test_edge_table(host_program):
    rng = np.random.default_rng(4)
    T0 = I.rigid([0.1, 0.2, -0.1], [0.3, -0.2, 0.1])
    cases, want = [], []

    def add(plane, S, flags, m=100, it=0, pf=0.0, pr=0.0, rel=1e-6):
        cases.append((plane, m, it, rel, rel, pf, pr, T0, S))
        want.append(flags)

    for plane in (False, True):
        add(plane, [0] * 32, I.FEW)                                                  # zero sums
        need = 6 if plane else 3
        for k, flags in ((need - 1, I.FEW), (need, None)):                           # one short, and exactly enough
            p, q, n = _pairs(rng, k)
            add(plane, _sums(p, q, n, plane), flags)
        p, q, n = _pairs(rng, 50)
        S = _sums(p, q, n, plane)
        bad = list(S)
        bad[30] = 1
        add(plane, bad, I.RANGE)                                                     # an out-of-range pair comes first
        fit, rmse = 50 / 100.0, np.sqrt(float(S[29 if plane else 16]) / I.SQ / 50.0)
        add(plane, S, I.CONVERGED, it=3, pf=fit, pr=rmse)                            # no change: converged
        add(plane, S, 0, it=0, pf=fit, pr=rmse)                                      # ... but never at iteration 0
        add(plane, S, 0, it=3, pf=fit, pr=rmse, rel=0.0)                             # ... nor with zero thresholds
        for scale in (2.0 ** -10, 60.0):                                             # tiny and huge coordinates
            p, q, n = _pairs(rng, 80, scale)
            add(plane, _sums(p, q, n, plane), None if scale < 1 else 0)
    # rank-deficient J^T J: all normals parallel; and every point on one line for point-to-point
    p, q, n = _pairs(rng, 60)
    n[:] = (0.0, 0.0, 1.0)
    add(True, _sums(p, q, n, True), I.SINGULAR)
    line = (np.linspace(-1, 1, 30)[:, None] * np.array([[1.0, 0.5, -0.25]])).astype(np.float32)
    add(False, _sums(line, (line + np.float32(0.01)).astype(np.float32), n[:30], False), I.SINGULAR)
    same = np.tile(np.array([[0.25, 0.5, -0.125]], dtype=np.float32), (10, 1))
    add(False, _sums(same, same, n[:10], False), I.SINGULAR)                         # every pair the same point
    got = _ask(host_program, [_step_line(*c) for c in cases])
    for c, w, row in zip(cases, want, got):
        if w is not None:
            assert int(row[0]) == w, (c[0], c[8][:2], int(row[0]), w)
        assert all(np.isfinite(float(v)) for v in row[3:19])                         # T stays a finite matrix
    _compare(host_program, cases)


def test_hand_derived_answers_bind_the_shipped_arithmetic(host_program):
    """The lattice shift and the rotation about the centroid of tests/test_icp_spec.py, with the sums built by the host
    program's own `terms` (one line per pair, added here as integers) and stepped by its `step`: the answers derived by hand
    hold for csrc/icp_math.h, not only for the restatement."""
    ax = (np.arange(5) - 2) * 0.25
    tgt = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    shift = np.array([2.0 ** -4, -(2.0 ** -5), 3 * 2.0 ** -5])
    truth = I.rigid([0.0, 0.0, 0.05], [0.0, 0.0, 0.0])
    P = tgt.astype(np.float64)
    s = np.linalg.svd(P.T @ P, compute_uv=False)
    c = float(np.abs(tgt).max())
    rot_bound = 2.0 * 3.0 * len(tgt) * (2.0 ** -25 + 2.0 * 2.0 ** -25 * c * c) / (s[0] * ((s[1] + s[2]) / s[0]))
    want_shift = np.eye(4)
    want_shift[:3, 3] = shift
    for src, want, bound in (((P - shift).astype(np.float32), want_shift, 1e-12),
                             ((P @ truth[:3, :3]).astype(np.float32), truth, max(rot_bound, 3.0 * rot_bound * c + 2.0 ** -25 * 3 * c))):
        moved = _ask(host_program, [f"transform {_fmt(np.eye(4)[:3])} {_fmt(x)}" for x in src])
        q = np.array([[float(v) for v in row] for row in moved], dtype=np.float32)
        assert np.array_equal(q, src)                                                # the identity moves nothing
        rows = _ask(host_program, [f"terms 0 {_fmt(p)} {_fmt(x)} 0 0 1" for p, x in zip(tgt, q)])
        S = [sum(int(r[1 + e]) for r in rows) for e in range(32)]
        assert all(int(r[0]) == 0 for r in rows) and S == I.accumulate(tgt, q, np.arange(len(tgt), dtype=np.int32))
        out = _ask(host_program, [_step_line(False, len(tgt), 0, 1e-6, 1e-6, 0.0, 0.0, np.eye(4), S)])[0]
        T1 = np.array([float(v) for v in out[3:19]]).reshape(4, 4)
        assert int(out[0]) == 0 and float(out[3 + 16]) == len(tgt)
        assert np.abs(T1 - want).max() <= bound, np.abs(T1 - want).max()
    # the second iteration of the lattice: from the recovered shift every distance is zero, and the third sees no change
    T1 = want_shift
    q = I.transform(T1, (P - shift).astype(np.float32))
    S = I.accumulate(tgt, q, np.arange(len(tgt), dtype=np.int32))
    out = _ask(host_program, [_step_line(False, len(tgt), 1, 1e-6, 1e-6, 1.0, float(np.linalg.norm(shift)), T1, S),
                              _step_line(False, len(tgt), 2, 1e-6, 1e-6, 1.0, 0.0, T1, S)])
    assert int(out[0][0]) == 0 and float(out[0][2]) == 0.0 and int(out[1][0]) == I.CONVERGED
