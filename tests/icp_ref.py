"""Numpy restatement of the ICP stage, written from include/epn_so3conv.h (epn_icp_refine_f32) and DESIGN.md 3.1m, not from the
kernel.  The transform's fma chain is exact rational arithmetic rounded once (this Python has no math.fma; float(Fraction) rounds
correctly), the search is tests/grid_nn_ref.py's brute force in the stated fp32 order, the sums are Python ints, the solve is
Python floats (every operation rounded on its own, in the header's order) with numpy's SVD for the projection.

What may be compared exactly with a device result, and what within T_TOL: correspondences, counts and the integer sums of an
iteration are exact GIVEN the bits of the transform it starts from; the transform after it and the rmse are held to T_TOL, which
bounds the distance between two correct fp64 evaluations of the step (solve_bound; derivation in DESIGN.md 3.1m).  The case
builders (checked_run) assert on the CPU that no decision of their reference run sits on a rounding error."""
import math
from fractions import Fraction

import numpy as np

import grid_nn_ref as G

NS, REC = 32, 20
MAX_M, MAX_ITER = 2 ** 20, 1024
LIN, SQ = 2.0 ** 32, 2.0 ** 24
COORD_MAX = 64.0
MARGIN_MIN, PIVOT_MIN = 1e-6, 2.0 ** -20
CONVERGED, FEW, SINGULAR, RANGE = 1, 2, 4, 8
T_TOL = 1e-9                 # the builders assert solve_bound <= T_TOL for every iteration of their runs
D2_GAP = 2.0 ** -22          # no candidate's d2 within r2 (1 +- D2_GAP): four fp32 ulps, d2 carrying three roundings
STOP_GAP = 2.0               # no change of rmse within [rel_rmse / STOP_GAP, rel_rmse * STOP_GAP] when it decides the stop
MARGIN_OK, PIVOT_OK = 1e-3, 2.0 ** -12
U = 2.0 ** -53


def fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def transform(T, src):
    """q_i = (float)fma(T_i0, s_0, fma(T_i1, s_1, fma(T_i2, s_2, T_i3))) -> float32 [m,3]; non-finite rows become NaN rows (they
    match nothing either way)."""
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    src = np.asarray(src, dtype=np.float32).reshape(-1, 3)
    out = np.full(src.shape, np.nan, dtype=np.float32)
    Tf = [[Fraction(float(T[i, j])) for j in range(4)] for i in range(3)]
    for r in np.flatnonzero(np.isfinite(src).all(axis=1)):
        s = [Fraction(float(v)) for v in src[r]]
        for i in range(3):
            v = float(Tf[i][2] * s[2] + Tf[i][3])
            v = float(Tf[i][1] * s[1] + Fraction(v))
            v = float(Tf[i][0] * s[0] + Fraction(v))
            out[r, i] = np.float32(v)
    return out


def term_table(plane):
    """[(e, ia, ib, scale)] of the sums that are products of two of the pair's values."""
    if not plane:
        t = [(0, 6, 6, 1.0)] + [(1 + i, i, 6, LIN) for i in range(3)] + [(4 + i, 3 + i, 6, LIN) for i in range(3)]
        t += [(7 + 3 * i + j, i, 3 + j, SQ) for i in range(3) for j in range(3)] + [(16, 7, 6, SQ)]
        return t
    t, e = [(0, 7, 7, 1.0)], 1
    for i in range(6):
        for j in range(i, 6):
            t.append((e, i, j, SQ))
            e += 1
    return t + [(22 + i, i, 6, SQ) for i in range(6)] + [(28, 6, 6, SQ), (29, 8, 7, SQ)]


def pair_values(p, q, n=None):
    """(p, q float32 [k,3], n float32 [k,3] or None) -> (V float64 [k,9], bad bool [k]) in the header's operation order."""
    P, Q = p.astype(np.float64), q.astype(np.float64)
    d = Q - P
    dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    with np.errstate(invalid="ignore"):
        bad = ~((np.abs(P) <= COORD_MAX).all(axis=1) & (np.abs(Q) <= COORD_MAX).all(axis=1))
    one, zero = np.ones(len(P)), np.zeros(len(P))
    if n is None:
        return np.stack((P[:, 0], P[:, 1], P[:, 2], Q[:, 0], Q[:, 1], Q[:, 2], one, dd, zero), axis=1), bad
    N = n.astype(np.float64)
    with np.errstate(invalid="ignore"):
        bad |= ~(np.abs(N) <= 1.0).all(axis=1)
        c0 = Q[:, 1] * N[:, 2] - Q[:, 2] * N[:, 1]
        c1 = Q[:, 2] * N[:, 0] - Q[:, 0] * N[:, 2]
        c2 = Q[:, 0] * N[:, 1] - Q[:, 1] * N[:, 0]
        r = (d[:, 0] * N[:, 0] + d[:, 1] * N[:, 1]) + d[:, 2] * N[:, 2]
    return np.stack((c0, c1, c2, N[:, 0], N[:, 1], N[:, 2], r, one, dd), axis=1), bad


def accumulate(tgt, q, nn_idx, normals=None):
    """The row of 32 integer sums of the matched pairs (Python ints)."""
    S = [0] * NS
    rows = np.flatnonzero(nn_idx >= 0)
    if rows.size == 0:
        return S
    mate = nn_idx[rows]
    V, bad = pair_values(np.asarray(tgt, dtype=np.float32)[mate], q[rows], None if normals is None else
                         np.asarray(normals, dtype=np.float32)[mate])
    S[30] = int(bad.sum())
    V = V[~bad]
    for e, ia, ib, scale in term_table(normals is not None):
        prod = V[:, ia] * V[:, ib]
        S[e] = sum(int(v) for v in np.rint(prod * scale))
    return S


def project(C):
    """(R maximising tr(R^T C), margin = (s2 + d s3) / s1) by numpy's SVD."""
    Uc, s, Vt = np.linalg.svd(C)
    d = 1.0 if np.linalg.det(Uc @ Vt) > 0 else -1.0
    R = Uc @ np.diag([1.0, 1.0, d]) @ Vt
    return R, ((s[1] + d * s[2]) / s[0] if s[0] > 0 else 0.0)


def p2p_system(S):
    N = float(S[0])
    sp = [float(S[1 + i]) / LIN for i in range(3)]
    sq = [float(S[4 + i]) / LIN for i in range(3)]
    C = np.array([[float(S[7 + 3 * i + j]) / SQ - (sp[i] * sq[j]) / N for j in range(3)] for i in range(3)])
    return np.array([v / N for v in sp]), np.array([v / N for v in sq]), C, sp, sq


def p2p_solve(S):
    pb, qb, C, _, _ = p2p_system(S)
    R, margin = project(C)
    return (0 if margin > MARGIN_MIN else SINGULAR), R, pb - R @ qb, margin


def cayley(w):
    a = [0.5 * w[0], 0.5 * w[1], 0.5 * w[2]]
    aa = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
    k, den = 1.0 - aa, 1.0 + aa
    return np.array([[(k + w[0] * a[0]) / den, (w[0] * a[1] - w[2]) / den, (w[0] * a[2] + w[1]) / den],
                     [(w[1] * a[0] + w[2]) / den, (k + w[1] * a[1]) / den, (w[1] * a[2] - w[0]) / den],
                     [(w[2] * a[0] - w[1]) / den, (w[2] * a[1] + w[0]) / den, (k + w[2] * a[2]) / den]])


def plane_system(S):
    A, e = [[0.0] * 6 for _ in range(6)], 1
    for i in range(6):
        for j in range(i, 6):
            A[i][j] = A[j][i] = float(S[e]) / SQ
            e += 1
    return A, [float(S[22 + i]) / SQ for i in range(6)]


def plane_solve(S):
    """-> (flags, dR, dt, the smallest d_k / A_kk)"""
    A, b = plane_system(S)
    L, d, singular, ratio = [[0.0] * 6 for _ in range(6)], [0.0] * 6, False, math.inf
    with np.errstate(all="ignore"):
        for k in range(6):
            dk = A[k][k]
            for j in range(k):
                dk = dk - (L[k][j] * d[j]) * L[k][j]
            if not dk > PIVOT_MIN * A[k][k]:
                singular = True
            ratio = min(ratio, dk / A[k][k] if A[k][k] > 0 else 0.0)
            d[k] = dk
            for i in range(k + 1, 6):
                v = A[i][k]
                for j in range(k):
                    v = v - (L[i][j] * d[j]) * L[k][j]
                L[i][k] = float(np.float64(v) / np.float64(dk))
    if singular:
        return SINGULAR, None, None, ratio
    y, x = [0.0] * 6, [0.0] * 6
    for i in range(6):
        v = -b[i]
        for j in range(i):
            v = v - L[i][j] * y[j]
        y[i] = v
    for i in range(5, -1, -1):
        v = y[i] / d[i]
        for j in range(i + 1, 6):
            v = v - L[j][i] * x[j]
        x[i] = v
    if not all(math.isfinite(v) for v in x):
        return SINGULAR, None, None, ratio
    return 0, cayley(x[:3]), np.array(x[3:]), ratio


def compose(dR, dt, T):
    out = np.array(T, dtype=np.float64).reshape(4, 4).copy()
    Tn = out.copy()
    for i in range(3):
        for j in range(4):
            out[i, j] = (dR[i, 0] * Tn[0, j] + dR[i, 1] * Tn[1, j]) + dR[i, 2] * Tn[2, j]
        out[i, 3] = out[i, 3] + dt[i]
    return out


def step(plane, S, m, it, rel_fitness, rel_rmse, prev_fitness, prev_rmse, T):
    """-> (flags, T_next, rec float64 [20], fitness, rmse, info): info holds what the builders' conditions look at."""
    T = np.array(T, dtype=np.float64).reshape(4, 4).copy()
    N, ssd = float(S[0]), float(S[29 if plane else 16]) / SQ
    rmse = math.sqrt(ssd / N) if S[0] > 0 else 0.0
    fitness = N / float(m)
    info = dict(d_fitness=abs(fitness - prev_fitness), d_rmse=abs(rmse - prev_rmse), conditioning=None, bound=0.0)
    flags = 0
    if S[30] != 0:
        flags = RANGE
    elif S[0] < (6 if plane else 3):
        flags = FEW
    elif it > 0 and info["d_fitness"] < rel_fitness and info["d_rmse"] < rel_rmse:
        flags = CONVERGED
    else:
        if plane:
            flags, dR, dt, info["conditioning"] = plane_solve(S)
        else:
            flags, dR, dt, info["conditioning"] = p2p_solve(S)
        if flags == 0:
            info["bound"] = solve_bound(S, plane, T)
            T = compose(dR, dt, T)
    T[3] = (0.0, 0.0, 0.0, 1.0)
    rec = np.concatenate((T.reshape(-1), [N, ssd, rmse, float(flags)]))
    return flags, T, rec, fitness, rmse, info


def solve_bound(S, plane, T):
    """A bound on max|T' - T''| between two correct fp64 evaluations of the step from the same integer sums.
    Point-to-point: an entry of C carries four roundings on |S_pq| / 2^24 + |sp_i sq_j| / N, so |dC|_F <= 4 u |that|_F per
    evaluation; the projection moves by at most 2 |dC| / (s1 margin) and has 1e-13 of its own
    (tests/test_rotation_host.py); dt follows dR through |qbar|.  Point-to-plane: LDL^T of a positive definite matrix is backward
    stable, |dx| <= 8 n^2 u cond(A) |x| with n = 6 per evaluation.  Either way dT enters T' = dT T through max|T| <= |t| + 1."""
    Tmax = 1.0 + np.abs(np.asarray(T)[:3, 3]).max()
    if not plane:
        pb, qb, C, sp, sq = p2p_system(S)
        N = float(S[0])
        mag = np.array([[abs(float(S[7 + 3 * i + j])) / SQ + abs(sp[i] * sq[j]) / N for j in range(3)] for i in range(3)])
        s = np.linalg.svd(C, compute_uv=False)
        _, margin = project(C)
        dR = (1e-13 + 2.0 * 2.0 * 4.0 * U * np.linalg.norm(mag) / s[0]) / margin
        dt = 3.0 * dR * np.abs(qb).max() + 8.0 * U * (np.abs(pb).max() + 3.0 * np.abs(qb).max())
        return 3.0 * dR * Tmax + dt
    A, b = plane_system(S)
    x = np.linalg.solve(np.array(A), -np.array(b))
    dx = 2.0 * 8.0 * 36.0 * U * np.linalg.cond(np.array(A)) * np.abs(x).max()
    return 3.0 * (dx + 16.0 * U) * Tmax + dx


def iterate_from(tgt, src, T, max_dist, normals=None, valid=None):
    """One iteration's integer half from the bits of T: -> (q float32 [m,3], nn_idx int32 [m], d2 float32 [m], S)."""
    q = transform(T, src)
    nn_idx, d2 = G.nearest(tgt, q, max_dist, valid=valid)
    return q, nn_idx, d2, accumulate(tgt, q, nn_idx, normals)


def run(tgt, src, T_init, max_dist, max_iter, rel_fitness=1e-6, rel_rmse=1e-6, normals=None, valid=None):
    """The whole loop -> dict(T, trace [max_iter,20], iterations, status, sums, nn_idx, steps): sums and nn_idx of the last live
    iteration, steps = per live iteration dict(T_in, q, nn_idx, d2, S, flags, info)."""
    src = np.asarray(src, dtype=np.float32).reshape(-1, 3)
    m, plane = src.shape[0], normals is not None
    T = np.array(T_init, dtype=np.float64).reshape(4, 4).copy()
    T[3] = (0.0, 0.0, 0.0, 1.0)
    trace = np.zeros((max_iter, REC))
    out = dict(iterations=0, status=0, sums=[0] * NS, nn_idx=np.full(m, -1, dtype=np.int32), steps=[])
    if m == 0 or max_iter == 0:
        trace[:, :16] = T.reshape(-1)
        return dict(out, T=T, trace=trace)
    pf = pr = 0.0
    stopped = False
    for it in range(max_iter):
        if stopped:
            trace[it] = trace[it - 1]
            continue
        q, nn_idx, d2, S = iterate_from(tgt, src, T, max_dist, normals, valid)
        T_in = T
        flags, T, rec, pf, pr, info = step(plane, S, m, it, rel_fitness, rel_rmse, pf, pr, T)
        trace[it] = rec
        out["steps"].append(dict(T_in=T_in, q=q, nn_idx=nn_idx, d2=d2, S=S, flags=flags, info=info, it=it))
        out["sums"], out["nn_idx"] = S, nn_idx
        out["status"] |= flags
        out["iterations"] += flags == 0
        stopped = flags != 0
    return dict(out, T=T, trace=trace)


def check_conditions(ref, tgt, max_dist, rel_fitness, rel_rmse, valid=None, edge_rows=()):
    """-> None when no decision of the run sits on a rounding error, else the reason.  edge_rows: source rows whose distance
    to the bound is constructed exactly by the case."""
    tgt = np.asarray(tgt, dtype=np.float32).reshape(-1, 3)
    r2 = np.float32(np.float64(max_dist) * np.float64(max_dist))
    part = G.participates(tgt, valid)
    for s in ref["steps"]:
        rows = np.setdiff1d(np.flatnonzero(np.isfinite(s["q"]).all(axis=1)), np.asarray(edge_rows, dtype=np.int64))
        if rows.size and part.any():
            d = s["q"][rows, None, :].astype(np.float64) - tgt[None, part, :].astype(np.float64)
            d2 = (d * d).sum(axis=2)
            if (np.abs(d2 - np.float64(r2)) <= D2_GAP * np.float64(r2)).any():
                return f"iteration {s['it']}: a candidate's d2 within the gap of r2"
        info = s["info"]
        if s["it"] > 0 and s["flags"] in (0, CONVERGED) and info["d_fitness"] < rel_fitness:
            if rel_rmse > 0 and rel_rmse / STOP_GAP <= info["d_rmse"] <= rel_rmse * STOP_GAP:
                return f"iteration {s['it']}: the change of rmse {info['d_rmse']} within the gap of {rel_rmse}"
        if s["flags"] == 0:
            if info["conditioning"] < (PIVOT_OK if "plane" in ref and ref["plane"] else MARGIN_OK):
                return f"iteration {s['it']}: conditioning {info['conditioning']}"
            if not info["bound"] <= T_TOL:
                return f"iteration {s['it']}: solve bound {info['bound']} above T_TOL"
    return None


def checked_run(make, what, max_iter, rel_fitness=1e-6, rel_rmse=1e-6, seeds=range(64)):
    """make(seed) -> dict(tgt, src, T_init, max_dist[, normals, valid, edge_rows]).  The first seed whose reference run meets
    check_conditions -> (case, ref)."""
    reason = None
    for seed in seeds:
        case = make(seed)
        ref = run(case["tgt"], case["src"], case["T_init"], case["max_dist"], max_iter, rel_fitness, rel_rmse,
                  normals=case.get("normals"), valid=case.get("valid"))
        ref["plane"] = case.get("normals") is not None
        reason = check_conditions(ref, case["tgt"], case["max_dist"], rel_fitness, rel_rmse, case.get("valid"),
                                  case.get("edge_rows", ()))
        if reason is None:
            return case, ref
    raise AssertionError(f"{what}: no seed meets the conditions ({reason})")


def rigid(axis_angle, t):
    """[4,4] from a rotation vector (Rodrigues, numpy) and a translation."""
    w = np.asarray(axis_angle, dtype=np.float64)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / (th if th > 0 else 1.0)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * (K @ K)
    T[:3, 3] = t
    return T


def unit_normals(n):
    """rows scaled to unit length in fp64, rounded to fp32 (every component stays within 1)."""
    n = np.asarray(n, dtype=np.float64)
    return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)


def corner_scene(rng, n_per=400, noise=0.0, extent=1.0):
    """Three orthogonal planes meeting at the origin (a room corner) -> (points float32 [3 n_per,3], normals float32)."""
    pts, nrm = [], []
    for a in range(3):
        p = rng.uniform(0.05, extent, (n_per, 3))
        p[:, a] = noise * rng.standard_normal(n_per)
        n = np.zeros((n_per, 3))
        n[:, a] = 1.0
        pts.append(p)
        nrm.append(n)
    return np.concatenate(pts).astype(np.float32), np.concatenate(nrm).astype(np.float32)


def cap_and_corner(rng, n=2000, noise=0.002):
    """A sphere cap next to a box corner, with Gaussian noise along the normal -> (points float32 [n,3], normals float32 [n,3])."""
    k = n // 2
    u = rng.uniform(0.6, 1.0, k)
    phi = rng.uniform(0, 2 * math.pi, k)
    s = np.sqrt(1 - u * u)
    nc = np.stack((s * np.cos(phi), s * np.sin(phi), u), axis=1)
    cap = 0.5 * nc + np.array([-0.6, 0.0, 0.0]) + noise * rng.standard_normal(k)[:, None] * nc
    cor, ncor = corner_scene(rng, (n - k) // 3, noise=0.0, extent=0.8)
    cor = cor.astype(np.float64) + noise * rng.standard_normal(len(cor))[:, None] * ncor + np.array([0.3, -0.4, -0.4])
    return np.concatenate((cap, cor)).astype(np.float32), np.concatenate((nc.astype(np.float32), ncor))
