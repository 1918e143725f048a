// The arithmetic of csrc/icp_refine.hip that needs no device: the rigid transform of a source point, the fixed-point terms one
// correspondence adds to the sums of an ICP iteration, and the step from those sums to the next transform -- the Horn fit of
// rigid_fit.h for point-to-point, a pivot-free LDL^T of the 6 x 6 normal equations and the Cayley map for point-to-plane, the
// composition, open3d's stop test and the failure flags.  Plain C++ on doubles, compiled into the kernels by hipcc and into a
// host program by any C++ compiler (tools/icp_host.cpp, which tests/test_icp_host.py builds with the address and
// undefined-behaviour sanitizers and compares with the numpy restatement tests/icp_ref.py).
// Specification: include/epn_so3conv.h (epn_icp_refine_f32) and DESIGN.md 3.1m.
// Every function of this file keeps its products and sums apart (no fma contraction) except transform_point, whose fma chain
// is explicit; fit_finish (rigid_fit.h) is compiled as it always was, which is why a transform is compared within a bound.
#pragma once
#include <cmath>

#include "rigid_fit.h"

#ifndef EPN_NO_CONTRACT
#if defined(__clang__)
#define EPN_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define EPN_NO_CONTRACT
#endif
#endif

namespace epn_icp {

constexpr int NS = 32;                   // int64 sums per row (both variants; the unused ones stay 0)
constexpr int REC = 20;                  // doubles per trace record: T[16], count, ssd, rmse, flags
constexpr int MAX_ITER = 1024;
constexpr long long MAX_M = 1 << 20;     // source points: a term is at most 2^18 * 2^24 + 1, and (2^42 + 1) * 2^20 < 2^63 (the header)
constexpr double LIN = 0x1p32;           // fixed point of the linear sums: units of 2^-32
constexpr double SQ = 0x1p24;            // fixed point of the product sums: units of 2^-24
constexpr double COORD_MAX = 64.0;       // |coordinate| of a matched pair; |component| <= 1 of its normal
constexpr double MARGIN_MIN = 1e-6;      // point-to-point: the Horn margin at or below it is "singular"
constexpr double PIVOT_MIN = 0x1p-20;    // point-to-plane: a pivot d_k <= PIVOT_MIN * A_kk is "singular"
constexpr int FLAG_CONVERGED = 1, FLAG_FEW = 2, FLAG_SINGULAR = 4, FLAG_RANGE = 8;
// where the sums sit in a row
constexpr int S_COUNT = 0, S_RANGE = 30;
constexpr int P2P_P = 1, P2P_Q = 4, P2P_PQ = 7, P2P_D2 = 16;
constexpr int PL_A = 1, PL_B = 22, PL_R2 = 28, PL_D2 = 29;

// q_i = (float)fma(T_i0, s_0, fma(T_i1, s_1, fma(T_i2, s_2, T_i3))): the chain of rigid_fit.h's sq_residual, rounded once to fp32
EPN_ROT_FN void transform_point(const double T[12], const float s[3], float q[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
        q[i] = (float)fma(T[4 * i], (double)s[0], fma(T[4 * i + 1], (double)s[1], fma(T[4 * i + 2], (double)s[2], T[4 * i + 3])));
}

// The nine values a matched pair's terms are products of, and whether the pair is out of range.  value_at picks one by a lane-dependent number.
struct Values {
    double v[9];
    bool bad;
};

EPN_ROT_FN double value_at(const Values &V, int i) {
    // a binary tree of selects on the bits of i (0 <= i <= 8): hipcc turns a CHAIN of `i == k` selects back into an indexed read
    // of the nine values, which then live in scratch or LDS; the tree keeps them in registers
    const bool b0 = (i & 1) != 0, b1 = (i & 2) != 0, b2 = (i & 4) != 0, b3 = (i & 8) != 0;
    const double x01 = b0 ? V.v[1] : V.v[0], x23 = b0 ? V.v[3] : V.v[2], x45 = b0 ? V.v[5] : V.v[4], x67 = b0 ? V.v[7] : V.v[6];
    const double y0 = b1 ? x23 : x01, y1 = b1 ? x67 : x45;
    const double z = b2 ? y1 : y0;
    const double x = b3 ? V.v[8] : z;
    return x;
}

// Point-to-point: V = {p0, p1, p2, q0, q1, q2, 1, dd, 0}, with d = q - p and dd = (d0 d0 + d1 d1) + d2 d2.  Out of range: a
// coordinate beyond COORD_MAX, NaN included.
EPN_ROT_FN Values p2p_values(const float p[3], const float q[3]) {
    EPN_NO_CONTRACT
    Values V;
    V.v[0] = (double)p[0]; V.v[1] = (double)p[1]; V.v[2] = (double)p[2];
    V.v[3] = (double)q[0]; V.v[4] = (double)q[1]; V.v[5] = (double)q[2];
    V.bad = !(fabs(V.v[0]) <= COORD_MAX) || !(fabs(V.v[1]) <= COORD_MAX) || !(fabs(V.v[2]) <= COORD_MAX) ||
            !(fabs(V.v[3]) <= COORD_MAX) || !(fabs(V.v[4]) <= COORD_MAX) || !(fabs(V.v[5]) <= COORD_MAX);
    const double d0 = V.v[3] - V.v[0], d1 = V.v[4] - V.v[1], d2 = V.v[5] - V.v[2];
    const double xx = d0 * d0, yy = d1 * d1, zz = d2 * d2;
    const double xy = xx + yy;
    V.v[6] = 1.0;
    V.v[7] = xy + zz;
    V.v[8] = 0.0;
    return V;
}

// Point-to-plane: V = {c0, c1, c2, n0, n1, n2, r, 1, dd} with c = q x n (c0 = q1 n2 - q2 n1, ...), r = (d0 n0 + d1 n1) + d2 n2, d
// and dd as above; J = the first six.  Out of range: as above, or a normal component beyond 1.
EPN_ROT_FN Values plane_values(const float p[3], const float q[3], const float n[3]) {
    EPN_NO_CONTRACT
    Values V;
    const double P0 = (double)p[0], P1 = (double)p[1], P2 = (double)p[2], Q0 = (double)q[0], Q1 = (double)q[1], Q2 = (double)q[2];
    const double N0 = (double)n[0], N1 = (double)n[1], N2 = (double)n[2];
    V.bad = !(fabs(P0) <= COORD_MAX) || !(fabs(P1) <= COORD_MAX) || !(fabs(P2) <= COORD_MAX) ||
            !(fabs(Q0) <= COORD_MAX) || !(fabs(Q1) <= COORD_MAX) || !(fabs(Q2) <= COORD_MAX) ||
            !(fabs(N0) <= 1.0) || !(fabs(N1) <= 1.0) || !(fabs(N2) <= 1.0);
    const double a0 = Q1 * N2, b0 = Q2 * N1, a1 = Q2 * N0, b1 = Q0 * N2, a2 = Q0 * N1, b2 = Q1 * N0;
    V.v[0] = a0 - b0;
    V.v[1] = a1 - b1;
    V.v[2] = a2 - b2;
    V.v[3] = N0; V.v[4] = N1; V.v[5] = N2;
    const double d0 = Q0 - P0, d1 = Q1 - P1, d2 = Q2 - P2;
    const double r0 = d0 * N0, r1 = d1 * N1, r2 = d2 * N2;
    const double r01 = r0 + r1;
    V.v[6] = r01 + r2;
    V.v[7] = 1.0;
    const double xx = d0 * d0, yy = d1 * d1, zz = d2 * d2;
    const double xy = xx + yy;
    V.v[8] = xy + zz;
    return V;
}

// Sum e of a row is the sum over the matched pairs of rint((value_at(V, ia) value_at(V, ib)) scale); scale = 0: the row has no sum e (S_RANGE, which
// counts the out-of-range pairs, is not a product).
EPN_ROT_FN void term_of(bool plane, int e, int &ia, int &ib, double &scale) {
    ia = 0; ib = 0; scale = 0.0;
    if (!plane) {
        if (e == S_COUNT) { ia = 6; ib = 6; scale = 1.0; }
        else if (e < P2P_PQ) { ia = e - P2P_P; ib = 6; scale = LIN; }                         // p0 p1 p2 q0 q1 q2
        else if (e < P2P_D2) { ia = (e - P2P_PQ) / 3; ib = 3 + (e - P2P_PQ) % 3; scale = SQ; }  // p_i q_j, row-major
        else if (e == P2P_D2) { ia = 7; ib = 6; scale = SQ; }
    } else {
        if (e == S_COUNT) { ia = 7; ib = 7; scale = 1.0; }
        else if (e < PL_B) {                                                                  // J_i J_j, i <= j, row-major
            int k = e - PL_A, i = 0;
            while (k >= 6 - i) { k -= 6 - i; ++i; }
            ia = i; ib = i + k; scale = SQ;
        }
        else if (e < PL_R2) { ia = e - PL_B; ib = 6; scale = SQ; }                            // J_i r
        else if (e == PL_R2) { ia = 6; ib = 6; scale = SQ; }
        else if (e == PL_D2) { ia = 8; ib = 7; scale = SQ; }
    }
}

// the product rounded once, then the exact scaling, then rint (ties to even): plane_fit.h's moments_add
EPN_ROT_FN long long term(double a, double b, double scale) {
    EPN_NO_CONTRACT
    const double prod = a * b;
    return llrint(prod * scale);
}

// Point-to-point: N = count, sp = S_p / 2^32, sq = S_q / 2^32, pbar = sp / N, qbar = sq / N, C_ij = S_pq,ij / 2^24 - (sp_i sq_j) / N;
// (R, t, margin) = fit_finish(pbar, qbar, C): the rotation and translation minimising sum |p - (R q + t)|^2.
EPN_ROT_FN int p2p_solve(const long long S[NS], double R[9], double t[3], double &margin) {
    EPN_NO_CONTRACT
    const double N = (double)S[S_COUNT];
    double sp[3], sq[3], pb[3], qb[3], C[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        sp[i] = (double)S[P2P_P + i] / LIN;
        sq[i] = (double)S[P2P_Q + i] / LIN;
        pb[i] = sp[i] / N;
        qb[i] = sq[i] / N;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double prod = sp[i] * sq[j];
            const double mean = prod / N;
            C[3 * i + j] = (double)S[P2P_PQ + 3 * i + j] / SQ - mean;
        }
    margin = 0.0;
    epn_fit::fit_finish(pb, qb, C, R, t, margin);
    return margin > MARGIN_MIN ? 0 : FLAG_SINGULAR;
}

// The Cayley map (I - [w]x / 2)^-1 (I + [w]x / 2) in closed form, with a = w / 2, aa = (a0 a0 + a1 a1) + a2 a2, k = 1 - aa,
// den = 1 + aa: R_ii = (k + w_i a_i) / den, R_ij = (w_i a_j -+ w_k) / den.  + - x / only; an exact rotation for every w.
EPN_ROT_FN void cayley(const double w[3], double R[9]) {
    EPN_NO_CONTRACT
    const double a0 = 0.5 * w[0], a1 = 0.5 * w[1], a2 = 0.5 * w[2];
    const double xx = a0 * a0, yy = a1 * a1, zz = a2 * a2;
    const double xy = xx + yy;
    const double aa = xy + zz;
    const double k = 1.0 - aa, den = 1.0 + aa;
    const double w00 = w[0] * a0, w01 = w[0] * a1, w02 = w[0] * a2, w10 = w[1] * a0, w11 = w[1] * a1, w12 = w[1] * a2;
    const double w20 = w[2] * a0, w21 = w[2] * a1, w22 = w[2] * a2;
    R[0] = (k + w00) / den;    R[1] = (w01 - w[2]) / den; R[2] = (w02 + w[1]) / den;
    R[3] = (w10 + w[2]) / den; R[4] = (k + w11) / den;    R[5] = (w12 - w[0]) / den;
    R[6] = (w20 - w[1]) / den; R[7] = (w21 + w[0]) / den; R[8] = (k + w22) / den;
}

// Point-to-plane: A = J^T J / 2^24 (symmetric from the 21 sums), b = J^T r / 2^24; A = L D L^T without pivoting, in ascending k:
// d_k = A_kk - sum_{j<k} (L_kj d_j) L_kj, L_ik = (A_ik - sum_{j<k} (L_ij d_j) L_kj) / d_k, the sums taken in ascending j from the
// left; singular when not d_k > PIVOT_MIN A_kk.  Then L y = -b, z = y / d, L^T x = z; w = x[0..3), t = x[3..6), R = cayley(w).
EPN_ROT_FN int plane_solve(const long long S[NS], double R[9], double t[3]) {
    EPN_NO_CONTRACT
    double A[6][6], L[6][6], d[6], y[6], x[6];
    {
        int e = PL_A;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j) {
                A[i][j] = A[j][i] = (double)S[e] / SQ;
                ++e;
            }
    }
    bool singular = false;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        double dk = A[k][k];
#pragma unroll
        for (int j = 0; j < k; ++j) {
            const double ld = L[k][j] * d[j];
            const double prod = ld * L[k][j];
            dk = dk - prod;
        }
        if (!(dk > PIVOT_MIN * A[k][k])) singular = true;
        d[k] = dk;
#pragma unroll
        for (int i = k + 1; i < 6; ++i) {
            double v = A[i][k];
#pragma unroll
            for (int j = 0; j < k; ++j) {
                const double ld = L[i][j] * d[j];
                const double prod = ld * L[k][j];
                v = v - prod;
            }
            L[i][k] = v / dk;
        }
    }
    if (singular) return FLAG_SINGULAR;
#pragma unroll
    for (int i = 0; i < 6; ++i) {                                      // L y = -b
        double v = -((double)S[PL_B + i] / SQ);
#pragma unroll
        for (int j = 0; j < i; ++j) {
            const double prod = L[i][j] * y[j];
            v = v - prod;
        }
        y[i] = v;
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {                                     // L^T x = y / d
        double v = y[i] / d[i];
#pragma unroll
        for (int j = i + 1; j < 6; ++j) {
            const double prod = L[j][i] * x[j];
            v = v - prod;
        }
        x[i] = v;
    }
    const double w[3] = {x[0], x[1], x[2]};
    cayley(w, R);
    t[0] = x[3]; t[1] = x[4]; t[2] = x[5];
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 6; ++i) finite = finite && std::isfinite(x[i]);
    return finite ? 0 : FLAG_SINGULAR;
}

// T <- dT T on the first three rows: R'_ij = (dR_i0 R_0j + dR_i1 R_1j) + dR_i2 R_2j, t'_i = ((dR_i0 t_0 + dR_i1 t_1) + dR_i2 t_2) + dt_i
EPN_ROT_FN void compose(const double dR[9], const double dt[3], double T[16]) {
    EPN_NO_CONTRACT
    double out[12];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double a = dR[3 * i] * T[j], b = dR[3 * i + 1] * T[4 + j], c = dR[3 * i + 2] * T[8 + j];
            const double ab = a + b;
            out[4 * i + j] = ab + c;
        }
        out[4 * i + 3] = out[4 * i + 3] + dt[i];
    }
#pragma unroll
    for (int e = 0; e < 12; ++e) T[e] = out[e];
}

// One iteration from its sums (m > 0 source points, iteration number iter >= 0): count, ssd = S_dd / 2^24, rmse = sqrt(ssd /
// count) (0 without a pair), fitness = count / m.  In this order: an out-of-range pair -> FLAG_RANGE; count < 3 (6 for
// point-to-plane) -> FLAG_FEW; iter > 0 and |fitness - prev_fitness| < rel_fitness and |rmse - prev_rmse| < rel_rmse ->
// FLAG_CONVERGED; the solve says singular -> FLAG_SINGULAR; otherwise T <- dT T.  With a flag T stays as it was.  prev_* take this
// iteration's values; rec = {T after the iteration, count, ssd, rmse, flags}; T's bottom row is written 0 0 0 1.  -> flags
EPN_ROT_FN int step(bool plane, const long long S[NS], long long m, int iter, double rel_fitness, double rel_rmse,
                    double &prev_fitness, double &prev_rmse, double T[16], double rec[REC]) {
    EPN_NO_CONTRACT
    const double N = (double)S[S_COUNT], ssd = (double)S[plane ? PL_D2 : P2P_D2] / SQ;
    const double rmse = S[S_COUNT] > 0 ? sqrt(ssd / N) : 0.0, fitness = N / (double)m;
    int flags = 0;
    if (S[S_RANGE] != 0) flags = FLAG_RANGE;
    else if (S[S_COUNT] < (plane ? 6 : 3)) flags = FLAG_FEW;
    else if (iter > 0 && fabs(fitness - prev_fitness) < rel_fitness && fabs(rmse - prev_rmse) < rel_rmse) flags = FLAG_CONVERGED;
    else {
        double dR[9], dt[3], margin;
        flags = plane ? plane_solve(S, dR, dt) : p2p_solve(S, dR, dt, margin);
        if (flags == 0) compose(dR, dt, T);
    }
    prev_fitness = fitness;
    prev_rmse = rmse;
    T[12] = 0.0; T[13] = 0.0; T[14] = 0.0; T[15] = 1.0;
#pragma unroll
    for (int e = 0; e < 16; ++e) rec[e] = T[e];
    rec[16] = N;
    rec[17] = ssd;
    rec[18] = rmse;
    rec[19] = (double)flags;
    return flags;
}

}  // namespace epn_icp
