// lsm_solve.h — the K x K normal-equation solve of the Longstaff-Schwartz regressions: the ONE text behind k3_solve_t
// (k3_lsm.hip: one lane, all S right-hand sides) and k6_solve_state (k6_storage.hip: lane s, right-hand side s).  gfx950 only.
#pragma once

// Moments m[] of the shifted / scaled basis z = (x - shift) scale: m[q] = sum z^q for q < 2K-1, then m[(2K-1) + s K + k] =
// sum z^k Y_s.  Solves right-hand sides s0 .. s0+nr-1 into out[0 .. nr-1][K]: least-squares coefficients in the RAW monomial
// basis (back-transformation z^k = scale^k (x - shift)^k); all zero for an empty system (m[0] <= 0).  Same algorithm as the
// host solver (mcx/plan.py solve_normal_equations): LU with partial pivoting of the Gram matrix, and for `degenerate` the
// minimum-norm solution of the exactly rank-1 system of a date on which every path shares x = x0 (the calibration date).
// Returns 1 for a numerically singular system (out stays zero: the caller reports it and writes no coefficients), else 0.
// K <= KA, nr <= NA: with K and nr known where the call is inlined every loop unrolls and the system lives in registers (with
// run-time bounds the local arrays sit in scratch memory: ~11 us for a 3 x 3 solve by one thread, mostly scratch latency).
// Pivoting by conditional row swaps with static indices: after the r-loop row c holds the largest |entry| of column c, as with
// LAPACK's single swap; the remaining rows may be ordered differently, the solution is the same up to rounding.
template <int KA, int NA>
__device__ __forceinline__ int lsm_solve(const double* __restrict__ m, int K, int s0, int nr, double shift, double scale, double x0,
                                         int degenerate, double (&out)[NA][KA])
{
#pragma unroll
    for (int s = 0; s < nr; ++s)
#pragma unroll
        for (int k = 0; k < K; ++k) out[s][k] = 0.0;
    const double n = m[0];
    int st = 0;
    if (n > 0.0 && degenerate) {
        double v[KA], vv = 0.0, xp = 1.0;
#pragma unroll
        for (int k = 0; k < K; ++k) { v[k] = xp; vv += xp * xp; xp *= x0; }
#pragma unroll
        for (int s = 0; s < nr; ++s) {
            const double mean_y = m[(2 * K - 1) + (s0 + s) * K] / n;
#pragma unroll
            for (int k = 0; k < K; ++k) out[s][k] = v[k] * (mean_y / vv);
        }
    } else if (n > 0.0) {
        double G[KA][KA], B[KA][NA];
        double gmax = 0.0;
#pragma unroll
        for (int j = 0; j < K; ++j)
#pragma unroll
            for (int k = 0; k < K; ++k) { G[j][k] = m[j + k]; gmax = fmax(gmax, fabs(G[j][k])); }
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int s = 0; s < nr; ++s) B[k][s] = m[(2 * K - 1) + (s0 + s) * K + k];
#pragma unroll
        for (int c = 0; c < K; ++c) {                                  // LU, partial pivoting
#pragma unroll
            for (int r = c + 1; r < K; ++r) {
                const bool sw = fabs(G[r][c]) > fabs(G[c][c]);
#pragma unroll
                for (int k = 0; k < K; ++k) { const double x = G[c][k], y = G[r][k]; G[c][k] = sw ? y : x; G[r][k] = sw ? x : y; }
#pragma unroll
                for (int s = 0; s < nr; ++s) { const double x = B[c][s], y = B[r][s]; B[c][s] = sw ? y : x; B[r][s] = sw ? x : y; }
            }
            if (!(fabs(G[c][c]) > 1e-14 * gmax)) st = 1;               // numerically singular
            const double piv = st ? 1.0 : G[c][c];
#pragma unroll
            for (int r = c + 1; r < K; ++r) {
                const double f = G[r][c] / piv;
#pragma unroll
                for (int k = c + 1; k < K; ++k) G[r][k] -= f * G[c][k];
#pragma unroll
                for (int s = 0; s < nr; ++s) B[r][s] -= f * B[c][s];
            }
        }
        if (st == 0) {
#pragma unroll
            for (int c = K - 1; c >= 0; --c)
#pragma unroll
                for (int s = 0; s < nr; ++s) {
                    double acc = B[c][s];
#pragma unroll
                    for (int k = c + 1; k < K; ++k) acc -= G[c][k] * B[k][s];
                    B[c][s] = acc / G[c][c];
                }
            // T = coefficient of x^j in z^k = scale^k C(k, j) (-shift)^(k-j)
            double sp = 1.0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                double binom = 1.0;
#pragma unroll
                for (int j = 0; j <= k; ++j) {
                    double ms = 1.0;
                    for (int e = 0; e < k - j; ++e) ms *= -shift;
                    const double T = sp * binom * ms;
#pragma unroll
                    for (int s = 0; s < nr; ++s) out[s][j] += T * B[k][s];
                    binom = binom * (double)(k - j) / (double)(j + 1);
                }
                sp *= scale;
            }
        }
    }
    return st;
}
