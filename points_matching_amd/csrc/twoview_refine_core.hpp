// twoview_refine_core.hpp — device arithmetic shared by the two refinements of a two-view model on its inliers: the
// fundamental matrix (fundamental_refine.hip, docs/SPEC.md S43-S45) and the calibrated relative pose (pose_refine.hip,
// S46-S47).  Both minimise the Sampson distance by Levenberg-Marquardt over a minimal parametrisation whose steps are
// Cayley rotations (S40 step 4), so this header holds the Sampson residual with its gradient in the 9 model entries, the
// chain rule of a left rotation, the LM sums and S24's damped Cholesky at N parameters.  Built with -ffp-contract=off
// like every unit: the only fused multiply-adds are the explicit fma() calls, so tests/twoview_refine_ref.c (the CPU
// restatement) reproduces the bits.
#pragma once
#include "homography_refine_core.hpp"

namespace pm_hrefine {

constexpr double TV_LAMBDA0 = 1e-3;       // S24's damping start
constexpr double TV_STEP_TOL = 1e-15;     // stop when max|d| <= this (every parameter is of unit scale)

__device__ __forceinline__ double dot3f(const double* a, const double* b) { return fma(a[0], b[0], fma(a[1], b[1], a[2] * b[2])); }

__device__ __forceinline__ void cross3u(const double* a, const double* b, double* o)
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// S45 step 3 / S47 step 1: the Sampson residual r = num * inv of the model m at x1 = (x1[0], x1[1], 1),
// x2 = (x2[0], x2[1], 1) with weights (w1, w2), and its gradient Gm in the 9 entries of m
__device__ __forceinline__ double sampson_grad(const double (&m)[9], const double (&x1)[3], const double (&x2)[3], double w1,
                                               double w2, double (&Gm)[9])
{
    const double a = fma(m[0], x1[0], fma(m[1], x1[1], m[2]));
    const double b = fma(m[3], x1[0], fma(m[4], x1[1], m[5]));
    const double c3 = fma(m[6], x1[0], fma(m[7], x1[1], m[8]));
    const double num = fma(x2[0], a, fma(x2[1], b, c3));
    const double c = fma(m[0], x2[0], fma(m[3], x2[1], m[6]));
    const double d = fma(m[1], x2[0], fma(m[4], x2[1], m[7]));
    const double den = fma(w2, fma(a, a, b * b), w1 * fma(c, c, d * d));
    const double inv = 1.0 / sqrt(den);
    const double r = num * inv;
    const double k = (r * inv) * inv;
    const double k2 = k * w2, k1 = k * w1;
    const double p[3] = {fma(-k2, a, inv * x2[0]), fma(-k2, b, inv * x2[1]), inv};
    const double q[3] = {k1 * c, k1 * d, 0.0};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Gm[3 * i + j] = fma(p[i], x1[j], -(x2[i] * q[j]));
    return r;
}

// The residual alone (the same operations, so the same bits as sampson_grad's)
__device__ __forceinline__ double sampson_res(const double (&m)[9], const double (&x1)[3], const double (&x2)[3], double w1,
                                              double w2)
{
    const double a = fma(m[0], x1[0], fma(m[1], x1[1], m[2]));
    const double b = fma(m[3], x1[0], fma(m[4], x1[1], m[5]));
    const double c3 = fma(m[6], x1[0], fma(m[7], x1[1], m[8]));
    const double num = fma(x2[0], a, fma(x2[1], b, c3));
    const double c = fma(m[0], x2[0], fma(m[3], x2[1], m[6]));
    const double d = fma(m[1], x2[0], fma(m[4], x2[1], m[7]));
    const double den = fma(w2, fma(a, a, b * b), w1 * fma(c, c, d * d));
    return num * (1.0 / sqrt(den));
}

// n_k = sum_ij G_ij ([e_k]x M)_ij: with N = G M^T, n = (N21 - N12, N02 - N20, N10 - N01).  TR: G and M are read
// transposed.
template <bool TR>
__device__ __forceinline__ void left_rot_grad(const double (&G)[9], const double (&M)[9], double (&n)[3])
{
    auto at = [](const double (&A)[9], int i, int j) { return TR ? A[3 * j + i] : A[3 * i + j]; };
    auto N = [&](int i, int l) { return fma(at(G, i, 0), at(M, l, 0), fma(at(G, i, 1), at(M, l, 1), at(G, i, 2) * at(M, l, 2))); };
    n[0] = N(2, 1) - N(1, 2);
    n[1] = N(0, 2) - N(2, 0);
    n[2] = N(1, 0) - N(0, 1);
}

// The LM sums of one inlier: N (N + 1) / 2 of J^T J (j <= k, row-major), N of J^T r, the cost
template <int N>
__device__ __forceinline__ void lm_sums(double (&acc)[N * (N + 1) / 2 + N + 1], const double (&J)[N], double r)
{
    int e = 0;
#pragma unroll
    for (int j = 0; j < N; ++j)
#pragma unroll
        for (int k = j; k < N; ++k, ++e) acc[e] = acc[e] + J[j] * J[k];
#pragma unroll
    for (int j = 0; j < N; ++j, ++e) acc[e] = acc[e] + J[j] * r;
    acc[e] = acc[e] + r * r;
}

// S24 step 4 at N parameters: (J^T J + lam * diag(J^T J)) d = -g by Cholesky in a fixed order.  jtjg: the packed upper
// triangle, then g (LDS); d: N doubles.  false = not positive definite.  Runs in one thread between two passes.
template <int N>
__device__ __attribute__((noinline)) bool lm_solve_n(const double* jtjg, double lam, double* d)
{
    double L[N][N], y[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const double ajj = jtjg[j * N - j * (j - 1) / 2];
        double dd = ajj + lam * ajj;
#pragma unroll
        for (int k = 0; k < j; ++k) dd = fma(-L[j][k], L[j][k], dd);
        if (!(dd > 0.0) || !(dd < __builtin_inf())) return false;
        L[j][j] = sqrt(dd);
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double v = jtjg[j * N - j * (j - 1) / 2 + (i - j)];
#pragma unroll
            for (int k = 0; k < j; ++k) v = fma(-L[i][k], L[j][k], v);
            L[i][j] = v / L[j][j];
        }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double v = -jtjg[N * (N + 1) / 2 + i];
#pragma unroll
        for (int k = 0; k < i; ++k) v = fma(-L[i][k], y[k], v);
        y[i] = v / L[i][i];
    }
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        double v = y[i];
#pragma unroll
        for (int k = i + 1; k < N; ++k) v = fma(-L[k][i], d[k], v);
        d[i] = v / L[i][i];
    }
    return true;
}

// max |d_i|; a NaN propagates
template <int N>
__device__ __forceinline__ double step_max(const double* d)
{
    double dmax = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i)
        if (!(fabs(d[i]) <= dmax)) dmax = fabs(d[i]);
    return dmax;
}

// S40 step 4: C = Cayley(d / 2)
__device__ __forceinline__ void cayley(const double* d, double (&C)[9])
{
    const double h0 = 0.5 * d[0], h1 = 0.5 * d[1], h2 = 0.5 * d[2];
    const double cc = (h0 * h0 + h1 * h1) + h2 * h2;
    const double s = 1.0 / (1.0 + cc), m = 1.0 - cc;
    C[0] = (m + 2.0 * (h0 * h0)) * s; C[1] = (2.0 * (h0 * h1 - h2)) * s; C[2] = (2.0 * (h0 * h2 + h1)) * s;
    C[3] = (2.0 * (h0 * h1 + h2)) * s; C[4] = (m + 2.0 * (h1 * h1)) * s; C[5] = (2.0 * (h1 * h2 - h0)) * s;
    C[6] = (2.0 * (h0 * h2 - h1)) * s; C[7] = (2.0 * (h1 * h2 + h0)) * s; C[8] = (m + 2.0 * (h2 * h2)) * s;
}

__device__ __forceinline__ void rot3(const double (&C)[9], const double* v, double* o)
{
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = (C[3 * r] * v[0] + C[3 * r + 1] * v[1]) + C[3 * r + 2] * v[2];
}

}  // namespace pm_hrefine
