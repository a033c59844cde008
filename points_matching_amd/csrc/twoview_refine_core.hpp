// twoview_refine_core.hpp — device arithmetic shared by the two refinements of a two-view model on its inliers: the
// fundamental matrix (fundamental_refine.hip, docs/SPEC.md S43-S45) and the calibrated relative pose (pose_refine.hip,
// S46-S47).  Both minimise the Sampson distance by Levenberg-Marquardt over a minimal parametrisation whose steps are
// Cayley rotations (S40 step 4).  This header holds what is two-view: the Sampson residual with its gradient in the 9
// model entries and the chain rule of a left rotation; the LM sums, S24's damped Cholesky at N parameters and the Cayley
// step are in lm_core.hpp.  Built with -ffp-contract=off like every unit: the only fused multiply-adds are the explicit
// fma() calls, so tests/twoview_refine_ref.c (the CPU restatement) reproduces the bits.
#pragma once
#include "lm_core.hpp"

namespace pm_hrefine {

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

}  // namespace pm_hrefine
