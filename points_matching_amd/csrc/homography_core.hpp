// homography_core.hpp — device arithmetic of robust homography estimation (docs/SPEC.md S19 4-sample, S20 normalised
// 4-point DLT, S21 division-free reprojection test).  The counterpart of cv::findHomography(pts1, pts2, RANSAC, thr),
// the sibling of the cv::findFundamentalMat call at main.cpp:95-98.  Built with -ffp-contract=off like the RANSAC-F
// units: the only fused multiply-adds are the explicit fma()/fmaf() calls, so tests/homography_ref.c (the CPU
// restatement) reproduces the same bits.  The Hartley normalisation, the 9 x 8 Householder QR and the scale/sign step are
// S7's (ransac_core.hpp), shared with the 8-point solve.
#pragma once
#include "ransac_core.hpp"

namespace pm_homog {

using pm_ransac::f32x2;
using pm_ransac::hartley;
using pm_ransac::householder_null9x8;
using pm_ransac::householder_qr9x8;
using pm_ransac::scale_sign;

// SPEC S19: the 4-sample is S6's walk (sample_core.hpp, sample_walk<4, STREAM>) on a stream of its own, n >= 4
constexpr uint64_t STREAM = 0x4A7C159E3779B97FULL;

// S20: |cross| of a normalised triple at or below this is collinear (normalised points sit at mean distance sqrt(2)
// from their centroid, so the bound is ~3.5e-5 of a typical triangle's doubled area)
constexpr double COLLINEAR_EPS = 1e-4;

// SPEC S20 step 2: doubled signed area of the normalised triple (a, b, c), unfused.
__device__ __forceinline__ double cross3(const double (&x)[4], const double (&y)[4], int a, int b, int c)
{
    return (x[b] - x[a]) * (y[c] - y[a]) - (y[b] - y[a]) * (x[c] - x[a]);
}

// SPEC S20 step 2: no collinear triple in either image, one orientation relation for all four triples.
__device__ __forceinline__ bool sample_ok(const double (&ax)[4], const double (&ay)[4], const double (&bx)[4],
                                          const double (&by)[4])
{
    const int tri[4][3] = {{0, 1, 2}, {0, 1, 3}, {0, 2, 3}, {1, 2, 3}};
    bool same[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const double c1 = cross3(ax, ay, tri[t][0], tri[t][1], tri[t][2]);
        const double c2 = cross3(bx, by, tri[t][0], tri[t][1], tri[t][2]);
        if (!(fabs(c1) > COLLINEAR_EPS) || !(fabs(c2) > COLLINEAR_EPS)) return false;
        same[t] = (c1 > 0.0) == (c2 > 0.0);
    }
    return same[0] == same[1] && same[0] == same[2] && same[0] == same[3];
}

// SPEC S20 steps 5-6: H ~ (s2 T2^-1) Hn T1, where s2 T2^-1 = [[1, 0, -t2x], [0, 1, -t2y], [0, 0, s2]], then unit norm
// and sign.  false = invalid (H untouched).
__device__ __forceinline__ bool denormalise(const double (&hn)[9], double s1, double t1x, double t1y, double s2,
                                           double t2x, double t2y, double (&H)[9])
{
    double M[3][3], Ho[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        M[i][0] = hn[3 * i] * s1;
        M[i][1] = hn[3 * i + 1] * s1;
        M[i][2] = fma(hn[3 * i], t1x, fma(hn[3 * i + 1], t1y, hn[3 * i + 2]));
    }
    const double u2x = -t2x, u2y = -t2y;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        Ho[j] = fma(u2x, M[2][j], M[0][j]);
        Ho[3 + j] = fma(u2y, M[2][j], M[1][j]);
        Ho[6 + j] = s2 * M[2][j];
    }
    return scale_sign(Ho, H);
}

// SPEC S20: normalised 4-point DLT.  Returns false for an invalid sample (H is then 0).
__device__ __forceinline__ bool solve4(const double (&x1)[4], const double (&y1)[4], const double (&x2)[4],
                                       const double (&y2)[4], double (&H)[9])
{
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] = 0.0;
    double ax[4], ay[4], bx[4], by[4], s1, t1x, t1y, s2, t2x, t2y;
    if (!hartley(x1, y1, ax, ay, s1, t1x, t1y)) return false;
    if (!hartley(x2, y2, bx, by, s2, t2x, t2y)) return false;
    if (!sample_ok(ax, ay, bx, by)) return false;
    // B = A^T (9 x 8): columns 2c and 2c+1 are the two constraint rows of correspondence c
    double B[9][8];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int k = 2 * c, l = 2 * c + 1;
        B[0][k] = -ax[c];        B[1][k] = -ay[c];        B[2][k] = -1.0;
        B[3][k] = 0.0;           B[4][k] = 0.0;           B[5][k] = 0.0;
        B[6][k] = bx[c] * ax[c]; B[7][k] = bx[c] * ay[c]; B[8][k] = bx[c];
        B[0][l] = 0.0;           B[1][l] = 0.0;           B[2][l] = 0.0;
        B[3][l] = -ax[c];        B[4][l] = -ay[c];        B[5][l] = -1.0;
        B[6][l] = by[c] * ax[c]; B[7][l] = by[c] * ay[c]; B[8][l] = by[c];
    }
    double beta[8], hn[9];
    householder_qr9x8(B, beta);
    householder_null9x8(B, beta, hn);
    return denormalise(hn, s1, t1x, t1y, s2, t2x, t2y, H);
}

// SPEC S21: fp32 one-way reprojection test of one correspondence against h = H32.  Outliers: NaN, and a right side
// thr2 * w^2 that is 0 (w == 0) or +inf (a huge coordinate overflows both sides, and inf <= inf would hold).
// 0 < rhs < inf is one v_cmp_class (positive subnormal or normal), as cheap as the w != 0 it replaces.
constexpr int CLASS_POS_FINITE = 0x180;
__device__ __forceinline__ bool inlier_h32(const float (&h)[9], float x, float y, float xp, float yp, float thr2)
{
    const float u = fmaf(h[0], x, fmaf(h[1], y, h[2]));
    const float v = fmaf(h[3], x, fmaf(h[4], y, h[5]));
    const float w = fmaf(h[6], x, fmaf(h[7], y, h[8]));
    const float du = fmaf(-xp, w, u);
    const float dv = fmaf(-yp, w, v);
    const float rhs = thr2 * (w * w);
    return (fmaf(du, du, dv * dv) <= rhs) && __builtin_amdgcn_classf(rhs, CLASS_POS_FINITE);
}

// SPEC S21 on two correspondences: the packed-f32 form of inlier_h32 (IEEE per component, same bits).
__device__ __forceinline__ void inlier_h32_x2(const float (&h)[9], f32x2 x, f32x2 y, f32x2 xp, f32x2 yp, float thr2,
                                              bool& ia, bool& ib)
{
#define PM_SPLAT(v) f32x2{(v), (v)}
    const f32x2 u = __builtin_elementwise_fma(PM_SPLAT(h[0]), x, __builtin_elementwise_fma(PM_SPLAT(h[1]), y, PM_SPLAT(h[2])));
    const f32x2 v = __builtin_elementwise_fma(PM_SPLAT(h[3]), x, __builtin_elementwise_fma(PM_SPLAT(h[4]), y, PM_SPLAT(h[5])));
    const f32x2 w = __builtin_elementwise_fma(PM_SPLAT(h[6]), x, __builtin_elementwise_fma(PM_SPLAT(h[7]), y, PM_SPLAT(h[8])));
    const f32x2 rhs = PM_SPLAT(thr2) * (w * w);
#undef PM_SPLAT
    const f32x2 du = __builtin_elementwise_fma(-xp, w, u);
    const f32x2 dv = __builtin_elementwise_fma(-yp, w, v);
    const f32x2 lhs = __builtin_elementwise_fma(du, du, dv * dv);
    ia = (lhs[0] <= rhs[0]) && __builtin_amdgcn_classf(rhs[0], CLASS_POS_FINITE);
    ib = (lhs[1] <= rhs[1]) && __builtin_amdgcn_classf(rhs[1], CLASS_POS_FINITE);
}

}  // namespace pm_homog
