// affine_core.hpp — device arithmetic of robust 2D affine estimation (docs/SPEC.md S26 2- and 3-samples, S27 minimal
// solves, S28 inlier test): the counterparts of cv::estimateAffine2D (6 DOF, FULL) and cv::estimateAffinePartial2D
// (4 DOF: rotation, uniform scale, translation; PARTIAL).  Built with -ffp-contract=off like every unit: the only fused
// multiply-adds are the explicit fma()/fmaf() calls, so tests/affine_ref.c (the CPU restatement) reproduces the bits.
// Models are 2 x 3 row-major, x2 ~ A [x1 y1 1]^T (OpenCV's layout); the kernels carry them as 9 doubles
// [a0 .. a5, 0, 0, 1], the third row of the equivalent homography.
#pragma once
#include "ransac_core.hpp"

namespace pm_affine {

using pm_ransac::f32x2;

enum { FULL = PM_AFFINE_FULL, PARTIAL = PM_AFFINE_PARTIAL };

// S26: sample size and sampler stream key of a model (the two 16-bit rotations of S6's constant S6, S13, S19 leave);
// the sample is S6's walk, sample_walk<MIN_PTS, STREAM> (sample_core.hpp)
template <int MODEL> struct Traits;
template <> struct Traits<FULL> {
    static constexpr int MIN_PTS = 3;
    static constexpr uint64_t STREAM = 0x79B97F4A7C159E37ULL;
};
template <> struct Traits<PARTIAL> {
    static constexpr int MIN_PTS = 2;
    static constexpr uint64_t STREAM = 0x7C159E3779B97F4AULL;
};

__device__ __forceinline__ bool finite6(const double (&A)[9])
{
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 6; ++i) ok = ok && fabs(A[i]) < __builtin_inf();     // NaN fails too
    return ok;
}

// S27 sample check of one image: no collinear triple (OpenCV's haveCollinearPoints [recalled]), NaN invalid.
__device__ __forceinline__ bool spread3(double det, double dx1, double dy1, double dx2, double dy2)
{
    const double FLT_EPS = 1.1920928955078125e-07;
    return fabs(det) > FLT_EPS * (((fabs(dx1) + fabs(dy1)) + fabs(dx2)) + fabs(dy2));
}

// SPEC S27, full: the affine map of 3 correspondences.  false = invalid sample (A is then 0).
__device__ __forceinline__ bool solve3(const double (&x1)[3], const double (&y1)[3], const double (&x2)[3],
                                       const double (&y2)[3], double (&A)[9])
{
#pragma unroll
    for (int i = 0; i < 9; ++i) A[i] = 0.0;
    const double dx1 = x1[1] - x1[0], dy1 = y1[1] - y1[0], dx2 = x1[2] - x1[0], dy2 = y1[2] - y1[0];
    const double e1 = x2[1] - x2[0], f1 = y2[1] - y2[0], e2 = x2[2] - x2[0], f2 = y2[2] - y2[0];
    const double det = dx1 * dy2 - dy1 * dx2;
    const double det2 = e1 * f2 - f1 * e2;
    if (!spread3(det, dx1, dy1, dx2, dy2) || !spread3(det2, e1, f1, e2, f2)) return false;
    const double idet = 1.0 / det;
    double a[9];
    a[0] = (e1 * dy2 - e2 * dy1) * idet;
    a[1] = (dx1 * e2 - dx2 * e1) * idet;
    a[2] = x2[0] - fma(a[0], x1[0], a[1] * y1[0]);
    a[3] = (f1 * dy2 - f2 * dy1) * idet;
    a[4] = (dx1 * f2 - dx2 * f1) * idet;
    a[5] = y2[0] - fma(a[3], x1[0], a[4] * y1[0]);
    a[6] = 0.0; a[7] = 0.0; a[8] = 1.0;
    if (!finite6(a)) return false;
#pragma unroll
    for (int i = 0; i < 9; ++i) A[i] = a[i];
    return true;
}

// SPEC S27, partial: the similarity [a, -b, tx; b, a, ty] of 2 correspondences.  false = invalid (A is then 0).
__device__ __forceinline__ bool solve2(const double (&x1)[2], const double (&y1)[2], const double (&x2)[2],
                                       const double (&y2)[2], double (&A)[9])
{
#pragma unroll
    for (int i = 0; i < 9; ++i) A[i] = 0.0;
    const double dx = x1[1] - x1[0], dy = y1[1] - y1[0], ex = x2[1] - x2[0], ey = y2[1] - y2[0];
    const double q = fma(dx, dx, dy * dy);
    if (!(q > 0.0) || !(q < __builtin_inf()) || !(fma(ex, ex, ey * ey) > 0.0)) return false;
    const double iq = 1.0 / q;
    const double a = fma(ex, dx, ey * dy) * iq;
    const double b = fma(ey, dx, -(ex * dy)) * iq;
    double m[9];
    m[0] = a; m[1] = -b; m[2] = x2[0] - fma(a, x1[0], -(b * y1[0]));
    m[3] = b; m[4] = a;  m[5] = y2[0] - fma(b, x1[0], a * y1[0]);
    m[6] = 0.0; m[7] = 0.0; m[8] = 1.0;
    if (!finite6(m)) return false;
#pragma unroll
    for (int i = 0; i < 9; ++i) A[i] = m[i];
    return true;
}

// S28 threshold: thr2 itself when 0 < thr2 < inf, else NaN (nothing is an inlier).  Uniform: computed once per kernel.
constexpr int CLASS_POS_FINITE = 0x180;
__device__ __forceinline__ float thr_or_nan(float thr2)
{
    return __builtin_amdgcn_classf(thr2, CLASS_POS_FINITE) ? thr2 : __builtin_nanf("");
}

// SPEC S28: fp32 forward residual test of one correspondence against a = A32 (a[6..8] unused).
__device__ __forceinline__ bool inlier_a32(const float (&a)[9], float x, float y, float xp, float yp, float thr2)
{
    const float u = fmaf(a[0], x, fmaf(a[1], y, a[2]));
    const float v = fmaf(a[3], x, fmaf(a[4], y, a[5]));
    const float du = u - xp, dv = v - yp;
    return fmaf(du, du, dv * dv) <= thr_or_nan(thr2);
}

// SPEC S28 on two correspondences: the packed-f32 form of inlier_a32 (IEEE per component, same bits).
__device__ __forceinline__ void inlier_a32_x2(const float (&a)[9], f32x2 x, f32x2 y, f32x2 xp, f32x2 yp, float thr2,
                                              bool& ia, bool& ib)
{
#define PM_SPLAT(v) f32x2{(v), (v)}
    const f32x2 u = __builtin_elementwise_fma(PM_SPLAT(a[0]), x, __builtin_elementwise_fma(PM_SPLAT(a[1]), y, PM_SPLAT(a[2])));
    const f32x2 v = __builtin_elementwise_fma(PM_SPLAT(a[3]), x, __builtin_elementwise_fma(PM_SPLAT(a[4]), y, PM_SPLAT(a[5])));
#undef PM_SPLAT
    const f32x2 du = u - xp, dv = v - yp;
    const f32x2 lhs = __builtin_elementwise_fma(du, du, dv * dv);
    const float t = thr_or_nan(thr2);
    ia = lhs[0] <= t;
    ib = lhs[1] <= t;
}

}  // namespace pm_affine
