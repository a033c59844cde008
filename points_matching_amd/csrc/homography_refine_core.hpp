// homography_refine_core.hpp — device arithmetic of the refinement of a robust homography on its inliers (docs/SPEC.md
// S23 least-squares DLT refit, S24 Levenberg-Marquardt on the forward transfer error, S25 result), the step
// cv::findHomography runs after its RANSAC loop: the per-correspondence terms of the passes and S23's 9 x 9 Jacobi on a
// wave (which fundamental_refine.hip uses too).  S24's damped Cholesky solve is lm_solve_n in lm_core.hpp.  Built with
// -ffp-contract=off like every unit: the only fused multiply-adds are the explicit fma() calls, so
// tests/homography_refine_ref.c (the CPU restatement) reproduces the bits.
#pragma once
#include <hip/hip_runtime.h>

namespace pm_hrefine {

constexpr int HR_NORMAL = 45;             // unique entries of the 9 x 9 normal matrix
constexpr int HR_LM = 45;                 // 36 of J^T J, 8 of J^T r, the cost
constexpr int HR_SWEEPS = 16;             // S23 Jacobi sweep cap
constexpr double HR_JACOBI_SKIP = 1e-17;  // S23: rotation (p, q) skipped unless |a_pq| > HR_JACOBI_SKIP * trace(M)
constexpr double HR_MIN_H8 = 1e-8;        // S24: LM needs |H[8]| >= this (H of unit norm)

// S24: squared forward transfer error of one correspondence under the 9 entries of h.
__device__ __forceinline__ double cost_term(const double (&h)[9], double x, double y, double xp, double yp)
{
    const double u = fma(h[0], x, fma(h[1], y, h[2]));
    const double v = fma(h[3], x, fma(h[4], y, h[5]));
    const double w = fma(h[6], x, fma(h[7], y, h[8]));
    const double iw = 1.0 / w;
    const double ru = u * iw - xp, rv = v * iw - yp;
    return fma(ru, ru, rv * rv);
}

// S23 pass 3: the two DLT rows of one normalised correspondence into the upper triangle of M (row-major, j <= k).
__device__ __forceinline__ void normal_term(double (&acc)[HR_NORMAL], double xn, double yn, double xq, double yq)
{
    const double a[9] = {-xn, -yn, -1.0, 0.0, 0.0, 0.0, xq * xn, xq * yn, xq};
    const double b[9] = {0.0, 0.0, 0.0, -xn, -yn, -1.0, yq * xn, yq * yn, yq};
    int e = 0;
#pragma unroll
    for (int j = 0; j < 9; ++j)
#pragma unroll
        for (int k = j; k < 9; ++k, ++e) acc[e] = acc[e] + fma(a[j], a[k], b[j] * b[k]);
}

// S24 pass: J^T J (upper triangle, row-major), J^T r and the cost of one correspondence at h (h[8] = 1).
__device__ __forceinline__ void lm_term(double (&acc)[HR_LM], const double (&h)[9], double x, double y, double xp,
                                        double yp)
{
    const double u = fma(h[0], x, fma(h[1], y, h[2]));
    const double v = fma(h[3], x, fma(h[4], y, h[5]));
    const double w = fma(h[6], x, fma(h[7], y, h[8]));
    const double iw = 1.0 / w;
    const double px = u * iw, py = v * iw;
    const double ru = px - xp, rv = py - yp;
    const double a = x * iw, b = y * iw, mpx = -px, mpy = -py;
    const double ju[8] = {a, b, iw, 0.0, 0.0, 0.0, mpx * a, mpx * b};
    const double jv[8] = {0.0, 0.0, 0.0, a, b, iw, mpy * a, mpy * b};
    int e = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int k = j; k < 8; ++k, ++e) acc[e] = acc[e] + fma(ju[j], ju[k], jv[j] * jv[k]);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[36 + j] = acc[36 + j] + fma(ju[j], ru, jv[j] * rv);
    acc[44] = acc[44] + fma(ru, ru, rv * rv);
}

// 64-bit value of lane l (l wave-uniform): two v_readlane.
__device__ __forceinline__ double readlane_d(double x, int l)
{
    const unsigned long long b = static_cast<unsigned long long>(__double_as_longlong(x));
    const unsigned lo = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(b & 0xFFFFFFFFu), l));
    const unsigned hi = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(b >> 32), l));
    return __longlong_as_double(static_cast<long long>((static_cast<unsigned long long>(hi) << 32) | lo));
}

// S23 step 3: eigenvector of the smallest eigenvalue of the symmetric 9 x 9 M (upper triangle m45) by cyclic Jacobi,
// run by ONE whole wave: lane k < 9 holds row k of A and row k of V, so the updates of a rotation's columns p and q are
// lane-local, and rows p and q are refilled from them by v_readlane (A stays exactly symmetric, as in the C
// restatement).  Every control value is read back through v_readlane, so it is wave-uniform.  hn: lane k < 9 returns
// component k.  false = invalid (trace not in (0, inf)).
__device__ __forceinline__ bool jacobi_min_wave(const double* m45, int lane, double& hn)
{
    double A[9], V[9];
    const int r = lane < 9 ? lane : 0;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const int a = r < j ? r : j, b = r < j ? j : r;
        const double m = m45[a * 9 - a * (a - 1) / 2 + (b - a)];
        A[j] = lane < 9 ? m : 0.0;
        V[j] = lane == j ? 1.0 : 0.0;
    }
    double tr = 0.0;
#pragma unroll
    for (int j = 0; j < 9; ++j) tr = tr + readlane_d(A[j], j);
    if (!(tr > 0.0) || !(tr < __builtin_inf())) return false;
    const double thr = HR_JACOBI_SKIP * tr;
    for (int sweep = 0; sweep < HR_SWEEPS; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 8; ++p) {
#pragma unroll
            for (int q = p + 1; q < 9; ++q) {
                const double apq = readlane_d(A[q], p);
                if (!(fabs(apq) > thr)) continue;
                rotated = true;
                const double app = readlane_d(A[p], p), aqq = readlane_d(A[q], q);
                const double theta = (aqq - app) / (2.0 * apq);
                double t = 1.0 / (fabs(theta) + sqrt(fma(theta, theta, 1.0)));
                if (theta < 0.0) t = -t;
                const double c = 1.0 / sqrt(fma(t, t, 1.0));
                const double s = t * c;
                // columns p and q of row `lane` (rows p and q themselves: the rotated diagonal and a zero)
                const double akp = A[p], akq = A[q];
                double np = fma(c, akp, -(s * akq)), nq = fma(s, akp, c * akq);
                if (lane == p) { np = fma(-t, apq, app); nq = 0.0; }
                if (lane == q) { np = 0.0; nq = fma(t, apq, aqq); }
                A[p] = np;
                A[q] = nq;
                // rows p and q: A[p][k] = A[k][p], A[q][k] = A[k][q] for k != p, q
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    if (k == p || k == q) continue;
                    const double vp = readlane_d(A[p], k), vq = readlane_d(A[q], k);
                    if (lane == p) A[k] = vp;
                    if (lane == q) A[k] = vq;
                }
                const double vkp = V[p], vkq = V[q];
                V[p] = fma(c, vkp, -(s * vkq));
                V[q] = fma(s, vkp, c * vkq);
            }
        }
        if (!rotated) break;
    }
    int mi = 0;
    double dmin = readlane_d(A[0], 0);
#pragma unroll
    for (int j = 1; j < 9; ++j) {
        const double dj = readlane_d(A[j], j);
        if (dj < dmin) { dmin = dj; mi = j; }
    }
    double vm = V[0];
#pragma unroll
    for (int j = 1; j < 9; ++j)
        if (mi == j) vm = V[j];
    hn = vm;
    return true;
}

}  // namespace pm_hrefine
