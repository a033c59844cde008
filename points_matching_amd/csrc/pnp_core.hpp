// pnp_core.hpp — device arithmetic of absolute camera pose (docs/SPEC.md S36 camera, S37 3-sample, S38 P3P solve, S39
// reprojection test): the counterpart of cv::solvePnPRansac for one pinhole camera without distortion.  Built with
// -ffp-contract=off like every unit: the only fused multiply-adds are the explicit fma() / fmaf() calls, so
// tests/pnp_ref.c (the CPU restatement) reproduces the bits.  The pose maps world to camera: x_cam = R X + t, R 3 x 3
// row-major; a candidate is 12 doubles (R, t).
#pragma once
#include "essential_core.hpp"

namespace pm_pnp {

using pm_essential::Cam;
using pm_essential::cross3;

constexpr uint64_t STREAM = 0x165667B19E3779F9ULL;   // S37: the 3-sample is S6's walk (sample_walk<3, STREAM>), n >= 3
constexpr int MAX_CAND = 4;           // S38: candidates per sample (model ids 4h .. 4h + 3)
constexpr int WORDS = 12;             // R (9), t (3)
constexpr int FLAG = 12;              // the valid flag (1.0 / 0.0) of a candidate slot
constexpr int M32 = 13;               // P32 = (float)(K [R|t]), 3 x 4 row-major, as 12 floats in doubles 13..18
constexpr int SLOT_DOUBLES = 20;      // a candidate slot of the solve launch: the above and one pad double

__device__ __forceinline__ double dot3(const double (&a)[3], const double (&b)[3])
{
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

// S38 step 1: pixel -> unit bearing; false if not finite
__device__ __forceinline__ bool bearing(const Cam& k, float u, float v, double (&f)[3])
{
    const double x = (static_cast<double>(u) - k.cx) / k.fx, y = (static_cast<double>(v) - k.cy) / k.fy;
    const double q = (x * x + y * y) + 1.0;
    const double inv = 1.0 / sqrt(q);
    f[0] = x * inv; f[1] = y * inv; f[2] = inv;
    return q < __builtin_inf();
}

// S38 step 5: orthonormal triad T = (e1, e2, n) of p0, p1, p2; false if a length is zero or not finite
__device__ __forceinline__ bool triad(const double (&p0)[3], const double (&p1)[3], const double (&p2)[3], double (&T)[3][3])
{
    double d1[3], d2[3], nn[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { d1[i] = p1[i] - p0[i]; d2[i] = p2[i] - p0[i]; }
    cross3(d1, d2, nn);
    const double l1 = dot3(d1, d1), ln = dot3(nn, nn);
    if (!(l1 > 0.0) || !(l1 < __builtin_inf()) || !(ln > 0.0) || !(ln < __builtin_inf())) return false;
    const double i1 = 1.0 / sqrt(l1), in = 1.0 / sqrt(ln);
#pragma unroll
    for (int i = 0; i < 3; ++i) { T[0][i] = d1[i] * i1; T[2][i] = nn[i] * in; }
    cross3(T[2], T[0], T[1]);
    return true;
}

// S39: P32 = (float)(K [R|t]), row-major 3 x 4
__device__ __forceinline__ void proj32(const Cam& k, const double* Rt, float* P)
{
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        P[c] = static_cast<float>(k.fx * Rt[c] + k.cx * Rt[6 + c]);
        P[4 + c] = static_cast<float>(k.fy * Rt[3 + c] + k.cy * Rt[6 + c]);
        P[8 + c] = static_cast<float>(Rt[6 + c]);
    }
    P[3] = static_cast<float>(k.fx * Rt[9] + k.cx * Rt[11]);
    P[7] = static_cast<float>(k.fy * Rt[10] + k.cy * Rt[11]);
    P[11] = static_cast<float>(Rt[11]);
}

// S38 on the 3 sampled world points X[i] and pixels (u[i], v[i]): candidate j (the j-th real root of the quartic,
// ascending) to out[SLOT_DOUBLES j ..]: R, t, valid flag, P32.  out holds MAX_CAND slots and is written in full.
__device__ __forceinline__ int p3p(const Cam& k, const float (&X)[3][3], const float (&u)[3], const float (&v)[3],
                                   double* __restrict__ out)
{
    for (int j = 0; j < SLOT_DOUBLES * MAX_CAND; ++j) out[j] = 0.0;
    double P[3][3], f[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) P[i][c] = static_cast<double>(X[i][c]);
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) ok = bearing(k, u[i], v[i], f[i]) && ok;
    double d1[3], d2[3], d12[3], nn[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { d1[i] = P[1][i] - P[0][i]; d2[i] = P[2][i] - P[0][i]; d12[i] = P[1][i] - P[2][i]; }
    cross3(d1, d2, nn);
    const double c2 = dot3(d1, d1), b2 = dot3(d2, d2), a2 = dot3(d12, d12), ln = dot3(nn, nn);
    if (!ok || !(ln > 1.4210854715202004e-14 * (c2 * b2)) || !(ln < __builtin_inf())) return 0;
    const double ca = dot3(f[1], f[2]), cb = dot3(f[0], f[2]), cg = dot3(f[0], f[1]);
    const double p = (a2 - c2) / b2, q = (a2 + c2) / b2, rc = c2 / b2, ra = a2 / b2;
    const double rbc = (b2 - c2) / b2, rba = (b2 - a2) / b2;
    double A[5];
    A[4] = (p - 1.0) * (p - 1.0) - 4.0 * rc * ca * ca;
    A[3] = 4.0 * ((p * (1.0 - p) * cb - (1.0 - q) * ca * cg) + 2.0 * rc * ca * ca * cb);
    A[2] = 2.0 * (((((p * p - 1.0) + 2.0 * p * p * cb * cb) + 2.0 * rbc * ca * ca) - 4.0 * q * ca * cb * cg) + 2.0 * rba * cg * cg);
    A[1] = 4.0 * ((-p * (1.0 + p) * cb + 2.0 * ra * cg * cg * cb) - (1.0 - q) * ca * cg);
    A[0] = (1.0 + p) * (1.0 + p) - 4.0 * ra * cg * cg;
    double TW[3][3];
    if (!triad(P[0], P[1], P[2], TW)) return 0;
    double roots[4];
    const int nr = pm_essential::real_roots<4>(A, roots);
    int nv = 0;
    for (int j = 0; j < nr; ++j) {
        const double r = roots[j];
        const double uu = (((p - 1.0) * r * r - 2.0 * p * cb * r) + (1.0 + p)) / (2.0 * (cg - r * ca));
        const double s0q = b2 / ((1.0 + r * r) - 2.0 * r * cb);
        if (!(s0q > 0.0) || !(s0q < __builtin_inf())) continue;
        const double s0 = sqrt(s0q), s1 = uu * s0, s2 = r * s0;
        if (!(s1 > 0.0) || !(s2 > 0.0) || !(s1 < __builtin_inf()) || !(s2 < __builtin_inf())) continue;
        double c[3][3], TC[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i) { c[0][i] = s0 * f[0][i]; c[1][i] = s1 * f[1][i]; c[2][i] = s2 * f[2][i]; }
        if (!triad(c[0], c[1], c[2], TC)) continue;
        double Rt[WORDS];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) Rt[3 * a + b] = (TC[0][a] * TW[0][b] + TC[1][a] * TW[1][b]) + TC[2][a] * TW[2][b];
#pragma unroll
        for (int a = 0; a < 3; ++a)
            Rt[9 + a] = c[0][a] - ((Rt[3 * a] * P[0][0] + Rt[3 * a + 1] * P[0][1]) + Rt[3 * a + 2] * P[0][2]);
        bool fin = true;
#pragma unroll
        for (int i = 0; i < WORDS; ++i) fin = fin && fabs(Rt[i]) < __builtin_inf();
        if (!fin) continue;
        double* o = out + SLOT_DOUBLES * j;
#pragma unroll
        for (int i = 0; i < WORDS; ++i) o[i] = Rt[i];
        o[FLAG] = 1.0;
        float P[WORDS];
        proj32(k, Rt, P);
        __builtin_memcpy(o + M32, P, sizeof P);               // 12 floats in doubles 13..18, no type punning
        ++nv;
    }
    return nv;
}

}  // namespace pm_pnp
