// lm_core.hpp — the leaves every on-device Levenberg-Marquardt refinement shares (homography, fundamental, relative pose,
// PnP, triangulation, bundle adjustment): docs/SPEC.md S24's damped Cholesky solve at N parameters, the packed
// J^T J / J^T r / cost sums of one residual row, S40 step 4's Cayley rotation step and pose update, and the two constants
// of S24.  Device code with no kernel and no LDS of its own: the LM loops stay in their kernels, which differ in
// what lives in LDS, where the step is applied and which thread does what.  Built with -ffp-contract=off like every unit:
// the only fused multiply-adds are the explicit fma() calls, and every operation order here is the one the spec fixes, so
// the CPU restatements (tests/*_ref.c) reproduce the bits.
#pragma once
#include <hip/hip_runtime.h>

#include "wave_ops.hpp"

namespace pm_hrefine {

constexpr double LM_LAMBDA0 = 1e-3;       // S24 initial damping (S40, S45, S47, S95, S115 start from it too)
constexpr double LM_STEP_TOL = 1e-15;     // S24: stop when max|d| <= LM_STEP_TOL * max(1, scale of the parameters)

// S24 step 4: (A + lam * diag(A)) d = -g by a Cholesky factor L L^T and two substitutions, in a fixed order.  H: the upper
// triangle of A = J^T J packed row-major (A[i][j], i >= j, is H[j*N - j*(j-1)/2 + (i - j)]); g = J^T r; d: N doubles.
// false = not positive definite.  The caller says at the call whether it is inlined.  A kernel in which one thread runs it
// between two passes, on sums in LDS, calls it [[clang::noinline]]: inlined into the LM loop of homography_refine it pushes
// the kernel past 256 VGPRs.  A lane that solves for its own point in registers (triangulate.hip) calls it
// [[clang::always_inline]].  It states the factor and the substitutions itself: built on lm_factor and lm_subst below it
// compiles to different code.
template <int N>
__device__ inline bool lm_solve_n(const double* H, const double* g, double lam, double* d)
{
    double L[N][N], y[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const double ajj = H[j * N - j * (j - 1) / 2];
        double dd = ajj + lam * ajj;
#pragma unroll
        for (int k = 0; k < j; ++k) dd = fma(-L[j][k], L[j][k], dd);
        if (!(dd > 0.0) || !(dd < __builtin_inf())) return false;
        L[j][j] = sqrt(dd);
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double v = H[j * N - j * (j - 1) / 2 + (i - j)];
#pragma unroll
            for (int k = 0; k < j; ++k) v = fma(-L[i][k], L[j][k], v);
            L[i][j] = v / L[j][j];
        }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double v = -g[i];
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

// The factor of lm_solve_n alone, L L^T = A + lam * diag(A), for a lane that substitutes against several right-hand sides
// (bundle adjustment's point blocks).  false = not positive definite.
template <int N>
__device__ __forceinline__ bool lm_factor(const double* H, double lam, double (&L)[N][N])
{
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const double ajj = H[j * N - j * (j - 1) / 2];
        double dd = ajj + lam * ajj;
#pragma unroll
        for (int k = 0; k < j; ++k) dd = fma(-L[j][k], L[j][k], dd);
        if (!(dd > 0.0) || !(dd < __builtin_inf())) return false;
        L[j][j] = sqrt(dd);
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double v = H[j * N - j * (j - 1) / 2 + (i - j)];
#pragma unroll
            for (int k = 0; k < j; ++k) v = fma(-L[i][k], L[j][k], v);
            L[i][j] = v / L[j][j];
        }
    }
    return true;
}

// The two substitutions of lm_solve_n alone: L L^T x = b
template <int N>
__device__ __forceinline__ void lm_subst(const double (&L)[N][N], const double* b, double* x)
{
    double y[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double v = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) v = fma(-L[i][k], y[k], v);
        y[i] = v / L[i][i];
    }
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
        double v = y[i];
#pragma unroll
        for (int k = i + 1; k < N; ++k) v = fma(-L[k][i], x[k], v);
        x[i] = v / L[i][i];
    }
}

// The LM sums of one residual row: N (N + 1) / 2 of J^T J (j <= k, row-major), N of J^T r, the cost
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

// The workgroup maximum of three values at once (the step test of bundle adjustment and of the pose graph: largest step,
// scale of the parameters, non-finite flag): a wave butterfly each, the NW wave maxima through s_max, one barrier.  Every
// thread of the NW waves calls it with its own three values and gets the three maxima; a NaN never wins.  (By value and a
// returned struct: with reference parameters the callers' `if (x > dmax) dmax = x` compile to branches.)
struct Max3 {
    double a, b, c;
};
template <int NW>
__device__ __forceinline__ Max3 group_max3(double (&s_max)[3][NW], int tid, double a, double b, double c)
{
    a = pm::wave_max_f64(a); b = pm::wave_max_f64(b); c = pm::wave_max_f64(c);
    if ((tid & 63) == 0) { s_max[0][tid >> 6] = a; s_max[1][tid >> 6] = b; s_max[2][tid >> 6] = c; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        a = s_max[0][w] > a ? s_max[0][w] : a;
        b = s_max[1][w] > b ? s_max[1][w] : b;
        c = s_max[2][w] > c ? s_max[2][w] : c;
    }
    return {a, b, c};
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

// out = C R, both row-major
__device__ __forceinline__ void left_rot(const double (&C)[9], const double* R, double* out)
{
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) out[3 * r + c] = (C[3 * r] * R[c] + C[3 * r + 1] * R[3 + c]) + C[3 * r + 2] * R[6 + c];
}

// S40 step 4 on a pose Rt = (R row-major, t): R' = C(d[0..2] / 2) R, t' = t + d[3..5]
__device__ __forceinline__ void pose_update(const double* Rt, const double* d, double* out)
{
    double C[9];
    cayley(d, C);
    left_rot(C, Rt, out);
#pragma unroll
    for (int i = 0; i < 3; ++i) out[9 + i] = Rt[9 + i] + d[3 + i];
}

}  // namespace pm_hrefine
