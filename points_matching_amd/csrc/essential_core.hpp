// essential_core.hpp — device arithmetic of calibrated relative pose (docs/SPEC.md S31 camera normalisation, S32
// 5-sample, S33 5-point solve, S35 decomposition, triangulation and cheirality): the counterparts of
// cv::findEssentialMat and cv::recoverPose for one camera shared by both views.  Built with -ffp-contract=off like every
// unit: the only fused multiply-adds are the explicit fma() calls, so tests/essential_ref.c (the CPU restatement)
// reproduces the bits.  E is 3 x 3 row-major with x2n^T E x1n = 0 on normalised coordinates.
//
// The solver is lane-serial fp64.  Its 10 x 20 elimination matrix (400 doubles) and the root lists are indexed at run
// time (pivot rows, root counts) and live in scratch; everything else is unrolled over compile-time indices.
#pragma once
#include "ransac_core.hpp"

namespace pm_essential {

constexpr uint64_t STREAM = 0xC2B2AE3D27D4EB4FULL;   // S32: the 5-sample is S6's walk (sample_walk<5, STREAM>), n >= 5
constexpr int MAX_MODELS = 10;        // S33: candidates per sample (model ids 10h .. 10h + 9)
constexpr int BISECT_STEPS = 64;      // S33 root bisection
constexpr int SWEEPS_E = 6;           // S35 Jacobi sweeps on E
constexpr int SWEEPS_T = 8;           // S35 Jacobi sweeps on the 4 x 4 triangulation system

// One camera shared by both views (pm_camera, by value: kernel argument)
struct Cam {
    double fx, fy, cx, cy;
};

// S31: pixel -> normalised, f64 arithmetic rounded to f32; NaN unless |value| <= 2^20 (a NaN, an infinity or a
// coordinate no pinhole image holds: S8's squares of the rest stay finite, so inf <= inf never makes such a row an inlier)
constexpr float NORM_MAX = 1048576.0f;
__device__ __forceinline__ float normalise1(float p, double c, double f)
{
    const float v = static_cast<float>((static_cast<double>(p) - c) / f);
    return fabsf(v) <= NORM_MAX ? v : __builtin_nanf("");
}
__device__ __forceinline__ float2 normalise(const Cam& k, float2 p)
{
    return float2{normalise1(p.x, k.cx, k.fx), normalise1(p.y, k.cy, k.fy)};
}

// S33 polynomial products in (x, y, z): linear [x y z 1] x linear -> quadratic (10 monomials
// x^2 xy xz x y^2 yz y z^2 z 1), quadratic x linear -> cubic (20 monomials in Nister's order
// x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1)
__device__ __forceinline__ void mul11(const double (&a)[4], const double (&b)[4], double (&o)[10])
{
    constexpr int Q2[4][4] = {{0, 1, 2, 3}, {1, 4, 5, 6}, {2, 5, 7, 8}, {3, 6, 8, 9}};
#pragma unroll
    for (int k = 0; k < 10; ++k) o[k] = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) o[Q2[i][j]] = fma(a[i], b[j], o[Q2[i][j]]);
}

__device__ __forceinline__ void mul21(const double (&a)[10], const double (&b)[4], double (&o)[20])
{
    constexpr int C3[10][4] = {{0, 2, 4, 5},   {2, 3, 8, 9},   {4, 8, 10, 11},   {5, 9, 11, 12},   {3, 1, 6, 7},
                               {8, 6, 13, 14}, {9, 7, 14, 15}, {10, 13, 16, 17}, {11, 14, 17, 18}, {12, 15, 18, 19}};
#pragma unroll
    for (int k = 0; k < 20; ++k) o[k] = 0.0;
#pragma unroll
    for (int q = 0; q < 10; ++q)
#pragma unroll
        for (int l = 0; l < 4; ++l) o[C3[q][l]] = fma(a[q], b[l], o[C3[q][l]]);
}

// S33: the 10 x 20 constraint matrix of E = x X + y Y + z Z + W: row 0 det E, rows 1 + 3i + j (M E)_ij with
// M = E E^T - (tr(E E^T) / 2) I
__device__ __forceinline__ void constraints(const double (&N)[4][9], double (&A)[10][20])
{
    double L[9][4], t0[10], t1[10], m[3][10], c[20], c2[20];
#pragma unroll
    for (int k = 0; k < 9; ++k) { L[k][0] = N[0][k]; L[k][1] = N[1][k]; L[k][2] = N[2][k]; L[k][3] = N[3][k]; }
    mul11(L[4], L[8], t0); mul11(L[5], L[7], t1);
#pragma unroll
    for (int q = 0; q < 10; ++q) m[0][q] = t0[q] - t1[q];
    mul11(L[3], L[8], t0); mul11(L[5], L[6], t1);
#pragma unroll
    for (int q = 0; q < 10; ++q) m[1][q] = t0[q] - t1[q];
    mul11(L[3], L[7], t0); mul11(L[4], L[6], t1);
#pragma unroll
    for (int q = 0; q < 10; ++q) m[2][q] = t0[q] - t1[q];
    mul21(m[0], L[0], c); mul21(m[1], L[1], c2);
#pragma unroll
    for (int k = 0; k < 20; ++k) c[k] = c[k] - c2[k];
    mul21(m[2], L[2], c2);
#pragma unroll
    for (int k = 0; k < 20; ++k) A[0][k] = c[k] + c2[k];
    double EE[3][3][10], tr[10];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) {
            mul11(L[3 * i], L[3 * j], EE[i][j]);
#pragma unroll
            for (int k = 1; k < 3; ++k) {
                mul11(L[3 * i + k], L[3 * j + k], t0);
#pragma unroll
                for (int q = 0; q < 10; ++q) EE[i][j][q] = EE[i][j][q] + t0[q];
            }
            if (j != i)
#pragma unroll
                for (int q = 0; q < 10; ++q) EE[j][i][q] = EE[i][j][q];
        }
#pragma unroll
    for (int q = 0; q < 10; ++q) tr[q] = (EE[0][0][q] + EE[1][1][q]) + EE[2][2][q];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int q = 0; q < 10; ++q) EE[i][i][q] = EE[i][i][q] - 0.5 * tr[q];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double r[20];
            mul21(EE[i][0], L[j], r);
#pragma unroll
            for (int k = 1; k < 3; ++k) {
                mul21(EE[i][k], L[3 * k + j], c);
#pragma unroll
                for (int q = 0; q < 20; ++q) r[q] = r[q] + c[q];
            }
#pragma unroll
            for (int q = 0; q < 20; ++q) A[1 + 3 * i + j][q] = r[q];
        }
}

// S33: Gauss-Jordan on the first 10 columns; pivot = first row of the strict maximum |A_rj| over r >= j.  false =
// singular (or not finite).
__device__ __forceinline__ bool gauss_jordan(double (&A)[10][20])
{
    for (int j = 0; j < 10; ++j) {
        int p = j;
        double pm = fabs(A[j][j]);
        for (int r = j + 1; r < 10; ++r)
            if (fabs(A[r][j]) > pm) { p = r; pm = fabs(A[r][j]); }
        if (!(pm > 0.0) || !(pm < __builtin_inf())) return false;
        if (p != j)
            for (int c = j; c < 20; ++c) { const double t = A[j][c]; A[j][c] = A[p][c]; A[p][c] = t; }
        const double inv = 1.0 / A[j][j];
        for (int c = j + 1; c < 20; ++c) A[j][c] = A[j][c] * inv;
        A[j][j] = 1.0;
        for (int r = 0; r < 10; ++r) {
            if (r == j) continue;
            const double f = A[r][j];
            for (int c = j + 1; c < 20; ++c) A[r][c] = fma(-f, A[j][c], A[r][c]);
            A[r][j] = 0.0;
        }
    }
    return true;
}

template <int NA, int NB>
__device__ __forceinline__ void polymul(const double (&a)[NA], const double (&b)[NB], double (&o)[NA + NB - 1])
{
#pragma unroll
    for (int k = 0; k < NA + NB - 1; ++k) o[k] = 0.0;
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) o[i + j] = fma(a[i], b[j], o[i + j]);
}

// S33: B(z) from the reduced rows (4, 5), (6, 7), (8, 9): per row the x and y coefficients (degree 3) and the constant
// (degree 4), ascending in z
struct Bz {
    double x[3][4], y[3][4], c[3][5];
};

__device__ __forceinline__ void make_bz(const double (&A)[10][20], Bz& B)
{
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double* a = A[4 + 2 * r];
        const double* b = A[5 + 2 * r];
        B.x[r][0] = a[12]; B.x[r][1] = a[11] - b[12]; B.x[r][2] = a[10] - b[11]; B.x[r][3] = -b[10];
        B.y[r][0] = a[15]; B.y[r][1] = a[14] - b[15]; B.y[r][2] = a[13] - b[14]; B.y[r][3] = -b[13];
        B.c[r][0] = a[19]; B.c[r][1] = a[18] - b[19]; B.c[r][2] = a[17] - b[18]; B.c[r][3] = a[16] - b[17];
        B.c[r][4] = -b[16];
    }
}

// S33: det B(z), degree 10, ascending
__device__ __forceinline__ void detpoly(const Bz& B, double (&p)[11])
{
    double s[8], u[8], c0[8], c1[8], s6[7], u6[7], c2[7], w[11], v[11];
    double bx1[4], by1[4], bc1[5], bx2[4], by2[4], bc2[5], bx0[4], by0[4], bc0[5];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        bx0[k] = B.x[0][k]; by0[k] = B.y[0][k]; bx1[k] = B.x[1][k]; by1[k] = B.y[1][k]; bx2[k] = B.x[2][k]; by2[k] = B.y[2][k];
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) { bc0[k] = B.c[0][k]; bc1[k] = B.c[1][k]; bc2[k] = B.c[2][k]; }
    polymul(by1, bc2, s); polymul(bc1, by2, u);
#pragma unroll
    for (int k = 0; k < 8; ++k) c0[k] = s[k] - u[k];
    polymul(bx1, bc2, s); polymul(bc1, bx2, u);
#pragma unroll
    for (int k = 0; k < 8; ++k) c1[k] = s[k] - u[k];
    polymul(bx1, by2, s6); polymul(by1, bx2, u6);
#pragma unroll
    for (int k = 0; k < 7; ++k) c2[k] = s6[k] - u6[k];
    polymul(bx0, c0, w); polymul(by0, c1, v);
#pragma unroll
    for (int k = 0; k < 11; ++k) p[k] = w[k] - v[k];
    polymul(bc0, c2, w);
#pragma unroll
    for (int k = 0; k < 11; ++k) p[k] = p[k] + w[k];
}

// S33 step 6: real roots of the degree-DEG p (ascending coefficients), ascending, by bracketing with the roots of its
// successive (monic) derivatives and BISECT_STEPS bisection steps per sign change.  Returns their number.  DEG = 10:
// the 5-point solve; DEG = 4: the P3P quartic (pnp_core.hpp, S38).
template <int DEG>
__device__ __forceinline__ int real_roots(const double (&p)[DEG + 1], double (&roots)[DEG])
{
    const double c10 = p[DEG];
    if (!(fabs(c10) > 0.0) || !(fabs(c10) < __builtin_inf())) return 0;
    double D[DEG + 1][DEG];
    double mx = 0.0;
    bool fin = true;
#pragma unroll
    for (int k = 0; k < DEG; ++k) {
        D[DEG][k] = p[k] / c10;
        fin = fin && fabs(D[DEG][k]) < __builtin_inf();
        if (fabs(D[DEG][k]) > mx) mx = fabs(D[DEG][k]);
    }
    if (!fin) return 0;
    const double R = 1.0 + mx;
#pragma unroll
    for (int d = DEG; d >= 2; --d)
#pragma unroll
        for (int k = 0; k < d - 1; ++k) D[d - 1][k] = D[d][k + 1] * (static_cast<double>(k + 1) / static_cast<double>(d));
    double r[DEG], e[DEG + 2];
    int m = 1;
    r[0] = -D[1][0];
#pragma unroll
    for (int d = 2; d <= DEG; ++d) {
        e[0] = -R;
        for (int i = 0; i < m; ++i) e[i + 1] = r[i] < -R ? -R : (r[i] > R ? R : r[i]);
        e[m + 1] = R;
        int nm = 0;
        for (int i = 0; i <= m; ++i) {
            double lo = e[i], hi = e[i + 1];
            double vlo = 1.0, vhi = 1.0;
#pragma unroll
            for (int k = d - 1; k >= 0; --k) { vlo = fma(vlo, lo, D[d][k]); vhi = fma(vhi, hi, D[d][k]); }
            const bool slo = vlo < 0.0;
            if (slo == (vhi < 0.0)) continue;
            for (int s = 0; s < BISECT_STEPS; ++s) {
                const double mid = 0.5 * (lo + hi);
                double v = 1.0;
#pragma unroll
                for (int k = d - 1; k >= 0; --k) v = fma(v, mid, D[d][k]);
                if ((v < 0.0) == slo) lo = mid; else hi = mid;
            }
            r[nm++] = 0.5 * (lo + hi);
        }
        m = nm;
    }
    for (int i = 0; i < m; ++i) roots[i] = r[i];
    return m;
}

template <int DEG>
__device__ __forceinline__ double horner(const double (&c)[DEG + 1], double z)
{
    double v = c[DEG];
#pragma unroll
    for (int k = DEG - 1; k >= 0; --k) v = fma(v, z, c[k]);
    return v;
}

__device__ __forceinline__ void cross3(const double (&a)[3], const double (&b)[3], double (&o)[3])
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// S33 on 5 normalised correspondences (f64): candidate j (the j-th real root, ascending) goes to out[10j .. 10j + 8],
// its valid flag (1.0 / 0.0) to out[10j + 9]; out holds MAX_MODELS slots and is written in full.  Returns the number of
// valid candidates.
__device__ __forceinline__ int solve5(const double (&x1)[5], const double (&y1)[5], const double (&x2)[5],
                                      const double (&y2)[5], double* __restrict__ out)
{
    for (int j = 0; j < 10 * MAX_MODELS; ++j) out[j] = 0.0;
    double B[9][5], beta[5];
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        B[0][c] = x2[c] * x1[c]; B[1][c] = x2[c] * y1[c]; B[2][c] = x2[c];
        B[3][c] = y2[c] * x1[c]; B[4][c] = y2[c] * y1[c]; B[5][c] = y2[c];
        B[6][c] = x1[c];         B[7][c] = y1[c];         B[8][c] = 1.0;
    }
    bool rank = true;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        double sigma = 0.0;
#pragma unroll
        for (int i = j + 1; i < 9; ++i) sigma = fma(B[i][j], B[i][j], sigma);
        const double alpha = B[j][j];
        const double nrm = sqrt(fma(alpha, alpha, sigma));
        rank = rank && nrm > 0.0;
        const double v0 = alpha + (alpha >= 0.0 ? nrm : -nrm);
        beta[j] = 2.0 / fma(v0, v0, sigma);
        B[j][j] = v0;
#pragma unroll
        for (int c = j + 1; c < 5; ++c) {
            double dot = v0 * B[j][c];
#pragma unroll
            for (int i = j + 1; i < 9; ++i) dot = fma(B[i][j], B[i][c], dot);
            const double w = beta[j] * dot;
            B[j][c] = fma(-w, v0, B[j][c]);
#pragma unroll
            for (int i = j + 1; i < 9; ++i) B[i][c] = fma(-w, B[i][j], B[i][c]);
        }
    }
    if (!rank) return 0;                    // (a rank-deficient column only spoils values that are then discarded)
    double N[4][9];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
#pragma unroll
        for (int i = 0; i < 9; ++i) N[b][i] = i == 5 + b ? 1.0 : 0.0;
#pragma unroll
        for (int j = 4; j >= 0; --j) {
            double dot = B[j][j] * N[b][j];
#pragma unroll
            for (int i = j + 1; i < 9; ++i) dot = fma(B[i][j], N[b][i], dot);
            const double w = beta[j] * dot;
            N[b][j] = fma(-w, B[j][j], N[b][j]);
#pragma unroll
            for (int i = j + 1; i < 9; ++i) N[b][i] = fma(-w, B[i][j], N[b][i]);
        }
    }
    double A[10][20];
    constraints(N, A);
    if (!gauss_jordan(A)) return 0;
    Bz Bm;
    make_bz(A, Bm);
    double p[11], roots[10];
    detpoly(Bm, p);
    const int nr = real_roots<10>(p, roots);
    int nv = 0;
    for (int j = 0; j < nr; ++j) {
        const double z = roots[j];
        double rw[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            rw[r][0] = horner<3>(Bm.x[r], z);
            rw[r][1] = horner<3>(Bm.y[r], z);
            rw[r][2] = horner<4>(Bm.c[r], z);
        }
        double cr[3][3];
        cross3(rw[0], rw[1], cr[0]);
        cross3(rw[1], rw[2], cr[1]);
        cross3(rw[0], rw[2], cr[2]);
        double c0 = cr[0][0], c1 = cr[0][1], c2 = cr[0][2];
#pragma unroll
        for (int k = 1; k < 3; ++k)
            if (fabs(cr[k][2]) > fabs(c2)) { c0 = cr[k][0]; c1 = cr[k][1]; c2 = cr[k][2]; }
        if (!(fabs(c2) > 0.0)) continue;
        const double x = c0 / c2, y = c1 / c2;
        double e[9], ss = 0.0;
#pragma unroll
        for (int i = 0; i < 9; ++i) e[i] = fma(x, N[0][i], fma(y, N[1][i], fma(z, N[2][i], N[3][i])));
#pragma unroll
        for (int i = 0; i < 9; ++i) ss = fma(e[i], e[i], ss);
        const double nrm = sqrt(ss);
        if (!(nrm > 0.0) || !(nrm < __builtin_inf())) continue;
        double ek = e[0];
#pragma unroll
        for (int i = 1; i < 9; ++i)
            if (fabs(e[i]) > fabs(ek)) ek = e[i];
        double inv = 1.0 / nrm;
        if (ek < 0.0) inv = -inv;
#pragma unroll
        for (int i = 0; i < 9; ++i) out[10 * j + i] = e[i] * inv;
        out[10 * j + 9] = 1.0;
        ++nv;
    }
    return nv;
}

// ---- S35 -------------------------------------------------------------------------------------------------------------
// One Jacobi (Hestenes) rotation of columns P, Q of the ROWS x NC matrix G and of V (NC x NC): S7 step 4's formulas.
template <int ROWS, int NC, int P, int Q>
__device__ __forceinline__ void jacobi_cols(double (&G)[ROWS][NC], double (&V)[NC][NC])
{
    double al = G[0][P] * G[0][P], be = G[0][Q] * G[0][Q], ga = G[0][P] * G[0][Q];
#pragma unroll
    for (int i = 1; i < ROWS; ++i) {
        al = fma(G[i][P], G[i][P], al);
        be = fma(G[i][Q], G[i][Q], be);
        ga = fma(G[i][P], G[i][Q], ga);
    }
    if (!(ga * ga > 4.930380657631324e-32 * (al * be))) return;
    const double zeta = (be - al) / (2.0 * ga);
    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(fma(zeta, zeta, 1.0)));
    const double c = 1.0 / sqrt(fma(t, t, 1.0));
    const double s = c * t;
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
        const double gp = G[i][P], gq = G[i][Q];
        G[i][P] = fma(c, gp, -(s * gq));
        G[i][Q] = fma(s, gp, c * gq);
    }
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const double vp = V[i][P], vq = V[i][Q];
        V[i][P] = fma(c, vp, -(s * vq));
        V[i][Q] = fma(s, vp, c * vq);
    }
}

template <int ROWS, int NC>
__device__ __forceinline__ double colnorm2(const double (&G)[ROWS][NC], int p)
{
    double a = 0.0;
#pragma unroll
    for (int q = 0; q < NC; ++q)
        if (q == p) {
            a = G[0][q] * G[0][q];
#pragma unroll
            for (int i = 1; i < ROWS; ++i) a = fma(G[i][q], G[i][q], a);
        }
    return a;
}

// The four pose candidates of an E: R1, R2 (row-major) and t, in the order (R1,t) (R2,t) (R1,-t) (R2,-t)
struct Poses {
    double R1[9], R2[9], t[3];
};

// S35: E -> R1, R2, t.  false = E not finite or of rank < 2.
__device__ __forceinline__ bool decompose(const double (&E)[9], Poses& ps)
{
    double G[3][3], V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    bool fin = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) { fin = fin && fabs(E[i]) < __builtin_inf(); G[i / 3][i % 3] = E[i]; }
    if (!fin) return false;
    for (int s = 0; s < SWEEPS_E; ++s) {
        jacobi_cols<3, 3, 0, 1>(G, V);
        jacobi_cols<3, 3, 0, 2>(G, V);
        jacobi_cols<3, 3, 1, 2>(G, V);
    }
    double cn[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) cn[p] = colnorm2<3, 3>(G, p);
    int m = 0;
    if (cn[1] < cn[m]) m = 1;
    if (cn[2] < cn[m]) m = 2;
    const int a = m == 0 ? 1 : 0, b = m == 2 ? 1 : 2;
    const int o0 = cn[b] > cn[a] ? b : a, o1 = cn[b] > cn[a] ? a : b;
    if (!(cn[o1] > 0.0)) return false;
    double u[3][3], v[3][3];
    const double s0 = 1.0 / sqrt(cn[o0]), s1 = 1.0 / sqrt(cn[o1]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        u[0][i] = G[i][o0] * s0;
        u[1][i] = G[i][o1] * s1;
        v[0][i] = V[i][o0]; v[1][i] = V[i][o1]; v[2][i] = V[i][m];
    }
    cross3(u[0], u[1], u[2]);
    double vc[3];
    cross3(v[1], v[2], vc);
    const double dv = fma(v[0][0], vc[0], fma(v[0][1], vc[1], v[0][2] * vc[2]));
    if (dv < 0.0)
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int i = 0; i < 3; ++i) v[k][i] = -v[k][i];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            ps.R1[3 * r + c] = fma(u[2][r], v[2][c], fma(u[0][r], v[1][c], -(u[1][r] * v[0][c])));
            ps.R2[3 * r + c] = fma(u[2][r], v[2][c], fma(u[1][r], v[0][c], -(u[0][r] * v[1][c])));
        }
    const double tn = sqrt(fma(u[2][0], u[2][0], fma(u[2][1], u[2][1], u[2][2] * u[2][2])));
    if (!(tn > 0.0) || !(tn < __builtin_inf())) return false;
    const double it = 1.0 / tn;
#pragma unroll
    for (int i = 0; i < 3; ++i) ps.t[i] = u[2][i] * it;
    return true;
}

// S35 step 2 on ROWS DLT rows (S94: two per view): one-sided Jacobi on the 4 columns of A with V = I, SWEEPS_T sweeps,
// Q = the column of V at the first strict minimum column norm.  A row of zeros changes no bit of any sum.
template <int ROWS>
__device__ __forceinline__ void dlt_null_vector(double (&A)[ROWS][4], double (&Q)[4])
{
    double V[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) V[r][c] = r == c ? 1.0 : 0.0;
    for (int s = 0; s < SWEEPS_T; ++s) {
        jacobi_cols<ROWS, 4, 0, 1>(A, V);
        jacobi_cols<ROWS, 4, 0, 2>(A, V);
        jacobi_cols<ROWS, 4, 0, 3>(A, V);
        jacobi_cols<ROWS, 4, 1, 2>(A, V);
        jacobi_cols<ROWS, 4, 1, 3>(A, V);
        jacobi_cols<ROWS, 4, 2, 3>(A, V);
    }
    double cm = colnorm2<ROWS, 4>(A, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) Q[i] = V[i][0];
#pragma unroll
    for (int p = 1; p < 4; ++p) {
        const double c = colnorm2<ROWS, 4>(A, p);
        if (c < cm) {
            cm = c;
#pragma unroll
            for (int i = 0; i < 4; ++i) Q[i] = V[i][p];
        }
    }
}

// S35: linear DLT of one correspondence against [I|0] and [R|t] (t = sg * ps.t): homogeneous Q
__device__ __forceinline__ void triangulate(const double (&R)[9], const double (&t)[3], double x1, double y1, double x2,
                                            double y2, double (&Q)[4])
{
    double A[4][4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const double p0 = c < 3 ? R[c] : t[0], p1 = c < 3 ? R[3 + c] : t[1], p2 = c < 3 ? R[6 + c] : t[2];
        A[0][c] = c == 0 ? -1.0 : (c == 2 ? x1 : 0.0);
        A[1][c] = c == 1 ? -1.0 : (c == 2 ? y1 : 0.0);
        A[2][c] = x2 * p2 - p0;
        A[3][c] = y2 * p2 - p1;
    }
    dlt_null_vector<4>(A, Q);
}

// S35: OpenCV's cheirality tests of Q for [R|t]
__device__ __forceinline__ bool cheiral(const double (&R)[9], const double (&t)[3], const double (&Q)[4], double dist)
{
    bool ok = Q[2] * Q[3] > 0.0;
    const double X = Q[0] / Q[3], Y = Q[1] / Q[3], Z = Q[2] / Q[3];
    ok = ok && Z < dist;
    const double z2 = fma(R[6], X, fma(R[7], Y, fma(R[8], Z, t[2])));
    return ok && z2 > 0.0 && z2 < dist;
}

}  // namespace pm_essential
