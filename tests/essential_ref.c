/* essential_ref.c — plain-C restatement of docs/SPEC.md S31-S35 (calibrated relative pose: camera normalisation, the
 * 5-sample, the 5-point solve, RANSAC-E scoring and pose recovery), test infrastructure only.  tests/essential_ref.py
 * builds it with `cc -O2 -ffp-contract=off -shared -fPIC` and loads it with ctypes; tests/test_essential_gpu.py compares
 * the HIP kernels with it bit for bit.  Every fused multiply-add is an explicit fma()/fmaf() call, exactly where the
 * SPEC names one.  K: {fx, fy, cx, cy}.  E: 9 doubles row-major, x2n^T E x1n = 0. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define NB 64          /* S33 bisection steps */
#define NSWEEP_E 6     /* S35 Jacobi sweeps of E */
#define NSWEEP_T 8     /* S35 Jacobi sweeps of the 4 x 4 triangulation system */

static uint64_t mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

/* ---- S31 */
int er_k_valid(const double K[4], float thr_px, float* thr_n)
{
    for (int i = 0; i < 4; ++i)
        if (!(fabs(K[i]) < INFINITY)) return 0;
    if (!(K[0] > 0.0) || !(K[1] > 0.0)) return 0;
    const float t = (float)((double)thr_px / (0.5 * (K[0] + K[1])));
    if (!(t > 0.0f) || !(t < INFINITY)) return 0;
    *thr_n = t;
    return 1;
}

static float er_norm1(float p, double c, double f)
{
    const float v = (float)(((double)p - c) / f);
    return fabsf(v) <= 1048576.0f ? v : NAN;                 /* NaN, an infinity, beyond 2^20: NaN */
}

void er_normalise(const double K[4], const float* xy, int n, float* out)
{
    for (int i = 0; i < n; ++i) {
        out[2 * i] = er_norm1(xy[2 * i], K[2], K[0]);
        out[2 * i + 1] = er_norm1(xy[2 * i + 1], K[3], K[1]);
    }
}

/* ---- S32 */
void er_sample(uint64_t seed, uint64_t h, int n, int* idx)
{
    const uint64_t stream = mix64(seed ^ 0xC2B2AE3D27D4EB4FULL) ^ mix64(h + 0xD1B54A32D192ED03ULL);
    int cnt = 0;
    for (uint64_t d = 0; d < 64 && cnt < 5; ++d) {
        const uint64_t r = mix64(stream + (d + 1) * 0x9E3779B97F4A7C15ULL);
        const int c = (int)(((r >> 32) * (uint64_t)(uint32_t)n) >> 32);
        int rep = 0;
        for (int s = 0; s < cnt; ++s) rep |= idx[s] == c;
        if (!rep) idx[cnt++] = c;
    }
    for (int c = 0; cnt < 5; ++c) {
        int rep = 0;
        for (int s = 0; s < cnt; ++s) rep |= idx[s] == c;
        if (!rep) idx[cnt++] = c;
    }
}

/* ---- S33 */
/* quadratic monomial of the linear variables (i, j) of (x, y, z, 1); cubic monomial of quadratic q times variable l */
static const int Q2[4][4] = {{0, 1, 2, 3}, {1, 4, 5, 6}, {2, 5, 7, 8}, {3, 6, 8, 9}};
static const int C3[10][4] = {{0, 2, 4, 5},   {2, 3, 8, 9},    {4, 8, 10, 11},  {5, 9, 11, 12},  {3, 1, 6, 7},
                              {8, 6, 13, 14}, {9, 7, 14, 15}, {10, 13, 16, 17}, {11, 14, 17, 18}, {12, 15, 18, 19}};

static void mul11(const double a[4], const double b[4], double o[10])
{
    for (int k = 0; k < 10; ++k) o[k] = 0.0;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) o[Q2[i][j]] = fma(a[i], b[j], o[Q2[i][j]]);
}

static void mul21(const double a[10], const double b[4], double o[20])
{
    for (int k = 0; k < 20; ++k) o[k] = 0.0;
    for (int q = 0; q < 10; ++q)
        for (int l = 0; l < 4; ++l) o[C3[q][l]] = fma(a[q], b[l], o[C3[q][l]]);
}

/* the 10 x 20 constraint matrix of E = x X + y Y + z Z + W (rows: det E, then (M E)_ij row-major) */
void er_constraints(const double X[9], const double Y[9], const double Z[9], const double W[9], double A[10][20])
{
    double L[9][4], t0[10], t1[10], m[3][10], c[20], c2[20];
    for (int k = 0; k < 9; ++k) { L[k][0] = X[k]; L[k][1] = Y[k]; L[k][2] = Z[k]; L[k][3] = W[k]; }
    mul11(L[4], L[8], t0); mul11(L[5], L[7], t1);
    for (int q = 0; q < 10; ++q) m[0][q] = t0[q] - t1[q];
    mul11(L[3], L[8], t0); mul11(L[5], L[6], t1);
    for (int q = 0; q < 10; ++q) m[1][q] = t0[q] - t1[q];
    mul11(L[3], L[7], t0); mul11(L[4], L[6], t1);
    for (int q = 0; q < 10; ++q) m[2][q] = t0[q] - t1[q];
    mul21(m[0], L[0], c); mul21(m[1], L[1], c2);
    for (int k = 0; k < 20; ++k) c[k] = c[k] - c2[k];
    mul21(m[2], L[2], c2);
    for (int k = 0; k < 20; ++k) A[0][k] = c[k] + c2[k];
    double EE[3][3][10], tr[10], M[3][3][10];
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) {
            mul11(L[3 * i], L[3 * j], EE[i][j]);
            for (int k = 1; k < 3; ++k) {
                mul11(L[3 * i + k], L[3 * j + k], t0);
                for (int q = 0; q < 10; ++q) EE[i][j][q] = EE[i][j][q] + t0[q];
            }
            if (j != i) memcpy(EE[j][i], EE[i][j], sizeof(t0));
        }
    for (int q = 0; q < 10; ++q) tr[q] = (EE[0][0][q] + EE[1][1][q]) + EE[2][2][q];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            for (int q = 0; q < 10; ++q) M[i][j][q] = i == j ? EE[i][j][q] - 0.5 * tr[q] : EE[i][j][q];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double* r = A[1 + 3 * i + j];
            mul21(M[i][0], L[j], r);
            for (int k = 1; k < 3; ++k) {
                mul21(M[i][k], L[3 * k + j], c);
                for (int q = 0; q < 20; ++q) r[q] = r[q] + c[q];
            }
        }
}

/* Gauss-Jordan on the first 10 columns: pivot = first row of the strict maximum |A_rj|, r >= j.  0 = singular. */
int er_gauss_jordan(double A[10][20])
{
    for (int j = 0; j < 10; ++j) {
        int p = j;
        double pm = fabs(A[j][j]);
        for (int r = j + 1; r < 10; ++r)
            if (fabs(A[r][j]) > pm) { p = r; pm = fabs(A[r][j]); }
        if (!(pm > 0.0) || !(pm < INFINITY)) return 0;
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
    return 1;
}

static void polymul(const double* a, int na, const double* b, int nb, double* o)
{
    for (int k = 0; k < na + nb - 1; ++k) o[k] = 0.0;
    for (int i = 0; i < na; ++i)
        for (int j = 0; j < nb; ++j) o[i + j] = fma(a[i], b[j], o[i + j]);
}

/* the 3 x 3 polynomial matrix B(z) (rows k, l, m; columns x, y, 1; coefficients ascending in z, degrees 3, 3, 4) of
 * the reduced rows (4, 5), (6, 7), (8, 9) */
void er_bz(const double A[10][20], double B[3][3][5])
{
    for (int r = 0; r < 3; ++r) {
        const double* a = A[4 + 2 * r];
        const double* b = A[5 + 2 * r];
        for (int v = 0; v < 2; ++v) {
            const int c = 10 + 3 * v;
            B[r][v][0] = a[c + 2];
            B[r][v][1] = a[c + 1] - b[c + 2];
            B[r][v][2] = a[c] - b[c + 1];
            B[r][v][3] = -b[c];
            B[r][v][4] = 0.0;
        }
        B[r][2][0] = a[19];
        B[r][2][1] = a[18] - b[19];
        B[r][2][2] = a[17] - b[18];
        B[r][2][3] = a[16] - b[17];
        B[r][2][4] = -b[16];
    }
}

/* det B(z): degree 10, coefficients ascending */
void er_detpoly(const double B[3][3][5], double p[11])
{
    double s[8], u[8], c0[8], c1[8], c2[7], w[11], v[11];
    polymul(B[1][1], 4, B[2][2], 5, s); polymul(B[1][2], 5, B[2][1], 4, u);
    for (int k = 0; k < 8; ++k) c0[k] = s[k] - u[k];
    polymul(B[1][0], 4, B[2][2], 5, s); polymul(B[1][2], 5, B[2][0], 4, u);
    for (int k = 0; k < 8; ++k) c1[k] = s[k] - u[k];
    polymul(B[1][0], 4, B[2][1], 4, s); polymul(B[1][1], 4, B[2][0], 4, u);
    for (int k = 0; k < 7; ++k) c2[k] = s[k] - u[k];
    polymul(B[0][0], 4, c0, 8, w); polymul(B[0][1], 4, c1, 8, v);
    for (int k = 0; k < 11; ++k) p[k] = w[k] - v[k];
    polymul(B[0][2], 5, c2, 7, w);
    for (int k = 0; k < 11; ++k) p[k] = p[k] + w[k];
}

/* real roots of p (degree 10), ascending; returns their number (0 when the leading coefficient is 0 / not finite) */
int er_roots(const double p[11], double* roots)
{
    const double c10 = p[10];
    if (!(fabs(c10) > 0.0) || !(fabs(c10) < INFINITY)) return 0;
    double D[11][10];               /* D[d][k]: monic q_d = z^d + sum_{k<d} D[d][k] z^k */
    double mx = 0.0;
    for (int k = 0; k < 10; ++k) {
        D[10][k] = p[k] / c10;
        if (!(fabs(D[10][k]) < INFINITY)) return 0;
        if (fabs(D[10][k]) > mx) mx = fabs(D[10][k]);
    }
    const double R = 1.0 + mx;
    for (int d = 10; d >= 2; --d)
        for (int k = 0; k < d - 1; ++k) D[d - 1][k] = D[d][k + 1] * ((double)(k + 1) / (double)d);
    double r[10], e[12];
    int m = 1;
    r[0] = -D[1][0];
    for (int d = 2; d <= 10; ++d) {
        e[0] = -R;
        for (int i = 0; i < m; ++i) e[i + 1] = r[i] < -R ? -R : (r[i] > R ? R : r[i]);
        e[m + 1] = R;
        int nm = 0;
        for (int i = 0; i <= m; ++i) {
            double lo = e[i], hi = e[i + 1];
            double vlo = 1.0, vhi = 1.0;
            for (int k = d - 1; k >= 0; --k) { vlo = fma(vlo, lo, D[d][k]); vhi = fma(vhi, hi, D[d][k]); }
            const int slo = vlo < 0.0;
            if (slo == (vhi < 0.0)) continue;
            for (int s = 0; s < NB; ++s) {
                const double mid = 0.5 * (lo + hi);
                double v = 1.0;
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

static double horner(const double* c, int deg, double z)
{
    double v = c[deg];
    for (int k = deg - 1; k >= 0; --k) v = fma(v, z, c[k]);
    return v;
}

static void cross3(const double a[3], const double b[3], double o[3])
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

/* S33 on 5 correspondences (normalised, f64): candidates E[10][9] and flags valid[10] (slot j = j-th root ascending).
 * Returns the number of valid candidates; stage (may be NULL) receives how far the solve got: 0 QR rank, 1 GJ,
 * 2 leading coefficient, 3 roots found. */
int er_solve5(const double* x1, const double* y1, const double* x2, const double* y2, double* E, int* valid, int* stage)
{
    for (int i = 0; i < 90; ++i) E[i] = 0.0;
    for (int j = 0; j < 10; ++j) valid[j] = 0;
    if (stage) *stage = 0;
    double B[9][5], beta[5];
    for (int c = 0; c < 5; ++c) {
        B[0][c] = x2[c] * x1[c]; B[1][c] = x2[c] * y1[c]; B[2][c] = x2[c];
        B[3][c] = y2[c] * x1[c]; B[4][c] = y2[c] * y1[c]; B[5][c] = y2[c];
        B[6][c] = x1[c];         B[7][c] = y1[c];         B[8][c] = 1.0;
    }
    for (int j = 0; j < 5; ++j) {
        double sigma = 0.0;
        for (int i = j + 1; i < 9; ++i) sigma = fma(B[i][j], B[i][j], sigma);
        const double alpha = B[j][j];
        const double nrm = sqrt(fma(alpha, alpha, sigma));
        if (!(nrm > 0.0)) return 0;
        const double v0 = alpha + (alpha >= 0.0 ? nrm : -nrm);
        beta[j] = 2.0 / fma(v0, v0, sigma);
        B[j][j] = v0;
        for (int c = j + 1; c < 5; ++c) {
            double dot = v0 * B[j][c];
            for (int i = j + 1; i < 9; ++i) dot = fma(B[i][j], B[i][c], dot);
            const double w = beta[j] * dot;
            B[j][c] = fma(-w, v0, B[j][c]);
            for (int i = j + 1; i < 9; ++i) B[i][c] = fma(-w, B[i][j], B[i][c]);
        }
    }
    double N[4][9];
    for (int b = 0; b < 4; ++b) {
        double* f = N[b];
        for (int i = 0; i < 9; ++i) f[i] = i == 5 + b ? 1.0 : 0.0;
        for (int j = 4; j >= 0; --j) {
            double dot = B[j][j] * f[j];
            for (int i = j + 1; i < 9; ++i) dot = fma(B[i][j], f[i], dot);
            const double w = beta[j] * dot;
            f[j] = fma(-w, B[j][j], f[j]);
            for (int i = j + 1; i < 9; ++i) f[i] = fma(-w, B[i][j], f[i]);
        }
    }
    double A[10][20];
    er_constraints(N[0], N[1], N[2], N[3], A);
    if (stage) *stage = 1;
    if (!er_gauss_jordan(A)) return 0;
    if (stage) *stage = 2;
    double Bz[3][3][5], p[11], roots[10];
    er_bz(A, Bz);
    er_detpoly(Bz, p);
    const int nr = er_roots(p, roots);
    if (stage) *stage = nr > 0 || (fabs(p[10]) > 0.0 && fabs(p[10]) < INFINITY) ? 3 : 2;
    int nv = 0;
    for (int j = 0; j < nr; ++j) {
        const double z = roots[j];
        double rw[3][3];
        for (int r = 0; r < 3; ++r) {
            rw[r][0] = horner(Bz[r][0], 3, z);
            rw[r][1] = horner(Bz[r][1], 3, z);
            rw[r][2] = horner(Bz[r][2], 4, z);
        }
        double cr[3][3];
        cross3(rw[0], rw[1], cr[0]);
        cross3(rw[1], rw[2], cr[1]);
        cross3(rw[0], rw[2], cr[2]);
        int b = 0;
        for (int k = 1; k < 3; ++k)
            if (fabs(cr[k][2]) > fabs(cr[b][2])) b = k;
        if (!(fabs(cr[b][2]) > 0.0)) continue;
        const double x = cr[b][0] / cr[b][2], y = cr[b][1] / cr[b][2];
        double e[9], ss = 0.0;
        for (int i = 0; i < 9; ++i) e[i] = fma(x, N[0][i], fma(y, N[1][i], fma(z, N[2][i], N[3][i])));
        for (int i = 0; i < 9; ++i) ss = fma(e[i], e[i], ss);
        const double nrm = sqrt(ss);
        if (!(nrm > 0.0) || !(nrm < INFINITY)) continue;
        int kb = 0;
        for (int i = 1; i < 9; ++i)
            if (fabs(e[i]) > fabs(e[kb])) kb = i;
        double inv = 1.0 / nrm;
        if (e[kb] < 0.0) inv = -inv;
        for (int i = 0; i < 9; ++i) E[9 * j + i] = e[i] * inv;
        valid[j] = 1;
        ++nv;
    }
    return nv;
}

/* S32 + S33 for sample h of n normalised correspondences (f32, interleaved) */
int er_candidates(const float* xy1n, const float* xy2n, int n, uint64_t seed, uint64_t h, double* E, int* valid)
{
    int idx[5];
    double x1[5], y1[5], x2[5], y2[5];
    for (int i = 0; i < 90; ++i) E[i] = 0.0;
    for (int j = 0; j < 10; ++j) valid[j] = 0;
    if (n < 5) return 0;
    er_sample(seed, h, n, idx);
    for (int i = 0; i < 5; ++i) {
        x1[i] = (double)xy1n[2 * idx[i]]; y1[i] = (double)xy1n[2 * idx[i] + 1];
        x2[i] = (double)xy2n[2 * idx[i]]; y2[i] = (double)xy2n[2 * idx[i] + 1];
    }
    return er_solve5(x1, y1, x2, y2, E, valid, 0);
}

/* ---- S34: S8 SAMPSON on normalised f32 coordinates */
int er_inlier(const float f[9], float x, float y, float xp, float yp, float thr2)
{
    const float a = fmaf(f[0], x, fmaf(f[1], y, f[2]));
    const float b = fmaf(f[3], x, fmaf(f[4], y, f[5]));
    const float c = fmaf(f[6], x, fmaf(f[7], y, f[8]));
    const float num = fmaf(xp, a, fmaf(yp, b, c));
    const float at = fmaf(f[0], xp, fmaf(f[3], yp, f[6]));
    const float bt = fmaf(f[1], xp, fmaf(f[4], yp, f[7]));
    const float n2 = num * num;
    const float den = fmaf(a, a, fmaf(b, b, fmaf(at, at, bt * bt)));
    return n2 <= thr2 * den;
}

int er_score(const double E[9], const float* xy1n, const float* xy2n, int n, float thr2, uint8_t* mask)
{
    float f[9];
    for (int i = 0; i < 9; ++i) f[i] = (float)E[i];
    int c = 0;
    for (int i = 0; i < n; ++i) {
        const int in = er_inlier(f, xy1n[2 * i], xy1n[2 * i + 1], xy2n[2 * i], xy2n[2 * i + 1], thr2);
        if (mask) mask[i] = (uint8_t)in;
        c += in;
    }
    return c;
}

/* Whole RANSAC-E over samples [hb, he) on pixel coordinates.  Returns the key (0: no model); E, mask, n_inliers set
 * (zero without a model).  xyn: 4 n floats of scratch. */
uint64_t er_run(const float* xy1, const float* xy2, int n, const double K[4], uint64_t seed, int64_t hb, int64_t he,
                float thr_px, float* xyn, double E[9], uint8_t* mask, int* n_inliers)
{
    float tn;
    for (int i = 0; i < 9; ++i) E[i] = 0.0;
    if (mask && n > 0) memset(mask, 0, (size_t)n);
    *n_inliers = 0;
    if (!er_k_valid(K, thr_px, &tn) || n < 5) return 0;
    const float thr2 = tn * tn;
    float* x1n = xyn;
    float* x2n = xyn + 2 * (size_t)n;
    er_normalise(K, xy1, n, x1n);
    er_normalise(K, xy2, n, x2n);
    uint64_t best = 0;
    double cand[90];
    int valid[10];
    for (int64_t h = hb; h < he; ++h) {
        er_candidates(x1n, x2n, n, seed, (uint64_t)h, cand, valid);
        for (int j = 0; j < 10; ++j) {
            if (!valid[j]) continue;
            const int c = er_score(cand + 9 * j, x1n, x2n, n, thr2, 0);
            const uint64_t id = 10 * (uint64_t)h + (uint64_t)j;
            const uint64_t key = ((uint64_t)(uint32_t)c << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)id);
            if (key > best) { best = key; memcpy(E, cand + 9 * j, sizeof(double) * 9); }
        }
    }
    if (best) *n_inliers = er_score(E, x1n, x2n, n, thr2, mask);
    return best;
}

/* ---- S35 */
static void jacobi_cols(double* G, double* V, int rows, int ncol, int p, int q)
{
    /* G: rows x ncol row-major; V: ncol x ncol row-major */
    double al = G[p] * G[p], be = G[q] * G[q], ga = G[p] * G[q];
    for (int i = 1; i < rows; ++i) {
        al = fma(G[i * ncol + p], G[i * ncol + p], al);
        be = fma(G[i * ncol + q], G[i * ncol + q], be);
        ga = fma(G[i * ncol + p], G[i * ncol + q], ga);
    }
    if (!(ga * ga > 4.930380657631324e-32 * (al * be))) return;
    const double zeta = (be - al) / (2.0 * ga);
    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(fma(zeta, zeta, 1.0)));
    const double c = 1.0 / sqrt(fma(t, t, 1.0));
    const double s = c * t;
    for (int i = 0; i < rows; ++i) {
        const double gp = G[i * ncol + p], gq = G[i * ncol + q];
        G[i * ncol + p] = fma(c, gp, -(s * gq));
        G[i * ncol + q] = fma(s, gp, c * gq);
    }
    for (int i = 0; i < ncol; ++i) {
        const double vp = V[i * ncol + p], vq = V[i * ncol + q];
        V[i * ncol + p] = fma(c, vp, -(s * vq));
        V[i * ncol + q] = fma(s, vp, c * vq);
    }
}

static double colnorm2(const double* G, int rows, int ncol, int p)
{
    double a = G[p] * G[p];
    for (int i = 1; i < rows; ++i) a = fma(G[i * ncol + p], G[i * ncol + p], a);
    return a;
}

/* E -> R1, R2 (row-major), t.  0 = E has rank < 2 or is not finite. */
int er_decompose(const double E[9], double R1[9], double R2[9], double t[3])
{
    double G[9], V[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, cn[3];
    memset(R1, 0, 9 * sizeof(double)); memset(R2, 0, 9 * sizeof(double)); memset(t, 0, 3 * sizeof(double));
    for (int i = 0; i < 9; ++i) {
        if (!(fabs(E[i]) < INFINITY)) return 0;
        G[i] = E[i];
    }
    for (int s = 0; s < NSWEEP_E; ++s) {
        jacobi_cols(G, V, 3, 3, 0, 1);
        jacobi_cols(G, V, 3, 3, 0, 2);
        jacobi_cols(G, V, 3, 3, 1, 2);
    }
    for (int p = 0; p < 3; ++p) cn[p] = colnorm2(G, 3, 3, p);
    int m = 0;
    if (cn[1] < cn[m]) m = 1;
    if (cn[2] < cn[m]) m = 2;
    const int a = m == 0 ? 1 : 0, b = m == 2 ? 1 : 2;
    const int o0 = cn[b] > cn[a] ? b : a, o1 = cn[b] > cn[a] ? a : b;
    if (!(cn[o1] > 0.0)) return 0;
    double u[3][3], v[3][3];
    const double s0 = 1.0 / sqrt(cn[o0]), s1 = 1.0 / sqrt(cn[o1]);
    for (int i = 0; i < 3; ++i) {
        u[0][i] = G[3 * i + o0] * s0;
        u[1][i] = G[3 * i + o1] * s1;
        v[0][i] = V[3 * i + o0]; v[1][i] = V[3 * i + o1]; v[2][i] = V[3 * i + m];
    }
    cross3(u[0], u[1], u[2]);
    double vc[3];
    cross3(v[1], v[2], vc);
    const double dv = fma(v[0][0], vc[0], fma(v[0][1], vc[1], v[0][2] * vc[2]));
    if (dv < 0.0)
        for (int k = 0; k < 3; ++k)
            for (int i = 0; i < 3; ++i) v[k][i] = -v[k][i];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            R1[3 * r + c] = fma(u[2][r], v[2][c], fma(u[0][r], v[1][c], -(u[1][r] * v[0][c])));
            R2[3 * r + c] = fma(u[2][r], v[2][c], fma(u[1][r], v[0][c], -(u[0][r] * v[1][c])));
        }
    const double tn = sqrt(fma(u[2][0], u[2][0], fma(u[2][1], u[2][1], u[2][2] * u[2][2])));
    if (!(tn > 0.0) || !(tn < INFINITY)) return 0;
    const double it = 1.0 / tn;
    for (int i = 0; i < 3; ++i) t[i] = u[2][i] * it;
    return 1;
}

/* linear DLT of one correspondence against [I|0] and [R|t]: homogeneous Q (4) */
void er_triangulate(const double R[9], const double t[3], double x1, double y1, double x2, double y2, double Q[4])
{
    double A[16], V[16];
    const double P0[4] = {R[0], R[1], R[2], t[0]}, P1[4] = {R[3], R[4], R[5], t[1]}, P2[4] = {R[6], R[7], R[8], t[2]};
    for (int c = 0; c < 4; ++c) {
        A[c] = c == 0 ? -1.0 : (c == 2 ? x1 : 0.0);
        A[4 + c] = c == 1 ? -1.0 : (c == 2 ? y1 : 0.0);
        A[8 + c] = x2 * P2[c] - P0[c];
        A[12 + c] = y2 * P2[c] - P1[c];
    }
    for (int i = 0; i < 16; ++i) V[i] = (i % 5) == 0 ? 1.0 : 0.0;
    for (int s = 0; s < NSWEEP_T; ++s)
        for (int p = 0; p < 3; ++p)
            for (int q = p + 1; q < 4; ++q) jacobi_cols(A, V, 4, 4, p, q);
    int m = 0;
    double cm = colnorm2(A, 4, 4, 0);
    for (int p = 1; p < 4; ++p) {
        const double c = colnorm2(A, 4, 4, p);
        if (c < cm) { m = p; cm = c; }
    }
    for (int i = 0; i < 4; ++i) Q[i] = V[4 * i + m];
}

/* OpenCV's cheirality tests on Q for [R|t] */
int er_cheiral(const double R[9], const double t[3], const double Q[4], double dist)
{
    int ok = Q[2] * Q[3] > 0.0;
    const double X = Q[0] / Q[3], Y = Q[1] / Q[3], Z = Q[2] / Q[3];
    ok = ok && Z < dist;
    const double z2 = fma(R[6], X, fma(R[7], Y, fma(R[8], Z, t[2])));
    return ok && z2 > 0.0 && z2 < dist;
}

/* Whole S35 on pixel coordinates.  mask_in may be NULL (all).  Returns n_good, or -1 when E does not decompose (R, t,
 * mask_out, points4 zero).  points4 (may be NULL): 4 n floats. */
int er_recover_pose(const float* xy1, const float* xy2, int n, const double K[4], const double E[9],
                    const uint8_t* mask_in, double dist, double R[9], double t[3], uint8_t* mask_out, float* points4,
                    int* good4)
{
    double R1[9], R2[9], tu[3];
    memset(R, 0, 9 * sizeof(double)); memset(t, 0, 3 * sizeof(double));
    if (n > 0) memset(mask_out, 0, (size_t)n);
    if (points4 && n > 0) memset(points4, 0, 16 * (size_t)n);
    for (int k = 0; k < 4; ++k) good4[k] = 0;
    if (!er_decompose(E, R1, R2, tu)) return -1;
    const double tm[3] = {-tu[0], -tu[1], -tu[2]};
    const double* Rs[4] = {R1, R2, R1, R2};
    const double* ts[4] = {tu, tu, tm, tm};
    for (int i = 0; i < n; ++i) {
        if (mask_in && !mask_in[i]) continue;
        float a[2], b[2];
        er_normalise(K, xy1 + 2 * i, 1, a);
        er_normalise(K, xy2 + 2 * i, 1, b);
        uint8_t bits = 0;
        for (int k = 0; k < 4; ++k) {
            double Q[4];
            er_triangulate(Rs[k], ts[k], a[0], a[1], b[0], b[1], Q);
            if (er_cheiral(Rs[k], ts[k], Q, dist)) { bits |= (uint8_t)(1u << k); ++good4[k]; }
        }
        mask_out[i] = bits;
    }
    const int* g = good4;
    int k;
    if (g[0] >= g[1] && g[0] >= g[2] && g[0] >= g[3]) k = 0;
    else if (g[1] >= g[0] && g[1] >= g[2] && g[1] >= g[3]) k = 1;
    else if (g[2] >= g[0] && g[2] >= g[1] && g[2] >= g[3]) k = 2;
    else k = 3;
    memcpy(R, Rs[k], 9 * sizeof(double));
    memcpy(t, ts[k], 3 * sizeof(double));
    for (int i = 0; i < n; ++i) {
        mask_out[i] = (uint8_t)((mask_out[i] >> k) & 1u);
        if (points4) {
            float a[2], b[2];
            double Q[4];
            er_normalise(K, xy1 + 2 * i, 1, a);
            er_normalise(K, xy2 + 2 * i, 1, b);
            er_triangulate(Rs[k], ts[k], a[0], a[1], b[0], b[1], Q);
            for (int c = 0; c < 4; ++c) points4[4 * i + c] = (float)Q[c];
        }
    }
    return g[k];
}
