/* homography_refine_ref.c — plain-C restatement of docs/SPEC.md S23-S25 (refinement of the robust homography on its
 * inliers: least-squares DLT refit + Levenberg-Marquardt), test infrastructure only.  tests/homography_refine_ref.py
 * builds it with `cc -O2 -ffp-contract=off -shared -fPIC` and loads it with ctypes; tests/test_homography_refine_gpu.py
 * compares the HIP kernel (csrc/homography_refine.hip) with it bit for bit.  Every fused multiply-add is an explicit
 * fma() call, exactly where the SPEC names one, and every sum over correspondences follows the S23 reduction order
 * literally: P partials, correspondence i into partial i mod P, then the stride-halving tree. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define P 512
#define JACOBI_SWEEPS 16
#define JACOBI_SKIP 1e-17
#define LM_LAMBDA0 1e-3
#define LM_MIN_H8 1e-8
#define LM_STEP_TOL 1e-15

typedef struct {
    double cost_in, cost_out;
    int32_t n_used, iters, status, reserved;
} hrr_info;

/* ---- S23 fixed reduction order ------------------------------------------------------------------------------- */
typedef void (*term_fn)(const void* ctx, double x1, double y1, double x2, double y2, double* acc);

static void reduce(const float* xy1, const float* xy2, int n, const uint8_t* mask, int K, term_fn f, const void* ctx,
                   double* out)
{
    double* part = (double*)calloc((size_t)P * K, sizeof(double));
    for (int i = 0; i < n; ++i) {
        if (!mask[i]) continue;
        f(ctx, (double)xy1[2 * i], (double)xy1[2 * i + 1], (double)xy2[2 * i], (double)xy2[2 * i + 1],
          part + (size_t)(i % P) * K);
    }
    for (int s = P / 2; s >= 1; s >>= 1)
        for (int p = 0; p < s; ++p)
            for (int k = 0; k < K; ++k) part[(size_t)p * K + k] = part[(size_t)p * K + k] + part[(size_t)(p + s) * K + k];
    memcpy(out, part, sizeof(double) * K);
    free(part);
}

/* S24: squared forward transfer error of one correspondence under the 9 entries of h */
static double cost_term(const double h[9], double x, double y, double xp, double yp)
{
    const double u = fma(h[0], x, fma(h[1], y, h[2]));
    const double v = fma(h[3], x, fma(h[4], y, h[5]));
    const double w = fma(h[6], x, fma(h[7], y, h[8]));
    const double iw = 1.0 / w;
    const double ru = u * iw - xp, rv = v * iw - yp;
    return fma(ru, ru, rv * rv);
}

/* pass 1: inlier count, coordinate sums, cost of H_in */
static void t_sums(const void* c, double x1, double y1, double x2, double y2, double* a)
{
    a[0] = a[0] + 1.0;
    a[1] = a[1] + x1; a[2] = a[2] + y1; a[3] = a[3] + x2; a[4] = a[4] + y2;
    a[5] = a[5] + cost_term((const double*)c, x1, y1, x2, y2);
}

/* pass 2: distances to the centroids; c = {cx1, cy1, cx2, cy2} */
static void t_dist(const void* c, double x1, double y1, double x2, double y2, double* a)
{
    const double* m = (const double*)c;
    const double dx1 = x1 - m[0], dy1 = y1 - m[1], dx2 = x2 - m[2], dy2 = y2 - m[3];
    a[0] = a[0] + sqrt(fma(dx1, dx1, dy1 * dy1));
    a[1] = a[1] + sqrt(fma(dx2, dx2, dy2 * dy2));
}

/* pass 3: upper triangle of M = sum a1^T a1 + a2^T a2, row-major (j <= k); c = {cx1, cy1, s1, cx2, cy2, s2} */
static void t_normal(const void* c, double x1, double y1, double x2, double y2, double* acc)
{
    const double* m = (const double*)c;
    const double xn = (x1 - m[0]) * m[2], yn = (y1 - m[1]) * m[2];
    const double xq = (x2 - m[3]) * m[5], yq = (y2 - m[4]) * m[5];
    const double a[9] = {-xn, -yn, -1.0, 0.0, 0.0, 0.0, xq * xn, xq * yn, xq};
    const double b[9] = {0.0, 0.0, 0.0, -xn, -yn, -1.0, yq * xn, yq * yn, yq};
    int e = 0;
    for (int j = 0; j < 9; ++j)
        for (int k = j; k < 9; ++k, ++e) acc[e] = acc[e] + fma(a[j], a[k], b[j] * b[k]);
}

/* pass 4: cost of one model */
static void t_cost(const void* c, double x1, double y1, double x2, double y2, double* a)
{
    a[0] = a[0] + cost_term((const double*)c, x1, y1, x2, y2);
}

/* LM pass: J^T J (upper triangle, row-major, 36), J^T r (8), cost (1) at h (h[8] = 1) */
static void t_lm(const void* c, double x, double y, double xp, double yp, double* acc)
{
    const double* h = (const double*)c;
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
    for (int j = 0; j < 8; ++j)
        for (int k = j; k < 8; ++k, ++e) acc[e] = acc[e] + fma(ju[j], ju[k], jv[j] * jv[k]);
    for (int j = 0; j < 8; ++j) acc[36 + j] = acc[36 + j] + fma(ju[j], ru, jv[j] * rv);
    acc[44] = acc[44] + fma(ru, ru, rv * rv);
}

static double cost_of(const float* xy1, const float* xy2, int n, const uint8_t* mask, const double h[9])
{
    double c;
    reduce(xy1, xy2, n, mask, 1, t_cost, h, &c);
    return c;
}

/* S20 step 6: unit Frobenius norm, H[8] >= 0; 0 = invalid */
static int scale_sign(const double in[9], double out[9])
{
    double ss = 0.0;
    for (int i = 0; i < 9; ++i) ss = fma(in[i], in[i], ss);
    const double nrm = sqrt(ss);
    if (!(nrm > 0.0) || !(nrm < INFINITY)) return 0;
    double inv = 1.0 / nrm;
    if (in[8] < 0.0) inv = -inv;
    for (int i = 0; i < 9; ++i) out[i] = in[i] * inv;
    return 1;
}

/* S23 Jacobi: eigenvector of the smallest eigenvalue of the symmetric 9 x 9 M (upper triangle m45).  0 = invalid. */
static int jacobi_min(const double m45[45], double hn[9], int* sweeps_out)
{
    double A[9][9], V[9][9];
    int e = 0;
    for (int j = 0; j < 9; ++j)
        for (int k = j; k < 9; ++k, ++e) { A[j][k] = m45[e]; A[k][j] = m45[e]; }
    for (int j = 0; j < 9; ++j)
        for (int k = 0; k < 9; ++k) V[j][k] = j == k ? 1.0 : 0.0;
    double tr = 0.0;
    for (int j = 0; j < 9; ++j) tr = tr + A[j][j];
    if (!(tr > 0.0) || !(tr < INFINITY)) return 0;
    const double thr = JACOBI_SKIP * tr;
    int sweep = 0;
    while (sweep < JACOBI_SWEEPS) {
        ++sweep;
        int rotated = 0;
        for (int p = 0; p < 8; ++p)
            for (int q = p + 1; q < 9; ++q) {
                const double apq = A[p][q];
                if (!(fabs(apq) > thr)) continue;
                rotated = 1;
                const double app = A[p][p], aqq = A[q][q];
                const double theta = (aqq - app) / (2.0 * apq);
                double t = 1.0 / (fabs(theta) + sqrt(fma(theta, theta, 1.0)));
                if (theta < 0.0) t = -t;
                const double c = 1.0 / sqrt(fma(t, t, 1.0));
                const double s = t * c;
                for (int k = 0; k < 9; ++k) {
                    if (k == p || k == q) continue;
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = fma(c, akp, -(s * akq));
                    A[k][q] = fma(s, akp, c * akq);
                }
                A[p][p] = fma(-t, apq, app);
                A[q][q] = fma(t, apq, aqq);
                A[p][q] = 0.0;
                A[q][p] = 0.0;
                for (int k = 0; k < 9; ++k) {
                    if (k == p || k == q) continue;
                    A[p][k] = A[k][p];
                    A[q][k] = A[k][q];
                }
                for (int k = 0; k < 9; ++k) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = fma(c, vkp, -(s * vkq));
                    V[k][q] = fma(s, vkp, c * vkq);
                }
            }
        if (!rotated) break;
    }
    int mi = 0;
    double dmin = A[0][0];
    for (int j = 1; j < 9; ++j)
        if (A[j][j] < dmin) { dmin = A[j][j]; mi = j; }
    for (int k = 0; k < 9; ++k) hn[k] = V[k][mi];
    if (sweeps_out) *sweeps_out = sweep;
    return 1;
}

/* S23: refit on the inliers.  Returns 1 with H (S20 convention) or 0 = no refit.  nu: inlier count, cost_in: the cost of
 * h_in (pass 1 computes both). */
static int refit(const float* xy1, const float* xy2, int n, const uint8_t* mask, const double h_in[9], double H[9],
                 double* nu, double* cost_in)
{
    double s6[6];
    reduce(xy1, xy2, n, mask, 6, t_sums, h_in, s6);
    *nu = s6[0];
    *cost_in = s6[5];
    for (int i = 0; i < 9; ++i) H[i] = 0.0;
    if (!(s6[0] >= 4.0)) return 0;
    const double c4[4] = {s6[1] / s6[0], s6[2] / s6[0], s6[3] / s6[0], s6[4] / s6[0]};
    double d2[2];
    reduce(xy1, xy2, n, mask, 2, t_dist, c4, d2);
    const double md1 = d2[0] / s6[0], md2 = d2[1] / s6[0];
    if (!(md1 > 0.0) || !(md1 < INFINITY) || !(md2 > 0.0) || !(md2 < INFINITY)) return 0;
    const double s1 = 1.4142135623730951 / md1, s2 = 1.4142135623730951 / md2;
    const double c6[6] = {c4[0], c4[1], s1, c4[2], c4[3], s2};
    double m45[45];
    reduce(xy1, xy2, n, mask, 45, t_normal, c6, m45);
    double hn[9];
    if (!jacobi_min(m45, hn, NULL)) return 0;
    /* S20 step 5 with t = -(s * c) */
    const double t1x = -(s1 * c4[0]), t1y = -(s1 * c4[1]), t2x = -(s2 * c4[2]), t2y = -(s2 * c4[3]);
    double M[3][3], Ho[9];
    for (int i = 0; i < 3; ++i) {
        M[i][0] = hn[3 * i] * s1;
        M[i][1] = hn[3 * i + 1] * s1;
        M[i][2] = fma(hn[3 * i], t1x, fma(hn[3 * i + 1], t1y, hn[3 * i + 2]));
    }
    const double u2x = -t2x, u2y = -t2y;
    for (int j = 0; j < 3; ++j) {
        Ho[j] = fma(u2x, M[2][j], M[0][j]);
        Ho[3 + j] = fma(u2y, M[2][j], M[1][j]);
        Ho[6 + j] = s2 * M[2][j];
    }
    if (!scale_sign(Ho, H)) { for (int i = 0; i < 9; ++i) H[i] = 0.0; return 0; }
    return 1;
}

/* S24: (JtJ + lam diag(JtJ)) d = -g by Cholesky; 0 = not positive definite */
static int lm_solve(const double jtj[36], const double g[8], double lam, double d[8])
{
    double A[8][8], L[8][8], y[8];
    int e = 0;
    for (int j = 0; j < 8; ++j)
        for (int k = j; k < 8; ++k, ++e) { A[j][k] = jtj[e]; A[k][j] = jtj[e]; }
    for (int j = 0; j < 8; ++j) A[j][j] = A[j][j] + lam * A[j][j];
    for (int j = 0; j < 8; ++j) {
        double dd = A[j][j];
        for (int k = 0; k < j; ++k) dd = fma(-L[j][k], L[j][k], dd);
        if (!(dd > 0.0) || !(dd < INFINITY)) return 0;
        L[j][j] = sqrt(dd);
        for (int i = j + 1; i < 8; ++i) {
            double v = A[i][j];
            for (int k = 0; k < j; ++k) v = fma(-L[i][k], L[j][k], v);
            L[i][j] = v / L[j][j];
        }
    }
    for (int i = 0; i < 8; ++i) {
        double v = -g[i];
        for (int k = 0; k < i; ++k) v = fma(-L[i][k], y[k], v);
        y[i] = v / L[i][i];
    }
    for (int i = 7; i >= 0; --i) {
        double v = y[i];
        for (int k = i + 1; k < 8; ++k) v = fma(-L[k][i], d[k], v);
        d[i] = v / L[i][i];
    }
    return 1;
}

/* S23-S25, the whole refinement.  Returns the status (0 refined, 1 kept H_in, 2 zero H_in). */
int hrr_refine(const float* xy1, const float* xy2, int n, const uint8_t* mask, const double H_in[9], int max_iters,
               double H_out[9], hrr_info* info)
{
    double hin[9];
    memcpy(hin, H_in, sizeof hin);
    hrr_info r = {0.0, 0.0, 0, 0, 1, 0};
    int zero = 1;
    for (int i = 0; i < 9; ++i) zero &= hin[i] == 0.0;
    if (zero) {
        r.status = 2;
        memcpy(H_out, hin, sizeof hin);
        if (info) *info = r;
        return r.status;
    }
    double href[9], nu, cost_in;
    const int ok_ref = refit(xy1, xy2, n, mask, hin, href, &nu, &cost_in);
    r.cost_in = cost_in;
    r.cost_out = cost_in;
    r.n_used = (int32_t)nu;
    double start[9], cost_start = cost_in;
    int from_ref = 0;
    memcpy(start, hin, sizeof start);
    if (ok_ref) {
        const double cr = cost_of(xy1, xy2, n, mask, href);
        if (cr <= cost_in) { memcpy(start, href, sizeof start); cost_start = cr; from_ref = 1; }
    }
    double out[9];
    memcpy(out, start, sizeof out);
    double cost_out = cost_start;
    int accepted = 0;
    if (nu >= 4.0 && max_iters > 0 && fabs(start[8]) >= LM_MIN_H8) {
        double h[9], ht[9], acc[45], jtj[36], g[8], d[8];
        for (int i = 0; i < 8; ++i) h[i] = start[i] / start[8];
        h[8] = 1.0;
        reduce(xy1, xy2, n, mask, 45, t_lm, h, acc);
        memcpy(jtj, acc, sizeof jtj);
        memcpy(g, acc + 36, sizeof g);
        double lam = LM_LAMBDA0, cur = cost_start;
        for (int it = 0; it < max_iters; ++it) {
            if (!lm_solve(jtj, g, lam, d)) break;
            double dmax = 0.0, hmax = 1.0;
            for (int i = 0; i < 8; ++i) {             /* NaN propagates into dmax and stops the loop */
                if (!(fabs(d[i]) <= dmax)) dmax = fabs(d[i]);
                if (!(fabs(h[i]) <= hmax)) hmax = fabs(h[i]);
            }
            if (!(dmax > LM_STEP_TOL * hmax)) break;
            for (int i = 0; i < 8; ++i) ht[i] = h[i] + d[i];
            ht[8] = 1.0;
            reduce(xy1, xy2, n, mask, 45, t_lm, ht, acc);
            ++r.iters;
            if (acc[44] < cur) {
                memcpy(h, ht, sizeof h);
                cur = acc[44];
                memcpy(jtj, acc, sizeof jtj);
                memcpy(g, acc + 36, sizeof g);
                lam = lam / 10.0;
                accepted = 1;
            } else {
                lam = lam * 10.0;
            }
        }
        if (accepted) {
            if (scale_sign(h, out)) cost_out = cur;
            else { memcpy(out, start, sizeof out); accepted = 0; }
        }
    }
    r.cost_out = cost_out;
    r.status = (from_ref || accepted) ? 0 : 1;
    memcpy(H_out, out, sizeof out);
    if (info) *info = r;
    return r.status;
}

/* S23 alone (for the SVD cross-check): 1 with H, or 0 = no refit */
int hrr_refit(const float* xy1, const float* xy2, int n, const uint8_t* mask, double H[9])
{
    const double one[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    double nu, c;
    return refit(xy1, xy2, n, mask, one, H, &nu, &c);
}

/* S24's cost of any 9-vector over the inliers, in the S23 order */
double hrr_cost(const float* xy1, const float* xy2, int n, const uint8_t* mask, const double H[9])
{
    return cost_of(xy1, xy2, n, mask, H);
}
