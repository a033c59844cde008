/* twoview_refine_ref.c — plain-C restatement of docs/SPEC.md S43-S47 (refinement of the fundamental matrix and of the
 * calibrated relative pose on their inliers: least-squares 8-point refit + rank-2 Levenberg-Marquardt for F, 5-parameter
 * Levenberg-Marquardt for (R, t)), test infrastructure only.  tests/twoview_refine_ref.py builds it with
 * `cc -O2 -ffp-contract=off -shared -fPIC` and loads it with ctypes; tests/test_twoview_refine_gpu.py compares the HIP
 * kernels (csrc/fundamental_refine.hip, csrc/pose_refine.hip) with it bit for bit.  Every fused multiply-add is an
 * explicit fma() call, exactly where the SPEC names one, and every sum over correspondences follows the S23 reduction
 * order literally: P partials, correspondence i into partial i mod P, then the stride-halving tree. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define P 512
#define JACOBI_SWEEPS 16
#define JACOBI_SKIP 1e-17
#define LM_LAMBDA0 1e-3
#define LM_STEP_TOL 1e-15

typedef struct {
    double cost_in, cost_out;
    int32_t n_used, iters, status, reserved;
} tv_info;

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

/* ---- small dense pieces shared by both refinements ----------------------------------------------------------- */
static double dot3f(const double a[3], const double b[3]) { return fma(a[0], b[0], fma(a[1], b[1], a[2] * b[2])); }

static void cross3(const double a[3], const double b[3], double o[3])
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

/* S7 step 6: unit Frobenius norm, F[8] >= 0; 0 = invalid */
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

/* S7 step 4: one-sided Jacobi on the columns of G with V = I, 6 sweeps; cn: the column norms after them */
static void jacobi3(double G[3][3], double V[3][3], double cn[3])
{
    static const int PQ[3][2] = {{0, 1}, {0, 2}, {1, 2}};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 6; ++sweep)
        for (int e = 0; e < 3; ++e) {
            const int p = PQ[e][0], q = PQ[e][1];
            double al = G[0][p] * G[0][p]; al = fma(G[1][p], G[1][p], al); al = fma(G[2][p], G[2][p], al);
            double be = G[0][q] * G[0][q]; be = fma(G[1][q], G[1][q], be); be = fma(G[2][q], G[2][q], be);
            double ga = G[0][p] * G[0][q]; ga = fma(G[1][p], G[1][q], ga); ga = fma(G[2][p], G[2][q], ga);
            if (!(ga * ga > 4.930380657631324e-32 * (al * be))) continue;
            const double zeta = (be - al) / (2.0 * ga);
            const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(fma(zeta, zeta, 1.0)));
            const double c = 1.0 / sqrt(fma(t, t, 1.0));
            const double s = c * t;
            for (int i = 0; i < 3; ++i) {
                const double gp = G[i][p], gq = G[i][q];
                G[i][p] = fma(c, gp, -(s * gq));
                G[i][q] = fma(s, gp, c * gq);
                const double vp = V[i][p], vq = V[i][q];
                V[i][p] = fma(c, vp, -(s * vq));
                V[i][q] = fma(s, vp, c * vq);
            }
        }
    for (int p = 0; p < 3; ++p) {
        double a = G[0][p] * G[0][p]; a = fma(G[1][p], G[1][p], a); a = fma(G[2][p], G[2][p], a);
        cn[p] = a;
    }
}

static int min_col(const double cn[3])
{
    int m = 0;
    double cm = cn[0];
    if (cn[1] < cm) { m = 1; cm = cn[1]; }
    if (cn[2] < cm) { m = 2; }
    return m;
}

/* S7 step 5: out = T2^T in T1 for T = [[s, 0, tx], [0, s, ty], [0, 0, 1]] */
static void conj(const double in[9], double s1, double t1x, double t1y, double s2, double t2x, double t2y, double out[9])
{
    double M[3][3];
    for (int i = 0; i < 3; ++i) {
        M[i][0] = in[3 * i] * s1;
        M[i][1] = in[3 * i + 1] * s1;
        M[i][2] = fma(in[3 * i], t1x, fma(in[3 * i + 1], t1y, in[3 * i + 2]));
    }
    for (int j = 0; j < 3; ++j) {
        out[j] = s2 * M[0][j];
        out[3 + j] = s2 * M[1][j];
        out[6 + j] = fma(t2x, M[0][j], fma(t2y, M[1][j], M[2][j]));
    }
}

/* S40 step 4: C = Cayley(d / 2) */
static void cayley(const double d[3], double C[9])
{
    const double h0 = 0.5 * d[0], h1 = 0.5 * d[1], h2 = 0.5 * d[2];
    const double cc = (h0 * h0 + h1 * h1) + h2 * h2;
    const double s = 1.0 / (1.0 + cc), m = 1.0 - cc;
    C[0] = (m + 2.0 * (h0 * h0)) * s; C[1] = (2.0 * (h0 * h1 - h2)) * s; C[2] = (2.0 * (h0 * h2 + h1)) * s;
    C[3] = (2.0 * (h0 * h1 + h2)) * s; C[4] = (m + 2.0 * (h1 * h1)) * s; C[5] = (2.0 * (h1 * h2 - h0)) * s;
    C[6] = (2.0 * (h0 * h2 - h1)) * s; C[7] = (2.0 * (h1 * h2 + h0)) * s; C[8] = (m + 2.0 * (h2 * h2)) * s;
}

static void rot3(const double C[9], const double v[3], double o[3])
{
    for (int r = 0; r < 3; ++r) o[r] = (C[3 * r] * v[0] + C[3 * r + 1] * v[1]) + C[3 * r + 2] * v[2];
}

/* S24 step 4 at N parameters: (JtJ + lam diag(JtJ)) d = -g by Cholesky; jtjg: the N (N + 1) / 2 entries j <= k of JtJ
 * (row-major), then g.  0 = not positive definite */
static int lm_solve(int N, const double* jtjg, double lam, double* d)
{
    double A[8][8], L[8][8], y[8];
    const double* g = jtjg + N * (N + 1) / 2;
    int e = 0;
    for (int j = 0; j < N; ++j)
        for (int k = j; k < N; ++k, ++e) { A[j][k] = jtjg[e]; A[k][j] = jtjg[e]; }
    for (int j = 0; j < N; ++j) A[j][j] = A[j][j] + lam * A[j][j];
    for (int j = 0; j < N; ++j) {
        double dd = A[j][j];
        for (int k = 0; k < j; ++k) dd = fma(-L[j][k], L[j][k], dd);
        if (!(dd > 0.0) || !(dd < INFINITY)) return 0;
        L[j][j] = sqrt(dd);
        for (int i = j + 1; i < N; ++i) {
            double v = A[i][j];
            for (int k = 0; k < j; ++k) v = fma(-L[i][k], L[j][k], v);
            L[i][j] = v / L[j][j];
        }
    }
    for (int i = 0; i < N; ++i) {
        double v = -g[i];
        for (int k = 0; k < i; ++k) v = fma(-L[i][k], y[k], v);
        y[i] = v / L[i][i];
    }
    for (int i = N - 1; i >= 0; --i) {
        double v = y[i];
        for (int k = i + 1; k < N; ++k) v = fma(-L[k][i], d[k], v);
        d[i] = v / L[i][i];
    }
    return 1;
}

/* S23 step 4: eigenvector of the smallest eigenvalue of the symmetric 9 x 9 M (upper triangle m45).  0 = invalid. */
static int jacobi_min(const double m45[45], double hn[9])
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
    for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
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
    return 1;
}

/* S45 / S47: the Sampson residual r = num * inv of the model m at (x1, x2) with weights (w1, w2), and its gradient Gm
 * with respect to the 9 entries of m */
static double sampson_grad(const double m[9], const double x1[3], const double x2[3], double w1, double w2, double Gm[9])
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
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Gm[3 * i + j] = fma(p[i], x1[j], -(x2[i] * q[j]));
    return r;
}

/* n_k = sum_ij G_ij ([e_k]x M)_ij: with N = G M^T, n = (N21 - N12, N02 - N20, N10 - N01) */
static void left_rot_grad(const double G[9], const double M[9], double n[3])
{
    double N[3][3];
    for (int i = 0; i < 3; ++i)
        for (int l = 0; l < 3; ++l) N[i][l] = fma(G[3 * i], M[3 * l], fma(G[3 * i + 1], M[3 * l + 1], G[3 * i + 2] * M[3 * l + 2]));
    n[0] = N[2][1] - N[1][2];
    n[1] = N[0][2] - N[2][0];
    n[2] = N[1][0] - N[0][1];
}

static void lm_sums(int N, const double* J, double r, double* acc)
{
    int e = 0;
    for (int j = 0; j < N; ++j)
        for (int k = j; k < N; ++k, ++e) acc[e] = acc[e] + J[j] * J[k];
    for (int j = 0; j < N; ++j, ++e) acc[e] = acc[e] + J[j] * r;
    acc[e] = acc[e] + r * r;
}

/* ================================================================================================================
 * S43-S45: the fundamental matrix
 * ============================================================================================================== */

/* S43: squared Sampson distance (px^2) of one correspondence under f */
static double f_cost_term(const double f[9], double x1, double y1, double x2, double y2)
{
    const double a = fma(f[0], x1, fma(f[1], y1, f[2]));
    const double b = fma(f[3], x1, fma(f[4], y1, f[5]));
    const double c = fma(f[6], x1, fma(f[7], y1, f[8]));
    const double num = fma(x2, a, fma(y2, b, c));
    const double at = fma(f[0], x2, fma(f[3], y2, f[6]));
    const double bt = fma(f[1], x2, fma(f[4], y2, f[7]));
    const double den = fma(a, a, fma(b, b, fma(at, at, bt * bt)));
    return (num * num) / den;
}

static void ft_sums(const void* c, double x1, double y1, double x2, double y2, double* a)
{
    a[0] = a[0] + 1.0;
    a[1] = a[1] + x1; a[2] = a[2] + y1; a[3] = a[3] + x2; a[4] = a[4] + y2;
    a[5] = a[5] + f_cost_term((const double*)c, x1, y1, x2, y2);
}

static void ft_dist(const void* c, double x1, double y1, double x2, double y2, double* a)
{
    const double* m = (const double*)c;
    const double dx1 = x1 - m[0], dy1 = y1 - m[1], dx2 = x2 - m[2], dy2 = y2 - m[3];
    a[0] = a[0] + sqrt(fma(dx1, dx1, dy1 * dy1));
    a[1] = a[1] + sqrt(fma(dx2, dx2, dy2 * dy2));
}

/* c = {cx1, cy1, s1, cx2, cy2, s2} */
static void ft_normal(const void* c, double x1, double y1, double x2, double y2, double* acc)
{
    const double* m = (const double*)c;
    const double xn = (x1 - m[0]) * m[2], yn = (y1 - m[1]) * m[2];
    const double xq = (x2 - m[3]) * m[5], yq = (y2 - m[4]) * m[5];
    const double r[9] = {xq * xn, xq * yn, xq, yq * xn, yq * yn, yq, xn, yn, 1.0};
    int e = 0;
    for (int j = 0; j < 9; ++j)
        for (int k = j; k < 9; ++k, ++e) acc[e] = acc[e] + r[j] * r[k];
}

static void ft_cost(const void* c, double x1, double y1, double x2, double y2, double* a)
{
    a[0] = a[0] + f_cost_term((const double*)c, x1, y1, x2, y2);
}

typedef struct {
    double nrm[6];              /* cx1, cy1, s1, cx2, cy2, s2 */
    double w1, w2;              /* s1^2, s2^2 */
    double F[9], u1[3], v1[3];
} f_lm_ctx;

/* S45 LM pass: 28 of J^T J, 7 of J^T r, the cost */
static void ft_lm(const void* c, double x1, double y1, double x2, double y2, double* acc)
{
    const f_lm_ctx* s = (const f_lm_ctx*)c;
    const double* m = s->nrm;
    const double p1[3] = {(x1 - m[0]) * m[2], (y1 - m[1]) * m[2], 1.0};
    const double p2[3] = {(x2 - m[3]) * m[5], (y2 - m[4]) * m[5], 1.0};
    double Gm[9], J[7], n[3], Gt[9], Ft[9], g[3];
    const double r = sampson_grad(s->F, p1, p2, s->w1, s->w2, Gm);
    left_rot_grad(Gm, s->F, n);
    J[0] = n[0]; J[1] = n[1]; J[2] = n[2];
    /* -F [e_k]x: the left rotation of F^T against Gm^T */
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) { Gt[3 * i + j] = Gm[3 * j + i]; Ft[3 * i + j] = s->F[3 * j + i]; }
    left_rot_grad(Gt, Ft, n);
    J[3] = n[0]; J[4] = n[1]; J[5] = n[2];
    for (int i = 0; i < 3; ++i) g[i] = dot3f(&Gm[3 * i], s->v1);
    J[6] = dot3f(s->u1, g);
    lm_sums(7, J, r, acc);
}

/* F = u0 v0^T + sigma u1 v1^T from the state st = (u0, u1, v0, v1, sigma) */
static void f_of_state(const double st[13], double F[9])
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) F[3 * i + j] = fma(st[i], st[6 + j], (st[12] * st[3 + i]) * st[9 + j]);
}

typedef struct {
    double nu, cost_in, nrm[6];
    int norm_ok, ref_ok;
    double Fref[9];
} f_refit_out;

/* S44: the refit.  nu, cost_in and (if valid) the normalisation are filled in either way */
static void f_refit(const float* xy1, const float* xy2, int n, const uint8_t* mask, const double f_in[9], f_refit_out* o)
{
    double s6[6];
    memset(o, 0, sizeof *o);
    reduce(xy1, xy2, n, mask, 6, ft_sums, f_in, s6);
    o->nu = s6[0];
    o->cost_in = s6[5];
    if (!(s6[0] >= 8.0)) return;
    const double c4[4] = {s6[1] / s6[0], s6[2] / s6[0], s6[3] / s6[0], s6[4] / s6[0]};
    double d2[2];
    reduce(xy1, xy2, n, mask, 2, ft_dist, c4, d2);
    const double md1 = d2[0] / s6[0], md2 = d2[1] / s6[0];
    if (!(md1 > 0.0) || !(md1 < INFINITY) || !(md2 > 0.0) || !(md2 < INFINITY)) return;
    const double s1 = 1.4142135623730951 / md1, s2 = 1.4142135623730951 / md2;
    const double c6[6] = {c4[0], c4[1], s1, c4[2], c4[3], s2};
    memcpy(o->nrm, c6, sizeof c6);
    o->norm_ok = 1;
    double m45[45], gn[9];
    reduce(xy1, xy2, n, mask, 45, ft_normal, c6, m45);
    if (!jacobi_min(m45, gn)) return;
    double G[3][3], V[3][3], cn[3], Fn[9], Fd[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) G[i][j] = gn[3 * i + j];
    jacobi3(G, V, cn);
    const int m = min_col(cn);
    for (int i = 0; i < 3; ++i) G[i][m] = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double a = G[i][0] * V[j][0]; a = fma(G[i][1], V[j][1], a); a = fma(G[i][2], V[j][2], a);
            Fn[3 * i + j] = a;
        }
    conj(Fn, s1, -(s1 * c4[0]), -(s1 * c4[1]), s2, -(s2 * c4[2]), -(s2 * c4[3]), Fd);
    o->ref_ok = scale_sign(Fd, o->Fref);
}

/* S45 step 2: the LM state of the start, in the normalised coordinates; 0 = no LM */
static int f_state(const double start[9], const double nrm[6], double st[13])
{
    double Fs[9], G[3][3], V[3][3], cn[3];
    conj(start, 1.0 / nrm[2], nrm[0], nrm[1], 1.0 / nrm[5], nrm[3], nrm[4], Fs);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) G[i][j] = Fs[3 * i + j];
    jacobi3(G, V, cn);
    const int m = min_col(cn);
    const int a = m == 0 ? 1 : 0, b = m == 2 ? 1 : 2;
    const int o0 = cn[b] > cn[a] ? b : a, o1 = cn[b] > cn[a] ? a : b;
    if (!(cn[o1] > 0.0) || !(cn[o0] < INFINITY)) return 0;
    const double sa = sqrt(cn[o0]), sb = sqrt(cn[o1]);
    const double ia = 1.0 / sa, ib = 1.0 / sb;
    for (int i = 0; i < 3; ++i) {
        st[i] = G[i][o0] * ia;
        st[3 + i] = G[i][o1] * ib;
        st[6 + i] = V[i][o0];
        st[9 + i] = V[i][o1];
    }
    st[12] = sb / sa;
    return 1;
}

/* S45 step 4: the trial state */
static void f_update(const double st[13], const double d[7], double out[13])
{
    double C[9];
    cayley(d, C);
    rot3(C, st, out);
    rot3(C, st + 3, out + 3);
    cayley(d + 3, C);
    rot3(C, st + 6, out + 6);
    rot3(C, st + 9, out + 9);
    out[12] = st[12] + d[6];
}

static double f_cost_of(const float* xy1, const float* xy2, int n, const uint8_t* mask, const double f[9])
{
    double c;
    reduce(xy1, xy2, n, mask, 1, ft_cost, f, &c);
    return c;
}

/* S43-S45, the whole refinement.  Returns the status (0 refined, 1 kept F_in, 2 zero F_in). */
int tv_f_refine(const float* xy1, const float* xy2, int n, const uint8_t* mask, const double F_in[9], int max_iters,
                double F_out[9], tv_info* info)
{
    double fin[9];
    memcpy(fin, F_in, sizeof fin);
    tv_info r = {0.0, 0.0, 0, 0, 1, 0};
    int zero = 1;
    for (int i = 0; i < 9; ++i) zero &= fin[i] == 0.0;
    if (zero) {
        r.status = 2;
        memcpy(F_out, fin, sizeof fin);
        if (info) *info = r;
        return r.status;
    }
    f_refit_out ro;
    f_refit(xy1, xy2, n, mask, fin, &ro);
    r.cost_in = ro.cost_in;
    r.n_used = (int32_t)ro.nu;
    double start[9], cost_start = ro.cost_in;
    int from_ref = 0;
    memcpy(start, fin, sizeof start);
    if (ro.ref_ok) {
        const double cr = f_cost_of(xy1, xy2, n, mask, ro.Fref);
        if (cr <= ro.cost_in) { memcpy(start, ro.Fref, sizeof start); cost_start = cr; from_ref = 1; }
    }
    double out[9];
    memcpy(out, start, sizeof out);
    double cost_out = cost_start;
    int accepted = 0;
    f_lm_ctx lc;
    double st[13];
    if (ro.norm_ok && max_iters > 0 && f_state(start, ro.nrm, st)) {
        double acc[36], jg[36], d[7], tr[13];
        memcpy(lc.nrm, ro.nrm, sizeof lc.nrm);
        lc.w1 = ro.nrm[2] * ro.nrm[2];
        lc.w2 = ro.nrm[5] * ro.nrm[5];
        f_of_state(st, lc.F);
        memcpy(lc.u1, st + 3, sizeof lc.u1);
        memcpy(lc.v1, st + 9, sizeof lc.v1);
        reduce(xy1, xy2, n, mask, 36, ft_lm, &lc, acc);
        memcpy(jg, acc, sizeof jg);
        double lam = LM_LAMBDA0, cur = acc[35];
        for (int it = 0; it < max_iters; ++it) {
            if (!lm_solve(7, jg, lam, d)) break;
            double dmax = 0.0;
            for (int i = 0; i < 7; ++i)               /* NaN propagates into dmax and stops the loop */
                if (!(fabs(d[i]) <= dmax)) dmax = fabs(d[i]);
            if (!(dmax > LM_STEP_TOL)) break;
            f_update(st, d, tr);
            f_of_state(tr, lc.F);
            memcpy(lc.u1, tr + 3, sizeof lc.u1);
            memcpy(lc.v1, tr + 9, sizeof lc.v1);
            reduce(xy1, xy2, n, mask, 36, ft_lm, &lc, acc);
            ++r.iters;
            if (acc[35] < cur) {
                memcpy(st, tr, sizeof st);
                cur = acc[35];
                memcpy(jg, acc, sizeof jg);
                lam = lam / 10.0;
                accepted = 1;
            } else {
                lam = lam * 10.0;
            }
        }
        if (accepted) {
            double Fn[9], Fd[9], Fl[9];
            const double* m = ro.nrm;
            f_of_state(st, Fn);
            conj(Fn, m[2], -(m[2] * m[0]), -(m[2] * m[1]), m[5], -(m[5] * m[3]), -(m[5] * m[4]), Fd);
            accepted = 0;
            if (scale_sign(Fd, Fl)) {
                const double cl = f_cost_of(xy1, xy2, n, mask, Fl);
                if (cl < cost_start) { memcpy(out, Fl, sizeof out); cost_out = cl; accepted = 1; }
            }
        }
    }
    r.cost_out = cost_out;
    r.status = (from_ref || accepted) ? 0 : 1;
    memcpy(F_out, out, sizeof out);
    if (info) *info = r;
    return r.status;
}

/* S44 alone (for the SVD cross-check): 1 with F, or 0 = no refit */
int tv_f_refit(const float* xy1, const float* xy2, int n, const uint8_t* mask, double F[9])
{
    const double one[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    f_refit_out ro;
    f_refit(xy1, xy2, n, mask, one, &ro);
    memcpy(F, ro.Fref, sizeof ro.Fref);
    return ro.ref_ok;
}

/* S43's cost of any 9-vector over the inliers, in the S23 order */
double tv_f_cost(const float* xy1, const float* xy2, int n, const uint8_t* mask, const double F[9])
{
    return f_cost_of(xy1, xy2, n, mask, F);
}

/* ================================================================================================================
 * S46-S47: the relative pose
 * ============================================================================================================== */

typedef struct {
    double K[4];                /* fx, fy, cx, cy */
    double R[9], t[3], E[9], b1[3], b2[3];
} p_ctx;

static void e_of(const double R[9], const double t[3], double E[9])
{
    for (int j = 0; j < 3; ++j) {
        E[j] = t[1] * R[6 + j] - t[2] * R[3 + j];
        E[3 + j] = t[2] * R[j] - t[0] * R[6 + j];
        E[6 + j] = t[0] * R[3 + j] - t[1] * R[j];
    }
}

/* S31: the normalised coordinate as the scorer reads it */
static double norm31(double x, double c, double f)
{
    const float v = (float)((x - c) / f);
    return fabsf(v) <= 1048576.0f ? (double)v : (double)NAN;      /* S31: NaN, an infinity, beyond 2^20: NaN */
}

/* S46: squared Sampson distance of one correspondence under E, in normalised units */
static double p_cost_term(const p_ctx* s, double x1, double y1, double x2, double y2)
{
    const double* K = s->K;
    const double p1[3] = {norm31(x1, K[2], K[0]), norm31(y1, K[3], K[1]), 1.0};
    const double p2[3] = {norm31(x2, K[2], K[0]), norm31(y2, K[3], K[1]), 1.0};
    double Gm[9];
    const double r = sampson_grad(s->E, p1, p2, 1.0, 1.0, Gm);
    return r * r;
}

static void pt_sums(const void* c, double x1, double y1, double x2, double y2, double* a)
{
    a[0] = a[0] + 1.0;
    a[1] = a[1] + p_cost_term((const p_ctx*)c, x1, y1, x2, y2);
}

/* S47 LM pass: 15 of J^T J, 5 of J^T r, the cost */
static void pt_lm(const void* c, double x1, double y1, double x2, double y2, double* acc)
{
    const p_ctx* s = (const p_ctx*)c;
    const double* K = s->K;
    const double* t = s->t;
    const double p1[3] = {norm31(x1, K[2], K[0]), norm31(y1, K[3], K[1]), 1.0};
    const double p2[3] = {norm31(x2, K[2], K[0]), norm31(y2, K[3], K[1]), 1.0};
    double Gm[9], G2[9], n[3], J[5];
    const double r = sampson_grad(s->E, p1, p2, 1.0, 1.0, Gm);
    for (int j = 0; j < 3; ++j) {
        G2[j] = t[2] * Gm[3 + j] - t[1] * Gm[6 + j];
        G2[3 + j] = t[0] * Gm[6 + j] - t[2] * Gm[j];
        G2[6 + j] = t[1] * Gm[j] - t[0] * Gm[3 + j];
    }
    left_rot_grad(G2, s->R, n);
    J[0] = n[0]; J[1] = n[1]; J[2] = n[2];
    left_rot_grad(Gm, s->R, n);
    J[3] = dot3f(s->b1, n);
    J[4] = dot3f(s->b2, n);
    lm_sums(5, J, r, acc);
}

/* S47 step 2: the deterministic orthonormal basis (b1, b2) of the plane orthogonal to the unit vector t */
static void tangent_basis(const double t[3], double b1[3], double b2[3])
{
    int k = 0;
    double m = fabs(t[0]);
    if (fabs(t[1]) < m) { k = 1; m = fabs(t[1]); }
    if (fabs(t[2]) < m) { k = 2; }
    const double e[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
    double w[3];
    cross3(t, e, w);
    const double inv = 1.0 / sqrt(dot3f(w, w));
    for (int i = 0; i < 3; ++i) b1[i] = w[i] * inv;
    cross3(t, b1, b2);
}

static void p_set(p_ctx* s, const double Rt[12])
{
    memcpy(s->R, Rt, sizeof s->R);
    memcpy(s->t, Rt + 9, sizeof s->t);
    e_of(s->R, s->t, s->E);
}

/* S33 step 8's scale and sign of E = [t]x R; zeros if its norm is not in (0, inf) */
static void e_out_of(const double Rt[12], double E[9])
{
    double e[9], ss = 0.0;
    e_of(Rt, Rt + 9, e);
    for (int i = 0; i < 9; ++i) ss = fma(e[i], e[i], ss);
    const double nrm = sqrt(ss);
    for (int i = 0; i < 9; ++i) E[i] = 0.0;
    if (!(nrm > 0.0) || !(nrm < INFINITY)) return;
    int mi = 0;
    for (int i = 1; i < 9; ++i)
        if (fabs(e[i]) > fabs(e[mi])) mi = i;
    double inv = 1.0 / nrm;
    if (e[mi] < 0.0) inv = -inv;
    for (int i = 0; i < 9; ++i) E[i] = e[i] * inv;
}

/* S46-S47, the whole refinement of (R, t) (12 doubles).  Returns the status (0 refined, 1 kept the input, 2 zero). */
int tv_pose_refine(const float* xy1, const float* xy2, int n, const double K[4], const uint8_t* mask, const double Rt_in[12],
                   int max_iters, double Rt_out[12], double E_out[9], tv_info* info)
{
    double in[12];
    memcpy(in, Rt_in, sizeof in);
    tv_info r = {0.0, 0.0, 0, 0, 1, 0};
    int zero = 1;
    for (int i = 0; i < 12; ++i) zero &= in[i] == 0.0;
    if (zero) {
        r.status = 2;
        memcpy(Rt_out, in, sizeof in);
        for (int i = 0; i < 9; ++i) E_out[i] = 0.0;
        if (info) *info = r;
        return r.status;
    }
    p_ctx s;
    memcpy(s.K, K, sizeof s.K);
    const double fm = 0.5 * (K[0] + K[1]);
    const double f2 = fm * fm;
    double s2[2];
    p_set(&s, in);
    reduce(xy1, xy2, n, mask, 2, pt_sums, &s, s2);
    const double nu = s2[0], cin = s2[1];
    r.n_used = (int32_t)nu;
    r.cost_in = cin * f2;
    double cur = cin, pose[12];
    int accepted = 0;
    memcpy(pose, in, sizeof pose);
    const double tt = dot3f(in + 9, in + 9);
    if (nu >= 5.0 && max_iters > 0 && tt > 0.0 && tt < INFINITY) {
        double acc[21], jg[21], d[5], tr[12], C[9];
        const double it0 = 1.0 / sqrt(tt);
        for (int i = 0; i < 3; ++i) pose[9 + i] = in[9 + i] * it0;
        p_set(&s, pose);
        tangent_basis(s.t, s.b1, s.b2);
        reduce(xy1, xy2, n, mask, 21, pt_lm, &s, acc);
        memcpy(jg, acc, sizeof jg);
        double lam = LM_LAMBDA0;
        for (int it = 0; it < max_iters; ++it) {
            if (!lm_solve(5, jg, lam, d)) break;
            double dmax = 0.0;
            for (int i = 0; i < 5; ++i)               /* NaN propagates into dmax and stops the loop */
                if (!(fabs(d[i]) <= dmax)) dmax = fabs(d[i]);
            if (!(dmax > LM_STEP_TOL)) break;
            cayley(d, C);
            for (int rr = 0; rr < 3; ++rr)
                for (int c = 0; c < 3; ++c)
                    tr[3 * rr + c] = (C[3 * rr] * pose[c] + C[3 * rr + 1] * pose[3 + c]) + C[3 * rr + 2] * pose[6 + c];
            double q[3];
            for (int i = 0; i < 3; ++i) q[i] = fma(d[4], s.b2[i], fma(d[3], s.b1[i], pose[9 + i]));
            const double iq = 1.0 / sqrt(dot3f(q, q));
            for (int i = 0; i < 3; ++i) tr[9 + i] = q[i] * iq;
            p_ctx st = s;
            p_set(&st, tr);
            tangent_basis(st.t, st.b1, st.b2);
            reduce(xy1, xy2, n, mask, 21, pt_lm, &st, acc);
            ++r.iters;
            if (acc[20] < cur) {
                memcpy(pose, tr, sizeof pose);
                s = st;
                cur = acc[20];
                memcpy(jg, acc, sizeof jg);
                lam = lam / 10.0;
                accepted = 1;
            } else {
                lam = lam * 10.0;
            }
        }
    }
    if (!accepted) memcpy(pose, in, sizeof pose);
    r.cost_out = accepted ? cur * f2 : r.cost_in;
    r.status = accepted ? 0 : 1;
    memcpy(Rt_out, pose, sizeof pose);
    e_out_of(pose, E_out);
    if (info) *info = r;
    return r.status;
}

/* S46's cost (px^2) of a pose over the inliers, in the S23 order */
double tv_pose_cost(const float* xy1, const float* xy2, int n, const double K[4], const uint8_t* mask, const double Rt[12])
{
    p_ctx s;
    double s2[2];
    memcpy(s.K, K, sizeof s.K);
    p_set(&s, Rt);
    reduce(xy1, xy2, n, mask, 2, pt_sums, &s, s2);
    const double fm = 0.5 * (K[0] + K[1]);
    return s2[1] * (fm * fm);
}
