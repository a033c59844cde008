/* pnp_ref.c — plain-C restatement of docs/SPEC.md S36-S40 (absolute camera pose: camera check, 3-sample, P3P solve,
 * division-free reprojection test, RANSAC-PnP winner, Levenberg-Marquardt refinement on the inliers).  Built with
 * -ffp-contract=off: the only fused multiply-adds are the explicit fma() / fmaf() calls, so every value is the bits the
 * HIP kernels (pnp_core.hpp, pnp_solve.hip, ransac_p_fused.hip, pnp_refine.hip) produce.  Loaded by pnp_ref.py. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define MAX_CAND 4
#define SLOT 12
#define BISECT_STEPS 64

static uint64_t mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

/* S36: K (fx, fy, cx, cy) finite with fx, fy > 0, and thresh_px finite and > 0 */
int pr_k_valid(const double* K, float thresh_px)
{
    for (int i = 0; i < 4; ++i)
        if (!isfinite(K[i])) return 0;
    return K[0] > 0.0 && K[1] > 0.0 && thresh_px > 0.0f && isfinite(thresh_px);
}

/* S37 */
void pr_sample(uint64_t seed, uint64_t h, int n, int32_t* idx)
{
    const uint64_t stream = mix64(seed ^ 0x165667B19E3779F9ULL) ^ mix64(h + 0xD1B54A32D192ED03ULL);
    int cnt = 0;
    for (uint64_t d = 0; d < 64 && cnt < 3; ++d) {
        const uint64_t r = mix64(stream + (d + 1) * 0x9E3779B97F4A7C15ULL);
        const int c = (int)(((r >> 32) * (uint64_t)(uint32_t)n) >> 32);
        int rep = 0;
        for (int s = 0; s < cnt; ++s) rep |= idx[s] == c;
        if (!rep) idx[cnt++] = c;
    }
    for (int c = 0; cnt < 3; ++c) {
        int rep = 0;
        for (int s = 0; s < cnt; ++s) rep |= idx[s] == c;
        if (!rep) idx[cnt++] = c;
    }
}

/* S33 step 6 at degree 4: real roots of p (ascending coefficients), ascending; returns their number */
int pr_roots(const double* p, double* roots)
{
    enum { DEG = 4 };
    const double c = p[DEG];
    if (!(fabs(c) > 0.0) || !(fabs(c) < INFINITY)) return 0;
    double D[DEG + 1][DEG];
    double mx = 0.0;
    int fin = 1;
    for (int k = 0; k < DEG; ++k) {
        D[DEG][k] = p[k] / c;
        fin = fin && fabs(D[DEG][k]) < INFINITY;
        if (fabs(D[DEG][k]) > mx) mx = fabs(D[DEG][k]);
    }
    if (!fin) return 0;
    const double R = 1.0 + mx;
    for (int d = DEG; d >= 2; --d)
        for (int k = 0; k < d - 1; ++k) D[d - 1][k] = D[d][k + 1] * ((double)(k + 1) / (double)d);
    double r[DEG], e[DEG + 2];
    int m = 1;
    r[0] = -D[1][0];
    for (int d = 2; d <= DEG; ++d) {
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
            for (int s = 0; s < BISECT_STEPS; ++s) {
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

static double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

static void cross3(const double* a, const double* b, double* o)
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

/* S38 step 1: pixel -> unit bearing; 0 if not finite */
static int bearing(const double* K, float u, float v, double* f)
{
    const double x = ((double)u - K[2]) / K[0], y = ((double)v - K[3]) / K[1];
    const double q = (x * x + y * y) + 1.0;
    const double inv = 1.0 / sqrt(q);
    f[0] = x * inv; f[1] = y * inv; f[2] = inv;
    return q < INFINITY;
}

/* S38 step 5: orthonormal triad (e1, e2, n) of p0, p1, p2; 0 if a length is zero or not finite */
static int triad(const double* p0, const double* p1, const double* p2, double T[3][3])
{
    double d1[3], d2[3], nn[3];
    for (int i = 0; i < 3; ++i) { d1[i] = p1[i] - p0[i]; d2[i] = p2[i] - p0[i]; }
    cross3(d1, d2, nn);
    const double l1 = dot3(d1, d1), ln = dot3(nn, nn);
    if (!(l1 > 0.0) || !(l1 < INFINITY) || !(ln > 0.0) || !(ln < INFINITY)) return 0;
    const double i1 = 1.0 / sqrt(l1), in = 1.0 / sqrt(ln);
    for (int i = 0; i < 3; ++i) { T[0][i] = d1[i] * i1; T[2][i] = nn[i] * in; }
    cross3(T[2], T[0], T[1]);
    return 1;
}

/* S38 on 3 world points X (3 x 3 f32) and their pixels uv (3 x 2 f32): out[SLOT j .. + 11] = R (row-major), t of
 * candidate j (zero when invalid), valid[j]; coef (may be NULL) = the quartic; returns the number of valid candidates */
int pr_p3p(const double* K, const float* X, const float* uv, double* out, int32_t* valid, double* coef)
{
    memset(out, 0, sizeof(double) * SLOT * MAX_CAND);
    for (int j = 0; j < MAX_CAND; ++j) valid[j] = 0;
    double P[3][3], f[3][3];
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) P[i][k] = (double)X[3 * i + k];
    int ok = 1;
    for (int i = 0; i < 3; ++i) ok = bearing(K, uv[2 * i], uv[2 * i + 1], f[i]) && ok;
    double d1[3], d2[3], d12[3], nn[3];
    for (int i = 0; i < 3; ++i) { d1[i] = P[1][i] - P[0][i]; d2[i] = P[2][i] - P[0][i]; d12[i] = P[1][i] - P[2][i]; }
    cross3(d1, d2, nn);
    const double c2 = dot3(d1, d1), b2 = dot3(d2, d2), a2 = dot3(d12, d12), ln = dot3(nn, nn);
    if (!ok || !(ln > 1.4210854715202004e-14 * (c2 * b2)) || !(ln < INFINITY)) return 0;
    const double ca = dot3(f[1], f[2]), cb = dot3(f[0], f[2]), cg = dot3(f[0], f[1]);
    const double p = (a2 - c2) / b2, q = (a2 + c2) / b2, rc = c2 / b2, ra = a2 / b2;
    const double rbc = (b2 - c2) / b2, rba = (b2 - a2) / b2;
    double A[5];
    A[4] = (p - 1.0) * (p - 1.0) - 4.0 * rc * ca * ca;
    A[3] = 4.0 * ((p * (1.0 - p) * cb - (1.0 - q) * ca * cg) + 2.0 * rc * ca * ca * cb);
    A[2] = 2.0 * (((((p * p - 1.0) + 2.0 * p * p * cb * cb) + 2.0 * rbc * ca * ca) - 4.0 * q * ca * cb * cg) + 2.0 * rba * cg * cg);
    A[1] = 4.0 * ((-p * (1.0 + p) * cb + 2.0 * ra * cg * cg * cb) - (1.0 - q) * ca * cg);
    A[0] = (1.0 + p) * (1.0 + p) - 4.0 * ra * cg * cg;
    if (coef) memcpy(coef, A, sizeof A);
    double TW[3][3];
    if (!triad(P[0], P[1], P[2], TW)) return 0;
    double roots[4];
    const int nr = pr_roots(A, roots);
    int nv = 0;
    for (int j = 0; j < nr; ++j) {
        const double v = roots[j];
        const double u = (((p - 1.0) * v * v - 2.0 * p * cb * v) + (1.0 + p)) / (2.0 * (cg - v * ca));
        const double s0q = b2 / ((1.0 + v * v) - 2.0 * v * cb);
        if (!(s0q > 0.0) || !(s0q < INFINITY)) continue;
        const double s0 = sqrt(s0q), s1 = u * s0, s2 = v * s0;
        if (!(s1 > 0.0) || !(s2 > 0.0) || !(s1 < INFINITY) || !(s2 < INFINITY)) continue;
        double c[3][3], TC[3][3];
        for (int i = 0; i < 3; ++i) { c[0][i] = s0 * f[0][i]; c[1][i] = s1 * f[1][i]; c[2][i] = s2 * f[2][i]; }
        if (!triad(c[0], c[1], c[2], TC)) continue;
        double Rt[SLOT];
        for (int r = 0; r < 3; ++r)
            for (int k = 0; k < 3; ++k) Rt[3 * r + k] = (TC[0][r] * TW[0][k] + TC[1][r] * TW[1][k]) + TC[2][r] * TW[2][k];
        for (int r = 0; r < 3; ++r)
            Rt[9 + r] = c[0][r] - ((Rt[3 * r] * P[0][0] + Rt[3 * r + 1] * P[0][1]) + Rt[3 * r + 2] * P[0][2]);
        int fin = 1;
        for (int i = 0; i < SLOT; ++i) fin = fin && fabs(Rt[i]) < INFINITY;
        if (!fin) continue;
        memcpy(out + SLOT * j, Rt, sizeof Rt);
        valid[j] = 1;
        ++nv;
    }
    return nv;
}

/* S39: P32 = (float)(K [R|t]), row-major 3 x 4 */
void pr_proj32(const double* K, const double* Rt, float* P)
{
    for (int c = 0; c < 3; ++c) {
        P[c] = (float)(K[0] * Rt[c] + K[2] * Rt[6 + c]);
        P[4 + c] = (float)(K[1] * Rt[3 + c] + K[3] * Rt[6 + c]);
        P[8 + c] = (float)Rt[6 + c];
    }
    P[3] = (float)(K[0] * Rt[9] + K[2] * Rt[11]);
    P[7] = (float)(K[1] * Rt[10] + K[3] * Rt[11]);
    P[11] = (float)Rt[11];
}

static int inlier(const float* P, const float* X, const float* uv, float thr2)
{
    const float x = X[0], y = X[1], z = X[2], u = uv[0], v = uv[1];
    const float a = fmaf(P[0], x, fmaf(P[1], y, fmaf(P[2], z, P[3])));
    const float b = fmaf(P[4], x, fmaf(P[5], y, fmaf(P[6], z, P[7])));
    const float w = fmaf(P[8], x, fmaf(P[9], y, fmaf(P[10], z, P[11])));
    const float du = fmaf(-u, w, a), dv = fmaf(-v, w, b);
    const float lhs = fmaf(du, du, dv * dv), rhs = thr2 * (w * w);
    return lhs <= rhs && w > 0.0f && rhs > 0.0f && rhs < INFINITY;
}

/* S39 of the pose Rt (12 doubles) over n correspondences: mask (may be NULL), returns the count */
int pr_score(const double* K, const double* Rt, const float* X, const float* uv, int n, float thr2, uint8_t* mask)
{
    float P[12];
    pr_proj32(K, Rt, P);
    int c = 0;
    for (int i = 0; i < n; ++i) {
        const int in = inlier(P, X + 3 * i, uv + 2 * i, thr2);
        if (mask) mask[i] = (uint8_t)in;
        c += in;
    }
    return c;
}

/* S37 + S38 of sample h: out 4 x 12, valid 4 (n < 4: no candidate) */
int pr_candidates(const double* K, const float* X, const float* uv, int n, uint64_t seed, uint64_t h, double* out,
                  int32_t* valid)
{
    memset(out, 0, sizeof(double) * SLOT * MAX_CAND);
    for (int j = 0; j < MAX_CAND; ++j) valid[j] = 0;
    if (n < 4) return 0;
    int32_t idx[3];
    pr_sample(seed, h, n, idx);
    float Xs[9], us[6];
    for (int i = 0; i < 3; ++i) {
        for (int k = 0; k < 3; ++k) Xs[3 * i + k] = X[3 * idx[i] + k];
        us[2 * i] = uv[2 * idx[i]]; us[2 * i + 1] = uv[2 * idx[i] + 1];
    }
    return pr_p3p(K, Xs, us, out, valid, 0);
}

/* S39: whole run over samples [hyp_begin, hyp_end) (model ids 4h + j): the key; Rt (12), mask (n), count */
uint64_t pr_run(const double* K, const float* X, const float* uv, int n, uint64_t seed, int64_t hyp_begin, int64_t hyp_end,
                float thresh_px, double* Rt, uint8_t* mask, int32_t* count)
{
    const float thr2 = thresh_px * thresh_px;
    uint64_t best = 0;
    double cand[SLOT * MAX_CAND];
    int32_t valid[MAX_CAND];
    memset(Rt, 0, sizeof(double) * SLOT);
    for (int64_t h = hyp_begin; h < hyp_end; ++h) {
        pr_candidates(K, X, uv, n, seed, (uint64_t)h, cand, valid);
        for (int j = 0; j < MAX_CAND; ++j) {
            if (!valid[j]) continue;
            const uint32_t id = (uint32_t)(4 * h + j);
            const int c = pr_score(K, cand + SLOT * j, X, uv, n, thr2, 0);
            const uint64_t key = ((uint64_t)(uint32_t)c << 32) | (uint64_t)(0xFFFFFFFFu - id);
            if (key > best) { best = key; memcpy(Rt, cand + SLOT * j, sizeof(double) * SLOT); }
        }
    }
    *count = 0;
    if (mask) memset(mask, 0, (size_t)n);
    if (best) *count = pr_score(K, Rt, X, uv, n, thr2, mask);
    return best;
}

/* ---- S40: Levenberg-Marquardt on the inliers ------------------------------------------------------------------------ */
#define HR_P 512
#define NJ 21            /* J^T J entries j <= k, row-major */
#define NLM (NJ + 6 + 1) /* + J^T r + cost */

/* S23's tree over the P partials */
static void reduce(double (*part)[NLM], int nk, double* out)
{
    for (int s = HR_P / 2; s >= 1; s >>= 1)
        for (int p = 0; p < s; ++p)
            for (int k = 0; k < nk; ++k) part[p][k] = part[p][k] + part[p + s][k];
    for (int k = 0; k < nk; ++k) out[k] = part[0][k];
}

/* Y = R X, x_cam = Y + t */
static void cam_point(const double* Rt, const float* X, double* xc, double* Y)
{
    const double x = X[0], y = X[1], z = X[2];
    for (int r = 0; r < 3; ++r) {
        Y[r] = (Rt[3 * r] * x + Rt[3 * r + 1] * y) + Rt[3 * r + 2] * z;
        xc[r] = Y[r] + Rt[9 + r];
    }
}

static double cost_term(const double* K, const double* Rt, const float* X, const float* uv)
{
    double xc[3], Y[3];
    cam_point(Rt, X, xc, Y);
    const double iz = 1.0 / xc[2];
    const double ru = (K[0] * (xc[0] * iz) + K[2]) - (double)uv[0];
    const double rv = (K[1] * (xc[1] * iz) + K[3]) - (double)uv[1];
    return fma(ru, ru, rv * rv);
}

static void lm_term(double* a, const double* K, const double* Rt, const float* X, const float* uv)
{
    double xc[3], Y[3];
    cam_point(Rt, X, xc, Y);
    const double iz = 1.0 / xc[2];
    const double px = xc[0] * iz, py = xc[1] * iz;
    const double ru = (K[0] * px + K[2]) - (double)uv[0];
    const double rv = (K[1] * py + K[3]) - (double)uv[1];
    const double fa = K[0] * iz, fb = K[1] * iz;
    const double ju[6] = {-((fa * px) * Y[1]), fa * Y[2] + (fa * px) * Y[0], -(fa * Y[1]), fa, 0.0, -(fa * px)};
    const double jv[6] = {-(fb * Y[2]) - (fb * py) * Y[1], (fb * py) * Y[0], fb * Y[0], 0.0, fb, -(fb * py)};
    int e = 0;
    for (int j = 0; j < 6; ++j)
        for (int k = j; k < 6; ++k, ++e) a[e] = a[e] + fma(ju[j], ju[k], jv[j] * jv[k]);
    for (int j = 0; j < 6; ++j) a[NJ + j] = a[NJ + j] + fma(ju[j], ru, jv[j] * rv);
    a[NJ + 6] = a[NJ + 6] + fma(ru, ru, rv * rv);
}

static void pass_cost(const double* K, const double* Rt, const float* X, const float* uv, int n, const uint8_t* mask,
                      double (*part)[NLM], double* nu, double* cost)
{
    memset(part, 0, sizeof(double) * NLM * HR_P);
    for (int i = 0; i < n; ++i) {
        if (!mask[i]) continue;
        double* a = part[i % HR_P];
        a[0] = a[0] + 1.0;
        a[1] = a[1] + cost_term(K, Rt, X + 3 * i, uv + 2 * i);
    }
    double out[2];
    reduce(part, 2, out);
    *nu = out[0];
    *cost = out[1];
}

static void pass_lm(const double* K, const double* Rt, const float* X, const float* uv, int n, const uint8_t* mask,
                    double (*part)[NLM], double* out)
{
    memset(part, 0, sizeof(double) * NLM * HR_P);
    for (int i = 0; i < n; ++i)
        if (mask[i]) lm_term(part[i % HR_P], K, Rt, X + 3 * i, uv + 2 * i);
    reduce(part, NLM, out);
}

/* S40 step 3: Cholesky of (JtJ + lam diag JtJ) d = -g, S24's order at 6 parameters */
int pr_lm_solve(const double* jtjg, double lam, double* d)
{
    double L[6][6], y[6];
    for (int j = 0; j < 6; ++j) {
        const double ajj = jtjg[j * 6 - j * (j - 1) / 2];
        double dd = ajj + lam * ajj;
        for (int k = 0; k < j; ++k) dd = fma(-L[j][k], L[j][k], dd);
        if (!(dd > 0.0) || !(dd < INFINITY)) return 0;
        L[j][j] = sqrt(dd);
        for (int i = j + 1; i < 6; ++i) {
            double v = jtjg[j * 6 - j * (j - 1) / 2 + (i - j)];
            for (int k = 0; k < j; ++k) v = fma(-L[i][k], L[j][k], v);
            L[i][j] = v / L[j][j];
        }
    }
    for (int i = 0; i < 6; ++i) {
        double v = -jtjg[NJ + i];
        for (int k = 0; k < i; ++k) v = fma(-L[i][k], y[k], v);
        y[i] = v / L[i][i];
    }
    for (int i = 5; i >= 0; --i) {
        double v = y[i];
        for (int k = i + 1; k < 6; ++k) v = fma(-L[k][i], d[k], v);
        d[i] = v / L[i][i];
    }
    return 1;
}

/* S40 step 4: R' = C(d[0..2] / 2) R (Cayley, transcendental-free), t' = t + d[3..5] */
void pr_update(const double* Rt, const double* d, double* out)
{
    const double h0 = 0.5 * d[0], h1 = 0.5 * d[1], h2 = 0.5 * d[2];
    const double cc = (h0 * h0 + h1 * h1) + h2 * h2;
    const double s = 1.0 / (1.0 + cc), m = 1.0 - cc;
    double C[9], R[9];
    C[0] = (m + 2.0 * (h0 * h0)) * s; C[1] = (2.0 * (h0 * h1 - h2)) * s; C[2] = (2.0 * (h0 * h2 + h1)) * s;
    C[3] = (2.0 * (h0 * h1 + h2)) * s; C[4] = (m + 2.0 * (h1 * h1)) * s; C[5] = (2.0 * (h1 * h2 - h0)) * s;
    C[6] = (2.0 * (h0 * h2 - h1)) * s; C[7] = (2.0 * (h1 * h2 + h0)) * s; C[8] = (m + 2.0 * (h2 * h2)) * s;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[3 * r + c] = (C[3 * r] * Rt[c] + C[3 * r + 1] * Rt[3 + c]) + C[3 * r + 2] * Rt[6 + c];
    for (int i = 0; i < 3; ++i) out[9 + i] = Rt[9 + i] + d[3 + i];
    memcpy(out, R, sizeof R);
}

/* S40: refinement of Rt_in (12) on the correspondences with mask[i] != 0.  Rt_out (12, may alias Rt_in),
 * costs = (cost_in, cost_out), ints = (n_used, iters, status) */
void pr_refine(const double* K, const float* X, const float* uv, int n, const uint8_t* mask, const double* Rt_in,
               int max_iters, double* Rt_out, double* costs, int32_t* ints)
{
    static double part[HR_P][NLM];
    double in[12];
    memcpy(in, Rt_in, sizeof in);
    int zero = 1;
    for (int i = 0; i < 12; ++i) zero = zero && in[i] == 0.0;
    if (zero) {
        memcpy(Rt_out, in, sizeof in);
        costs[0] = costs[1] = 0.0;
        ints[0] = ints[1] = 0;
        ints[2] = 2;
        return;
    }
    double nu, cost_in;
    pass_cost(K, in, X, uv, n, mask, part, &nu, &cost_in);
    double cur = cost_in, cr[12], jg[NLM];
    memcpy(cr, in, sizeof cr);
    int iters = 0, accepted = 0;
    if (nu >= 4.0 && max_iters > 0) {
        pass_lm(K, cr, X, uv, n, mask, part, jg);
        double lam = 1e-3;
        for (int it = 0; it < max_iters; ++it) {
            double d[6];
            if (!pr_lm_solve(jg, lam, d)) break;
            double dmax = 0.0, hmax = 1.0;
            for (int i = 0; i < 6; ++i)
                if (!(fabs(d[i]) <= dmax)) dmax = fabs(d[i]);
            for (int i = 0; i < 3; ++i)
                if (!(fabs(cr[9 + i]) <= hmax)) hmax = fabs(cr[9 + i]);
            if (!(dmax > 1e-15 * hmax)) break;
            double tr[12], jt[NLM];
            pr_update(cr, d, tr);
            pass_lm(K, tr, X, uv, n, mask, part, jt);
            ++iters;
            if (jt[NLM - 1] < cur) {
                cur = jt[NLM - 1];
                lam = lam / 10.0;
                accepted = 1;
                memcpy(cr, tr, sizeof cr);
                memcpy(jg, jt, sizeof jg);
            } else {
                lam = lam * 10.0;
            }
        }
    }
    memcpy(Rt_out, accepted ? cr : in, sizeof in);
    costs[0] = cost_in;
    costs[1] = accepted ? cur : cost_in;
    ints[0] = (int32_t)nu;
    ints[1] = iters;
    ints[2] = accepted ? 0 : 1;
}
