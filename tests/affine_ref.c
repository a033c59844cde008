/* affine_ref.c — plain-C restatement of docs/SPEC.md S26-S30 (robust 2D affine and similarity estimation and the
 * least-squares refit on the inliers), test infrastructure only.  tests/affine_ref.py builds it with
 * `cc -O2 -ffp-contract=off -shared -fPIC` and loads it with ctypes; tests/test_affine_gpu.py compares the HIP kernels
 * with it bit for bit.  Every fused multiply-add is an explicit fma()/fmaf() call, exactly where the SPEC names one.
 * model: 0 = full (6 DOF, 3-point samples), 1 = partial (4 DOF, 2-point samples).  A: 6 doubles, 2 x 3 row-major. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define P 512

static uint64_t mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

int ar_min_pts(int model) { return model == 0 ? 3 : 2; }

/* S26 */
void ar_sample(int model, uint64_t seed, uint64_t h, int n, int* idx)
{
    const int k = ar_min_pts(model);
    const uint64_t key = model == 0 ? 0x79B97F4A7C159E37ULL : 0x7C159E3779B97F4AULL;
    const uint64_t stream = mix64(seed ^ key) ^ mix64(h + 0xD1B54A32D192ED03ULL);
    int cnt = 0;
    for (uint64_t d = 0; d < 64 && cnt < k; ++d) {
        const uint64_t r = mix64(stream + (d + 1) * 0x9E3779B97F4A7C15ULL);
        const int c = (int)(((r >> 32) * (uint64_t)(uint32_t)n) >> 32);
        int rep = 0;
        for (int s = 0; s < cnt; ++s) rep |= idx[s] == c;
        if (!rep) idx[cnt++] = c;
    }
    for (int c = 0; cnt < k; ++c) {
        int rep = 0;
        for (int s = 0; s < cnt; ++s) rep |= idx[s] == c;
        if (!rep) idx[cnt++] = c;
    }
}

static int finite6(const double a[6])
{
    for (int i = 0; i < 6; ++i)
        if (!(fabs(a[i]) < INFINITY)) return 0;
    return 1;
}

/* S27 sample check of one image (haveCollinearPoints) */
static int spread3(double det, double dx1, double dy1, double dx2, double dy2)
{
    const double eps = 1.1920928955078125e-07;   /* FLT_EPSILON */
    return fabs(det) > eps * (((fabs(dx1) + fabs(dy1)) + fabs(dx2)) + fabs(dy2));
}

/* S27: minimal solve of MIN_PTS points (arrays of 3 or 2); 1 = valid (A set), 0 = invalid (A = 0) */
int ar_solve(int model, const double* x1, const double* y1, const double* x2, const double* y2, double A[6])
{
    double a[6];
    for (int i = 0; i < 6; ++i) A[i] = 0.0;
    if (model == 0) {
        const double dx1 = x1[1] - x1[0], dy1 = y1[1] - y1[0], dx2 = x1[2] - x1[0], dy2 = y1[2] - y1[0];
        const double e1 = x2[1] - x2[0], f1 = y2[1] - y2[0], e2 = x2[2] - x2[0], f2 = y2[2] - y2[0];
        const double det = dx1 * dy2 - dy1 * dx2;
        const double det2 = e1 * f2 - f1 * e2;
        if (!spread3(det, dx1, dy1, dx2, dy2) || !spread3(det2, e1, f1, e2, f2)) return 0;
        const double idet = 1.0 / det;
        a[0] = (e1 * dy2 - e2 * dy1) * idet;
        a[1] = (dx1 * e2 - dx2 * e1) * idet;
        a[2] = x2[0] - fma(a[0], x1[0], a[1] * y1[0]);
        a[3] = (f1 * dy2 - f2 * dy1) * idet;
        a[4] = (dx1 * f2 - dx2 * f1) * idet;
        a[5] = y2[0] - fma(a[3], x1[0], a[4] * y1[0]);
    } else {
        const double dx = x1[1] - x1[0], dy = y1[1] - y1[0], ex = x2[1] - x2[0], ey = y2[1] - y2[0];
        const double q = fma(dx, dx, dy * dy);
        if (!(q > 0.0) || !(q < INFINITY) || !(fma(ex, ex, ey * ey) > 0.0)) return 0;
        const double iq = 1.0 / q;
        const double s = fma(ex, dx, ey * dy) * iq;
        const double b = fma(ey, dx, -(ex * dy)) * iq;
        a[0] = s; a[1] = -b; a[2] = x2[0] - fma(s, x1[0], -(b * y1[0]));
        a[3] = b; a[4] = s;  a[5] = y2[0] - fma(b, x1[0], s * y1[0]);
    }
    if (!finite6(a)) return 0;
    memcpy(A, a, sizeof a);
    return 1;
}

/* S26 + S27 for hypothesis h of (xy1, xy2), n >= MIN_PTS */
int ar_model(int model, const float* xy1, const float* xy2, int n, uint64_t seed, uint64_t h, double A[6])
{
    int idx[3];
    double x1[3], y1[3], x2[3], y2[3];
    ar_sample(model, seed, h, n, idx);
    for (int i = 0; i < ar_min_pts(model); ++i) {
        x1[i] = (double)xy1[2 * idx[i]]; y1[i] = (double)xy1[2 * idx[i] + 1];
        x2[i] = (double)xy2[2 * idx[i]]; y2[i] = (double)xy2[2 * idx[i] + 1];
    }
    return ar_solve(model, x1, y1, x2, y2, A);
}

/* S28 */
int ar_inlier(const float a[6], float x, float y, float xp, float yp, float thr2)
{
    const float u = fmaf(a[0], x, fmaf(a[1], y, a[2]));
    const float v = fmaf(a[3], x, fmaf(a[4], y, a[5]));
    const float du = u - xp, dv = v - yp;
    return (fmaf(du, du, dv * dv) <= thr2) && (thr2 > 0.f) && (thr2 < INFINITY);
}

/* S28 over all n with the f32 rounding of A; mask may be NULL; returns the inlier count */
int ar_score(const double A[6], const float* xy1, const float* xy2, int n, float thresh_px, uint8_t* mask)
{
    float a[6];
    const float thr2 = thresh_px * thresh_px;
    int c = 0;
    for (int i = 0; i < 6; ++i) a[i] = (float)A[i];
    for (int i = 0; i < n; ++i) {
        const int in = ar_inlier(a, xy1[2 * i], xy1[2 * i + 1], xy2[2 * i], xy2[2 * i + 1], thr2);
        if (mask) mask[i] = (uint8_t)in;
        c += in;
    }
    return c;
}

/* S29: the whole run over ids [hb, he); returns the winner's key (0: no valid model, A = 0, mask = 0) */
uint64_t ar_run(int model, const float* xy1, const float* xy2, int n, uint64_t seed, int64_t hb, int64_t he,
                float thresh_px, double A[6], uint8_t* mask, int* n_inliers)
{
    uint64_t best = 0;
    double Ah[6];
    for (int i = 0; i < 6; ++i) A[i] = 0.0;
    if (mask) memset(mask, 0, (size_t)n);
    *n_inliers = 0;
    if (n < ar_min_pts(model)) return 0;
    for (int64_t h = hb; h < he; ++h) {
        if (!ar_model(model, xy1, xy2, n, seed, (uint64_t)h, Ah)) continue;
        const uint64_t c = (uint64_t)(uint32_t)ar_score(Ah, xy1, xy2, n, thresh_px, NULL);
        const uint64_t key = (c << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)h);
        if (key > best) { best = key; memcpy(A, Ah, sizeof Ah); }
    }
    if (best) *n_inliers = ar_score(A, xy1, xy2, n, thresh_px, mask);
    return best;
}

/* ---- S30 ---------------------------------------------------------------------------------------------------------- */

static double cost_term(const double a[6], double x, double y, double xp, double yp)
{
    const double ru = fma(a[0], x, fma(a[1], y, a[2])) - xp;
    const double rv = fma(a[3], x, fma(a[4], y, a[5])) - yp;
    return fma(ru, ru, rv * rv);
}

/* S23's fixed order: partial i mod P in ascending i (inliers only), then the stride-halving tree */
typedef void (*term_fn)(double* acc, const double* ctx, double x1, double y1, double x2, double y2);

static void reduce(const float* xy1, const float* xy2, int n, const uint8_t* mask, int k, term_fn term,
                   const double* ctx, double* out)
{
    static double part[P][8];
    memset(part, 0, sizeof part);
    for (int i = 0; i < n; ++i) {
        if (!mask[i]) continue;
        term(part[i % P], ctx, (double)xy1[2 * i], (double)xy1[2 * i + 1], (double)xy2[2 * i], (double)xy2[2 * i + 1]);
    }
    for (int s = P / 2; s >= 1; s >>= 1)
        for (int p = 0; p < s; ++p)
            for (int j = 0; j < k; ++j) part[p][j] = part[p][j] + part[p + s][j];
    for (int j = 0; j < k; ++j) out[j] = part[0][j];
}

static void term1(double* a, const double* c, double x1, double y1, double x2, double y2)
{
    a[0] = a[0] + 1.0;
    a[1] = a[1] + x1; a[2] = a[2] + y1; a[3] = a[3] + x2; a[4] = a[4] + y2;
    a[5] = a[5] + cost_term(c, x1, y1, x2, y2);
}

/* c = (cx1, cy1, cx2, cy2) */
static void term2_full(double* a, const double* c, double x1, double y1, double x2, double y2)
{
    const double dx = x1 - c[0], dy = y1 - c[1], ex = x2 - c[2], ey = y2 - c[3];
    a[0] = a[0] + dx * dx; a[1] = a[1] + dx * dy; a[2] = a[2] + dy * dy;
    a[3] = a[3] + dx * ex; a[4] = a[4] + dy * ex; a[5] = a[5] + dx * ey; a[6] = a[6] + dy * ey;
}

static void term2_partial(double* a, const double* c, double x1, double y1, double x2, double y2)
{
    const double dx = x1 - c[0], dy = y1 - c[1], ex = x2 - c[2], ey = y2 - c[3];
    a[0] = a[0] + fma(dx, dx, dy * dy);
    a[1] = a[1] + fma(dx, ex, dy * ey);
    a[2] = a[2] + fma(dx, ey, -(dy * ex));
}

static void term3(double* a, const double* c, double x1, double y1, double x2, double y2)
{
    a[0] = a[0] + cost_term(c, x1, y1, x2, y2);
}

/* S30: the refit; A_out may alias A_in.  info = (cost_in, cost_out), ints = (n_used, status).  Returns the status. */
int ar_refine(int model, const float* xy1, const float* xy2, int n, const uint8_t* mask, const double A_in[6],
              double A_out[6], double costs[2], int ints[2])
{
    double ain[6], s[8], aref[6];
    memcpy(ain, A_in, sizeof ain);
    int zero = 1;
    for (int i = 0; i < 6; ++i) zero = zero && ain[i] == 0.0;
    if (zero) {
        memcpy(A_out, ain, sizeof ain);
        costs[0] = costs[1] = 0.0;
        ints[0] = 0; ints[1] = 2;
        return 2;
    }
    reduce(xy1, xy2, n, mask, 6, term1, ain, s);
    const double nu = s[0], cost_in = s[5];
    const double c[4] = {s[1] / nu, s[2] / nu, s[3] / nu, s[4] / nu};
    int ok_ref = 0;
    if (nu >= (double)ar_min_pts(model)) {
        if (model == 0) {
            reduce(xy1, xy2, n, mask, 7, term2_full, c, s);
            const double sxx = s[0], sxy = s[1], syy = s[2], sxe = s[3], sye = s[4], sxf = s[5], syf = s[6];
            const double det = sxx * syy - sxy * sxy;
            if (det > 1e-12 * (sxx * syy) && det < INFINITY) {
                const double idet = 1.0 / det;
                aref[0] = (sxe * syy - sye * sxy) * idet;
                aref[1] = (sxx * sye - sxy * sxe) * idet;
                aref[2] = c[2] - fma(aref[0], c[0], aref[1] * c[1]);
                aref[3] = (sxf * syy - syf * sxy) * idet;
                aref[4] = (sxx * syf - sxy * sxf) * idet;
                aref[5] = c[3] - fma(aref[3], c[0], aref[4] * c[1]);
                ok_ref = 1;
            }
        } else {
            reduce(xy1, xy2, n, mask, 3, term2_partial, c, s);
            const double q = s[0];
            if (q > 0.0 && q < INFINITY) {
                const double a = s[1] / q, b = s[2] / q;
                aref[0] = a; aref[1] = -b; aref[2] = c[2] - fma(a, c[0], -(b * c[1]));
                aref[3] = b; aref[4] = a;  aref[5] = c[3] - fma(b, c[0], a * c[1]);
                ok_ref = 1;
            }
        }
    }
    double cost_out = cost_in;
    int accepted = 0;
    if (ok_ref) {
        reduce(xy1, xy2, n, mask, 1, term3, aref, s);
        if (s[0] <= cost_in) { cost_out = s[0]; accepted = 1; }
    }
    memcpy(A_out, accepted ? aref : ain, sizeof ain);
    costs[0] = cost_in; costs[1] = cost_out;
    ints[0] = (int)nu; ints[1] = accepted ? 0 : 1;
    return ints[1];
}
