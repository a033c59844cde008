/* homography_ref.c — plain-C restatement of docs/SPEC.md S19-S22 (robust homography), test infrastructure only.
 * tests/test_homography_cpu.py builds it with `cc -O2 -ffp-contract=off -shared -fPIC` and loads it with ctypes;
 * tests/test_homography_gpu.py compares the HIP kernel with it bit for bit.  Every fused multiply-add is an explicit
 * fma()/fmaf() call, exactly where the SPEC names one. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define COLLINEAR_EPS 1e-4

static uint64_t mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

/* S19 */
void hr_sample4(uint64_t seed, uint64_t h, int n, int idx[4])
{
    const uint64_t stream = mix64(seed ^ 0x4A7C159E3779B97FULL) ^ mix64(h + 0xD1B54A32D192ED03ULL);
    int cnt = 0;
    for (uint64_t d = 0; d < 64 && cnt < 4; ++d) {
        const uint64_t r = mix64(stream + (d + 1) * 0x9E3779B97F4A7C15ULL);
        const int c = (int)(((r >> 32) * (uint64_t)(uint32_t)n) >> 32);
        int rep = 0;
        for (int s = 0; s < cnt; ++s) rep |= idx[s] == c;
        if (!rep) idx[cnt++] = c;
    }
    for (int c = 0; cnt < 4; ++c) {
        int rep = 0;
        for (int s = 0; s < cnt; ++s) rep |= idx[s] == c;
        if (!rep) idx[cnt++] = c;
    }
}

/* S20 step 1 */
static int hartley4(const double px[4], const double py[4], double nx[4], double ny[4], double* s, double* tx, double* ty)
{
    double cx = px[0], cy = py[0], md = 0.0;
    for (int i = 1; i < 4; ++i) { cx = cx + px[i]; cy = cy + py[i]; }
    cx = cx * 0.25; cy = cy * 0.25;
    for (int i = 0; i < 4; ++i) {
        const double dx = px[i] - cx, dy = py[i] - cy;
        md = md + sqrt(fma(dx, dx, dy * dy));
    }
    md = md * 0.25;
    if (!(md > 0.0) || !(md < INFINITY)) return 0;
    *s = 1.4142135623730951 / md;
    for (int i = 0; i < 4; ++i) { nx[i] = (px[i] - cx) * *s; ny[i] = (py[i] - cy) * *s; }
    *tx = -(*s * cx); *ty = -(*s * cy);
    return 1;
}

static double cross3(const double x[4], const double y[4], int a, int b, int c)
{
    return (x[b] - x[a]) * (y[c] - y[a]) - (y[b] - y[a]) * (x[c] - x[a]);
}

/* S20 step 2: 1 = valid sample */
static int sample_ok(const double ax[4], const double ay[4], const double bx[4], const double by[4])
{
    static const int tri[4][3] = {{0, 1, 2}, {0, 1, 3}, {0, 2, 3}, {1, 2, 3}};
    int same[4];
    for (int t = 0; t < 4; ++t) {
        const double c1 = cross3(ax, ay, tri[t][0], tri[t][1], tri[t][2]);
        const double c2 = cross3(bx, by, tri[t][0], tri[t][1], tri[t][2]);
        if (!(fabs(c1) > COLLINEAR_EPS) || !(fabs(c2) > COLLINEAR_EPS)) return 0;
        same[t] = (c1 > 0.0) == (c2 > 0.0);
    }
    return same[0] == same[1] && same[0] == same[2] && same[0] == same[3];
}

/* S20: 1 = valid; H = 0 otherwise */
int hr_solve4(const double x1[4], const double y1[4], const double x2[4], const double y2[4], double H[9])
{
    double ax[4], ay[4], bx[4], by[4], s1, t1x, t1y, s2, t2x, t2y, B[9][8], beta[8], f[9], M[3][3], Ho[9];
    for (int i = 0; i < 9; ++i) H[i] = 0.0;
    if (!hartley4(x1, y1, ax, ay, &s1, &t1x, &t1y)) return 0;
    if (!hartley4(x2, y2, bx, by, &s2, &t2x, &t2y)) return 0;
    if (!sample_ok(ax, ay, bx, by)) return 0;
    /* step 3: B = A^T, columns 2c, 2c+1 = the two constraint rows of correspondence c */
    for (int c = 0; c < 4; ++c) {
        const double rk[9] = {-ax[c], -ay[c], -1.0, 0.0, 0.0, 0.0, bx[c] * ax[c], bx[c] * ay[c], bx[c]};
        const double rl[9] = {0.0, 0.0, 0.0, -ax[c], -ay[c], -1.0, by[c] * ax[c], by[c] * ay[c], by[c]};
        for (int i = 0; i < 9; ++i) { B[i][2 * c] = rk[i]; B[i][2 * c + 1] = rl[i]; }
    }
    /* step 4: S7 step 3's Householder QR and null vector */
    for (int j = 0; j < 8; ++j) {
        double sigma = 0.0;
        for (int i = j + 1; i < 9; ++i) sigma = fma(B[i][j], B[i][j], sigma);
        const double alpha = B[j][j];
        const double nrm = sqrt(fma(alpha, alpha, sigma));
        if (!(nrm > 0.0)) { beta[j] = 0.0; continue; }
        const double v0 = alpha + (alpha >= 0.0 ? nrm : -nrm);
        beta[j] = 2.0 / fma(v0, v0, sigma);
        B[j][j] = v0;
        for (int c = j + 1; c < 8; ++c) {
            double dot = v0 * B[j][c];
            for (int i = j + 1; i < 9; ++i) dot = fma(B[i][j], B[i][c], dot);
            const double w = beta[j] * dot;
            B[j][c] = fma(-w, v0, B[j][c]);
            for (int i = j + 1; i < 9; ++i) B[i][c] = fma(-w, B[i][j], B[i][c]);
        }
    }
    for (int i = 0; i < 8; ++i) f[i] = 0.0;
    f[8] = 1.0;
    for (int j = 7; j >= 0; --j) {
        if (beta[j] == 0.0) continue;
        double dot = B[j][j] * f[j];
        for (int i = j + 1; i < 9; ++i) dot = fma(B[i][j], f[i], dot);
        const double w = beta[j] * dot;
        f[j] = fma(-w, B[j][j], f[j]);
        for (int i = j + 1; i < 9; ++i) f[i] = fma(-w, B[i][j], f[i]);
    }
    /* step 5: H ~ (s2 T2^-1) Hn T1 */
    for (int i = 0; i < 3; ++i) {
        M[i][0] = f[3 * i] * s1;
        M[i][1] = f[3 * i + 1] * s1;
        M[i][2] = fma(f[3 * i], t1x, fma(f[3 * i + 1], t1y, f[3 * i + 2]));
    }
    const double u2x = -t2x, u2y = -t2y;
    for (int j = 0; j < 3; ++j) {
        Ho[j] = fma(u2x, M[2][j], M[0][j]);
        Ho[3 + j] = fma(u2y, M[2][j], M[1][j]);
        Ho[6 + j] = s2 * M[2][j];
    }
    /* step 6 */
    double ss = 0.0;
    for (int i = 0; i < 9; ++i) ss = fma(Ho[i], Ho[i], ss);
    const double nrm = sqrt(ss);
    if (!(nrm > 0.0) || !(nrm < INFINITY)) return 0;
    double inv = 1.0 / nrm;
    if (Ho[8] < 0.0) inv = -inv;
    for (int i = 0; i < 9; ++i) H[i] = Ho[i] * inv;
    return 1;
}

/* S19 + S20 for hypothesis h of (xy1, xy2), n >= 4 */
int hr_model(const float* xy1, const float* xy2, int n, uint64_t seed, uint64_t h, double H[9])
{
    int idx[4];
    double x1[4], y1[4], x2[4], y2[4];
    hr_sample4(seed, h, n, idx);
    for (int i = 0; i < 4; ++i) {
        x1[i] = (double)xy1[2 * idx[i]]; y1[i] = (double)xy1[2 * idx[i] + 1];
        x2[i] = (double)xy2[2 * idx[i]]; y2[i] = (double)xy2[2 * idx[i] + 1];
    }
    return hr_solve4(x1, y1, x2, y2, H);
}

/* S21 */
int hr_inlier(const float h[9], float x, float y, float xp, float yp, float thr2)
{
    const float u = fmaf(h[0], x, fmaf(h[1], y, h[2]));
    const float v = fmaf(h[3], x, fmaf(h[4], y, h[5]));
    const float w = fmaf(h[6], x, fmaf(h[7], y, h[8]));
    const float du = fmaf(-xp, w, u);
    const float dv = fmaf(-yp, w, v);
    const float rhs = thr2 * (w * w);
    return (fmaf(du, du, dv * dv) <= rhs) && (rhs > 0.f) && (rhs < INFINITY);
}

/* S21 over all n with the f32 rounding of H; mask may be NULL; returns the inlier count */
int hr_score(const double H[9], const float* xy1, const float* xy2, int n, float thresh_px, uint8_t* mask)
{
    float h[9];
    const float thr2 = thresh_px * thresh_px;
    int c = 0;
    for (int i = 0; i < 9; ++i) h[i] = (float)H[i];
    for (int i = 0; i < n; ++i) {
        const int in = hr_inlier(h, xy1[2 * i], xy1[2 * i + 1], xy2[2 * i], xy2[2 * i + 1], thr2);
        if (mask) mask[i] = (uint8_t)in;
        c += in;
    }
    return c;
}

/* S22: the whole run over ids [hb, he); returns the winner's key (0: no valid model, H = 0, mask = 0) */
uint64_t hr_run(const float* xy1, const float* xy2, int n, uint64_t seed, int64_t hb, int64_t he, float thresh_px,
                double H[9], uint8_t* mask, int* n_inliers)
{
    uint64_t best = 0;
    double Hh[9];
    for (int i = 0; i < 9; ++i) H[i] = 0.0;
    if (mask) memset(mask, 0, (size_t)n);
    *n_inliers = 0;
    if (n < 4) return 0;
    for (int64_t h = hb; h < he; ++h) {
        if (!hr_model(xy1, xy2, n, seed, (uint64_t)h, Hh)) continue;
        const uint64_t c = (uint64_t)(uint32_t)hr_score(Hh, xy1, xy2, n, thresh_px, NULL);
        const uint64_t key = (c << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)h);
        if (key > best) { best = key; memcpy(H, Hh, sizeof Hh); }
    }
    if (best) *n_inliers = hr_score(H, xy1, xy2, n, thresh_px, mask);
    return best;
}
