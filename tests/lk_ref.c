/* lk_ref.c — plain-C restatement of docs/SPEC.md S61-S66 (sparse pyramidal Lucas-Kanade tracking), written from the SPEC
 * text.  It is the checker of tests/test_track_lk_*.py and is loaded through tests/cref.py; nothing of the library includes
 * or links it.  Every stage is exported on its own: pyramid plan and level (S61), window origin / weights and window samples
 * (S62), template and normal matrix (S63), one point through the levels (S64, S65), the forward-backward rule (S66) and the
 * whole call.  Build: -O2 -ffp-contract=off (no fused operation anywhere). */
#include <math.h>
#include <stdint.h>
#include <string.h>

typedef struct lk_params {
    int32_t win_radius, max_level, max_iters;
    float eps, min_eig, fb_thresh;
    int32_t flags, reserved;
} lk_params;

#define LK_USE_INITIAL 1
#define LK_MAX_N 33                     /* 2 * 15 + 1 + 2 */

/* ---- S61 ---------------------------------------------------------------------------------------------------------------- */
static int r101(int i, int n)
{
    if (i < 0) return -i;
    if (i >= n) return 2 * n - 2 - i;
    return i;
}

/* level sizes and offsets (in pixels, tight pitch) of the pyramid of a w x h image; returns the number of levels */
int lk_pyr_plan(int w, int h, int max_level, int32_t* lw, int32_t* lh, int64_t* off)
{
    int n = 0;
    int64_t o = 0;
    for (;;) {
        lw[n] = w;
        lh[n] = h;
        off[n] = o;
        o += (int64_t)w * h;
        ++n;
        w = (w + 1) / 2;
        h = (h + 1) / 2;
        if (n > max_level || w < 16 || h < 16) break;
    }
    return n;
}

void lk_pyr_down(const uint8_t* in, int w, int h, uint8_t* out)
{
    static const int k[5] = {1, 4, 6, 4, 1};
    const int ow = (w + 1) / 2, oh = (h + 1) / 2;
    for (int y = 0; y < oh; ++y)
        for (int x = 0; x < ow; ++x) {
            int s = 0;
            for (int j = -2; j <= 2; ++j)
                for (int i = -2; i <= 2; ++i) s += k[i + 2] * k[j + 2] * in[(size_t)r101(2 * y + j, h) * w + r101(2 * x + i, w)];
            out[(size_t)y * ow + x] = (uint8_t)((s + 128) >> 8);
        }
}

/* whole pyramid into buf (tight planes at off[]); returns the number of levels */
int lk_pyr_build(const uint8_t* img, int w, int h, int stride, int max_level, uint8_t* buf, int32_t* lw, int32_t* lh, int64_t* off)
{
    const int n = lk_pyr_plan(w, h, max_level, lw, lh, off);
    for (int y = 0; y < h; ++y) memcpy(buf + (size_t)y * w, img + (size_t)y * stride, (size_t)w);
    for (int l = 1; l < n; ++l) lk_pyr_down(buf + off[l - 1], lw[l - 1], lh[l - 1], buf + off[l]);
    return n;
}

/* ---- S62 ---------------------------------------------------------------------------------------------------------------- */
/* origin and weights of a window of n x n samples with top-left (px, py); returns 1 when the window lies inside the level,
 * 0 when it leaves it (origin and weights are then written only where px, py allowed computing them) */
int lk_window_origin(float px, float py, int n, int w, int h, int32_t* ix, int32_t* iy, int32_t wt[4])
{
    if (!isfinite(px) || !isfinite(py)) return 0;
    if (fabsf(px) > 1e6f || fabsf(py) > 1e6f) return 0;
    const float fx = floorf(px), fy = floorf(py);
    const float a = px - fx, b = py - fy;
    wt[0] = (int)nearbyintf(((1.0f - a) * (1.0f - b)) * 16384.0f);
    wt[1] = (int)nearbyintf((a * (1.0f - b)) * 16384.0f);
    wt[2] = (int)nearbyintf(((1.0f - a) * b) * 16384.0f);
    wt[3] = 16384 - wt[0] - wt[1] - wt[2];
    *ix = (int)fx;
    *iy = (int)fy;
    if (*ix < 0 || *iy < 0) return 0;
    if (*ix + n > w - 1 || *iy + n > h - 1) return 0;
    return 1;
}

static int sample(const uint8_t* I, int w, int x, int y, const int32_t wt[4])
{
    const uint8_t* p = I + (size_t)y * w + x;
    return (p[0] * wt[0] + p[1] * wt[1] + p[w] * wt[2] + p[w + 1] * wt[3] + 256) >> 9;
}

/* n x n samples, row-major, into out; returns 0 when the window leaves the level (out untouched) */
int lk_sample_window(const uint8_t* I, int w, int h, float px, float py, int n, int16_t* out)
{
    int32_t ix, iy, wt[4];
    if (!lk_window_origin(px, py, n, w, h, &ix, &iy, wt)) return 0;
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) out[j * n + i] = (int16_t)sample(I, w, ix + i, iy + j, wt);
    return 1;
}

/* ---- S63 ---------------------------------------------------------------------------------------------------------------- */
/* (px, py): the point on this level.  T: (n + 2)^2 samples; gx, gy: n^2; G: Gxx, Gxy, Gyy, D, e.
 * Returns 0 = usable, 1 = the template leaves the level, 2 = flat (eigenvalue or determinant test). */
int lk_template(const uint8_t* I, int w, int h, float px, float py, int r, float min_eig, int16_t* T, int16_t* gx, int16_t* gy,
                double G[5])
{
    const int n = 2 * r + 1, m = n + 2, N = n * n;
    if (!lk_sample_window(I, w, h, px - (float)(r + 1), py - (float)(r + 1), m, T)) return 1;
    int64_t sxx = 0, sxy = 0, syy = 0;
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) {
            const int c = (j + 1) * m + (i + 1);
            const int dx = T[c + 1] - T[c - 1], dy = T[c + m] - T[c - m];
            gx[j * n + i] = (int16_t)dx;
            gy[j * n + i] = (int16_t)dy;
            sxx += (int64_t)dx * dx;
            sxy += (int64_t)dx * dy;
            syy += (int64_t)dy * dy;
        }
    const double Gxx = (double)sxx, Gxy = (double)sxy, Gyy = (double)syy;
    const double D = Gxx * Gyy - Gxy * Gxy;
    const double e = ((Gxx + Gyy) - sqrt((Gxx - Gyy) * (Gxx - Gyy) + 4.0 * (Gxy * Gxy))) / (2.0 * N * 4096.0);
    G[0] = Gxx; G[1] = Gxy; G[2] = Gyy; G[3] = D; G[4] = e;
    if (!(e >= (double)min_eig) || !(D > 0)) return 2;
    return 0;
}

/* ---- S64, S65 ----------------------------------------------------------------------------------------------------------- */
static float canon(float v)            /* a NaN is stored as the quiet NaN 0x7FC00000 */
{
    if (v != v) {
        const uint32_t q = 0x7FC00000u;
        memcpy(&v, &q, 4);
    }
    return v;
}

/* one point from pyramid A into pyramid B (both with the plan lw, lh, off, nlev); returns the status 1, 2 or 3 */
int lk_track_point(const uint8_t* A, const uint8_t* B, const int32_t* lw, const int32_t* lh, const int64_t* off, int nlev, float ptx,
                   float pty, int use_init, float inx, float iny, const lk_params* P, float out[2], float* err)
{
    const int r = P->win_radius, n = 2 * r + 1, m = n + 2, N = n * n;
    const int top = P->max_level < nlev - 1 ? P->max_level : nlev - 1;
    int16_t T[LK_MAX_N * LK_MAX_N], gx[31 * 31], gy[31 * 31], J[31 * 31];
    double G[5];
    float g0 = 0, g1 = 0;
    int status = 2;
    *err = -1.0f;
    for (int l = top; l >= 0; --l) {
        const float s = 1.0f / (float)(1 << l);
        const float px = ptx * s, py = pty * s;
        if (l == top) {
            g0 = use_init ? inx * s : px;
            g1 = use_init ? iny * s : py;
        } else {
            g0 = 2.0f * g0;
            g1 = 2.0f * g1;
        }
        const int t = lk_template(A + off[l], lw[l], lh[l], px, py, r, P->min_eig, T, gx, gy, G);
        if (t != 0) {
            if (l == 0) status = t == 1 ? 2 : 3;
            continue;
        }
        int left = 0;
        for (int it = 0; it < P->max_iters; ++it) {
            if (!lk_sample_window(B + off[l], lw[l], lh[l], g0 - (float)r, g1 - (float)r, n, J)) {
                left = 1;
                break;
            }
            int64_t bx = 0, by = 0, sa = 0;
            for (int j = 0; j < n; ++j)
                for (int i = 0; i < n; ++i) {
                    const int d = J[j * n + i] - T[(j + 1) * m + (i + 1)];
                    bx += (int64_t)d * gx[j * n + i];
                    by += (int64_t)d * gy[j * n + i];
                    sa += d < 0 ? -d : d;
                }
            if (l == 0) *err = (float)((double)sa / (32.0 * N));
            const double dx = 2.0 * (G[1] * (double)by - G[2] * (double)bx) / G[3];
            const double dy = 2.0 * (G[1] * (double)bx - G[0] * (double)by) / G[3];
            g0 = g0 + (float)dx;
            g1 = g1 + (float)dy;
            if (dx * dx + dy * dy <= (double)P->eps * (double)P->eps) break;
        }
        if (l == 0) status = left ? 2 : 1;
    }
    out[0] = canon(g0);
    out[1] = canon(g1);
    return status;
}

/* ---- S66 ---------------------------------------------------------------------------------------------------------------- */
/* the rule on a backward result: returns the status (1 or 4) and writes fb */
int lk_fb_check(float ptx, float pty, float backx, float backy, int back_status, float fb_thresh, float* fb)
{
    const float ex = backx - ptx, ey = backy - pty;
    *fb = canon(sqrtf(ex * ex + ey * ey));
    const int ok = back_status == 1 && (double)ex * (double)ex + (double)ey * (double)ey <= (double)fb_thresh * (double)fb_thresh;
    return ok ? 1 : 4;
}

/* the whole call over n points; err and fb may be NULL */
void lk_track(const uint8_t* A, const uint8_t* B, const int32_t* lw, const int32_t* lh, const int64_t* off, int nlev, const float* pts,
              int n, const float* init, const lk_params* P, float* out, uint8_t* status, float* err, float* fb)
{
    const int use_init = (P->flags & LK_USE_INITIAL) != 0;
    for (int i = 0; i < n; ++i) {
        float e = -1.0f, f = -1.0f;
        int st = lk_track_point(A, B, lw, lh, off, nlev, pts[2 * i], pts[2 * i + 1], use_init, use_init ? init[2 * i] : 0.0f,
                                use_init ? init[2 * i + 1] : 0.0f, P, out + 2 * i, &e);
        if (st == 1 && P->fb_thresh > 0) {
            float back[2], e2;
            const int bs = lk_track_point(B, A, lw, lh, off, nlev, out[2 * i], out[2 * i + 1], 0, 0.0f, 0.0f, P, back, &e2);
            st = lk_fb_check(pts[2 * i], pts[2 * i + 1], back[0], back[1], bs, P->fb_thresh, &f);
        }
        status[i] = (uint8_t)st;
        if (err) err[i] = e;
        if (fb) fb[i] = f;
    }
}

/* stable selection of the status-1 points (the gather form); returns the count */
int lk_gather(const float* pts, const float* out, const uint8_t* status, int n, float* xy1, float* xy2, int32_t* src_idx)
{
    int c = 0;
    for (int i = 0; i < n; ++i)
        if (status[i] == 1) {
            xy1[2 * c] = pts[2 * i];
            xy1[2 * c + 1] = pts[2 * i + 1];
            xy2[2 * c] = out[2 * i];
            xy2[2 * c + 1] = out[2 * i + 1];
            src_idx[c] = i;
            ++c;
        }
    return c;
}
