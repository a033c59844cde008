/* Plain-C restatement of docs/SPEC.md S85-S87 (block matching on a rectified 8-bit pair, the left-right check, the depth at
 * given points): brute force, every cost a double loop over its window, nothing shared between pixels or disparities.  The GPU
 * tests compare the library against it bit for bit; tests/test_stereo_cpu.py pins it against numpy. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define ST_INVALID (-32768)
#define ST_FROM_RIGHT 1

int st_invalid(void) { return ST_INVALID; }
int st_from_right(void) { return ST_FROM_RIGHT; }

/* S85 sub-pixel step from the three costs: floor((16 (p - n) + den) / (2 den)), 0 when den == 0 */
int st_subpixel(int p, int c, int n)
{
    const int den = p + n - 2 * c;
    int num, d2, q;
    if (den == 0) return 0;
    num = 16 * (p - n) + den;
    d2 = 2 * den;
    q = num / d2;
    if ((num % d2 != 0) && ((num < 0) != (d2 < 0))) --q;
    return q;
}

static int cost(const uint8_t* base, const uint8_t* other, int bstride, int ostride, int x, int y, int r, int shift)
{
    int i, j, sum = 0;
    for (j = -r; j <= r; ++j)
        for (i = -r; i <= r; ++i) {
            const int a = base[(size_t)(y + j) * bstride + x + i], b = other[(size_t)(y + j) * ostride + x + i + shift];
            sum += a > b ? a - b : b - a;
        }
    return sum;
}

/* S85.  disp: h rows of dstride elements, w written per row.  Returns n_valid. */
int st_bm(const uint8_t* left, const uint8_t* right, int w, int h, int lstride, int rstride, int min_disp, int num_disp, int radius,
          int uniqueness, int flags, int16_t* disp, int dstride)
{
    const int r = radius, dmin = min_disp, dmax = min_disp + num_disp - 1, from_right = (flags & ST_FROM_RIGHT) != 0;
    const uint8_t* base = from_right ? right : left;
    const uint8_t* other = from_right ? left : right;
    const int bstride = from_right ? rstride : lstride, ostride = from_right ? lstride : rstride;
    const int x0 = from_right ? r - (dmin < 0 ? dmin : 0) : r + (dmax > 0 ? dmax : 0);
    const int x1 = from_right ? w - 1 - r - (dmax > 0 ? dmax : 0) : w - 1 - r + (dmin < 0 ? dmin : 0);
    int x, y, d, n_valid = 0;
    int c[2049];
    for (y = 0; y < h; ++y)
        for (x = 0; x < w; ++x) {
            int d1, c1, have2 = 0, c2 = 0, off = 0;
            int16_t* out = disp + (size_t)y * dstride + x;
            *out = ST_INVALID;
            if (y < r || y > h - 1 - r || x < x0 || x > x1) continue;
            for (d = dmin; d <= dmax; ++d) c[d - dmin] = cost(base, other, bstride, ostride, x, y, r, from_right ? d : -d);
            d1 = dmin;
            for (d = dmin + 1; d <= dmax; ++d)
                if (c[d - dmin] < c[d1 - dmin]) d1 = d;
            c1 = c[d1 - dmin];
            for (d = dmin; d <= dmax; ++d)
                if (d - d1 > 1 || d1 - d > 1)
                    if (!have2 || c[d - dmin] < c2) {
                        c2 = c[d - dmin];
                        have2 = 1;
                    }
            if (have2 && c2 * (100 - uniqueness) < c1 * 100) continue;
            if (d1 > dmin && d1 < dmax) off = st_subpixel(c[d1 - 1 - dmin], c1, c[d1 + 1 - dmin]);
            *out = (int16_t)(16 * d1 + off);
            ++n_valid;
        }
    return n_valid;
}

/* S86, in place on the left map.  Returns n_valid afterwards. */
int st_lr_check(int16_t* left, const int16_t* right, int w, int h, int lstride, int rstride, int max_diff16)
{
    int x, y, n_valid = 0;
    for (y = 0; y < h; ++y)
        for (x = 0; x < w; ++x) {
            int16_t* p = left + (size_t)y * lstride + x;
            const int v = *p;
            int xr, vr, diff;
            if (v == ST_INVALID) continue;
            xr = x - (int)floor((v + 8) / 16.0);
            *p = ST_INVALID;
            if (xr < 0 || xr >= w) continue;
            vr = right[(size_t)y * rstride + xr];
            if (vr == ST_INVALID) continue;
            diff = v > vr ? v - vr : vr - v;
            if (diff > max_diff16) continue;
            *p = (int16_t)v;
            ++n_valid;
        }
    return n_valid;
}

/* S87.  K = (fx, fy, cx, cy); R: 9 doubles or NULL; xyz: n rows of three floats. */
void st_points(const int16_t* disp, int w, int h, int dstride, const double* K, double baseline, const double* R, const float* pts, int n,
               float* xyz)
{
    const double fx = K[0], fy = K[1], cx = K[2], cy = K[3];
    const double fb16 = (fx * baseline) * 16.0;
    const uint32_t qnan = 0x7FC00000u;
    int i, k;
    for (i = 0; i < n; ++i) {
        const double x = (double)pts[2 * i], y = (double)pts[2 * i + 1];
        float* o = xyz + 3 * (size_t)i;
        double xi, yi, X, Y, Z;
        int v;
        for (k = 0; k < 3; ++k) memcpy(o + k, &qnan, 4);
        if (!isfinite(x) || !isfinite(y)) continue;
        xi = floor(x + 0.5);
        yi = floor(y + 0.5);
        if (!(xi >= 0.0 && xi < (double)w && yi >= 0.0 && yi < (double)h)) continue;
        v = disp[(size_t)(int)yi * dstride + (int)xi];
        if (v == ST_INVALID || v <= 0) continue;
        Z = fb16 / (double)v;
        X = ((x - cx) / fx) * Z;
        Y = ((y - cy) / fy) * Z;
        if (R) {
            o[0] = (float)((R[0] * X + R[3] * Y) + R[6] * Z);
            o[1] = (float)((R[1] * X + R[4] * Y) + R[7] * Z);
            o[2] = (float)((R[2] * X + R[5] * Y) + R[8] * Z);
        } else {
            o[0] = (float)X;
            o[1] = (float)Y;
            o[2] = (float)Z;
        }
    }
}
