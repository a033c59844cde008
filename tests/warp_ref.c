/* warp_ref.c — plain-C restatement of docs/SPEC.md S75-S78: warping an 8-bit image by a 3 x 3 (or lifted 2 x 3) model with
 * integer bilinear sampling at 1/32 pixel, and the point transform.  One pixel, one point at a time, nothing shared between
 * them; built by tests/cref.py with -ffp-contract=off, so every product and sum below is its own rounding. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define WARP_INVERT 1
#define WARP_REPLICATE 2
#define WARP_AFFINE 4

/* S75: m[9] = the matrix the positions use; returns 0 usable, 1 singular or non-finite, 2 the zero model. */
int warp_model(const double* M, int flags, double m[9])
{
    double a[9];
    int n = (flags & WARP_AFFINE) ? 6 : 9, finite = 1, zero = 1, i;
    for (i = 0; i < 9; ++i) a[i] = i < n ? M[i] : (i == 8 ? 1.0 : 0.0);
    for (i = 0; i < n; ++i) {
        if (!isfinite(a[i])) finite = 0;
        if (a[i] != 0.0) zero = 0;
    }
    {
        const double c0 = a[4] * a[8] - a[5] * a[7], c1 = a[5] * a[6] - a[3] * a[8], c2 = a[3] * a[7] - a[4] * a[6];
        const double det = (a[0] * c0 + a[1] * c1) + a[2] * c2;
        if (flags & WARP_INVERT) {
            m[0] = c0;
            m[1] = a[2] * a[7] - a[1] * a[8];
            m[2] = a[1] * a[5] - a[2] * a[4];
            m[3] = c1;
            m[4] = a[0] * a[8] - a[2] * a[6];
            m[5] = a[2] * a[3] - a[0] * a[5];
            m[6] = c2;
            m[7] = a[1] * a[6] - a[0] * a[7];
            m[8] = a[0] * a[4] - a[1] * a[3];
        } else {
            memcpy(m, a, sizeof a);
        }
        if (zero) return 2;
        if (!finite || det == 0.0 || !isfinite(det)) return 1;
    }
    return 0;
}

/* S76: the Q5 position of output pixel (x, y); 0 = outside. */
int warp_position(const double m[9], int x, int y, int32_t* qx, int32_t* qy)
{
    const double dx = (double)x, dy = (double)y;
    const double X = (m[0] * dx + m[1] * dy) + m[2];
    const double Y = (m[3] * dx + m[4] * dy) + m[5];
    const double W = (m[6] * dx + m[7] * dy) + m[8];
    double r, fx, fy;
    if (W == 0.0) return 0;
    r = 32.0 / W;
    fx = X * r;
    fy = Y * r;
    if (!isfinite(fx) || !isfinite(fy)) return 0;
    if (fabs(fx) >= 1073741824.0 || fabs(fy) >= 1073741824.0) return 0;
    *qx = (int32_t)rint(fx);
    *qy = (int32_t)rint(fy);
    return 1;
}

static int32_t floor_shift5(int32_t q) { return q >= 0 ? q / 32 : -((31 - q) / 32); }      /* q >> 5 without relying on it */

/* S77: the grey value at the Q5 position; *ok = every tap of non-zero weight lies inside the source. */
int warp_sample(const uint8_t* src, int sw, int sh, int sstride, int32_t qx, int32_t qy, int replicate, int border, int* ok)
{
    const int32_t x0 = floor_shift5(qx), y0 = floor_shift5(qy);
    const int ax = (int)(qx - 32 * x0), ay = (int)(qy - 32 * y0);
    const int wx[2] = {32 - ax, ax}, wy[2] = {32 - ay, ay};
    int sum = 0, i, j;
    *ok = 1;
    for (j = 0; j < 2; ++j)
        for (i = 0; i < 2; ++i) {
            const int wgt = wx[i] * wy[j];
            int xx = x0 + i, yy = y0 + j, in, v;
            if (wgt == 0) continue;
            in = xx >= 0 && xx < sw && yy >= 0 && yy < sh;
            if (!in) *ok = 0;
            if (replicate) {
                xx = xx < 0 ? 0 : (xx > sw - 1 ? sw - 1 : xx);
                yy = yy < 0 ? 0 : (yy > sh - 1 ? sh - 1 : yy);
                v = src[(size_t)yy * sstride + xx];
            } else {
                v = in ? src[(size_t)yy * sstride + xx] : border;
            }
            sum += wgt * v;
        }
    return (sum + 512) >> 10;
}

/* The whole call: dst (dh rows of dstride bytes, dw written), valid (dw x dh, may be NULL), info[2] = status, n_valid (may be
 * NULL).  Returns the status. */
int warp_image(const uint8_t* src, int sw, int sh, int sstride, const double* M, int flags, int border, uint8_t* dst, int dw, int dh,
               int dstride, uint8_t* valid, int32_t* info)
{
    double m[9];
    const int status = warp_model(M, flags, m);
    int32_t n_valid = 0;
    int x, y;
    for (y = 0; y < dh; ++y)
        for (x = 0; x < dw; ++x) {
            int32_t qx, qy;
            int out = border, ok = 0;
            if (status == 0 && warp_position(m, x, y, &qx, &qy))
                out = warp_sample(src, sw, sh, sstride, qx, qy, (flags & WARP_REPLICATE) != 0, border, &ok);
            dst[(size_t)y * dstride + x] = (uint8_t)out;
            if (valid) valid[(size_t)y * dw + x] = (uint8_t)ok;
            n_valid += ok;
        }
    if (info) {
        info[0] = status;
        info[1] = n_valid;
    }
    return status;
}

/* S78: out may be pts. */
void warp_points(const double* M, int flags, const float* pts, int n, float* out)
{
    double m[9];
    const int status = warp_model(M, flags, m);
    int i;
    for (i = 0; i < n; ++i) {
        const double x = (double)pts[2 * i], y = (double)pts[2 * i + 1];
        const double X = (m[0] * x + m[1] * y) + m[2];
        const double Y = (m[3] * x + m[4] * y) + m[5];
        const double W = (m[6] * x + m[7] * y) + m[8];
        const double qx = X / W, qy = Y / W;
        if (status != 0 || W == 0.0 || !isfinite(qx) || !isfinite(qy)) {
            out[2 * i] = out[2 * i + 1] = NAN;
        } else {
            out[2 * i] = (float)qx;
            out[2 * i + 1] = (float)qy;
        }
    }
}
