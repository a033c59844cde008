/* undistort_ref.c — plain-C restatement of docs/SPEC.md S79-S83: the 5-coefficient lens model, points through it both ways,
 * the Q5 source position of an undistorted pixel, the map, the remap and the fused image.  One pixel, one point at a time,
 * nothing shared between them; built by tests/cref.py with -ffp-contract=off, so every product and sum below is its own
 * rounding.  cam = {fx, fy, cx, cy}; lens = {k1, k2, p1, p2, k3} or NULL (all zero); R = 9 doubles row-major or NULL (the
 * rotation step is skipped); ncam = the new camera or NULL (= cam). */
#include <math.h>
#include <stdint.h>
#include <string.h>

static const double ZERO_LENS[5] = {0.0, 0.0, 0.0, 0.0, 0.0};

/* S79 on normalised (x, y): out = {xd, yd, rad} */
void und_forward_norm(const double* lens, double x, double y, double out[3])
{
    const double k1 = lens[0], k2 = lens[1], p1 = lens[2], p2 = lens[3], k3 = lens[4];
    const double xx = x * x, yy = y * y, r2 = xx + yy;
    const double rad = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2;
    const double dX = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * xx);
    const double dY = p1 * (r2 + 2.0 * yy) + 2.0 * p2 * x * y;
    out[0] = x * rad + dX;
    out[1] = y * rad + dY;
    out[2] = rad;
}

/* S79 whole: normalised (x, y) -> pixel (u, v) under cam; returns rad */
double und_forward(const double* cam, const double* lens, double x, double y, double uv[2])
{
    double o[3];
    und_forward_norm(lens ? lens : ZERO_LENS, x, y, o);
    uv[0] = cam[0] * o[0] + cam[2];
    uv[1] = cam[1] * o[1] + cam[3];
    return o[2];
}

/* S80 in fp64, unrounded: ideal pixel (u, v) under ncam -> distorted pixel under cam; 0 = no position */
int und_source_position(const double* cam, const double* lens, const double* R, const double* ncam, double u, double v, double out[2])
{
    const double* nc = ncam ? ncam : cam;
    const double ifx = 1.0 / nc[0], ify = 1.0 / nc[1];
    double x = (u - nc[2]) * ifx, y = (v - nc[3]) * ify, rad;
    if (R) {
        const double X = (R[0] * x + R[3] * y) + R[6];
        const double Y = (R[1] * x + R[4] * y) + R[7];
        const double Z = (R[2] * x + R[5] * y) + R[8];
        double iz;
        if (!(Z > 0.0)) return 0;
        iz = 1.0 / Z;
        x = X * iz;
        y = Y * iz;
    }
    rad = und_forward(cam, lens, x, y, out);
    if (!(rad > 0.0)) return 0;
    return isfinite(out[0]) && isfinite(out[1]);
}

/* S80: out may be pts */
void und_distort_points(const double* cam, const double* lens, const double* R, const double* ncam, const float* pts, int n, float* out)
{
    int i;
    for (i = 0; i < n; ++i) {
        double s[2];
        if (und_source_position(cam, lens, R, ncam, (double)pts[2 * i], (double)pts[2 * i + 1], s)) {
            out[2 * i] = (float)s[0];
            out[2 * i + 1] = (float)s[1];
        } else {
            out[2 * i] = out[2 * i + 1] = NAN;
        }
    }
}

/* S81: out may be pts */
void und_undistort_points(const double* cam, const double* lens, const double* R, const double* ncam, int iters, double tol_px, const float* pts,
                          int n, float* out)
{
    const double* nc = ncam ? ncam : cam;
    const double* l = lens ? lens : ZERO_LENS;
    const double ifx = 1.0 / cam[0], ify = 1.0 / cam[1], tol2 = tol_px * tol_px;
    int i, it;
    for (i = 0; i < n; ++i) {
        const double x0 = ((double)pts[2 * i] - cam[2]) * ifx, y0 = ((double)pts[2 * i + 1] - cam[3]) * ify;
        double x = x0, y = y0, o[3], ex, ey, u, v;
        int ok;
        for (it = 0; it < iters; ++it) {
            const double xx = x * x, yy = y * y, r2 = xx + yy;
            const double ic = 1.0 / (1.0 + ((l[4] * r2 + l[1]) * r2 + l[0]) * r2);
            const double dX = 2.0 * l[2] * x * y + l[3] * (r2 + 2.0 * xx);
            const double dY = l[2] * (r2 + 2.0 * yy) + 2.0 * l[3] * x * y;
            x = (x0 - dX) * ic;
            y = (y0 - dY) * ic;
        }
        und_forward_norm(l, x, y, o);
        ex = cam[0] * (o[0] - x0);
        ey = cam[1] * (o[1] - y0);
        ok = o[2] > 0.0 && ex * ex + ey * ey <= tol2;
        if (R) {
            const double X = (R[0] * x + R[1] * y) + R[2];
            const double Y = (R[3] * x + R[4] * y) + R[5];
            const double Z = (R[6] * x + R[7] * y) + R[8];
            const double iz = 1.0 / Z;
            ok = ok && Z > 0.0;
            x = X * iz;
            y = Y * iz;
        }
        u = nc[0] * x + nc[2];
        v = nc[1] * y + nc[3];
        if (ok && isfinite(u) && isfinite(v)) {
            out[2 * i] = (float)u;
            out[2 * i + 1] = (float)v;
        } else {
            out[2 * i] = out[2 * i + 1] = NAN;
        }
    }
}

/* S82: the Q5 position of output pixel (px, py); 0 = unusable */
int und_position(const double* cam, const double* lens, const double* R, const double* ncam, int px, int py, int32_t* qx, int32_t* qy)
{
    double s[2], fx, fy;
    if (!und_source_position(cam, lens, R, ncam, (double)px, (double)py, s)) return 0;
    fx = s[0] * 32.0;
    fy = s[1] * 32.0;
    if (!(fabs(fx) < 1073741824.0) || !(fabs(fy) < 1073741824.0)) return 0;
    *qx = (int32_t)rint(fx);
    *qy = (int32_t)rint(fy);
    return 1;
}

/* S83: dw * dh pairs */
void und_map(const double* cam, const double* lens, const double* R, const double* ncam, int dw, int dh, int32_t* map)
{
    int x, y;
    for (y = 0; y < dh; ++y)
        for (x = 0; x < dw; ++x) {
            int32_t qx, qy;
            if (!und_position(cam, lens, R, ncam, x, y, &qx, &qy)) qx = qy = INT32_MIN;
            map[2 * ((size_t)y * dw + x)] = qx;
            map[2 * ((size_t)y * dw + x) + 1] = qy;
        }
}

/* S77 at any int32 Q5 position, in 64-bit integers */
static int und_sample(const uint8_t* src, int sw, int sh, int sstride, int32_t qx, int32_t qy, int replicate, int border, int* ok)
{
    const int64_t x0 = (qx >= 0 ? (int64_t)qx / 32 : -((31 - (int64_t)qx) / 32)), y0 = (qy >= 0 ? (int64_t)qy / 32 : -((31 - (int64_t)qy) / 32));
    const int64_t ax = (int64_t)qx - 32 * x0, ay = (int64_t)qy - 32 * y0;
    const int64_t wx[2] = {32 - ax, ax}, wy[2] = {32 - ay, ay};
    int64_t sum = 0;
    int i, j;
    *ok = 1;
    for (j = 0; j < 2; ++j)
        for (i = 0; i < 2; ++i) {
            const int64_t wgt = wx[i] * wy[j];
            int64_t xx = x0 + i, yy = y0 + j;
            int in, v;
            if (wgt == 0) continue;
            in = xx >= 0 && xx < sw && yy >= 0 && yy < sh;
            if (!in) *ok = 0;
            if (replicate) {
                xx = xx < 0 ? 0 : (xx > sw - 1 ? sw - 1 : xx);
                yy = yy < 0 ? 0 : (yy > sh - 1 ? sh - 1 : yy);
                v = src[(size_t)yy * sstride + (size_t)xx];
            } else {
                v = in ? src[(size_t)yy * sstride + (size_t)xx] : border;
            }
            sum += wgt * v;
        }
    return (int)((sum + 512) >> 10);
}

/* S83: dst (dh rows of dstride bytes, dw written), valid (dw x dh, may be NULL); returns n_valid */
int und_remap(const uint8_t* src, int sw, int sh, int sstride, const int32_t* map, int replicate, int border, uint8_t* dst, int dw, int dh,
              int dstride, uint8_t* valid)
{
    int32_t n_valid = 0;
    int x, y;
    for (y = 0; y < dh; ++y)
        for (x = 0; x < dw; ++x) {
            const int32_t qx = map[2 * ((size_t)y * dw + x)], qy = map[2 * ((size_t)y * dw + x) + 1];
            int out = border, ok = 0;
            if (!(qx == INT32_MIN && qy == INT32_MIN)) out = und_sample(src, sw, sh, sstride, qx, qy, replicate, border, &ok);
            dst[(size_t)y * dstride + x] = (uint8_t)out;
            if (valid) valid[(size_t)y * dw + x] = (uint8_t)ok;
            n_valid += ok;
        }
    return n_valid;
}

/* S82 + S77, pixel by pixel, without a map; returns n_valid */
int und_image(const uint8_t* src, int sw, int sh, int sstride, const double* cam, const double* lens, const double* R, const double* ncam,
              int replicate, int border, uint8_t* dst, int dw, int dh, int dstride, uint8_t* valid)
{
    int32_t n_valid = 0;
    int x, y;
    for (y = 0; y < dh; ++y)
        for (x = 0; x < dw; ++x) {
            int32_t qx, qy;
            int out = border, ok = 0;
            if (und_position(cam, lens, R, ncam, x, y, &qx, &qy)) out = und_sample(src, sw, sh, sstride, qx, qy, replicate, border, &ok);
            dst[(size_t)y * dstride + x] = (uint8_t)out;
            if (valid) valid[(size_t)y * dw + x] = (uint8_t)ok;
            n_valid += ok;
        }
    return n_valid;
}
