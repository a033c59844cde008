/* Plain-C restatement of docs/SPEC.md S89-S92 (semi-global matching on a rectified 8-bit pair: census cost, 4 or 8 paths,
 * S85's winner on the summed path costs): brute force.  The census bits are compared one by one from the pixels, the cost volume
 * and one L volume per direction are stored whole, each direction is a plain scan over the rectangle in an order that visits a
 * pixel's predecessor first.  The GPU tests compare the library against it bit for bit; tests/test_sgm_cpu.py pins it against
 * numpy. */
#include <stdint.h>
#include <stdlib.h>

#define SG_INVALID (-32768)
#define SG_FROM_RIGHT 1

int sg_invalid(void) { return SG_INVALID; }

/* S85's floor((16 (p - n) + den) / (2 den)), 0 when den == 0 */
static int subpixel(int p, int c, int n)
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

/* S89, S90: the differing census bits of base(x, y) and other(xo, y) */
static int cost(const uint8_t* base, const uint8_t* other, int bstride, int ostride, int x, int xo, int y)
{
    int i, j, sum = 0;
    const int cb = base[(size_t)y * bstride + x], co = other[(size_t)y * ostride + xo];
    for (j = -3; j <= 3; ++j)
        for (i = -4; i <= 4; ++i) {
            const int a = base[(size_t)(y + j) * bstride + x + i] < cb, b = other[(size_t)(y + j) * ostride + xo + i] < co;
            if (i == 0 && j == 0) continue;
            sum += a != b;
        }
    return sum;
}

/* S89-S92.  disp: h rows of dstride elements, w written per row.  Returns n_valid, or -1 when memory runs out. */
int sg_sgm(const uint8_t* left, const uint8_t* right, int w, int h, int lstride, int rstride, int min_disp, int num_disp, int p1, int p2,
           int paths, int uniqueness, int flags, int16_t* disp, int dstride)
{
    static const int DX[8] = {1, -1, 0, 0, 1, -1, 1, -1}, DY[8] = {0, 0, 1, -1, 1, 1, -1, -1};
    const int D = num_disp, dmin = min_disp, dmax = min_disp + num_disp - 1, from_right = (flags & SG_FROM_RIGHT) != 0;
    const uint8_t* base = from_right ? right : left;
    const uint8_t* other = from_right ? left : right;
    const int bstride = from_right ? rstride : lstride, ostride = from_right ? lstride : rstride;
    const int x0 = from_right ? 4 - (dmin < 0 ? dmin : 0) : 4 + (dmax > 0 ? dmax : 0);
    const int x1 = from_right ? w - 5 - (dmax > 0 ? dmax : 0) : w - 5 + (dmin < 0 ? dmin : 0);
    const int y0 = 3, y1 = h - 4;
    const int wc = x1 - x0 + 1, hc = y1 - y0 + 1;
    int x, y, k, r, n_valid = 0;
    size_t vol;
    int *C, *L, *S;
    for (y = 0; y < h; ++y)
        for (x = 0; x < w; ++x) disp[(size_t)y * dstride + x] = SG_INVALID;
    if (wc <= 0 || hc <= 0) return 0;
    vol = (size_t)wc * hc * D;
    C = (int*)malloc(vol * sizeof(int));
    L = (int*)malloc(vol * sizeof(int));
    S = (int*)calloc(vol, sizeof(int));
    if (!C || !L || !S) {
        free(C); free(L); free(S);
        return -1;
    }
#define AT(xx, yy) (((size_t)((yy) - y0) * wc + ((xx) - x0)) * D)
    for (y = y0; y <= y1; ++y)
        for (x = x0; x <= x1; ++x)
            for (k = 0; k < D; ++k) C[AT(x, y) + k] = cost(base, other, bstride, ostride, x, from_right ? x + (dmin + k) : x - (dmin + k), y);
    for (r = 0; r < paths; ++r) {
        const int dx = DX[r], dy = DY[r];
        int iy, ix;
        for (iy = 0; iy < hc; ++iy) {
            y = dy >= 0 ? y0 + iy : y1 - iy;                       /* the predecessor's row comes first */
            for (ix = 0; ix < wc; ++ix) {
                const int* c;
                int* l;
                int qx, qy;
                x = dx >= 0 ? x0 + ix : x1 - ix;                   /* within a row, the predecessor's column first */
                c = C + AT(x, y);
                l = L + AT(x, y);
                qx = x - dx;
                qy = y - dy;
                if (qx < x0 || qx > x1 || qy < y0 || qy > y1) {
                    for (k = 0; k < D; ++k) l[k] = c[k];
                } else {
                    const int* q = L + AT(qx, qy);
                    int m = q[0];
                    for (k = 1; k < D; ++k)
                        if (q[k] < m) m = q[k];
                    for (k = 0; k < D; ++k) {
                        int best = q[k];
                        if (k > 0 && q[k - 1] + p1 < best) best = q[k - 1] + p1;
                        if (k < D - 1 && q[k + 1] + p1 < best) best = q[k + 1] + p1;
                        if (m + p2 < best) best = m + p2;
                        l[k] = c[k] + best - m;
                    }
                }
            }
        }
        for (vol = 0; vol < (size_t)wc * hc * D; ++vol) S[vol] += L[vol];
    }
    for (y = y0; y <= y1; ++y)
        for (x = x0; x <= x1; ++x) {
            const int* s = S + AT(x, y);
            int k1 = 0, c1, have2 = 0, c2 = 0, off = 0;
            for (k = 1; k < D; ++k)
                if (s[k] < s[k1]) k1 = k;
            c1 = s[k1];
            for (k = 0; k < D; ++k)
                if (k - k1 > 1 || k1 - k > 1)
                    if (!have2 || s[k] < c2) {
                        c2 = s[k];
                        have2 = 1;
                    }
            if (have2 && c2 * (100 - uniqueness) < c1 * 100) continue;
            if (k1 > 0 && k1 < D - 1) off = subpixel(s[k1 - 1], c1, s[k1 + 1]);
            disp[(size_t)y * dstride + x] = (int16_t)(16 * (dmin + k1) + off);
            ++n_valid;
        }
#undef AT
    free(C); free(L); free(S);
    return n_valid;
}
