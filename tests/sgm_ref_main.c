/* Stand-alone driver of tests/sgm_ref.c (SPEC S89-S92) on the limit shapes: one computed pixel and none, 256 disparities, ranges
 * that touch -1024 and 1024, p2 = 1023, odd strides.  Every buffer lies between guard bytes that the program checks itself, as
 * it checks the elements between the rows of the map, the pixels outside the computed rectangle and the count.  The test builds
 * it with AddressSanitizer and UBSan and runs it as a child process: exit status 0 and an empty stderr. */
#include <stdio.h>
#include <string.h>

#include "sgm_ref.c"

#define GUARD 64

static unsigned rnd_state = 12345u;
static unsigned rnd(void)
{
    rnd_state = rnd_state * 1664525u + 1013904223u;
    return rnd_state >> 24;
}

static int fail(const char* what, int id)
{
    printf("case %d: %s\n", id, what);
    return 1;
}

/* returns 0 when every check holds */
static int run_case(int id, int w, int h, int lstride, int rstride, int dstride, int dmin, int D, int p1, int p2, int paths, int uniq, int flags)
{
    const int dmax = dmin + D - 1, fr = flags & SG_FROM_RIGHT;
    const int x0 = fr ? 4 - (dmin < 0 ? dmin : 0) : 4 + (dmax > 0 ? dmax : 0);
    const int x1 = fr ? w - 5 - (dmax > 0 ? dmax : 0) : w - 5 + (dmin < 0 ? dmin : 0);
    const int y0 = 3, y1 = h - 4;
    const long computed = (x1 >= x0 && y1 >= y0) ? (long)(x1 - x0 + 1) * (y1 - y0 + 1) : 0;
    const size_t lb = (size_t)(h - 1) * lstride + w, rb = (size_t)(h - 1) * rstride + w, db = (size_t)(h - 1) * dstride + w;
    uint8_t* lbuf = (uint8_t*)malloc(lb + 2 * GUARD);
    uint8_t* rbuf = (uint8_t*)malloc(rb + 2 * GUARD);
    int16_t* dbuf = (int16_t*)malloc((db + 2 * GUARD) * sizeof(int16_t));
    size_t i;
    int x, y, n, bad = 0;
    long valid = 0;
    if (!lbuf || !rbuf || !dbuf) return fail("out of memory", id);
    for (i = 0; i < lb + 2 * GUARD; ++i) lbuf[i] = (uint8_t)rnd();
    for (i = 0; i < rb + 2 * GUARD; ++i) rbuf[i] = (uint8_t)rnd();
    for (i = 0; i < db + 2 * GUARD; ++i) dbuf[i] = 0x5A5A;
    n = sg_sgm(lbuf + GUARD, rbuf + GUARD, w, h, lstride, rstride, dmin, D, p1, p2, paths, uniq, flags, dbuf + GUARD, dstride);
    if (n < 0) bad = fail("the restatement ran out of memory", id);
    for (i = 0; i < GUARD; ++i)
        if (dbuf[i] != 0x5A5A || dbuf[GUARD + db + i] != 0x5A5A) bad = fail("a guard of the map changed", id);
    for (y = 0; y < h; ++y) {
        for (x = w; x < dstride && y < h - 1; ++x)
            if (dbuf[GUARD + (size_t)y * dstride + x] != 0x5A5A) bad = fail("an element between the rows changed", id);
        for (x = 0; x < w; ++x) {
            const int v = dbuf[GUARD + (size_t)y * dstride + x];
            const int inside = x >= x0 && x <= x1 && y >= y0 && y <= y1;
            if (v != SG_INVALID) {
                ++valid;
                if (!inside) bad = fail("a value outside the computed rectangle", id);
                if (v < 16 * dmin - 8 || v > 16 * dmax + 8) bad = fail("a value outside the disparity range", id);
                if (D == 1 && v != 16 * dmin) bad = fail("one disparity, another value", id);
            }
        }
    }
    if (valid != n) bad = fail("n_valid is not the count", id);
    if (uniq == 0 && n != computed) bad = fail("uniqueness 0 rejected a pixel", id);
    if (n > computed) bad = fail("more valid pixels than computed ones", id);
    free(lbuf); free(rbuf); free(dbuf);
    return bad;
}

int main(void)
{
    int bad = 0, id = 0, flags, paths;
    for (flags = 0; flags <= 1; ++flags)
        for (paths = 4; paths <= 8; paths += 4) {
            /* one computed pixel, then none in each direction, then 1 x 1 */
            bad |= run_case(id++, 9 + 5, 7, 14, 14, 14, 0, 6, 4, 24, paths, 0, flags);
            bad |= run_case(id++, 9 + 4, 7, 13, 13, 13, 0, 6, 4, 24, paths, 0, flags);
            bad |= run_case(id++, 9 + 5, 6, 14, 14, 14, 0, 6, 4, 24, paths, 0, flags);
            bad |= run_case(id++, 9 + 2 + 3, 7, 17, 15, 19, -2, 6, 4, 24, paths, 15, flags);
            bad |= run_case(id++, 1, 1, 1, 1, 1, 0, 1, 0, 0, paths, 0, flags);
            bad |= run_case(id++, 1, 1, 3, 5, 7, -1024, 256, 1023, 1023, paths, 99, flags);
            /* 256 disparities, odd strides */
            bad |= run_case(id++, 9 + 255 + 6, 9, 271, 273, 275, 0, 256, 4, 24, paths, 0, flags);
            bad |= run_case(id++, 9 + 255 + 6, 9, 277, 271, 281, -100, 256, 0, 1023, paths, 15, flags);
            /* the ends of the range: dmin = -1024, dmax = 1024 */
            bad |= run_case(id++, 9 + 1024 + 5, 8, 1039, 1041, 1043, -1024, 3, 7, 7, paths, 0, flags);
            bad |= run_case(id++, 9 + 1024 + 5, 8, 1038, 1039, 1045, 1022, 3, 1023, 1023, paths, 15, flags);
            bad |= run_case(id++, 9 + 1024 + 3, 7, 1037, 1037, 1037, 769, 256, 0, 1023, paths, 99, flags);
            bad |= run_case(id++, 9 + 1024 + 3, 7, 1037, 1039, 1041, -1024, 256, 0, 0, paths, 0, flags);
            /* a rectangle one pixel high and one pixel wide */
            bad |= run_case(id++, 40, 7, 41, 43, 45, -3, 9, 4, 24, paths, 15, flags);
            bad |= run_case(id++, 9 + 8, 30, 17, 19, 21, 0, 9, 4, 24, paths, 15, flags);
        }
    if (bad) return 1;
    printf("ok %d cases\n", id);
    return 0;
}
