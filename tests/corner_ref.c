/* corner_ref.c — plain serial restatement of docs/SPEC.md S67-S70 (minimum-eigenvalue corners with a greedy minimum-distance
 * selection), for the tests only.  Direct block sums, no running sums, no tiling; one function per section.  Loaded through
 * tests/cref.py by tests/corner_ref.py. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

/* S67: 1 when (x, y) lies in the valid region V. */
int corner_in_v(int w, int h, int r, int x, int y)
{
    return x >= r + 1 && x <= w - r - 3 && y >= r + 1 && y <= h - r - 3;
}

/* S67: the response e of one pixel of V (img: h rows of w bytes). */
double corner_response(const uint8_t* img, int w, int h, int r, int x, int y)
{
    int32_t A = 0, B = 0, C = 0;
    (void)h;
    for (int v = y - r; v <= y + r; ++v)
        for (int u = x - r; u <= x + r; ++u) {
            const int cx = (int)img[(size_t)v * w + u + 1] - (int)img[(size_t)v * w + u - 1];
            const int cy = (int)img[(size_t)(v + 1) * w + u] - (int)img[(size_t)(v - 1) * w + u];
            A += cx * cx;
            B += cx * cy;
            C += cy * cy;
        }
    const double a = (double)A, b = (double)B, c = (double)C;
    const double N = (double)((2 * r + 1) * (2 * r + 1));
    return ((a + c) - sqrt((a - c) * (a - c) + 4.0 * (b * b))) / (8.0 * N);
}

/* S67: e at every pixel of V into plane (h x w doubles; pixels outside V are left alone). */
void corner_response_plane(const uint8_t* img, int w, int h, int r, double* plane)
{
    for (int y = r + 1; y <= h - r - 3; ++y)
        for (int x = r + 1; x <= w - r - 3; ++x) plane[(size_t)y * w + x] = corner_response(img, w, h, r, x, y);
}

/* S68: the candidates in scan order: pos[i] = y * w + x, e[i]; at most cap are written, all are counted. */
int corner_candidates(const uint8_t* img, int w, int h, int r, float min_eig, int cap, int32_t* pos, double* e_out)
{
    static const int before[4][2] = {{-1, -1}, {0, -1}, {1, -1}, {-1, 0}};
    static const int after[4][2] = {{1, 0}, {-1, 1}, {0, 1}, {1, 1}};
    double* plane = (double*)malloc((size_t)w * h * sizeof(double));
    int n = 0;
    corner_response_plane(img, w, h, r, plane);
    for (int y = r + 1; y <= h - r - 3; ++y)
        for (int x = r + 1; x <= w - r - 3; ++x) {
            const double e = plane[(size_t)y * w + x];
            int ok = e >= (double)min_eig && e > 0;
            for (int k = 0; k < 4 && ok; ++k) {
                int u = x + before[k][0], v = y + before[k][1];
                if (corner_in_v(w, h, r, u, v) && !(e > plane[(size_t)v * w + u])) ok = 0;
                u = x + after[k][0];
                v = y + after[k][1];
                if (corner_in_v(w, h, r, u, v) && !(e >= plane[(size_t)v * w + u])) ok = 0;
            }
            if (!ok) continue;
            if (n < cap) {
                pos[n] = y * w + x;
                e_out[n] = e;
            }
            ++n;
        }
    free(plane);
    return n;
}

static int cmp_u64(const void* a, const void* b)
{
    const uint64_t x = *(const uint64_t*)a, y = *(const uint64_t*)b;
    return x < y ? -1 : (x > y ? 1 : 0);
}

/* S69: sorts the n candidates: rank_pos[k], rank_s[k] = position and fp32 score of rank k; returns the number of ranks that
 * survive the relative quality cut (a prefix). */
int corner_rank(int n, const int32_t* pos, const double* e, float quality, int32_t* rank_pos, float* rank_s)
{
    uint64_t* keys = (uint64_t*)malloc((size_t)(n > 0 ? n : 1) * sizeof(uint64_t));
    int kept = 0;
    for (int i = 0; i < n; ++i) {
        const float s = (float)e[i];
        uint32_t bits;
        memcpy(&bits, &s, 4);
        keys[i] = ((uint64_t)(~bits) << 32) | (uint32_t)pos[i];
    }
    qsort(keys, (size_t)n, sizeof(uint64_t), cmp_u64);
    for (int k = 0; k < n; ++k) {
        const uint32_t bits = ~(uint32_t)(keys[k] >> 32);
        memcpy(&rank_s[k], &bits, 4);
        rank_pos[k] = (int32_t)(uint32_t)keys[k];
    }
    if (n > 0) {
        const float floor_s = quality * rank_s[0];
        while (kept < n && !(rank_s[kept] < floor_s)) ++kept;
    }
    free(keys);
    return kept;
}

/* S70: the greedy walk over the first n ranks.  keep: n_keep x 2 floats.  Writes xy / score rows in acceptance order and, where
 * asked for, fate[k] of every rank: 1 accepted, 2 rejected, 0 not walked (the walk stopped first).  Returns the count. */
int corner_select(int n, int w, const int32_t* rank_pos, const float* rank_s, float min_dist, const float* keep, int n_keep,
                  int max_corners, float* xy, float* score, uint8_t* fate)
{
    const float md2 = min_dist * min_dist;
    int m = 0;
    if (fate) memset(fate, 0, (size_t)n);
    for (int k = 0; k < n && m < max_corners; ++k) {
        const float fx = (float)(rank_pos[k] % w), fy = (float)(rank_pos[k] / w);
        int blocked = 0;
        for (int j = 0; j < n_keep && !blocked; ++j) {
            const float dx = fx - keep[2 * j], dy = fy - keep[2 * j + 1];
            if (dx * dx + dy * dy < md2) blocked = 1;
        }
        for (int j = 0; j < m && !blocked; ++j) {
            const float dx = fx - xy[2 * j], dy = fy - xy[2 * j + 1];
            if (dx * dx + dy * dy < md2) blocked = 1;
        }
        if (fate) fate[k] = blocked ? 2 : 1;
        if (blocked) continue;
        xy[2 * m] = fx;
        xy[2 * m + 1] = fy;
        if (score) score[m] = rank_s[k];
        ++m;
    }
    return m;
}

/* S67-S70 in one call.  Returns the number of corners; *n_cand: the candidates after S68. */
int corner_detect(const uint8_t* img, int w, int h, int r, float min_eig, float quality, float min_dist, const float* keep, int n_keep,
                  int max_corners, float* xy, float* score, int* n_cand)
{
    const int cap = w * h;
    int32_t* pos = (int32_t*)malloc((size_t)cap * sizeof(int32_t));
    double* e = (double*)malloc((size_t)cap * sizeof(double));
    int32_t* rpos = (int32_t*)malloc((size_t)cap * sizeof(int32_t));
    float* rs = (float*)malloc((size_t)cap * sizeof(float));
    const int n = corner_candidates(img, w, h, r, min_eig, cap, pos, e);
    const int kept = corner_rank(n, pos, e, quality, rpos, rs);
    const int m = corner_select(kept, w, rpos, rs, min_dist, keep, n_keep, max_corners, xy, score, NULL);
    if (n_cand) *n_cand = n;
    free(pos);
    free(e);
    free(rpos);
    free(rs);
    return m;
}
