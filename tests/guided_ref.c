/* guided_ref.c — plain-C restatement of docs/SPEC.md S48-S50 (guided matching), written from the SPEC text: the fmaf
 * gates of S8 / S21 with the model rounded once to float, the S1 loop (on floats, or on bytes converted to float), the
 * S2 popcount, S3 keys and a full sort of the admitted rows per query, S4 on the 2-NN list.  It shares no code with the
 * library or the oracle.  Build: cc -O2 -ffp-contract=off (tests/cref.py). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct { int32_t queryIdx, trainIdx, imgIdx; float distance; } gr_match;

enum { GR_F_SAMPSON = 0, GR_F_SYM = 1, GR_H = 2 };
enum { GR_DESC_F32 = 0, GR_DESC_U8 = 1, GR_DESC_BINARY = 2 };

/* S48: 1 when the rounded model may admit anything at all */
static int model_usable(const double* M, float* m32)
{
    int nonzero = 0;
    for (int i = 0; i < 9; ++i) {
        m32[i] = (float)M[i];
        if (!isfinite(m32[i])) return 0;
        if (m32[i] != 0.0f) nonzero = 1;
    }
    return nonzero;
}

static int gate32(int kind, const float* f, float thr2, float x, float y, float xp, float yp)
{
    if (kind == GR_H) {
        float u = fmaf(f[0], x, fmaf(f[1], y, f[2]));
        float v = fmaf(f[3], x, fmaf(f[4], y, f[5]));
        float w = fmaf(f[6], x, fmaf(f[7], y, f[8]));
        float du = fmaf(-xp, w, u);
        float dv = fmaf(-yp, w, v);
        float rhs = thr2 * (w * w);
        return (fmaf(du, du, dv * dv) <= rhs) && (0.0f < rhs) && (rhs < INFINITY);
    }
    float a = fmaf(f[0], x, fmaf(f[1], y, f[2]));
    float b = fmaf(f[3], x, fmaf(f[4], y, f[5]));
    float c = fmaf(f[6], x, fmaf(f[7], y, f[8]));
    float num = fmaf(xp, a, fmaf(yp, b, c));
    float at = fmaf(f[0], xp, fmaf(f[3], yp, f[6]));
    float bt = fmaf(f[1], xp, fmaf(f[4], yp, f[7]));
    float n2 = num * num;
    if (kind == GR_F_SAMPSON) {
        float den = fmaf(a, a, fmaf(b, b, fmaf(at, at, bt * bt)));
        return n2 <= thr2 * den;
    }
    return (n2 <= thr2 * fmaf(a, a, b * b)) && (n2 <= thr2 * fmaf(at, at, bt * bt));
}

/* gate(i, j) for one pair of keypoints; model in doubles as the library receives it */
int gr_gate(int kind, const double* M, float tau, float x, float y, float xp, float yp)
{
    float m[9];
    if (!model_usable(M, m)) return 0;
    return gate32(kind, m, tau * tau, x, y, xp, yp);
}

/* S1 on two rows given as floats */
static float s1_distance(const float* a, const float* b, int dim)
{
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, s[4], d2;
    int j = 0;
    for (; j + 8 <= dim; j += 8)
        for (int l = 0; l < 8; ++l) {
            float t = a[j + l] - b[j + l];
            float p = t * t;
            acc[l] = acc[l] + p;
        }
    for (int l = 0; l < 4; ++l) s[l] = acc[l] + acc[l + 4];
    d2 = ((s[0] + s[1]) + s[2]) + s[3];
    for (; j < dim; ++j) {
        float t = a[j] - b[j];
        float p = t * t;
        d2 = d2 + p;
    }
    return sqrtf(d2);
}

static float s2_distance(const uint8_t* a, const uint8_t* b, int bytes)
{
    int c = 0;
    for (int i = 0; i < bytes; ++i) {
        unsigned v = (unsigned)(a[i] ^ b[i]);
        while (v) { c += (int)(v & 1u); v >>= 1; }
    }
    return (float)c;
}

static uint64_t s3_key(float d, int j)
{
    uint32_t bits;
    if (d != d) bits = 0x7FC00000u;
    else memcpy(&bits, &d, 4);
    return ((uint64_t)bits << 32) | (uint32_t)j;
}

static int cmp_u64(const void* a, const void* b)
{
    uint64_t x = *(const uint64_t*)a, y = *(const uint64_t*)b;
    return x < y ? -1 : (x > y ? 1 : 0);
}

/* S49.  desc: GR_DESC_*; width: dim or bytes.  out: nq x k records; n_admitted: nq counts (may be NULL). */
int gr_knn(int desc, const void* q, int nq, const void* t, int nt, int width, const float* kp1, const float* kp2, int kind,
           const double* M, float tau, int k, gr_match* out, int32_t* n_admitted)
{
    float m[9];
    const int usable = model_usable(M, m);
    const float thr2 = tau * tau;
    uint64_t* keys = (uint64_t*)malloc(sizeof(uint64_t) * (size_t)(nt > 0 ? nt : 1));
    float* qa = (float*)malloc(sizeof(float) * (size_t)width);
    float* ta = (float*)malloc(sizeof(float) * (size_t)width);
    if (!keys || !qa || !ta) return -1;
    for (int i = 0; i < nq; ++i) {
        int n = 0;
        if (desc == GR_DESC_U8)
            for (int c = 0; c < width; ++c) qa[c] = (float)((const uint8_t*)q)[(size_t)i * width + c];
        for (int j = 0; j < nt && usable; ++j) {
            float d;
            if (!gate32(kind, m, thr2, kp1[2 * i], kp1[2 * i + 1], kp2[2 * j], kp2[2 * j + 1])) continue;
            if (desc == GR_DESC_F32) {
                d = s1_distance((const float*)q + (size_t)i * width, (const float*)t + (size_t)j * width, width);
            } else if (desc == GR_DESC_U8) {
                for (int c = 0; c < width; ++c) ta[c] = (float)((const uint8_t*)t)[(size_t)j * width + c];
                d = s1_distance(qa, ta, width);
            } else {
                d = s2_distance((const uint8_t*)q + (size_t)i * width, (const uint8_t*)t + (size_t)j * width, width);
            }
            keys[n++] = s3_key(d, j);
        }
        qsort(keys, (size_t)n, sizeof(uint64_t), cmp_u64);
        for (int r = 0; r < k; ++r) {
            gr_match* o = out + (size_t)i * k + r;
            o->queryIdx = i;
            o->imgIdx = 0;
            if (r < n) {
                uint32_t bits = (uint32_t)(keys[r] >> 32);
                o->trainIdx = (int32_t)(uint32_t)keys[r];
                memcpy(&o->distance, &bits, 4);
            } else {
                o->trainIdx = -1;
                o->distance = INFINITY;
            }
        }
        if (n_admitted) n_admitted[i] = n;
    }
    free(keys); free(qa); free(ta);
    return 0;
}

/* S50: guided 2-NN (into knn, nq x 2), S4, survivors in query order with their keypoints.  Returns the survivor count. */
int gr_match_guided(int desc, const void* q, int nq, const void* t, int nt, int width, const float* kp1, const float* kp2,
                    int kind, const double* M, float tau, float ratio, gr_match* knn, gr_match* good, float* xy1, float* xy2)
{
    int n = 0;
    if (gr_knn(desc, q, nq, t, nt, width, kp1, kp2, kind, M, tau, 2, knn, NULL) != 0) return -1;
    for (int i = 0; i < nq; ++i) {
        const gr_match* a = knn + 2 * (size_t)i;
        float rhs = ratio * a[1].distance;
        if (a[0].trainIdx < 0 || a[1].trainIdx < 0 || !(a[0].distance < rhs)) continue;
        good[n] = a[0];
        xy1[2 * n] = kp1[2 * i];                 xy1[2 * n + 1] = kp1[2 * i + 1];
        xy2[2 * n] = kp2[2 * a[0].trainIdx];     xy2[2 * n + 1] = kp2[2 * a[0].trainIdx + 1];
        ++n;
    }
    return n;
}
