/* vocab_ref.c — plain-C restatement of docs/SPEC.md S102-S106 (visual vocabularies: stride initialisation, assignment,
 * centroid update, the training loop with its records, bag-of-words encoding).  One thread, no tricks: every loop is the
 * sentence of the spec it stands for.  Built and loaded by tests/vocab_ref.py. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define VR_L2_U8 0
#define VR_BITS 1

typedef struct vr_iter { int32_t n_changed, n_empty, n_moved, reserved; uint64_t cost; } vr_iter;

/* the integer distance of S105's cost: squared L2 of the bytes, or the bit count of the XOR */
static uint32_t vr_idist(int kind, const uint8_t* a, const uint8_t* b, int bytes)
{
    uint32_t d = 0;
    for (int i = 0; i < bytes; ++i) {
        if (kind == VR_L2_U8) {
            const int t = (int)a[i] - (int)b[i];
            d += (uint32_t)(t * t);
        } else {
            d += (uint32_t)__builtin_popcount((unsigned)(a[i] ^ b[i]));
        }
    }
    return d;
}

/* the matcher's distance (S1 on u8 values is the exact integer, at most 256 * 255^2 < 2^24, then one sqrtf; S2 is the count) */
static float vr_fdist(int kind, uint32_t d)
{
    return kind == VR_L2_U8 ? sqrtf((float)d) : (float)d;
}

/* S105: word i takes the bytes of row floor(i * n / K) */
void vr_init_stride(const uint8_t* rows, int n, int bytes, int K, uint8_t* words)
{
    for (int i = 0; i < K; ++i) {
        const int64_t r = (int64_t)i * n / K;
        memcpy(words + (size_t)i * bytes, rows + (size_t)r * bytes, (size_t)bytes);
    }
}

/* S103: the k = 1 record of the matcher with the vocabulary as the train set: words scanned upward, strict < on the
 * float distance (S3 compares after the square root), so the lowest word index wins a tie.  idist may be NULL. */
void vr_assign(int kind, int bytes, const uint8_t* words, int K, const uint8_t* rows, int n, int32_t* labels, float* dist,
               uint32_t* idist)
{
    for (int i = 0; i < n; ++i) {
        int best = -1;
        float bd = 0.f;
        uint32_t bi = 0;
        for (int c = 0; c < K; ++c) {
            const uint32_t di = vr_idist(kind, rows + (size_t)i * bytes, words + (size_t)c * bytes, bytes);
            const float d = vr_fdist(kind, di);
            if (best < 0 || d < bd) { best = c; bd = d; bi = di; }
        }
        labels[i] = best;
        if (dist) dist[i] = bd;
        if (idist) idist[i] = bi;
    }
}

/* S104: rounded mean (halves up) / majority bit (an even split gives 0); a word without rows keeps its bytes */
void vr_update(int kind, int bytes, uint8_t* words, int K, const uint8_t* rows, int n, const int32_t* labels, int32_t* n_empty,
               int32_t* n_moved)
{
    const int A = kind == VR_L2_U8 ? bytes : bytes * 8;
    uint64_t* acc = (uint64_t*)calloc((size_t)K * A, sizeof(uint64_t));
    uint64_t* cnt = (uint64_t*)calloc((size_t)K, sizeof(uint64_t));
    for (int i = 0; i < n; ++i) {
        const int c = labels[i];
        const uint8_t* r = rows + (size_t)i * bytes;
        cnt[c] += 1;
        for (int a = 0; a < A; ++a)
            acc[(size_t)c * A + a] += kind == VR_L2_U8 ? r[a] : (uint64_t)((r[a >> 3] >> (a & 7)) & 1u);
    }
    *n_empty = 0;
    *n_moved = 0;
    for (int c = 0; c < K; ++c) {
        uint8_t* w = words + (size_t)c * bytes;
        if (cnt[c] == 0) { *n_empty += 1; continue; }
        int moved = 0;
        for (int b = 0; b < bytes; ++b) {
            uint8_t v = 0;
            if (kind == VR_L2_U8) {
                v = (uint8_t)((2 * acc[(size_t)c * A + b] + cnt[c]) / (2 * cnt[c]));
            } else {
                for (int k = 0; k < 8; ++k)
                    if (2 * acc[(size_t)c * A + 8 * b + k] > cnt[c]) v |= (uint8_t)(1u << k);
            }
            moved |= v != w[b];
            w[b] = v;
        }
        *n_moved += moved;
    }
    free(acc);
    free(cnt);
}

/* S105: iteration t = S103, then S104.  labels: n, the labels of the last iteration (untouched when iters == 0); info: iters
 * records; words_after: iters x K x bytes, the vocabulary after every iteration (may be NULL). */
void vr_train(int kind, int bytes, uint8_t* words, int K, const uint8_t* rows, int n, int iters, int32_t* labels, vr_iter* info,
              uint8_t* words_after)
{
    int32_t* cur = (int32_t*)malloc(sizeof(int32_t) * (size_t)n);
    int32_t* prev = (int32_t*)malloc(sizeof(int32_t) * (size_t)n);
    uint32_t* id = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)n);
    for (int t = 0; t < iters; ++t) {
        vr_iter r;
        memset(&r, 0, sizeof r);
        vr_assign(kind, bytes, words, K, rows, n, cur, NULL, id);
        for (int i = 0; i < n; ++i) {
            r.n_changed += t == 0 || cur[i] != prev[i];
            r.cost += id[i];
        }
        vr_update(kind, bytes, words, K, rows, n, cur, &r.n_empty, &r.n_moved);
        if (info) info[t] = r;
        if (words_after) memcpy(words_after + (size_t)t * K * bytes, words, (size_t)K * bytes);
        memcpy(prev, cur, sizeof(int32_t) * (size_t)n);
    }
    if (iters > 0 && labels) memcpy(labels, cur, sizeof(int32_t) * (size_t)n);
    free(cur);
    free(prev);
    free(id);
}

/* S106: m = n without a count, else clamp(count, 0, n); labels and distances of the rows below m, -1 / NaN from m to n,
 * the histogram of the labels below m over exactly K words.  Any output may be NULL. */
void vr_encode(int kind, int bytes, const uint8_t* words, int K, const uint8_t* rows, int n, int has_count, int32_t count,
               int32_t* out_words, float* out_dist, uint32_t* hist)
{
    const int m = !has_count ? n : (count < 0 ? 0 : (count > n ? n : count));
    int32_t* lab = (int32_t*)malloc(sizeof(int32_t) * (size_t)(m > 0 ? m : 1));
    float* d = (float*)malloc(sizeof(float) * (size_t)(m > 0 ? m : 1));
    vr_assign(kind, bytes, words, K, rows, m, lab, d, NULL);
    if (hist) memset(hist, 0, sizeof(uint32_t) * (size_t)K);
    for (int i = 0; i < n; ++i) {
        if (out_words) out_words[i] = i < m ? lab[i] : -1;
        if (out_dist) out_dist[i] = i < m ? d[i] : NAN;
        if (hist && i < m) hist[lab[i]] += 1;
    }
    free(lab);
    free(d);
}
