/* bowdb_ref.c — plain-C restatement of docs/SPEC.md S107-S112 (the image database: adding a histogram, weights and
 * ilog2_q8, norms, the exact L1 score, the ordered selection).  One thread, no tricks: every loop is the sentence of the
 * spec it stands for.  Built and loaded by tests/bowdb_ref.py. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct br_db {
    int K, max_images, max_entries;
    int n_images, n_entries;
    uint32_t* offsets;   /* max_images + 1 */
    uint32_t* norms;     /* max_images */
    uint32_t* words;     /* max_entries */
    uint16_t* tfs;       /* max_entries */
    uint32_t* df;        /* K */
    uint32_t* weight;    /* K */
} br_db;

br_db* br_create(int K, int max_images, int max_entries)
{
    br_db* d = (br_db*)calloc(1, sizeof(br_db));
    d->K = K; d->max_images = max_images; d->max_entries = max_entries;
    d->offsets = (uint32_t*)calloc((size_t)max_images + 1, 4);
    d->norms = (uint32_t*)calloc((size_t)max_images, 4);
    d->words = (uint32_t*)calloc((size_t)max_entries, 4);
    d->tfs = (uint16_t*)calloc((size_t)max_entries, 2);
    d->df = (uint32_t*)calloc((size_t)K, 4);
    d->weight = (uint32_t*)calloc((size_t)K, 4);
    for (int w = 0; w < K; ++w) d->weight[w] = 1;                       /* S107: weights start at 1 */
    return d;
}

void br_destroy(br_db* d)
{
    if (!d) return;
    free(d->offsets); free(d->norms); free(d->words); free(d->tfs); free(d->df); free(d->weight);
    free(d);
}

/* S107: all images, entries and df go; the weights stay */
void br_clear(br_db* d)
{
    d->n_images = 0; d->n_entries = 0;
    memset(d->df, 0, (size_t)d->K * 4);
}

/* S108 */
int32_t br_add(br_db* d, const uint32_t* hist)
{
    uint64_t T = 0, nnz = 0;
    for (int w = 0; w < d->K; ++w) { T += hist[w]; nnz += hist[w] != 0; }
    if (T < 1 || T > 65535) return -1;
    if (d->n_images >= d->max_images || (uint64_t)d->n_entries + nnz > (uint64_t)d->max_entries) return -2;
    uint32_t norm = 0;
    for (int w = 0; w < d->K; ++w) {
        if (hist[w] == 0) continue;
        d->words[d->n_entries] = (uint32_t)w;
        d->tfs[d->n_entries] = (uint16_t)hist[w];
        d->n_entries += 1;
        d->df[w] += 1;
        norm += hist[w] * d->weight[w];
    }
    d->norms[d->n_images] = norm;
    d->n_images += 1;
    d->offsets[d->n_images] = (uint32_t)d->n_entries;
    return d->n_images - 1;
}

/* S109: the norm of every image under the current weights */
static void br_norms(br_db* d)
{
    for (int i = 0; i < d->n_images; ++i) {
        uint32_t s = 0;
        for (uint32_t e = d->offsets[i]; e < d->offsets[i + 1]; ++e) s += (uint32_t)d->tfs[e] * d->weight[d->words[e]];
        d->norms[i] = s;
    }
}

int br_set_weights(br_db* d, const uint32_t* weights)
{
    for (int w = 0; w < d->K; ++w)
        if (weights[w] > 8191) return -1;
    memcpy(d->weight, weights, (size_t)d->K * 4);
    br_norms(d);
    return 0;
}

/* S109: floor(256 * log2(N / dd)) for 1 <= dd <= N */
uint32_t br_ilog2_q8(uint32_t N, uint32_t dd)
{
    uint32_t e = 0;
    while (((uint64_t)dd << (e + 1)) <= (uint64_t)N) ++e;
    uint64_t m = ((uint64_t)N << 30) / ((uint64_t)dd << e);
    uint32_t f = 0;
    for (int i = 0; i < 8; ++i) {
        m = (m * m) >> 30;
        f <<= 1;
        if (m >= ((uint64_t)1 << 31)) { f |= 1; m >>= 1; }
    }
    return (e << 8) | f;
}

void br_idf(br_db* d)
{
    const uint32_t N = (uint32_t)d->n_images;
    if (N == 0) return;
    for (int w = 0; w < d->K; ++w) d->weight[w] = br_ilog2_q8(N, d->df[w] > 1 ? d->df[w] : 1);
    br_norms(d);
}

/* S110 for every image into all[0 .. n_images); returns 0 when the query is refused (then every score is 0) */
static int br_scores(const br_db* d, const uint32_t* hist, double* all)
{
    uint64_t T = 0, Nq = 0;
    for (int w = 0; w < d->K; ++w) T += hist[w];
    const int ok = T >= 1 && T <= 65535;
    if (ok)
        for (int w = 0; w < d->K; ++w) Nq += (uint64_t)hist[w] * d->weight[w];
    for (int i = 0; i < d->n_images; ++i) {
        const uint64_t Nd = d->norms[i];
        all[i] = 0.0;
        if (!ok || Nq == 0 || Nd == 0) continue;
        uint64_t S = 0;
        for (uint32_t e = d->offsets[i]; e < d->offsets[i + 1]; ++e) {
            const uint32_t w = d->words[e];
            const uint64_t a = (uint64_t)hist[w] * d->weight[w] * Nd, b = (uint64_t)d->tfs[e] * d->weight[w] * Nq;
            S += a < b ? a : b;
        }
        all[i] = (double)S / (double)(Nq * Nd);
    }
    return ok;
}

/* S111: ids / scores have `top` elements, all (may be NULL) n_images; returns the count */
int32_t br_query(const br_db* d, const uint32_t* hist, int top, int excl_lo, int excl_hi, int32_t* ids, double* scores, double* all)
{
    double* s = (double*)calloc((size_t)d->n_images + 1, 8);
    char* taken = (char*)calloc((size_t)d->n_images + 1, 1);
    br_scores(d, hist, s);
    if (all) memcpy(all, s, (size_t)d->n_images * 8);
    int32_t count = 0;
    for (int j = 0; j < top; ++j) {                                     /* the best remaining candidate, `top` times */
        int best = -1;
        for (int i = 0; i < d->n_images; ++i) {
            if (taken[i] || !(s[i] > 0.0) || (i >= excl_lo && i < excl_hi)) continue;
            if (best < 0 || s[i] > s[best]) best = i;                   /* equal scores: the lower id stays */
        }
        if (best < 0) break;
        taken[best] = 1;
        ids[count] = best;
        scores[count] = s[best];
        count += 1;
    }
    for (int j = count; j < top; ++j) {
        const uint64_t qnan = 0x7FF8000000000000ull;
        ids[j] = -1;
        memcpy(&scores[j], &qnan, 8);
    }
    free(s); free(taken);
    return count;
}

/* a database as pm_bowdb_get wrote it out (a persisted one): the inverse of br_get */
int br_load(br_db* d, int32_t n_images, int32_t n_entries, const uint32_t* offsets, const uint32_t* words, const uint16_t* tfs,
            const uint32_t* norms, const uint32_t* df, const uint32_t* weights)
{
    if (n_images < 0 || n_images > d->max_images || n_entries < 0 || n_entries > d->max_entries) return -1;
    d->n_images = n_images; d->n_entries = n_entries;
    memcpy(d->offsets, offsets, ((size_t)n_images + 1) * 4);
    memcpy(d->words, words, (size_t)n_entries * 4);
    memcpy(d->tfs, tfs, (size_t)n_entries * 2);
    memcpy(d->norms, norms, (size_t)n_images * 4);
    memcpy(d->df, df, (size_t)d->K * 4);
    memcpy(d->weight, weights, (size_t)d->K * 4);
    return 0;
}

void br_get(const br_db* d, int32_t* n_images, int32_t* n_entries, uint32_t* offsets, uint32_t* words, uint16_t* tfs, uint32_t* norms,
            uint32_t* df, uint32_t* weights)
{
    if (n_images) *n_images = d->n_images;
    if (n_entries) *n_entries = d->n_entries;
    if (offsets) memcpy(offsets, d->offsets, ((size_t)d->n_images + 1) * 4);
    if (words) memcpy(words, d->words, (size_t)d->n_entries * 4);
    if (tfs) memcpy(tfs, d->tfs, (size_t)d->n_entries * 2);
    if (norms) memcpy(norms, d->norms, (size_t)d->n_images * 4);
    if (df) memcpy(df, d->df, (size_t)d->K * 4);
    if (weights) memcpy(weights, d->weight, (size_t)d->K * 4);
}
