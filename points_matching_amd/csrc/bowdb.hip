// bowdb.hip — the image database on top of the bag-of-words histogram (docs/SPEC.md S107-S112): an append-only forward
// index of (word, tf) entries, tf-idf weights, DBoW2's L1 score kept exact in integers, and an exact top-N selection.
//
//   bow_add        one 1024-thread workgroup.  Each wave owns a contiguous stretch of the K words and walks it 64 words at a
//                  time: the first walk gives T, nnz and the norm, the block combines the sixteen waves and decides
//                  (accepted, -1, -2), the second walk appends the non-zero words in ascending order behind the entry cursor
//                  (position = cursor + the count of set ballot bits below the lane) and raises their df.  One writer per
//                  word and per entry: no atomics.
//   bow_idf        one thread per word: S109's ilog2_q8 of the image count and df.
//   bow_norms      one wave per image: Nd = sum tf * weight[w]; after a change of the weights.
//   bow_query_vec  one 1024-thread workgroup: the dense table {q_w, weight[w]} (8 bytes per word, at most 2 MiB: it stays in
//                  an XCD's L2), T and Nq.  A refused query (T = 0 or T > 65535) leaves Nq = 0 and every score becomes 0.
//   bow_score      the hot path.  One wave per image, a fixed grid striding the images below the device-side count; lanes
//                  stride the image's entries four wave-widths at a time (a 4-byte and a 2-byte coalesced load each), gather
//                  the 8-byte table entry, form q_w * Nd and d_w * Nq in u64, min, add; a u64 butterfly over the wave and
//                  one fp64 division per image.
//   bow_top        exact selection under (score descending, id ascending).  A 1024-thread workgroup streams its slice of
//                  the scores, keeps the candidates that beat its current top-th key in a 2048-key LDS buffer and, when the
//                  buffer could overflow, sorts it (bitonic, 96-bit keys: the score's bits, then ~id) and keeps the first
//                  `top`.  The keys are distinct, so the first `top` of a set do not depend on the order they were met in.
//                  Up to 32768 images (of max_images) one workgroup does it all; above, up to 64 workgroups each leave their
//                  slice's first `top` keys in scratch and a second launch selects among those.
//
// A pm_bowdb owns one device block; pm_bowdb_create is the only allocation of the _dev path.
#include <new>

#include "pm_common.hpp"
#include "wave_ops.hpp"

namespace {

constexpr int BW_MAX_K = 262144;
constexpr int BW_MAX_IMAGES = 1 << 22;
constexpr int BW_MAX_ENTRIES = 1 << 28;
constexpr unsigned BW_MAX_T = 65535;
constexpr unsigned BW_MAX_WEIGHT = 8191;
constexpr int BW_MAX_TOP = 256;
constexpr int BW_WG = 1024;                        // bow_add, bow_query_vec, bow_top: one workgroup of 16 waves
constexpr int BW_BUF = 2048;                       // keys of the selection buffer
constexpr int BW_SLICE = 32768;                    // images per selection workgroup before a second one is worth its launch
constexpr int BW_MAX_SLICES = 64;
constexpr unsigned long long BW_QNAN = 0x7FF8000000000000ull;

struct BwScalars {
    unsigned n_images, n_entries;
    unsigned Nq, pad;                              // Nq of the last query: 0 when it was refused
};

// the stretch of words of wave `wv` of 16: whole groups of 64, so that every ballot below sees 64 lanes
__device__ __forceinline__ void bw_stretch(int K, int wv, int& lo, int& hi)
{
    const int per = (((K + 15) >> 4) + 63) & ~63;
    lo = min(K, wv * per);
    hi = min(K, lo + per);
}

__global__ __launch_bounds__(BW_WG) void bow_add(const uint32_t* __restrict__ hist, int K, unsigned max_images, unsigned max_entries,
                                                 BwScalars* __restrict__ sc, uint32_t* __restrict__ offsets, uint32_t* __restrict__ norms,
                                                 uint32_t* __restrict__ words, uint16_t* __restrict__ tfs, uint32_t* __restrict__ df,
                                                 const uint32_t* __restrict__ weight, int32_t* __restrict__ d_id)
{
    __shared__ unsigned long long s_T[16], s_norm[16];
    __shared__ unsigned s_nnz[16];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned n_img = sc->n_images, n_ent = sc->n_entries;
    int lo, hi;
    bw_stretch(K, wv, lo, hi);
    unsigned long long T = 0, norm = 0;
    unsigned nnz = 0;
    for (int b = lo; b < hi; b += 64) {
        const int w = b + lane;
        if (w < hi) {
            const unsigned h = hist[w];
            T += h;
            norm += static_cast<unsigned long long>(h) * weight[w];
            nnz += h != 0;
        }
    }
    T = pm::wave_sum_u64(T);
    norm = pm::wave_sum_u64(norm);
    nnz = pm::wave_sum_u32(nnz);
    if (lane == 0) { s_T[wv] = T; s_norm[wv] = norm; s_nnz[wv] = nnz; }
    __syncthreads();
    unsigned long long T_all = 0, norm_all = 0;
    unsigned nnz_all = 0, before = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        T_all += s_T[i];
        norm_all += s_norm[i];
        if (i < wv) before += s_nnz[i];
        nnz_all += s_nnz[i];
    }
    int id;
    if (T_all == 0 || T_all > BW_MAX_T) id = -1;
    else if (n_img >= max_images || static_cast<unsigned long long>(n_ent) + nnz_all > max_entries) id = -2;
    else id = static_cast<int>(n_img);
    if (id >= 0) {
        unsigned cursor = n_ent + before;
        for (int b = lo; b < hi; b += 64) {
            const int w = b + lane;
            const unsigned h = w < hi ? hist[w] : 0u;
            const unsigned long long mask = __ballot(h != 0);
            if (h != 0) {
                const unsigned pos = cursor + static_cast<unsigned>(pm::lane_rank(mask, lane));
                words[pos] = static_cast<uint32_t>(w);
                tfs[pos] = static_cast<uint16_t>(h);
                df[w] += 1;
            }
            cursor += static_cast<unsigned>(__popcll(mask));
        }
    }
    __syncthreads();                                                  // every thread has read the scalars
    if (threadIdx.x == 0) {
        if (id >= 0) {
            offsets[n_img + 1] = n_ent + nnz_all;
            norms[n_img] = static_cast<uint32_t>(norm_all);           // T <= 65535 and weights <= 8191: below 2^29
            sc->n_images = n_img + 1;
            sc->n_entries = n_ent + nnz_all;
        }
        if (d_id) *d_id = id;
    }
}

// S109: floor(256 * log2(N / d)) for 1 <= d <= N <= 2^22 by eight squarings of the Q30 mantissa
__device__ __forceinline__ unsigned bw_ilog2_q8(unsigned N, unsigned d)
{
    unsigned e = 0;
    while ((static_cast<unsigned long long>(d) << (e + 1)) <= N) ++e;
    unsigned long long m = (static_cast<unsigned long long>(N) << 30) / (static_cast<unsigned long long>(d) << e);
    unsigned f = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        m = (m * m) >> 30;
        f <<= 1;
        if (m >= (1ull << 31)) { f |= 1u; m >>= 1; }
    }
    return (e << 8) | f;
}

__global__ __launch_bounds__(256) void bow_idf(const BwScalars* __restrict__ sc, const uint32_t* __restrict__ df, uint32_t* __restrict__ weight, int K)
{
    const int w = blockIdx.x * 256 + threadIdx.x;
    const unsigned N = sc->n_images;
    if (w >= K || N == 0) return;
    const unsigned d = df[w];
    weight[w] = bw_ilog2_q8(N, d < 1 ? 1u : (d > N ? N : d));       // (df <= N by construction)
}

__global__ __launch_bounds__(256) void bow_norms(const BwScalars* __restrict__ sc, const uint32_t* __restrict__ offsets,
                                                 const uint32_t* __restrict__ words, const uint16_t* __restrict__ tfs,
                                                 const uint32_t* __restrict__ weight, uint32_t* __restrict__ norms)
{
    const int lane = threadIdx.x & 63;
    const unsigned N = sc->n_images, nwaves = gridDim.x * 4;
    for (unsigned i = blockIdx.x * 4 + (threadIdx.x >> 6); i < N; i += nwaves) {
        const unsigned off = offsets[i], end = offsets[i + 1];
        unsigned s = 0;
        for (unsigned e = off + lane; e < end; e += 64) s += static_cast<unsigned>(tfs[e]) * weight[words[e]];
        s = pm::wave_sum_u32(s);
        if (lane == 0) norms[i] = s;
    }
}

__global__ __launch_bounds__(BW_WG) void bow_query_vec(const uint32_t* __restrict__ hist, int K, const uint32_t* __restrict__ weight,
                                                       uint2* __restrict__ qw, BwScalars* __restrict__ sc)
{
    __shared__ unsigned long long s_T[16], s_Nq[16];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int lo, hi;
    bw_stretch(K, wv, lo, hi);
    unsigned long long T = 0, Nq = 0;
    for (int b = lo; b < hi; b += 64) {
        const int w = b + lane;
        if (w < hi) {
            const unsigned h = hist[w], wt = weight[w];
            const unsigned long long q = static_cast<unsigned long long>(h) * wt;
            T += h;
            Nq += q;
            qw[w] = make_uint2(static_cast<unsigned>(q), wt);        // (exact whenever the query is accepted)
        }
    }
    T = pm::wave_sum_u64(T);
    Nq = pm::wave_sum_u64(Nq);
    if (lane == 0) { s_T[wv] = T; s_Nq[wv] = Nq; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long T_all = 0, Nq_all = 0;
        for (int i = 0; i < 16; ++i) { T_all += s_T[i]; Nq_all += s_Nq[i]; }
        const bool ok = T_all >= 1 && T_all <= BW_MAX_T;
        sc->Nq = ok ? static_cast<unsigned>(Nq_all) : 0u;
    }
}

__global__ __launch_bounds__(256) void bow_score(const BwScalars* __restrict__ sc, const uint32_t* __restrict__ offsets,
                                                 const uint32_t* __restrict__ norms, const uint32_t* __restrict__ words,
                                                 const uint16_t* __restrict__ tfs, const uint2* __restrict__ qw,
                                                 double* __restrict__ scores, double* __restrict__ d_all)
{
    const int lane = threadIdx.x & 63;
    const unsigned N = sc->n_images, nwaves = gridDim.x * 4;
    const unsigned long long Nq = sc->Nq;
    for (unsigned i = blockIdx.x * 4 + (threadIdx.x >> 6); i < N; i += nwaves) {
        const unsigned off = offsets[i], end = offsets[i + 1];
        const unsigned long long Nd = norms[i];
        const bool live = Nq != 0 && Nd != 0;                         // wave-uniform
        unsigned long long S = 0;
        if (live) {
            for (unsigned b = off; b < end; b += 256) {
                unsigned w[4], tf[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {                         // four steps' loads in flight together
                    const unsigned e = b + u * 64 + lane;
                    const bool ok = e < end;
                    w[u] = ok ? words[e] : 0u;
                    tf[u] = ok ? static_cast<unsigned>(tfs[e]) : 0u;  // tf 0: the term is min(.., 0) = 0
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint2 t = qw[w[u]];
                    const unsigned long long a = static_cast<unsigned long long>(t.x) * Nd;
                    const unsigned long long d = static_cast<unsigned long long>(tf[u] * t.y) * Nq;
                    S += a < d ? a : d;
                }
            }
            S = pm::wave_sum_u64(S);
        }
        if (lane == 0) {
            const double s = live ? static_cast<double>(S) / static_cast<double>(Nq * Nd) : 0.0;
            scores[i] = s;
            if (d_all) d_all[i] = s;
        }
    }
}

// key order: the score's bits (scores are >= 0, so the bits order as the values do), then ~id.  (0, 0) is below every candidate.
__device__ __forceinline__ bool bw_above(unsigned long long ah, unsigned al, unsigned long long bh, unsigned bl)
{
    return ah > bh || (ah == bh && al > bl);
}

// sorts the 2048 keys descending, keeps the first `top`; returns the new count, thr = the top-th key or (0, 0)
__device__ __forceinline__ unsigned bw_sort_keep(unsigned long long* kh, unsigned* kl, unsigned cnt, unsigned top,
                                                  unsigned long long& thr_h, unsigned& thr_l)
{
    const unsigned t = threadIdx.x;
    for (unsigned i = t; i < BW_BUF; i += BW_WG)
        if (i >= cnt) { kh[i] = 0; kl[i] = 0; }
    __syncthreads();
    for (unsigned k = 2; k <= BW_BUF; k <<= 1) {
        for (unsigned j = k >> 1; j > 0; j >>= 1) {
            const unsigned a = ((t & ~(j - 1)) << 1) | (t & (j - 1)), b = a + j;
            const unsigned long long ah = kh[a], bh = kh[b];
            const unsigned al = kl[a], bl = kl[b];
            const bool desc = (a & k) == 0;
            if (bw_above(bh, bl, ah, al) == desc) { kh[a] = bh; kl[a] = bl; kh[b] = ah; kl[b] = al; }
            __syncthreads();
        }
    }
    const unsigned kept = cnt < top ? cnt : top;
    thr_h = 0; thr_l = 0;
    if (kept == top) { thr_h = kh[top - 1]; thr_l = kl[top - 1]; }
    __syncthreads();
    return kept;
}

// FROM_SCORES: the elements are the images of this workgroup's slice, candidates those with a positive score outside
// [excl_lo, excl_hi).  Otherwise: the n_part keys that the sliced launch left.  `final`: write the caller's outputs, else
// this workgroup's 256 keys of scratch.
template <bool FROM_SCORES>
__global__ __launch_bounds__(BW_WG) void bow_top(const BwScalars* __restrict__ sc, const double* __restrict__ scores, int excl_lo, int excl_hi,
                                                 unsigned long long* __restrict__ part_h, unsigned* __restrict__ part_l, unsigned n_part,
                                                 unsigned top, int final, int32_t* __restrict__ d_ids, double* __restrict__ d_scores,
                                                 int32_t* __restrict__ d_count)
{
    __shared__ unsigned long long kh[BW_BUF];
    __shared__ unsigned kl[BW_BUF];
    __shared__ unsigned wcnt[16];
    const unsigned t = threadIdx.x, lane = t & 63, wv = t >> 6;
    unsigned lo = 0, hi = n_part;
    if (FROM_SCORES) {
        const unsigned N = sc->n_images;
        const unsigned per = (N + gridDim.x - 1) / gridDim.x;
        lo = min(N, blockIdx.x * per);
        hi = min(N, lo + per);
    }
    unsigned cnt = 0, thr_l = 0;
    unsigned long long thr_h = 0;
    for (unsigned b = lo; b < hi; b += 4 * BW_WG) {
        unsigned long long eh[4];
        unsigned el[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const unsigned i = b + u * BW_WG + t;
            eh[u] = 0; el[u] = 0;
            if (i < hi) {
                if (FROM_SCORES) {
                    const bool excluded = static_cast<int>(i) >= excl_lo && static_cast<int>(i) < excl_hi;
                    eh[u] = excluded ? 0ull : static_cast<unsigned long long>(__double_as_longlong(scores[i]));
                    el[u] = 0xFFFFFFFFu - i;
                } else {
                    eh[u] = part_h[i];
                    el[u] = part_l[i];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (cnt > BW_BUF - BW_WG) cnt = bw_sort_keep(kh, kl, cnt, top, thr_h, thr_l);      // uniform
            const bool pass = eh[u] != 0 && bw_above(eh[u], el[u], thr_h, thr_l);
            const unsigned long long mask = __ballot(pass);
            if (lane == 0) wcnt[wv] = static_cast<unsigned>(__popcll(mask));
            const unsigned total = static_cast<unsigned>(__syncthreads_count(pass));
            if (total == 0) continue;                                 // uniform; nobody read wcnt
            if (pass) {
                unsigned pos = cnt + static_cast<unsigned>(pm::lane_rank(mask, lane));
                for (unsigned i = 0; i < wv; ++i) pos += wcnt[i];
                kh[pos] = eh[u];
                kl[pos] = el[u];
            }
            cnt += total;
            __syncthreads();
        }
    }
    cnt = bw_sort_keep(kh, kl, cnt, top, thr_h, thr_l);
    if (final) {
        if (t < top) {
            const bool have = t < cnt;
            if (d_ids) d_ids[t] = have ? static_cast<int32_t>(0xFFFFFFFFu - kl[t]) : -1;
            if (d_scores) d_scores[t] = __longlong_as_double(static_cast<long long>(have ? kh[t] : BW_QNAN));
        }
        if (t == 0 && d_count) *d_count = static_cast<int32_t>(cnt);
    } else if (t < BW_MAX_TOP) {
        const bool have = t < cnt;
        part_h[blockIdx.x * BW_MAX_TOP + t] = have ? kh[t] : 0ull;
        part_l[blockIdx.x * BW_MAX_TOP + t] = have ? kl[t] : 0u;
    }
}

}  // namespace

struct pm_bowdb {
    int device = 0;
    int K = 0, max_images = 0, max_entries = 0;
    char* mem = nullptr;              // the one device block
    BwScalars* sc = nullptr;
    uint32_t* offsets = nullptr;      // max_images + 1; offsets[0] = 0
    uint32_t* norms = nullptr;        // max_images
    double* scores = nullptr;         // max_images: the last query's
    uint32_t* words = nullptr;        // max_entries
    uint16_t* tfs = nullptr;          // max_entries
    uint32_t* df = nullptr;           // K
    uint32_t* weight = nullptr;       // K
    uint2* qw = nullptr;              // K: {q_w, weight[w]} of the last query
    unsigned long long* part_h = nullptr;   // 64 x 256 keys of the sliced selection
    unsigned* part_l = nullptr;
    size_t b_zero = 0;                // scalars, offsets: what create clears
};

namespace {

#define BW_REQUIRE_OBJECT(ctx_, db_)                                                                                    \
    do {                                                                                                                \
        PM_REQUIRE((ctx_) != nullptr, PM_E_INVALID, "ctx is null");                                                     \
        PM_REFUSE_CAPTURE(ctx_);                                                                                        \
        PM_REQUIRE((db_)->device == (ctx_)->device, PM_E_INVALID, "database of another device");                        \
        PM_HIP_CHECK(hipSetDevice((ctx_)->device));                                                                     \
    } while (0)

inline unsigned image_grid(const pm_ctx* ctx, const pm_bowdb* db)
{
    const long long want = (static_cast<long long>(db->max_images) + 3) / 4, cap = static_cast<long long>(ctx->n_cu) * 8;
    return static_cast<unsigned>(want < cap ? want : cap);
}

int launch_norms(pm_ctx* ctx, pm_bowdb* db)
{
    hipLaunchKernelGGL(bow_norms, dim3(image_grid(ctx, db)), dim3(256), 0, ctx->stream, db->sc, db->offsets, db->words, db->tfs, db->weight, db->norms);
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

__global__ void bow_fill_u32(uint32_t* p, int n, uint32_t v)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

}  // namespace

extern "C" int pm_bowdb_create(pm_ctx* ctx, int K, int max_images, int max_entries, pm_bowdb** out)
{
    PM_REQUIRE(out != nullptr, PM_E_INVALID, "null output pointer");
    *out = nullptr;
    PM_REQUIRE(K >= 1 && K <= BW_MAX_K, PM_E_INVALID, "need 1 <= K <= 262144");
    PM_REQUIRE(max_images >= 1 && max_images <= BW_MAX_IMAGES, PM_E_INVALID, "need 1 <= max_images <= 2^22");
    PM_REQUIRE(max_entries >= 1 && max_entries <= BW_MAX_ENTRIES, PM_E_INVALID, "need 1 <= max_entries <= 2^28");
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    pm_bowdb* db = new (std::nothrow) pm_bowdb;
    PM_REQUIRE(db != nullptr, PM_E_NOMEM, "out of host memory");
    db->device = ctx->device; db->K = K; db->max_images = max_images; db->max_entries = max_entries;
    const size_t NI = static_cast<size_t>(max_images), NE = static_cast<size_t>(max_entries), NK = static_cast<size_t>(K);
    const size_t b_sc = 256, b_off = pm::align_up((NI + 1) * 4, 256), b_norm = pm::align_up(NI * 4, 256), b_score = pm::align_up(NI * 8, 256);
    const size_t b_words = pm::align_up(NE * 4, 256), b_tfs = pm::align_up(NE * 2, 256), b_k = pm::align_up(NK * 4, 256), b_qw = pm::align_up(NK * 8, 256);
    const size_t b_ph = static_cast<size_t>(BW_MAX_SLICES) * BW_MAX_TOP * 8, b_pl = static_cast<size_t>(BW_MAX_SLICES) * BW_MAX_TOP * 4;
    const size_t total = b_sc + b_off + b_norm + b_score + b_words + b_tfs + 2 * b_k + b_qw + b_ph + b_pl;
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&db->mem), total);
    if (e != hipSuccess) {
        pm::set_error("pm_bowdb_create: hipMalloc of %zu bytes failed: %s", total, hipGetErrorString(e));
        delete db;
        return PM_E_NOMEM;
    }
    char* p = db->mem;
    db->sc = reinterpret_cast<BwScalars*>(p); p += b_sc;
    db->offsets = reinterpret_cast<uint32_t*>(p); p += b_off;
    db->df = reinterpret_cast<uint32_t*>(p); p += b_k;
    db->weight = reinterpret_cast<uint32_t*>(p); p += b_k;
    db->norms = reinterpret_cast<uint32_t*>(p); p += b_norm;
    db->scores = reinterpret_cast<double*>(p); p += b_score;
    db->qw = reinterpret_cast<uint2*>(p); p += b_qw;
    db->part_h = reinterpret_cast<unsigned long long*>(p); p += b_ph;
    db->part_l = reinterpret_cast<unsigned*>(p); p += b_pl;
    db->words = reinterpret_cast<uint32_t*>(p); p += b_words;
    db->tfs = reinterpret_cast<uint16_t*>(p);
    db->b_zero = b_sc + b_off + b_k;
    // counts, offsets and df start at zero, weights at 1
    e = hipMemsetAsync(db->mem, 0, db->b_zero, ctx->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(bow_fill_u32, dim3(static_cast<unsigned>((K + 255) / 256)), dim3(256), 0, ctx->stream, db->weight, K, 1u);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        pm::set_error("pm_bowdb_create: clearing the block failed: %s", hipGetErrorString(e));
        (void)hipFree(db->mem);
        delete db;
        return PM_E_HIP;
    }
    *out = db;
    return PM_OK;
}

extern "C" int pm_bowdb_destroy(pm_bowdb* db)
{
    if (!db) return PM_OK;
    int rc = PM_OK;
    if (db->mem && (hipSetDevice(db->device) != hipSuccess || hipFree(db->mem) != hipSuccess)) rc = PM_E_HIP;
    delete db;
    return rc;
}

extern "C" int pm_bowdb_clear_dev(pm_ctx* ctx, pm_bowdb* db)
{
    PM_REQUIRE(db != nullptr, PM_E_INVALID, "null argument");
    BW_REQUIRE_OBJECT(ctx, db);
    PM_HIP_CHECK(hipMemsetAsync(db->mem, 0, db->b_zero, ctx->stream));    // counts, offsets, df; the weights stay
    return PM_OK;
}

extern "C" int pm_bowdb_add_dev(pm_ctx* ctx, pm_bowdb* db, const uint32_t* d_hist, int32_t* d_id)
{
    PM_REQUIRE(db != nullptr && d_hist != nullptr, PM_E_INVALID, "null argument");
    BW_REQUIRE_OBJECT(ctx, db);
    pm::ScopedKernelTime t(ctx, "bow_add");
    hipLaunchKernelGGL(bow_add, dim3(1), dim3(BW_WG), 0, ctx->stream, d_hist, db->K, static_cast<unsigned>(db->max_images),
                       static_cast<unsigned>(db->max_entries), db->sc, db->offsets, db->norms, db->words, db->tfs, db->df, db->weight, d_id);
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_bowdb_add(pm_ctx* ctx, pm_bowdb* db, const uint32_t* hist, int32_t* id)
{
    PM_REQUIRE(db != nullptr && hist != nullptr, PM_E_INVALID, "null argument");
    BW_REQUIRE_OBJECT(ctx, db);
    const size_t hb = static_cast<size_t>(db->K) * 4;
    pm::StagedBlock b(ctx, "pm_bowdb_add");
    const size_t o_h = b.add(hb), o_id = b.add(4);
    b.alloc();
    b.upload(o_h, hist, hb);
    if (b.rc == PM_OK) b.rc = pm_bowdb_add_dev(ctx, db, b.at<const uint32_t>(o_h), b.at<int32_t>(o_id));
    if (id) b.download(id, o_id, 4);
    return b.sync();
}

extern "C" int pm_bowdb_set_weights(pm_ctx* ctx, pm_bowdb* db, const uint32_t* weights)
{
    PM_REQUIRE(db != nullptr && weights != nullptr, PM_E_INVALID, "null argument");
    for (int w = 0; w < db->K; ++w) PM_REQUIRE(weights[w] <= BW_MAX_WEIGHT, PM_E_INVALID, "a weight above 8191");
    BW_REQUIRE_OBJECT(ctx, db);
    PM_HIP_CHECK(hipMemcpyAsync(db->weight, weights, static_cast<size_t>(db->K) * 4, hipMemcpyHostToDevice, ctx->stream));
    {
        pm::ScopedKernelTime t(ctx, "bow_norms");
        const int rc = launch_norms(ctx, db);
        if (rc != PM_OK) return rc;
    }
    PM_HIP_CHECK(hipStreamSynchronize(ctx->stream));                   // the caller's buffer is free again on return
    return PM_OK;
}

extern "C" int pm_bowdb_get_weights(pm_ctx* ctx, const pm_bowdb* db, uint32_t* weights)
{
    PM_REQUIRE(db != nullptr && weights != nullptr, PM_E_INVALID, "null argument");
    BW_REQUIRE_OBJECT(ctx, db);
    PM_HIP_CHECK(hipMemcpyAsync(weights, db->weight, static_cast<size_t>(db->K) * 4, hipMemcpyDeviceToHost, ctx->stream));
    PM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PM_OK;
}

extern "C" int pm_bowdb_idf_dev(pm_ctx* ctx, pm_bowdb* db)
{
    PM_REQUIRE(db != nullptr, PM_E_INVALID, "null argument");
    BW_REQUIRE_OBJECT(ctx, db);
    {
        pm::ScopedKernelTime t(ctx, "bow_idf");
        hipLaunchKernelGGL(bow_idf, dim3(static_cast<unsigned>((db->K + 255) / 256)), dim3(256), 0, ctx->stream, db->sc, db->df, db->weight, db->K);
        PM_HIP_CHECK(hipGetLastError());
    }
    pm::ScopedKernelTime t(ctx, "bow_norms");
    return launch_norms(ctx, db);
}

extern "C" int pm_bowdb_query_dev(pm_ctx* ctx, pm_bowdb* db, const uint32_t* d_hist, int top, int excl_lo, int excl_hi, int32_t* d_ids,
                                  double* d_scores, int32_t* d_count, double* d_all)
{
    PM_REQUIRE(db != nullptr && d_hist != nullptr, PM_E_INVALID, "null argument");
    PM_REQUIRE(top >= 1 && top <= BW_MAX_TOP, PM_E_INVALID, "need 1 <= top <= 256");
    BW_REQUIRE_OBJECT(ctx, db);
    {
        pm::ScopedKernelTime t(ctx, "bow_query_vec");
        hipLaunchKernelGGL(bow_query_vec, dim3(1), dim3(BW_WG), 0, ctx->stream, d_hist, db->K, db->weight, db->qw, db->sc);
    }
    {
        pm::ScopedKernelTime t(ctx, "bow_score");
        hipLaunchKernelGGL(bow_score, dim3(image_grid(ctx, db)), dim3(256), 0, ctx->stream, db->sc, db->offsets, db->norms, db->words, db->tfs,
                           db->qw, db->scores, d_all);
    }
    if (d_ids || d_scores || d_count) {
        pm::ScopedKernelTime t(ctx, "bow_top");
        int slices = (db->max_images + BW_SLICE - 1) / BW_SLICE;
        if (slices > BW_MAX_SLICES) slices = BW_MAX_SLICES;
        const unsigned utop = static_cast<unsigned>(top);
        if (slices == 1) {
            hipLaunchKernelGGL(bow_top<true>, dim3(1), dim3(BW_WG), 0, ctx->stream, db->sc, db->scores, excl_lo, excl_hi, db->part_h, db->part_l, 0u,
                               utop, 1, d_ids, d_scores, d_count);
        } else {
            hipLaunchKernelGGL(bow_top<true>, dim3(slices), dim3(BW_WG), 0, ctx->stream, db->sc, db->scores, excl_lo, excl_hi, db->part_h, db->part_l, 0u,
                               utop, 0, static_cast<int32_t*>(nullptr), static_cast<double*>(nullptr), static_cast<int32_t*>(nullptr));
            hipLaunchKernelGGL(bow_top<false>, dim3(1), dim3(BW_WG), 0, ctx->stream, db->sc, db->scores, excl_lo, excl_hi, db->part_h, db->part_l,
                               static_cast<unsigned>(slices * BW_MAX_TOP), utop, 1, d_ids, d_scores, d_count);
        }
    }
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_bowdb_query(pm_ctx* ctx, pm_bowdb* db, const uint32_t* hist, int top, int excl_lo, int excl_hi, int32_t* ids, double* scores,
                              int32_t* count, double* all)
{
    PM_REQUIRE(db != nullptr && hist != nullptr, PM_E_INVALID, "null argument");
    PM_REQUIRE(top >= 1 && top <= BW_MAX_TOP, PM_E_INVALID, "need 1 <= top <= 256");
    BW_REQUIRE_OBJECT(ctx, db);
    uint32_t n_images = 0;
    if (all) {                                                         // how many scores there will be
        PM_HIP_CHECK(hipMemcpyAsync(&n_images, &db->sc->n_images, 4, hipMemcpyDeviceToHost, ctx->stream));
        PM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    const size_t hb = static_cast<size_t>(db->K) * 4, ib = ids ? static_cast<size_t>(top) * 4 : 0, sb = scores ? static_cast<size_t>(top) * 8 : 0;
    const size_t cb = count ? 4 : 0, ab = static_cast<size_t>(n_images) * 8;
    pm::StagedBlock b(ctx, "pm_bowdb_query");
    const size_t o_all = b.add(ab), o_s = b.add(sb), o_h = b.add(hb), o_i = b.add(ib), o_c = b.add(cb);
    b.alloc();
    b.upload(o_h, hist, hb);
    if (b.rc == PM_OK)
        b.rc = pm_bowdb_query_dev(ctx, db, b.at<const uint32_t>(o_h), top, excl_lo, excl_hi, ids ? b.at<int32_t>(o_i) : nullptr,
                                  scores ? b.at<double>(o_s) : nullptr, count ? b.at<int32_t>(o_c) : nullptr, ab ? b.at<double>(o_all) : nullptr);
    b.download(ids, o_i, ib);
    b.download(scores, o_s, sb);
    b.download(count, o_c, cb);
    b.download(all, o_all, ab);
    return b.sync();
}

extern "C" int pm_bowdb_get(pm_ctx* ctx, const pm_bowdb* db, int32_t* n_images, int32_t* n_entries, uint32_t* offsets, uint32_t* words,
                            uint16_t* tfs, uint32_t* norms, uint32_t* df, uint32_t* weights)
{
    PM_REQUIRE(db != nullptr, PM_E_INVALID, "null argument");
    BW_REQUIRE_OBJECT(ctx, db);
    BwScalars s;
    PM_HIP_CHECK(hipMemcpyAsync(&s, db->sc, sizeof(s), hipMemcpyDeviceToHost, ctx->stream));
    PM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    const size_t N = s.n_images, E = s.n_entries, NK = static_cast<size_t>(db->K);
    if (n_images) *n_images = static_cast<int32_t>(N);
    if (n_entries) *n_entries = static_cast<int32_t>(E);
    if (offsets) PM_HIP_CHECK(hipMemcpyAsync(offsets, db->offsets, (N + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (words && E) PM_HIP_CHECK(hipMemcpyAsync(words, db->words, E * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (tfs && E) PM_HIP_CHECK(hipMemcpyAsync(tfs, db->tfs, E * 2, hipMemcpyDeviceToHost, ctx->stream));
    if (norms && N) PM_HIP_CHECK(hipMemcpyAsync(norms, db->norms, N * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (df) PM_HIP_CHECK(hipMemcpyAsync(df, db->df, NK * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (weights) PM_HIP_CHECK(hipMemcpyAsync(weights, db->weight, NK * 4, hipMemcpyDeviceToHost, ctx->stream));
    PM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PM_OK;
}
