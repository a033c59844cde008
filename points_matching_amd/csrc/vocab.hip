// vocab.hip — visual vocabularies (docs/SPEC.md S102-S106): k-means on u8 rows and k-majority on bit rows, and the
// bag-of-words encoding of a set of rows.  The quantiser is the brute-force matcher with the vocabulary as its train set
// (pm_bf_knn_l2_u8_dev / pm_bf_knn_hamming_u8_dev, k = 1); what lives here is everything around that call:
//
//   vocab_init     word i <- row floor(i * n / K): a gather, one thread per dword.
//   vocab_update   the scatter-reduction of one iteration.  A wave takes 64 rows with their matcher records, orders them
//                  by label (a 64-key bitonic sort of label << 6 | lane), then walks the sorted rows with the running sums
//                  of the current label in registers and flushes them with integer atomics once per run of equal labels.
//                  u8 rows: a lane owns a dword of the row (four byte sums); 64 / (bytes / 4) rows go side by side, each
//                  lane group walking its own stretch of the sorted order.  The accumulators of a word are stored plane-
//                  major ([4][bytes / 4]), so one atomic instruction of a lane group covers bytes contiguous bytes: 256 B
//                  for 256-byte rows, two 128-B segments for 128-byte rows.  Bit rows: a lane owns bits lane, 64 + lane, ...
//                  (ceil(bits / 64) counters), one row per step, each atomic instruction 256 contiguous bytes.
//                  Integer sums do not depend on arrival order, so no ordering protocol is needed.  The same pass compares
//                  the labels with the previous iteration's, stores them, and adds n_changed and the cost once per wave.
//   vocab_finish   one thread per dword of a word: S104's rounded mean / majority, the new bytes, n_empty and n_moved, and
//                  every accumulator and count back to zero; then a one-thread launch under the same timing name writes the
//                  iteration record and returns the four running scalars to zero (a kernel boundary is the hand-off: no
//                  in-launch ticket between workgroups).
//   vocab_hist     labels, distances and the histogram of the rows below the device count: one atomic per distinct word
//                  of a wave; -1 / NaN tails.
//
// A pm_vocab owns one device block: words, accumulators, counts, the matcher's records for max_rows rows, the previous
// labels and the scalars.  The _dev calls run the matcher, which resets the context's arena, so none of this is carved there.
#include <new>

#include "pm_common.hpp"
#include "wave_ops.hpp"

namespace {

constexpr int VC_MAX_K = 262144;
constexpr int VC_MAX_ROWS = 1 << 24;           // 255 * 2^24 < 2^32: a u32 byte sum cannot overflow
constexpr int VC_MAX_ITERS = 1000;
constexpr unsigned VC_NO_KEY = 0xFFFFFFC0u;    // sort key of a lane without a row (| lane): behind every label
constexpr unsigned VC_NONE = 0xFFFFFFFFu;

struct VcScalars {                             // running sums of one iteration; all zero between iterations
    unsigned n_changed, n_empty, n_moved, pad;
    unsigned long long cost, pad2;
};
static_assert(sizeof(VcScalars) == 32, "scalar block");
static_assert(sizeof(pm_vocab_iter) == 24, "iteration record");

__global__ __launch_bounds__(256) void vocab_init(const uint32_t* __restrict__ rows, int n, uint32_t* __restrict__ words, int K, int W)
{
    const long long t = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (t >= static_cast<long long>(K) * W) return;
    const int w = static_cast<int>(t / W), j = static_cast<int>(t - static_cast<long long>(w) * W);
    const long long r = static_cast<long long>(w) * n / K;
    words[t] = rows[r * W + j];
}

// ascending bitonic sort of one distinct key per lane
__device__ __forceinline__ unsigned vc_sort64(unsigned key, int lane)
{
#pragma unroll
    for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            const unsigned other = static_cast<unsigned>(__shfl_xor(static_cast<int>(key), j, 64));
            const bool up = (lane & k) == 0, low = (lane & j) == 0;
            key = (up == low) ? min(key, other) : max(key, other);
        }
    }
    return key;
}

// KIND 0: u8 rows, squared L2.  KIND 1: bit rows, Hamming.  W = dwords per row (1 .. 64; bit rows 1 .. 16).
template <int KIND>
__global__ __launch_bounds__(256) void vocab_update(const pm_match* __restrict__ rec, const uint32_t* __restrict__ rows,
                                                    const uint32_t* __restrict__ words, int n, int K, int W, int first,
                                                    int32_t* __restrict__ labels, int32_t* __restrict__ labels_out,
                                                    unsigned* __restrict__ acc, unsigned* __restrict__ count, VcScalars* __restrict__ sc)
{
    const int lane = threadIdx.x & 63;
    const int base = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;      // first row of this wave; n <= 2^24
    if (base >= n) return;                                            // whole waves only: every shuffle below sees 64 lanes
    const int i = base + lane;
    const bool have = i < n;
    int lab = -1;
    unsigned cost = 0;
    bool changed = false;
    if (have) {
        const pm_match m = rec[i];
        lab = m.trainIdx;
        if (KIND == 1) cost = static_cast<unsigned>(m.distance);      // the bit count, exact in the float
        changed = first || labels[i] != lab;
        labels[i] = lab;
        if (labels_out) labels_out[i] = lab;
    }
    const bool ok = have && lab >= 0 && lab < K;                      // (the matcher gives nothing else; never index past K)
    const unsigned n_changed = static_cast<unsigned>(__popcll(__ballot(changed)));
    const unsigned key = vc_sort64(ok ? (static_cast<unsigned>(lab) << 6) | lane : VC_NO_KEY | lane, lane);

    if (KIND == 0) {
        const int rpi = 64 / W;                                       // rows side by side in one wave-instruction
        const int g = lane / W, j = lane - g * W;
        const int S = (64 + rpi - 1) / rpi;                           // sorted rows per lane group
        const bool act = g < rpi;
        unsigned s0 = 0, s1 = 0, s2 = 0, s3 = 0, cnt = 0, cur = VC_NONE;
        auto flush = [&]() {
            if (cur != VC_NONE && cnt) {
                unsigned* a = acc + static_cast<size_t>(cur) * (4 * W) + j;
                atomicAdd(a, s0);
                atomicAdd(a + W, s1);
                atomicAdd(a + 2 * W, s2);
                atomicAdd(a + 3 * W, s3);
                if (j == 0) atomicAdd(count + cur, cnt);
            }
        };
        for (int t0 = 0; t0 < S; t0 += 4) {
            unsigned kk[4], rv[4], wv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {                             // four steps' loads in flight together
                const int p = g * S + t0 + u;
                const unsigned k = static_cast<unsigned>(__shfl(static_cast<int>(key), p & 63, 64));
                const bool v = act && t0 + u < S && p < 64 && k < VC_NO_KEY;
                kk[u] = v ? k : VC_NONE;
                rv[u] = 0; wv[u] = 0;
                if (v) {
                    rv[u] = rows[static_cast<size_t>(base + (k & 63)) * W + j];
                    wv[u] = words[static_cast<size_t>(k >> 6) * W + j];
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (kk[u] == VC_NONE) continue;
                const unsigned l = kk[u] >> 6;
                if (l != cur) { flush(); cur = l; s0 = s1 = s2 = s3 = cnt = 0; }
                const unsigned r = rv[u], w = wv[u];
                const int d0 = static_cast<int>(r & 255u) - static_cast<int>(w & 255u);
                const int d1 = static_cast<int>((r >> 8) & 255u) - static_cast<int>((w >> 8) & 255u);
                const int d2 = static_cast<int>((r >> 16) & 255u) - static_cast<int>((w >> 16) & 255u);
                const int d3 = static_cast<int>(r >> 24) - static_cast<int>(w >> 24);
                s0 += r & 255u; s1 += (r >> 8) & 255u; s2 += (r >> 16) & 255u; s3 += r >> 24;
                cost += static_cast<unsigned>(d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3);   // a wave's 64 rows: below 2^30
                ++cnt;
            }
        }
        flush();
    } else {
        const int cpl = (W + 1) >> 1;                                 // counters per lane: bits lane, 64 + lane, ...
        const int half = lane >> 5, bit = lane & 31;
        unsigned s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        unsigned cnt = 0, cur = VC_NONE;
        auto flush = [&]() {
            if (cur != VC_NONE && cnt) {
                unsigned* a = acc + static_cast<size_t>(cur) * (32 * W) + lane;
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    if (c < cpl && 2 * c + half < W) atomicAdd(a + 64 * c, s[c]);
                if (lane == 0) atomicAdd(count + cur, cnt);
            }
        };
        for (int t0 = 0; t0 < 64; t0 += 2) {
            unsigned kk[2], rv[2][8];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const unsigned k = static_cast<unsigned>(__shfl(static_cast<int>(key), t0 + u, 64));   // wave-uniform
                kk[u] = k < VC_NO_KEY ? k : VC_NONE;
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    rv[u][c] = 0;
                    if (kk[u] != VC_NONE && c < cpl && 2 * c + half < W) rv[u][c] = rows[static_cast<size_t>(base + (k & 63)) * W + 2 * c + half];
                }
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (kk[u] == VC_NONE) continue;
                const unsigned l = kk[u] >> 6;
                if (l != cur) {
                    flush();
                    cur = l; cnt = 0;
#pragma unroll
                    for (int c = 0; c < 8; ++c) s[c] = 0;
                }
#pragma unroll
                for (int c = 0; c < 8; ++c) s[c] += (rv[u][c] >> bit) & 1u;
                ++cnt;
            }
        }
        flush();
    }
    cost = pm::wave_sum_u32(cost);
    if (lane == 0) {
        if (n_changed) atomicAdd(&sc->n_changed, n_changed);
        if (cost) atomicAdd(&sc->cost, static_cast<unsigned long long>(cost));
    }
}

// One thread per dword of a word, a word on Wp = 2^wshift >= W lanes of one wave.
template <int KIND>
__global__ __launch_bounds__(256) void vocab_finish(uint32_t* __restrict__ words, unsigned* __restrict__ acc, unsigned* __restrict__ count,
                                                    int K, int W, int wshift, VcScalars* __restrict__ sc)
{
    const long long t = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int Wp = 1 << wshift;
    const long long wl = t >> wshift;
    const int j = static_cast<int>(t & (Wp - 1));
    const bool word_ok = wl < K;
    const int w = word_ok ? static_cast<int>(wl) : 0;
    const bool lead = word_ok && j == 0;
    unsigned cnt = 0;
    if (lead) {
        cnt = count[w];
        if (cnt) count[w] = 0;
    }
    cnt = static_cast<unsigned>(__shfl(static_cast<int>(cnt), lane & ~(Wp - 1), 64));
    bool moved = false;
    if (word_ok && j < W && cnt) {
        const uint32_t old = words[static_cast<size_t>(w) * W + j];
        uint32_t nw = 0;
        if (KIND == 0) {
            unsigned* a = acc + static_cast<size_t>(w) * (4 * W) + j;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const unsigned s = a[c * W];
                a[c * W] = 0;
                const unsigned q = s / cnt, r = s - q * cnt;          // (2 s + cnt) / (2 cnt) without leaving 32 bits
                nw |= (q + (2 * r >= cnt ? 1u : 0u)) << (8 * c);
            }
        } else {
            uint4* a = reinterpret_cast<uint4*>(acc + static_cast<size_t>(w) * (32 * W) + 32 * j);
#pragma unroll
            for (int v = 0; v < 8; ++v) {
                const uint4 s = a[v];
                a[v] = make_uint4(0, 0, 0, 0);
                nw |= (2 * s.x > cnt ? 1u : 0u) << (4 * v);
                nw |= (2 * s.y > cnt ? 1u : 0u) << (4 * v + 1);
                nw |= (2 * s.z > cnt ? 1u : 0u) << (4 * v + 2);
                nw |= (2 * s.w > cnt ? 1u : 0u) << (4 * v + 3);
            }
        }
        moved = nw != old;
        if (moved) words[static_cast<size_t>(w) * W + j] = nw;
    }
    const unsigned long long mv = __ballot(moved);
    const unsigned long long group = (Wp == 64 ? ~0ull : ((1ull << Wp) - 1ull)) << (lane & ~(Wp - 1));
    const unsigned n_moved = static_cast<unsigned>(__popcll(__ballot(lead && (mv & group) != 0)));
    const unsigned n_empty = static_cast<unsigned>(__popcll(__ballot(lead && cnt == 0)));
    if (lane == 0) {
        if (n_moved) atomicAdd(&sc->n_moved, n_moved);
        if (n_empty) atomicAdd(&sc->n_empty, n_empty);
    }
}

__global__ void vocab_record(VcScalars* __restrict__ sc, pm_vocab_iter* __restrict__ out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (out) {
        pm_vocab_iter r;
        r.n_changed = static_cast<int32_t>(sc->n_changed);
        r.n_empty = static_cast<int32_t>(sc->n_empty);
        r.n_moved = static_cast<int32_t>(sc->n_moved);
        r.reserved = 0;
        r.cost = sc->cost;
        *out = r;
    }
    sc->n_changed = 0; sc->n_empty = 0; sc->n_moved = 0; sc->pad = 0;
    sc->cost = 0; sc->pad2 = 0;
}

__global__ __launch_bounds__(256) void vocab_hist(const pm_match* __restrict__ rec, int n, const int32_t* __restrict__ d_n, int K,
                                                  int32_t* __restrict__ d_words, float* __restrict__ d_dist, unsigned* __restrict__ d_hist)
{
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int m = pm::clamped_count(d_n, n);
    const bool live = i < m;
    int lab = -1;
    float d = __uint_as_float(0x7FC00000u);
    if (live) {
        const pm_match r = rec[i];
        lab = r.trainIdx;
        d = r.distance;
    }
    if (i < n) {
        if (d_words) d_words[i] = lab;
        if (d_dist) d_dist[i] = d;
    }
    if (!d_hist) return;
    bool todo = live && lab >= 0 && lab < K;
    unsigned long long left = __ballot(todo);                         // wave-uniform loop: one atomic per distinct word
    while (left) {
        const int leader = __ffsll(static_cast<long long>(left)) - 1;
        const int l = __shfl(lab, leader, 64);
        const unsigned long long same = __ballot(todo && lab == l);
        if (lane == leader) atomicAdd(d_hist + l, static_cast<unsigned>(__popcll(same)));
        if (lab == l) todo = false;
        left &= ~same;
    }
}

inline bool bytes_ok(int kind, int bytes)
{
    return bytes >= 4 && bytes % 4 == 0 && bytes <= (kind == PM_VOCAB_L2_U8 ? 256 : 64);
}

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

}  // namespace

struct pm_vocab {
    int device = 0;
    int kind = 0, bytes = 0, K = 0, max_rows = 0;
    char* mem = nullptr;              // the one device block
    uint32_t* words = nullptr;        // K x bytes
    unsigned* acc = nullptr;          // K x (bytes | bytes * 8) u32, zero between iterations
    unsigned* count = nullptr;        // K, zero between iterations
    pm_match* rec = nullptr;          // max_rows records of the matcher
    int32_t* labels = nullptr;        // max_rows labels of the previous iteration
    VcScalars* sc = nullptr;
};

namespace {

int run_matcher(pm_ctx* ctx, const pm_vocab* v, const uint8_t* d_rows, int n)
{
    const uint8_t* w = reinterpret_cast<const uint8_t*>(v->words);
    return v->kind == PM_VOCAB_L2_U8 ? pm_bf_knn_l2_u8_dev(ctx, d_rows, n, w, v->K, v->bytes, 1, v->rec)
                                     : pm_bf_knn_hamming_u8_dev(ctx, d_rows, n, w, v->K, v->bytes, 1, v->rec);
}

// what every call on an object checks after its own arguments
#define VC_REQUIRE_OBJECT(ctx_, v_)                                                                                     \
    do {                                                                                                                \
        PM_REQUIRE((ctx_) != nullptr, PM_E_INVALID, "ctx is null");                                                     \
        PM_REFUSE_CAPTURE(ctx_);                                                                                        \
        PM_REQUIRE((v_)->device == (ctx_)->device, PM_E_INVALID, "vocabulary of another device");                       \
        PM_HIP_CHECK(hipSetDevice((ctx_)->device));                                                                     \
    } while (0)

}  // namespace

extern "C" int pm_vocab_create(pm_ctx* ctx, int kind, int bytes, int K, int max_rows, pm_vocab** out)
{
    PM_REQUIRE(out != nullptr, PM_E_INVALID, "null output pointer");
    *out = nullptr;
    PM_REQUIRE(kind == PM_VOCAB_L2_U8 || kind == PM_VOCAB_BITS, PM_E_INVALID, "kind must be PM_VOCAB_L2_U8 or PM_VOCAB_BITS");
    PM_REQUIRE(bytes_ok(kind, bytes), PM_E_INVALID, "bytes must be a multiple of 4 in [4, 256] (u8 rows) or [4, 64] (bit rows)");
    PM_REQUIRE(K >= 1 && K <= VC_MAX_K, PM_E_INVALID, "need 1 <= K <= 262144");
    PM_REQUIRE(max_rows >= 1, PM_E_INVALID, "need max_rows >= 1");
    PM_REQUIRE(max_rows <= VC_MAX_ROWS, PM_E_UNSUPPORTED, "max_rows above 2^24: a u32 sum of a cluster could overflow");
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    pm_vocab* v = new (std::nothrow) pm_vocab;
    PM_REQUIRE(v != nullptr, PM_E_NOMEM, "out of host memory");
    v->device = ctx->device; v->kind = kind; v->bytes = bytes; v->K = K; v->max_rows = max_rows;
    const size_t A = kind == PM_VOCAB_L2_U8 ? bytes : bytes * 8;
    const size_t b_words = pm::align_up(static_cast<size_t>(K) * bytes, 256), b_acc = pm::align_up(static_cast<size_t>(K) * A * 4, 256);
    const size_t b_count = pm::align_up(static_cast<size_t>(K) * 4, 256), b_rec = pm::align_up(static_cast<size_t>(max_rows) * sizeof(pm_match), 256);
    const size_t b_lab = pm::align_up(static_cast<size_t>(max_rows) * 4, 256), b_sc = 256;
    const size_t total = b_words + b_acc + b_count + b_rec + b_lab + b_sc;
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&v->mem), total);
    if (e != hipSuccess) {
        pm::set_error("pm_vocab_create: hipMalloc of %zu bytes failed: %s", total, hipGetErrorString(e));
        delete v;
        return PM_E_NOMEM;
    }
    char* p = v->mem;
    v->words = reinterpret_cast<uint32_t*>(p); p += b_words;
    v->acc = reinterpret_cast<unsigned*>(p); p += b_acc;
    v->count = reinterpret_cast<unsigned*>(p); p += b_count;
    v->rec = reinterpret_cast<pm_match*>(p); p += b_rec;
    v->labels = reinterpret_cast<int32_t*>(p); p += b_lab;
    v->sc = reinterpret_cast<VcScalars*>(p);
    // words, accumulators, counts and scalars start at zero; the kernels return the last three to zero themselves
    e = hipMemsetAsync(v->mem, 0, b_words + b_acc + b_count, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(v->sc, 0, b_sc, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        pm::set_error("pm_vocab_create: clearing the block failed: %s", hipGetErrorString(e));
        (void)hipFree(v->mem);
        delete v;
        return PM_E_HIP;
    }
    *out = v;
    return PM_OK;
}

extern "C" int pm_vocab_destroy(pm_vocab* v)
{
    if (!v) return PM_OK;
    int rc = PM_OK;
    if (v->mem && (hipSetDevice(v->device) != hipSuccess || hipFree(v->mem) != hipSuccess)) rc = PM_E_HIP;
    delete v;
    return rc;
}

extern "C" int pm_vocab_set_dev(pm_ctx* ctx, pm_vocab* v, const uint8_t* d_words)
{
    PM_REQUIRE(v != nullptr && d_words != nullptr, PM_E_INVALID, "null argument");
    VC_REQUIRE_OBJECT(ctx, v);
    PM_HIP_CHECK(hipMemcpyAsync(v->words, d_words, static_cast<size_t>(v->K) * v->bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return PM_OK;
}

extern "C" int pm_vocab_set(pm_ctx* ctx, pm_vocab* v, const uint8_t* words)
{
    PM_REQUIRE(v != nullptr && words != nullptr, PM_E_INVALID, "null argument");
    VC_REQUIRE_OBJECT(ctx, v);
    PM_HIP_CHECK(hipMemcpyAsync(v->words, words, static_cast<size_t>(v->K) * v->bytes, hipMemcpyHostToDevice, ctx->stream));
    PM_HIP_CHECK(hipStreamSynchronize(ctx->stream));                   // the caller's buffer is free again on return
    return PM_OK;
}

extern "C" int pm_vocab_get(pm_ctx* ctx, const pm_vocab* v, uint8_t* words)
{
    PM_REQUIRE(v != nullptr && words != nullptr, PM_E_INVALID, "null argument");
    VC_REQUIRE_OBJECT(ctx, v);
    PM_HIP_CHECK(hipMemcpyAsync(words, v->words, static_cast<size_t>(v->K) * v->bytes, hipMemcpyDeviceToHost, ctx->stream));
    PM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PM_OK;
}

extern "C" int pm_vocab_init_stride_dev(pm_ctx* ctx, pm_vocab* v, const uint8_t* d_rows, int n)
{
    PM_REQUIRE(v != nullptr && d_rows != nullptr, PM_E_INVALID, "null argument");
    PM_REQUIRE(n >= 1 && n <= v->max_rows, PM_E_INVALID, "need 1 <= n <= max_rows");
    PM_REQUIRE(aligned4(d_rows), PM_E_INVALID, "rows must be 4-byte aligned");
    VC_REQUIRE_OBJECT(ctx, v);
    const int W = v->bytes / 4;
    const long long threads = static_cast<long long>(v->K) * W;
    pm::ScopedKernelTime t(ctx, "vocab_init");
    hipLaunchKernelGGL(vocab_init, dim3(static_cast<unsigned>((threads + 255) / 256)), dim3(256), 0, ctx->stream,
                       reinterpret_cast<const uint32_t*>(d_rows), n, v->words, v->K, W);
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_vocab_train_dev(pm_ctx* ctx, pm_vocab* v, const uint8_t* d_rows, int n, int iters, int32_t* d_labels, pm_vocab_iter* d_info)
{
    PM_REQUIRE(iters >= 0 && iters <= VC_MAX_ITERS, PM_E_INVALID, "need 0 <= iters <= 1000");
    PM_REQUIRE(v != nullptr && d_rows != nullptr, PM_E_INVALID, "null argument");
    PM_REQUIRE(n >= 1 && n <= v->max_rows, PM_E_INVALID, "need 1 <= n <= max_rows");
    PM_REQUIRE(aligned4(d_rows), PM_E_INVALID, "rows must be 4-byte aligned");
    VC_REQUIRE_OBJECT(ctx, v);
    const int W = v->bytes / 4;
    int wshift = 0;
    while ((1 << wshift) < W) ++wshift;
    const unsigned g_update = static_cast<unsigned>(((n + 63) / 64 + 3) / 4);
    const unsigned g_finish = static_cast<unsigned>(((static_cast<long long>(v->K) << wshift) + 255) / 256);
    const uint32_t* rows32 = reinterpret_cast<const uint32_t*>(d_rows);
    for (int t = 0; t < iters; ++t) {
        const int rc = run_matcher(ctx, v, d_rows, n);
        if (rc != PM_OK) return rc;                                    // nothing of this iteration has been enqueued
        int32_t* lab_out = t == iters - 1 ? d_labels : nullptr;
        {
            pm::ScopedKernelTime tm(ctx, "vocab_update");
            if (v->kind == PM_VOCAB_L2_U8)
                hipLaunchKernelGGL(vocab_update<0>, dim3(g_update), dim3(256), 0, ctx->stream, v->rec, rows32, v->words, n, v->K, W,
                                   t == 0 ? 1 : 0, v->labels, lab_out, v->acc, v->count, v->sc);
            else
                hipLaunchKernelGGL(vocab_update<1>, dim3(g_update), dim3(256), 0, ctx->stream, v->rec, rows32, v->words, n, v->K, W,
                                   t == 0 ? 1 : 0, v->labels, lab_out, v->acc, v->count, v->sc);
        }
        {
            pm::ScopedKernelTime tm(ctx, "vocab_finish");
            if (v->kind == PM_VOCAB_L2_U8)
                hipLaunchKernelGGL(vocab_finish<0>, dim3(g_finish), dim3(256), 0, ctx->stream, v->words, v->acc, v->count, v->K, W, wshift, v->sc);
            else
                hipLaunchKernelGGL(vocab_finish<1>, dim3(g_finish), dim3(256), 0, ctx->stream, v->words, v->acc, v->count, v->K, W, wshift, v->sc);
            hipLaunchKernelGGL(vocab_record, dim3(1), dim3(64), 0, ctx->stream, v->sc, d_info ? d_info + t : nullptr);
        }
        PM_HIP_CHECK(hipGetLastError());
    }
    return PM_OK;
}

extern "C" int pm_vocab_train(pm_ctx* ctx, pm_vocab* v, const uint8_t* rows, int n, int iters, int32_t* labels, pm_vocab_iter* info)
{
    PM_REQUIRE(iters >= 0 && iters <= VC_MAX_ITERS, PM_E_INVALID, "need 0 <= iters <= 1000");
    PM_REQUIRE(v != nullptr && rows != nullptr, PM_E_INVALID, "null argument");
    PM_REQUIRE(n >= 1 && n <= v->max_rows, PM_E_INVALID, "need 1 <= n <= max_rows");
    VC_REQUIRE_OBJECT(ctx, v);
    if (iters == 0) return PM_OK;
    const size_t rb = static_cast<size_t>(n) * v->bytes, lb = labels ? static_cast<size_t>(n) * 4 : 0;
    const size_t ib = info ? static_cast<size_t>(iters) * sizeof(pm_vocab_iter) : 0;
    pm::StagedBlock b(ctx, "pm_vocab_train");
    const size_t o_rows = b.add(rb), o_lab = b.add(lb), o_info = b.add(ib);
    b.alloc();
    b.upload(o_rows, rows, rb);
    if (b.rc == PM_OK)
        b.rc = pm_vocab_train_dev(ctx, v, b.at<const uint8_t>(o_rows), n, iters, labels ? b.at<int32_t>(o_lab) : nullptr,
                                  info ? b.at<pm_vocab_iter>(o_info) : nullptr);
    b.download(labels, o_lab, lb);
    b.download(info, o_info, ib);
    return b.sync();
}

extern "C" int pm_vocab_assign_dev(pm_ctx* ctx, const pm_vocab* v, const uint8_t* d_rows, int n, const int32_t* d_n, int32_t* d_words,
                                   float* d_dist, uint32_t* d_hist)
{
    PM_REQUIRE(v != nullptr && d_rows != nullptr, PM_E_INVALID, "null argument");
    PM_REQUIRE(n >= 1 && n <= v->max_rows, PM_E_INVALID, "need 1 <= n <= max_rows");
    PM_REQUIRE(aligned4(d_rows), PM_E_INVALID, "rows must be 4-byte aligned");
    VC_REQUIRE_OBJECT(ctx, v);
    const int rc = run_matcher(ctx, v, d_rows, n);
    if (rc != PM_OK) return rc;
    pm::ScopedKernelTime t(ctx, "vocab_hist");
    if (d_hist) PM_HIP_CHECK(hipMemsetAsync(d_hist, 0, static_cast<size_t>(v->K) * 4, ctx->stream));
    hipLaunchKernelGGL(vocab_hist, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, ctx->stream, v->rec, n, d_n, v->K, d_words,
                       d_dist, d_hist);
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_vocab_assign(pm_ctx* ctx, const pm_vocab* v, const uint8_t* rows, int n, int32_t* words, float* dist, uint32_t* hist)
{
    PM_REQUIRE(v != nullptr && rows != nullptr, PM_E_INVALID, "null argument");
    PM_REQUIRE(n >= 1 && n <= v->max_rows, PM_E_INVALID, "need 1 <= n <= max_rows");
    VC_REQUIRE_OBJECT(ctx, v);
    const size_t rb = static_cast<size_t>(n) * v->bytes, wb = words ? static_cast<size_t>(n) * 4 : 0, db = dist ? static_cast<size_t>(n) * 4 : 0;
    const size_t hb = hist ? static_cast<size_t>(v->K) * 4 : 0;
    pm::StagedBlock b(ctx, "pm_vocab_assign");
    const size_t o_rows = b.add(rb), o_w = b.add(wb), o_d = b.add(db), o_h = b.add(hb);
    b.alloc();
    b.upload(o_rows, rows, rb);
    if (b.rc == PM_OK)
        b.rc = pm_vocab_assign_dev(ctx, v, b.at<const uint8_t>(o_rows), n, nullptr, words ? b.at<int32_t>(o_w) : nullptr,
                                   dist ? b.at<float>(o_d) : nullptr, hist ? b.at<uint32_t>(o_h) : nullptr);
    b.download(words, o_w, wb);
    b.download(dist, o_d, db);
    b.download(hist, o_h, hb);
    return b.sync();
}
