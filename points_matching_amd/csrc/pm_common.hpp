// pm_common.hpp — context, error plumbing, scratch arena and per-kernel event timing shared by
// the translation units of libpm_hip.so.  gfx950 only; no CUDA-compat layer.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "image_args.hpp"
#include "pm.h"
#include "stage_layout.hpp"

namespace pm {

void set_error(const char* fmt, ...);

#define PM_HIP_CHECK(expr)                                                              \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess) {                                                         \
            ::pm::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),      \
                            __FILE__, __LINE__);                                        \
            return PM_E_HIP;                                                            \
        }                                                                               \
    } while (0)

#define PM_REQUIRE(cond, status, msg)                                                   \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            ::pm::set_error("%s: %s", __func__, msg);                                   \
            return (status);                                                            \
        }                                                                               \
    } while (0)

// a pm_image::Check (image_args.hpp) that did not pass: its status and its message under the caller's name
#define PM_REQUIRE_PASS(check)                                                          \
    do {                                                                                \
        const ::pm_image::Check c_ = (check);                                           \
        PM_REQUIRE(c_.status == PM_OK, c_.status, c_.why);                              \
    } while (0)

// The matcher and the compaction kernels tag their side-band words with a per-call epoch that the HOST increments (it
// stands in for a memset per call).  A captured graph freezes that argument: a replay could take the previous replay's
// look-back counts for its own.  So these calls refuse a capturing stream instead of recording something unreplayable.
inline bool stream_is_capturing(hipStream_t s)
{
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &st) == hipSuccess && st != hipStreamCaptureStatusNone;
}
#define PM_REFUSE_CAPTURE(ctx_)                                                                                         \
    PM_REQUIRE(!::pm::stream_is_capturing((ctx_)->stream), PM_E_UNSUPPORTED,                                            \
               "the stream is capturing a graph: this call carries a per-call epoch argument and cannot be replayed")

struct KernelTimer {
    double total_ms = 0.0;
    int launches = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};

}  // namespace pm

constexpr int PM_MAX_DEVICES = 64;      // per-device one-time state (kernel attributes) is kept in arrays of this size

struct pm_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    // grow-only device scratch; carved by a bump pointer that every API call resets
    char* arena = nullptr;
    size_t arena_cap = 0;
    size_t arena_off = 0;
    // Graph capture (pm.h, "Graph capture of the estimator calls"): arena_capturing is what arena_reset saw on the stream;
    // a carve made under it sets arena_in_graph, after which a growth retires the block instead of freeing it (a recorded
    // graph holds its addresses).  Retired blocks are freed in pm_ctx_destroy.
    bool arena_capturing = false;
    bool arena_in_graph = false;
    std::vector<char*> arena_retired;
    // pinned host staging for small results
    void* pinned = nullptr;
    size_t pinned_cap = 0;
    // timing
    bool timing = false;
    std::map<std::string, pm::KernelTimer> timers;
    std::vector<hipEvent_t> event_pool;
    int n_cu = 256;
    // kNN side-band: [0..1] epoch-tagged 64-bit maxima (never cleared), diag words (re-scan count,
    // non-finite flag) filled only while knn_diag is on
    unsigned long long* knn_stats = nullptr;
    unsigned* knn_diag_words = nullptr;
    unsigned knn_epoch = 0;
    bool knn_diag = false;
    // stable compaction: epoch-tagged per-block survivor counts
    unsigned* fg_counts = nullptr;
    unsigned fg_epoch = 0;
    // compaction fused into the L2 refinement: kf_cap arrival words (8 B) followed by kf_cap epoch-tagged counts (4 B)
    unsigned long long* kf_tile = nullptr;
    int kf_cap = 0;
    unsigned kf_epoch = 0;
    // arrival tickets / counters of the one-launch RANSAC kernels; every launch returns them to zero
    int* sync_words = nullptr;
    int opts[PM_OPT_COUNT_] = {};          // pm_ctx_set_option
    // f32 copies of u8 descriptor rows for the shapes pm_bf_knn_l2_u8 hands to the f32 matcher (grow-only)
    float* widen = nullptr;
    size_t widen_cap = 0;
    // feature front end (features.hip): tables, candidate counter, Gaussian pyramid, candidates and row staging (grow-only;
    // apart from the arena so that pm_detect_level_get can read the pyramid of the last call), and that call's octave plan
    char* feat = nullptr;
    size_t feat_cap = 0;
    size_t feat_counter_off = 0;
    int feat_noct = 0;
    int feat_w[16] = {}, feat_h[16] = {};
    size_t feat_off[16] = {};              // byte offset of each octave's six planes
    // point descriptors (describe_points.hip): the Q20 bin table and the steered offsets of S72 / S73, uploaded on the first call
    char* desc_tab = nullptr;
};

namespace pm {

// ensure capacity (may sync + realloc).  A growth on a capturing stream is refused before anything is touched
// (PM_E_UNSUPPORTED); a block that a captured graph may hold is retired, not freed, and the new one is at least twice as large.
int arena_reserve(pm_ctx* ctx, size_t bytes);
void arena_reset(pm_ctx* ctx);                          // also notes whether the stream is capturing, for arena_take
void* arena_take(pm_ctx* ctx, size_t bytes);            // 256-B aligned carve; nullptr if over cap
// The arrival words of the one-launch RANSAC kernels (ctx->sync_words), allocated and zeroed on a context's first such call;
// on a capturing stream that first call is refused (PM_E_UNSUPPORTED) before anything is allocated or enqueued.  Who owns
// which word: ransac_internal.hpp (SyncWord), checked there against the size here.
constexpr size_t SYNC_WORDS_BYTES = 256;
int sync_words_reserve(pm_ctx* ctx);
int pinned_reserve(pm_ctx* ctx, size_t bytes);
// The private device block of a host-pointer entry point around its _dev form (the _dev form resets the arena, so the
// staged rows cannot live there): add() the parts, alloc(), upload(), rc = the _dev form, download(), sync().  The first
// failing step sets the status and the message and every later step is skipped.  A caller that succeeded leaves through
// sync(); after a failure the destructor synchronises the stream before it frees.  (Hidden: the dynamic symbol table stays.)
struct __attribute__((visibility("hidden"))) StagedBlock : StageLayout {
    pm_ctx* ctx;
    const char* who;                                             // the caller's name, for the messages
    char* base = nullptr;
    int rc = PM_OK;                                              // the first failure so far
    StagedBlock(pm_ctx* c, const char* w) : ctx(c), who(w) {}
    StagedBlock(const StagedBlock&) = delete;
    ~StagedBlock();
    int alloc();                                                 // one hipMalloc of `total` bytes; PM_E_NOMEM
    void upload(size_t off, const void* src, size_t bytes);      // both on ctx->stream, nothing for 0 bytes; PM_E_HIP
    void download(void* dst, size_t off, size_t bytes);
    int sync();                                                  // synchronises the stream; returns rc
    template <class T> T* at(size_t off) const { return reinterpret_cast<T*>(base + off); }
    void step(hipError_t e, int status, const char* what);
    // A plain matcher's whole sequence around dev(d_q, d_t, d_out).  Three blocks, not one: freeing a device block of 2 MiB
    // or more costs ~220 us, below that under 1 us (profiles/host_stage_timing.json), and 1 MiB row sets are an everyday shape.
    template <class Dev> static int knn(pm_ctx* ctx, const char* who, const void* q, size_t qb, const void* t, size_t tb, void* out, size_t ob, Dev dev)
    {
        StagedBlock bq(ctx, who), bt(ctx, who), bo(ctx, who);       // destroyed bo, bt, bq: the one that failed synchronises before bq, bt go
        const size_t o_q = bq.add(qb), o_t = bt.add(tb), o_out = bo.add(ob);
        if (bq.alloc() != PM_OK || bt.alloc() != PM_OK || bo.alloc() != PM_OK) return PM_E_NOMEM;
        bq.upload(o_q, q, qb);
        if (bq.rc == PM_OK) bt.upload(o_t, t, tb);
        if (bq.rc != PM_OK || bt.rc != PM_OK) return PM_E_HIP;
        bo.rc = dev(bq.base, bt.base, bo.base);
        bo.download(out, o_out, ob);
        return bo.sync();
    }
    // An image -> image call's whole sequence around dev(d_extra, d_src, d_dst, d_valid, d_info).  extra is the call's own input
    // (a model, a map; 0 bytes: none).  dst is uploaded, so that the bytes between its rows come back as they were; valid and
    // info are staged, and handed to dev, only when the caller asked for them.
    template <class Dev> static int image(pm_ctx* ctx, const char* who, const void* extra, size_t extra_b, const uint8_t* src, int sw, int sh,
                                          int sstride, uint8_t* dst, int dw, int dh, int dstride, uint8_t* valid, pm_warp_info* info, Dev dev)
    {
        const size_t src_b = pm_image::span(sw, sh, sstride, 1), dst_b = pm_image::span(dw, dh, dstride, 1), val_b = static_cast<size_t>(dw) * dh;
        StagedBlock b(ctx, who);
        const size_t o_extra = b.add(extra_b), o_info = b.add(sizeof(pm_warp_info)), o_src = b.add(src_b), o_dst = b.add(dst_b);
        const size_t o_val = b.add(valid ? val_b : 0);
        b.alloc();
        b.upload(o_extra, extra, extra_b);
        b.upload(o_src, src, src_b);
        b.upload(o_dst, dst, dst_b);
        if (b.rc == PM_OK)
            b.rc = dev(b.at<const char>(o_extra), b.at<const uint8_t>(o_src), b.at<uint8_t>(o_dst), valid ? b.at<uint8_t>(o_val) : nullptr,
                       info ? b.at<pm_warp_info>(o_info) : nullptr);
        b.download(dst, o_dst, dst_b);
        if (valid) b.download(valid, o_val, val_b);
        if (info) b.download(info, o_info, sizeof(pm_warp_info));
        return b.sync();
    }
    // A stereo matcher's whole sequence: the left map by base(d_left, d_right, d_disp, d_info) and, with lr_max_diff16 >= 0, the
    // right map (w elements per row) by from_right(d_left, d_right, d_rmap) and S86 on the two.  disp is uploaded, so that the
    // elements between its rows come back as they were.  n_valid is always counted on the device: the count is of the last pass.
    template <class Base, class FromRight>
    static int stereo(pm_ctx* ctx, const char* who, const uint8_t* left, const uint8_t* right, int w, int h, int lstride, int rstride,
                      int lr_max_diff16, int16_t* disp, int dstride, pm_stereo_info* info, Base base, FromRight from_right)
    {
        const bool lr = lr_max_diff16 >= 0;
        const size_t l_b = pm_image::span(w, h, lstride, 1), r_b = pm_image::span(w, h, rstride, 1), d_b = pm_image::span(w, h, dstride, 2);
        const size_t rmap_b = lr ? static_cast<size_t>(w) * h * 2 : 0;
        StagedBlock b(ctx, who);
        const size_t o_info = b.add(sizeof(pm_stereo_info)), o_l = b.add(l_b), o_r = b.add(r_b), o_d = b.add(d_b), o_rmap = b.add(rmap_b);
        b.alloc();
        b.upload(o_l, left, l_b);
        b.upload(o_r, right, r_b);
        b.upload(o_d, disp, d_b);
        pm_stereo_info* d_info = b.at<pm_stereo_info>(o_info);
        if (b.rc == PM_OK) b.rc = base(b.at<const uint8_t>(o_l), b.at<const uint8_t>(o_r), b.at<int16_t>(o_d), d_info);
        if (lr && b.rc == PM_OK) b.rc = from_right(b.at<const uint8_t>(o_l), b.at<const uint8_t>(o_r), b.at<int16_t>(o_rmap));
        if (lr && b.rc == PM_OK) b.rc = pm_stereo_lr_check_dev(ctx, b.at<int16_t>(o_d), b.at<int16_t>(o_rmap), w, h, dstride, w, lr_max_diff16, d_info);
        b.download(disp, o_d, d_b);
        if (info) b.download(info, o_info, sizeof(pm_stereo_info));
        return b.sync();
    }
};

// RAII event bracket: records start/stop on ctx->stream when timing is on.
struct ScopedKernelTime {
    pm_ctx* ctx;
    hipEvent_t a = nullptr, b = nullptr;
    const char* name;
    ScopedKernelTime(pm_ctx* c, const char* n);
    ~ScopedKernelTime();
};

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

#if defined(__HIPCC__)
// n = *d_n clamped to [0, cap]; NULL = cap (the -1 that the point sources write on overflow counts as 0)
__device__ __forceinline__ int clamped_count(const int32_t* d_n, int cap)
{
    const int n = d_n ? *d_n : cap;
    return n < 0 ? 0 : (n > cap ? cap : n);
}
#endif

}  // namespace pm
