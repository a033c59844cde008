// capture_host_main.cpp — the host-side rules of graph capture (include/pm.h, "Graph capture of the estimator calls")
// checked without a device: csrc/pm_capi.cpp is compiled as it is and linked against the stand-in HIP runtime below, which
// counts what the library asks of it and lets the test say whether the stream "is capturing".  Built and run by
// tests/test_capture_cpu.py; prints one line per check and exits non-zero on the first that fails.
#include <cstdlib>
#include <set>

#include "pm_common.hpp"

namespace {
bool g_capturing = false;
bool g_capture_broken = false;              // a call that ends a real capture with an error was made while capturing
int n_malloc = 0, n_free = 0, n_sync = 0, n_memset_async = 0, n_event_create = 0, n_event_record = 0, n_bad_free = 0;
std::set<void*> g_live;

struct Counts {
    int malloc_, free_, sync, memset_async, event_record;
    bool operator==(const Counts& o) const
    {
        return malloc_ == o.malloc_ && free_ == o.free_ && sync == o.sync && memset_async == o.memset_async &&
               event_record == o.event_record;
    }
};
Counts counts() { return Counts{n_malloc, n_free, n_sync, n_memset_async, n_event_record}; }
}  // namespace

// ---- the stand-in runtime: host memory, no device, a capture flag ------------------------------------------------------------
extern "C" {
hipError_t hipGetDeviceCount(int* n) { *n = 1; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetDeviceProperties(hipDeviceProp_t* p, int) { memset(p, 0, sizeof *p); p->multiProcessorCount = 256; return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { *s = reinterpret_cast<hipStream_t>(malloc(8)); return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) { free(s); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t)
{
    ++n_sync;
    if (g_capturing) { g_capture_broken = true; return hipErrorStreamCaptureUnsupported; }
    return hipSuccess;
}
hipError_t hipStreamIsCapturing(hipStream_t, hipStreamCaptureStatus* st)
{
    *st = g_capturing ? hipStreamCaptureStatusActive : hipStreamCaptureStatusNone;
    return hipSuccess;
}
hipError_t hipMalloc(void** p, size_t n)
{
    ++n_malloc;
    *p = malloc(n ? n : 1);
    g_live.insert(*p);
    return hipSuccess;
}
hipError_t hipFree(void* p)
{
    ++n_free;
    if (!p) return hipSuccess;
    if (!g_live.erase(p)) { ++n_bad_free; return hipErrorInvalidValue; }
    free(p);
    return hipSuccess;
}
hipError_t hipHostMalloc(void** p, size_t n, unsigned) { *p = malloc(n ? n : 1); return hipSuccess; }
hipError_t hipHostFree(void* p) { free(p); return hipSuccess; }
hipError_t hipMemset(void* p, int v, size_t n) { memset(p, v, n); return hipSuccess; }
hipError_t hipMemsetAsync(void* p, int v, size_t n, hipStream_t) { ++n_memset_async; memset(p, v, n); return hipSuccess; }
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) { memcpy(d, s, n); return hipSuccess; }
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t) { memcpy(d, s, n); return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t* e) { ++n_event_create; *e = reinterpret_cast<hipEvent_t>(malloc(8)); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { free(e); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { ++n_event_record; return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 0.5f; return hipSuccess; }
const char* hipGetErrorString(hipError_t e)
{
    return e == hipErrorStreamCaptureUnsupported ? "operation not permitted when stream is capturing" : "stand-in error";
}
}

#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            printf("FAILED %s:%d: %s   [last error: %s]\n", __FILE__, __LINE__, #cond, pm_last_error()); \
            return 1;                                                                      \
        }                                                                                  \
    } while (0)

static bool names_the_remedy() { return strstr(pm_last_error(), "eager call") && strstr(pm_last_error(), "capturing"); }

int main()
{
    constexpr size_t MiB = size_t(1) << 20;
    size_t cap = 0;
    int retired = -1;

    // 1. first call of a context under capture: refused before anything is touched; the same context works afterwards
    pm_ctx* c = nullptr;
    CHECK(pm_ctx_create(0, &c) == PM_OK);
    CHECK(pm_ctx_scratch_info(c, &cap, &retired) == PM_OK && cap == 0 && retired == 0);
    g_capturing = true;
    Counts before = counts();
    const int rc_arena = pm::arena_reserve(c, 1000);
    CHECK(counts() == before && !g_capture_broken);                          // the side effects first, then the status
    CHECK(rc_arena == PM_E_UNSUPPORTED && names_the_remedy());
    const int rc_words = pm::sync_words_reserve(c);
    CHECK(counts() == before && !g_capture_broken);
    CHECK(rc_words == PM_E_UNSUPPORTED && names_the_remedy());
    CHECK(pm_ctx_scratch_info(c, &cap, &retired) == PM_OK && cap == 0 && retired == 0 && c->sync_words == nullptr);
    g_capturing = false;
    CHECK(pm::arena_reserve(c, 1000) == PM_OK && pm::sync_words_reserve(c) == PM_OK);
    CHECK(pm_ctx_scratch_info(c, &cap, nullptr) == PM_OK && cap == MiB && c->sync_words != nullptr);
    CHECK(n_memset_async == before.memset_async + 1);
    printf("ok first call under capture refused without side effects\n");

    // 2. warmed context under capture: what fits is carved with no runtime call at all; what does not fit is refused
    g_capturing = true;
    before = counts();
    CHECK(pm::arena_reserve(c, 4096) == PM_OK && pm::sync_words_reserve(c) == PM_OK);
    pm::arena_reset(c);
    char* in_graph = static_cast<char*>(pm::arena_take(c, 4096));
    CHECK(in_graph != nullptr && counts() == before);
    CHECK(pm::arena_reserve(c, 3 * MiB) == PM_E_UNSUPPORTED && names_the_remedy());
    CHECK(counts() == before && !g_capture_broken);
    CHECK(pm_ctx_scratch_info(c, &cap, &retired) == PM_OK && cap == MiB && retired == 0);
    g_capturing = false;
    printf("ok warmed context records what fits and refuses what does not\n");

    // 3. growth after a carve under capture: the block is retired, not freed, and the new one is at least twice as large
    before = counts();
    CHECK(pm::arena_reserve(c, MiB + 1) == PM_OK);
    CHECK(n_free == before.free_ && g_live.count(in_graph) == 1);
    CHECK(pm_ctx_scratch_info(c, &cap, &retired) == PM_OK && retired == 1 && cap >= 2 * MiB);
    const size_t cap3 = cap;
    // ... and a carve made eagerly from the new block marks nothing: the next growth frees it
    pm::arena_reset(c);
    char* eager = static_cast<char*>(pm::arena_take(c, 4096));
    CHECK(eager != nullptr && eager != in_graph);
    before = counts();
    CHECK(pm::arena_reserve(c, 8 * MiB) == PM_OK);
    CHECK(n_free == before.free_ + 1 && g_live.count(in_graph) == 1);       // (a freed address may come back: count, not look up)
    CHECK(pm_ctx_scratch_info(c, &cap, &retired) == PM_OK && retired == 1 && cap == 10 * MiB && cap > cap3);
    // a second recorded block is retired as well
    g_capturing = true;
    pm::arena_reset(c);
    char* in_graph2 = static_cast<char*>(pm::arena_take(c, 64));
    g_capturing = false;
    CHECK(pm::arena_reserve(c, 11 * MiB) == PM_OK);
    CHECK(pm_ctx_scratch_info(c, &cap, &retired) == PM_OK && retired == 2 && cap >= 20 * MiB && g_live.count(in_graph2) == 1);
    printf("ok a block a graph may hold is retired, every other block is freed\n");

    // 4. timing: no event on a capturing stream, events as before on any other
    CHECK(pm_ctx_timing_enable(c, 1) == PM_OK);
    g_capturing = true;
    before = counts();
    const int created = n_event_create;
    { pm::ScopedKernelTime t(c, "probe"); }
    CHECK(counts() == before && n_event_create == created);
    g_capturing = false;
    { pm::ScopedKernelTime t(c, "probe"); }
    CHECK(n_event_record == before.event_record + 2);
    double ms = 0.0;
    int launches = -1;
    CHECK(pm_ctx_timing_get(c, "probe", &ms, &launches) == PM_OK && launches == 1 && ms == 0.5);
    printf("ok timing records nothing on a capturing stream\n");

    // 5. destroying the context frees the live block and every retired one
    CHECK(pm_ctx_destroy(c) == PM_OK);
    CHECK(g_live.empty() && n_bad_free == 0);
    printf("ok pm_ctx_destroy frees the retired blocks\n");

    // 6. a context that never sees a capture: blocks are sized and freed as they always were
    CHECK(pm_ctx_create(0, &c) == PM_OK);
    CHECK(pm::arena_reserve(c, MiB + 1) == PM_OK);
    pm::arena_reset(c);
    CHECK(pm::arena_take(c, 4096) != nullptr);
    before = counts();
    CHECK(pm::arena_reserve(c, 4 * MiB) == PM_OK);
    CHECK(n_free == before.free_ + 1 && n_malloc == before.malloc_ + 1 && n_sync == before.sync + 1);
    CHECK(pm_ctx_scratch_info(c, &cap, &retired) == PM_OK && retired == 0 && cap == 5 * MiB);
    CHECK(pm_ctx_scratch_info(nullptr, &cap, &retired) == PM_E_INVALID && pm_ctx_scratch_info(c, nullptr, nullptr) == PM_OK);
    CHECK(pm_ctx_destroy(c) == PM_OK && g_live.empty() && n_bad_free == 0);
    printf("ok without a capture nothing is retired\n");
    printf("ALL OK\n");
    return 0;
}
