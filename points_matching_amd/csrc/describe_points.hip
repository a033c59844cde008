// describe_points.hip — oriented 256-bit descriptors of GIVEN points on one level of a pm_pyramid (docs/SPEC.md S71-S74): the
// `compute` half of cv::ORB::compute for the corners of corners.hip and the tracked points of track_lk.hip, which makes them
// matchable by appearance (knn_hamming.hip, the cross-check and the guided matchers, cols = 32).
//
// Every quantity is an integer: the pixels are u8, the two moments and the 5 x 5 box sums are exact integer sums, the bin is
// an arg-max of int64 dot products with a Q20 table, and the tests compare box sums.  No transcendental function runs per
// point, so the 32 bytes are a function of the level, the point and the flags alone, bit for bit tests/describe_ref.c.
//
// Launches, all on the context's stream:
//   desc_points    one wave per point, four points per workgroup: the 35 x 35 patch to the wave's LDS slice, the 31 x 31 plane
//                  of box sums by two separable passes, the moments over the disc, the bin, four ballots of 64 tests
//   desc_compact   the gather form only: one workgroup scans the valid flags in input order and moves the rows
#include <cmath>

#include "pm_common.hpp"
#include "pyramid.hpp"
#include "wave_ops.hpp"

namespace {

constexpr int NBIN = 36;
constexpr int NTEST = 256;
constexpr int REACH = 17;                                      // 15 (largest offset coordinate) + 2 (half a box)
constexpr int PATCH = 2 * REACH + 1;                           // 35
constexpr int PITCH = PATCH + 1;                               // 36 bytes a patch row: rows start on a dword
constexpr int PLANE = 31;                                      // box sums at offsets -15 .. 15
constexpr int PX_BYTES = (PATCH * PITCH + 15) & ~15;           // 1264
constexpr int ROW_SHORTS = (PATCH * PLANE + 7) & ~7;           // 35 rows of 31 horizontal 5-sums: 1088 shorts
constexpr int BOX_SHORTS = (PLANE * PLANE + 7) & ~7;           // 968 shorts
constexpr int WAVE_BYTES = PX_BYTES + 2 * (ROW_SHORTS + BOX_SHORTS);   // 5376 bytes of LDS per wave
constexpr int WPB = 4;                                         // waves (= points) per workgroup
static_assert(WAVE_BYTES % 16 == 0 && WPB * WAVE_BYTES <= 65536, "desc_points: LDS slices");

// the context's table buffer: cos_sin_q20[72] (int32), then at Q20_BYTES the steered offsets [37][256][4] (int8)
constexpr size_t Q20_BYTES = 512;
constexpr size_t STEER_BYTES = static_cast<size_t>(NBIN + 1) * NTEST * 4;
constexpr size_t TAB_BYTES = Q20_BYTES + STEER_BYTES;

struct DescTables {
    int32_t q20[2 * NBIN];
    int8_t steer[NBIN + 1][NTEST][4];
};

// S72 / S73 from the fp64 bin cosines and sines of S56 and the pattern of S58, both as the feature front end states them.
const DescTables& desc_tables()
{
    static const DescTables t = [] {
        DescTables d;
        memset(&d, 0, sizeof d);
        double cs[2 * NBIN];
        int8_t base[NTEST][4];
        (void)pm_detect_tables(nullptr, nullptr, nullptr, nullptr, nullptr, cs);
        (void)pm_detect_bits_table(&base[0][0], nullptr);
        const double* sn = cs + NBIN;
        for (int b = 0; b < NBIN; ++b) {
            d.q20[b] = static_cast<int32_t>(std::nearbyint(1048576.0 * cs[b]));
            d.q20[NBIN + b] = static_cast<int32_t>(std::nearbyint(1048576.0 * sn[b]));
            for (int i = 0; i < NTEST; ++i)
                for (int p = 0; p < 4; p += 2) {
                    const double x = base[i][p], y = base[i][p + 1];
                    d.steer[b][i][p] = static_cast<int8_t>(std::nearbyint(cs[b] * x - sn[b] * y));
                    d.steer[b][i][p + 1] = static_cast<int8_t>(std::nearbyint(sn[b] * x + cs[b] * y));
                }
        }
        memcpy(d.steer[NBIN], base, sizeof base);
        return d;
    }();
    return t;
}

struct DescArgs {
    const uint8_t* plane;              // the level, tight rows of w bytes
    int w, h;
    float scale;                       // 2^-level
    int upright;
    const int32_t* q20;
    const int8_t* steer;
    const float* pts;
    const int32_t* d_n;
    int cap, pad;
    uint8_t* desc;
    uint8_t* valid;
    uint8_t* bin;
};

using pm::wave_lds_sync;
using pm::wave_sum_i32;

// No workgroup barrier anywhere: a wave owns its point and its LDS slice, so a wave behind the count may leave at once and the
// waves of a workgroup may take the valid and the invalid path side by side.  Every branch below is wave-uniform.
__global__ __launch_bounds__(64 * WPB) void desc_points(const DescArgs a)
{
    __shared__ __attribute__((aligned(16))) unsigned char s_mem[WPB][WAVE_BYTES];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int pt = blockIdx.x * WPB + wave;
    if (pt >= pm::clamped_count(a.d_n, a.cap)) return;
    unsigned char* s_px = s_mem[wave];
    unsigned short* s_row = reinterpret_cast<unsigned short*>(s_px + PX_BYTES);
    unsigned short* s_box = s_row + ROW_SHORTS;
    uint8_t* out = a.desc + static_cast<size_t>(pt) * 32;

    // S71
    const float x = a.pts[2 * static_cast<size_t>(pt)], y = a.pts[2 * static_cast<size_t>(pt) + 1];
    bool ok = fabsf(x) <= 1e6f && fabsf(y) <= 1e6f;               // false for NaN, infinity, beyond 1e6
    int cx = 0, cy = 0;
    if (ok) {
        cx = static_cast<int>(rintf(x * a.scale));
        cy = static_cast<int>(rintf(y * a.scale));
        ok = cx >= REACH && cx <= a.w - REACH - 1 && cy >= REACH && cy <= a.h - REACH - 1;
    }
    if (!ok) {
        if (lane < 32) out[lane] = 0;
        if (lane == 0) {
            if (a.valid) a.valid[pt] = 0;
            if (a.bin) a.bin[pt] = 255;
        }
        return;
    }

    // the patch: s_px[j * PITCH + i] = pixel (cx - 17 + i, cy - 17 + j)
    const uint8_t* src = a.plane + static_cast<size_t>(cy - REACH) * a.w + (cx - REACH);
    for (int e = lane; e < PATCH * PATCH; e += 64) {
        const int j = (e * 1873) >> 16, i = e - j * PATCH;           // e / 35 for e < 1225
        s_px[j * PITCH + i] = src[static_cast<size_t>(j) * a.w + i];
    }
    wave_lds_sync();

    // S74, first pass: s_row[j * 31 + i] = the five pixels i .. i + 4 of patch row j
    for (int e = lane; e < PATCH * PLANE; e += 64) {
        const int j = (e * 2115) >> 16, i = e - j * PLANE;           // e / 31 for e < 1085
        const unsigned char* p = s_px + j * PITCH + i;
        s_row[e] = static_cast<unsigned short>(p[0] + p[1] + p[2] + p[3] + p[4]);
    }

    // S72: the moments over the disc, on the same patch; S74, second pass
    int bin = NBIN;
    int m10 = 0, m01 = 0;
    if (!a.upright) {
        for (int e = lane; e < PLANE * PLANE; e += 64) {
            const int j = (e * 2115) >> 16, i = e - j * PLANE;
            const int dx = i - 15, dy = j - 15;
            const int v = dx * dx + dy * dy <= 225 ? s_px[(j + 2) * PITCH + (i + 2)] : 0;
            m10 += dx * v;
            m01 += dy * v;
        }
    }
    wave_lds_sync();
    for (int e = lane; e < PLANE * PLANE; e += 64) {
        const unsigned short* p = s_row + e;                          // box (i, j): rows j .. j + 4 of column i
        s_box[e] = static_cast<unsigned short>(p[0] + p[PLANE] + p[2 * PLANE] + p[3 * PLANE] + p[4 * PLANE]);
    }
    if (!a.upright) {
        m10 = wave_sum_i32(m10);
        m01 = wave_sum_i32(m01);
        // lanes 0 .. 35 hold the dots; the butterfly keeps the larger dot, of equal dots the lower bin
        long long dot = lane < NBIN ? static_cast<long long>(m10) * a.q20[lane] + static_cast<long long>(m01) * a.q20[NBIN + lane]
                                    : -0x7FFFFFFFFFFFFFFFLL - 1;
        int b = lane;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const long long od = __shfl_xor(dot, m, 64);
            const int ob = __shfl_xor(b, m, 64);
            if (od > dot || (od == dot && ob < b)) {
                dot = od;
                b = ob;
            }
        }
        bin = __builtin_amdgcn_readfirstlane(b);
    }
    wave_lds_sync();

    // S73 / S74: lane t evaluates tests t, t + 64, t + 128, t + 192; a ballot is eight packed bytes (S60)
    const int* tests = reinterpret_cast<const int*>(a.steer + static_cast<size_t>(bin) * (NTEST * 4));
    unsigned long long bal[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int t4 = tests[q * 64 + lane];
        const int dx1 = static_cast<signed char>(t4), dy1 = static_cast<signed char>(t4 >> 8);
        const int dx2 = static_cast<signed char>(t4 >> 16), dy2 = static_cast<signed char>(t4 >> 24);
        const unsigned b1 = s_box[(dy1 + 15) * PLANE + (dx1 + 15)], b2 = s_box[(dy2 + 15) * PLANE + (dx2 + 15)];
        bal[q] = __ballot(b1 < b2);
    }
    // one byte per lane: the caller's rows need no alignment
    if (lane < 32) {
        const int q = lane >> 3;
        const unsigned long long word = q == 0 ? bal[0] : (q == 1 ? bal[1] : (q == 2 ? bal[2] : bal[3]));
        out[lane] = static_cast<uint8_t>(word >> (8 * (lane & 7)));
    }
    if (lane == 0) {
        if (a.valid) a.valid[pt] = 1;
        if (a.bin) a.bin[pt] = static_cast<uint8_t>(bin);
    }
}

// ---- the gather form.  One workgroup selects the valid rows in order (pm::select_stable_1024); a chunk's descriptor bytes are
// then moved one per thread and step, so that a row's 32 bytes go out as one segment.
__global__ __launch_bounds__(1024) void desc_compact(const float* pts, const int32_t* d_n, int cap, const uint8_t* rows, const uint8_t* valid,
                                                     float* xy, uint8_t* desc, int32_t* src_idx, int32_t* count)
{
    __shared__ int s_dst[1024];
    const int n = pm::clamped_count(d_n, cap);
    const int tid = threadIdx.x;
    pm::select_stable_1024(
        n, count, [&](int r) { return valid[r] != 0; },
        [&](int r, int d) {
            s_dst[tid] = d;
            if (d < 0) return;
            const unsigned* p = reinterpret_cast<const unsigned*>(pts) + 2 * static_cast<size_t>(r);     // bit copies
            unsigned* o = reinterpret_cast<unsigned*>(xy) + 2 * static_cast<size_t>(d);
            o[0] = p[0];
            o[1] = p[1];
            if (src_idx) src_idx[d] = r;
        },
        [&](int r0) {
            const int m = min(1024, n - r0);
            for (int e = tid; e < m * 32; e += 1024) {
                const int k = e >> 5, byte = e & 31;
                const int dst = s_dst[k];
                if (dst >= 0) desc[static_cast<size_t>(dst) * 32 + byte] = rows[static_cast<size_t>(r0 + k) * 32 + byte];
            }
        });
}

// ---- host side -----------------------------------------------------------------------------------------------------------

int check_params(const pm_describe_params* p)
{
    PM_REQUIRE(p != nullptr, PM_E_INVALID, "null parameters");
    PM_REQUIRE(p->level >= 0 && p->level <= 7, PM_E_INVALID, "level outside [0, 7]");
    PM_REQUIRE((p->flags & ~PM_DESCRIBE_UPRIGHT) == 0, PM_E_INVALID, "unknown flag bits");
    PM_REQUIRE(p->reserved[0] == 0 && p->reserved[1] == 0, PM_E_INVALID, "reserved != 0");
    return PM_OK;
}

int check_dev_args(pm_ctx* ctx, const pm_pyramid* pyr, const float* d_pts, int cap, const pm_describe_params* p)
{
    PM_REQUIRE(pyr != nullptr && d_pts != nullptr, PM_E_INVALID, "null pyramid or points");
    const int rc = check_params(p);
    if (rc != PM_OK) return rc;
    PM_REQUIRE(p->level < pyr->nlev, PM_E_INVALID, "the pyramid has no such level");
    PM_REQUIRE(pyr->device == ctx->device, PM_E_INVALID, "pyramid of another device");
    PM_REQUIRE(cap >= 0, PM_E_INVALID, "cap < 0");
    PM_REQUIRE(cap >= 1, PM_E_UNSUPPORTED, "cap == 0: nothing to describe");
    return PM_OK;
}

// The tables go to the device once per context (a blocking copy: one synchronisation on the first call).
int tables_ready(pm_ctx* ctx)
{
    if (ctx->desc_tab) return PM_OK;
    char* mem = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&mem), TAB_BYTES) != hipSuccess) {
        pm::set_error("pm_describe_points: hipMalloc of %zu bytes failed", TAB_BYTES);
        return PM_E_NOMEM;
    }
    const DescTables& t = desc_tables();
    if (hipMemcpy(mem, t.q20, sizeof t.q20, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(mem + Q20_BYTES, t.steer, STEER_BYTES, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(mem);
        pm::set_error("pm_describe_points: the table upload failed");
        return PM_E_HIP;
    }
    ctx->desc_tab = mem;
    return PM_OK;
}

void describe_enqueue(pm_ctx* ctx, const pm_pyramid* pyr, const float* d_pts, const int32_t* d_n, int cap, const pm_describe_params* p,
                      uint8_t* d_desc, uint8_t* d_valid, uint8_t* d_bin)
{
    DescArgs a;
    memset(&a, 0, sizeof a);
    const int l = p->level;
    a.plane = pyr->mem + pyr->off[l];
    a.w = pyr->lw[l];
    a.h = pyr->lh[l];
    a.scale = 1.0f / static_cast<float>(1 << l);
    a.upright = (p->flags & PM_DESCRIBE_UPRIGHT) != 0;
    a.q20 = reinterpret_cast<const int32_t*>(ctx->desc_tab);
    a.steer = reinterpret_cast<const int8_t*>(ctx->desc_tab + Q20_BYTES);
    a.pts = d_pts;
    a.d_n = d_n;
    a.cap = cap;
    a.desc = d_desc;
    a.valid = d_valid;
    a.bin = d_bin;
    pm::ScopedKernelTime timer(ctx, "desc_points");
    hipLaunchKernelGGL(desc_points, dim3(static_cast<unsigned>((cap + WPB - 1) / WPB)), dim3(64 * WPB), 0, ctx->stream, a);
}

}  // namespace

extern "C" int pm_describe_points_dev(pm_ctx* ctx, const pm_pyramid* pyr, const float* d_pts, const int32_t* d_n, int cap,
                                      const pm_describe_params* p, uint8_t* d_desc, uint8_t* d_valid, uint8_t* d_bin)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    PM_REQUIRE(d_desc != nullptr, PM_E_INVALID, "null output pointer");
    int rc = check_dev_args(ctx, pyr, d_pts, cap, p);
    if (rc != PM_OK) return rc;
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    rc = tables_ready(ctx);
    if (rc != PM_OK) return rc;
    describe_enqueue(ctx, pyr, d_pts, d_n, cap, p, d_desc, d_valid, d_bin);
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_describe_points_gather_dev(pm_ctx* ctx, const pm_pyramid* pyr, const float* d_pts, const int32_t* d_n, int cap,
                                             const pm_describe_params* p, float* d_xy, uint8_t* d_desc, int32_t* d_src_idx,
                                             int32_t* d_count)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    PM_REQUIRE(d_xy != nullptr && d_desc != nullptr && d_count != nullptr, PM_E_INVALID, "null output pointer");
    int rc = check_dev_args(ctx, pyr, d_pts, cap, p);
    if (rc != PM_OK) return rc;
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    rc = tables_ready(ctx);
    if (rc != PM_OK) return rc;
    // the aligned rows and their flags live in the context's scratch arena
    const size_t rb = pm::align_up(static_cast<size_t>(cap) * 32, 256), vb = pm::align_up(static_cast<size_t>(cap), 256);
    rc = pm::arena_reserve(ctx, rb + vb + 512);
    if (rc != PM_OK) return rc;
    pm::arena_reset(ctx);
    uint8_t* t_rows = static_cast<uint8_t*>(pm::arena_take(ctx, rb));
    uint8_t* t_valid = static_cast<uint8_t*>(pm::arena_take(ctx, vb));
    PM_REQUIRE(t_rows != nullptr && t_valid != nullptr, PM_E_NOMEM, "scratch arena too small");
    describe_enqueue(ctx, pyr, d_pts, d_n, cap, p, t_rows, t_valid, nullptr);
    {
        pm::ScopedKernelTime timer(ctx, "desc_compact");
        hipLaunchKernelGGL(desc_compact, dim3(1), dim3(1024), 0, ctx->stream, d_pts, d_n, cap, t_rows, t_valid, d_xy, d_desc, d_src_idx,
                           d_count);
    }
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_describe_points(pm_ctx* ctx, const uint8_t* img, int w, int h, int stride, const float* pts, int n,
                                  const pm_describe_params* p, uint8_t* desc, uint8_t* valid, uint8_t* bin)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    PM_REQUIRE(img != nullptr && pts != nullptr && desc != nullptr, PM_E_INVALID, "null pointer");
    PM_REQUIRE(w >= 1 && h >= 1 && stride >= w && n >= 0, PM_E_INVALID, "need w, h >= 1, stride >= w, n >= 0");
    int rc = check_params(p);
    if (rc != PM_OK) return rc;
    PM_REQUIRE(n >= 1, PM_E_UNSUPPORTED, "n == 0: nothing to describe");
    pm_pyramid* pyr = nullptr;
    rc = pm_pyramid_create(ctx, w, h, p->level, &pyr);
    if (rc == PM_OK && p->level >= pyr->nlev) {
        pm::set_error("%s: an image of this size has no such level", __func__);
        rc = PM_E_INVALID;
    }
    if (rc == PM_OK) {                                       // the block is freed before the pyramid is destroyed
        const size_t img_b = static_cast<size_t>(h) * stride, xy_b = static_cast<size_t>(n) * 8, row_b = static_cast<size_t>(n) * 32;
        pm::StagedBlock b(ctx, __func__);
        const size_t o_img = b.add(img_b), o_pts = b.add(xy_b), o_desc = b.add(row_b), o_valid = b.add(static_cast<size_t>(n));
        const size_t o_bin = b.add(static_cast<size_t>(n));
        b.alloc();
        b.upload(o_img, img, img_b);
        b.upload(o_pts, pts, xy_b);
        if (b.rc == PM_OK) b.rc = pm_pyramid_build_dev(ctx, pyr, b.at<uint8_t>(o_img), stride);
        if (b.rc == PM_OK)
            b.rc = pm_describe_points_dev(ctx, pyr, b.at<float>(o_pts), nullptr, n, p, b.at<uint8_t>(o_desc), b.at<uint8_t>(o_valid),
                                          b.at<uint8_t>(o_bin));
        b.download(desc, o_desc, row_b);
        if (valid) b.download(valid, o_valid, static_cast<size_t>(n));
        if (bin) b.download(bin, o_bin, static_cast<size_t>(n));
        rc = b.sync();
    }
    (void)pm_pyramid_destroy(pyr);
    return rc;
}

// The tables of S72 / S73 (no GPU needed): cos_sin_q20 = C[0..35] then S[0..35]; steered = [37][256][4] offsets, row 36 the
// pattern of S58.  Either may be NULL.
extern "C" int pm_describe_points_tables(int32_t cos_sin_q20[72], int8_t steered[37 * 256 * 4])
{
    const DescTables& t = desc_tables();
    if (cos_sin_q20) memcpy(cos_sin_q20, t.q20, sizeof t.q20);
    if (steered) memcpy(steered, t.steer, sizeof t.steer);
    return PM_OK;
}
