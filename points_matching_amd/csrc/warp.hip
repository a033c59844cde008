// warp.hip — applying a 2-D model to pixels and to points: pm_warp[_dev], pm_transform_points[_dev] (docs/SPEC.md S75-S78).
//
// warp_bilinear: one thread produces four horizontally adjacent output pixels, a 256-thread workgroup (16 x 16 threads) a
// 64 x 16 output tile, so that the source footprint of a tile stays compact for the vector cache.  The model is read in the
// prologue of every thread through a wave-uniform address (and its adjugate derived there under PM_WARP_INVERT): no launch
// of its own.  Positions are fp64 exactly as S76 states them, one expression per pixel and nothing carried from pixel to
// pixel; a last row of exactly (0, 0, 1) takes a wave-uniform branch without the division.  Source taps are plain global
// byte loads; a tap of weight zero is never loaded.  The four results leave as one dword where the address is 4-byte aligned
// and all four are inside the row, as bytes otherwise (the caller's base pointer and stride may be odd).  n_valid: wave
// ballots, four wave totals through LDS, one integer atomic per workgroup.  The sample, the four-byte store and the ballot count
// live in warp_core.hpp, which undistort.hip shares; the count clamp and the host form (StagedBlock::image) in pm_common.hpp,
// the range and size rules in image_args.hpp.
//
// warp_points: one thread per point, the count protocol of pm_track_lk_dev; d_out may be d_pts (a thread reads its own row
// before it writes it).
#include <cmath>
#include <cstdint>

#include "pm_common.hpp"
#include "warp_core.hpp"

namespace {

using warp_core::TILE_W;
using warp_core::TILE_H;
using warp_core::PX;
using warp_core::sample;
using warp_core::store4;
using pm::clamped_count;

constexpr int KNOWN_FLAGS = PM_WARP_INVERT | PM_WARP_REPLICATE | PM_WARP_AFFINE;

struct Model {
    double m[9];
    int status;                                          // 0 usable, 1 singular or non-finite, 2 the zero model
};

// S75: the nine doubles the positions use, or the reason there are none.  Unfused: every product and sum is its own operation.
__device__ __forceinline__ Model load_model(const double* __restrict__ M, int flags)
{
    Model r;
    double a[9];
    const int n = (flags & PM_WARP_AFFINE) ? 6 : 9;
#pragma unroll
    for (int i = 0; i < 9; ++i) a[i] = i < n ? M[i] : (i == 8 ? 1.0 : 0.0);
    bool finite = true, zero = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        if (i < n) {
            finite = finite && isfinite(a[i]);
            zero = zero && a[i] == 0.0;
        }
    }
    const double c0 = a[4] * a[8] - a[5] * a[7], c1 = a[5] * a[6] - a[3] * a[8], c2 = a[3] * a[7] - a[4] * a[6];
    const double det = (a[0] * c0 + a[1] * c1) + a[2] * c2;
    r.status = zero ? 2 : ((!finite || det == 0.0 || !isfinite(det)) ? 1 : 0);
    if (flags & PM_WARP_INVERT) {
        r.m[0] = c0;
        r.m[1] = a[2] * a[7] - a[1] * a[8];
        r.m[2] = a[1] * a[5] - a[2] * a[4];
        r.m[3] = c1;
        r.m[4] = a[0] * a[8] - a[2] * a[6];
        r.m[5] = a[2] * a[3] - a[0] * a[5];
        r.m[6] = c2;
        r.m[7] = a[1] * a[6] - a[0] * a[7];
        r.m[8] = a[0] * a[4] - a[1] * a[3];
    } else {
#pragma unroll
        for (int i = 0; i < 9; ++i) r.m[i] = a[i];
    }
    return r;
}

struct WarpArgs {
    const uint8_t* src;
    int sw, sh, sstride;
    const double* M;
    int flags, border;
    uint8_t* dst;
    int dw, dh, dstride;
    uint8_t* valid;
    pm_warp_info* info;
};

// S76 from the homogeneous position: false = outside.
template <bool UNIT_W>
__device__ __forceinline__ bool position(double X, double Y, double W, int& qx, int& qy)
{
    double fx, fy;
    if (UNIT_W) {
        fx = X * 32.0;
        fy = Y * 32.0;
    } else {
        if (W == 0.0) return false;
        const double r = 32.0 / W;
        fx = X * r;
        fy = Y * r;
    }
    if (!(fabs(fx) < 1073741824.0) || !(fabs(fy) < 1073741824.0)) return false;      // also false for NaN and infinities
    qx = static_cast<int>(rint(fx));
    qy = static_cast<int>(rint(fy));
    return true;
}

template <bool REPLICATE, bool UNIT_W>
__device__ __forceinline__ void warp_pixels(const WarpArgs& a, const Model& mdl, int x, int y, int cnt, int out[PX], int ok[PX])
{
    const double* m = mdl.m;
    const double dy = static_cast<double>(y);
    const double ty0 = m[1] * dy, ty1 = m[4] * dy, ty2 = m[7] * dy;
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        out[j] = a.border;
        ok[j] = 0;
        if (j < cnt) {
            const double dx = static_cast<double>(x + j);
            const double X = (m[0] * dx + ty0) + m[2];
            const double Y = (m[3] * dx + ty1) + m[5];
            const double W = UNIT_W ? 1.0 : (m[6] * dx + ty2) + m[8];
            int qx, qy;
            if (position<UNIT_W>(X, Y, W, qx, qy)) {
                bool in;
                out[j] = sample<REPLICATE>(a, qx, qy, in);
                ok[j] = in ? 1 : 0;
            }
        }
    }
}

__global__ __launch_bounds__(256) void warp_bilinear(WarpArgs a)
{
    __shared__ int s_cnt[4];
    const int tid = threadIdx.x;
    const int x = blockIdx.x * TILE_W + (tid & 15) * PX, y = blockIdx.y * TILE_H + (tid >> 4);
    const Model mdl = load_model(a.M, a.flags);
    const int cnt = y < a.dh ? min(PX, a.dw - x) : 0;              // pixels of this thread inside the output (may be <= 0)
    int out[PX], ok[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        out[j] = a.border;
        ok[j] = 0;
    }
    if (mdl.status == 0 && cnt > 0) {
        const bool unit_w = mdl.m[6] == 0.0 && mdl.m[7] == 0.0 && mdl.m[8] == 1.0;        // wave-uniform
        const bool rep = (a.flags & PM_WARP_REPLICATE) != 0;
        if (unit_w) {
            if (rep) warp_pixels<true, true>(a, mdl, x, y, cnt, out, ok);
            else warp_pixels<false, true>(a, mdl, x, y, cnt, out, ok);
        } else {
            if (rep) warp_pixels<true, false>(a, mdl, x, y, cnt, out, ok);
            else warp_pixels<false, false>(a, mdl, x, y, cnt, out, ok);
        }
    }
    if (cnt > 0) {
        store4(a.dst + static_cast<size_t>(y) * a.dstride + x, out, cnt);
        if (a.valid) store4(a.valid + static_cast<size_t>(y) * a.dw + x, ok, cnt);
    }
    if (a.info) {                                                   // (kernel argument: the same for every thread)
        warp_core::block_valid_totals(ok, s_cnt, tid);
        if (tid == 0) {
            const int sum = warp_core::block_valid_sum(s_cnt);
            if (sum) atomicAdd(&a.info->n_valid, sum);
            if (blockIdx.x == 0 && blockIdx.y == 0) a.info->status = mdl.status;
        }
    }
}

// S78
__global__ __launch_bounds__(256) void warp_points(const double* __restrict__ M, int flags, const float* pts, const int32_t* d_n, int cap,
                                                   float* out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= clamped_count(d_n, cap)) return;
    const Model mdl = load_model(M, flags);
    const double* m = mdl.m;
    const double x = static_cast<double>(pts[2 * static_cast<size_t>(i)]), y = static_cast<double>(pts[2 * static_cast<size_t>(i) + 1]);
    const double X = (m[0] * x + m[1] * y) + m[2];
    const double Y = (m[3] * x + m[4] * y) + m[5];
    const double W = (m[6] * x + m[7] * y) + m[8];
    const double qx = X / W, qy = Y / W;
    float ox = static_cast<float>(qx), oy = static_cast<float>(qy);
    if (mdl.status != 0 || W == 0.0 || !isfinite(qx) || !isfinite(qy)) ox = oy = __uint_as_float(0x7FC00000u);
    out[2 * static_cast<size_t>(i)] = ox;
    out[2 * static_cast<size_t>(i) + 1] = oy;
}

// ---- host side -----------------------------------------------------------------------------------------------------------

int check_warp_args(const void* src, int sw, int sh, int sstride, const void* M, const pm_warp_params* p, const void* dst, int dw, int dh,
                    int dstride)
{
    PM_REQUIRE(src != nullptr && M != nullptr && p != nullptr && dst != nullptr, PM_E_INVALID, "null pointer");
    PM_REQUIRE((p->flags & ~KNOWN_FLAGS) == 0, PM_E_INVALID, "unknown flag bits");
    PM_REQUIRE(p->border_value >= 0 && p->border_value <= 255, PM_E_INVALID, "border_value outside [0, 255]");
    PM_REQUIRE(p->reserved[0] == 0 && p->reserved[1] == 0, PM_E_INVALID, "reserved != 0");
    PM_REQUIRE(sw >= 1 && sh >= 1 && dw >= 1 && dh >= 1, PM_E_INVALID, "need sizes >= 1");
    PM_REQUIRE(sstride >= sw && dstride >= dw, PM_E_INVALID, "a stride below its width");
    PM_REQUIRE_PASS(pm_image::pixel_cap(sw, sh));
    PM_REQUIRE_PASS(pm_image::pixel_cap(dw, dh));
    return PM_OK;
}

int check_points_args(const void* M, int flags, const void* pts, const void* out)
{
    PM_REQUIRE(M != nullptr && pts != nullptr && out != nullptr, PM_E_INVALID, "null pointer");
    PM_REQUIRE((flags & ~(PM_WARP_INVERT | PM_WARP_AFFINE)) == 0, PM_E_INVALID, "unknown flag bits");
    return PM_OK;
}

}  // namespace

extern "C" int pm_warp_dev(pm_ctx* ctx, const uint8_t* d_src, int sw, int sh, int sstride, const double* d_M, const pm_warp_params* p,
                           uint8_t* d_dst, int dw, int dh, int dstride, uint8_t* d_valid, pm_warp_info* d_info)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    const int rc = check_warp_args(d_src, sw, sh, sstride, d_M, p, d_dst, dw, dh, dstride);
    if (rc != PM_OK) return rc;
    PM_REQUIRE(!pm_image::overlap(d_src, pm_image::span(sw, sh, sstride, 1), d_dst, pm_image::span(dw, dh, dstride, 1)), PM_E_INVALID,
               "source and destination overlap");
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    if (d_info) PM_HIP_CHECK(hipMemsetAsync(d_info, 0, sizeof(pm_warp_info), ctx->stream));
    WarpArgs a;
    a.src = d_src; a.sw = sw; a.sh = sh; a.sstride = sstride;
    a.M = d_M; a.flags = p->flags; a.border = p->border_value;
    a.dst = d_dst; a.dw = dw; a.dh = dh; a.dstride = dstride;
    a.valid = d_valid; a.info = d_info;
    {
        pm::ScopedKernelTime timer(ctx, "warp_bilinear");
        hipLaunchKernelGGL(warp_bilinear, dim3(static_cast<unsigned>((dw + TILE_W - 1) / TILE_W), static_cast<unsigned>((dh + TILE_H - 1) / TILE_H)),
                           dim3(256), 0, ctx->stream, a);
    }
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_warp(pm_ctx* ctx, const uint8_t* src, int sw, int sh, int sstride, const double* M, const pm_warp_params* p, uint8_t* dst,
                       int dw, int dh, int dstride, uint8_t* valid, pm_warp_info* info)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    const int rc = check_warp_args(src, sw, sh, sstride, M, p, dst, dw, dh, dstride);
    if (rc != PM_OK) return rc;
    const size_t m_b = sizeof(double) * ((p->flags & PM_WARP_AFFINE) ? 6 : 9);
    auto dev = [&](const void* d_M, const uint8_t* d_src, uint8_t* d_dst, uint8_t* d_valid, pm_warp_info* d_info) {
        return pm_warp_dev(ctx, d_src, sw, sh, sstride, static_cast<const double*>(d_M), p, d_dst, dw, dh, dstride, d_valid, d_info);
    };
    return pm::StagedBlock::image(ctx, __func__, M, m_b, src, sw, sh, sstride, dst, dw, dh, dstride, valid, info, dev);
}

extern "C" int pm_transform_points_dev(pm_ctx* ctx, const double* d_M, int flags, const float* d_pts, const int32_t* d_n, int cap,
                                       float* d_out)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    const int rc = check_points_args(d_M, flags, d_pts, d_out);
    if (rc != PM_OK) return rc;
    PM_REQUIRE(cap >= 0, PM_E_INVALID, "cap < 0");
    PM_REQUIRE(cap >= 1, PM_E_UNSUPPORTED, "cap == 0: nothing to transform");
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    {
        pm::ScopedKernelTime timer(ctx, "warp_points");
        hipLaunchKernelGGL(warp_points, dim3(static_cast<unsigned>((cap + 255) / 256)), dim3(256), 0, ctx->stream, d_M, flags, d_pts, d_n, cap,
                           d_out);
    }
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_transform_points(pm_ctx* ctx, const double* M, int flags, const float* pts, int n, float* out)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    const int rc = check_points_args(M, flags, pts, out);
    if (rc != PM_OK) return rc;
    PM_REQUIRE(n >= 0, PM_E_INVALID, "n < 0");
    PM_REQUIRE(n >= 1, PM_E_UNSUPPORTED, "n == 0: nothing to transform");
    const size_t m_b = sizeof(double) * ((flags & PM_WARP_AFFINE) ? 6 : 9), xy_b = static_cast<size_t>(n) * 8;
    pm::StagedBlock b(ctx, __func__);
    const size_t o_m = b.add(m_b), o_pts = b.add(xy_b);
    b.alloc();
    b.upload(o_m, M, m_b);
    b.upload(o_pts, pts, xy_b);
    if (b.rc == PM_OK) b.rc = pm_transform_points_dev(ctx, b.at<double>(o_m), flags, b.at<float>(o_pts), nullptr, n, b.at<float>(o_pts));
    b.download(out, o_pts, xy_b);
    return b.sync();
}
