// undistort.hip — the lens model in front of the calibrated estimators and of the image front end: pm_undistort_points[_dev],
// pm_distort_points[_dev], pm_undistort[_dev], pm_undistort_map_dev, pm_remap[_dev] (docs/SPEC.md S79-S83).
//
// Camera, new camera, lens and R are host values: they are checked on the host and travel as ONE kernel argument by value
// (LensArgs), so no kernel reads the model from memory and there is no setup launch.  The arithmetic is fp64, a polynomial
// and divisions, every product and sum its own operation (the build keeps -ffp-contract=off).
//
// undistort_bilinear / undistort_map / remap_q5 take warp_bilinear's geometry (warp_core.hpp): four horizontally adjacent
// output pixels per thread, a 64 x 16 tile per 256-thread workgroup, dword stores where aligned, one integer atomic per
// workgroup for n_valid.  The terms that depend on the row alone (y, y * y, the three products of R with y) are computed once
// per thread.  R == NULL and an all-zero lens take wave-uniform branches (template instantiations chosen from kernel
// arguments): without R the rotation step is not there at all, as S80 states it; with a zero lens S79 leaves (x, y) as they
// are up to the sign of a zero, which rint(32 * s) does not keep, so the position bits are those of the general path.
// remap_q5 reads its 8-byte map entry with a plain global load: the non-temporal form measured 3 % slower.
//
// undistort_points / distort_points: one thread per point, the count protocol of warp_points; d_out may be d_pts.
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
using pm_image::overlap;
using pm_image::span;

struct LensArgs {
    double fx, fy, cx, cy;              // K: the camera the lens belongs to
    double ifx, ify;                    // 1.0 / fx, 1.0 / fy
    double nfx, nfy, ncx, ncy;          // K_new
    double nifx, nify;                  // 1.0 / nfx, 1.0 / nfy
    double k1, k2, p1, p2, k3;
    double R[9];
    int has_R, has_lens;                // R given; any coefficient non-zero
};

// S79 on normalised (x, y): the distorted normalised position and rad.
__device__ __forceinline__ void forward(const LensArgs& L, double x, double y, double& xd, double& yd, double& rad)
{
    const double xx = x * x, yy = y * y, r2 = xx + yy;
    rad = 1.0 + ((L.k3 * r2 + L.k2) * r2 + L.k1) * r2;
    const double dX = 2.0 * L.p1 * x * y + L.p2 * (r2 + 2.0 * xx);
    const double dY = L.p1 * (r2 + 2.0 * yy) + 2.0 * L.p2 * x * y;
    xd = x * rad + dX;
    yd = y * rad + dY;
}

// S80 after the normalisation: (x, y) under K_new -> the pixel under K; false = no position.  ry[3] = R[3] * y, R[4] * y,
// R[5] * y of the caller's y (used with HAS_R), yy = y * y (used without).
template <bool HAS_R, bool HAS_LENS>
__device__ __forceinline__ bool distort(const LensArgs& L, double x, double y, const double ry[3], double yy, double& u, double& v)
{
    if (HAS_R) {
        const double X = (L.R[0] * x + ry[0]) + L.R[6];
        const double Y = (L.R[1] * x + ry[1]) + L.R[7];
        const double Z = (L.R[2] * x + ry[2]) + L.R[8];
        if (!(Z > 0.0)) return false;
        const double iz = 1.0 / Z;
        x = X * iz;
        y = Y * iz;
        yy = y * y;
    }
    if (HAS_LENS) {
        const double xx = x * x, r2 = xx + yy;
        const double rad = 1.0 + ((L.k3 * r2 + L.k2) * r2 + L.k1) * r2;
        if (!(rad > 0.0)) return false;
        const double dX = 2.0 * L.p1 * x * y + L.p2 * (r2 + 2.0 * xx);
        const double dY = L.p1 * (r2 + 2.0 * yy) + 2.0 * L.p2 * x * y;
        x = x * rad + dX;
        y = y * rad + dY;
    }
    u = L.fx * x + L.cx;
    v = L.fy * y + L.cy;
    return isfinite(u) && isfinite(v);
}

// S82: the Q5 position of an output pixel; false = unusable.
template <bool HAS_R, bool HAS_LENS>
__device__ __forceinline__ bool position(const LensArgs& L, int px, double y, const double ry[3], double yy, int& qx, int& qy)
{
    const double x = (static_cast<double>(px) - L.ncx) * L.nifx;
    double u, v;
    if (!distort<HAS_R, HAS_LENS>(L, x, y, ry, yy, u, v)) return false;
    const double fx = u * 32.0, fy = v * 32.0;
    if (!(fabs(fx) < 1073741824.0) || !(fabs(fy) < 1073741824.0)) return false;
    qx = static_cast<int>(rint(fx));
    qy = static_cast<int>(rint(fy));
    return true;
}

struct ImageArgs {
    const uint8_t* src;
    int sw, sh, sstride;
    int replicate, border;
    uint8_t* dst;
    int dw, dh, dstride;
    uint8_t* valid;
    pm_warp_info* info;
};

// the tail of the three image kernels: the four results, their valid bytes, one atomic per workgroup
__device__ __forceinline__ void finish(const ImageArgs& a, int x, int y, int cnt, const int out[PX], const int ok[PX], int* s_cnt, int tid)
{
    if (cnt > 0) {
        store4(a.dst + static_cast<size_t>(y) * a.dstride + x, out, cnt);
        if (a.valid) store4(a.valid + static_cast<size_t>(y) * a.dw + x, ok, cnt);
    }
    if (a.info) {                                                   // (kernel argument: the same for every thread)
        warp_core::block_valid_totals(ok, s_cnt, tid);
        if (tid == 0) {
            const int sum = warp_core::block_valid_sum(s_cnt);
            if (sum) atomicAdd(&a.info->n_valid, sum);
        }
    }
}

// the Q5 positions of a thread's four pixels; (INT32_MIN, INT32_MIN) where there is none (S83's mark)
template <bool HAS_R, bool HAS_LENS>
__device__ __forceinline__ void row_positions(const LensArgs& L, int x, int y, int cnt, int qx[PX], int qy[PX])
{
    const double yn = (static_cast<double>(y) - L.ncy) * L.nify;
    const double ry[3] = {L.R[3] * yn, L.R[4] * yn, L.R[5] * yn};
    const double yy = yn * yn;
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        int a = 0, b = 0;
        const bool ok = j < cnt && position<HAS_R, HAS_LENS>(L, x + j, yn, ry, yy, a, b);
        qx[j] = ok ? a : INT32_MIN;
        qy[j] = ok ? b : INT32_MIN;
    }
}

__device__ __forceinline__ void positions(const LensArgs& L, int x, int y, int cnt, int qx[PX], int qy[PX])
{
    if (L.has_R) {                                                  // wave-uniform: kernel arguments
        if (L.has_lens) row_positions<true, true>(L, x, y, cnt, qx, qy);
        else row_positions<true, false>(L, x, y, cnt, qx, qy);
    } else {
        if (L.has_lens) row_positions<false, true>(L, x, y, cnt, qx, qy);
        else row_positions<false, false>(L, x, y, cnt, qx, qy);
    }
}

// S77 at four positions; the pair (INT32_MIN, INT32_MIN) is not sampled
__device__ __forceinline__ void sample4(const ImageArgs& a, int cnt, const int qx[PX], const int qy[PX], int out[PX], int ok[PX])
{
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        out[j] = a.border;
        ok[j] = 0;
        if (j < cnt && !(qx[j] == INT32_MIN && qy[j] == INT32_MIN)) {
            bool in;
            out[j] = a.replicate ? sample<true>(a, qx[j], qy[j], in) : sample<false>(a, qx[j], qy[j], in);
            ok[j] = in ? 1 : 0;
        }
    }
}

// S82 + S77, fused
__global__ __launch_bounds__(256) void undistort_bilinear(ImageArgs a, LensArgs L)
{
    __shared__ int s_cnt[4];
    const int tid = threadIdx.x;
    const int x = blockIdx.x * TILE_W + (tid & 15) * PX, y = blockIdx.y * TILE_H + (tid >> 4);
    const int cnt = y < a.dh ? min(PX, a.dw - x) : 0;              // pixels of this thread inside the output (may be <= 0)
    int qx[PX], qy[PX], out[PX], ok[PX];
    positions(L, x, y, cnt, qx, qy);
    sample4(a, cnt, qx, qy, out, ok);
    finish(a, x, y, cnt, out, ok, s_cnt, tid);
}

// S83: the map alone, (qx, qy) pairs, (INT32_MIN, INT32_MIN) where S82 has no usable position
__global__ __launch_bounds__(256) void undistort_map(LensArgs L, int dw, int dh, int2* map)
{
    const int tid = threadIdx.x;
    const int x = blockIdx.x * TILE_W + (tid & 15) * PX, y = blockIdx.y * TILE_H + (tid >> 4);
    const int cnt = y < dh ? min(PX, dw - x) : 0;
    int qx[PX], qy[PX];
    positions(L, x, y, cnt, qx, qy);
#pragma unroll
    for (int j = 0; j < PX; ++j)
        if (j < cnt) map[static_cast<size_t>(y) * dw + x + j] = make_int2(qx[j], qy[j]);
}

// S83: S77 at the positions of a map
__global__ __launch_bounds__(256) void remap_q5(ImageArgs a, const int2* __restrict__ map)
{
    __shared__ int s_cnt[4];
    const int tid = threadIdx.x;
    const int x = blockIdx.x * TILE_W + (tid & 15) * PX, y = blockIdx.y * TILE_H + (tid >> 4);
    const int cnt = y < a.dh ? min(PX, a.dw - x) : 0;
    int qx[PX], qy[PX], out[PX], ok[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        qx[j] = qy[j] = INT32_MIN;
        if (j < cnt) {
            const int2 q = map[static_cast<size_t>(y) * a.dw + x + j];
            qx[j] = q.x;
            qy[j] = q.y;
        }
    }
    sample4(a, cnt, qx, qy, out, ok);
    finish(a, x, y, cnt, out, ok, s_cnt, tid);
}

__device__ __forceinline__ void store_point(float* out, int i, bool ok, double u, double v)
{
    float ou = static_cast<float>(u), ov = static_cast<float>(v);
    if (!ok) ou = ov = __uint_as_float(0x7FC00000u);
    out[2 * static_cast<size_t>(i)] = ou;
    out[2 * static_cast<size_t>(i) + 1] = ov;
}

// S80
__global__ __launch_bounds__(256) void distort_points(LensArgs L, const float* pts, const int32_t* d_n, int cap, float* out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= clamped_count(d_n, cap)) return;
    const double x = (static_cast<double>(pts[2 * static_cast<size_t>(i)]) - L.ncx) * L.nifx;
    const double y = (static_cast<double>(pts[2 * static_cast<size_t>(i) + 1]) - L.ncy) * L.nify;
    const double ry[3] = {L.R[3] * y, L.R[4] * y, L.R[5] * y};
    double u = 0.0, v = 0.0;
    const bool ok = L.has_R ? distort<true, true>(L, x, y, ry, y * y, u, v) : distort<false, true>(L, x, y, ry, y * y, u, v);
    store_point(out, i, ok, u, v);
}

// S81
__global__ __launch_bounds__(256) void undistort_points(LensArgs L, int iters, double tol2, const float* pts, const int32_t* d_n, int cap, float* out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= clamped_count(d_n, cap)) return;
    const double x0 = (static_cast<double>(pts[2 * static_cast<size_t>(i)]) - L.cx) * L.ifx;
    const double y0 = (static_cast<double>(pts[2 * static_cast<size_t>(i) + 1]) - L.cy) * L.ify;
    double x = x0, y = y0;
    for (int it = 0; it < iters; ++it) {
        const double xx = x * x, yy = y * y, r2 = xx + yy;
        const double ic = 1.0 / (1.0 + ((L.k3 * r2 + L.k2) * r2 + L.k1) * r2);
        const double dX = 2.0 * L.p1 * x * y + L.p2 * (r2 + 2.0 * xx);
        const double dY = L.p1 * (r2 + 2.0 * yy) + 2.0 * L.p2 * x * y;
        x = (x0 - dX) * ic;
        y = (y0 - dY) * ic;
    }
    double xd, yd, rad;
    forward(L, x, y, xd, yd, rad);
    const double ex = L.fx * (xd - x0), ey = L.fy * (yd - y0);
    bool ok = rad > 0.0 && ex * ex + ey * ey <= tol2;                // false for NaN
    if (L.has_R) {
        const double X = (L.R[0] * x + L.R[1] * y) + L.R[2];
        const double Y = (L.R[3] * x + L.R[4] * y) + L.R[5];
        const double Z = (L.R[6] * x + L.R[7] * y) + L.R[8];
        ok = ok && Z > 0.0;
        const double iz = 1.0 / Z;
        x = X * iz;
        y = Y * iz;
    }
    const double u = L.nfx * x + L.ncx, v = L.nfy * y + L.ncy;
    store_point(out, i, ok && isfinite(u) && isfinite(v), u, v);
}

// ---- host side -----------------------------------------------------------------------------------------------------------

bool camera_ok(const pm_camera* K)
{
    return std::isfinite(K->fx) && std::isfinite(K->fy) && std::isfinite(K->cx) && std::isfinite(K->cy) && K->fx > 0.0 && K->fy > 0.0;
}

// K, lens, R, K_new as the caller gave them -> the kernel argument
int make_lens(const pm_camera* K, const pm_lens* lens, const double* R, const pm_camera* K_new, LensArgs* L)
{
    PM_REQUIRE(K != nullptr, PM_E_INVALID, "K is null");
    PM_REQUIRE(camera_ok(K), PM_E_INVALID, "K needs finite values and fx, fy > 0");
    const pm_camera* N = K_new ? K_new : K;
    PM_REQUIRE(camera_ok(N), PM_E_INVALID, "K_new needs finite values and fx, fy > 0");
    L->fx = K->fx; L->fy = K->fy; L->cx = K->cx; L->cy = K->cy;
    L->ifx = 1.0 / K->fx; L->ify = 1.0 / K->fy;
    L->nfx = N->fx; L->nfy = N->fy; L->ncx = N->cx; L->ncy = N->cy;
    L->nifx = 1.0 / N->fx; L->nify = 1.0 / N->fy;
    L->k1 = L->k2 = L->p1 = L->p2 = L->k3 = 0.0;
    L->has_lens = 0;
    if (lens) {
        PM_REQUIRE(std::isfinite(lens->k1) && std::isfinite(lens->k2) && std::isfinite(lens->p1) && std::isfinite(lens->p2) && std::isfinite(lens->k3),
                   PM_E_INVALID, "a lens coefficient is not finite");
        L->k1 = lens->k1; L->k2 = lens->k2; L->p1 = lens->p1; L->p2 = lens->p2; L->k3 = lens->k3;
        L->has_lens = (lens->k1 != 0.0 || lens->k2 != 0.0 || lens->p1 != 0.0 || lens->p2 != 0.0 || lens->k3 != 0.0) ? 1 : 0;
    }
    L->has_R = R ? 1 : 0;
    for (int i = 0; i < 9; ++i) {
        PM_REQUIRE(!R || std::isfinite(R[i]), PM_E_INVALID, "an entry of R is not finite");
        L->R[i] = R ? R[i] : (i % 4 == 0 ? 1.0 : 0.0);
    }
    return PM_OK;
}

int check_params(const pm_warp_params* p)
{
    PM_REQUIRE(p != nullptr, PM_E_INVALID, "null pointer");
    PM_REQUIRE((p->flags & ~PM_WARP_REPLICATE) == 0, PM_E_INVALID, "unknown flag bits");
    PM_REQUIRE(p->border_value >= 0 && p->border_value <= 255, PM_E_INVALID, "border_value outside [0, 255]");
    PM_REQUIRE(p->reserved[0] == 0 && p->reserved[1] == 0, PM_E_INVALID, "reserved != 0");
    return PM_OK;
}

int check_image_args(const void* src, int sw, int sh, int sstride, const pm_warp_params* p, const void* dst, int dw, int dh, int dstride)
{
    PM_REQUIRE(src != nullptr && dst != nullptr, PM_E_INVALID, "null pointer");
    const int rc = check_params(p);
    if (rc != PM_OK) return rc;
    PM_REQUIRE(sw >= 1 && sh >= 1 && dw >= 1 && dh >= 1, PM_E_INVALID, "need sizes >= 1");
    PM_REQUIRE(sstride >= sw && dstride >= dw, PM_E_INVALID, "a stride below its width");
    PM_REQUIRE_PASS(pm_image::pixel_cap(sw, sh));
    PM_REQUIRE_PASS(pm_image::pixel_cap(dw, dh));
    return PM_OK;
}

ImageArgs image_args(const uint8_t* src, int sw, int sh, int sstride, const pm_warp_params* p, uint8_t* dst, int dw, int dh, int dstride,
                     uint8_t* valid, pm_warp_info* info)
{
    ImageArgs a;
    a.src = src; a.sw = sw; a.sh = sh; a.sstride = sstride;
    a.replicate = (p->flags & PM_WARP_REPLICATE) != 0; a.border = p->border_value;
    a.dst = dst; a.dw = dw; a.dh = dh; a.dstride = dstride;
    a.valid = valid; a.info = info;
    return a;
}

dim3 tiles(int dw, int dh) { return dim3(static_cast<unsigned>((dw + TILE_W - 1) / TILE_W), static_cast<unsigned>((dh + TILE_H - 1) / TILE_H)); }

int check_points_args(const void* pts, const void* out, int n, const char* zero_msg)
{
    PM_REQUIRE(pts != nullptr && out != nullptr, PM_E_INVALID, "null pointer");
    PM_REQUIRE(n >= 0, PM_E_INVALID, "cap or n < 0");
    PM_REQUIRE(n >= 1, PM_E_UNSUPPORTED, zero_msg);
    return PM_OK;
}

int check_solver(int iters, double tol_px)
{
    PM_REQUIRE(iters >= 1 && iters <= 50, PM_E_INVALID, "iters outside [1, 50]");
    PM_REQUIRE(std::isfinite(tol_px) && tol_px > 0.0, PM_E_INVALID, "tol_px must be finite and > 0");
    return PM_OK;
}

}  // namespace

extern "C" int pm_undistort_dev(pm_ctx* ctx, const uint8_t* d_src, int sw, int sh, int sstride, const pm_camera* K, const pm_lens* lens,
                                const double* R, const pm_camera* K_new, const pm_warp_params* p, uint8_t* d_dst, int dw, int dh, int dstride,
                                uint8_t* d_valid, pm_warp_info* d_info)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    int rc = check_image_args(d_src, sw, sh, sstride, p, d_dst, dw, dh, dstride);
    if (rc != PM_OK) return rc;
    LensArgs L;
    rc = make_lens(K, lens, R, K_new, &L);
    if (rc != PM_OK) return rc;
    PM_REQUIRE(!overlap(d_src, span(sw, sh, sstride, 1), d_dst, span(dw, dh, dstride, 1)), PM_E_INVALID, "source and destination overlap");
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    if (d_info) PM_HIP_CHECK(hipMemsetAsync(d_info, 0, sizeof(pm_warp_info), ctx->stream));
    const ImageArgs a = image_args(d_src, sw, sh, sstride, p, d_dst, dw, dh, dstride, d_valid, d_info);
    {
        pm::ScopedKernelTime timer(ctx, "undistort_bilinear");
        hipLaunchKernelGGL(undistort_bilinear, tiles(dw, dh), dim3(256), 0, ctx->stream, a, L);
    }
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_undistort(pm_ctx* ctx, const uint8_t* src, int sw, int sh, int sstride, const pm_camera* K, const pm_lens* lens, const double* R,
                            const pm_camera* K_new, const pm_warp_params* p, uint8_t* dst, int dw, int dh, int dstride, uint8_t* valid,
                            pm_warp_info* info)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    int rc = check_image_args(src, sw, sh, sstride, p, dst, dw, dh, dstride);
    if (rc != PM_OK) return rc;
    LensArgs L;
    rc = make_lens(K, lens, R, K_new, &L);
    if (rc != PM_OK) return rc;
    auto dev = [&](const void*, const uint8_t* d_src, uint8_t* d_dst, uint8_t* d_valid, pm_warp_info* d_info) {
        return pm_undistort_dev(ctx, d_src, sw, sh, sstride, K, lens, R, K_new, p, d_dst, dw, dh, dstride, d_valid, d_info);
    };
    return pm::StagedBlock::image(ctx, __func__, nullptr, 0, src, sw, sh, sstride, dst, dw, dh, dstride, valid, info, dev);
}

extern "C" int pm_undistort_map_dev(pm_ctx* ctx, const pm_camera* K, const pm_lens* lens, const double* R, const pm_camera* K_new, int dw, int dh,
                                    int32_t* d_map)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    PM_REQUIRE(d_map != nullptr, PM_E_INVALID, "null pointer");
    PM_REQUIRE((reinterpret_cast<uintptr_t>(d_map) & 7) == 0, PM_E_INVALID, "d_map is not 8-byte aligned");
    PM_REQUIRE(dw >= 1 && dh >= 1, PM_E_INVALID, "need sizes >= 1");
    PM_REQUIRE_PASS(pm_image::pixel_cap(dw, dh));
    LensArgs L;
    const int rc = make_lens(K, lens, R, K_new, &L);
    if (rc != PM_OK) return rc;
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    {
        pm::ScopedKernelTime timer(ctx, "undistort_map");
        hipLaunchKernelGGL(undistort_map, tiles(dw, dh), dim3(256), 0, ctx->stream, L, dw, dh, reinterpret_cast<int2*>(d_map));
    }
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_remap_dev(pm_ctx* ctx, const uint8_t* d_src, int sw, int sh, int sstride, const int32_t* d_map, const pm_warp_params* p,
                            uint8_t* d_dst, int dw, int dh, int dstride, uint8_t* d_valid, pm_warp_info* d_info)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    PM_REQUIRE(d_map != nullptr, PM_E_INVALID, "null pointer");
    const int rc = check_image_args(d_src, sw, sh, sstride, p, d_dst, dw, dh, dstride);
    if (rc != PM_OK) return rc;
    PM_REQUIRE((reinterpret_cast<uintptr_t>(d_map) & 7) == 0, PM_E_INVALID, "d_map is not 8-byte aligned");
    const size_t dst_b = span(dw, dh, dstride, 1);
    PM_REQUIRE(!overlap(d_src, span(sw, sh, sstride, 1), d_dst, dst_b), PM_E_INVALID, "source and destination overlap");
    PM_REQUIRE(!overlap(d_map, static_cast<size_t>(dw) * dh * 8, d_dst, dst_b), PM_E_INVALID, "map and destination overlap");
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    if (d_info) PM_HIP_CHECK(hipMemsetAsync(d_info, 0, sizeof(pm_warp_info), ctx->stream));
    const ImageArgs a = image_args(d_src, sw, sh, sstride, p, d_dst, dw, dh, dstride, d_valid, d_info);
    {
        pm::ScopedKernelTime timer(ctx, "remap_q5");
        hipLaunchKernelGGL(remap_q5, tiles(dw, dh), dim3(256), 0, ctx->stream, a, reinterpret_cast<const int2*>(d_map));
    }
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_remap(pm_ctx* ctx, const uint8_t* src, int sw, int sh, int sstride, const int32_t* map, const pm_warp_params* p, uint8_t* dst,
                        int dw, int dh, int dstride, uint8_t* valid, pm_warp_info* info)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    PM_REQUIRE(map != nullptr, PM_E_INVALID, "null pointer");
    const int rc = check_image_args(src, sw, sh, sstride, p, dst, dw, dh, dstride);
    if (rc != PM_OK) return rc;
    auto dev = [&](const void* d_map, const uint8_t* d_src, uint8_t* d_dst, uint8_t* d_valid, pm_warp_info* d_info) {
        return pm_remap_dev(ctx, d_src, sw, sh, sstride, static_cast<const int32_t*>(d_map), p, d_dst, dw, dh, dstride, d_valid, d_info);
    };
    return pm::StagedBlock::image(ctx, __func__, map, static_cast<size_t>(dw) * dh * 8, src, sw, sh, sstride, dst, dw, dh, dstride, valid, info, dev);
}

extern "C" int pm_undistort_points_dev(pm_ctx* ctx, const pm_camera* K, const pm_lens* lens, const double* R, const pm_camera* K_new, int iters,
                                       double tol_px, const float* d_pts, const int32_t* d_n, int cap, float* d_out)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    int rc = check_points_args(d_pts, d_out, cap, "cap == 0: nothing to undistort");
    if (rc == PM_OK) rc = check_solver(iters, tol_px);
    if (rc != PM_OK) return rc;
    LensArgs L;
    rc = make_lens(K, lens, R, K_new, &L);
    if (rc != PM_OK) return rc;
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    {
        pm::ScopedKernelTime timer(ctx, "undistort_points");
        hipLaunchKernelGGL(undistort_points, dim3(static_cast<unsigned>((cap + 255) / 256)), dim3(256), 0, ctx->stream, L, iters, tol_px * tol_px,
                           d_pts, d_n, cap, d_out);
    }
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_distort_points_dev(pm_ctx* ctx, const pm_camera* K, const pm_lens* lens, const double* R, const pm_camera* K_new,
                                     const float* d_pts, const int32_t* d_n, int cap, float* d_out)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    int rc = check_points_args(d_pts, d_out, cap, "cap == 0: nothing to distort");
    if (rc != PM_OK) return rc;
    LensArgs L;
    rc = make_lens(K, lens, R, K_new, &L);
    if (rc != PM_OK) return rc;
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    {
        pm::ScopedKernelTime timer(ctx, "distort_points");
        hipLaunchKernelGGL(distort_points, dim3(static_cast<unsigned>((cap + 255) / 256)), dim3(256), 0, ctx->stream, L, d_pts, d_n, cap, d_out);
    }
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

namespace {

// the host forms of the two point calls: one staged block, transformed in place on the device
template <class Dev>
int points_host(pm_ctx* ctx, const char* who, const float* pts, int n, float* out, Dev dev)
{
    const size_t xy_b = static_cast<size_t>(n) * 8;
    pm::StagedBlock b(ctx, who);
    const size_t o_pts = b.add(xy_b);
    b.alloc();
    b.upload(o_pts, pts, xy_b);
    if (b.rc == PM_OK) b.rc = dev(b.at<float>(o_pts));
    b.download(out, o_pts, xy_b);
    return b.sync();
}

}  // namespace

extern "C" int pm_undistort_points(pm_ctx* ctx, const pm_camera* K, const pm_lens* lens, const double* R, const pm_camera* K_new, int iters,
                                   double tol_px, const float* pts, int n, float* out)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    int rc = check_points_args(pts, out, n, "n == 0: nothing to undistort");
    if (rc == PM_OK) rc = check_solver(iters, tol_px);
    if (rc != PM_OK) return rc;
    LensArgs L;
    rc = make_lens(K, lens, R, K_new, &L);
    if (rc != PM_OK) return rc;
    return points_host(ctx, __func__, pts, n, out,
                       [&](float* d) { return pm_undistort_points_dev(ctx, K, lens, R, K_new, iters, tol_px, d, nullptr, n, d); });
}

extern "C" int pm_distort_points(pm_ctx* ctx, const pm_camera* K, const pm_lens* lens, const double* R, const pm_camera* K_new, const float* pts,
                                 int n, float* out)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    int rc = check_points_args(pts, out, n, "n == 0: nothing to distort");
    if (rc != PM_OK) return rc;
    LensArgs L;
    rc = make_lens(K, lens, R, K_new, &L);
    if (rc != PM_OK) return rc;
    return points_host(ctx, __func__, pts, n, out, [&](float* d) { return pm_distort_points_dev(ctx, K, lens, R, K_new, d, nullptr, n, d); });
}
