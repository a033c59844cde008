// track_lk.hip — sparse optical-flow tracking: pyramidal Lucas-Kanade on the device (docs/SPEC.md S61-S66).  The counterpart
// of cv::calcOpticalFlowPyrLK / cv::cuda::SparsePyrLKOpticalFlow for a frame-to-frame front end: the previous frame's points
// are tracked into the next frame, and the survivors leave as the two compacted xy arrays and the device-side count that
// every *_run_dev estimator takes as a pm_points_view.
//
// Every sum of S61-S66 is an exact integer sum (samples are grey level x 32 in int16, products and sums in int64), so the
// lanes of a wave may add in any order and the bits stay a function of the two images alone.  The handful of fp64 operations
// (determinant, eigenvalue, the 2 x 2 solve) run redundantly on all 64 lanes, so every branch is wave-uniform.
//
// Launches, all on the context's stream:
//   lk_pyr_down   one per pyramid level: 5-tap binomial, separable through an LDS tile, integer arithmetic (S61)
//   lk_track      one wave per point: level loop, iteration loop and the backward track of the forward-backward check
//   lk_compact    the gather form only: one workgroup scans the status-1 flags in input order and moves the rows (S66)
#include <algorithm>

#include "pm_common.hpp"
#include "pyramid.hpp"
#include "wave_ops.hpp"

namespace {

constexpr int MAX_LEV = 8;
constexpr int MAX_R = 15;
constexpr int T_MAX = (2 * MAX_R + 3) * (2 * MAX_R + 3);      // template with its one-sample rim: 33 x 33
constexpr int G_MAX = (2 * MAX_R + 1) * (2 * MAX_R + 1);      // gradient planes: 31 x 31
constexpr int WAVE_SHORTS = (T_MAX + 2 * G_MAX + 7) & ~7;     // 3016 shorts = 6032 bytes of LDS per wave
constexpr int WPB = 4;                                        // waves (= points) per workgroup

struct PyrDesc {
    const uint8_t* base;
    int nlev, pad;
    int w[MAX_LEV], h[MAX_LEV];
    size_t off[MAX_LEV];
};

struct LkArgs {
    PyrDesc pyr[2];                    // [0] previous frame, [1] next frame; the backward track swaps the roles
    pm_lk_params prm;
    const float* pts;
    const int32_t* d_n;
    const float* init;
    float* out;
    uint8_t* status;
    float* err;
    float* fb;
    int cap, pad;
};

// ---- S61: one level.  A workgroup makes a 32 x 8 output tile: the 67 x 19 input pixels it needs go to LDS (reflected without
// repeating the edge pixel), the x pass leaves 19 rows of 32 sums, the y pass adds five of them.  Integers throughout.
constexpr int PT_X = 32, PT_Y = 8, PIN_X = 2 * PT_X + 3, PIN_Y = 2 * PT_Y + 3;
__device__ __forceinline__ int r101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

__global__ __launch_bounds__(256) void lk_pyr_down(const uint8_t* in, int w, int h, uint8_t* out, int ow, int oh)
{
    __shared__ unsigned char s_in[PIN_Y][PIN_X + 1];
    __shared__ unsigned short s_row[PIN_Y][PT_X];
    const int tid = threadIdx.x;
    const int ox0 = blockIdx.x * PT_X, oy0 = blockIdx.y * PT_Y;
    for (int e = tid; e < PIN_Y * PIN_X; e += 256) {
        const int jy = e / PIN_X, jx = e - jy * PIN_X;
        // (rows and columns past the last output pixel of a partial tile are clamped into the plane: they feed no output)
        const int ys = r101(min(2 * oy0 - 2 + jy, h + 1), h), xs = r101(min(2 * ox0 - 2 + jx, w + 1), w);
        s_in[jy][jx] = in[static_cast<size_t>(ys) * w + xs];
    }
    __syncthreads();
    for (int e = tid; e < PIN_Y * PT_X; e += 256) {
        const int jy = e / PT_X, tx = e - jy * PT_X;
        const unsigned char* p = &s_in[jy][2 * tx];
        s_row[jy][tx] = static_cast<unsigned short>(p[0] + 4 * p[1] + 6 * p[2] + 4 * p[3] + p[4]);
    }
    __syncthreads();
    const int tx = tid & (PT_X - 1), ty = tid / PT_X;
    const int x = ox0 + tx, y = oy0 + ty;
    if (x < ow && y < oh) {
        const int s = s_row[2 * ty][tx] + 4 * s_row[2 * ty + 1][tx] + 6 * s_row[2 * ty + 2][tx] + 4 * s_row[2 * ty + 3][tx] +
                      s_row[2 * ty + 4][tx];
        out[static_cast<size_t>(y) * ow + x] = static_cast<uint8_t>((s + 128) >> 8);
    }
}

// ---- S62: origin and the four 14-bit weights of a window with top-left (px, py); false when the window leaves the level
struct Win {
    int ix, iy, w00, w01, w10, w11;
};

__device__ __forceinline__ bool window_origin(float px, float py, int n, int w, int h, Win& o)
{
    if (!(fabsf(px) <= 1e6f) || !(fabsf(py) <= 1e6f)) return false;          // NaN, infinity, beyond 1e6
    const float fx = floorf(px), fy = floorf(py);
    const float a = px - fx, b = py - fy;
    o.w00 = static_cast<int>(rintf(((1.0f - a) * (1.0f - b)) * 16384.0f));
    o.w01 = static_cast<int>(rintf((a * (1.0f - b)) * 16384.0f));
    o.w10 = static_cast<int>(rintf(((1.0f - a) * b) * 16384.0f));
    o.w11 = 16384 - o.w00 - o.w01 - o.w10;
    o.ix = static_cast<int>(fx);
    o.iy = static_cast<int>(fy);
    return o.ix >= 0 && o.iy >= 0 && o.ix + n <= w - 1 && o.iy + n <= h - 1;
}

__device__ __forceinline__ int sample(const uint8_t* p, int w, const Win& o)
{
    return (p[0] * o.w00 + p[1] * o.w01 + p[w] * o.w10 + p[w + 1] * o.w11 + 256) >> 9;
}

using pm::wave_lds_sync;
using pm::wave_sum_i64;         // the sums below are long long throughout: exact

__device__ __forceinline__ float canon(float v) { return v != v ? __uint_as_float(0x7FC00000u) : v; }

// ---- S63 - S65: one point from pyramid a.pyr[dir] into a.pyr[dir ^ 1], by the 64 lanes of the calling wave.  Returns the
// status 1, 2 or 3; o0, o1: the last guess; err as S65.  Every value that steers a branch is the same on all lanes.
__device__ __forceinline__ int track_point(const LkArgs& a, int dir, float ptx, float pty, bool use_init, float inx, float iny, short* sT,
                                           short* sgx, short* sgy, int lane, float& o0, float& o1, float& err)
{
    const PyrDesc& A = a.pyr[dir];
    const PyrDesc& B = a.pyr[dir ^ 1];
    const int r = a.prm.win_radius, n = 2 * r + 1, m = n + 2, N = n * n;
    const unsigned inv_n = (65536u + n - 1) / n, inv_m = (65536u + m - 1) / m;      // e / n == (e * inv_n) >> 16 for e < 33 * 33
    const int top = min(a.prm.max_level, A.nlev - 1);
    const double eps2 = static_cast<double>(a.prm.eps) * static_cast<double>(a.prm.eps);
    float g0 = 0.f, g1 = 0.f;
    int status = 2;
    err = -1.0f;
    for (int l = top; l >= 0; --l) {
        const float s = 1.0f / static_cast<float>(1 << l);
        const float px = ptx * s, py = pty * s;
        if (l == top) {
            g0 = use_init ? inx * s : px;
            g1 = use_init ? iny * s : py;
        } else {
            g0 = 2.0f * g0;
            g1 = 2.0f * g1;
        }
        const int w = A.w[l], h = A.h[l];
        const uint8_t* Ia = A.base + A.off[l];
        const uint8_t* Ib = B.base + B.off[l];
        Win o;
        int code = 0;
        double Gxx = 0, Gxy = 0, Gyy = 0, D = 0;
        if (!window_origin(px - static_cast<float>(r + 1), py - static_cast<float>(r + 1), m, w, h, o)) {
            code = 1;
        } else {
            wave_lds_sync();                                       // the reads of the level above are over
            for (int e = lane; e < m * m; e += 64) {
                const int j = static_cast<int>((e * inv_m) >> 16), i = e - j * m;
                sT[e] = static_cast<short>(sample(Ia + static_cast<size_t>(o.iy + j) * w + (o.ix + i), w, o));
            }
            wave_lds_sync();
            long long sxx = 0, sxy = 0, syy = 0;
            for (int e = lane; e < N; e += 64) {
                const int j = static_cast<int>((e * inv_n) >> 16), i = e - j * n;
                const int c = (j + 1) * m + (i + 1);
                const int dx = sT[c + 1] - sT[c - 1], dy = sT[c + m] - sT[c - m];
                sgx[e] = static_cast<short>(dx);
                sgy[e] = static_cast<short>(dy);
                sxx += dx * dx;                                    // |dx| <= 8161: the product fits an int
                sxy += dx * dy;
                syy += dy * dy;
            }
            wave_lds_sync();
            Gxx = static_cast<double>(wave_sum_i64(sxx));
            Gxy = static_cast<double>(wave_sum_i64(sxy));
            Gyy = static_cast<double>(wave_sum_i64(syy));
            D = Gxx * Gyy - Gxy * Gxy;
            const double ev = ((Gxx + Gyy) - sqrt((Gxx - Gyy) * (Gxx - Gyy) + 4.0 * (Gxy * Gxy))) / (2.0 * N * 4096.0);
            if (!(ev >= static_cast<double>(a.prm.min_eig)) || !(D > 0)) code = 2;
        }
        if (code != 0) {
            if (l == 0) status = code == 1 ? 2 : 3;
            continue;
        }
        bool left = false;
        for (int it = 0; it < a.prm.max_iters; ++it) {
            if (!window_origin(g0 - static_cast<float>(r), g1 - static_cast<float>(r), n, w, h, o)) {
                left = true;
                break;
            }
            long long bx = 0, by = 0, sa = 0;
            for (int e = lane; e < N; e += 64) {
                const int j = static_cast<int>((e * inv_n) >> 16), i = e - j * n;
                const int d = sample(Ib + static_cast<size_t>(o.iy + j) * w + (o.ix + i), w, o) - sT[(j + 1) * m + (i + 1)];
                bx += d * sgx[e];
                by += d * sgy[e];
                sa += d < 0 ? -d : d;
            }
            const double dbx = static_cast<double>(wave_sum_i64(bx)), dby = static_cast<double>(wave_sum_i64(by));
            const long long tsa = wave_sum_i64(sa);
            if (l == 0) err = static_cast<float>(static_cast<double>(tsa) / (32.0 * N));
            const double dx = 2.0 * (Gxy * dby - Gyy * dbx) / D;
            const double dy = 2.0 * (Gxy * dbx - Gxx * dby) / D;
            g0 = g0 + static_cast<float>(dx);
            g1 = g1 + static_cast<float>(dy);
            if (dx * dx + dy * dy <= eps2) break;
        }
        if (l == 0) status = left ? 2 : 1;
    }
    o0 = canon(g0);
    o1 = canon(g1);
    return status;
}

__global__ __launch_bounds__(64 * WPB) void lk_track(const LkArgs a)
{
    __shared__ __attribute__((aligned(16))) short s_mem[WPB][WAVE_SHORTS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int pt = blockIdx.x * WPB + wave;
    if (pt >= pm::clamped_count(a.d_n, a.cap)) return;                // (no workgroup barrier anywhere below)
    short* sT = s_mem[wave];
    short* sgx = sT + T_MAX;
    short* sgy = sgx + G_MAX;
    const float ptx = a.pts[2 * static_cast<size_t>(pt)], pty = a.pts[2 * static_cast<size_t>(pt) + 1];
    const bool use_init = (a.prm.flags & PM_LK_USE_INITIAL) != 0;
    const float inx = use_init ? a.init[2 * static_cast<size_t>(pt)] : 0.f, iny = use_init ? a.init[2 * static_cast<size_t>(pt) + 1] : 0.f;
    float o0, o1, err, fb = -1.0f;
    int status = track_point(a, 0, ptx, pty, use_init, inx, iny, sT, sgx, sgy, lane, o0, o1, err);
    if (status == 1 && a.prm.fb_thresh > 0) {
        float b0, b1, berr;
        const int bs = track_point(a, 1, o0, o1, false, 0.f, 0.f, sT, sgx, sgy, lane, b0, b1, berr);
        const float ex = b0 - ptx, ey = b1 - pty;
        fb = canon(sqrtf(ex * ex + ey * ey));
        const bool keep = bs == 1 && static_cast<double>(ex) * static_cast<double>(ex) + static_cast<double>(ey) * static_cast<double>(ey) <=
                                         static_cast<double>(a.prm.fb_thresh) * static_cast<double>(a.prm.fb_thresh);
        status = keep ? 1 : 4;
    }
    if (lane == 0) {
        a.out[2 * static_cast<size_t>(pt)] = o0;
        a.out[2 * static_cast<size_t>(pt) + 1] = o1;
        a.status[pt] = static_cast<uint8_t>(status);
        if (a.err) a.err[pt] = err;
        if (a.fb) a.fb[pt] = fb;
    }
}

// ---- S66: the gather form.  One workgroup selects the tracked rows in order (pm::select_stable_1024) and moves them.
__global__ __launch_bounds__(1024) void lk_compact(const float* pts, const int32_t* d_n, int cap, const float* out, const uint8_t* status,
                                                   float* xy1, float* xy2, int32_t* src_idx, int32_t* count)
{
    pm::select_stable_1024(
        pm::clamped_count(d_n, cap), count, [&](int r) { return status[r] == 1; },
        [&](int r, int dst) {
            if (dst < 0) return;
            const size_t d = static_cast<size_t>(dst), s = static_cast<size_t>(r);
            xy1[2 * d] = pts[2 * s];
            xy1[2 * d + 1] = pts[2 * s + 1];
            xy2[2 * d] = out[2 * s];
            xy2[2 * d + 1] = out[2 * s + 1];
            if (src_idx) src_idx[d] = r;
        },
        [](int) {});
}

// ---- host side -----------------------------------------------------------------------------------------------------------

int plan_levels(int w, int h, int max_level, int* lw, int* lh, size_t* off, size_t* total)
{
    int n = 0;
    size_t o = 0;
    for (;;) {
        lw[n] = w;
        lh[n] = h;
        off[n] = o;
        o += pm::align_up(static_cast<size_t>(w) * h, 256);
        ++n;
        w = (w + 1) / 2;
        h = (h + 1) / 2;
        if (n > max_level || w < 16 || h < 16) break;
    }
    *total = o;
    return n;
}

PyrDesc describe(const pm_pyramid* p)
{
    PyrDesc d;
    memset(&d, 0, sizeof d);
    d.base = p->mem;
    d.nlev = p->nlev;
    for (int l = 0; l < p->nlev; ++l) {
        d.w[l] = p->lw[l];
        d.h[l] = p->lh[l];
        d.off[l] = p->off[l];
    }
    return d;
}

int check_params(const pm_lk_params* p)
{
    PM_REQUIRE(p != nullptr, PM_E_INVALID, "null parameters");
    PM_REQUIRE(p->win_radius >= 2 && p->win_radius <= MAX_R, PM_E_INVALID, "win_radius outside [2, 15]");
    PM_REQUIRE(p->max_level >= 0 && p->max_level <= 7, PM_E_INVALID, "max_level outside [0, 7]");
    PM_REQUIRE(p->max_iters >= 1 && p->max_iters <= 100, PM_E_INVALID, "max_iters outside [1, 100]");
    PM_REQUIRE(p->eps >= 0 && p->eps <= 3.0e38f, PM_E_INVALID, "eps must be finite and >= 0");
    PM_REQUIRE(p->min_eig >= 0 && p->min_eig <= 3.0e38f, PM_E_INVALID, "min_eig must be finite and >= 0");
    PM_REQUIRE(p->fb_thresh >= 0 && p->fb_thresh <= 3.0e38f, PM_E_INVALID, "fb_thresh must be 0 or finite and > 0");
    PM_REQUIRE((p->flags & ~PM_LK_USE_INITIAL) == 0 && p->reserved == 0, PM_E_INVALID, "unknown flag bits or reserved != 0");
    return PM_OK;
}

int check_track_args(pm_ctx* ctx, const pm_pyramid* prev, const pm_pyramid* next, const float* pts, int cap, const float* init,
                     const pm_lk_params* p)
{
    PM_REQUIRE(prev != nullptr && next != nullptr && pts != nullptr, PM_E_INVALID, "null pyramid or points");
    const int rc = check_params(p);
    if (rc != PM_OK) return rc;
    PM_REQUIRE(((p->flags & PM_LK_USE_INITIAL) != 0) == (init != nullptr), PM_E_INVALID,
               "initial points are required with PM_LK_USE_INITIAL and only then");
    PM_REQUIRE(prev->w == next->w && prev->h == next->h && prev->nlev == next->nlev, PM_E_INVALID, "pyramids of different shape");
    PM_REQUIRE(prev->device == ctx->device && next->device == ctx->device, PM_E_INVALID, "pyramid of another device");
    PM_REQUIRE(cap >= 0, PM_E_INVALID, "cap < 0");
    PM_REQUIRE(cap >= 1, PM_E_UNSUPPORTED, "cap == 0: nothing to track");
    return PM_OK;
}

void track_enqueue(pm_ctx* ctx, const pm_pyramid* prev, const pm_pyramid* next, const float* d_pts, const int32_t* d_n, int cap,
                   const float* d_init, const pm_lk_params* p, float* d_out, uint8_t* d_status, float* d_err, float* d_fb)
{
    LkArgs a;
    memset(&a, 0, sizeof a);
    a.pyr[0] = describe(prev);
    a.pyr[1] = describe(next);
    a.prm = *p;
    a.pts = d_pts;
    a.d_n = d_n;
    a.init = d_init;
    a.out = d_out;
    a.status = d_status;
    a.err = d_err;
    a.fb = d_fb;
    a.cap = cap;
    pm::ScopedKernelTime timer(ctx, "lk_track");
    hipLaunchKernelGGL(lk_track, dim3(static_cast<unsigned>((cap + WPB - 1) / WPB)), dim3(64 * WPB), 0, ctx->stream, a);
}

int build_enqueue(pm_ctx* ctx, pm_pyramid* pyr, const uint8_t* d_img, int stride)
{
    PM_HIP_CHECK(hipMemcpy2DAsync(pyr->mem, static_cast<size_t>(pyr->w), d_img, static_cast<size_t>(stride), static_cast<size_t>(pyr->w),
                                  static_cast<size_t>(pyr->h), hipMemcpyDeviceToDevice, ctx->stream));
    for (int l = 1; l < pyr->nlev; ++l) {
        const int ow = pyr->lw[l], oh = pyr->lh[l];
        pm::ScopedKernelTime timer(ctx, "lk_pyr_down");
        hipLaunchKernelGGL(lk_pyr_down, dim3((ow + PT_X - 1) / PT_X, (oh + PT_Y - 1) / PT_Y), dim3(256), 0, ctx->stream,
                           pyr->mem + pyr->off[l - 1], pyr->lw[l - 1], pyr->lh[l - 1], pyr->mem + pyr->off[l], ow, oh);
    }
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

}  // namespace

extern "C" int pm_pyramid_create(pm_ctx* ctx, int w, int h, int max_level, pm_pyramid** out)
{
    PM_REQUIRE(ctx != nullptr && out != nullptr, PM_E_INVALID, "null context or output pointer");
    *out = nullptr;
    PM_REFUSE_CAPTURE(ctx);
    PM_REQUIRE(max_level >= 0 && max_level <= 7, PM_E_INVALID, "max_level outside [0, 7]");
    PM_REQUIRE(w >= 1 && h >= 1, PM_E_INVALID, "need w, h >= 1");
    PM_REQUIRE(w >= 16 && h >= 16, PM_E_UNSUPPORTED, "images below 16 pixels a side are not tracked");
    PM_REQUIRE_PASS(pm_image::pixel_cap(w, h));
    pm_pyramid* p = new pm_pyramid;
    p->device = ctx->device;
    p->w = w;
    p->h = h;
    p->nlev = plan_levels(w, h, max_level, p->lw, p->lh, p->off, &p->bytes);
    if (hipSetDevice(ctx->device) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&p->mem), p->bytes) != hipSuccess) {
        pm::set_error("pm_pyramid_create: hipMalloc of %zu bytes failed", p->bytes);
        delete p;
        return PM_E_NOMEM;
    }
    *out = p;
    return PM_OK;
}

extern "C" int pm_pyramid_destroy(pm_pyramid* pyr)
{
    if (!pyr) return PM_OK;
    int rc = PM_OK;
    if (pyr->mem && (hipSetDevice(pyr->device) != hipSuccess || hipFree(pyr->mem) != hipSuccess)) rc = PM_E_HIP;
    delete pyr;
    return rc;
}

extern "C" int pm_pyramid_build_dev(pm_ctx* ctx, pm_pyramid* pyr, const uint8_t* d_img, int stride)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    PM_REQUIRE(pyr != nullptr && d_img != nullptr, PM_E_INVALID, "null pyramid or image");
    PM_REQUIRE(stride >= pyr->w, PM_E_INVALID, "stride < w");
    PM_REQUIRE(pyr->device == ctx->device, PM_E_INVALID, "pyramid of another device");
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    return build_enqueue(ctx, pyr, d_img, stride);
}

extern "C" int pm_pyramid_level_get(pm_ctx* ctx, const pm_pyramid* pyr, int level, uint8_t* plane, int cap, int* w_out, int* h_out)
{
    PM_REQUIRE(ctx != nullptr && pyr != nullptr, PM_E_INVALID, "null context or pyramid");
    if (w_out) *w_out = 0;
    if (h_out) *h_out = 0;
    if (level == -1) {                                  // the number of levels, through w_out
        if (w_out) *w_out = pyr->nlev;
        return PM_OK;
    }
    PM_REQUIRE(level >= 0 && level < pyr->nlev, PM_E_INVALID, "no such level");
    const int w = pyr->lw[level], h = pyr->lh[level];
    if (w_out) *w_out = w;
    if (h_out) *h_out = h;
    if (!plane) return PM_OK;
    const size_t n = static_cast<size_t>(w) * h;
    PM_REQUIRE(cap >= 0 && static_cast<size_t>(cap) >= n, PM_E_INVALID, "plane buffer too small");
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    PM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    PM_HIP_CHECK(hipMemcpy(plane, pyr->mem + pyr->off[level], n, hipMemcpyDeviceToHost));
    return PM_OK;
}

extern "C" int pm_track_lk_dev(pm_ctx* ctx, const pm_pyramid* prev, const pm_pyramid* next, const float* d_pts, const int32_t* d_n, int cap,
                               const float* d_init, const pm_lk_params* p, float* d_out, uint8_t* d_status, float* d_err, float* d_fb)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    PM_REQUIRE(d_out != nullptr && d_status != nullptr, PM_E_INVALID, "null output pointer");
    const int rc = check_track_args(ctx, prev, next, d_pts, cap, d_init, p);
    if (rc != PM_OK) return rc;
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    track_enqueue(ctx, prev, next, d_pts, d_n, cap, d_init, p, d_out, d_status, d_err, d_fb);
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_track_lk_gather_dev(pm_ctx* ctx, const pm_pyramid* prev, const pm_pyramid* next, const float* d_pts, const int32_t* d_n,
                                      int cap, const float* d_init, const pm_lk_params* p, float* d_xy1, float* d_xy2,
                                      int32_t* d_src_idx, int32_t* d_count, float* d_out, uint8_t* d_status)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    PM_REQUIRE(d_xy1 != nullptr && d_xy2 != nullptr && d_count != nullptr, PM_E_INVALID, "null output pointer");
    int rc = check_track_args(ctx, prev, next, d_pts, cap, d_init, p);
    if (rc != PM_OK) return rc;
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    if (!d_out || !d_status) {                          // the rows the caller does not want live in the context's scratch arena
        const size_t ob = pm::align_up(static_cast<size_t>(cap) * 8, 256), sb = pm::align_up(static_cast<size_t>(cap), 256);
        rc = pm::arena_reserve(ctx, ob + sb + 512);
        if (rc != PM_OK) return rc;
        pm::arena_reset(ctx);
        float* t_out = static_cast<float*>(pm::arena_take(ctx, ob));
        uint8_t* t_status = static_cast<uint8_t*>(pm::arena_take(ctx, sb));
        PM_REQUIRE(t_out != nullptr && t_status != nullptr, PM_E_NOMEM, "scratch arena too small");
        if (!d_out) d_out = t_out;
        if (!d_status) d_status = t_status;
    }
    track_enqueue(ctx, prev, next, d_pts, d_n, cap, d_init, p, d_out, d_status, nullptr, nullptr);
    {
        pm::ScopedKernelTime timer(ctx, "lk_compact");
        hipLaunchKernelGGL(lk_compact, dim3(1), dim3(1024), 0, ctx->stream, d_pts, d_n, cap, d_out, d_status, d_xy1, d_xy2, d_src_idx,
                           d_count);
    }
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_track_lk(pm_ctx* ctx, const uint8_t* img1, const uint8_t* img2, int w, int h, int stride, const float* pts, int n,
                           const float* init, const pm_lk_params* p, float* out, uint8_t* status, float* err, float* fb)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    PM_REQUIRE(img1 != nullptr && img2 != nullptr && pts != nullptr && out != nullptr && status != nullptr, PM_E_INVALID, "null pointer");
    PM_REQUIRE(w >= 1 && h >= 1 && stride >= w && n >= 0, PM_E_INVALID, "need w, h >= 1, stride >= w, n >= 0");
    int rc = check_params(p);
    if (rc != PM_OK) return rc;
    PM_REQUIRE(((p->flags & PM_LK_USE_INITIAL) != 0) == (init != nullptr), PM_E_INVALID,
               "initial points are required with PM_LK_USE_INITIAL and only then");
    PM_REQUIRE(n >= 1, PM_E_UNSUPPORTED, "n == 0: nothing to track");
    pm_pyramid *pa = nullptr, *pb = nullptr;
    rc = pm_pyramid_create(ctx, w, h, p->max_level, &pa);
    if (rc == PM_OK) rc = pm_pyramid_create(ctx, w, h, p->max_level, &pb);
    if (rc == PM_OK) {                                   // the block is freed before the pyramids are destroyed
        const size_t img_b = static_cast<size_t>(h) * stride, xy_b = static_cast<size_t>(n) * 8, f_b = static_cast<size_t>(n) * 4;
        pm::StagedBlock b(ctx, __func__);
        const size_t o_1 = b.add(img_b), o_2 = b.add(img_b), o_pts = b.add(xy_b), o_init = b.add(xy_b), o_out = b.add(xy_b);
        const size_t o_err = b.add(f_b), o_fb = b.add(f_b), o_st = b.add(static_cast<size_t>(n));
        b.alloc();
        b.upload(o_1, img1, img_b);
        b.upload(o_2, img2, img_b);
        b.upload(o_pts, pts, xy_b);
        if (init) b.upload(o_init, init, xy_b);
        if (b.rc == PM_OK) b.rc = build_enqueue(ctx, pa, b.at<uint8_t>(o_1), stride);
        if (b.rc == PM_OK) b.rc = build_enqueue(ctx, pb, b.at<uint8_t>(o_2), stride);
        if (b.rc == PM_OK)
            b.rc = pm_track_lk_dev(ctx, pa, pb, b.at<float>(o_pts), nullptr, n, init ? b.at<float>(o_init) : nullptr, p, b.at<float>(o_out),
                                   b.at<uint8_t>(o_st), b.at<float>(o_err), b.at<float>(o_fb));
        b.download(out, o_out, xy_b);
        b.download(status, o_st, static_cast<size_t>(n));
        if (err) b.download(err, o_err, f_b);
        if (fb) b.download(fb, o_fb, f_b);
        rc = b.sync();
    }
    (void)pm_pyramid_destroy(pa);
    (void)pm_pyramid_destroy(pb);
    return rc;
}
