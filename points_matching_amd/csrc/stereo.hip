// stereo.hip — dense stereo on a rectified pair: pm_stereo_rectify, pm_stereo_bm[_dev], pm_stereo_lr_check_dev,
// pm_stereo_points[_dev] (docs/SPEC.md S84-S88).  Every quantity of S85 and S86 is an integer, so the order of the sums is free
// and the outputs are a function of the inputs alone; S87 is a sequence of single fp64 operations.
//
// stereo_bm: a LANE OWNS A DISPARITY.  A 256-thread workgroup owns a 64 x 4 output tile, each of its four waves one row
// segment.  The base tile (64 + 2r columns, 4 + 2r rows) and the other image's tile, widened by D - 1 columns, are staged in
// LDS once.  A wave walks its segment left to right; per column it forms the column sums V(col, d) over the 2r + 1 window rows:
// the base pixel is one LDS address for the whole wave (a broadcast), the other image's pixels of the 64 lanes are 64
// consecutive bytes (16 banks, four lanes per dword, no conflict), and v_sad_u8 adds |a - b| to the running sum in one
// instruction.  The window slides: C(x) = C(x - 1) + V(x + r) - V(x - r - 1), with the last 2r + 1 column sums in a
// per-lane ring in LDS (u16: V <= 21 * 255).  D > 64 gives a lane up to four disparities (template NC), so the cost curve of
// a pixel lies across the lanes: the winner is stereo_core::winner (stereo_core.hpp, shared with stereo_sgm.hip): one DPP wave
// minimum of the key (cost << 9) | (d - dmin), which is the lowest-d tie rule; c2 a second minimum; p and n two lane reads.  A
// lane keeps the result of "its" column and the segment goes out as one 128-byte store.  One integer atomic per workgroup for
// n_valid.  The range and size rules of the arguments are image_args.hpp's, the host form is StagedBlock::stereo (pm_common.hpp).
//
// stereo_lr_check (S86): a 64 x 32 tile per workgroup, eight rows per thread.  stereo_points (S87): one thread per point.
#include <cmath>
#include <cstdint>

#include "pm_common.hpp"
#include "stereo_core.hpp"
#include "stereo_rectify_core.hpp"
#include "wave_ops.hpp"

namespace {

using pm_image::overlap;
using pm_image::span;
using stereo_core::INVALID;

constexpr int TILE_W = 64, TILE_H = 4;                    // output tile of a workgroup: one 64-pixel row segment per wave

struct BmArgs {
    const uint8_t* base;                                  // the image whose pixels get a disparity (right with FROM_RIGHT)
    const uint8_t* other;
    int w, h, bstride, ostride;
    int dmin, D, r, uniq;
    int sgn;                                              // the other image's column of (x, d) is x + sgn * d
    int cx0, cx1;                                         // computed columns, inclusive (cx1 < cx0: none)
    int nbx;                                              // tiles per row of tiles
    int bw, ow;                                           // LDS row pitches of the two tiles (multiples of 4)
    int16_t* disp;
    int dstride;
    pm_stereo_info* info;
};

// rows x pitch bytes of img, from (row0, col0), into LDS; 0 outside the image (never read by a computed pixel)
__device__ __forceinline__ void stage(uint8_t* dst, const uint8_t* img, int w, int h, int stride, int row0, int col0, int rows, int pitch, int tid)
{
    const int words = pitch >> 2;
    for (int e = tid; e < rows * words; e += 256) {
        const int ry = e / words, rx = (e - ry * words) << 2;
        const int y = row0 + ry;
        unsigned word = 0;
        if (y >= 0 && y < h) {
            const uint8_t* row = img + static_cast<size_t>(y) * stride;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int x = col0 + rx + b;
                if (x >= 0 && x < w) word |= static_cast<unsigned>(row[x]) << (8 * b);
            }
        }
        *reinterpret_cast<unsigned*>(dst + ry * pitch + rx) = word;
    }
}

template <int NC>
__global__ __launch_bounds__(256) void stereo_bm(BmArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t s_mem[];
    __shared__ int s_cnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int by = blockIdx.x / a.nbx, bx = blockIdx.x - by * a.nbx;
    const int x0 = bx * TILE_W, y0 = by * TILE_H;
    const int r = a.r, D = a.D, win = 2 * r + 1, rows = TILE_H + 2 * r;
    uint8_t* s_base = s_mem;
    uint8_t* s_other = s_base + rows * a.bw;
    uint16_t* s_ring = reinterpret_cast<uint16_t*>(s_other + rows * a.ow) + wave * (win * 64 * NC);

    const int xs = max(x0, a.cx0), xe = min(x0 + TILE_W - 1, a.cx1);                  // the computed columns of this tile
    const int y = y0 + wave;
    const bool row_computed = y >= r && y <= a.h - 1 - r && xs <= xe;                // wave-uniform
    if (xs <= xe) {                                                                  // workgroup-uniform
        const int dmax = a.dmin + D - 1;
        stage(s_base, a.base, a.w, a.h, a.bstride, y0 - r, x0 - r, rows, a.bw, tid);
        stage(s_other, a.other, a.w, a.h, a.ostride, y0 - r, x0 - r + (a.sgn < 0 ? -dmax : a.dmin), rows, a.ow, tid);
    }
    __syncthreads();

    int mine = INVALID;                                                              // the result of column x0 + lane
    if (row_computed) {
        int off[NC];                                                                 // column offset of this lane's disparities in s_other
        bool live[NC];
        unsigned C[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int k = lane + 64 * c;
            live[c] = k < D;
            const int kc = min(k, D - 1);
            off[c] = a.sgn < 0 ? D - 1 - kc : kc;
            C[c] = 0;
        }
        for (int e = 0; e < win; ++e)
#pragma unroll
            for (int c = 0; c < NC; ++c) s_ring[(e * NC + c) * 64 + lane] = 0;
        int pos = 0;
        for (int col = xs - r; col <= xe + r; ++col) {
            const int rel = col - (x0 - r);
            unsigned V[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) V[c] = 0;
            for (int j = 0; j < win; ++j) {
                const unsigned b = s_base[(wave + j) * a.bw + rel];                  // one address per wave: a broadcast
                const uint8_t* o = s_other + (wave + j) * a.ow + rel;
#pragma unroll
                for (int c = 0; c < NC; ++c) V[c] = __builtin_amdgcn_sad_u8(b, o[off[c]], V[c]);
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                uint16_t* slot = s_ring + (pos * NC + c) * 64 + lane;
                C[c] += V[c] - *slot;
                *slot = static_cast<uint16_t>(V[c]);
            }
            pos = pos + 1 == win ? 0 : pos + 1;
            const int x = col - r;
            if (x < xs) continue;                                                    // the window is not whole yet

            const int won = stereo_core::winner<pm::wave_min_u32>(C, live, lane, D, a.dmin, a.uniq).value;          // wave-uniform
            if (lane == x - x0) mine = won;
        }
    }
    const int x = x0 + lane;
    const bool inside = y < a.h && x < a.w;
    if (inside) a.disp[static_cast<size_t>(y) * a.dstride + x] = static_cast<int16_t>(mine);
    if (a.info) {                                                                    // (kernel argument: the same for every thread)
        const int total = __popcll(__ballot(inside && mine != INVALID));
        if (lane == 0) s_cnt[wave] = total;
        __syncthreads();
        if (tid == 0) {
            const int sum = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
            if (sum) atomicAdd(&a.info->n_valid, sum);
        }
    }
}

// S86, in place on the left map: a 64 x 32 tile per workgroup (a thread takes 8 rows), so that the one atomic per workgroup on
// n_valid stays rare: with a 64 x 4 tile the 8100 atomics of a 1920 x 1080 map took longer than the pixels
constexpr int LR_TILE_H = 32;

__global__ __launch_bounds__(256) void stereo_lr_check(int16_t* left, const int16_t* __restrict__ right, int w, int h, int lstride, int rstride,
                                                       int max_diff, int nbx, pm_stereo_info* info)
{
    __shared__ int s_cnt[4];
    const int tid = threadIdx.x;
    const int by = blockIdx.x / nbx, bx = blockIdx.x - by * nbx;
    const int x = bx * 64 + (tid & 63);
    int total = 0;
    for (int k = 0; k < LR_TILE_H / 4; ++k) {
        const int y = by * LR_TILE_H + 4 * k + (tid >> 6);
        bool valid = false;
        if (x < w && y < h) {
            int16_t* p = left + static_cast<size_t>(y) * lstride + x;
            const int v = *p;
            if (v != INVALID) {
                const int xr = x - ((v + 8) >> 4);
                if (xr >= 0 && xr < w) {
                    const int vr = right[static_cast<size_t>(y) * rstride + xr];
                    valid = vr != INVALID && abs(v - vr) <= max_diff;
                }
                if (!valid) *p = static_cast<int16_t>(INVALID);
            }
        }
        total += __popcll(__ballot(valid));
    }
    if (info) {
        if ((tid & 63) == 0) s_cnt[tid >> 6] = total;
        __syncthreads();
        if (tid == 0) {
            const int sum = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
            if (sum) atomicAdd(&info->n_valid, sum);
        }
    }
}

struct PointArgs {
    double fx, fy, cx, cy;
    double fb16;                                          // (fx * baseline) * 16
    double R[9];
    int has_R;
};

// S87
__global__ __launch_bounds__(256) void stereo_points(PointArgs a, const int16_t* __restrict__ disp, int w, int h, int dstride, const float* pts,
                                                     const int32_t* d_n, int cap, float* xyz)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= pm::clamped_count(d_n, cap)) return;
    const double x = static_cast<double>(pts[2 * static_cast<size_t>(i)]), y = static_cast<double>(pts[2 * static_cast<size_t>(i) + 1]);
    const float nan = __uint_as_float(0x7FC00000u);
    float o0 = nan, o1 = nan, o2 = nan;
    const double xi = floor(x + 0.5), yi = floor(y + 0.5);
    if (isfinite(x) && isfinite(y) && xi >= 0.0 && xi < static_cast<double>(w) && yi >= 0.0 && yi < static_cast<double>(h)) {
        const int v = disp[static_cast<size_t>(static_cast<int>(yi)) * dstride + static_cast<int>(xi)];
        if (v != INVALID && v > 0) {
            const double Z = a.fb16 / static_cast<double>(v);
            const double X = ((x - a.cx) / a.fx) * Z;
            const double Y = ((y - a.cy) / a.fy) * Z;
            if (a.has_R) {
                o0 = static_cast<float>((a.R[0] * X + a.R[3] * Y) + a.R[6] * Z);
                o1 = static_cast<float>((a.R[1] * X + a.R[4] * Y) + a.R[7] * Z);
                o2 = static_cast<float>((a.R[2] * X + a.R[5] * Y) + a.R[8] * Z);
            } else {
                o0 = static_cast<float>(X);
                o1 = static_cast<float>(Y);
                o2 = static_cast<float>(Z);
            }
        }
    }
    xyz[3 * static_cast<size_t>(i)] = o0;
    xyz[3 * static_cast<size_t>(i) + 1] = o1;
    xyz[3 * static_cast<size_t>(i) + 2] = o2;
}

// ---- host side -----------------------------------------------------------------------------------------------------------

int check_bm(const void* left, const void* right, int w, int h, int lstride, int rstride, const pm_stereo_params* p, const void* disp, int dstride)
{
    PM_REQUIRE(left != nullptr && right != nullptr && p != nullptr && disp != nullptr, PM_E_INVALID, "null pointer");
    PM_REQUIRE((p->flags & ~PM_STEREO_FROM_RIGHT) == 0, PM_E_INVALID, "unknown flag bits");
    PM_REQUIRE(p->reserved[0] == 0 && p->reserved[1] == 0 && p->reserved[2] == 0, PM_E_INVALID, "reserved != 0");
    PM_REQUIRE(p->radius >= 1 && p->radius <= 10, PM_E_INVALID, "radius outside [1, 10]");
    PM_REQUIRE(p->num_disp >= 1 && p->num_disp <= 256, PM_E_INVALID, "num_disp outside [1, 256]");
    PM_REQUIRE(p->min_disp >= -1024 && p->min_disp + p->num_disp - 1 <= 1024, PM_E_INVALID, "disparities outside [-1024, 1024]");
    PM_REQUIRE(p->uniqueness >= 0 && p->uniqueness <= 99, PM_E_INVALID, "uniqueness outside [0, 99]");
    PM_REQUIRE(w >= 1 && h >= 1, PM_E_INVALID, "need sizes >= 1");
    PM_REQUIRE(lstride >= w && rstride >= w && dstride >= w, PM_E_INVALID, "a stride below the width");
    PM_REQUIRE_PASS(pm_image::pixel_cap(w, h));
    return PM_OK;
}

int check_lr(const void* left, const void* right, int w, int h, int lstride, int rstride, int max_diff16)
{
    PM_REQUIRE(left != nullptr && right != nullptr, PM_E_INVALID, "null pointer");
    PM_REQUIRE(max_diff16 >= 0, PM_E_INVALID, "max_diff16 < 0");
    PM_REQUIRE(w >= 1 && h >= 1, PM_E_INVALID, "need sizes >= 1");
    PM_REQUIRE(lstride >= w && rstride >= w, PM_E_INVALID, "a stride below the width");
    PM_REQUIRE_PASS(pm_image::pixel_cap(w, h));
    return PM_OK;
}

int make_points(const void* disp, int w, int h, int dstride, const pm_camera* K, double baseline, const double* R, const void* pts, const void* xyz,
                int n, PointArgs* a)
{
    PM_REQUIRE(disp != nullptr && K != nullptr && pts != nullptr && xyz != nullptr, PM_E_INVALID, "null pointer");
    PM_REQUIRE(std::isfinite(K->fx) && std::isfinite(K->fy) && std::isfinite(K->cx) && std::isfinite(K->cy) && K->fx > 0.0 && K->fy > 0.0,
               PM_E_INVALID, "K_rect needs finite values and fx, fy > 0");
    PM_REQUIRE(std::isfinite(baseline) && baseline > 0.0, PM_E_INVALID, "baseline must be finite and > 0");
    PM_REQUIRE(w >= 1 && h >= 1, PM_E_INVALID, "need sizes >= 1");
    PM_REQUIRE(dstride >= w, PM_E_INVALID, "a stride below the width");
    PM_REQUIRE(n >= 0, PM_E_INVALID, "cap or n < 0");
    a->fx = K->fx; a->fy = K->fy; a->cx = K->cx; a->cy = K->cy;
    a->fb16 = (K->fx * baseline) * 16.0;
    a->has_R = R ? 1 : 0;
    for (int i = 0; i < 9; ++i) {
        PM_REQUIRE(!R || std::isfinite(R[i]), PM_E_INVALID, "an entry of R is not finite");
        a->R[i] = R ? R[i] : (i % 4 == 0 ? 1.0 : 0.0);
    }
    PM_REQUIRE_PASS(pm_image::pixel_cap(w, h));
    PM_REQUIRE(n >= 1, PM_E_UNSUPPORTED, "cap == 0 or n == 0: no points");
    const size_t x_b = static_cast<size_t>(n) * 12;
    PM_REQUIRE(!overlap(xyz, x_b, disp, span(w, h, dstride, 2)) && !overlap(xyz, x_b, pts, static_cast<size_t>(n) * 8), PM_E_INVALID,
               "the output rows overlap the map or the points");
    return PM_OK;
}

unsigned tiles(int w, int h) { return static_cast<unsigned>((w + 63) / 64) * static_cast<unsigned>((h + 3) / 4); }

}  // namespace

extern "C" int pm_stereo_rectify(const double R[9], const double t[3], double R1[9], double R2[9], double* baseline, int* left_is_view2)
{
    PM_REQUIRE(R != nullptr && t != nullptr && R1 != nullptr && R2 != nullptr && baseline != nullptr && left_is_view2 != nullptr, PM_E_INVALID,
               "null pointer");
    PM_REQUIRE(pm_stereo::finite12(R, t), PM_E_INVALID, "R or t is not finite");
    const int rc = pm_stereo::rectify(R, t, R1, R2, baseline, left_is_view2);
    PM_REQUIRE(rc != PM_E_NO_MODEL, PM_E_NO_MODEL, "no baseline, or an optical axis along it");
    PM_REQUIRE(rc != PM_E_UNSUPPORTED, PM_E_UNSUPPORTED, "a vertical rig (|c_y| > |c_x|)");
    return rc;
}

extern "C" int pm_stereo_bm_dev(pm_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right, int w, int h, int lstride, int rstride,
                                const pm_stereo_params* p, int16_t* d_disp, int dstride, pm_stereo_info* d_info)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    const int rc = check_bm(d_left, d_right, w, h, lstride, rstride, p, d_disp, dstride);
    if (rc != PM_OK) return rc;
    PM_REQUIRE_PASS(pm_image::disparity_map_ranges(d_left, d_right, w, h, lstride, rstride, d_disp, dstride, d_info));
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    if (d_info) PM_HIP_CHECK(hipMemsetAsync(d_info, 0, sizeof(pm_stereo_info), ctx->stream));
    const bool from_right = (p->flags & PM_STEREO_FROM_RIGHT) != 0;
    const int r = p->radius, D = p->num_disp, dmin = p->min_disp;
    const pm_image::Columns cols = pm_image::computed_columns(from_right, r, dmin, dmin + D - 1, w);
    BmArgs a;
    a.base = from_right ? d_right : d_left;
    a.other = from_right ? d_left : d_right;
    a.bstride = from_right ? rstride : lstride;
    a.ostride = from_right ? lstride : rstride;
    a.w = w; a.h = h;
    a.dmin = dmin; a.D = D; a.r = r; a.uniq = p->uniqueness;
    a.sgn = from_right ? 1 : -1;
    a.cx0 = cols.x0; a.cx1 = cols.x1;
    a.nbx = (w + TILE_W - 1) / TILE_W;
    a.bw = (TILE_W + 2 * r + 3) & ~3;
    a.ow = (TILE_W + 2 * r + D - 1 + 3) & ~3;
    a.disp = d_disp; a.dstride = dstride; a.info = d_info;
    const int nc = (D + 63) / 64, rows = TILE_H + 2 * r;
    const size_t lds = static_cast<size_t>(rows) * (a.bw + a.ow) + static_cast<size_t>(4) * (2 * r + 1) * 64 * nc * sizeof(uint16_t);
    {
        pm::ScopedKernelTime timer(ctx, "stereo_bm");
        const dim3 grid(tiles(w, h)), block(256);
        switch (nc) {
        case 1: hipLaunchKernelGGL(stereo_bm<1>, grid, block, lds, ctx->stream, a); break;
        case 2: hipLaunchKernelGGL(stereo_bm<2>, grid, block, lds, ctx->stream, a); break;
        case 3: hipLaunchKernelGGL(stereo_bm<3>, grid, block, lds, ctx->stream, a); break;
        default: hipLaunchKernelGGL(stereo_bm<4>, grid, block, lds, ctx->stream, a); break;
        }
    }
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_stereo_lr_check_dev(pm_ctx* ctx, int16_t* d_left, const int16_t* d_right, int w, int h, int lstride, int rstride,
                                      int max_diff16, pm_stereo_info* d_info)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    const int rc = check_lr(d_left, d_right, w, h, lstride, rstride, max_diff16);
    if (rc != PM_OK) return rc;
    PM_REQUIRE(!overlap(d_left, span(w, h, lstride, 2), d_right, span(w, h, rstride, 2)), PM_E_INVALID, "the two maps overlap");
    PM_REQUIRE(!d_info || (!overlap(d_info, sizeof(pm_stereo_info), d_left, span(w, h, lstride, 2)) &&
                           !overlap(d_info, sizeof(pm_stereo_info), d_right, span(w, h, rstride, 2))),
               PM_E_INVALID, "the info record overlaps a map");
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    if (d_info) PM_HIP_CHECK(hipMemsetAsync(d_info, 0, sizeof(pm_stereo_info), ctx->stream));
    {
        pm::ScopedKernelTime timer(ctx, "stereo_lr_check");
        const unsigned grid = static_cast<unsigned>((w + 63) / 64) * static_cast<unsigned>((h + LR_TILE_H - 1) / LR_TILE_H);
        hipLaunchKernelGGL(stereo_lr_check, dim3(grid), dim3(256), 0, ctx->stream, d_left, d_right, w, h, lstride, rstride, max_diff16,
                           (w + 63) / 64, d_info);
    }
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_stereo_bm(pm_ctx* ctx, const uint8_t* left, const uint8_t* right, int w, int h, int lstride, int rstride,
                            const pm_stereo_params* p, int lr_max_diff16, int16_t* disp, int dstride, pm_stereo_info* info)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    const int rc = check_bm(left, right, w, h, lstride, rstride, p, disp, dstride);
    if (rc != PM_OK) return rc;
    const bool lr = lr_max_diff16 >= 0;
    PM_REQUIRE(!lr || (p->flags & PM_STEREO_FROM_RIGHT) == 0, PM_E_INVALID, "the left-right check needs the left map: no PM_STEREO_FROM_RIGHT");
    PM_REQUIRE_PASS(pm_image::disparity_map_ranges(left, right, w, h, lstride, rstride, disp, dstride, info));
    pm_stereo_params q = *p;
    q.flags |= PM_STEREO_FROM_RIGHT;
    return pm::StagedBlock::stereo(
        ctx, __func__, left, right, w, h, lstride, rstride, lr_max_diff16, disp, dstride, info,
        [&](const uint8_t* l, const uint8_t* r, int16_t* d, pm_stereo_info* i) { return pm_stereo_bm_dev(ctx, l, r, w, h, lstride, rstride, p, d, dstride, i); },
        [&](const uint8_t* l, const uint8_t* r, int16_t* d) { return pm_stereo_bm_dev(ctx, l, r, w, h, lstride, rstride, &q, d, w, nullptr); });
}

extern "C" int pm_stereo_points_dev(pm_ctx* ctx, const int16_t* d_disp, int w, int h, int dstride, const pm_camera* K_rect, double baseline,
                                    const double* R, const float* d_pts, const int32_t* d_n, int cap, float* d_xyz)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    PointArgs a;
    const int rc = make_points(d_disp, w, h, dstride, K_rect, baseline, R, d_pts, d_xyz, cap, &a);
    if (rc != PM_OK) return rc;
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    {
        pm::ScopedKernelTime timer(ctx, "stereo_points");
        hipLaunchKernelGGL(stereo_points, dim3((static_cast<unsigned>(cap) + 255u) / 256u), dim3(256), 0, ctx->stream, a, d_disp, w, h, dstride, d_pts,
                           d_n, cap, d_xyz);
    }
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_stereo_points(pm_ctx* ctx, const int16_t* disp, int w, int h, int dstride, const pm_camera* K_rect, double baseline,
                                const double* R, const float* pts, int n, float* xyz)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    PointArgs a;
    const int rc = make_points(disp, w, h, dstride, K_rect, baseline, R, pts, xyz, n, &a);
    if (rc != PM_OK) return rc;
    const size_t d_b = span(w, h, dstride, 2), p_b = static_cast<size_t>(n) * 8, x_b = static_cast<size_t>(n) * 12;
    pm::StagedBlock b(ctx, __func__);
    const size_t o_d = b.add(d_b), o_p = b.add(p_b), o_x = b.add(x_b);
    b.alloc();
    b.upload(o_d, disp, d_b);
    b.upload(o_p, pts, p_b);
    if (b.rc == PM_OK)
        b.rc = pm_stereo_points_dev(ctx, b.at<int16_t>(o_d), w, h, dstride, K_rect, baseline, R, b.at<float>(o_p), nullptr, n, b.at<float>(o_x));
    b.download(xyz, o_x, x_b);
    return b.sync();
}
