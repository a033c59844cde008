// corners.hip — minimum-eigenvalue (Shi-Tomasi) corners on level 0 of a pm_pyramid (docs/SPEC.md S67-S70): the point source of
// the tracking route.  The counterpart of cv::goodFeaturesToTrack(..., mask): the strongest corners that keep a minimum
// distance from each other and from an existing point set, so that a video loop can top its surviving tracks up.
//
// The score is the tracker's own quantity.  The block sums are exact int32 sums of integer central differences, and the
// eigenvalue is the fp64 expression of S63 on them, so at an integer pixel the score is bit for bit the value lk_track tests
// against min_eig at level 0 for win_radius == block_radius.
//
// Launches, all on the context's stream:
//   corner_extrema  a workgroup per 64 x 16 tile: pixels + halo to LDS, int16 gradient planes, separable block sums, the
//                   eigenvalue on the tile and a one-pixel rim, the 3 x 3 rule of S68; survivors appended through one
//                   atomic counter that keeps counting past the capacity
//   corner_rank     rank by counting smaller 64-bit keys (S69); every candidate is written to its rank
//   corner_select   one workgroup: quality cut, greedy minimum-distance walk (S70) in chunks of one candidate per thread,
//                   the counts, the overflow rule and the replenish offsets, all from device-side counts
#include <algorithm>

#include "pm_common.hpp"
#include "pyramid.hpp"
#include "wave_ops.hpp"

namespace {

constexpr int MAX_R = 15;
constexpr int CT_X = 64, CT_Y = 16;                            // output tile
constexpr int CE_X = CT_X + 2, CE_Y = CT_Y + 2;                // eigenvalues: the tile and its one-pixel rim
constexpr int CG_X = CE_X + 2 * MAX_R, CG_Y = CE_Y + 2 * MAX_R;   // gradients under every block of the rim: 96 x 48 at r = 15
constexpr int CP_X = CG_X + 2, CP_Y = CG_Y + 2;                // pixels under the gradients: 98 x 50
constexpr int LDS_GRAD = 2 * CG_X * CG_Y * 2;                  // two int16 planes, 18432 bytes; the eigenvalues reuse them
constexpr int LDS_ROW = 3 * CG_Y * CE_X * 4;                   // three int32 planes of row sums, 38016 bytes
constexpr int LDS_PIX = (CP_X * CP_Y + 15) & ~15;              // 4912 bytes
constexpr int LDS_TOTAL = LDS_GRAD + LDS_ROW + LDS_PIX;        // 61360 bytes
static_assert(CE_X * CE_Y * 8 <= LDS_GRAD, "the eigenvalue plane must fit the gradient planes it replaces");
static_assert(LDS_TOTAL <= 65536, "corner_extrema: static LDS above 64 KiB");

// ---- S67 + S68: one tile.  Output pixel (0, 0) of the tile is (r + 1 + 64 bx, r + 1 + 16 by), the first pixel of V.
__global__ __launch_bounds__(256) void corner_extrema(const uint8_t* img, int w, int h, int r, float min_eig, unsigned* counter, unsigned cap,
                                                      unsigned long long* keys)
{
    __shared__ __attribute__((aligned(16))) unsigned char s_raw[LDS_TOTAL];
    short* s_cx = reinterpret_cast<short*>(s_raw);
    short* s_cy = s_cx + CG_X * CG_Y;
    double* s_e = reinterpret_cast<double*>(s_raw);            // (written after the last read of the gradients)
    int* s_row = reinterpret_cast<int*>(s_raw + LDS_GRAD);
    unsigned char* s_px = s_raw + LDS_GRAD + LDS_ROW;
    constexpr int ROW_PLANE = CG_Y * CE_X;
    const int tid = threadIdx.x;
    const int n = 2 * r + 1;
    const int gw = CE_X + 2 * r, gh = CE_Y + 2 * r, pw = gw + 2, ph = gh + 2;
    const int x0 = r + 1 + blockIdx.x * CT_X, y0 = r + 1 + blockIdx.y * CT_Y;
    const int px0 = x0 - r - 2, py0 = y0 - r - 2;              // >= -1
    // pixels; coordinates outside the image are clamped into it: they feed only positions outside V
    for (int e = tid; e < pw * ph; e += 256) {
        const int jy = e / pw, jx = e - jy * pw;
        const int xs = min(max(px0 + jx, 0), w - 1), ys = min(max(py0 + jy, 0), h - 1);
        s_px[e] = img[static_cast<size_t>(ys) * w + xs];
    }
    __syncthreads();
    for (int e = tid; e < gw * gh; e += 256) {
        const int j = e / gw, i = e - j * gw;
        const unsigned char* p = s_px + (j + 1) * pw + (i + 1);
        s_cx[e] = static_cast<short>(static_cast<int>(p[1]) - static_cast<int>(p[-1]));
        s_cy[e] = static_cast<short>(static_cast<int>(p[pw]) - static_cast<int>(p[-pw]));
    }
    __syncthreads();
    // row pass: sums of 2r + 1 products along x, for each of the gh gradient rows and the 66 columns of the rim
    for (int e = tid; e < gh * CE_X; e += 256) {
        const int j = e / CE_X, i = e - j * CE_X;
        const short* cx = s_cx + j * gw + i;
        const short* cy = s_cy + j * gw + i;
        int a = 0, b = 0, c = 0;
        for (int k = 0; k < n; ++k) {
            const int dx = cx[k], dy = cy[k];
            a += dx * dx;
            b += dx * dy;
            c += dy * dy;
        }
        s_row[e] = a;
        s_row[ROW_PLANE + e] = b;
        s_row[2 * ROW_PLANE + e] = c;
    }
    __syncthreads();
    // column pass and the eigenvalue; positions outside V hold -infinity, which every comparison of S68 ignores
    const double inv = 8.0 * static_cast<double>(n * n);
    for (int e = tid; e < CE_X * CE_Y; e += 256) {
        const int j = e / CE_X, i = e - j * CE_X;
        const int x = x0 - 1 + i, y = y0 - 1 + j;
        double ev = -__builtin_huge_val();
        if (x >= r + 1 && x <= w - r - 3 && y >= r + 1 && y <= h - r - 3) {
            const int* p = s_row + j * CE_X + i;
            int a = 0, b = 0, c = 0;
            for (int k = 0; k < n; ++k) {
                a += p[k * CE_X];
                b += p[ROW_PLANE + k * CE_X];
                c += p[2 * ROW_PLANE + k * CE_X];
            }
            const double A = static_cast<double>(a), B = static_cast<double>(b), C = static_cast<double>(c);
            ev = ((A + C) - sqrt((A - C) * (A - C) + 4.0 * (B * B))) / inv;
        }
        s_e[e] = ev;
    }
    __syncthreads();
    const double floor_e = static_cast<double>(min_eig);
    const int tx = tid & (CT_X - 1);
    for (int ty = tid / CT_X; ty < CT_Y; ty += 256 / CT_X) {
        const double* p = s_e + (ty + 1) * CE_X + (tx + 1);
        const double c = p[0];
        if (!(c >= floor_e) || !(c > 0)) continue;             // (outside V: -infinity)
        if (!(c > p[-CE_X - 1]) || !(c > p[-CE_X]) || !(c > p[-CE_X + 1]) || !(c > p[-1])) continue;
        if (!(c >= p[1]) || !(c >= p[CE_X - 1]) || !(c >= p[CE_X]) || !(c >= p[CE_X + 1])) continue;
        const unsigned slot = atomicAdd(counter, 1u);          // keeps counting past the capacity: the host reads the need
        if (slot >= cap) continue;
        const unsigned pos = static_cast<unsigned>(y0 + ty) * static_cast<unsigned>(w) + static_cast<unsigned>(x0 + tx);
        keys[slot] = (static_cast<unsigned long long>(~__float_as_uint(static_cast<float>(c))) << 32) | pos;
    }
}

// ---- S69: keys are distinct; ascending key order = score descending, then scan order.  rank = number of smaller keys.
__global__ __launch_bounds__(256) void corner_rank(const unsigned* counter, unsigned cap, const unsigned long long* keys,
                                                   unsigned long long* sorted)
{
    __shared__ unsigned long long s_key[256];
    const unsigned n = *counter;
    if (n > cap) return;
    if (blockIdx.x * 256u >= n) return;
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    const unsigned long long mine = t < n ? keys[t] : 0ull;
    const unsigned rank = pm::rank_below(keys, n, mine, s_key);
    if (t < n) sorted[rank] = mine;
}

// ---- S69 quality cut + S70.  One workgroup walks the ranks in chunks of ST, one candidate per thread:
//   1. each candidate against the keep points and the rows accepted so far (the output array is the accepted list);
//   2. its conflicts with the lower ranks of the chunk, as a bit mask;
//   3. rounds: accepted once every conflicting lower rank is rejected, rejected once one is accepted.  The lowest undecided
//      rank is decided in every round, so the rounds end, with the serial loop's decisions;
//   4. the accepted ranks are appended in rank order up to the limit.
constexpr int ST = 512, SW = ST / 64;

struct SelArgs {
    const unsigned* counter;
    const unsigned long long* sorted;
    unsigned cap;
    int w;
    float quality, min_dist;
    const float* keep;                 // the _dev form: cap_keep rows and an optional device count
    const int32_t* d_n_keep;
    int cap_keep, max_corners;
    float* xy;                         // the _dev form: rows from 0; replenish: d_pts, whose first *d_count rows are the keep points
    float* score;
    int32_t* d_n;                      // the _dev form: *d_n; replenish: *d_n_new (may be null)
    int32_t* d_count;                  // replenish only
    int cap_pts, target;
    int replenish, pad;
};

__device__ __forceinline__ bool blocks(float fx, float fy, float ox, float oy, float md2)
{
    const float dx = fx - ox, dy = fy - oy;
    return dx * dx + dy * dy < md2;
}

__global__ __launch_bounds__(ST) void corner_select(const SelArgs a)
{
    __shared__ float s_x[ST], s_y[ST];
    __shared__ unsigned long long s_acc[SW], s_rej[SW];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const unsigned cnt = *a.counter;
    int n_keep, row_off, limit;
    const float* keep;
    if (a.replenish) {
        const int c = *a.d_count;
        n_keep = c < 0 ? 0 : (c > a.cap_pts ? a.cap_pts : c);
        keep = a.xy;
        row_off = n_keep;
        limit = max(min(a.target, a.cap_pts) - n_keep, 0);
    } else {
        const int c = a.keep ? (a.d_n_keep ? *a.d_n_keep : a.cap_keep) : 0;
        n_keep = c < 0 ? 0 : (c > a.cap_keep ? a.cap_keep : c);
        keep = a.keep;
        row_off = 0;
        limit = a.max_corners;
    }
    __syncthreads();                                           // every thread has read *d_count before thread 0 writes it
    if (cnt > a.cap) {                                         // overflow: no rows, never a subset
        if (tid == 0 && a.d_n) *a.d_n = -1;
        return;
    }
    const unsigned n = cnt;
    const float md2 = a.min_dist * a.min_dist;
    const float thr = n ? a.quality * __uint_as_float(~static_cast<unsigned>(a.sorted[0] >> 32)) : 0.f;
    float* out = a.xy + 2 * static_cast<size_t>(row_off);
    float* out_s = a.score ? a.score + row_off : nullptr;
    int n_acc = 0;
    for (unsigned base = 0; base < n && n_acc < limit; base += ST) {
        const unsigned idx = base + tid;
        const unsigned long long key = idx < n ? a.sorted[idx] : 0ull;
        const float s = __uint_as_float(~static_cast<unsigned>(key >> 32));
        const unsigned pos = static_cast<unsigned>(key);
        const unsigned yy = pos / static_cast<unsigned>(a.w);
        const float fx = static_cast<float>(pos - yy * static_cast<unsigned>(a.w)), fy = static_cast<float>(yy);
        int state = (idx < n && !(s < thr)) ? 0 : 2;           // 0 undecided, 1 accepted, 2 rejected
        if (state == 0) {
            bool hit = false;
            for (int k = 0; k < n_keep; ++k) hit |= blocks(fx, fy, keep[2 * static_cast<size_t>(k)], keep[2 * static_cast<size_t>(k) + 1], md2);
            for (int k = 0; k < n_acc; ++k) hit |= blocks(fx, fy, out[2 * static_cast<size_t>(k)], out[2 * static_cast<size_t>(k) + 1], md2);
            if (hit) state = 2;
        }
        s_x[tid] = fx;
        s_y[tid] = fy;
        __syncthreads();
        unsigned long long conf[SW];
#pragma unroll
        for (int wd = 0; wd < SW; ++wd) {
            unsigned long long m = 0;
            if (wd <= wv && __any(state == 0)) {
#pragma unroll 4
                for (int j = 0; j < 64; ++j)
                    if (blocks(fx, fy, s_x[wd * 64 + j], s_y[wd * 64 + j], md2)) m |= 1ull << j;
                if (wd == wv) m &= (1ull << lane) - 1ull;      // lower ranks only
            }
            conf[wd] = m;
        }
        for (;;) {
            const unsigned long long ba = __ballot(state == 1), br = __ballot(state == 2);
            if (lane == 0) {
                s_acc[wv] = ba;
                s_rej[wv] = br;
            }
            __syncthreads();
            bool all_done = true, blocked = false, pending = false;
#pragma unroll
            for (int wd = 0; wd < SW; ++wd) {
                const unsigned long long ac = s_acc[wd], rj = s_rej[wd];
                all_done &= (ac | rj) == ~0ull;
                blocked |= (conf[wd] & ac) != 0;
                pending |= (conf[wd] & ~(ac | rj)) != 0;
            }
            if (all_done) break;                               // (the same words on every thread: a uniform exit)
            if (state == 0) state = blocked ? 2 : (pending ? 0 : 1);
            __syncthreads();
        }
        // append in rank order; s_acc holds the final flags
        int before = 0, total = 0;
#pragma unroll
        for (int wd = 0; wd < SW; ++wd) {
            const int c = __popcll(s_acc[wd]);
            if (wd < wv) before += c;
            total += c;
        }
        before += pm::lane_rank(s_acc[wv], lane);
        const int row = n_acc + before;
        if (state == 1 && row < limit) {
            out[2 * static_cast<size_t>(row)] = fx;
            out[2 * static_cast<size_t>(row) + 1] = fy;
            if (out_s) out_s[row] = s;
        }
        n_acc = min(n_acc + total, limit);
        __syncthreads();                                       // the rows are visible to, and s_x / s_acc free for, the next chunk
    }
    if (tid == 0) {
        if (a.d_n) *a.d_n = n_acc;
        if (a.replenish) *a.d_count = n_keep + n_acc;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------

int check_params(const pm_corner_params* p)
{
    PM_REQUIRE(p != nullptr, PM_E_INVALID, "null parameters");
    PM_REQUIRE(p->block_radius >= 1 && p->block_radius <= MAX_R, PM_E_INVALID, "block_radius outside [1, 15]");
    PM_REQUIRE(p->min_eig >= 0 && p->min_eig <= 3.0e38f, PM_E_INVALID, "min_eig must be finite and >= 0");
    PM_REQUIRE(p->quality >= 0 && p->quality <= 1.0f, PM_E_INVALID, "quality outside [0, 1]");
    PM_REQUIRE(p->min_dist >= 0 && p->min_dist <= 1.0e6f, PM_E_INVALID, "min_dist outside [0, 1e6]");
    PM_REQUIRE(p->capacity >= 0 && p->capacity <= (1 << 24), PM_E_INVALID, "capacity outside [0, 2^24]");
    PM_REQUIRE(p->flags == 0 && p->reserved[0] == 0 && p->reserved[1] == 0, PM_E_INVALID, "flags or reserved != 0");
    return PM_OK;
}

size_t run_capacity(const pm_corner_params* p, int rows)
{
    if (p->capacity > 0) return static_cast<size_t>(p->capacity);
    return std::min<size_t>(std::max<size_t>(65536, 8 * static_cast<size_t>(rows)), size_t(1) << 24);
}

// The three launches.  a: the selection's arguments but for the scratch pointers; cap: candidate capacity of this run.
// counter_out (may be null) receives the device address of the candidate counter, which is the need after an overflow.
int corners_enqueue(pm_ctx* ctx, const pm_pyramid* pyr, const pm_corner_params* p, size_t cap, SelArgs a, unsigned** counter_out)
{
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t key_b = pm::align_up(cap * 8, 256);
    int rc = pm::arena_reserve(ctx, 256 + 2 * key_b + 512);
    if (rc != PM_OK) return rc;
    pm::arena_reset(ctx);
    unsigned* counter = static_cast<unsigned*>(pm::arena_take(ctx, 256));
    unsigned long long* keys = static_cast<unsigned long long*>(pm::arena_take(ctx, key_b));
    unsigned long long* sorted = static_cast<unsigned long long*>(pm::arena_take(ctx, key_b));
    PM_REQUIRE(counter != nullptr && keys != nullptr && sorted != nullptr, PM_E_NOMEM, "scratch arena too small");
    if (counter_out) *counter_out = counter;
    hipStream_t s = ctx->stream;
    PM_HIP_CHECK(hipMemsetAsync(counter, 0, sizeof(unsigned), s));
    const int r = p->block_radius;
    const int vw = pyr->w - 2 * r - 3, vh = pyr->h - 2 * r - 3;   // V: r + 1 .. w - r - 3
    if (vw >= 1 && vh >= 1) {
        {
            pm::ScopedKernelTime timer(ctx, "corner_extrema");
            hipLaunchKernelGGL(corner_extrema, dim3((vw + CT_X - 1) / CT_X, (vh + CT_Y - 1) / CT_Y), dim3(256), 0, s, pyr->mem + pyr->off[0],
                               pyr->w, pyr->h, r, p->min_eig, counter, static_cast<unsigned>(cap), keys);
        }
        {
            pm::ScopedKernelTime timer(ctx, "corner_rank");
            hipLaunchKernelGGL(corner_rank, dim3(static_cast<unsigned>((cap + 255) / 256)), dim3(256), 0, s, counter, static_cast<unsigned>(cap),
                               keys, sorted);
        }
    }
    a.counter = counter;
    a.sorted = sorted;
    a.cap = static_cast<unsigned>(cap);
    a.w = pyr->w;
    a.quality = p->quality;
    a.min_dist = p->min_dist;
    {
        pm::ScopedKernelTime timer(ctx, "corner_select");
        hipLaunchKernelGGL(corner_select, dim3(1), dim3(ST), 0, s, a);
    }
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

int check_dev_args(pm_ctx* ctx, const pm_pyramid* pyr, const pm_corner_params* p, const float* d_keep, int cap_keep, int max_corners,
                   const float* d_xy, const int32_t* d_n)
{
    PM_REQUIRE(pyr != nullptr && d_xy != nullptr && d_n != nullptr, PM_E_INVALID, "null pyramid or output pointer");
    const int rc = check_params(p);
    if (rc != PM_OK) return rc;
    PM_REQUIRE(cap_keep >= 0 && (d_keep != nullptr || cap_keep == 0), PM_E_INVALID, "cap_keep < 0, or keep points missing");
    PM_REQUIRE(max_corners >= 0, PM_E_INVALID, "max_corners < 0");
    PM_REQUIRE(pyr->device == ctx->device, PM_E_INVALID, "pyramid of another device");
    PM_REQUIRE(max_corners >= 1, PM_E_UNSUPPORTED, "max_corners == 0: nothing to find");
    return PM_OK;
}

SelArgs dev_args(const float* d_keep, const int32_t* d_n_keep, int cap_keep, int max_corners, float* d_xy, float* d_score, int32_t* d_n)
{
    SelArgs a;
    memset(&a, 0, sizeof a);
    a.keep = cap_keep > 0 ? d_keep : nullptr;
    a.d_n_keep = d_n_keep;
    a.cap_keep = cap_keep;
    a.max_corners = max_corners;
    a.xy = d_xy;
    a.score = d_score;
    a.d_n = d_n;
    return a;
}

}  // namespace

extern "C" int pm_corners_dev(pm_ctx* ctx, const pm_pyramid* pyr, const pm_corner_params* p, const float* d_keep, const int32_t* d_n_keep,
                              int cap_keep, int max_corners, float* d_xy, float* d_score, int32_t* d_n)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    const int rc = check_dev_args(ctx, pyr, p, d_keep, cap_keep, max_corners, d_xy, d_n);
    if (rc != PM_OK) return rc;
    return corners_enqueue(ctx, pyr, p, run_capacity(p, max_corners), dev_args(d_keep, d_n_keep, cap_keep, max_corners, d_xy, d_score, d_n),
                           nullptr);
}

extern "C" int pm_corners_replenish_dev(pm_ctx* ctx, const pm_pyramid* pyr, const pm_corner_params* p, float* d_pts, int32_t* d_count,
                                        int cap, int target, float* d_score, int32_t* d_n_new)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    PM_REQUIRE(pyr != nullptr && d_pts != nullptr && d_count != nullptr, PM_E_INVALID, "null pyramid, points or count pointer");
    const int rc = check_params(p);
    if (rc != PM_OK) return rc;
    PM_REQUIRE(cap >= 0 && target >= 0, PM_E_INVALID, "cap < 0 or target < 0");
    PM_REQUIRE(pyr->device == ctx->device, PM_E_INVALID, "pyramid of another device");
    PM_REQUIRE(cap >= 1, PM_E_UNSUPPORTED, "cap == 0: no room for points");
    SelArgs a;
    memset(&a, 0, sizeof a);
    a.xy = d_pts;
    a.score = d_score;
    a.d_n = d_n_new;
    a.d_count = d_count;
    a.cap_pts = cap;
    a.target = target;
    a.replenish = 1;
    return corners_enqueue(ctx, pyr, p, run_capacity(p, std::min(target, cap)), a, nullptr);
}

extern "C" int pm_corners(pm_ctx* ctx, const uint8_t* img, int w, int h, int stride, const pm_corner_params* p, const float* keep, int n_keep,
                          int max_corners, float* xy, float* score, int32_t* n_out)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    PM_REQUIRE(img != nullptr && xy != nullptr && n_out != nullptr, PM_E_INVALID, "null pointer");
    PM_REQUIRE(w >= 1 && h >= 1 && stride >= w, PM_E_INVALID, "need w, h >= 1, stride >= w");
    PM_REQUIRE(n_keep >= 0 && (keep != nullptr || n_keep == 0), PM_E_INVALID, "n_keep < 0, or keep points missing");
    PM_REQUIRE(max_corners >= 0, PM_E_INVALID, "max_corners < 0");
    int rc = check_params(p);
    if (rc != PM_OK) return rc;
    PM_REQUIRE(max_corners >= 1, PM_E_UNSUPPORTED, "max_corners == 0: nothing to find");
    *n_out = 0;
    pm_pyramid* pyr = nullptr;
    rc = pm_pyramid_create(ctx, w, h, 0, &pyr);
    if (rc == PM_OK) {                                       // the blocks are freed before the pyramid is destroyed
        const size_t img_b = static_cast<size_t>(h) * stride, keep_b = static_cast<size_t>(n_keep) * 8;
        pm::StagedBlock in(ctx, __func__);                   // lives across the rounds
        const size_t o_img = in.add(img_b), o_keep = in.add(keep_b);
        in.alloc();
        in.upload(o_img, img, img_b);
        in.upload(o_keep, keep, keep_b);
        if (in.rc == PM_OK) in.rc = pm_pyramid_build_dev(ctx, pyr, in.at<uint8_t>(o_img), stride);
        rc = in.sync();
        size_t cap = run_capacity(p, max_corners);
        int32_t n = 0;
        // two rounds at most: the counter of an overflowed run is the exact need of the next (same image, same floor)
        for (int round = 0; rc == PM_OK && round < 2; ++round) {
            const size_t rows = static_cast<size_t>(max_corners);
            pm::StagedBlock b(ctx, __func__);                // this round's outputs
            const size_t o_n = b.add(sizeof n), o_xy = b.add(rows * 8), o_s = b.add(rows * 4);
            b.alloc();
            unsigned* d_counter = nullptr;
            if (b.rc == PM_OK)
                b.rc = corners_enqueue(ctx, pyr, p, cap,
                                       dev_args(n_keep ? in.at<float>(o_keep) : nullptr, nullptr, n_keep, max_corners, b.at<float>(o_xy),
                                                b.at<float>(o_s), b.at<int32_t>(o_n)),
                                       &d_counter);
            unsigned need = 0;
            b.download(&n, o_n, sizeof n);
            if (b.rc == PM_OK) b.step(hipMemcpyAsync(&need, d_counter, sizeof need, hipMemcpyDeviceToHost, ctx->stream), PM_E_HIP, "D2H copy");
            rc = b.sync();
            if (rc == PM_OK && n >= 0) {
                b.download(xy, o_xy, static_cast<size_t>(n) * 8);
                if (score) b.download(score, o_s, static_cast<size_t>(n) * 4);
                rc = b.sync();
                if (rc == PM_OK) *n_out = n;                 // only once every row has arrived
                break;
            }
            if (rc == PM_OK) {
                if (need <= cap) { pm::set_error("%s: overflow reported without a larger need", __func__); rc = PM_E_HIP; }
                else cap = need;
            }
        }
        if (rc == PM_OK && n < 0) { pm::set_error("%s: the candidate buffer overflowed again after growing", __func__); rc = PM_E_HIP; }
    }
    (void)pm_pyramid_destroy(pyr);
    return rc;
}
