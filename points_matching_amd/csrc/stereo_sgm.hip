// stereo_sgm.hip — semi-global matching on a rectified 8-bit pair: pm_stereo_sgm[_dev] (docs/SPEC.md S89-S92).  Every quantity
// is an integer, so the order of the sums is free and the map is a function of the inputs alone.
//
// sgm_census: a 256-thread workgroup owns a 64 x 4 tile of one image, staged with its 4-column / 3-row margin in LDS; a thread
// forms the 62 bits of its pixel and stores one u64.  The workgroups of the base image also fill the map with
// PM_STEREO_INVALID, so the last pass only has to write the computed rectangle.
//
// sgm_path: A LANE OWNS A DISPARITY, as in stereo_bm, and a WAVE WALKS A PATH.  Lane k holds L_r(p, dmin + k) (NC = ceil(D / 64)
// values per lane).  Per step the cost is recomputed from the census words, never stored: the base word is one address for the
// wave, the other image's words of the 64 lanes are 512 consecutive bytes, the cost one 64-bit population count of the
// exclusive or.  min_k L_r(q, k) is one DPP wave minimum; L_r(q, d -+ 1) a shift by one lane, with the lane at the edge of a
// 64-lane group reading the neighbouring group.  Lanes beyond D hold BIG, which no minimum picks, so the terms of S91 whose
// d -+ 1 is outside the range drop out by themselves.  The sums S are u16 laid out [y][x][d]: a step's read-add-write is one
// contiguous row of 2 D bytes.  A step's words and sums are loaded eight steps ahead (four for D > 128) into a register ring.
// A horizontal pass has a wave per row.  A vertical or diagonal pass has a wave per start column that steps one row at a time
// and moves its column by dx; when it leaves the rectangle's side it enters at the other side and restarts with L = C, so wc
// waves cover every diagonal path.  The first pass writes S, the others add, the last one does not store: it picks the winner
// of S85 with the sums still in registers (stereo_core::winner, the one stereo_bm calls) and writes the map.  The range and size
// rules of the arguments are image_args.hpp's, the host form is StagedBlock::stereo (pm_common.hpp).
#include <cstdint>

#include "pm_common.hpp"
#include "stereo_core.hpp"
#include "stereo_sgm_plan.hpp"
#include "wave_ops.hpp"

namespace {

using stereo_core::INVALID;

constexpr unsigned BIG = 1u << 16;                        // above every L_r + p2 (<= 2108): a lane that holds no disparity
constexpr int TW = pm_sgm::CENSUS_TILE_W, TH = pm_sgm::CENSUS_TILE_H, MX = pm_sgm::MARGIN_X, MY = pm_sgm::MARGIN_Y;
constexpr int LW = TW + 2 * MX, LH = TH + 2 * MY;         // the staged tile: 72 x 10 bytes
using u64 = unsigned long long;

struct CensusArgs {
    const uint8_t* img[2];                                // [0]: the image whose pixels get a disparity
    int stride[2];
    u64* out[2];                                          // planes of `rows` x w words, row 0 is image row 3
    int w, h, rows, nbx;
    int16_t* disp;
    int dstride;
};

__global__ __launch_bounds__(256) void sgm_census(CensusArgs a)
{
    __shared__ uint8_t s_t[LH][LW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, which = blockIdx.y;
    const int by = blockIdx.x / a.nbx, bx = blockIdx.x - by * a.nbx;
    const int x0 = bx * TW, y0 = by * TH;
    const uint8_t* img = a.img[which];
    const int stride = a.stride[which];
    for (int e = tid; e < LH * LW; e += 256) {
        const int ry = e / LW, rx = e - ry * LW;
        const int y = y0 - MY + ry, x = x0 - MX + rx;
        s_t[ry][rx] = (y >= 0 && y < a.h && x >= 0 && x < a.w) ? img[static_cast<size_t>(y) * stride + x] : 0;
    }
    __syncthreads();
    const int x = x0 + lane, y = y0 + wave;
    if (x >= a.w || y >= a.h) return;
    if (which == 0) a.disp[static_cast<size_t>(y) * a.dstride + x] = static_cast<int16_t>(INVALID);
    if (y < MY || y > a.h - 1 - MY) return;
    u64 bits = 0;
    if (x >= MX && x <= a.w - 1 - MX) {                   // elsewhere no computed pixel reads the word
        const unsigned c = s_t[wave + MY][lane + MX];
#pragma unroll
        for (int j = 0; j < 2 * MY + 1; ++j)
#pragma unroll
            for (int i = 0; i < 2 * MX + 1; ++i)
                if (j != MY || i != MX) bits = (bits << 1) | (s_t[wave + j][lane + i] < c ? 1u : 0u);
    }
    a.out[which][static_cast<size_t>(y - MY) * a.w + x] = bits;
}

struct PathArgs {
    const u64* cb;                                        // census planes: base and other
    const u64* co;
    uint16_t* S;                                          // [hc][wc][D]
    int w, cx0, wc, hc;
    int dmin, D, sgn, p1, p2;
    int dx, dy, steps;
    int uniq;                                             // the winner pass only
    int16_t* disp;                                        // at (cx0, cy0) of the map
    int dstride;
    pm_stereo_info* info;
};

enum { WRITE = 0, ADD = 1, WINNER = 2 };

// One wave per workgroup: blockIdx.x is the row (dy == 0) or the start column.
template <int NC, int MODE>
__global__ __launch_bounds__(64) void sgm_path(PathArgs a)
{
    const int lane = threadIdx.x, D = a.D;
    int col, row;
    if (a.dy == 0) {
        row = blockIdx.x;
        col = a.dx > 0 ? 0 : a.wc - 1;
    } else {
        col = blockIdx.x;
        row = a.dy > 0 ? 0 : a.hc - 1;
    }
    int off[NC], kc[NC];                                  // column offset of this lane's disparities in the other plane
    bool live[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int k = lane + 64 * c;
        live[c] = k < D;
        kc[c] = min(k, D - 1);
        off[c] = a.sgn * (a.dmin + kc[c]);
    }
    // A step's words and sums are loaded K steps ahead into a ring of registers (every index a constant after unrolling): with
    // one or two waves on a SIMD nothing else hides the latency of memory, and registers are plentiful at that occupancy.
    // K is bounded by the 63 memory operations the wave's counter can tell apart: a step issues 1 + 2 NC loads and NC stores.
    // The base word is loaded through a vector address on purpose (vzero is a VGPR the compiler cannot fold): scalar loads
    // return out of order, so waiting for one waits for them all, the one just issued for K steps ahead included.
    constexpr int K = NC <= 2 ? 8 : 4;
    int vzero;
    asm volatile("v_mov_b32 %0, 0" : "=v"(vzero));
    u64 ring_b[K], ring_o[K][NC];
    unsigned ring_s[K][NC];
    // Positions are pointers moved by constants (64-bit multiplies per step cost more than the step's arithmetic): per step
    // dx + dy w census words and (dx + dy wc) D sums, and -+ wc columns where a diagonal wave enters at the other side.
    const ptrdiff_t cen_step = static_cast<ptrdiff_t>(a.dy) * a.w + a.dx, cen_wrap = a.wc;
    const ptrdiff_t sum_step = (static_cast<ptrdiff_t>(a.dy) * a.wc + a.dx) * D, sum_wrap = static_cast<ptrdiff_t>(a.wc) * D;
    const size_t cen0 = static_cast<size_t>(row) * a.w + a.cx0 + col, sum0 = (static_cast<size_t>(row) * a.wc + col) * D;
    int hcol = col;                                       // the position the next load is for
    const u64* hb = a.cb + cen0 + vzero;
    const u64* ho = a.co + cen0;
    const uint16_t* hs = a.S + sum0;
    auto load = [&](u64& b, u64(&o)[NC], unsigned(&s)[NC]) __attribute__((always_inline)) {
        b = *hb;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            o[c] = ho[off[c]];
            s[c] = MODE != WRITE ? hs[kc[c]] : 0u;        // a lane beyond D reads the last sum and never uses it
        }
        hcol += a.dx;
        ptrdiff_t dc = cen_step, ds = sum_step;
        if (hcol < 0) hcol = a.wc - 1, dc += cen_wrap, ds += sum_wrap;
        else if (hcol >= a.wc) hcol = 0, dc -= cen_wrap, ds -= sum_wrap;
        hb += dc;
        ho += dc;
        hs += ds;
    };
#pragma unroll
    for (int u = 0; u < K; ++u) {
        ring_b[u] = 0;
#pragma unroll
        for (int c = 0; c < NC; ++c) ring_o[u][c] = 0, ring_s[u][c] = 0;
        if (u < a.steps) load(ring_b[u], ring_o[u], ring_s[u]);
    }

    unsigned L[NC], m = 0;
    bool restart = true;
    int n_valid = 0;
    uint16_t* cs = a.S + sum0;                            // this step's sums and its pixel of the map
    int16_t* cd = a.disp + static_cast<size_t>(row) * a.dstride + col;
    const ptrdiff_t map_step = static_cast<ptrdiff_t>(a.dy) * a.dstride + a.dx;
    // one step at the current position (col, cs, cd) from ring slot (rb, ro, rs), which is refilled for the step K ahead when there is one
    auto advance = [&](u64& rb, u64(&ro)[NC], unsigned(&rs)[NC], bool refill) __attribute__((always_inline)) {
        const u64 cur_b = rb;
        u64 cur_o[NC];
        unsigned cur_s[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) cur_o[c] = ro[c], cur_s[c] = rs[c];
        int ncol = col + a.dx;
        ptrdiff_t ds = sum_step, dm = map_step;
        bool nrestart = false;
        if (ncol < 0) ncol = a.wc - 1, nrestart = true, ds += sum_wrap, dm += a.wc;
        else if (ncol >= a.wc) ncol = 0, nrestart = true, ds -= sum_wrap, dm -= a.wc;

        unsigned lo = BIG;
        if (restart) {
#pragma unroll
            for (int c = 0; c < NC; ++c) L[c] = live[c] ? static_cast<unsigned>(__popcll(cur_b ^ cur_o[c])) : BIG;
        } else {
            unsigned nl[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                // L(q, d - 1), L(q, d + 1): the wave shifted by one lane in one DPP move each (wave_shr:1, wave_shl:1); the two
                // lanes at the ends of the wave are set below, so what the shift leaves in them does not matter
                unsigned below = static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(L[c]), 0x138, 0xF, 0xF, false));
                unsigned above = static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(L[c]), 0x130, 0xF, 0xF, false));
                const unsigned edge_lo = c > 0 ? __builtin_amdgcn_readlane(L[c > 0 ? c - 1 : 0], 63) : BIG;
                const unsigned edge_hi = c < NC - 1 ? __builtin_amdgcn_readlane(L[c < NC - 1 ? c + 1 : c], 0) : BIG;
                if (lane == 0) below = edge_lo;
                if (lane == 63) above = edge_hi;
                const unsigned best = min(min(L[c], m + a.p2), min(below, above) + a.p1);
                nl[c] = live[c] ? static_cast<unsigned>(__popcll(cur_b ^ cur_o[c])) + best - m : BIG;
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) L[c] = nl[c];
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) lo = min(lo, L[c]);
        m = pm::wave_min_u32_id(lo);

        unsigned Sv[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) Sv[c] = cur_s[c] + L[c];
        if (MODE != WINNER) {
#pragma unroll
            for (int c = 0; c < NC; ++c)
                if (live[c]) cs[lane + 64 * c] = static_cast<uint16_t>(Sv[c]);
        } else {
            const stereo_core::Won won = stereo_core::winner<pm::wave_min_u32_id>(Sv, live, lane, D, a.dmin, a.uniq);
            if (won.kept) ++n_valid;
            if (lane == 0) *cd = static_cast<int16_t>(won.value);
        }
        col = ncol;
        cs += ds;
        cd += dm;
        restart = nrestart;
        // refilled last, when the slot's values are dead: the loads land in the registers the loop carries, and the only wait
        // is the one in front of a slot's first use K - 1 steps later (refilled first, every round ended waiting for them all)
        if (refill) load(rb, ro, rs);
    };
    int step = 0;
    for (; step + 2 * K <= a.steps; step += K)            // whole rounds of the ring in which every slot is refilled
#pragma unroll
        for (int u = 0; u < K; ++u) advance(ring_b[u], ring_o[u], ring_s[u], true);
    for (; step < a.steps; step += K)                     // the last one or two rounds
#pragma unroll
        for (int u = 0; u < K; ++u)
            if (step + u < a.steps) advance(ring_b[u], ring_o[u], ring_s[u], step + u + K < a.steps);
    if (MODE == WINNER && a.info && lane == 0 && n_valid) atomicAdd(&a.info->n_valid, n_valid);
}

template <int MODE>
void launch_path(int nc, unsigned grid, hipStream_t stream, const PathArgs& a)
{
    switch (nc) {
    case 1: hipLaunchKernelGGL((sgm_path<1, MODE>), dim3(grid), dim3(64), 0, stream, a); break;
    case 2: hipLaunchKernelGGL((sgm_path<2, MODE>), dim3(grid), dim3(64), 0, stream, a); break;
    case 3: hipLaunchKernelGGL((sgm_path<3, MODE>), dim3(grid), dim3(64), 0, stream, a); break;
    default: hipLaunchKernelGGL((sgm_path<4, MODE>), dim3(grid), dim3(64), 0, stream, a); break;
    }
}

// the checks of S90's contract in pm_stereo_bm's order; the plan on success
int check_sgm(const void* left, const void* right, int w, int h, int lstride, int rstride, const pm_sgm_params* p, const void* disp, int dstride,
              pm_sgm::Plan* plan)
{
    PM_REQUIRE(left != nullptr && right != nullptr && p != nullptr && disp != nullptr, PM_E_INVALID, "null pointer");
    *plan = pm_sgm::plan(w, h, lstride, rstride, dstride, p);
    PM_REQUIRE(plan->status == PM_OK, plan->status, plan->why);
    return PM_OK;
}

}  // namespace

extern "C" int pm_stereo_sgm_dev(pm_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right, int w, int h, int lstride, int rstride,
                                 const pm_sgm_params* p, int16_t* d_disp, int dstride, pm_stereo_info* d_info)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    pm_sgm::Plan q;
    const int rc = check_sgm(d_left, d_right, w, h, lstride, rstride, p, d_disp, dstride, &q);
    if (rc != PM_OK) return rc;
    PM_REQUIRE_PASS(pm_image::disparity_map_ranges(d_left, d_right, w, h, lstride, rstride, d_disp, dstride, d_info));
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    pm::arena_reset(ctx);
    const int rc3 = pm::arena_reserve(ctx, q.need);
    if (rc3 != PM_OK) return rc3;
    u64* cb = static_cast<u64*>(pm::arena_take(ctx, q.census_bytes));
    u64* co = static_cast<u64*>(pm::arena_take(ctx, q.census_bytes));
    uint16_t* S = static_cast<uint16_t*>(pm::arena_take(ctx, q.s_bytes));
    PM_REQUIRE(cb && co && S, PM_E_NOMEM, "scratch arena too small");
    if (d_info) PM_HIP_CHECK(hipMemsetAsync(d_info, 0, sizeof(pm_stereo_info), ctx->stream));
    {
        CensusArgs c;
        c.img[0] = q.from_right ? d_right : d_left;
        c.img[1] = q.from_right ? d_left : d_right;
        c.stride[0] = q.from_right ? rstride : lstride;
        c.stride[1] = q.from_right ? lstride : rstride;
        c.out[0] = cb; c.out[1] = co;
        c.w = w; c.h = h; c.rows = q.rows;
        c.nbx = (w + TW - 1) / TW;
        c.disp = d_disp; c.dstride = dstride;
        pm::ScopedKernelTime timer(ctx, "sgm_census");
        hipLaunchKernelGGL(sgm_census, dim3(q.census_grid_x, 2), dim3(256), 0, ctx->stream, c);
    }
    PM_HIP_CHECK(hipGetLastError());
    PathArgs a;
    a.cb = cb; a.co = co; a.S = S;
    a.w = w; a.cx0 = q.cx0; a.wc = q.wc; a.hc = q.hc;
    a.dmin = p->min_disp; a.D = p->num_disp; a.sgn = q.sgn; a.p1 = p->p1; a.p2 = p->p2;
    a.uniq = p->uniqueness;
    a.disp = d_disp + static_cast<size_t>(q.cy0) * dstride + q.cx0;
    a.dstride = dstride; a.info = d_info;
    for (int i = 0; i < q.npass; ++i) {
        a.dx = q.pass[i].dx; a.dy = q.pass[i].dy; a.steps = q.pass[i].steps;
        const bool last = i == q.npass - 1;
        pm::ScopedKernelTime timer(ctx, last ? "sgm_path_winner" : "sgm_path");
        if (i == 0) launch_path<WRITE>(q.nc, q.pass[i].grid, ctx->stream, a);
        else if (!last) launch_path<ADD>(q.nc, q.pass[i].grid, ctx->stream, a);
        else launch_path<WINNER>(q.nc, q.pass[i].grid, ctx->stream, a);
    }
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_stereo_sgm(pm_ctx* ctx, const uint8_t* left, const uint8_t* right, int w, int h, int lstride, int rstride,
                             const pm_sgm_params* p, int lr_max_diff16, int16_t* disp, int dstride, pm_stereo_info* info)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REFUSE_CAPTURE(ctx);
    pm_sgm::Plan q;
    const int rc = check_sgm(left, right, w, h, lstride, rstride, p, disp, dstride, &q);
    if (rc != PM_OK) return rc;
    const bool lr = lr_max_diff16 >= 0;
    PM_REQUIRE(!lr || (p->flags & PM_STEREO_FROM_RIGHT) == 0, PM_E_INVALID, "the left-right check needs the left map: no PM_STEREO_FROM_RIGHT");
    PM_REQUIRE_PASS(pm_image::disparity_map_ranges(left, right, w, h, lstride, rstride, disp, dstride, info));
    pm_sgm_params pr = *p;
    pr.flags |= PM_STEREO_FROM_RIGHT;
    return pm::StagedBlock::stereo(
        ctx, __func__, left, right, w, h, lstride, rstride, lr_max_diff16, disp, dstride, info,
        [&](const uint8_t* l, const uint8_t* r, int16_t* d, pm_stereo_info* i) { return pm_stereo_sgm_dev(ctx, l, r, w, h, lstride, rstride, p, d, dstride, i); },
        [&](const uint8_t* l, const uint8_t* r, int16_t* d) { return pm_stereo_sgm_dev(ctx, l, r, w, h, lstride, rstride, &pr, d, w, nullptr); });
}
