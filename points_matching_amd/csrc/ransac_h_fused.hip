// ransac_h_fused.hip — RANSAC-H in ONE launch on gfx950 (MI355X): 4-sample + normalised 4-point DLT + reprojection
// scoring of every hypothesis against every correspondence + winner + inlier mask (docs/SPEC.md S19-S22).  The
// counterpart of cv::findHomography(pts1, pts2, RANSAC, thr), sibling of the findFundamentalMat call at main.cpp:95-98.
//
// Same mapping as the default RANSAC-F launch (ransac_fused_kernels.hpp, ransac_fused_lds), whose view, slot and
// SGPR-model helpers it reuses:
//   * a workgroup owns `hb` consecutive hypothesis ids; lane s < hb of the first wave(s) samples and solves hypothesis s
//     (fp64, S20) while the other waves load the correspondences into LDS as packed pairs;
//   * 12 waves score WHOLE hypotheses (wave w: ids w, w + 12, ...): operands by ds_read_b64, model in SGPR pairs
//     feeding v_pk_fma_f32, verdicts counted on the scalar unit (s_bcnt1 of the ballot) — no atomics;
//   * each workgroup writes its best key (S22) and fp64 model to its slot and draws a ticket; the last one picks the
//     winner, publishes key / H / count and writes the mask.
#include "homography_core.hpp"
#include "homography_refine_core.hpp"
#include "ransac_fused_kernels.hpp"

namespace pm_ransac {
namespace {

using namespace pm_homog;

constexpr int RH_SYNC_WORD = 8;       // arrival ticket in ctx->sync_words (RANSAC-F uses words 0 and 2)

// SPEC S21 on two correspondences, model in SGPR pairs (the packed form of inlier_h32, same operations bit for bit).
// u, v, w use exactly the coefficient pairs of RANSAC-F's a, b, c.
__device__ __forceinline__ void inlier_h_pk_model(const ModelS& m, f32x2 x, f32x2 y, f32x2 xp, f32x2 yp, float thr2,
                                                  bool& ia, bool& ib)
{
    const f32x2 u = sfma_out<0>(m.q03, x, sfma_in<0, 1>(m.q12, y));        // h0*x + (h1*y + h2)
    const f32x2 v = sfma_out<1>(m.q03, x, sfma_in<0, 1>(m.q45, y));        // h3*x + (h4*y + h5)
    const f32x2 w = sfma_out<1>(m.q36, x, sfma_in<0, 1>(m.q78, y));        // h6*x + (h7*y + h8)
    const f32x2 du = __builtin_elementwise_fma(-xp, w, u);
    const f32x2 dv = __builtin_elementwise_fma(-yp, w, v);
    const f32x2 lhs = __builtin_elementwise_fma(du, du, dv * dv);
    const f32x2 rhs = f32x2{thr2, thr2} * (w * w);
    ia = (lhs[0] <= rhs[0]) && (w[0] != 0.f);
    ib = (lhs[1] <= rhs[1]) && (w[1] != 0.f);
}

__device__ __forceinline__ bool hyp_h_view(const pm_points_view& v, const int* __restrict__ offs, int n, uint64_t seed,
                                           uint64_t h, double (&H)[9])
{
    int idx[4];
    sample4(seed, h, n, idx);
    double x1[4], y1[4], x2[4], y2[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float2 a, b;
        view_point(v, offs, idx[i], a, b);
        x1[i] = static_cast<double>(a.x); y1[i] = static_cast<double>(a.y);
        x2[i] = static_cast<double>(b.x); y2[i] = static_cast<double>(b.y);
    }
    return solve4(x1, y1, x2, y2, H);
}

// NH hypotheses of one wave over the slots of the LDS tile in one pass (as score_lds).
template <int NH>
__device__ __forceinline__ void score_h_lds(const float (*s_mdl)[12], int* s_cnt, const f32x2* pp, int kslots, int s0, float thr2,
                                            int lane)
{
    ModelS ms[NH];
    int c[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        const float* m = s_mdl[s0 + h * RL_WAVES];
        ms[h] = model_to_sgprs(*reinterpret_cast<const f32x4v*>(m), *reinterpret_cast<const f32x4v*>(m + 4),
                               *reinterpret_cast<const f32x2*>(m + 8));
        c[h] = 0;
    }
    for (int slot = 0; slot < kslots; ++slot) {
        const f32x2 x = pp[0], y = pp[64], xp = pp[128], yp = pp[192];
        pp += 256;
#pragma unroll
        for (int h = 0; h < NH; ++h) {
            bool ia, ib;
            inlier_h_pk_model(ms[h], x, y, xp, yp, thr2, ia, ib);
            c[h] += __popcll(__ballot(ia)) + __popcll(__ballot(ib));
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int h = 0; h < NH; ++h) s_cnt[s0 + h * RL_WAVES] += c[h];
    }
}

__global__ __launch_bounds__(RL_THREADS) void ransac_h_fused(pm_points_view v, uint64_t seed, int64_t hyp_begin, int nh, int hb,
                                                             float thr2, int tile_slots, RfSlot* __restrict__ slots,
                                                             int* __restrict__ ticket, RfOut out)
{
    extern __shared__ __attribute__((aligned(16))) f32x2 s_pts[];           // [tile_slots][4][64]: X, Y, XP, YP pairs
    __shared__ __attribute__((aligned(16))) float s_mdl[RF_HB_MAX][12];    // f32 model + valid flag of hypothesis s
    __shared__ double s_m64[RF_HB_MAX][9];
    __shared__ int s_cnt[RF_HB_MAX];
    __shared__ int s_offs[PM_MAX_PARTS + 1];
    __shared__ unsigned long long s_wk[RL_WAVES];
    __shared__ double s_H64[9];
    __shared__ int s_role;
    __shared__ int s_wc[RL_WAVES];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int n;
    if (v.parts == 1) {
        n = view_count1(v);
    } else {
        view_offsets(v, s_offs, tid);
        __syncthreads();
        n = s_offs[v.parts];
    }
    const int tile_pts = tile_slots * RL_SLOT_PTS;
    const int ntiles = n > tile_pts ? (n + tile_pts - 1) / tile_pts : 1;
    const float nanv = __builtin_nanf("");
    // slot `slot`, lane `l` of the tile that starts at point `base`: points base + 2*(64*slot + l) and +1 (NaN past n)
    auto load_pair = [&](int base, int slot, int l) {
        const int i0 = base + 2 * (64 * slot + l);
        float2 a0 = {nanv, nanv}, b0 = a0, a1 = a0, b1 = a0;
        if (v.parts == 1) {
            if (n > 0) {
                const int j0 = i0 < n ? i0 : n - 1, j1 = i0 + 1 < n ? i0 + 1 : n - 1;      // clamped: never past n
                a0 = *reinterpret_cast<const float2*>(v.xy1 + 2 * static_cast<size_t>(j0));
                a1 = *reinterpret_cast<const float2*>(v.xy1 + 2 * static_cast<size_t>(j1));
                b0 = *reinterpret_cast<const float2*>(v.xy2 + 2 * static_cast<size_t>(j0));
                b1 = *reinterpret_cast<const float2*>(v.xy2 + 2 * static_cast<size_t>(j1));
            }
            if (i0 >= n) { a0 = float2{nanv, nanv}; b0 = a0; }
            if (i0 + 1 >= n) { a1 = float2{nanv, nanv}; b1 = a1; }
        } else {
            if (i0 < n) view_point(v, s_offs, i0, a0, b0);
            if (i0 + 1 < n) view_point(v, s_offs, i0 + 1, a1, b1);
        }
        f32x2* d = s_pts + (static_cast<size_t>(slot) * 4) * 64 + l;
        d[0] = f32x2{a0.x, a1.x}; d[64] = f32x2{a0.y, a1.y}; d[128] = f32x2{b0.x, b1.x}; d[192] = f32x2{b0.y, b1.y};
    };
    auto tile_kslots = [&](int t) {
        int k = (n - t * tile_pts + RL_SLOT_PTS - 1) / RL_SLOT_PTS;
        return k < 0 ? 0 : (k > tile_slots ? tile_slots : k);
    };

    // ---- solve (threads < hcount: S19, S20) || tile 0 -> LDS (the other waves)
    const int h0 = static_cast<int>(blockIdx.x) * hb;
    const int hcount = nh - h0 < hb ? nh - h0 : hb;
    const int solver_waves = (hcount + 63) / 64;
    if (wave < solver_waves) {
        if (tid < hcount) {
            double H[9];
            bool ok = false;
#pragma unroll
            for (int i = 0; i < 9; ++i) H[i] = 0.0;
            if (n >= 4) ok = hyp_h_view(v, s_offs, n, seed, static_cast<uint64_t>(hyp_begin + h0 + tid), H);
#pragma unroll
            for (int i = 0; i < 9; ++i) { s_mdl[tid][i] = static_cast<float>(H[i]); s_m64[tid][i] = H[i]; }
            s_mdl[tid][9] = ok ? 1.f : 0.f;
            s_mdl[tid][10] = 0.f; s_mdl[tid][11] = 0.f;
            s_cnt[tid] = 0;
        }
    } else {
        const int k0 = tile_kslots(0);
        for (int slot = wave - solver_waves; slot < k0; slot += RL_WAVES - solver_waves) load_pair(0, slot, lane);
    }
    __syncthreads();

    // ---- score: wave w takes whole hypotheses w, w + 12, ...
    for (int t = 0; t < ntiles; ++t) {
        const int kslots = tile_kslots(t);
        if (t > 0) {
            __syncthreads();
            for (int slot = wave; slot < kslots; slot += RL_WAVES) load_pair(t * tile_pts, slot, lane);
            __syncthreads();
        }
        for (int s = wave; s < hcount; s += 4 * RL_WAVES) {
            const int left = (hcount - s + RL_WAVES - 1) / RL_WAVES;
            if (left >= 4) score_h_lds<4>(s_mdl, s_cnt, s_pts + lane, kslots, s, thr2, lane);
            else if (left == 3) score_h_lds<3>(s_mdl, s_cnt, s_pts + lane, kslots, s, thr2, lane);
            else if (left == 2) score_h_lds<2>(s_mdl, s_cnt, s_pts + lane, kslots, s, thr2, lane);
            else score_h_lds<1>(s_mdl, s_cnt, s_pts + lane, kslots, s, thr2, lane);
        }
    }
    __syncthreads();

    // ---- the workgroup's best key (S22: most inliers, then lowest id) and its slot
    unsigned long long key = 0ull;
    if (tid < hcount && s_mdl[tid][9] != 0.f)
        key = (static_cast<unsigned long long>(static_cast<uint32_t>(s_cnt[tid])) << 32) |
              static_cast<unsigned long long>(0xFFFFFFFFu - static_cast<uint32_t>(hyp_begin + h0 + tid));
    const unsigned long long kbest = wg_max_u64<RL_WAVES>(key, s_wk, tid);
    if (wave == 0) {
        const int sb = kbest ? static_cast<int>(static_cast<int64_t>(0xFFFFFFFFu - static_cast<uint32_t>(kbest)) - hyp_begin) - h0 : 0;
        // slots as ten arrays of gridDim.x words (H[0] .. H[8], key)
        double* sf = reinterpret_cast<double*>(slots) + static_cast<size_t>(lane) * gridDim.x + blockIdx.x;
        if (lane < 9) __hip_atomic_store(sf, kbest ? s_m64[sb][lane] : 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (lane == 9) __hip_atomic_store(reinterpret_cast<unsigned long long*>(sf), kbest, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the slot is written through before the ticket is drawn
        if (lane == 0) {
            const int tk = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_role = tk == static_cast<int>(gridDim.x) - 1 ? 1 : 0;
        }
    }
    __syncthreads();
    if (s_role == 0) return;

    // ---- last workgroup: every slot is complete.  Winner = max key over the slots.
    if (tid == 0) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
    unsigned long long kb = 0ull;
    double hbst[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) hbst[i] = 0.0;
    for (int j = tid; j < static_cast<int>(gridDim.x); j += RL_THREADS) {
        const double* sf = reinterpret_cast<const double*>(slots) + j;
        const unsigned long long kj = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(sf + 9 * static_cast<size_t>(gridDim.x)),
                                                        __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        double hj[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) hj[i] = __hip_atomic_load(sf + i * static_cast<size_t>(gridDim.x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (kj > kb) {
            kb = kj;
#pragma unroll
            for (int i = 0; i < 9; ++i) hbst[i] = hj[i];
        }
    }
    const unsigned long long kwin = wg_max_u64<RL_WAVES>(kb, s_wk, tid);
    const bool ok = kwin != 0ull && n >= 4;
    if (tid < 9) s_H64[tid] = 0.0;
    __syncthreads();
    if (ok && kb == kwin) {                                  // exactly one thread: keys of distinct ids differ
#pragma unroll
        for (int i = 0; i < 9; ++i) s_H64[i] = hbst[i];
    }
    __syncthreads();
    if (tid < 9 && out.F) out.F[tid] = s_H64[tid];
    if (tid == 9) *out.key = ok ? kwin : 0ull;
    float hw[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) hw[i] = static_cast<float>(s_H64[i]);
    int mine = 0;
    for (int t = 0; t < ntiles; ++t) {
        const int kslots = tile_kslots(t);
        if (ntiles > 1) {                                    // (a single tile is still in LDS)
            __syncthreads();
            for (int slot = wave; slot < kslots; slot += RL_WAVES) load_pair(t * tile_pts, slot, lane);
            __syncthreads();
        }
        for (int slot = wave; slot < kslots; slot += RL_WAVES) {
            const f32x2* pp = s_pts + static_cast<size_t>(slot) * 256 + lane;
            bool ia, ib;
            inlier_h32_x2(hw, pp[0], pp[64], pp[128], pp[192], thr2, ia, ib);
            ia = ia && ok; ib = ib && ok;
            const int i0 = t * tile_pts + 2 * (64 * slot + lane);
            if (i0 < out.mask_len) out.mask[i0] = ia ? 1 : 0;
            if (i0 + 1 < out.mask_len) out.mask[i0 + 1] = ib ? 1 : 0;
            mine += __popcll(__ballot(ia)) + __popcll(__ballot(ib));     // wave-uniform
        }
    }
    if (lane == 0) s_wc[wave] = mine;
    const int covered = n > 0 ? (n + RL_SLOT_PTS - 1) / RL_SLOT_PTS * RL_SLOT_PTS : 0;
    for (int i = covered + tid; i < out.mask_len; i += RL_THREADS) out.mask[i] = 0;
    __syncthreads();
    if (tid == 0) {
        int tot = 0;
#pragma unroll
        for (int w = 0; w < RL_WAVES; ++w) tot += s_wc[w];
        if (out.n_inliers) *out.n_inliers = tot;
    }
}

int check_params_h(const pm_ransac_params* p)
{
    PM_REQUIRE(p != nullptr, PM_E_INVALID, "params is null");
    PM_REQUIRE(p->hyp_begin >= 0 && p->hyp_end > p->hyp_begin && p->hyp_end <= 0x100000000LL, PM_E_INVALID,
               "hypothesis ids must satisfy 0 <= begin < end <= 2^32");
    PM_REQUIRE(p->hyp_end - p->hyp_begin <= 0x7FFFFFFFLL, PM_E_INVALID,
               "a single launch takes at most 2^31 - 1 hypothesis ids: split the range");
    PM_REQUIRE(p->error_kind == PM_ERR_REPROJ, PM_E_INVALID, "error_kind must be PM_ERR_REPROJ");
    return PM_OK;
}

// Enqueue the one-launch run.  The arena must already be reserved for fused_scratch_bytes(); it is carved here.
int h_launch(pm_ctx* ctx, const pm_points_view& v, const pm_ransac_params* p, unsigned long long* d_key, double* d_H,
             uint8_t* d_mask, int mask_len, int* d_ninl)
{
    const long long nh = p->hyp_end - p->hyp_begin;
    const long long cap_total = static_cast<long long>(v.parts) * v.cap;
    const int hb = fused_hb(ctx, nh);
    const int nwg = static_cast<int>((nh + hb - 1) / hb);
    RfSlot* slots = static_cast<RfSlot*>(pm::arena_take(ctx, sizeof(RfSlot) * static_cast<size_t>(nwg)));
    PM_REQUIRE(slots, PM_E_NOMEM, "scratch arena too small");
    int* sync = nullptr;
    int rc = sync_words(ctx, &sync);
    if (rc != PM_OK) return rc;
    RfOut out{};
    out.key = d_key; out.F = d_H; out.mask = d_mask; out.mask_len = mask_len; out.n_inliers = d_ninl;
    const float thr2 = p->thresh_px * p->thresh_px;
    const long long need = (cap_total + RL_SLOT_PTS - 1) / RL_SLOT_PTS;
    const int tile_slots = static_cast<int>(need < 1 ? 1 : (need > RL_MAX_SLOTS ? RL_MAX_SLOTS : need));
    const size_t lds = static_cast<size_t>(tile_slots) * 4 * 64 * sizeof(f32x2);
    static bool attr_done_dev[PM_MAX_DEVICES] = {};
    if (!attr_done_dev[ctx->device]) {
        PM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&ransac_h_fused), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         RL_MAX_SLOTS * 4 * 64 * static_cast<int>(sizeof(f32x2))));
        attr_done_dev[ctx->device] = true;
    }
    pm::ScopedKernelTime t(ctx, "ransac_h_fused");
    hipLaunchKernelGGL(ransac_h_fused, dim3(nwg), dim3(RL_THREADS), lds, ctx->stream, v, p->seed, p->hyp_begin,
                       static_cast<int>(nh), hb, thr2, tile_slots, slots, sync + RH_SYNC_WORD, out);
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

// Host-pointer driver of pm_ransac_homography (range) and pm_ransac_homography_from_hyp (the range [hyp, hyp + 1)).
int host_run_h(pm_ctx* ctx, const float* xy1, const float* xy2, int n, const pm_ransac_params* p, double H[9],
               uint8_t* mask, int* n_inliers, uint64_t* best_key)
{
    if (H) for (int i = 0; i < 9; ++i) H[i] = 0.0;
    if (mask && n > 0) memset(mask, 0, static_cast<size_t>(n));
    if (n_inliers) *n_inliers = 0;
    if (best_key) *best_key = 0;
    int rc = check_params_h(p);
    if (rc != PM_OK) return rc;
    PM_REQUIRE(n >= 0 && (n == 0 || (xy1 && xy2)), PM_E_INVALID, "bad point arrays");
    if (n < 4) { pm::set_error("need at least 4 correspondences, got %d", n); return PM_E_TOO_FEW; }
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_HIP_CHECK(hipSetDevice(ctx->device));

    const size_t xyb = sizeof(float) * 2 * static_cast<size_t>(n);
    const size_t need = 2 * pm::align_up(xyb, 256) + pm::align_up(static_cast<size_t>(n), 256) + 3 * 256 +
                        fused_scratch_bytes(ctx, p) + 2048;
    rc = pm::arena_reserve(ctx, need);
    if (rc != PM_OK) return rc;
    pm::arena_reset(ctx);
    float* dxy1 = static_cast<float*>(pm::arena_take(ctx, xyb));
    float* dxy2 = static_cast<float*>(pm::arena_take(ctx, xyb));
    uint8_t* dmask = static_cast<uint8_t*>(pm::arena_take(ctx, static_cast<size_t>(n)));
    unsigned long long* dkey = static_cast<unsigned long long*>(pm::arena_take(ctx, 8));
    double* dH = static_cast<double*>(pm::arena_take(ctx, sizeof(double) * 9));
    int* dninl = static_cast<int*>(pm::arena_take(ctx, sizeof(int)));
    PM_REQUIRE(dxy1 && dxy2 && dmask && dkey && dH && dninl, PM_E_NOMEM, "scratch arena too small");
    constexpr size_t HP_MASK = 96;                           // pinned layout: key (8) | H (72) | count (4) | pad | mask
    rc = pm::pinned_reserve(ctx, HP_MASK + static_cast<size_t>(n));
    if (rc != PM_OK) return rc;

    PM_HIP_CHECK(hipMemcpyAsync(dxy1, xy1, xyb, hipMemcpyHostToDevice, ctx->stream));
    PM_HIP_CHECK(hipMemcpyAsync(dxy2, xy2, xyb, hipMemcpyHostToDevice, ctx->stream));
    const pm_points_view v{dxy1, dxy2, nullptr, 1, n, 0, 1, 0};
    rc = h_launch(ctx, v, p, dkey, dH, dmask, n, dninl);
    if (rc != PM_OK) return rc;
    char* hp = static_cast<char*>(ctx->pinned);
    unsigned long long* hkey = reinterpret_cast<unsigned long long*>(hp);
    double* hH = reinterpret_cast<double*>(hp + 8);
    int* hninl = reinterpret_cast<int*>(hp + 80);
    uint8_t* hmask = reinterpret_cast<uint8_t*>(hp + HP_MASK);
    PM_HIP_CHECK(hipMemcpyAsync(hkey, dkey, 8, hipMemcpyDeviceToHost, ctx->stream));
    PM_HIP_CHECK(hipMemcpyAsync(hH, dH, sizeof(double) * 9, hipMemcpyDeviceToHost, ctx->stream));
    PM_HIP_CHECK(hipMemcpyAsync(hninl, dninl, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    PM_HIP_CHECK(hipMemcpyAsync(hmask, dmask, static_cast<size_t>(n), hipMemcpyDeviceToHost, ctx->stream));
    PM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (best_key) *best_key = *hkey;
    if (*hkey == 0ull) {
        pm::set_error("no valid model (all hypotheses degenerate)");
        return PM_E_NO_MODEL;
    }
    if (H) memcpy(H, hH, sizeof(double) * 9);
    if (mask) memcpy(mask, hmask, static_cast<size_t>(n));
    if (n_inliers) *n_inliers = *hninl;
    return PM_OK;
}

}  // namespace

// for pm_ransac_homography_refined (homography_refine.hip): RANSAC-H and the refinement on one stream, one synchronisation
int ransac_h_check(const pm_ransac_params* p) { return check_params_h(p); }
int ransac_h_enqueue(pm_ctx* ctx, const pm_points_view& v, const pm_ransac_params* p, unsigned long long* d_key,
                     double* d_H, uint8_t* d_mask, int mask_len, int* d_ninl)
{
    return h_launch(ctx, v, p, d_key, d_H, d_mask, mask_len, d_ninl);
}
}  // namespace pm_ransac

using namespace pm_ransac;

extern "C" int pm_ransac_homography(pm_ctx* ctx, const float* xy1, const float* xy2, int n, const pm_ransac_params* p,
                                    double H[9], uint8_t* mask, int* n_inliers, uint64_t* best_key)
{
    return host_run_h(ctx, xy1, xy2, n, p, H, mask, n_inliers, best_key);
}

extern "C" int pm_ransac_homography_from_hyp(pm_ctx* ctx, const float* xy1, const float* xy2, int n,
                                             const pm_ransac_params* p, int64_t hyp, double H[9], uint8_t* mask,
                                             int* n_inliers)
{
    if (H) for (int i = 0; i < 9; ++i) H[i] = 0.0;
    if (n_inliers) *n_inliers = 0;
    PM_REQUIRE(hyp >= 0 && hyp < 0x100000000LL, PM_E_INVALID, "hypothesis id must satisfy 0 <= hyp < 2^32");
    PM_REQUIRE(p != nullptr, PM_E_INVALID, "params is null");
    pm_ransac_params q = *p;
    q.hyp_begin = hyp;
    q.hyp_end = hyp + 1;
    return host_run_h(ctx, xy1, xy2, n, &q, H, mask, n_inliers, nullptr);
}

extern "C" int pm_ransac_homography_run_dev(pm_ctx* ctx, const pm_points_view* view, const pm_ransac_params* p,
                                            uint64_t* d_best_key, double* d_H, uint8_t* d_mask, int mask_len,
                                            int32_t* d_n_inliers)
{
    PM_REQUIRE(d_best_key && d_H && d_mask && d_n_inliers, PM_E_INVALID, "null argument");
    PM_REQUIRE(mask_len >= 0, PM_E_INVALID, "mask_len must be >= 0");
    int rc = check_params_h(p);
    if (rc != PM_OK) return rc;
    rc = check_view(view);
    if (rc != PM_OK) return rc;
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    rc = pm::arena_reserve(ctx, fused_scratch_bytes(ctx, p) + 1024);
    if (rc != PM_OK) return rc;
    pm::arena_reset(ctx);
    return h_launch(ctx, *view, p, reinterpret_cast<unsigned long long*>(d_best_key), d_H, d_mask, mask_len, d_n_inliers);
}
