// knn_l2.hip — brute-force L2 k-NN over float descriptors on gfx950 (MI355X).
//
// Replaces `matcher.match(imageDesc1, imageDesc2, matchePoints, Mat())` (main.cpp:46) with the
// BruteForceMatcher<L2<float>> of main.cpp:43, generalised to k-NN.  The RESULT is defined by
// docs/SPEC.md S1/S3: distance = sqrtf(canonical sum of squared differences), order =
// (distance bits, trainIdx).  How it is computed here:
//
//   knn_l2_prep    row norms ||q||^2, ||t||^2 (+ max train norm, non-finite flag)
//   knn_l2_mfma    COARSE pass on the matrix cores: v_mfma_f32_32x32x2_f32 accumulates q.t over
//                  D; s = ||t||^2 - 2 q.t ranks the train rows of a query up to a proven error
//                  eps.  Train rows ride the MFMA M dimension and queries the N dimension, so a
//                  lane owns ONE query column and keeps its 4 smallest s (value, index) in
//                  registers for the whole sweep: no cross-lane traffic in the loop.
//   knn_l2_refine  per query: tau = k-th smallest coarse value; every slot within
//                  (tau+eps)(1+2^-20)+eps is re-evaluated in the canonical op order on the VALU
//                  and the k smallest canonical keys are emitted.  A sub-list whose 4th entry
//                  is still inside the window may have dropped a candidate: that query is
//                  re-scanned exactly (rare; always correct).
//   knn_l2_exact   general kernel (any dim, k <= 16): canonical distances for every pair on the
//                  VALU out of LDS tiles.  Also the `PM_KNN_FORCE_EXACT` path.
//
// Both routes are bit-identical by construction (tests/test_knn_l2_gpu.py asserts it).
//
// The kernels are filed by stage in headers private to this translation unit: knn_l2_prep.hpp (the prep kernels),
// knn_l2_refine.hpp (both refinement kernels and the fused tail), knn_l2_exact.hpp (the exact kernel), over
// knn_l2_canonical.hpp (SPEC S1 distance and S3 key).  This file keeps the launch half: plan -> launches, and the C ABI.
#include <cstdlib>
#include <type_traits>

#include "image_args.hpp"
#include "knn_l2_exact.hpp"
#include "knn_l2_plan.hpp"
#include "knn_l2_prep.hpp"
#include "knn_l2_refine.hpp"

namespace {

using namespace pm_knn;

// u8 route: ratio test + compaction + gather inside the refinement launch?  A kernel boundary costs about what the in-launch
// look-back behind the slowest workgroup costs, so from 1024 queries up the two forms measure the same (call, us, two launches
// / fused: 1024^2 14.95 / 14.83, 2048^2 16.3 / 16.2, 8192^2 26.5 / 26.1) and the separate launch stays the default; up to 512
// queries (<= 32 workgroups, one look-back hop) the fused form is 1.6-1.8 us shorter (512^2 15.1 / 13.3, 128^2 14.1 / 12.4;
// tools/small_fusion.py) and is the default.  PM_OPT_FILTER_FUSION pins either form.
constexpr int PM_U8_FUSED_MAX_NQ = 768;
__host__ inline bool u8_fused_by_default(int nq) { return nq <= PM_U8_FUSED_MAX_NQ; }

int run_exact(pm_ctx* ctx, const float* dq, int nq, const float* dt, int nt, int dim, int k, pm_match* dout)
{
    if (nq == 0) return PM_OK;
    PM_REQUIRE(dout != nullptr, PM_E_INVALID, "this shape takes the exact kernel, which needs the k-NN record buffer (d_knn)");
    dim3 grid((nq + EXQ_WG - 1) / EXQ_WG);
    pm::ScopedKernelTime t(ctx, "knn_l2_exact");
    if (k == 1)
        hipLaunchKernelGGL(knn_l2_exact<1>, grid, dim3(256), 0, ctx->stream, dq, dt, nq, nt, dim, k, dout);
    else if (k == 2)
        hipLaunchKernelGGL(knn_l2_exact<2>, grid, dim3(256), 0, ctx->stream, dq, dt, nq, nt, dim, k, dout);
    else
        hipLaunchKernelGGL(knn_l2_exact<4>, grid, dim3(256), 0, ctx->stream, dq, dt, nq, nt, dim, k, dout);
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

// per-context words of the fused compaction: arrival word + epoch-tagged survivor count per 32-query tile
int kf_prepare(pm_ctx* ctx, int nq, KnnFuse& fz, int queries_per_tile = 32)
{
    const int tiles = (nq + queries_per_tile - 1) / queries_per_tile;
    if (tiles > ctx->kf_cap) {
        PM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (ctx->kf_tile) PM_HIP_CHECK(hipFree(ctx->kf_tile));
        ctx->kf_tile = nullptr;
        ctx->kf_cap = 0;
        const int cap = tiles < 4096 ? 4096 : tiles + tiles / 2;
        PM_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&ctx->kf_tile), static_cast<size_t>(cap) * 12));
        PM_HIP_CHECK(hipMemsetAsync(ctx->kf_tile, 0, static_cast<size_t>(cap) * 12, ctx->stream));
        ctx->kf_cap = cap;
        ctx->kf_epoch = 0;
    }
    if (++ctx->kf_epoch >= (1u << 24)) {          // 24-bit tag: restart
        PM_HIP_CHECK(hipMemsetAsync(ctx->kf_tile, 0, static_cast<size_t>(ctx->kf_cap) * 12, ctx->stream));
        ctx->kf_epoch = 1;
    }
    fz.tile = ctx->kf_tile;
    fz.tilecnt = reinterpret_cast<unsigned*>(ctx->kf_tile + ctx->kf_cap);
    fz.err = reinterpret_cast<unsigned*>(ctx->knn_stats) + 12;      // byte 48 of the side-band block
    fz.epoch = ctx->kf_epoch;
    return PM_OK;
}

KnnL2Request knn_l2_request(const pm_ctx* ctx, const void* q, const void* t, bool u8_rows, int nq, int nt, int dim, int k, int flags,
                            bool fuse)
{
    KnnL2Request r{};
    r.nq = nq; r.nt = nt; r.dim = dim; r.k = k; r.flags = flags; r.n_cu = ctx->n_cu;
    std::memcpy(r.opts, ctx->opts, sizeof(r.opts));
    r.u8_rows = u8_rows;
    r.aligned = ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(t)) & (u8_rows ? 3 : 15)) == 0;
    r.fuse = fuse;
    return r;
}

KnnGeom knn_geom(const KnnGeomPlan& g, const float* cand)
{
    return KnnGeom{cand, g.slots, g.tiles_per_split, g.rows_per_tile, g.lid_mask, g.eps_coef, g.embed_coef, g.eps_coef_gen,
                   g.abs_gen, g.int_shift};
}

// A plan value -> a template argument: f(std::integral_constant<V>) for the V of the list that equals v (the last one
// when none does, like the `default:` of a switch).  Every V of the list is instantiated.  v is compared as the list's type:
// pick<true, false> takes any non-zero v for true.
template <auto V, auto... Rest, typename T, typename F>
inline void pick(T v, F&& f)
{
    if constexpr (sizeof...(Rest) == 0) f(std::integral_constant<decltype(V), V>{});
    else if (static_cast<decltype(V)>(v) == V) f(std::integral_constant<decltype(V), V>{});
    else pick<Rest...>(v, f);
}

// The launch half of the matcher: obeys a KNN_MATRIX plan (knn_l2_plan.hpp) and decides nothing.  `fuse` (the plan was made
// with fuse = true): ratio test + compaction + gather ride the refinement launch.  uq / ut != null: the rows are u8
// (dq / dt are not read in that mode).  The arena is carved per call; callers that interleave calls on one context are
// serialised by the stream.
int knn_l2_enqueue(pm_ctx* ctx, const KnnL2Plan& p, const float* dq, int nq, const float* dt, int nt, int dim, int k,
                   pm_match* dout, const KnnFuse* fuse, const uint8_t* uq = nullptr, const uint8_t* ut = nullptr)
{
    PM_REFUSE_CAPTURE(ctx);
    int rc = pm::arena_reserve(ctx, p.need);
    if (rc != PM_OK) return rc;
    pm::arena_reset(ctx);
    float* qnorm = static_cast<float*>(pm::arena_take(ctx, p.qnorm_bytes));
    float* tnorm = static_cast<float*>(pm::arena_take(ctx, p.tnorm_bytes));
    float* cval32 = p.want32 ? static_cast<float*>(pm::arena_take(ctx, p.c32)) : nullptr;
    float* cval16 = p.want16 ? static_cast<float*>(pm::arena_take(ctx, p.c16)) : nullptr;
    _Float16* Qh = p.want16 ? static_cast<_Float16*>(pm::arena_take(ctx, p.qh)) : nullptr;
    _Float16* Th = p.want16 ? static_cast<_Float16*>(pm::arena_take(ctx, p.th)) : nullptr;
    void* seeds = p.sdb ? pm::arena_take(ctx, p.sdb) : nullptr;
    void* Qf = p.qfb ? pm::arena_take(ctx, p.qfb) : nullptr;
    PM_REQUIRE(qnorm && tnorm && (!p.want32 || cval32) && (!p.want16 || (cval16 && Qh && Th)) && (!p.sdb || seeds) && (!p.qfb || Qf),
               PM_E_NOMEM, "scratch arena too small");
    KnnFuse fz{};
    if (fuse) {
        fz = *fuse;
        fz.pk = static_cast<unsigned long long*>(pm::arena_take(ctx, p.pkb));
        PM_REQUIRE(fz.pk != nullptr, PM_E_NOMEM, "scratch arena too small");
        rc = kf_prepare(ctx, nq, fz, p.kf_tile);
        if (rc != PM_OK) return rc;
    }
    const KnnGeom g32 = knn_geom(p.g32, cval32), g16 = knn_geom(p.g16, cval16);

    unsigned long long* stats = ctx->knn_stats;          // persistent, epoch-tagged: never cleared
    if (++ctx->knn_epoch == 0u) {              // 2^32 calls: restart the epoch tags
        PM_HIP_CHECK(hipMemsetAsync(stats, 0, 32, ctx->stream));
        ctx->knn_epoch = 1u;
    }
    const unsigned epoch = ctx->knn_epoch;
    unsigned* diag = nullptr;
    if (ctx->knn_diag) {
        diag = ctx->knn_diag_words;
        PM_HIP_CHECK(hipMemsetAsync(diag, 0, 12, ctx->stream));
    }
    const int nq_pad = p.nq_pad, nt_pad = p.nt_pad, t_wide = p.t_wide, route = p.route;
    {
        pm::ScopedKernelTime t(ctx, "knn_l2_prep");
        const dim3 grid(p.prep_grid);
        uint2 *Q8 = reinterpret_cast<uint2*>(Qh), *T8 = reinterpret_cast<uint2*>(Th), *Qf2 = static_cast<uint2*>(Qf);
        // the f16 family's <DP, ALIGNED> from the plan
        auto dp_al = [&](auto&& launch) {
            pick<128, 256>(p.dp16, [&](auto DP) { pick<true, false>(p.vec, [&](auto AL) { launch(DP, AL); }); });
        };
        auto prep8 = [&](auto IT) {
            pick<true, false>(dim == U8_DP, [&](auto FULL) {
                hipLaunchKernelGGL((knn_l2_prep8<IT, FULL>), grid, dim3(256), 0, ctx->stream, dq, nq, nq_pad, dt, nt, nt_pad, dim, qnorm,
                                   tnorm, Q8, T8, static_cast<int*>(seeds), stats, epoch, t_wide, Qf2);
            });
        };
        switch (p.prep) {
        case KNN_PREP_U8ROWS:
            hipLaunchKernelGGL(knn_l2_prep8_u8, grid, dim3(256), 0, ctx->stream, uq, nq, nq_pad, ut, nt, nt_pad, dim, qnorm, tnorm,
                               Q8, T8, static_cast<int*>(seeds), t_wide, Qf2);
            break;
        case KNN_PREP8_16: prep8(std::integral_constant<int, 1>{}); break;
        case KNN_PREP8_32: prep8(std::integral_constant<int, 2>{}); break;
        case KNN_PREP8_64: prep8(std::integral_constant<int, 4>{}); break;
        case KNN_PREP16_SEEDED:
            hipLaunchKernelGGL((knn_l2_prep16<true, 128, true>), grid, dim3(256), 0, ctx->stream, dq, nq, nq_pad, dt, nt, nt_pad, dim,
                               qnorm, tnorm, Qh, Th, static_cast<float*>(seeds), stats, epoch);
            break;
        case KNN_PREP16_UNIT:
            dp_al([&](auto DP, auto AL) {
                hipLaunchKernelGGL((knn_l2_prep16u<DP, AL>), grid, dim3(256), 0, ctx->stream, dq, nq, nq_pad, dt, nt, nt_pad, dim, qnorm,
                                   tnorm, Qh, Th, stats, epoch);
            });
            break;
        case KNN_PREP16:
            dp_al([&](auto DP, auto AL) {
                hipLaunchKernelGGL((knn_l2_prep16<false, DP, AL>), grid, dim3(256), 0, ctx->stream, dq, nq, nq_pad, dt, nt, nt_pad, dim,
                                   qnorm, tnorm, Qh, Th, nullptr, stats, epoch);
            });
            break;
        default:
            hipLaunchKernelGGL(knn_l2_prep, grid, dim3(256), 0, ctx->stream, dq, nq, dt, nt, dim, qnorm, tnorm, stats, epoch);
            break;
        }
        if (p.prep_gen == KNN_GEN_PREP16G)
            dp_al([&](auto DP, auto AL) {
                hipLaunchKernelGGL((knn_l2_prep16g<DP, AL>), grid, dim3(256), 0, ctx->stream, dq, nq, nq_pad, dt, nt, nt_pad, dim, qnorm,
                                   tnorm, Qh, Th, stats, epoch);
            });
        else if (p.prep_gen == KNN_GEN_OFF) hipLaunchKernelGGL(knn_gen_off, dim3(1), dim3(64), 0, ctx->stream, stats, epoch);
        PM_HIP_CHECK(hipGetLastError());
    }
    if (route == ROUTE_U8_HINT) {
        rc = launch_coarse_u8(ctx, Qh, Qf, Th, static_cast<const int*>(seeds), nq, nq_pad, nt, p.splits16, g16.tiles_per_split,
                              reinterpret_cast<int*>(cval16), g16.slots, p.u8_group, p.u8_form);
        if (rc != PM_OK) return rc;
    } else if (p.f16s) {
        rc = launch_coarse_f16s(ctx, Qh, Th, static_cast<const float*>(seeds), nq, nq_pad, nt, p.splits16, g16.tiles_per_split,
                                ~g16.lid_mask, cval16, g16.slots);
        if (rc != PM_OK) return rc;
    } else if (p.want16) {
        rc = launch_coarse_f16(ctx, Qh, Th, nq, nq_pad, nt, p.splits16, g16.tiles_per_split, ~g16.lid_mask, cval16,
                               g16.slots, stats, epoch, route == ROUTE_AUTO ? 1 : 0, p.dp16);
        if (rc != PM_OK) return rc;
    }
    if (p.want32) {
        rc = launch_coarse_f32(ctx, dq, nq, dt, nt, dim, tnorm, p.splits32, g32.tiles_per_split, ~g32.lid_mask, cval32,
                               g32.slots, stats, epoch, route == ROUTE_AUTO ? 1 : 0);
        if (rc != PM_OK) return rc;
    }
    pm::ScopedKernelTime t(ctx, "knn_l2_refine");
    // (a fused tail never rides a KM == 4 instantiation of either kernel)
    if (p.refine8) {
        // 0: the fused tail (two neighbours per lane), else KM = 2 or 4 neighbours per lane
        const int tail = p.refine_fuse ? 0 : p.refine_km;
        pick<1, 2, 4, 8, 16>(p.refine_ns, [&](auto NS) { pick<4, 8, 16>(p.refine_group, [&](auto GROUP) { pick<0, 2, 4>(tail, [&](auto TAIL) {
            hipLaunchKernelGGL((knn_l2_refine8<NS, GROUP, TAIL == 4 ? 4 : 2, TAIL == 0>), dim3((nq + 15) / 16), dim3(256), 0, ctx->stream,
                               dq, dt, reinterpret_cast<const uint4*>(Qh), reinterpret_cast<const uint4*>(Th), qnorm, tnorm,
                               reinterpret_cast<const int*>(cval16), stats, epoch, diag, nq, nt, dim, k, g16.slots, g16.tiles_per_split,
                               dout, fz, t_wide ? U8_WIDE_ROW16 : U8_ROW16);
        }); }); });
    } else {
        pick<1, 2, 4, 8>(p.refine_ns, [&](auto NS) { pick<true, false>(p.refine_fuse, [&](auto FUSE) { pick<true, false>(p.refine_gen, [&](auto GEN) {
            pick<true, false>(p.refine_vec, [&](auto VEC) { pick<2, 4>(p.refine_km, [&](auto KM) {
                hipLaunchKernelGGL((knn_l2_refine<VEC, NS, FUSE && KM == 2, GEN, KM>), dim3((nq + 3) / 4), dim3(256), 0, ctx->stream,
                                   dq, dt, qnorm, stats, epoch, diag, nq, nt, dim, k, g16, g32, route, dout, fz);
            }); });
        }); }); });
    }
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

// Plan and run one matcher call.  *verdict tells the caller what happened: KNN_MATRIX — done, fused tail included;
// KNN_EXACT — the exact kernel wrote dout, and a caller that wanted the fused tail still has to filter; KNN_WIDEN (u8 rows
// only) — nothing ran: the shape needs the f32 matcher on widened copies.
int knn_l2_run(pm_ctx* ctx, const float* dq, int nq, const float* dt, int nt, int dim, int k, int flags, pm_match* dout,
               const KnnFuse* fuse, int* verdict, const uint8_t* uq = nullptr, const uint8_t* ut = nullptr)
{
    const bool u8 = uq != nullptr;
    const KnnL2Plan p = knn_l2_plan(knn_l2_request(ctx, u8 ? static_cast<const void*>(uq) : dq, u8 ? static_cast<const void*>(ut) : dt, u8,
                                                   nq, nt, dim, k, flags, fuse != nullptr));
    *verdict = p.verdict;
    if (p.verdict == KNN_EXACT) return run_exact(ctx, dq, nq, dt, nt, dim, k, dout);
    if (p.verdict == KNN_WIDEN) return PM_OK;
    return knn_l2_enqueue(ctx, p, dq, nq, dt, nt, dim, k, dout, fuse, uq, ut);
}

// What the k-NN forms of pm_bf_knn_l2_* require of their arguments (rows on the host or the device, f32 or u8), and what
// the ratio forms require after their own null-argument check (the f32 form also checks the train pointer).
using ArgCheck = pm_image::Check;        // a status and a message, which PM_REQUIRE_PASS reports under the caller's name
ArgCheck knn_args(const pm_ctx* ctx, const void* q, int nq, const void* t, int nt, int dim, int k, const void* out)
{
    if (ctx == nullptr) return {PM_E_INVALID, "ctx is null"};
    if (!(nq >= 0 && nt >= 0 && dim >= 1 && k >= 1 && k <= PM_MAX_K)) return {PM_E_INVALID, "need nq,nt >= 0, dim >= 1, 1 <= k <= PM_MAX_K"};
    if (!(nq == 0 || (q && out))) return {PM_E_INVALID, "null query/output pointer"};
    if (!(nt == 0 || t)) return {PM_E_INVALID, "null train pointer"};
    return {};
}

ArgCheck ratio_args(const void* q, int nq, const void* t, bool check_t, int nt, int dim, const void* good, const void* kp1,
                           const void* kp2, const void* xy1, const void* xy2)
{
    if (!(nq >= 0 && nt >= 0 && dim >= 1)) return {PM_E_INVALID, "need nq,nt >= 0, dim >= 1"};
    if (!(nq == 0 || (q && good))) return {PM_E_INVALID, "null query/output pointer"};
    if (check_t && !(nt == 0 || t)) return {PM_E_INVALID, "null train pointer"};
    if ((kp1 == nullptr) != (kp2 == nullptr)) return {PM_E_INVALID, "give both keypoint arrays or none"};
    if (!(kp1 == nullptr || (xy1 && xy2))) return {PM_E_INVALID, "null point outputs"};
    return {};
}

}  // namespace

extern "C" int pm_bf_knn_l2_f32_dev(pm_ctx* ctx, const float* dq, int nq, const float* dt, int nt, int dim,
                                    int k, int flags, pm_match* dout)
{
    PM_REQUIRE_PASS(knn_args(ctx, dq, nq, dt, nt, dim, k, dout));
    if (nq == 0) return PM_OK;
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    PM_REFUSE_CAPTURE(ctx);
    int verdict;
    return knn_l2_run(ctx, dq, nq, dt, nt, dim, k, flags, dout, nullptr, &verdict);
}

// main.cpp:46 + :49-69 (ratio form) + :77-78 + :89-91 in one call: 2-NN, ratio test, stable compaction and keypoint
// gather, as the matcher launches followed by the filter launch, or (no record buffer given, or PM_OPT_FILTER_FUSION
// = 2) with the last three riding the refinement launch.  Same outputs either way.
extern "C" int pm_bf_knn_l2_ratio_dev(pm_ctx* ctx, const float* d_q, int nq, const float* d_t, int nt, int dim, int flags,
                                      float ratio, const float* d_kp1_xy, const float* d_kp2_xy, pm_match* d_knn,
                                      pm_match* d_good, float* d_xy1, float* d_xy2, int32_t* d_n_good)
{
    PM_REQUIRE(ctx != nullptr && d_n_good != nullptr, PM_E_INVALID, "null argument");
    PM_REQUIRE_PASS(ratio_args(d_q, nq, d_t, true, nt, dim, d_good, d_kp1_xy, d_kp2_xy, d_xy1, d_xy2));
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    PM_REFUSE_CAPTURE(ctx);
    if (nq == 0) {
        PM_HIP_CHECK(hipMemsetAsync(d_n_good, 0, sizeof(int32_t), ctx->stream));
        return PM_OK;
    }
    KnnFuse fz{};
    fz.ratio = ratio; fz.kp1 = d_kp1_xy; fz.kp2 = d_kp2_xy; fz.good = d_good; fz.xy1 = d_xy1; fz.xy2 = d_xy2; fz.n_out = d_n_good;
    // Measured at C3 (8192 queries): refinement 10.0 us + filter launch 6.4 us against 19.8 us for the fused launch — the
    // in-launch hand-off (write-through store, drain, arrival atomic, look-back, dependent loads) costs about what the
    // launch boundary it replaces costs, and it lengthens every workgroup.  So the two-launch form is the default
    // whenever the caller provides the record buffer; PM_OPT_FILTER_FUSION = 2 selects the fused launch, 1 the two launches.
    // u8 route (PM_KNN_HINT_U8): its refinement holds 16 whole queries per workgroup, so the fused tail is one count per
    // workgroup and a look-back — PM_OPT_FILTER_FUSION = 0 takes the form that measured faster there.
    const int fusion = ctx->opts[PM_OPT_FILTER_FUSION];
    const bool u8_hint = (flags & PM_KNN_HINT_U8) && !(flags & (PM_KNN_FORCE_F32 | PM_KNN_FORCE_EXACT));
    const bool separate = fusion == 1 || (fusion == 0 && d_knn != nullptr && !(u8_hint && u8_fused_by_default(nq)));
    int rc, verdict;
    if (!separate) {
        rc = knn_l2_run(ctx, d_q, nq, d_t, nt, dim, 2, flags, d_knn, &fz, &verdict);
        if (rc != PM_OK || verdict == KNN_MATRIX) return rc;         // failed, or done (fused)
        // the exact kernel ran (shape outside the MFMA routes) into d_knn; the filter follows as its own launch
        return pm_filter_ratio_gather_dev(ctx, d_knn, nq, 2, ratio, d_kp1_xy, d_kp2_xy, d_good, d_xy1, d_xy2, d_n_good);
    }
    PM_REQUIRE(d_knn != nullptr, PM_E_INVALID, "the two-launch form needs d_knn");
    rc = knn_l2_run(ctx, d_q, nq, d_t, nt, dim, 2, flags, d_knn, nullptr, &verdict);
    if (rc != PM_OK) return rc;
    return pm_filter_ratio_gather_dev(ctx, d_knn, nq, 2, ratio, d_kp1_xy, d_kp2_xy, d_good, d_xy1, d_xy2, d_n_good);
}

// ---- u8 descriptor rows (pm_bf_knn_l2_u8*): the u8 route with nothing to convert but one XOR; other shapes go through
// the f32 matcher on widened copies.  Result = pm_bf_knn_l2_f32 on the same values, bit for bit.
namespace {
int u8_widened(pm_ctx* ctx, const uint8_t* dq, int nq, const uint8_t* dt, int nt, int dim, const float** fq, const float** ft)
{
    const size_t a = pm::align_up(static_cast<size_t>(nq) * dim, 64), b = static_cast<size_t>(nt) * dim;
    if ((a + b) * sizeof(float) > ctx->widen_cap) {
        PM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (ctx->widen) PM_HIP_CHECK(hipFree(ctx->widen));
        ctx->widen = nullptr;
        ctx->widen_cap = 0;
        const size_t cap = pm::align_up((a + b) * sizeof(float) * 5 / 4, size_t(1) << 20);
        PM_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&ctx->widen), cap));
        ctx->widen_cap = cap;
    }
    if (static_cast<size_t>(nq) * dim)
        hipLaunchKernelGGL(knn_u8_widen, dim3(256), dim3(256), 0, ctx->stream, dq, static_cast<size_t>(nq) * dim, ctx->widen);
    if (b) hipLaunchKernelGGL(knn_u8_widen, dim3(256), dim3(256), 0, ctx->stream, dt, b, ctx->widen + a);
    PM_HIP_CHECK(hipGetLastError());
    *fq = ctx->widen;
    *ft = ctx->widen + a;
    return PM_OK;
}
}  // namespace

extern "C" int pm_bf_knn_l2_u8_dev(pm_ctx* ctx, const uint8_t* dq, int nq, const uint8_t* dt, int nt, int dim, int k,
                                   pm_match* dout)
{
    PM_REQUIRE_PASS(knn_args(ctx, dq, nq, dt, nt, dim, k, dout));
    if (nq == 0) return PM_OK;
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    PM_REFUSE_CAPTURE(ctx);
    int verdict;
    int rc = knn_l2_run(ctx, nullptr, nq, nullptr, nt, dim, k, 0, dout, nullptr, &verdict, dq, dt);
    if (rc != PM_OK || verdict != KNN_WIDEN) return rc;
    const float *fq = nullptr, *ft = nullptr;
    rc = u8_widened(ctx, dq, nq, dt, nt, dim, &fq, &ft);
    if (rc != PM_OK) return rc;
    return knn_l2_run(ctx, fq, nq, ft, nt, dim, k, PM_KNN_HINT_INTEGER, dout, nullptr, &verdict);
}

extern "C" int pm_bf_knn_l2_u8_ratio_dev(pm_ctx* ctx, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int dim, float ratio,
                                         const float* d_kp1_xy, const float* d_kp2_xy, pm_match* d_knn, pm_match* d_good,
                                         float* d_xy1, float* d_xy2, int32_t* d_n_good)
{
    PM_REQUIRE(ctx != nullptr && d_n_good != nullptr && d_knn != nullptr, PM_E_INVALID, "null argument (the u8 form needs the record buffer)");
    PM_REQUIRE_PASS(ratio_args(d_q, nq, d_t, false, nt, dim, d_good, d_kp1_xy, d_kp2_xy, d_xy1, d_xy2));
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    PM_REFUSE_CAPTURE(ctx);
    if (nq == 0) {
        PM_HIP_CHECK(hipMemsetAsync(d_n_good, 0, sizeof(int32_t), ctx->stream));
        return PM_OK;
    }
    const int fusion = ctx->opts[PM_OPT_FILTER_FUSION];
    if (fusion == 2 || (fusion == 0 && u8_fused_by_default(nq))) {
        KnnFuse fz{};
        fz.ratio = ratio; fz.kp1 = d_kp1_xy; fz.kp2 = d_kp2_xy; fz.good = d_good; fz.xy1 = d_xy1; fz.xy2 = d_xy2; fz.n_out = d_n_good;
        int verdict;
        const int rf = knn_l2_run(ctx, nullptr, nq, nullptr, nt, dim, 2, 0, d_knn, &fz, &verdict, d_q, d_t);
        if (rf != PM_OK || verdict != KNN_WIDEN) return rf;  // failed, or done (fused); else a shape for the widened f32 path
    }
    const int rc = pm_bf_knn_l2_u8_dev(ctx, d_q, nq, d_t, nt, dim, 2, d_knn);
    if (rc != PM_OK) return rc;
    return pm_filter_ratio_gather_dev(ctx, d_knn, nq, 2, ratio, d_kp1_xy, d_kp2_xy, d_good, d_xy1, d_xy2, d_n_good);
}

extern "C" int pm_bf_knn_l2_u8(pm_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, int dim, int k, pm_match* out)
{
    PM_REQUIRE_PASS(knn_args(ctx, q, nq, t, nt, dim, k, out));
    if (nq == 0) return PM_OK;
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    return pm::StagedBlock::knn(ctx, __func__, q, static_cast<size_t>(nq) * dim, t, static_cast<size_t>(nt) * dim, out,
                                  sizeof(pm_match) * static_cast<size_t>(nq) * k, [&](void* dq, void* dt, void* dout) {
        return pm_bf_knn_l2_u8_dev(ctx, static_cast<const uint8_t*>(dq), nq, static_cast<const uint8_t*>(dt), nt, dim, k,
                                   static_cast<pm_match*>(dout));
    });
}

extern "C" int pm_bf_knn_l2_f32(pm_ctx* ctx, const float* q, int nq, const float* t, int nt, int dim, int k,
                                int flags, pm_match* out)
{
    PM_REQUIRE_PASS(knn_args(ctx, q, nq, t, nt, dim, k, out));
    if (nq == 0) return PM_OK;
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    return pm::StagedBlock::knn(ctx, __func__, q, sizeof(float) * static_cast<size_t>(nq) * dim, t, sizeof(float) * static_cast<size_t>(nt) * dim,
                                  out, sizeof(pm_match) * static_cast<size_t>(nq) * k, [&](void* dq, void* dt, void* dout) {
        return pm_bf_knn_l2_f32_dev(ctx, static_cast<const float*>(dq), nq, static_cast<const float*>(dt), nt, dim, k, flags,
                                    static_cast<pm_match*>(dout));
    });
}
