// ransac_internal.hpp — host functions shared across translation units: the entry points of ransac_fused.hip used by
// the C-ABI functions in ransac.hip (host-pointer and device-resident single-shard runs) and by the multi-GPU driver
// (mgpu.cpp), the view check of every device-resident entry point, the table of arrival words, and the one enqueue of
// each kernel file that estimators.cpp drives: homography (ransac_h_fused.hip, homography_refine.hip), affine
// (ransac_a_fused.hip, affine_refine.hip), calibrated relative pose (essential_solve.hip, ransac_e_fused.hip,
// recover_pose.hip), the two-view refinements (fundamental_refine.hip, pose_refine.hip), absolute pose (pnp_solve.hip,
// ransac_p_fused.hip, pnp_refine.hip) and 3-D alignment (align3d_solve.hip, ransac_align3d_fused.hip, align3d_refine.hip).
#pragma once
#include "ransac_core.hpp"

namespace pm_ransac {

// The arrival words in ctx->sync_words (pm_common.hpp), one entry per launch that draws tickets.  An entry owns the word
// it names and the next one (the finish kernel counts inliers there); every launch returns its words to zero.  Families
// may follow one another on one context and stream, so no two entries may meet.
enum SyncWord : int {
    SYNC_F = 0,                 // ransac_fused, ransac_fused_lds<FModel>
    SYNC_F_FINISH = 2,          // ransac_finish (ransac_shard.hip)
    SYNC_H = 8,
    SYNC_A = 12,
    SYNC_E = 16,
    SYNC_P = 20,
    SYNC_X = 24,                // 3-D alignment
};
constexpr bool sync_words_ok()
{
    constexpr int w[] = {SYNC_F, SYNC_F_FINISH, SYNC_H, SYNC_A, SYNC_E, SYNC_P, SYNC_X};
    constexpr int n = sizeof w / sizeof w[0], words = static_cast<int>(pm::SYNC_WORDS_BYTES / sizeof(int));
    for (int i = 0; i < n; ++i) {
        if (w[i] < 0 || w[i] + 2 > words) return false;
        for (int j = 0; j < i; ++j)
            if (w[i] - w[j] < 2 && w[j] - w[i] < 2) return false;
    }
    return true;
}
static_assert(sync_words_ok(), "two arrival-word entries overlap, or one lies outside ctx->sync_words");

constexpr int RF_HB_MAX = 128;          // hypothesis ids per workgroup, at most
int fused_hb(const pm_ctx* ctx, long long nh);
size_t fused_scratch_bytes(const pm_ctx* ctx, const pm_ransac_params* p);
int fused_launch(pm_ctx* ctx, const pm_points_view& v, const pm_ransac_params* p, int shard, pm_ransac_record* d_rec,
                 unsigned long long* d_key, double* d_F, uint8_t* d_mask, int mask_len, int* d_ninl, FinalOut** fo_out);

inline int check_view(const pm_points_view* v)
{
    PM_REQUIRE(v != nullptr && v->xy1 && v->xy2, PM_E_INVALID, "null correspondence view");
    PM_REQUIRE(v->parts >= 1 && v->parts <= PM_MAX_PARTS && v->cap >= 1, PM_E_INVALID, "need 1 <= parts <= 64, cap >= 1");
    PM_REQUIRE(v->parts == 1 || (v->pitch_xy >= 2LL * v->cap), PM_E_INVALID, "pitch_xy smaller than a part");
    PM_REQUIRE(static_cast<long long>(v->parts) * v->cap <= 0x7FFFFFFFLL, PM_E_INVALID, "view too large");
    return PM_OK;
}

// The launches below are each enqueued on ctx->stream with no synchronisation and no argument check.
// Homography and affine.  The RANSAC pair carves its workgroup slots from the arena, which must hold
// fused_scratch_bytes() more; model is PM_AFFINE_FULL or PM_AFFINE_PARTIAL.
int ransac_h_enqueue(pm_ctx* ctx, const pm_points_view& v, const pm_ransac_params* p, unsigned long long* d_key,
                     double* d_H, uint8_t* d_mask, int mask_len, int* d_ninl);
int ransac_a_enqueue(pm_ctx* ctx, int model, const pm_points_view& v, const pm_ransac_params* p, unsigned long long* d_key,
                     double* d_A, uint8_t* d_mask, int mask_len, int* d_ninl);
int homography_refine_enqueue(pm_ctx* ctx, const pm_points_view& v, const uint8_t* d_mask, const double* d_H_in,
                              int max_iters, double* d_H_out, pm_h_refine_info* d_info);
int affine_refine_enqueue(pm_ctx* ctx, int model, const pm_points_view& v, const uint8_t* d_mask, const double* d_A_in,
                          double* d_A_out, pm_h_refine_info* d_info);

// Calibrated relative pose.  essential_solve_enqueue normalises the view by K into d_xyn (two arrays of 2 * parts * cap
// floats) with its count in *d_n, and solves samples [hyp_begin, hyp_end) of p into d_cand (100 doubles per sample);
// ransac_e_enqueue scores model ids [q->hyp_begin, q->hyp_end) (10 per sample, d_cand at the first) on the normalised
// view vn, q->thresh_px being the normalised threshold (carves its slots like ransac_h_enqueue); recover_pose_enqueue
// is one workgroup over the raw view.
int essential_solve_enqueue(pm_ctx* ctx, const pm_points_view& v, const pm_camera& K, const pm_ransac_params* p, float* d_xyn,
                            int* d_n, double* d_cand);
int ransac_e_enqueue(pm_ctx* ctx, const pm_points_view& vn, const pm_ransac_params* q, const double* d_cand,
                     unsigned long long* d_key, double* d_E, uint8_t* d_mask, int mask_len, int* d_ninl);
int recover_pose_enqueue(pm_ctx* ctx, const pm_points_view& v, const pm_camera& K, const double* d_E, const uint8_t* d_mask_in,
                         double dist, double* d_R, double* d_t, uint8_t* d_mask_out, int mask_len, int* d_n_good,
                         float* d_points4);

// Refinement of the fundamental matrix (S43-S45) and of a relative pose (S46-S47) on their inliers: one workgroup each
// over the raw view; d_E_out (the E of the refined pose) may be null.
int fundamental_refine_enqueue(pm_ctx* ctx, const pm_points_view& v, const uint8_t* d_mask, const double* d_F_in,
                               int max_iters, double* d_F_out, pm_h_refine_info* d_info);
int pose_refine_enqueue(pm_ctx* ctx, const pm_points_view& v, const pm_camera& K, const uint8_t* d_mask,
                        const double* d_Rt_in, int max_iters, double* d_Rt_out, double* d_E_out, pm_h_refine_info* d_info);

// Absolute pose.  pnp_solve_enqueue solves samples [hyp_begin, hyp_end) of p into d_cand (80 doubles per sample) from the
// one-part view v (xy1 = world points, 3 floats each; xy2 = pixels); ransac_p_enqueue scores model ids [q->hyp_begin,
// q->hyp_end) (4 per sample, d_cand at the first) over the same view (carves its slots like ransac_h_enqueue).
int pnp_solve_enqueue(pm_ctx* ctx, const pm_points_view& v, const pm_camera& K, const pm_ransac_params* p, double* d_cand);
int ransac_p_enqueue(pm_ctx* ctx, const pm_points_view& v, const pm_ransac_params* q, const double* d_cand,
                     unsigned long long* d_key, double* d_Rt, uint8_t* d_mask, int mask_len, int* d_ninl);
// pnp_refine_enqueue: S40 on the same view, one workgroup; gather_pnp_enqueue: the device chain's match -> row gather.
int pnp_refine_enqueue(pm_ctx* ctx, const pm_points_view& v, const pm_camera& K, const uint8_t* d_mask, const double* d_Rt_in,
                       int max_iters, double* d_Rt_out, pm_h_refine_info* d_info);
int gather_pnp_enqueue(pm_ctx* ctx, const pm_match* d_m, const int32_t* d_count, int cap, const float* d_kp_xy, int n_kp,
                       const float* d_obj, int n_obj, float* d_uv, float* d_xyz);

// 3-D to 3-D alignment (S97-S101); model is PM_ALIGN3D_RIGID or PM_ALIGN3D_SIMILARITY.  align3d_solve_enqueue solves
// samples [hyp_begin, hyp_end) of p into d_cand (20 doubles per sample) from the one-part view v (xy1, xy2: the rows of
// the two frames, 3 floats each); ransac_align3d_enqueue scores model ids [q->hyp_begin, q->hyp_end) (one per sample,
// d_cand at the first) over the same view (carves its slots like ransac_h_enqueue); align3d_refine_enqueue: S101 on the
// same view, one workgroup; gather_align3d_enqueue: the device chain's match -> two row arrays.
int align3d_solve_enqueue(pm_ctx* ctx, int model, const pm_points_view& v, const pm_ransac_params* p, double* d_cand);
int ransac_align3d_enqueue(pm_ctx* ctx, const pm_points_view& v, const pm_ransac_params* q, const double* d_cand,
                           unsigned long long* d_key, double* d_T, uint8_t* d_mask, int mask_len, int* d_ninl);
int align3d_refine_enqueue(pm_ctx* ctx, int model, const pm_points_view& v, const uint8_t* d_mask, const double* d_T_in,
                           double* d_T_out, pm_h_refine_info* d_info);
int gather_align3d_enqueue(pm_ctx* ctx, const pm_match* d_m, const int32_t* d_count, int cap, const float* d_tab1, int n1,
                           const float* d_tab2, int n2, float* d_xyz1, float* d_xyz2);

}  // namespace pm_ransac
