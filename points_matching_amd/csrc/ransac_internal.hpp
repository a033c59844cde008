// ransac_internal.hpp — entry points of ransac_fused.hip used by the C-ABI functions in ransac.hip (host-pointer
// and device-resident single-shard runs) and by the multi-GPU driver (mgpu.cpp), of ransac_h_fused.hip used by
// homography_refine.hip, and of the affine pair ransac_a_fused.hip / affine_refine.hip used by each other.
#pragma once
#include "ransac_core.hpp"

namespace pm_ransac {

constexpr int RF_HB_MAX = 128;          // hypothesis ids per workgroup, at most
int fused_hb(const pm_ctx* ctx, long long nh);
size_t fused_scratch_bytes(const pm_ctx* ctx, const pm_ransac_params* p);
int fused_launch(pm_ctx* ctx, const pm_points_view& v, const pm_ransac_params* p, int shard, pm_ransac_record* d_rec,
                 unsigned long long* d_key, double* d_F, uint8_t* d_mask, int mask_len, int* d_ninl, FinalOut** fo_out);

// Host side of the RANSAC-H launch (ransac_h_fused.hip), for pm_ransac_homography_refined: the argument check and the
// enqueue itself (no synchronisation; the arena must hold fused_scratch_bytes() more, as for pm_ransac_homography).
int ransac_h_check(const pm_ransac_params* p);
int ransac_h_enqueue(pm_ctx* ctx, const pm_points_view& v, const pm_ransac_params* p, unsigned long long* d_key,
                     double* d_H, uint8_t* d_mask, int mask_len, int* d_ninl);

// The affine family (ransac_a_fused.hip, affine_refine.hip): the model check and sample size every affine entry point
// uses (ransac_a_fused.hip), and the enqueue of the refit (affine_refine.hip; no synchronisation, no per-call state),
// which pm_estimate_affine runs after RANSAC-A on the same stream.
int ransac_a_check_model(int model);
int ransac_a_min_pts(int model);
int affine_refine_enqueue(pm_ctx* ctx, int model, const pm_points_view& v, const uint8_t* d_mask, const double* d_A_in,
                          double* d_A_out, pm_h_refine_info* d_info);

}  // namespace pm_ransac
