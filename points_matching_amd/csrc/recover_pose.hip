// recover_pose.hip — pose recovery from an essential matrix on gfx950 (MI355X), one launch of one workgroup
// (docs/SPEC.md S35; OpenCV's recoverPose structure [recalled]):
//   * thread 0 decomposes E (one-sided Jacobi) into the candidates (R1,t) (R2,t) (R1,-t) (R2,-t) and leaves them in LDS;
//   * every thread triangulates its masked correspondences against the four candidates (linear DLT, 4 x 4 Jacobi),
//     applies the cheirality tests and keeps the four verdicts as bits in its own mask bytes; the integer counts meet
//     in LDS (any order);
//   * thread 0 picks the candidate with OpenCV's >= chain and publishes R, t and the count; every thread then turns its
//     bytes into the chosen candidate's mask and (optionally) writes its triangulated points.
// It reads the view and E on the device, so it chains after RANSAC-E with no host round trip.
#include "essential_core.hpp"
#include "ransac_fused_kernels.hpp"

namespace pm_ransac {
namespace {

using namespace pm_essential;

constexpr int RP_THREADS = 512;

// candidate c of the four: R1 or R2 (c odd), t or -t (c >= 2)
__device__ __forceinline__ void load_pose(const double* __restrict__ s_ps, int c, double (&R)[9], double (&t)[3])
{
    const double* r = s_ps + ((c & 1) ? 9 : 0);
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = r[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = c < 2 ? s_ps[18 + i] : -s_ps[18 + i];
}

__global__ __launch_bounds__(RP_THREADS) void recover_pose_kernel(pm_points_view v, Cam k, const double* __restrict__ dE,
                                                                  const uint8_t* __restrict__ mask_in, double dist,
                                                                  double* __restrict__ R_out, double* __restrict__ t_out,
                                                                  uint8_t* mask_out, int mask_len, int* __restrict__ n_good,
                                                                  float* __restrict__ points4)
{
    __shared__ int s_offs[PM_MAX_PARTS + 1];
    __shared__ double s_ps[21];                         // R1, R2, t
    __shared__ int s_ok, s_pick;
    __shared__ int s_cnt[4];
    const int tid = threadIdx.x;
    int n;
    if (v.parts == 1) {
        n = view_count1(v);
    } else {
        view_offsets(v, s_offs, tid);
        __syncthreads();
        n = s_offs[v.parts];
    }
    if (tid == 0) {
        double E[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) E[i] = dE[i];
        Poses ps;
        const bool ok = decompose(E, ps);
#pragma unroll
        for (int i = 0; i < 9; ++i) { s_ps[i] = ps.R1[i]; s_ps[9 + i] = ps.R2[i]; }
#pragma unroll
        for (int i = 0; i < 3; ++i) s_ps[18 + i] = ps.t[i];
        s_ok = ok ? 1 : 0;
    }
    if (tid < 4) s_cnt[tid] = 0;
    __syncthreads();
    if (!s_ok) {                                        // E does not decompose: R = 0, t = 0, nothing passes
        if (tid < 9) R_out[tid] = 0.0;
        if (tid < 3) t_out[tid] = 0.0;
        if (tid == 0) *n_good = 0;
        for (int i = tid; i < mask_len; i += RP_THREADS) mask_out[i] = 0;
        if (points4)
            for (int i = tid; i < 4 * n; i += RP_THREADS) points4[i] = 0.f;
        return;
    }
    int cnt[4] = {0, 0, 0, 0};
    for (int i = tid; i < n; i += RP_THREADS) {
        unsigned bits = 0u;
        if (!mask_in || mask_in[i]) {
            float2 a, b;
            view_point(v, s_offs, i, a, b);
            a = normalise(k, a);
            b = normalise(k, b);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                double R[9], t[3], Q[4];
                load_pose(s_ps, c, R, t);
                triangulate(R, t, a.x, a.y, b.x, b.y, Q);
                if (cheiral(R, t, Q, dist)) { bits |= 1u << c; ++cnt[c]; }
            }
        }
        mask_out[i] = static_cast<uint8_t>(bits);       // the four verdicts until the choice (this thread's bytes only)
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (cnt[c]) atomicAdd(&s_cnt[c], cnt[c]);
    __syncthreads();
    if (tid == 0) {
        const int g0 = s_cnt[0], g1 = s_cnt[1], g2 = s_cnt[2], g3 = s_cnt[3];
        int c;
        if (g0 >= g1 && g0 >= g2 && g0 >= g3) c = 0;
        else if (g1 >= g0 && g1 >= g2 && g1 >= g3) c = 1;
        else if (g2 >= g0 && g2 >= g1 && g2 >= g3) c = 2;
        else c = 3;
        s_pick = c;
        double R[9], t[3];
        load_pose(s_ps, c, R, t);
#pragma unroll
        for (int i = 0; i < 9; ++i) R_out[i] = R[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) t_out[i] = t[i];
        *n_good = s_cnt[c];
    }
    __syncthreads();
    const int c = s_pick;
    double R[9], t[3];
    load_pose(s_ps, c, R, t);
    for (int i = tid; i < n; i += RP_THREADS) {
        mask_out[i] = static_cast<uint8_t>((mask_out[i] >> c) & 1u);
        if (points4) {
            float2 a, b;
            view_point(v, s_offs, i, a, b);
            a = normalise(k, a);
            b = normalise(k, b);
            double Q[4];
            triangulate(R, t, a.x, a.y, b.x, b.y, Q);
            *reinterpret_cast<float4*>(points4 + 4 * static_cast<size_t>(i)) =
                float4{static_cast<float>(Q[0]), static_cast<float>(Q[1]), static_cast<float>(Q[2]), static_cast<float>(Q[3])};
        }
    }
    for (int i = n + tid; i < mask_len; i += RP_THREADS) mask_out[i] = 0;
}

}  // namespace

int recover_pose_enqueue(pm_ctx* ctx, const pm_points_view& v, const pm_camera& K, const double* d_E, const uint8_t* d_mask_in,
                         double dist, double* d_R, double* d_t, uint8_t* d_mask_out, int mask_len, int* d_n_good,
                         float* d_points4)
{
    pm::ScopedKernelTime t(ctx, "recover_pose");
    hipLaunchKernelGGL(recover_pose_kernel, dim3(1), dim3(RP_THREADS), 0, ctx->stream, v, Cam{K.fx, K.fy, K.cx, K.cy}, d_E,
                       d_mask_in, dist, d_R, d_t, d_mask_out, mask_len, d_n_good, d_points4);
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

}  // namespace pm_ransac
