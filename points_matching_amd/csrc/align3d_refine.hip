// align3d_refine.hip — least-squares refit of a 3-D to 3-D transform x2 = s R x1 + t on its inliers in ONE launch on
// gfx950 (MI355X), docs/SPEC.md S101: Horn's closed-form absolute orientation (the unit quaternion that maximises
// q^T N q), with Umeyama's least-squares scale for the similarity.  The mask is not recomputed.  Also the two small
// kernels that close the device chain: pm_transform_points3[_dev] (a 13-double model applied to rows) and
// pm_gather_align3d_dev (compacted matches -> two row arrays).
//
// One workgroup of HR_P = 512 threads, thread p owning partial p of S23's fixed reduction order (refine_reduce.hpp), the
// way affine_refine.hip uses it.  Three passes over the usable inliers (mask[i] != 0 and six finite values), straight
// from global memory:
//   1. count, the six coordinate sums and the cost of T_in (8 sums);
//   2. the nine centred cross-moments sum b_c a_c^T and the two centred second moments (11 sums), then Horn's 4 x 4
//      matrix, its eigenvectors by cyclic Jacobi with a fixed sweep count, the quaternion's rotation, scale and
//      translation in every thread (every thread takes the same decisions);
//   3. the cost of the refit, which is kept only if it is not higher than T_in's.
// The launch keeps no per-call state, so the device form may be captured; the host forms (estimators.cpp)
// synchronise.
#include "align3d_core.hpp"
#include "ransac_fused_kernels.hpp"
#include "refine_reduce.hpp"

namespace pm_x3refine {
namespace {

using namespace pm_align3d;
using pm_hrefine::HR_P;
using pm_hrefine::tree;
using pm_ransac::view_count1;

constexpr int XR_SWEEPS = 10;            // S101: cyclic Jacobi sweeps over the 4 x 4 matrix, always all of them
constexpr double XR_GAP_REL = 1e-9;      // S101: the rotation is determined only if l1 - l2 > XR_GAP_REL * l1

struct Row {
    double a[3], b[3];
    bool ok;
};

// row i of the one-part view; ok: all six values finite
__device__ __forceinline__ Row row(const pm_points_view& v, int i)
{
    const float* p = v.xy1 + 3 * static_cast<size_t>(i);
    const float* q = v.xy2 + 3 * static_cast<size_t>(i);
    Row r;
    r.ok = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        r.a[c] = static_cast<double>(p[c]);
        r.b[c] = static_cast<double>(q[c]);
        r.ok = r.ok && fabs(r.a[c]) < __builtin_inf() && fabs(r.b[c]) < __builtin_inf();
    }
    return r;
}

// S101: the 12 doubles a cost pass uses, M = s R (each product once) and t
__device__ __forceinline__ void cost_model(const double (&T)[13], double (&M)[12])
{
#pragma unroll
    for (int i = 0; i < 9; ++i) M[i] = T[12] * T[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) M[9 + i] = T[9 + i];
}

// S101: squared residual of one correspondence under M
__device__ __forceinline__ double cost_term(const double (&M)[12], const Row& r)
{
    double e[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
        e[k] = (((M[3 * k] * r.a[0] + M[3 * k + 1] * r.a[1]) + M[3 * k + 2] * r.a[2]) + M[9 + k]) - r.b[k];
    return fma(e[0], e[0], fma(e[1], e[1], e[2] * e[2]));
}

// S101: one Jacobi rotation of the symmetric A (both triangles kept) in the (P, Q) plane, accumulated into V
template <int P, int Q>
__device__ __forceinline__ void jacobi_rot(double (&A)[4][4], double (&V)[4][4])
{
    const double apq = A[P][Q];
    if (apq == 0.0 || !(fabs(apq) < __builtin_inf())) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double akp = A[k][P], akq = A[k][Q];
        A[k][P] = c * akp - s * akq;
        A[k][Q] = s * akp + c * akq;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double apk = A[P][k], aqk = A[Q][k];
        A[P][k] = c * apk - s * aqk;
        A[Q][k] = s * apk + c * aqk;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double vkp = V[k][P], vkq = V[k][Q];
        V[k][P] = c * vkp - s * vkq;
        V[k][Q] = s * vkp + c * vkq;
    }
}

// S101 steps 3-6 on the moments S[3r + c] = sum b_r a_c, qa = sum |a_c|^2 and the centroids: T (13); false: not determined
template <int MODEL>
__device__ __forceinline__ bool horn(const double* S, double qa, const double (&ca)[3], const double (&cb)[3], double (&T)[13])
{
    // Horn's matrix, S_xy = sum a_x b_y = S[3 * 1 + 0]
    const double Sxx = S[0], Sxy = S[3], Sxz = S[6], Syx = S[1], Syy = S[4], Syz = S[7], Szx = S[2], Szy = S[5], Szz = S[8];
    double A[4][4], V[4][4];
    A[0][0] = (Sxx + Syy) + Szz; A[0][1] = Syz - Szy;         A[0][2] = Szx - Sxz;          A[0][3] = Sxy - Syx;
    A[1][1] = (Sxx - Syy) - Szz; A[1][2] = Sxy + Syx;         A[1][3] = Szx + Sxz;
    A[2][2] = (Syy - Sxx) - Szz; A[2][3] = Syz + Szy;
    A[3][3] = (Szz - Sxx) - Syy;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < i) A[i][j] = A[j][i];
            V[i][j] = i == j ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < XR_SWEEPS; ++sweep) {
        jacobi_rot<0, 1>(A, V); jacobi_rot<0, 2>(A, V); jacobi_rot<0, 3>(A, V);
        jacobi_rot<1, 2>(A, V); jacobi_rot<1, 3>(A, V); jacobi_rot<2, 3>(A, V);
    }
    // the largest eigenvalue (ties: lowest index) and the largest of the rest
    double l1 = A[0][0], q[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
    int k1 = 0;
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (A[k][k] > l1) {
            l1 = A[k][k]; k1 = k;
#pragma unroll
            for (int i = 0; i < 4; ++i) q[i] = V[i][k];
        }
    double l2 = -__builtin_inf();
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k != k1 && A[k][k] > l2) l2 = A[k][k];
    if (!(l1 > 0.0) || !(l1 < __builtin_inf()) || !(l1 - l2 > XR_GAP_REL * l1)) return false;
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double ww = w * w, xx = x * x, yy = y * y, zz = z * z;
    const double iq = 1.0 / (((ww + xx) + yy) + zz);
    T[0] = (((ww + xx) - yy) - zz) * iq; T[1] = (2.0 * (x * y - w * z)) * iq;  T[2] = (2.0 * (x * z + w * y)) * iq;
    T[3] = (2.0 * (x * y + w * z)) * iq;  T[4] = (((ww - xx) + yy) - zz) * iq; T[5] = (2.0 * (y * z - w * x)) * iq;
    T[6] = (2.0 * (x * z - w * y)) * iq;  T[7] = (2.0 * (y * z + w * x)) * iq;  T[8] = (((ww - xx) - yy) + zz) * iq;
    double s = 1.0;
    if constexpr (MODEL == SIMILARITY) {
        double num = 0.0;
#pragma unroll
        for (int i = 0; i < 9; ++i) num = num + T[i] * S[i];
        s = num / qa;
        if (!(s > 0.0) || !(s < __builtin_inf())) return false;
    }
    T[12] = s;
#pragma unroll
    for (int r = 0; r < 3; ++r) T[9 + r] = cb[r] - s * ((T[3 * r] * ca[0] + T[3 * r + 1] * ca[1]) + T[3 * r + 2] * ca[2]);
    bool fin = true;
#pragma unroll
    for (int i = 0; i < 13; ++i) fin = fin && fabs(T[i]) < __builtin_inf();
    return fin;
}

// v: one-part view, xy1 = rows of the first frame, xy2 = of the second (3 floats each)
template <int MODEL>
__global__ __launch_bounds__(HR_P) void align3d_refine(pm_points_view v, const uint8_t* mask, const double* T_in, double* T_out,
                                                       pm_h_refine_info* info)
{
    __shared__ double s_x[pm_hrefine::HR_CH][HR_P / 2];
    __shared__ double s_red[12];
    __shared__ double s_in[13];

    const int tid = threadIdx.x;
    const int n = view_count1(v);
    if (tid < 13) s_in[tid] = T_in[tid];     // read before any write: T_out may alias T_in
    __syncthreads();
    double in[13];
    bool zero = true;
#pragma unroll
    for (int i = 0; i < 13; ++i) { in[i] = s_in[i]; zero = zero && in[i] == 0.0; }
    if (zero) {                              // S101 status 2: no model
        if (tid == 0) {
#pragma unroll
            for (int i = 0; i < 13; ++i) T_out[i] = in[i];
            if (info) *info = pm_h_refine_info{0.0, 0.0, 0, 0, 2, 0};
        }
        return;
    }

    // ---- pass 1: usable inlier count, coordinate sums, cost of T_in
    double Min[12];
    cost_model(in, Min);
    {
        double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int i = tid; i < n; i += HR_P) {
            if (!mask[i]) continue;
            const Row r = row(v, i);
            if (!r.ok) continue;
            acc[0] = acc[0] + 1.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) { acc[1 + c] = acc[1 + c] + r.a[c]; acc[4 + c] = acc[4 + c] + r.b[c]; }
            acc[7] = acc[7] + cost_term(Min, r);
        }
        tree<8>(acc, tid, s_x, s_red);
    }
    const double nu = s_red[0], cost_in = s_red[7];
    double ca[3], cb[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { ca[c] = s_red[1 + c] / nu; cb[c] = s_red[4 + c] / nu; }
    __syncthreads();                         // s_red is read before pass 2 writes it

    // ---- pass 2: centred moments and the closed-form fit (every thread takes the same decisions)
    double ref[13];
#pragma unroll
    for (int i = 0; i < 13; ++i) ref[i] = 0.0;
    bool ok_ref = false;
    if (nu >= 3.0) {
        double acc[11];
#pragma unroll
        for (int k = 0; k < 11; ++k) acc[k] = 0.0;
        for (int i = tid; i < n; i += HR_P) {
            if (!mask[i]) continue;
            const Row r = row(v, i);
            if (!r.ok) continue;
            double da[3], db[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) { da[c] = r.a[c] - ca[c]; db[c] = r.b[c] - cb[c]; }
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[3 * k + c] = acc[3 * k + c] + db[k] * da[c];
            acc[9] = acc[9] + dot3(da, da);
            acc[10] = acc[10] + dot3(db, db);
        }
        tree<11>(acc, tid, s_x, s_red);
        double S[11];
#pragma unroll
        for (int k = 0; k < 11; ++k) S[k] = s_red[k];
        __syncthreads();
        ok_ref = horn<MODEL>(S, S[9], ca, cb, ref);
    }

    // ---- pass 3: cost of the refit; kept iff cost_ref <= cost_in (NaN: no)
    double cost_out = cost_in;
    bool accepted = false;
    if (ok_ref) {
        double Mref[12];
        cost_model(ref, Mref);
        double acc[1] = {0.0};
        for (int i = tid; i < n; i += HR_P) {
            if (!mask[i]) continue;
            const Row r = row(v, i);
            if (!r.ok) continue;
            acc[0] = acc[0] + cost_term(Mref, r);
        }
        tree<1>(acc, tid, s_x, s_red);
        const double cr = s_red[0];
        if (cr <= cost_in) { cost_out = cr; accepted = true; }
    }
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 13; ++i) T_out[i] = accepted ? ref[i] : in[i];
        if (info) *info = pm_h_refine_info{cost_in, cost_out, static_cast<int32_t>(nu), 0, accepted ? 0 : 1, 0};
    }
}

// S101 (points): row i < n = clamp(*d_n, 0, cap) under the 13-double model T, fp64, one rounding to fp32; a row with a
// non-finite input or result is three quiet NaNs.  out may be xyz: a thread reads its own row before it writes it.
__global__ __launch_bounds__(256) void transform_points3(const double* __restrict__ T, const float* xyz, const int32_t* d_n,
                                                         int cap, float* out)
{
    const int i = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    if (i >= pm::clamped_count(d_n, cap)) return;
    const double s = T[12];
    const float* p = xyz + 3 * static_cast<size_t>(i);
    const double x = static_cast<double>(p[0]), y = static_cast<double>(p[1]), z = static_cast<double>(p[2]);
    double o[3];
    bool fin = true;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        o[r] = (((s * T[3 * r]) * x + (s * T[3 * r + 1]) * y) + (s * T[3 * r + 2]) * z) + T[9 + r];
        fin = fin && fabs(o[r]) < __builtin_inf();
    }
    const float nanv = __builtin_nanf("");
    float* q = out + 3 * static_cast<size_t>(i);
#pragma unroll
    for (int r = 0; r < 3; ++r) q[r] = fin ? static_cast<float>(o[r]) : nanv;
}

// The device chain's gather: row i < n = clamp(*count, 0, cap) of the compacted match list gives
// xyz1[i] = tab1[queryIdx] and xyz2[i] = tab2[trainIdx]; an index out of range gives a NaN row (never an S99 inlier)
__global__ __launch_bounds__(256) void gather_align3d(const pm_match* __restrict__ m, const int32_t* __restrict__ count, int cap,
                                                      const float* __restrict__ tab1, int n1, const float* __restrict__ tab2,
                                                      int n2, float* __restrict__ xyz1, float* __restrict__ xyz2)
{
    const int n = pm::clamped_count(count, cap);
    const float nanv = __builtin_nanf("");
    for (int i = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x); i < n; i += static_cast<int>(gridDim.x) * 256) {
        const int q = m[i].queryIdx, t = m[i].trainIdx;
        float a[3] = {nanv, nanv, nanv}, b[3] = {nanv, nanv, nanv};
        if (q >= 0 && q < n1) {
            const float* o = tab1 + 3 * static_cast<size_t>(q);
            a[0] = o[0]; a[1] = o[1]; a[2] = o[2];
        }
        if (t >= 0 && t < n2) {
            const float* o = tab2 + 3 * static_cast<size_t>(t);
            b[0] = o[0]; b[1] = o[1]; b[2] = o[2];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            xyz1[3 * static_cast<size_t>(i) + c] = a[c];
            xyz2[3 * static_cast<size_t>(i) + c] = b[c];
        }
    }
}

}  // namespace
}  // namespace pm_x3refine

int pm_ransac::align3d_refine_enqueue(pm_ctx* ctx, int model, const pm_points_view& v, const uint8_t* d_mask,
                                      const double* d_T_in, double* d_T_out, pm_h_refine_info* d_info)
{
    using namespace pm_x3refine;
    pm::ScopedKernelTime t(ctx, "align3d_refine");
    if (model == PM_ALIGN3D_RIGID)
        hipLaunchKernelGGL(align3d_refine<RIGID>, dim3(1), dim3(HR_P), 0, ctx->stream, v, d_mask, d_T_in, d_T_out, d_info);
    else
        hipLaunchKernelGGL(align3d_refine<SIMILARITY>, dim3(1), dim3(HR_P), 0, ctx->stream, v, d_mask, d_T_in, d_T_out, d_info);
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

int pm_ransac::gather_align3d_enqueue(pm_ctx* ctx, const pm_match* d_m, const int32_t* d_count, int cap, const float* d_tab1,
                                      int n1, const float* d_tab2, int n2, float* d_xyz1, float* d_xyz2)
{
    using namespace pm_x3refine;
    const int nwg = (cap + 255) / 256 < 1024 ? (cap + 255) / 256 : 1024;
    pm::ScopedKernelTime t(ctx, "gather_align3d");
    hipLaunchKernelGGL(gather_align3d, dim3(nwg < 1 ? 1 : nwg), dim3(256), 0, ctx->stream, d_m, d_count, cap, d_tab1, n1, d_tab2,
                       n2, d_xyz1, d_xyz2);
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_transform_points3_dev(pm_ctx* ctx, const double* d_T, const float* d_xyz, const int32_t* d_n, int cap,
                                        float* d_out)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REQUIRE(d_T != nullptr && d_xyz != nullptr && d_out != nullptr, PM_E_INVALID, "null pointer");
    PM_REQUIRE(cap >= 0, PM_E_INVALID, "cap < 0");
    PM_REQUIRE(cap >= 1, PM_E_UNSUPPORTED, "cap == 0: nothing to transform");
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    {
        pm::ScopedKernelTime timer(ctx, "transform_points3");
        hipLaunchKernelGGL(pm_x3refine::transform_points3, dim3(static_cast<unsigned>((cap + 255) / 256)), dim3(256), 0, ctx->stream,
                           d_T, d_xyz, d_n, cap, d_out);
    }
    PM_HIP_CHECK(hipGetLastError());
    return PM_OK;
}

extern "C" int pm_transform_points3(pm_ctx* ctx, const double* T, const float* xyz, int n, float* out)
{
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_REQUIRE(T != nullptr && xyz != nullptr && out != nullptr, PM_E_INVALID, "null pointer");
    PM_REQUIRE(n >= 0, PM_E_INVALID, "n < 0");
    PM_REQUIRE(n >= 1, PM_E_UNSUPPORTED, "n == 0: nothing to transform");
    const size_t t_b = sizeof(double) * 13, xyz_b = static_cast<size_t>(n) * 12;
    pm::StagedBlock b(ctx, __func__);
    const size_t o_t = b.add(t_b), o_xyz = b.add(xyz_b);
    b.alloc();
    b.upload(o_t, T, t_b);
    b.upload(o_xyz, xyz, xyz_b);
    if (b.rc == PM_OK) b.rc = pm_transform_points3_dev(ctx, b.at<double>(o_t), b.at<float>(o_xyz), nullptr, n, b.at<float>(o_xyz));
    b.download(out, o_xyz, xyz_b);
    return b.sync();
}
