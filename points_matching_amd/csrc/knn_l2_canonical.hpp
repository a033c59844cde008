// knn_l2_canonical.hpp — what defines a result bit of the L2 matcher: the canonical squared distance (SPEC S1) and the
// ordering key (SPEC S3), seen once by the prep, refinement and exact kernels.  Private to knn_l2.hip (anonymous namespace:
// no other translation unit includes this header).
#pragma once
#include "knn_shared.hpp"
#include "wave_ops.hpp"

namespace {

using namespace pm_knn;

constexpr float KNN_INF = __builtin_inff();

__device__ __forceinline__ uint32_t f32_bits(float f) { return __float_as_uint(f); }

// SPEC S3 ordering key; NaN distances are canonicalised so they sort after +inf.
__device__ __forceinline__ uint64_t knn_key(float dist, int idx)
{
    uint32_t b = (dist != dist) ? 0x7FC00000u : f32_bits(dist);
    return (static_cast<uint64_t>(b) << 32) | static_cast<uint32_t>(idx);
}

// SPEC S1 — canonical squared distance: eight lane accumulators over 8-wide strides, unfused
// multiply and add, (acc[l]+acc[l+4]) lane-wise, ((s0+s1)+s2)+s3, scalar tail.  The TU is built
// with -ffp-contract=off, so none of these contract into v_fma/v_mac.
template <bool VEC4>
__device__ __forceinline__ float l2sqr_canonical(const float* __restrict__ a,
                                                 const float* __restrict__ b, int dim)
{
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int j = 0;
    if (VEC4) {
        for (; j + 8 <= dim; j += 8) {
            const f32x4 a0 = *reinterpret_cast<const f32x4*>(a + j);
            const f32x4 a1 = *reinterpret_cast<const f32x4*>(a + j + 4);
            const f32x4 b0 = *reinterpret_cast<const f32x4*>(b + j);
            const f32x4 b1 = *reinterpret_cast<const f32x4*>(b + j + 4);
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                float t = a0[l] - b0[l];
                float p = t * t;
                acc[l] = acc[l] + p;
                float u = a1[l] - b1[l];
                float w = u * u;
                acc[l + 4] = acc[l + 4] + w;
            }
        }
    } else {
        for (; j + 8 <= dim; j += 8) {
#pragma unroll
            for (int l = 0; l < 8; ++l) {
                float t = a[j + l] - b[j + l];
                float p = t * t;
                acc[l] = acc[l] + p;
            }
        }
    }
    const float s0 = acc[0] + acc[4], s1 = acc[1] + acc[5], s2 = acc[2] + acc[6],
                s3 = acc[3] + acc[7];
    float d = ((s0 + s1) + s2) + s3;
    for (; j < dim; ++j) {
        float t = a[j] - b[j];
        float p = t * t;
        d = d + p;
    }
    return d;
}

// the KM smallest (key, distance) pairs a lane has seen, ascending (refinement: KM = 2 for k <= 2, 4 for k <= 4; exact kernel:
// KL keys per pass)
template <int KM>
struct BestN {
    uint64_t k[KM];
    float d[KM];
    __device__ __forceinline__ void init()
    {
#pragma unroll
        for (int i = 0; i < KM; ++i) { k[i] = ~0ull; d[i] = KNN_INF; }
    }
    __device__ __forceinline__ void insert(uint64_t key, float dist)
    {
        if (key < k[KM - 1]) {
            k[KM - 1] = key; d[KM - 1] = dist;
#pragma unroll
            for (int i = KM - 1; i > 0; --i)
                if (k[i] < k[i - 1]) {
                    const uint64_t t = k[i]; k[i] = k[i - 1]; k[i - 1] = t;
                    const float u = d[i]; d[i] = d[i - 1]; d[i - 1] = u;
                }
        }
    }
    __device__ __forceinline__ void pop()
    {
#pragma unroll
        for (int i = 0; i + 1 < KM; ++i) { k[i] = k[i + 1]; d[i] = d[i + 1]; }
        k[KM - 1] = ~0ull; d[KM - 1] = KNN_INF;
    }
};

using pm::wave_min_f32;
using pm::wave_min_u64;

}  // namespace
