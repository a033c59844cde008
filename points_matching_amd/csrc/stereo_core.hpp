// stereo_core.hpp — what stereo.hip (S84-S88) and stereo_sgm.hip (S89-S92) share on the device, where A LANE OWNS A DISPARITY
// (lane + 64 c of register group c, NC groups): the read of one disparity's value and S85's winner.  Device code only; one copy
// for both files.
#pragma once
#include <cstdint>

#include "pm_common.hpp"

namespace stereo_core {

constexpr int INVALID = PM_STEREO_INVALID;
constexpr unsigned NO_KEY = 0xFFFFFFFFu;

// the value that the lane of disparity index k holds; k is wave-uniform
template <int NC>
__device__ __forceinline__ unsigned group_read(const unsigned (&v)[NC], int k)
{
    unsigned r = __builtin_amdgcn_readlane(v[0], k & 63);          // a lane read per group and scalar selects: no indexed array
#pragma unroll
    for (int c = 1; c < NC; ++c) {
        const unsigned t = __builtin_amdgcn_readlane(v[c], k & 63);
        r = (k >> 6) == c ? t : r;
    }
    return r;
}

// S85 on the costs C of one pixel (below 2^23; live[c]: the lane's disparity of group c is below D): the map value, which is
// INVALID when the uniqueness test rejects the pixel; no kept value equals INVALID (the smallest is 16 * (-1024) - 8).  `kept`
// says the same as value != INVALID: sgm_path counts n_valid with it, which keeps that kernel's instruction and scalar-register
// counts what they were with its own copy of this text (comparing the value changed both).
// The winner is one wave minimum of the key (cost << 9) | k, which is the lowest-d tie rule; c2 a second minimum over the
// disparities outside k1 +- 1; the parabola's neighbours two lane reads.  The result is wave-uniform; all 64 lanes must be
// active.  WAVE_MIN is the caller's reduction: stereo_bm and sgm_path each keep the one they were measured with.
struct Won {
    int value;
    bool kept;
};
template <unsigned (*WAVE_MIN)(unsigned), int NC>
__device__ __forceinline__ Won winner(const unsigned (&C)[NC], const bool (&live)[NC], int lane, int D, int dmin, int uniq)
{
    unsigned key = NO_KEY;
#pragma unroll
    for (int c = 0; c < NC; ++c)
        if (live[c]) key = min(key, (C[c] << 9) | static_cast<unsigned>(lane + 64 * c));
    key = WAVE_MIN(key);
    const int c1 = static_cast<int>(key >> 9), k1 = static_cast<int>(key & 511u);
    bool keep = true;
    if (uniq > 0) {
        unsigned second = NO_KEY;
#pragma unroll
        for (int c = 0; c < NC; ++c)
            if (live[c] && abs(lane + 64 * c - k1) > 1) second = min(second, C[c]);
        second = WAVE_MIN(second);
        if (second != NO_KEY && static_cast<int>(second) * (100 - uniq) < c1 * 100) keep = false;
    }
    int sub = 0;
    if (k1 > 0 && k1 < D - 1) {
        const int p = static_cast<int>(group_read<NC>(C, k1 - 1)), n = static_cast<int>(group_read<NC>(C, k1 + 1));
        const int den = p + n - 2 * c1;
        if (den != 0) {
            const int num = 16 * (p - n) + den, d2 = 2 * den;                    // den > 0: c1 is the minimum
            sub = num / d2;
            if (num < 0 && sub * d2 != num) --sub;                               // floor
        }
    }
    return {keep ? 16 * (dmin + k1) + sub : INVALID, keep};
}

}  // namespace stereo_core
