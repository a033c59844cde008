// C face of the minimal-sample draws (csrc/sample_core.hpp) for tests/test_sampler_cpu.py, built with the host compiler
// alone: sample8 and sample_walk at every family's sample size and stream constants.  The constants are restated here
// from docs/SPEC.md (S13, S19, S26, S32, S37, S97); the test also reads the named constants next to each family in csrc/
// and compares them with sampler_salt().
#include <cstdint>

#include "sample_core.hpp"

namespace {

constexpr int FAMILIES = 8;      // F, LMedS, H, A-full, A-partial, E, PnP, 3-D alignment
constexpr int SIZE[FAMILIES] = {8, 7, 4, 3, 2, 5, 3, 3};
constexpr uint64_t H_SALT = 0xD1B54A32D192ED03ULL;
constexpr uint64_t SALT[FAMILIES][2] = {
    {0x9E3779B97F4A7C15ULL, H_SALT}, {0x7F4A7C159E3779B9ULL, H_SALT}, {0x4A7C159E3779B97FULL, H_SALT},
    {0x79B97F4A7C159E37ULL, H_SALT}, {0x7C159E3779B97F4AULL, H_SALT}, {0xC2B2AE3D27D4EB4FULL, H_SALT},
    {0x165667B19E3779F9ULL, H_SALT}, {0x3C6EF372FE94F82BULL, 0xA54FF53A5F1D36F1ULL}};

template <int F>
void one(uint64_t seed, uint64_t h, int n, int32_t* out)
{
    int idx[SIZE[F]];
    if constexpr (F == 0) pm_ransac::sample8(seed, h, n, idx);
    else pm_ransac::sample_walk<SIZE[F], SALT[F][0], SALT[F][1]>(seed, h, n, idx);
    for (int s = 0; s < SIZE[F]; ++s) out[s] = idx[s];
}

template <int F>
void many(uint64_t seed, const uint64_t* h, int count, int n, int32_t* out)
{
    for (int i = 0; i < count; ++i) one<F>(seed, h[i], n, out + static_cast<int64_t>(SIZE[F]) * i);
}

}  // namespace

extern "C" int sampler_size(int family) { return family >= 0 && family < FAMILIES ? SIZE[family] : -1; }

extern "C" uint64_t sampler_salt(int family, int which) { return SALT[family][which]; }

// out[SIZE * i ..] = the sample of (seed, h[i], n), n >= SIZE; returns SIZE, or -1 for an unknown family
extern "C" int sampler_batch(int family, uint64_t seed, const uint64_t* h, int count, int n, int32_t* out)
{
    switch (family) {
    case 0: many<0>(seed, h, count, n, out); break;
    case 1: many<1>(seed, h, count, n, out); break;
    case 2: many<2>(seed, h, count, n, out); break;
    case 3: many<3>(seed, h, count, n, out); break;
    case 4: many<4>(seed, h, count, n, out); break;
    case 5: many<5>(seed, h, count, n, out); break;
    case 6: many<6>(seed, h, count, n, out); break;
    case 7: many<7>(seed, h, count, n, out); break;
    default: return -1;
    }
    return SIZE[family];
}
