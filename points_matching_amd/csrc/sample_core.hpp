// sample_core.hpp — the minimal-sample draws of every robust estimator (docs/SPEC.md S6 and its per-family restatements
// S13, S19, S26, S32, S37, S97): mix64, RANSAC-F's sample8 and the draw-and-skip walk sample_walk<K, salts> that every
// other family calls with its own sample size and stream constants (named next to each family: homography_core.hpp,
// affine_core.hpp, essential_core.hpp, pnp_core.hpp, align3d_core.hpp, lmeds.hip).  Integer arithmetic only, and nothing
// but <cstdint>: the device units include it through ransac_core.hpp, and a plain host compiler can include it too
// (tests/sampler_shim.cpp checks every index against the CPU references without a GPU).
//
// Two shapes were tried and change the device code, so they are not used ("One sampler, one 3x4 base, one
// ticket table"): a per-family one-line wrapper around sample_walk, and a helper holding the loop that sample8's rare
// path and sample_walk have in common.  Call sample_walk directly; leave sample8's tail its own.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PM_SAMPLE_FN __host__ __device__ __forceinline__
#else
#define PM_SAMPLE_FN inline
#endif

namespace pm_ransac {

PM_SAMPLE_FN uint64_t mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// SPEC S6: 8 distinct indices in [0, n) as a pure function of (seed, h, n): draws d = 0, 1, ... give candidates
// c_d = floor(n * hi32(mix64(stream + (d+1)*phi)) / 2^32); a candidate equal to an earlier one is skipped; after 64
// draws the smallest unused integers complete the sample.  Same results as the sequential loop of the oracle, computed
// so that the 64-bit multiplies of the first eight draws are independent (they dominated: 5.3k of the solver's 24k
// cycles with the draw-by-draw loop) and the common case — eight distinct candidates — touches no select chains.
PM_SAMPLE_FN void sample8(uint64_t seed, uint64_t h, int n, int (&idx)[8])
{
    const uint64_t stream = mix64(seed ^ 0x9E3779B97F4A7C15ULL) ^ mix64(h + 0xD1B54A32D192ED03ULL);
    int cand[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        const uint64_t r = mix64(stream + static_cast<uint64_t>(d + 1) * 0x9E3779B97F4A7C15ULL);
        cand[d] = static_cast<int>(((r >> 32) * static_cast<uint64_t>(static_cast<uint32_t>(n))) >> 32);
    }
    unsigned dup = 0u;                         // bit d: candidate d repeats an earlier one (so it is skipped)
#pragma unroll
    for (int d = 1; d < 8; ++d)
#pragma unroll
        for (int e = 0; e < d; ++e) dup |= (cand[e] == cand[d] ? 1u : 0u) << d;
#pragma unroll
    for (int s = 0; s < 8; ++s) idx[s] = cand[s];
    if (dup == 0u) return;
    // rare: keep the first occurrences in draw order, then go on drawing
#pragma unroll
    for (int s = 0; s < 8; ++s) idx[s] = -1;
    int cnt = 0;
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        if (!((dup >> d) & 1u)) {
#pragma unroll
            for (int s = 0; s < 8; ++s)
                if (s == cnt) idx[s] = cand[d];
            ++cnt;
        }
    }
    for (uint64_t d = 8; d < 64 && cnt < 8; ++d) {
        const uint64_t r = mix64(stream + (d + 1) * 0x9E3779B97F4A7C15ULL);
        const int c = static_cast<int>(((r >> 32) * static_cast<uint64_t>(static_cast<uint32_t>(n))) >> 32);
        bool rep = false;
#pragma unroll
        for (int s = 0; s < 8; ++s) rep |= (s < cnt) && (idx[s] == c);
        if (!rep) {
#pragma unroll
            for (int s = 0; s < 8; ++s)
                if (s == cnt) idx[s] = c;
            ++cnt;
        }
    }
    for (int c = 0; cnt < 8; ++c) {
        bool rep = false;
#pragma unroll
        for (int s = 0; s < 8; ++s) rep |= (s < cnt) && (idx[s] == c);
        if (!rep) {
#pragma unroll
            for (int s = 0; s < 8; ++s)
                if (s == cnt) idx[s] = c;
            ++cnt;
        }
    }
}

// S6's walk for the other families: K distinct indices in [0, n), n >= K, as a pure function of (seed, h, n) on the
// stream mix64(seed ^ SEED_SALT) ^ mix64(h + H_SALT), draw by draw.
template <int K, uint64_t SEED_SALT, uint64_t H_SALT = 0xD1B54A32D192ED03ULL>
PM_SAMPLE_FN void sample_walk(uint64_t seed, uint64_t h, int n, int (&idx)[K])
{
    const uint64_t stream = mix64(seed ^ SEED_SALT) ^ mix64(h + H_SALT);
#pragma unroll
    for (int s = 0; s < K; ++s) idx[s] = -1;
    int cnt = 0;
    for (uint64_t d = 0; d < 64 && cnt < K; ++d) {
        const uint64_t r = mix64(stream + (d + 1) * 0x9E3779B97F4A7C15ULL);
        const int c = static_cast<int>(((r >> 32) * static_cast<uint64_t>(static_cast<uint32_t>(n))) >> 32);
        bool rep = false;
#pragma unroll
        for (int s = 0; s < K; ++s) rep |= (s < cnt) && (idx[s] == c);
        if (!rep) {
#pragma unroll
            for (int s = 0; s < K; ++s)
                if (s == cnt) idx[s] = c;
            ++cnt;
        }
    }
    for (int c = 0; cnt < K; ++c) {
        bool rep = false;
#pragma unroll
        for (int s = 0; s < K; ++s) rep |= (s < cnt) && (idx[s] == c);
        if (!rep) {
#pragma unroll
            for (int s = 0; s < K; ++s)
                if (s == cnt) idx[s] = c;
            ++cnt;
        }
    }
}

}  // namespace pm_ransac
