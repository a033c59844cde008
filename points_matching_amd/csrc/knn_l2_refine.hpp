// knn_l2_refine.hpp — the refinement kernels of the L2 matcher (knn_l2_refine: canonical f32 re-evaluation, one wave per
// query; knn_l2_refine8: integer re-evaluation on the u8 route's byte copies, four queries per wave) and the fused tail both
// share (ratio test + stable compaction + keypoint gather in the refinement launch).  Private to knn_l2.hip, which holds the
// scheme and the launcher (anonymous namespace: no other translation unit includes this header).
#pragma once
#include "knn_l2_prep.hpp"          // query_scale / train_half_exp: the SAME functions as in the general-float prep

namespace {

using namespace pm_knn;

// ---------------------------------------------------------------------------------------------
// refinement: one wave per query
// ---------------------------------------------------------------------------------------------
// the KM smallest coarse values of a lane's slots (for the k-th smallest over the wave / row; BestN: knn_l2_canonical.hpp)
template <typename V, int KM>
struct MinN {
    V m[KM];
    __device__ __forceinline__ void init(V big)
    {
#pragma unroll
        for (int i = 0; i < KM; ++i) m[i] = big;
    }
    __device__ __forceinline__ void insert(V v)
    {
        if (v < m[KM - 1]) {
            m[KM - 1] = v;
#pragma unroll
            for (int i = KM - 1; i > 0; --i)
                if (m[i] < m[i - 1]) { const V t = m[i]; m[i] = m[i - 1]; m[i - 1] = t; }
        }
    }
    __device__ __forceinline__ void pop(V big)
    {
#pragma unroll
        for (int i = 0; i + 1 < KM; ++i) m[i] = m[i + 1];
        m[KM - 1] = big;
    }
};

// Candidate-list geometry of one coarse route (how a slot index and the embedded row id map back
// to a train row, and how wide the refinement window must be).
struct KnnGeom {
    const float* cand;        // [nq][slots]
    int slots;                // splits * KNN_C
    int tiles_per_split;
    int rows_per_tile;        // 64 (f32 route) or 128 (f16 route); ids per tile = rows/2
    unsigned lid_mask;
    float eps_coef;           // fp error of the coarse value, times (||q||^2 + max||t||^2)
    float embed_coef;         // truncation by the embedded id, times (||q||^2 + 2 max||t||^2)
    float eps_coef_gen;       // f16 route on general floats: rounding of the copies, same factor (SPEC S1c)
    float abs_gen;            // ... plus this many units of the SCALED accumulator (flushed subnormals, seed rounding)
    int int_shift;            // u8 route: candidates are ints (w << int_shift) | id and qnorm holds ||q - 128||^2; else 0
};

// position of the r-th (0-based) set bit of m; r < popcount(m)
__device__ __forceinline__ int nth_set_bit(unsigned long long m, int r)
{
    int pos = 0;
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) {
        const int c = __popcll((m >> pos) & ((1ull << w) - 1ull));
        if (r >= c) { r -= c; pos += w; }
    }
    return pos;
}

// SPEC S1 evaluated by 8 consecutive lanes: lane l (0..7) of the group IS accumulator l of the
// canonical form (same products, same order), the combine uses the canonical association.  The
// 16 loads per operand of a lane are independent, so one candidate costs about one memory round
// trip instead of dim/8 dependent ones.  Result valid in the group's lane 0.
__device__ __forceinline__ float l2sqr_canonical_coop8(const float* __restrict__ a, const float* __restrict__ b,
                                                       int dim, int l)
{
    float acc = 0.f;
    const int full8 = dim & ~7;
    int j0 = 0;
    // Blocks of 16 (then 8) column groups with NO per-element condition: all loads of a block are
    // issued before the first subtraction.  (A guarded or clamped element makes hipcc wait for
    // every pair of loads in turn: 16 dependent memory round trips per candidate.)
    for (; j0 + 128 <= full8; j0 += 128) {
        float av[16], bv[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) { av[u] = a[j0 + 8 * u + l]; bv[u] = b[j0 + 8 * u + l]; }
#pragma unroll
        for (int u = 0; u < 16; ++u) { const float t = av[u] - bv[u]; const float p = t * t; acc = acc + p; }
    }
    for (; j0 + 64 <= full8; j0 += 64) {
        float av[8], bv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { av[u] = a[j0 + 8 * u + l]; bv[u] = b[j0 + 8 * u + l]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) { const float t = av[u] - bv[u]; const float p = t * t; acc = acc + p; }
    }
    for (; j0 < full8; j0 += 8) {
        const float t = a[j0 + l] - b[j0 + l];
        const float p = t * t;
        acc = acc + p;
    }
    float d = pm::coop8_combine(acc);                        // meaningful in lane 0
    for (int j = full8; j < dim; ++j) {
        const float t = a[j] - b[j];
        const float p = t * t;
        d = d + p;
    }
    return d;
}

// Ratio test + stable compaction + keypoint gather (main.cpp:49-69 in its ratio form, :77-78, :89-91) fused into the
// refinement launch.  Tiles of 32 queries = 8 workgroups.  A workgroup adds (1 << 32 | its 4 keep bits) to the tile's
// arrival word with ONE agent-scope atomic; the workgroup whose add completes the tile owns the tile's compaction: it
// publishes the tile's survivor count (epoch-tagged, so nothing is ever cleared), sums the counts of the tiles before it
// (decoupled look-back: one polling lane per earlier tile; earlier tiles belong to earlier workgroups, which the
// dispatcher started first) and writes the tile's survivors at prefix + rank.  What it needs from the other seven
// workgroups — nearest neighbour and distance of each query — reaches it as one 8-byte write-through store per query
// (agent scope, drained before the arrival add), read back with agent-scope loads.
struct KnnFuse {
    float ratio;
    const float* kp1;             // may be null together with kp2 / xy1 / xy2: match list only
    const float* kp2;
    pm_match* good;
    float* xy1;
    float* xy2;
    int* n_out;
    unsigned long long* pk;       // [nq] (distance bits << 32) | trainIdx of the nearest neighbour
    unsigned long long* tile;     // [tiles] arrival word: arrivals << 32 | 32 keep bits; back to 0 when the tile is taken
    unsigned* tilecnt;            // [tiles] epoch << 8 | survivors (epoch-tagged, never cleared)
    unsigned* err;                // set to the epoch if a look-back gave up (never observed; read by pm_ctx_filter_fusion_status)
    unsigned epoch;
};
constexpr int KF_TILE_BLOCKS = 8;                 // workgroups (of 4 queries) per tile
constexpr unsigned KF_SPIN_LIMIT = 1u << 22;

// The tail both refinement kernels end with, once.  Unit `mine` (a 32-query tile of knn_l2_refine, a 16-query workgroup of
// knn_l2_refine8) publishes its survivor count and sums the counts of the units before it: decoupled look-back, one polling
// lane per earlier unit.  Earlier units belong to workgroups the dispatcher started earlier; the spin is bounded anyway, and
// a give-up leaves the epoch in the error word.  Called by all 256 threads (one workgroup barrier); -> survivors before `mine`.
__device__ __forceinline__ int kf_prefix(const KnnFuse& fz, int mine, int cnt)
{
    __shared__ int s_pre[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0)
        __hip_atomic_store(&fz.tilecnt[mine], (fz.epoch << 8) | static_cast<unsigned>(cnt), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int before = 0;
    for (int j = tid; j < mine; j += 256) {
        unsigned v = 0u, spins = 0u;
        for (;;) {
            v = __hip_atomic_load(&fz.tilecnt[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((v >> 8) == fz.epoch || ++spins > KF_SPIN_LIMIT) break;
            __builtin_amdgcn_s_sleep(1);
        }
        if ((v >> 8) == fz.epoch) before += static_cast<int>(v & 255u);
        else __hip_atomic_store(fz.err, fz.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o, 64);
    if (lane == 0) s_pre[wave] = before;
    __syncthreads();
    return s_pre[0] + s_pre[1] + s_pre[2] + s_pre[3];
}

// survivor `off` of the call: query qi with its nearest neighbour's record (distance bits << 32) | trainIdx, and the
// keypoints of the pair when the caller gave them
__device__ __forceinline__ void kf_emit(const KnnFuse& fz, int qi, int off, unsigned long long rec)
{
    pm_match m;
    m.queryIdx = qi;
    m.trainIdx = static_cast<int>(static_cast<uint32_t>(rec));
    m.imgIdx = 0;
    m.distance = __uint_as_float(static_cast<uint32_t>(rec >> 32));
    fz.good[off] = m;
    if (fz.kp1) {
        *reinterpret_cast<float2*>(fz.xy1 + 2 * static_cast<size_t>(off)) =
            *reinterpret_cast<const float2*>(fz.kp1 + 2 * static_cast<size_t>(qi));
        *reinterpret_cast<float2*>(fz.xy2 + 2 * static_cast<size_t>(off)) =
            *reinterpret_cast<const float2*>(fz.kp2 + 2 * static_cast<size_t>(m.trainIdx));
    }
}

// the last unit of the grid knows the total
__device__ __forceinline__ void kf_finish(const KnnFuse& fz, bool last_unit, int total) { if (last_unit && threadIdx.x == 0) *fz.n_out = total; }

// NS = candidate-list entries a lane holds (ceil(slots / 64) rounded up to 1, 2, 4 or 8): the slot
// values are read ONCE into registers, the candidates of all lists are compacted into one per-wave
// LDS list and evaluated together (8 rows per round), so neither the number of lists nor the way the
// candidates spread over them adds rounds.  (This kernel is VALU-issue bound: one wave per query.)
// (amdgpu_num_sgpr: the fused tail's pointers pushed the kernel to 95 SGPRs, and above 80 a CU admits 7 instead of 8
// of these workgroups — 1792 of the 2048 at C3, i.e. a second round: 10 -> 20 us.  Capped, the kernel stays at 8.)
// GEN: the automatic route may have ranked general floats on rounded copies (SPEC S1c); the other routes are
// instantiated without that code (its scalar loads and the rescale cost the headline path 0.6 us at C3).
// KM: neighbours a lane keeps (2: k <= 2; 4: k <= 4 — the coarse lists hold 4 groups per (query, split), so the k-th
// smallest coarse value still bounds the k-th neighbour; a full list inside the window re-scans its split, as for k <= 2)
template <bool VEC4, int NS, bool FUSE, bool GEN, int KM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_sgpr(80))) void knn_l2_refine(
    const float* __restrict__ Q, const float* __restrict__ T, const float* __restrict__ qnorm,
    const unsigned long long* __restrict__ stats, unsigned epoch, unsigned* __restrict__ diag, int nq, int nt,
    int dim, int k, KnnGeom g16, KnnGeom g32, int route, pm_match* __restrict__ out, KnnFuse fz)
{
    __shared__ int clist[4][64 * NS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int q = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wave);
    bool ghost = false;                                      // FUSE: waves past the last query stay for the barriers
    if (q >= nq) {                                           // wave-uniform
        if (!FUSE) return;                                   // (no block barriers below without FUSE)
        ghost = true;
        q = nq - 1;
    }
    const float* qp = Q + static_cast<size_t>(q) * dim;
    const float na = qnorm[q];
    const unsigned long long s0 = stats[0], s1 = stats[1];
    const float tmax = static_cast<unsigned>(s0 >> 32) == epoch ? __uint_as_float(static_cast<unsigned>(s0)) : 0.f;
    const bool flagged = static_cast<unsigned>(s1 >> 32) == epoch;
    const bool ineligible = flagged && (s1 & 2ull);          // data not integer-valued / too large for f16
    // which coarse route produced the lists; a wrong integer hint voids them (exact re-scan)
    bool general = false;                                                        // f16-rounded scaled copies
    if constexpr (GEN) {
        const unsigned long long s3 = stats[3];
        const bool gen_off = static_cast<unsigned>(s3 >> 32) == epoch;          // the general-float f16 route withdrew
        general = route == ROUTE_AUTO && ineligible && !gen_off;
    }
    const bool hinted = route == ROUTE_F16_HINT || route == ROUTE_U8_HINT;
    const bool use16 = hinted || (route == ROUTE_AUTO && (!ineligible || general));
    const bool nonfinite = (flagged && (s1 & 1ull)) || (hinted && ineligible);
    const KnnGeom g = use16 ? g16 : g32;
    float unscale = 1.f, eps_c = g.eps_coef, eps_abs = 0.f;
    bool unranked = false;
    if constexpr (GEN) {
        if (general) {
            const QueryScale qs = query_scale(train_half_exp(s0, epoch), na);
            unscale = qs.unscale;
            eps_c = g.eps_coef_gen;
            eps_abs = g.abs_gen * qs.unscale;
            unranked = qs.unranked;
        }
    }
    if (diag && lane == 0 && !ghost && q == 0) diag[2] = general ? 1u : (use16 ? (g.int_shift ? 3u : 0u) : 2u);
    const int slots = g.slots, tiles_per_split = g.tiles_per_split, rows_per_tile = g.rows_per_tile;
    const unsigned lid_mask = g.lid_mask;
    // window half-width: fp error of the coarse value + truncation by the embedded row id
    // (u8 route: exact integers, the coarse value is d2 or d2 - 1)
    const float eps = g.int_shift ? 1.f : eps_c * (na + tmax) + g.embed_coef * (na + 2.f * tmax) + eps_abs;
    const float* cv = g.cand + static_cast<size_t>(q) * slots;
    const int gshift = 31 - __clz(rows_per_tile >> 3);       // groups per tile = rows/8 = 2^gshift

    // slot s = lane + 64*i: value w = q.t - ||t||^2/2 (+id bits) -> coarse squared distance
    // d2a = ||q||^2 - 2w; first of the 4 consecutive rows of the group the slot names
    float val[NS];
    int row0[NS];
    MinN<float, KM> mn;
    mn.init(KNN_INF);
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int s = lane + 64 * i;
        const float w = s < slots ? cv[s] : -KNN_INF;
        const float ws = GEN ? w * unscale : w;                                  // (a power of two: the id bits survive)
        float v = w > -1.0e38f ? fmaf(-2.f, ws, na) : KNN_INF;
        if (g.int_shift) {                                                       // wave-uniform: integer candidates
            const int wi = static_cast<int>(__float_as_uint(w)) >> g.int_shift;
            v = (s < slots && wi > U8_PAD_SEED) ? fmaf(-2.f, static_cast<float>(wi), na) : KNN_INF;
        }
        const unsigned gid2 = __float_as_uint(w) & lid_mask;   // (group id << 1) | lane half
        const unsigned gid = gid2 >> 1;
        const int split = s >> 2, hh = static_cast<int>(gid2 & 1u);      // s / KNN_C
        const int tile = static_cast<int>(gid >> gshift), rem = static_cast<int>(gid & ((1u << gshift) - 1u));
        val[i] = v;
        row0[i] = (split * tiles_per_split + tile) * rows_per_tile + 32 * (rem >> 2) + 8 * (rem & 3) + 4 * hh;
        mn.insert(v);
    }
    static_assert(KNN_C == 4, "slot decoding assumes 4 entries per list");
    // k-th smallest coarse value over all slots (k <= KM)
    float tau = KNN_INF;
    for (int round = 0; round < k; ++round) {
        tau = wave_min_f32(mn.m[0]);
        const unsigned long long owners = __ballot(mn.m[0] == tau);
        if (owners == 0ull) break;               // NaN guard
        const int first = __ffsll(static_cast<long long>(owners)) - 1;
        if (lane == first) mn.pop(KNN_INF);
    }
    const float thr = (tau + eps) * 1.00000095367431640625f + eps;

    // Non-finite inputs (or a window that is not finite) void the coarse ranking: scan everything.
    const bool rescan = nonfinite || !(thr < KNN_INF) || unranked;
    if (diag && lane == 0 && !ghost) { if (rescan) atomicAdd(&diag[0], 1u); if (nonfinite) diag[1] = 1u; }

    BestN<KM> b;
    b.init();
    if (!rescan) {
        const int grp = lane >> 3, l = lane & 7;
        int total = 0;
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            if (64 * i >= slots) break;                     // wave-uniform
            const int s = lane + 64 * i;
            const bool in = s < slots;
            const float v = val[i];
            const int j = row0[i];
            // a sub-list (4 consecutive slots) whose 4th entry is inside the window may have
            // dropped candidates: its rows are scanned below instead of trusting its slots
            unsigned long long spilled = __ballot(in && (s & (KNN_C - 1)) == KNN_C - 1 && v <= thr);
            const bool mine_spilled = (spilled >> (lane | (KNN_C - 1))) & 1ull;
            const bool is_cand = in && v <= thr && j < nt && !mine_spilled;
            const unsigned long long cand = __ballot(is_cand);
            if (is_cand) clist[wave][total + pm::lane_rank(cand, lane)] = j;
            total += __popcll(cand);
            if (diag && lane == 0 && spilled && !ghost) atomicAdd(&diag[0], static_cast<unsigned>(__popcll(spilled)));
            while (spilled) {                               // wave-uniform, rare: every row of that split
                const int split = (64 * i + __ffsll(static_cast<long long>(spilled)) - 1) / KNN_C;
                spilled &= spilled - 1ull;
                const int row_begin = split * tiles_per_split * rows_per_tile;
                for (int lid = lane; lid < tiles_per_split * rows_per_tile; lid += 64) {
                    const int row = row_begin + lid;
                    if (row < nt) {
                        const float d = __builtin_sqrtf(
                            l2sqr_canonical<VEC4>(qp, T + static_cast<size_t>(row) * dim, dim));
                        b.insert(knn_key(d, row), d);
                    }
                }
            }
        }
        // the candidate list was written by some lanes and is read by others of the SAME wave: order the LDS
        // stores before the loads explicitly (no workgroup barrier: waves run on independent queries)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int nc = 4 * total;                           // every candidate group is 4 consecutive rows
        for (int r0 = 0; r0 < nc; r0 += 8) {                // 8 rows per round, 8 lanes each
            const int rank = r0 + grp;
            const bool live0 = rank < nc;
            int jj = clist[wave][live0 ? rank >> 2 : 0] + (rank & 3);
            const bool live = live0 && jj < nt;
            jj = jj < nt ? jj : nt - 1;
            const float d2 = l2sqr_canonical_coop8(qp, T + static_cast<size_t>(jj) * dim, dim, l);
            if (live && l == 0) {
                const float d = __builtin_sqrtf(d2);
                b.insert(knn_key(d, jj), d);
            }
        }
    } else {
        for (int j = lane; j < nt; j += 64) {
            const float d =
                __builtin_sqrtf(l2sqr_canonical<VEC4>(qp, T + static_cast<size_t>(j) * dim, dim));
            b.insert(knn_key(d, j), d);
        }
    }
    int nn_idx[2] = {-1, -1};                                // wave-uniform copies of the first two neighbours (FUSE)
    float nn_d[2] = {KNN_INF, KNN_INF};
    for (int c = 0; c < k; ++c) {
        const uint64_t best = wave_min_u64(b.k[0]);
        const unsigned long long owners = __ballot(b.k[0] == best);
        const int first = __ffsll(static_cast<long long>(owners)) - 1;
        const float dist = __shfl(b.d[0], first, 64);
        if (lane == first) b.pop();
        pm_match m;
        m.queryIdx = q;
        m.imgIdx = 0;
        if (best == ~0ull) { m.trainIdx = -1; m.distance = KNN_INF; }
        else { m.trainIdx = static_cast<int>(static_cast<uint32_t>(best)); m.distance = dist; }
        if (c < 2) { nn_idx[c] = m.trainIdx; nn_d[c] = m.distance; }
        if (lane == 0 && !ghost && out) out[static_cast<size_t>(q) * k + c] = m;
    }
    if (!FUSE) return;

    // ---- ratio test + stable compaction + gather, in this launch (see KnnFuse)
    __shared__ unsigned s_keep[4];
    __shared__ unsigned s_bits;
    __shared__ int s_last;
    const int tid = threadIdx.x;
    {
        const float rhs = fz.ratio * nn_d[1];                // pm_filter_ratio: float multiply, strict <
        const bool keep = !ghost && nn_idx[0] >= 0 && nn_idx[1] >= 0 && nn_d[0] < rhs;
        if (lane == 0) {
            if (!ghost)
                __hip_atomic_store(&fz.pk[q], (static_cast<unsigned long long>(f32_bits(nn_d[0])) << 32) |
                                                  static_cast<unsigned long long>(static_cast<uint32_t>(nn_idx[0])),
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_keep[wave] = keep ? 1u : 0u;
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // this wave's 8-byte record is written through
    __syncthreads();
    const int blk = static_cast<int>(blockIdx.x), tile = blk / KF_TILE_BLOCKS;
    const int nblk = static_cast<int>(gridDim.x), ntiles = (nblk + KF_TILE_BLOCKS - 1) / KF_TILE_BLOCKS;
    if (tid == 0) {
        const unsigned bits4 = s_keep[0] | (s_keep[1] << 1) | (s_keep[2] << 2) | (s_keep[3] << 3);
        const unsigned long long add = (1ull << 32) | (static_cast<unsigned long long>(bits4) << (4 * (blk % KF_TILE_BLOCKS)));
        const unsigned long long old = __hip_atomic_fetch_add(&fz.tile[tile], add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int in_tile = nblk - tile * KF_TILE_BLOCKS < KF_TILE_BLOCKS ? nblk - tile * KF_TILE_BLOCKS : KF_TILE_BLOCKS;
        const bool last = static_cast<int>(old >> 32) == in_tile - 1;
        s_last = last ? 1 : 0;
        if (last) {
            s_bits = static_cast<unsigned>(old + add);
            __hip_atomic_store(&fz.tile[tile], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next call
        }
    }
    __syncthreads();
    if (!s_last) return;
    const unsigned bits = s_bits;
    const int cnt = __popc(bits);
    const int prefix = kf_prefix(fz, tile, cnt);
    if (tid < 32 && ((bits >> tid) & 1u)) {
        const int qi = tile * (4 * KF_TILE_BLOCKS) + tid;
        kf_emit(fz, qi, prefix + __popc(bits & ((1u << tid) - 1u)),
                __hip_atomic_load(&fz.pk[qi], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
    kf_finish(fz, tile == ntiles - 1, prefix + cnt);
}

// ---------------------------------------------------------------------------------------------
// u8 route refinement (round 3; rows read eight lanes to a row since round 5).  For u8-valued data every partial sum
// of the canonical f32 distance (SPEC S1) is an integer below 2^24, i.e. the canonical value IS the integer squared
// distance, whatever the summation order and whichever lanes add which bytes — so the rows are re-evaluated on the
// centred byte copies the coarse pass already made: d2 = ||q'||^2 + ||t'||^2 - 2 q'.t' with 32 v_dot4_i32_i8 per row
// (128 B per row instead of 512 B and ~400 f32 operations), distance = sqrtf(float(d2)) (correctly rounded), key =
// (distance bits, index) as everywhere.  Candidate groups hold GROUP = 4, 8 or 16 rows (the coarse kernel's selection
// cost falls with the group size).  A wrong hint (bit 1 of stats[1]) sends every query to the canonical f32 scan.
//
// A row is read by EIGHT lanes, lane `sub` taking its 16-byte unit `sub` (with wide rows: of the row's first eight
// units), so one load instruction of the wave fetches eight whole 128-byte rows in eight cache lines.  The first form let
// one lane read one whole row as eight 16-byte loads 128 bytes apart: every instruction touched 64 lines and every line
// was visited eight times (the pattern of coarse form 4).  Each lane multiplies its unit with the same unit of
// the query (4 v_dot4_i32_i8) and three DPP adds inside the eight lanes leave the row's dot product in every one of them.
// Eight such steps cover eight rows per eight lanes, and the lane with sub == step keeps that step's sum: every lane
// still owns one row per pass, and everything after the sum (tnorm, sqrtf, the per-lane BestN) is what it was.  DPP needs
// whole rows of lanes: a lane group with no row left loads from a valid row and drops the sum.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int u8_unit_dot8(const uint4& qu, const uint4& tu)
{
    int a = __builtin_amdgcn_sdot4(static_cast<int>(qu.x), static_cast<int>(tu.x), 0, false);
    a = __builtin_amdgcn_sdot4(static_cast<int>(qu.y), static_cast<int>(tu.y), a, false);
    a = __builtin_amdgcn_sdot4(static_cast<int>(qu.z), static_cast<int>(tu.z), a, false);
    a = __builtin_amdgcn_sdot4(static_cast<int>(qu.w), static_cast<int>(tu.w), a, false);
    // (pm::dpp_u32 with old = 0 and bound_ctrl: every source lane is live, and in this form the add takes the DPP operand
    // itself — v_add_u32_dpp, three instructions for the three steps instead of six)
    a += __builtin_amdgcn_update_dpp(0, a, 0xB1, 0xF, 0xF, true);          // quad_perm:[1,0,3,2]
    a += __builtin_amdgcn_update_dpp(0, a, 0x4E, 0xF, 0xF, true);          // quad_perm:[2,3,0,1]
    a += __builtin_amdgcn_update_dpp(0, a, 0x141, 0xF, 0xF, true);         // row_half_mirror: the other quad of the eight
    return a;
}

// FOUR queries per wave, one 16-lane row each: the candidate slots of a query (32 at config C3) never filled a wave, and
// the first form of this kernel (one wave per query, ~300 instructions, like knn_l2_refine) was issue-bound at ~5 us for
// 8192 queries.  Here the k-th-smallest search and the final top-k are 4-step DPP reductions inside a row (row_ror: no
// cross-row traffic, no v_readlane) shared by four queries, and the usual two candidate groups of 8 rows are exactly
// one pass of a row of lanes: 16 candidate rows per query and pass.  The 16 lanes read them as two halves of eight
// (u8_unit_dot8 above): in step j = 0..7 half hh = l >> 3 reads candidate r0 + 2j + hh, so a load instruction of the wave
// covers 4 queries x 2 rows x 128 B, and lane (hh, sub) ends the pass owning candidate r0 + 2 sub + hh.  A lane holds
// one 16-byte unit of its query, not the whole row.  A query with an overflowing list, fewer than k ranked groups or a
// wrong hint scans all train rows (rare).

// Exact re-scans of knn_l2_refine8 (round 3).  A list whose 4th entry is inside the window may have dropped candidates
// (SPEC S1b), so the rows of that split are evaluated exactly; runs of identical train rows — repeated texture — make that
// a common case (12 identical rows fill a list with four groups at the same distance).  The first form of this kernel let
// the query's 16 lanes walk ALL train rows: 512 dependent passes at 8192 rows, and because a launch lasts as long as its
// slowest wave the matcher call went from 23 to 225 us with 52 such queries among 8192 (1 ms at 32k x 32k).  Now only the
// spilled SPLITS are evaluated, by all 64 lanes of the wave for one of its four queries at a time (a variant that handed
// them to the whole workgroup cut the tail further but cost every launch a barrier: +1 us at config C3).
//
// The rows are read like the common path's (u8_unit_dot8): `qu` is unit lane & 7 of the owner's query, and in step
// j = 0..7 the eight lanes of group g = lane >> 3 read row base + 8j + g, so a load instruction of the wave fetches eight
// consecutive rows.  The lane with (lane & 7) == j keeps step j's sum: a lane inserts one row per 64, as before.  All eight
// loads of an iteration are in flight at once: round 3 split a row into two halves because whole rows in flight cost the
// common path a wave per SIMD (106 VGPRs); with one query unit per lane the compiler's resource report shows no
// instantiation losing occupancy (82 VGPRs at most for k <= 2, 90 for k <= 4), so the split is gone.
template <int KM>
__device__ __forceinline__ void r8_scan_rows(BestN<KM>& tb, const uint4& qu, int qn, const uint4* __restrict__ T8,
                                             const float* __restrict__ tnorm, int t_row16, int row_begin, int row_end, int lane)
{
    const int sub = lane & 7, g = lane >> 3;
    for (int base = row_begin; base < row_end; base += 64) {
        const int row = base + 8 * sub + g;
        const bool ok = row < row_end;
        float tn = tnorm[ok ? row : row_begin];
        uint4 tv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {                         // (all eight loads ahead of the first use)
            const int rj = base + 8 * j + g;
            tv[j] = T8[static_cast<size_t>(rj < row_end ? rj : row_begin) * t_row16 + sub];
        }
        asm volatile("" : "+v"(tn));                          // (the norm travels with the rows)
        int acc = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int sum = u8_unit_dot8(qu, tv[j]);
            acc = sub == j ? sum : acc;
        }
        asm volatile("" : "+v"(acc));                         // (sums and selects stay with their DPP moves)
        const float d = __builtin_sqrtf(static_cast<float>(qn + static_cast<int>(tn) - 2 * acc));
        if (ok) tb.insert(knn_key(d, row), d);
    }
}

// FUSE (k == 2): the ratio test, the stable compaction and the keypoint gather (main.cpp:49-69 in its ratio form, :77-78,
// :89-91) ride this launch.  A workgroup holds 16 whole queries, so nothing is handed between workgroups but ONE
// epoch-tagged survivor count each (decoupled look-back over the earlier workgroups, as in filter_ratio_gather); `out`
// may then be null.
template <int NS, int GROUP, int KM, bool FUSE>
__global__ __launch_bounds__(256) void knn_l2_refine8(
    const float* __restrict__ Q, const float* __restrict__ T, const uint4* __restrict__ Q8, const uint4* __restrict__ T8,
    const float* __restrict__ qnorm, const float* __restrict__ tnorm, const int* __restrict__ cand,
    const unsigned long long* __restrict__ stats, unsigned epoch, unsigned* __restrict__ diag, int nq, int nt, int dim, int k,
    int slots, int tiles_per_split, pm_match* __restrict__ out, KnnFuse fz, int t_row16)
{
    constexpr int GPB = 16 / GROUP;                          // groups per 32-row block and lane half
    constexpr int IMAX = 0x7FFFFFFF;
    __shared__ int clist[4][4][16 * NS];                     // [wave][query of the wave][candidate]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int qi = lane >> 4, l = lane & 15;
    const int q = blockIdx.x * 16 + wave * 4 + qi;
    const bool live = q < nq;
    const int qc = live ? q : nq - 1;                        // rows past the last query shadow it (no early exit: DPP rows stay whole)
    const unsigned long long s1 = stats[1];
    const bool wrong_hint = static_cast<unsigned>(s1 >> 32) == epoch;       // any flag: not u8-valued (or not finite)
    if (diag && threadIdx.x == 0 && blockIdx.x == 0) diag[2] = 3u;
    const int qn = static_cast<int>(qnorm[qc]);
    const int* cv = cand + static_cast<size_t>(qc) * slots;
    const int sub = l & 7, hf = l >> 3;                      // 16-byte unit of a row, and half of the 16-lane row
    const uint4 qu = Q8[static_cast<size_t>(qc) * U8_ROW16 + sub];         // the lane's unit of the query's centred bytes

    // slot s = l + 16*i: candidate (w << U8_SHIFT) | (group id << 1 | lane half); coarse squared distance
    // d2a = ||q'||^2 - 2w = d2 or d2 - 1 of the group's best row
    int val[NS], code[NS];
    MinN<int, KM> mn;
    mn.init(IMAX);
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int s = l + 16 * i;
        const int c = s < slots ? cv[s] : I8_EMPTY;
        const int wi = c >> U8_SHIFT;
        const int v = wi > U8_PAD_SEED ? qn - 2 * wi : IMAX;
        const int gid2 = c & ((1 << U8_SHIFT) - 1);
        const int gid = gid2 >> 1, hh = gid2 & 1;
        const int split = s >> 2;
        const int tile = gid / (4 * GPB), rem = gid % (4 * GPB);
        val[i] = v;
        // first row of the group's 32-row block | (group inside the block << 1) | lane half   (block rows are multiples of 32)
        code[i] = ((split * tiles_per_split + tile) * H_TT + 32 * (rem / GPB)) | ((rem % GPB) << 1) | hh;
        mn.insert(v);
    }
    static_assert(KNN_C == 4, "slot decoding assumes 4 entries per list");
    int tau = IMAX;
    for (int round = 0; round < k; ++round) {                // k <= KM
        tau = static_cast<int>(pm::row16_min_u32(static_cast<unsigned>(mn.m[0]) ^ 0x80000000u) ^ 0x80000000u);
        const unsigned owners = static_cast<unsigned>(__ballot(mn.m[0] == tau) >> (16 * qi)) & 0xFFFFu;
        if (l == __ffs(static_cast<int>(owners)) - 1) mn.pop(IMAX);
    }
    const bool full = wrong_hint || tau == IMAX;             // fewer than k ranked groups (nt < k, ...): scan everything
    const int thr = tau == IMAX ? 0 : tau + 1;

    // a list whose 4th entry is inside the window may have dropped candidates: the rows of that SPLIT are evaluated exactly
    // (by the workgroup, below); its ranked groups are then not expanded a second time
    unsigned long long spill = 0ull;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        if (16 * i >= slots) break;                          // wave-uniform
        const int s = l + 16 * i;
        unsigned sp = static_cast<unsigned>(__ballot(s < slots && !full && (s & (KNN_C - 1)) == KNN_C - 1 && val[i] <= thr) >> (16 * qi)) & 0xFFFFu;
        while (sp) {                                         // (at most four lists per 16 slots)
            const int bit = __ffs(static_cast<int>(sp)) - 1;
            sp &= sp - 1u;
            spill |= 1ull << ((bit + 16 * i) >> 2);
        }
    }
    int total = 0;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        if (16 * i >= slots) break;                          // wave-uniform
        const int s = l + 16 * i;
        const bool is_cand = s < slots && !full && val[i] <= thr && !((spill >> (s >> 2)) & 1ull);
        const unsigned rm = static_cast<unsigned>(__ballot(is_cand) >> (16 * qi)) & 0xFFFFu;
        if (is_cand) clist[wave][qi][total + __popc(rm & ((1u << l) - 1u))] = code[i];
        total += __popc(rm);
    }
    if (diag && l == 0 && live && (full || spill)) { atomicAdd(&diag[0], 1u); if (wrong_hint) diag[1] = 1u; }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();

    BestN<KM> b;
    b.init();
    // Candidate p = 0..15 of a pass is row p % GROUP of group p / GROUP of the pass; rows of a group come four in a run, the
    // next four 8 further on.  Step j gives this half candidate 2j + hf, so that the lane ends up owning candidate 2 sub + hf.
    constexpr unsigned NO_ROW = 0x7FFFFF00u;                 // first row of a group past the list: no train set has it
    auto group_row = [](int pos) { return (pos & 3) + 8 * (pos >> 2); };
    const int ngroups = full ? 0 : total;
    const int own_grp = (2 * sub) / GROUP, own_off = group_row((2 * sub) % GROUP);
    const char* tunit = reinterpret_cast<const char*>(T8 + sub);           // the lane's unit of row 0
    const unsigned tpitch = 16u * static_cast<unsigned>(t_row16), last = static_cast<unsigned>(nt - 1);
    for (int g0 = 0; __any(g0 < ngroups); g0 += GPB) {       // 16 rows per query and pass; a lane ends up owning one
        unsigned first[GPB];                                 // first row of the pass's groups, + hf
#pragma unroll
        for (int g = 0; g < GPB; ++g) {
            const int cd = clist[wave][qi][g0 + g];          // (past the list: whatever LDS held)
            const unsigned r = static_cast<unsigned>((cd & ~31) + 8 * (GROUP / 4) * ((cd >> 1) & 15) + 4 * (cd & 1) + hf);
            first[g] = g0 + g < ngroups ? r : NO_ROW;
        }
        unsigned mine = first[0];
#pragma unroll
        for (int g = 1; g < GPB; ++g) mine = own_grp == g ? first[g] : mine;
        mine += own_off;
        float tn = tnorm[min(mine, last)];
        uint4 tv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {                        // all eight loads ahead of the first use
            const unsigned row = first[(2 * j) / GROUP] + group_row((2 * j) % GROUP);
            // no such row (past the list, or past the train set in its last block): a valid address, the sum is dropped
            tv[j] = *reinterpret_cast<const uint4*>(tunit + static_cast<size_t>(min(row, last)) * tpitch);
        }
        asm volatile("" : "+v"(tn));                         // (the norm travels with the rows, not behind the branch below)
        int dot = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int sum = u8_unit_dot8(qu, tv[j]);
            dot = sub == j ? sum : dot;
        }
        asm volatile("" : "+v"(dot));                        // (sums and selects stay with their DPP moves, outside the branch)
        if (mine <= last) {
            const float d = __builtin_sqrtf(static_cast<float>(qn + static_cast<int>(tn) - 2 * dot));
            b.insert(knn_key(d, static_cast<int>(mine)), d);
        }
    }
    if (wrong_hint) {                                        // canonical scan of the f32 rows (a wrong hint only costs time)
        const float* qp = Q + static_cast<size_t>(qc) * dim;
        for (int j = l; j < nt; j += 16) {
            const float d = __builtin_sqrtf(l2sqr_canonical<true>(qp, T + static_cast<size_t>(j) * dim, dim));
            b.insert(knn_key(d, j), d);
        }
    }
    // ---- exact re-scans, by the whole WAVE for one of its four queries at a time (no barrier, no LDS: the common case pays
    // one ballot).  The owner row's masks reach the other 48 lanes by shuffles, its bytes are read again; every lane keeps the KM best keys
    // of the rows it evaluated, and KM wave-wide minimum reductions hand the best of them to the owner.
    {
        const bool need = live && !wrong_hint && (full || spill != 0ull);
        unsigned long long needy = __ballot(need && l == 0);             // bit 16*qi: row qi needs a scan
        while (needy) {
            const int src = __ffsll(static_cast<long long>(needy)) - 1;      // the owner row's first lane
            needy &= needy - 1ull;
            const int oqi = __shfl(qc, src, 64);                            // the owner's query: its bytes again (one address per wave)
            const uint4 oq = Q8[static_cast<size_t>(oqi) * U8_ROW16 + (lane & 7)];      // (the lane's unit of them)
            const int oqn = __shfl(qn, src, 64);
            const int oall = __shfl(full ? 1 : 0, src, 64);
            const unsigned mlo = __shfl(static_cast<unsigned>(spill), src, 64), mhi = __shfl(static_cast<unsigned>(spill >> 32), src, 64);
            unsigned long long mm = oall ? 0ull : ((static_cast<unsigned long long>(mhi) << 32) | mlo);
            BestN<KM> tb;
            tb.init();
            const int rows_per_split = tiles_per_split * H_TT;
            if (oall) {
                r8_scan_rows<KM>(tb, oq, oqn, T8, tnorm, t_row16, 0, nt, lane);
            } else {
                while (mm) {
                    const int sp = __ffsll(static_cast<long long>(mm)) - 1;
                    mm &= mm - 1ull;
                    const int r0 = sp * rows_per_split;
                    r8_scan_rows<KM>(tb, oq, oqn, T8, tnorm, t_row16, r0, r0 + rows_per_split < nt ? r0 + rows_per_split : nt, lane);
                }
            }
            for (int j = 0; j < KM; ++j) {                               // the KM best of the wave's keys -> the owner's first lane
                const uint64_t m = pm::wave_min_u64(tb.k[0]);
                if (tb.k[0] == m && m != ~0ull) tb.pop();                // (keys are distinct rows)
                if (lane == src && m != ~0ull) b.insert(m, __uint_as_float(static_cast<unsigned>(m >> 32)));
            }
        }
    }
    int nn_idx[2] = {-1, -1};                                // the first two neighbours of the row's query (FUSE)
    float nn_d[2] = {KNN_INF, KNN_INF};
    for (int c = 0; c < k; ++c) {
        const uint64_t best = pm::row16_min_u64(b.k[0]);
        const unsigned owners = static_cast<unsigned>(__ballot(b.k[0] == best) >> (16 * qi)) & 0xFFFFu;
        const int first = __ffs(static_cast<int>(owners)) - 1;
        const float dist = __shfl(b.d[0], 16 * qi + first, 64);
        if (l == first) b.pop();
        pm_match m;
        m.queryIdx = q;
        m.imgIdx = 0;
        if (best == ~0ull) { m.trainIdx = -1; m.distance = KNN_INF; }
        else { m.trainIdx = static_cast<int>(static_cast<uint32_t>(best)); m.distance = dist; }
        if (c < 2) { nn_idx[c] = m.trainIdx; nn_d[c] = m.distance; }
        if (l == 0 && live && out) out[static_cast<size_t>(q) * k + c] = m;
    }
    if constexpr (FUSE) {
        __shared__ unsigned s_bits[4];
        __shared__ unsigned long long s_rec[16];
        const int tid = threadIdx.x;
        const float rhs = fz.ratio * nn_d[1];                // pm_filter_ratio: float multiply, strict <
        const bool keep = live && nn_idx[0] >= 0 && nn_idx[1] >= 0 && nn_d[0] < rhs;
        if (l == 0)
            s_rec[wave * 4 + qi] = (static_cast<unsigned long long>(f32_bits(nn_d[0])) << 32) |
                                   static_cast<unsigned long long>(static_cast<uint32_t>(nn_idx[0]));
        const unsigned long long bal = __ballot(l == 0 && keep);
        if (lane == 0)
            s_bits[wave] = static_cast<unsigned>(bal & 1ull) | (static_cast<unsigned>((bal >> 16) & 1ull) << 1) |
                           (static_cast<unsigned>((bal >> 32) & 1ull) << 2) | (static_cast<unsigned>((bal >> 48) & 1ull) << 3);
        __syncthreads();
        const unsigned bits = s_bits[0] | (s_bits[1] << 4) | (s_bits[2] << 8) | (s_bits[3] << 12);
        const int cnt = __popc(bits);
        const int blk = static_cast<int>(blockIdx.x);
        const int prefix = kf_prefix(fz, blk, cnt);
        if (tid < 16 && ((bits >> tid) & 1u)) kf_emit(fz, blk * 16 + tid, prefix + __popc(bits & ((1u << tid) - 1u)), s_rec[tid]);
        kf_finish(fz, blk == static_cast<int>(gridDim.x) - 1, prefix + cnt);
    }
}

}  // namespace
