// knn_l2_plan.hpp — route planning of the L2 matcher: everything knn_l2.hip decides before it touches the device, as a
// pure function of a dozen integers.  Plain C++ (no HIP header, no pm_ctx, no pointer beyond its alignment class), so the
// decision table is tested on the CPU: tests/test_knn_plan_cpu.py and tests/golden/knn_l2_plan_cases.json.  A route
// change is a change here plus a reviewed edit of that table; the launcher (knn_l2_enqueue) only obeys the plan.
#pragma once
#include <cstddef>

#include "knn_constants.hpp"
#include "pm.h"

namespace pm_knn {

enum { ROUTE_F32 = 0, ROUTE_F16_HINT = 1, ROUTE_AUTO = 2, ROUTE_U8_HINT = 3 };

struct KnnL2Request {
    int nq, nt, dim, k, flags, n_cu;
    int opts[PM_OPT_COUNT_];      // the context's options (pm_ctx_set_option)
    bool u8_rows;                 // the rows are u8 (pm_bf_knn_l2_u8*): only the u8 route takes them
    bool aligned;                 // both base pointers 16-byte aligned (f32 rows) / 4-byte aligned (u8 rows)
    bool fuse;                    // ratio test + compaction + gather are to ride the refinement launch (k == 2)
};

enum KnnVerdict {
    KNN_MATRIX = 0,               // a matrix-core route: the rest of the plan holds
    KNN_EXACT = 1,                // the exact VALU kernel (a fused tail cannot ride it: the caller filters afterwards)
    KNN_WIDEN = 2                 // u8 rows outside the u8 route: the caller widens them to f32 and plans again
};
// first prep launch
enum KnnPrep {
    KNN_PREP_U8ROWS,              // knn_l2_prep8_u8, 64 rows per workgroup
    KNN_PREP8_16,                 // knn_l2_prep8<1, dim == 128>, 16 rows per workgroup
    KNN_PREP8_64,                 // knn_l2_prep8<4, dim == 128>, 64 rows per workgroup
    KNN_PREP16_SEEDED,            // knn_l2_prep16<true, 128, true>
    KNN_PREP16_UNIT,              // knn_l2_prep16u<dp16, vec>
    KNN_PREP16,                   // knn_l2_prep16<false, dp16, vec>
    KNN_PREP32,                   // knn_l2_prep (norms only)
    KNN_PREP8_32                  // knn_l2_prep8<2, dim == 128>, 32 rows per workgroup (PM_OPT_KNN_PREP_ROWS = 3)
};
// what follows it on the automatic route
enum KnnPrepGen { KNN_GEN_NONE, KNN_GEN_PREP16G /* knn_l2_prep16g<dp16, vec> */, KNN_GEN_OFF /* knn_gen_off */ };

// KnnGeom (knn_l2.hip) without the candidate pointer, which the launcher carves from the arena
struct KnnGeomPlan {
    int slots, tiles_per_split, rows_per_tile;
    unsigned lid_mask;
    float eps_coef, embed_coef, eps_coef_gen, abs_gen;
    int int_shift;
};

struct KnnL2Plan {
    int verdict;
    int route;
    bool want32, want16;          // which coarse passes are enqueued
    bool vec;                     // rows are read as 16-byte vectors
    int dp16;                     // padded columns of the f16 copies
    bool unit_hint, gen32, f16s;
    int u8_form, u8_group;
    bool u8_int_refine;
    int t_wide;
    int qb_wg, nq_pad, nt_pad;
    KnnGeomPlan g32, g16;
    int splits32, splits16, lid_bits32, lid_bits16;
    // scratch, in carving order; every part is rounded up to 256 bytes
    size_t qnorm_bytes, tnorm_bytes, c32, c16, qh, th, sdb, qfb, pkb, need;
    int kf_tile;                  // queries per look-back tile of the fused tail (kf_prepare)
    int prep, prep_grid;          // KnnPrep and its grid
    int prep_gen;                 // KnnPrepGen (grid prep_grid; knn_gen_off: one workgroup)
    // template parameters of the refinement launch: knn_l2_refine8<NS, GROUP, KM, FUSE> (refine8) or
    // knn_l2_refine<VEC, NS, FUSE, GEN, KM>
    bool refine8;
    int refine_ns, refine_group, refine_km;
    bool refine_fuse, refine_vec, refine_gen;
};

inline size_t knn_align256(size_t x) { return (x + 255) / 256 * 256; }

// (hidden: an inline function of a shared library is otherwise an exported weak symbol)
__attribute__((visibility("hidden"))) inline KnnL2Plan knn_l2_plan(const KnnL2Request& r)
{
    KnnL2Plan p{};
    const int nq = r.nq, nt = r.nt, dim = r.dim, k = r.k, n_cu = r.n_cu;
    const int* opts = r.opts;
    const bool u8in = r.u8_rows, fuse = r.fuse;
    int flags = r.flags;
    p.verdict = KNN_WIDEN;
    if (u8in) {
        if (!(k <= 4 && (dim % 4) == 0 && dim <= 128 && nt >= 1 && r.aligned)) return p;
        flags = PM_KNN_HINT_U8;
    }

    // Rows are read as 16-byte vectors when dim % 4 == 0 and the base pointers are 16-byte aligned.  The f32-input pass
    // and the u8 route need that and dim <= 128 ("narrow"); the f16 passes also take any other layout (element loads in
    // the prep and refinement kernels: the padded copies do not care) and up to 256 dimensions (17 k-chunks).  Anything
    // else takes the exact kernel, whose loads are scalar unless both conditions hold.
    const bool vec = (dim % 4) == 0 && (u8in || r.aligned);
    const bool narrow = vec && dim <= 128;
    const bool wide16 = !narrow && !(flags & PM_KNN_FORCE_F32) && opts[PM_OPT_KNN_WIDE] != 1;
    const bool fast = !(flags & PM_KNN_FORCE_EXACT) && (k <= 2 || (k <= 4 && opts[PM_OPT_KNN_WIDE] != 1)) && dim <= 256 &&
                      nt >= 1 && (narrow || wide16) && (dim >= 4 || !vec);
    if (!fast) {
        if (!u8in) p.verdict = KNN_EXACT;                    // (u8 rows have no f32 image here: the caller widens first)
        return p;
    }
    int route = (flags & PM_KNN_FORCE_F32) ? ROUTE_F32 : ((flags & PM_KNN_HINT_U8) && narrow) ? ROUTE_U8_HINT :
                (flags & (PM_KNN_HINT_INTEGER | PM_KNN_HINT_U8)) ? ROUTE_F16_HINT : ROUTE_AUTO;
    const int dp16 = dim <= 128 ? 128 : 256;                 // padded columns of the f16 copies
    // automatic route: general floats rank on rounded f16 copies too (SPEC S1c); the f32-input pass is enqueued only when
    // forced (PM_KNN_FORCE_F32) or when PM_OPT_KNN_GENERAL_F16 = 1 keeps it as the automatic route's pass for such data
    // PM_KNN_HINT_UNIT_NORM: the automatic route's general-float form with its two prep launches in one (knn_l2_prep16u)
    const bool unit_hint = (flags & PM_KNN_HINT_UNIT_NORM) && route == ROUTE_AUTO;
    const bool gen32 = route == ROUTE_AUTO && !unit_hint && opts[PM_OPT_KNN_GENERAL_F16] == 1 && narrow;
    const bool want32 = route == ROUTE_F32 || gen32, want16 = route != ROUTE_F32;

    // ---- f32 route geometry: 64-row tiles, 128 queries per workgroup, two workgroups per CU.
    // (A 128-row tile with one workgroup per CU measured 172 us against 153 us at C3.)
    constexpr int TT = TT32;
    KnnGeomPlan g32{}, g16{};
    int splits32 = 1, splits16 = 1, lid_bits32 = 3, lid_bits16 = 4;
    {
        const int nqb = (nq + QB - 1) / QB;
        const int ntiles = (nt + TT - 1) / TT;
        int splits = (2 * n_cu + nqb - 1) / nqb;
        // at most 2048 train rows per split: the id embedded in a candidate costs mantissa bits, and with them
        // the window widens (more candidates, overflowing lists -> split re-scans): 9-10 id bits at most
        if (splits < (ntiles + 31) / 32) splits = (ntiles + 31) / 32;
        if (splits > ntiles) splits = ntiles;
        if (splits > 64) splits = 64;
        if (splits < 1) splits = 1;
        g32.tiles_per_split = (ntiles + splits - 1) / splits;
        splits32 = (ntiles + g32.tiles_per_split - 1) / g32.tiles_per_split;
        g32.slots = splits32 * KNN_C;
        g32.rows_per_tile = TT;
        // candidate id = (row-group id inside a lane's stream: tile_in_split*(TT/8) + block*4 + group) * 2 + lane half,
        // in the low mantissa bits
        while ((1 << lid_bits32) < g32.tiles_per_split * (TT / 8) * 2) ++lid_bits32;
        g32.lid_mask = (1u << lid_bits32) - 1u;
        // |coarse - canonical| <= (6*dim + 32) * 2^-24 * (||q||^2 + ||t||^2), plus the id truncation
        // 2^(bits-23) * (||q||^2 + 2||t||^2); see docs/SPEC.md S1b
        g32.eps_coef = static_cast<float>((6.0 * dim + 32.0) * 5.9604644775390625e-8 * 1.001);
        g32.embed_coef = static_cast<float>(static_cast<double>(1u << lid_bits32) * 1.1920928955078125e-7 * 1.01);
    }
    // ---- f16 route geometry: 128-row tiles, 256 queries per workgroup (4 waves x 64)
    // (u8 ring kernel in its 16-wave form, PM_OPT_KNN_F16_WAVES = 3: 512 queries per workgroup)
    // u8 coarse kernel form (PM_OPT_KNN_RING): 1 two LDS tile buffers, 2 / 3 ring, 4 / 5 register-operand forms (128 queries
    // per workgroup), 6 register-operand form with a split per WAVE — long sweeps only: taken when every CU stays busy with
    // splits of at least 8 tiles (1024 rows), else the two-buffer tile kernel runs
    const bool u8_default_group = opts[PM_OPT_KNN_U8_GROUP] != 1 && opts[PM_OPT_KNN_U8_GROUP] != 3;
    const bool u8_asked = ((flags & PM_KNN_HINT_U8) || u8in) && !(flags & PM_KNN_FORCE_F32);
    int u8_form = (u8_asked && u8_default_group) ? opts[PM_OPT_KNN_RING] : 1;
    int ws_splits = 0;
    if (u8_form == 6) {
        const int ntl = (nt + H_TT - 1) / H_TT, nqb128 = (nq + H_QB - 1) / H_QB * 2;
        int sp = (8 * n_cu + nqb128 - 1) / nqb128;                     // 8 waves per workgroup, one split each
        if (sp < (ntl + 15) / 16) sp = (ntl + 15) / 16;
        if (sp > 64) sp = 64;
        if (sp > ntl) sp = ntl;
        if (sp < 1) sp = 1;
        const int tps = (ntl + sp - 1) / sp;
        const bool fits = (static_cast<long long>(nt) + 3 * H_TT) * (U8_WIDE_ROW16 * 16) < 0x7FFFFFFFLL;   // 32-bit DMA offsets
        if (tps >= 8 && tps <= 16 && fits) ws_splits = sp; else u8_form = 1;
    }
    if (u8_form == 5 && (static_cast<long long>(nt) + 3 * H_TT) * (U8_WIDE_ROW16 * 16) >= 0x7FFFFFFFLL) u8_form = 1;
    const int qb_wg = u8_form >= 4 ? 128 : (u8_form >= 2 && opts[PM_OPT_KNN_F16_WAVES] == 3) ? 512 : H_QB;
    const int q_unit = qb_wg > H_QB ? qb_wg : H_QB;           // (a multiple of 256 also when workgroups take 128 queries)
    const int nq_pad = (nq + q_unit - 1) / q_unit * q_unit, nt_pad = (nt + H_TT - 1) / H_TT * H_TT;
    {
        const int nqb = nq_pad / qb_wg;
        const int ntiles = nt_pad / H_TT;
        // train splits sized for ONE workgroup per CU: with LDS-DMA staging a lone workgroup keeps the matrix pipe as busy as
        // two co-resident ones did with register staging (C3: 18.9 vs 19.0-21.7 us, 4096 x 4096: 10.0 vs 11.6 us), and half
        // the splits are half the candidate lists the refinement has to read.  PM_OPT_KNN_WG_PER_CU = 2: two per CU.
        const int wg_per_cu = opts[PM_OPT_KNN_WG_PER_CU] == 2 ? 2 : 1;
        int splits = ws_splits ? ws_splits : (wg_per_cu * n_cu + nqb - 1) / nqb;
        if (splits < (ntiles + 15) / 16) splits = (ntiles + 15) / 16;          // <= 2048 rows per split (see above)
        if (splits > ntiles) splits = ntiles;
        if (splits > 64) splits = 64;
        if (splits < 1) splits = 1;
        g16.tiles_per_split = (ntiles + splits - 1) / splits;
        splits16 = (ntiles + g16.tiles_per_split - 1) / g16.tiles_per_split;
        g16.slots = splits16 * KNN_C;
        g16.rows_per_tile = H_TT;
        while ((1 << lid_bits16) < g16.tiles_per_split * (H_TT / 8) * 2) ++lid_bits16;
        g16.lid_mask = (1u << lid_bits16) - 1u;
        g16.eps_coef = 0.f;           // integer data: the f16 products and f32 sums are exact
        // general floats through the same kernel (SPEC S1c).  d2a = ||q||^2 - 2w, so the window pays TWICE the error of
        // w: 2 (2^-10 + 2^-22) ||q|| ||t|| <= 2^-10 (1 + 2^-12) (||q||^2 + ||t||^2) for the two roundings, an eighth on top
        // for the matrix core's internal summation order, plus the f32 route's term for the accumulation and the norms
        g16.eps_coef_gen = static_cast<float>(9.765625e-4 * 1.125 + (6.0 * dim + 32.0) * 5.9604644775390625e-8 * 1.001);
        // ... and, in units of the SCALED accumulator: f16 subnormals flushed on either operand (2 * 2^-14 * 2^10 per
        // element) and the seed's 1/16 rounding times r / 2 <= 64, both doubled
        g16.abs_gen = static_cast<float>(dim) / 4.f + 4.f;
        g16.embed_coef = static_cast<float>(static_cast<double>(1u << lid_bits16) * 1.1920928955078125e-7 * 1.01);
    }
    // the seeded forms (round 3) of the two hint routes: LDS-DMA staging only, and the u8 route's integer candidates
    // leave 9 bits for the id (<= 2048 train rows per split, which the split rule above keeps below 64 splits)
    const int seeded_opt = opts[PM_OPT_KNN_SEEDED];
    if (route == ROUTE_U8_HINT && (lid_bits16 > U8_SHIFT || (static_cast<long long>(nt_pad) + H_TT) * U8_DP >= 0x7FFFFFFFLL ||
                                   seeded_opt == 1))
    {
        if (u8in) return p;                                     // (u8 rows: the caller widens and takes the f32 entry point)
        route = ROUTE_F16_HINT;                                 // u8-valued data satisfy the integer premise too
    }
    // rows per candidate group of the u8 route: PM_OPT_KNN_U8_GROUP 1 / 2 / 3 = 4 / 8 / 16 (0: 8)
    const int u8_group = opts[PM_OPT_KNN_U8_GROUP] == 1 ? 4 : (opts[PM_OPT_KNN_U8_GROUP] == 3 ? 16 : 8);
    // u8 refinement: integer re-evaluation on the byte copies (default) or the canonical f32 kernel (4-row groups only)
    const bool u8_int_refine = !(opts[PM_OPT_KNN_U8_REFINE] == 1 && u8_group == 4);
    // (f16 pass: the seeded form measured SLOWER than the seed chunk — C3 21.1 vs 18.7 us, 32k x 32k 199 vs 203 us: the four
    // C-in reads per block cost what the ninth MFMA cost — so it runs only when PM_OPT_KNN_SEEDED = 2 asks for it)
    const bool f16s = route == ROUTE_F16_HINT && seeded_opt == 2 && narrow &&
                      (static_cast<long long>(nt_pad) + H_TT) * (F16S_ROW16 * 16) < 0x7FFFFFFFLL;
    const bool u8r = route == ROUTE_U8_HINT;
    if (u8r) {
        g16.lid_mask = (1u << U8_SHIFT) - 1u;
        g16.int_shift = U8_SHIFT;
        g16.embed_coef = 0.f;
    }
    if (u8in && !(u8r && u8_int_refine)) return p;
    if ((want32 && lid_bits32 > 16) || (want16 && lid_bits16 > 16)) {    // > 64k rows per lane stream
        p.verdict = KNN_EXACT;
        return p;
    }

    // scratch: norms, f16 copies, candidate lists
    const size_t c32 = want32 ? sizeof(float) * static_cast<size_t>(nq) * g32.slots : 0;
    const size_t c16 = want16 ? sizeof(float) * static_cast<size_t>(nq) * g16.slots : 0;
    const size_t rowb = u8r ? U8_DP : 2 * static_cast<size_t>(f16s ? H_DP : dp16 + 16);   // bytes per row of the coarse copies
    const size_t qh = want16 ? rowb * static_cast<size_t>(nq_pad) : 0;
    const int t_wide = (u8r && u8_form >= 5) ? 1 : 0;            // 144-byte train rows with the seeds in the pad slots (knn_u8_rega)
    const size_t th = want16 ? (t_wide ? static_cast<size_t>(U8_WIDE_ROW16) * 16 : rowb) * static_cast<size_t>(nt_pad) : 0;
    const size_t sdb = (u8r || f16s) ? 4 * static_cast<size_t>(nt_pad + H_TT) : 0;       // seeds (+ one tile of slack)
    // u8 route, two-buffer coarse form (the only one that reads it): the query copy in B-fragment order too
    const size_t qfb = (u8r && u8_form <= 1) ? qh : 0;
    const size_t pkb = fuse ? sizeof(unsigned long long) * static_cast<size_t>(nq) : 0;
    p.qnorm_bytes = sizeof(float) * static_cast<size_t>(nq);
    p.tnorm_bytes = sizeof(float) * static_cast<size_t>(nt);
    p.need = knn_align256(p.qnorm_bytes) + knn_align256(p.tnorm_bytes) + knn_align256(c32) + knn_align256(c16) +
             knn_align256(qh) + knn_align256(th) + knn_align256(sdb) + knn_align256(pkb) + knn_align256(qfb) + 2048;

    p.verdict = KNN_MATRIX;
    p.route = route;
    p.want32 = want32; p.want16 = want16; p.vec = vec; p.dp16 = dp16;
    p.unit_hint = unit_hint; p.gen32 = gen32; p.f16s = f16s;
    p.u8_form = u8_form; p.u8_group = u8_group; p.u8_int_refine = u8_int_refine; p.t_wide = t_wide;
    p.qb_wg = qb_wg; p.nq_pad = nq_pad; p.nt_pad = nt_pad;
    p.g32 = g32; p.g16 = g16;
    p.splits32 = splits32; p.splits16 = splits16; p.lid_bits32 = lid_bits32; p.lid_bits16 = lid_bits16;
    p.c32 = c32; p.c16 = c16; p.qh = qh; p.th = th; p.sdb = sdb; p.qfb = qfb; p.pkb = pkb;
    p.refine8 = u8r && u8_int_refine;
    p.kf_tile = p.refine8 ? 16 : 32;                          // (refine8: one count per 16-query workgroup)

    p.prep_grid = nq_pad / 64 + nt_pad / 64;
    if (u8in) p.prep = KNN_PREP_U8ROWS;
    else if (u8r && opts[PM_OPT_KNN_PREP_ROWS] == 3) {
        p.prep = KNN_PREP8_32;
        p.prep_grid = nq_pad / 32 + nt_pad / 32;
    }
    else if (u8r && opts[PM_OPT_KNN_PREP_ROWS] != 1) {
        // 16 rows per workgroup: matcher call 23.5 -> 22.2 us at C3, 15.1 -> 14.2 at C2; with the r6 body 16 / 32 / 64 rows
        // give 19.7-20.2 / 20.0 / 21.1-21.3 us at C3 and 133.0-133.8 us alike at 32k (profiles/r06_bench_c3_ab.txt): 16 stays
        p.prep = KNN_PREP8_16;
        p.prep_grid = nq_pad / 16 + nt_pad / 16;
    }
    else if (u8r) p.prep = KNN_PREP8_64;
    else if (f16s) p.prep = KNN_PREP16_SEEDED;
    else if (unit_hint) p.prep = KNN_PREP16_UNIT;
    else if (want16) p.prep = KNN_PREP16;
    else {
        p.prep = KNN_PREP32;
        p.prep_grid = (nq + 63) / 64 + (nt + 63) / 64;
    }
    // automatic route: data that failed the integer premise get f16-ROUNDED scaled copies instead (the train scale
    // needs the norm maximum of the pass above, hence a launch of its own; it returns at once for integer data)
    p.prep_gen = (route == ROUTE_AUTO && !gen32 && !unit_hint) ? KNN_GEN_PREP16G : gen32 ? KNN_GEN_OFF : KNN_GEN_NONE;

    if (p.refine8) {
        // slots of a query per lane of its 16-lane row
        p.refine_ns = g16.slots <= 16 ? 1 : g16.slots <= 32 ? 2 : g16.slots <= 64 ? 4 : g16.slots <= 128 ? 8 : 16;
        p.refine_group = u8_group;
        p.refine_km = (fuse || k <= 2) ? 2 : 4;
        p.refine_fuse = fuse;
    } else {
        const int max_slots = (want16 ? g16.slots : 0) > (want32 ? g32.slots : 0) ? g16.slots : g32.slots;
        p.refine_ns = max_slots <= 64 ? 1 : max_slots <= 128 ? 2 : max_slots <= 256 ? 4 : 8;
        p.refine_km = k <= 2 ? 2 : 4;
        p.refine_fuse = fuse && k <= 2;
        p.refine_vec = vec;
        p.refine_gen = route == ROUTE_AUTO;
    }
    return p;
}

}  // namespace pm_knn
