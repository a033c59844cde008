// knn_shared.hpp — constants (knn_constants.hpp), index helpers and entry points shared by the two translation units of the L2
// matcher: knn_l2.hip (prep, refinement, exact kernel, C ABI) and knn_coarse.hip (the two MFMA
// coarse kernels, built with -ffinite-math-only so that the selection can use the plain
// max/med3 builtins: no canonicalising v_max per operand, and MFMA->VALU read hazards stay under
// the compiler's hazard recogniser instead of hand-placed inline asm).
#pragma once
#include "knn_constants.hpp"
#include "pm_common.hpp"

namespace pm_knn {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

// position of train row `row` (global index) in the seed array
__host__ __device__ inline int seed_pos(int row)
{
    const int i = row & 31;
    return (row & ~31) + 16 * ((i >> 2) & 1) + (i & 3) + 4 * (i >> 3);
}

// Query copy of the u8 two-buffer coarse kernel in B-FRAGMENT order: for every block of 32 queries, k-chunk c and lane
// l = 32h + r, the 16 bytes that lane l of a wave holds as its chunk-c B operand (query 32*blk + r, bytes 32c + 16h ..
// + 15).  A wave's fragment load of one chunk is then 1 KiB of contiguous memory (8 cache lines) instead of 32 lines.
// Index, in 8-byte units, of bytes 8*sub .. 8*sub + 7 of query row `row`:
__host__ __device__ inline size_t u8_qfrag_index2(int row, int sub)
{
    return ((static_cast<size_t>(row >> 5) * U8_NCH + (sub >> 2)) * 64 + ((sub >> 1) & 1) * 32 + (row & 31)) * 2 + (sub & 1);
}

// "wide" train rows of the register-operand coarse form with a split per wave (knn_u8_rega<.., WSPLIT>): 144 bytes = the
// LDS image of a row, so a 32-row block is 4.5 KiB of contiguous memory that LDS-DMA copies as it is; the 16-byte pad slot
// of row j < 8 of a block holds the block's seeds at seed-order positions 4j .. 4j+3 (a lane half's 16 C-in values are
// the pad slots of rows 4h .. 4h+3: four ds_read_b128).  Pad slots of rows 8 .. 31 are unused.
__host__ __device__ inline size_t u8_wide_seed_index(int row)           // index, in ints, into the wide train copy
{
    const int p = seed_pos(row) - (row & ~31);
    return (static_cast<size_t>(row & ~31) + (p >> 2)) * (U8_WIDE_ROW16 * 4) + U8_ROW16 * 4 + (p & 3);
}

// Enqueue the seeded coarse passes.  Q8/T8: nq_pad x 128 / nt_pad x 128 centred bytes; Qh/Th: n_pad x 128 halfs;
// seeds: nt_pad (+ H_TT slack) 4-byte seeds in seed order.  Candidates: u8 route int (w << U8_SHIFT) | id, f16s
// route float with the id in the low mantissa bits (keep_mask as on the f16 route).
// group_rows: rows per candidate group (4, 8 or 16); form: 0 / 1 two LDS tile buffers, 2 / 3 ring of 8 LDS tile buffers
// with counted waits, 4 / 5 / 6 the register-operand forms (grid and splits sized for 128 queries per workgroup; 6: one
// split per WAVE, grid.y = ceil(splits / 8)).
// Qf: the query copy in B-fragment order (u8_qfrag_index2), read by the two-buffer form (form 0 / 1) instead of Q8.
int launch_coarse_u8(pm_ctx* ctx, const void* Q8, const void* Qf, const void* T8, const int* seeds, int nq, int nq_pad, int nt,
                     int splits, int tiles_per_split, int* cval, int slots, int group_rows, int form);
int launch_coarse_f16s(pm_ctx* ctx, const _Float16* Qh, const _Float16* Th, const float* seeds, int nq, int nq_pad, int nt,
                       int splits, int tiles_per_split, unsigned keep_mask, float* cval, int slots);

// Enqueue the f32-MFMA coarse pass (dim % 4 == 0, dim <= 128).  only_if_ineligible != 0: the
// kernel runs only when prep16 flagged the data as not f16-eligible (auto route).
int launch_coarse_f32(pm_ctx* ctx, const float* dq, int nq, const float* dt, int nt, int dim, const float* tnorm,
                      int splits, int tiles_per_split, unsigned keep_mask, float* cval, int slots,
                      const unsigned long long* stats, unsigned epoch, int only_if_ineligible);
// Enqueue the exact f16-MFMA coarse pass on the padded f16 copies.  mode 1: run only if eligible.
// dp: padded data columns of the copies, 128 or 256.
int launch_coarse_f16(pm_ctx* ctx, const _Float16* Qh, const _Float16* Th, int nq, int nq_pad, int nt, int splits,
                      int tiles_per_split, unsigned keep_mask, float* cval, int slots,
                      const unsigned long long* stats, unsigned epoch, int mode, int dp = 128);

// Enqueue the i8-MFMA coarse pass of the Hamming matcher on the expanded +-1 copies.  A candidate
// is (dot << I8_SHIFT) | group id, dot = 256 - 2*hamming.
// bits: 256 (timed as knn_hamming_mfma_i8) or 512 (knn_hamming512_mfma_i8, dot = 512 - 2*hamming).
int launch_coarse_i8(pm_ctx* ctx, const void* Qe, const void* Te, int nq, int nq_pad, int nt, int splits,
                     int tiles_per_split, int* cval, int slots, int bits = I8_BITS);

}  // namespace pm_knn
