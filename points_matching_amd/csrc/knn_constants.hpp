// knn_constants.hpp — tile and row-layout constants of the L2 and Hamming matchers.  Plain C++, no HIP header: the kernels
// (through knn_shared.hpp) and the host-only route planner (knn_l2_plan.hpp) read the same definitions.
#pragma once

namespace pm_knn {

constexpr int KNN_C = 4;          // coarse candidates kept per (query, split, lane-half)
constexpr int QB = 128;           // queries per workgroup, f32 route (4 waves x 32)
constexpr int TT32 = 64;          // train rows per LDS tile, f32 route
constexpr float KNN_BIG = 3.0e38f;   // finite sentinel: stays finite under the id insert

// f16 route (integer-valued descriptors)
constexpr int H_DP = 128;               // data columns
constexpr int H_ROW = H_DP + 16;        // halfs per global row (288 B): data + seed chunk
constexpr int H_LDS_ROW = H_ROW + 8;    // halfs per LDS row (304 B: 16 rows of a lane group hit 16 slots)
constexpr int H_NCH = H_ROW / 16;       // 9 k-chunks of 16
constexpr int H_TT = 128;               // train rows per tile
constexpr int H_QB = 256;               // queries per workgroup (4 waves x 64)
constexpr float H_MAXABS = 361.f;       // 128 * 361^2 < 2^24
constexpr int H_ROW16 = H_ROW / 8;      // 16-byte units per global row (18)
constexpr int H_LDS_ROW16 = H_LDS_ROW / 8;   // 16-byte units per LDS row (19)

// i8 route (256-bit binary descriptors expanded to +-1 bytes): 256-byte rows = 8 chunks of 32 bytes,
// no seed chunk (rows padding the last tile are all-zero: dot = 0, the refinement knows them by
// their index); row groups of 8 rows
constexpr int I8_BITS = 256;
constexpr int I8_NCH = 8;
constexpr int I8_ROW16 = 16;
constexpr int I8_LDS_ROW16 = 17;        // 272-byte LDS rows: 16 rows of a lane group hit 16 different slots
constexpr int I8_GROUP_ROWS = 8;
constexpr int I8_SHIFT = 16;             // candidate = (dot << 16) | group id, |dot| <= 256
constexpr int I8_EMPTY = static_cast<int>(0x80000000u);   // an unfilled list entry
// ... and its 512-bit form (descriptors of 33 .. 64 bytes, zero-padded to 64): 512-byte rows = 16 chunks, same groups,
// same candidate layout (|dot| <= 512)
constexpr int I8W_BITS = 512;
constexpr int I8W_NCH = 16;
constexpr int I8W_ROW16 = 32;

// Seeded routes (round 3): the per-row term -||t||^2/2 no longer rides a k-chunk of its own through the matrix pipe; it
// STARTS the accumulators.  A 32-row block's 32 seeds are kept in the order of the 32x32 C/D layout ("seed order":
// position 16*h + reg <-> row (reg&3) + 8*(reg>>2) + 4*h of the block), so a lane's 16 C-in registers are four
// ds_read_b128 of a 512-byte per-tile array that is staged by one more LDS-DMA piece.  Every issued MFMA is then
// algorithmic work (2*D flop per pair).
//   u8 route   u8-valued descriptors (OpenCV SIFT: 0..255) centred to x - 128 and ranked on v_mfma_i32_32x32x32_i8:
//              128-byte rows = 4 k-chunks, exact integers; seed = -(||t - 128||^2 >> 1), so the coarse squared
//              distance ||q'||^2 - 2w is d2 or d2 - 1 (the refinement's window carries the unit);
//   f16s route integer-valued descriptors with |x| <= 361 on v_mfma_f32_32x32x16_f16: 256-byte rows = 8 chunks.
constexpr int U8_DP = 128;              // data columns (bytes) per row
constexpr int U8_NCH = 4;               // k-chunks of 32 bytes
constexpr int U8_ROW16 = 8;             // 16-byte units per global row
constexpr int U8_LDS_ROW16 = 9;         // 144-byte LDS rows: 16 rows of a lane group hit 16 different 16-byte slots
constexpr int U8_SHIFT = 9;             // candidate = (w << 9) | (group id << 1 | lane half); |w| < 2^22
constexpr int U8_PAD_SEED = -(1 << 22); // seed of the rows padding the last tile: below every real w (>= -3.13e6)
constexpr int U8_WIDE_ROW16 = 9;        // 16-byte units per "wide" train row (u8_wide_seed_index in knn_shared.hpp)
constexpr int F16S_NCH = 8;
constexpr int F16S_ROW16 = 16;
constexpr int F16S_LDS_ROW16 = 17;
constexpr int SEED_TILE_BYTES = H_TT * 4;       // one tile's seeds (128 x 4 B), seed order inside each 32-row block

}  // namespace pm_knn
