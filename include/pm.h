/* pm.h — C ABI of the MI355X-native two-view point matcher (libpm_hip.so).
 *
 * This is the drop-in boundary for the ONE hot path of wenxiaoshuai/Points-Matching:
 *   descriptor match  ->  strong-match filter  ->  point gather  ->  robust F  ->  residual report
 * i.e. `Points Matching/main.cpp:42-46, 49-69, 71-79, 89-91, 95-98, 103-123` (cited per entry
 * point below as main.cpp:N).  The reference has no FFI of its own: its boundary is the two
 * OpenCV call sites (main.cpp:46, main.cpp:95-98) plus the glue around them, so every symbol
 * here replaces one of those call sites or glue blocks.
 *
 * Conventions
 *   - plain C: pointers + sizes, no C++/torch types; every function returns a pm_status
 *     (0 = ok, <0 = error) and never throws across the boundary (the reference's OpenCV calls
 *     raise cv::Exception instead).
 *   - caller owns every buffer; the library owns only the context's scratch arena.  The arena grows on demand
 *     (one stream synchronisation and a reallocation) and never shrinks.  A block from which a call on a
 *     capturing stream took memory is not freed when the arena grows later: it is retired and freed by
 *     pm_ctx_destroy, so a recorded graph stays valid for the life of the context ("Graph capture of the
 *     estimator calls" below; pm_ctx_scratch_info).
 *   - a context is bound to one HIP device + one HIP stream and is NOT thread-safe; distinct
 *     contexts are independent.
 *   - functions without a `_dev` suffix take HOST pointers and block until the result is in
 *     the caller's buffers.  `_dev` variants take DEVICE pointers (hipMalloc'd / torch
 *     tensor .data_ptr()), enqueue on the context's stream and return without synchronising;
 *     call pm_ctx_synchronize() (or synchronise the stream you attached) before reading.
 *   - exact arithmetic (op order, tie rules, RNG) is frozen in docs/SPEC.md.
 */
#ifndef PM_H_
#define PM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PM_VERSION_MAJOR 0
#define PM_VERSION_MINOR 1

/* ---- status codes ------------------------------------------------------------------------- */
typedef enum pm_status {
    PM_OK            =  0,
    PM_E_INVALID     = -1,  /* bad argument (null pointer, negative size, k out of range ...)   */
    PM_E_TOO_FEW     = -2,  /* fewer than 8 correspondences (cv::findFundamentalMat: count<7 fails) */
    PM_E_NO_MODEL    = -3,  /* every hypothesis in the range was degenerate; F = 0, mask = 0     */
    PM_E_HIP         = -4,  /* a HIP runtime call failed; see pm_last_error()                    */
    PM_E_NOMEM       = -5,
    PM_E_UNSUPPORTED = -6
} pm_status;

/* One match record.  Mirrors cv::DMatch (OpenCV 2.4: {int queryIdx; int trainIdx; int imgIdx;
 * float distance;}) as used at main.cpp:45, :54-55, :65, :76-78, :110, :113.  16 bytes. */
typedef struct pm_match {
    int32_t queryIdx;
    int32_t trainIdx;   /* -1 when fewer than k train rows exist */
    int32_t imgIdx;     /* always 0 (single train image, as in main.cpp:46) */
    float   distance;   /* L2: sqrt of the squared distance; Hamming: bit count as float */
} pm_match;

typedef struct pm_ctx pm_ctx;   /* opaque */

/* ---- context -------------------------------------------------------------------------------
 * Replaces the implicit OpenCV global state behind main.cpp:44-46 / :95-98. */
int  pm_ctx_create(int device, pm_ctx** out);
int  pm_ctx_destroy(pm_ctx* ctx);
/* Attach an externally owned hipStream_t (passed as void*); NULL restores the context's own
 * stream.  Lets a caller time the kernels with events on its own stream. */
int  pm_ctx_set_stream(pm_ctx* ctx, void* hip_stream);
int  pm_ctx_synchronize(pm_ctx* ctx);
/* Device buffers for callers without a HIP runtime of their own (a plain-C host that wants the _dev entry points):
 * hipMalloc / hipFree on the context's device, and copies that are ordered behind the work already enqueued on the
 * context's stream and block until done.  pm_device_free synchronises the stream first; a NULL pointer is PM_OK. */
int  pm_device_alloc(pm_ctx* ctx, size_t bytes, void** d_out);
int  pm_device_free(pm_ctx* ctx, void* d_ptr);
int  pm_device_upload(pm_ctx* ctx, void* d_dst, const void* src, size_t bytes);
int  pm_device_download(pm_ctx* ctx, void* dst, const void* d_src, size_t bytes);
/* Per-kernel timing with hipEvents on the context's stream.  enable!=0 starts collecting.
 * pm_ctx_timing_get: mean milliseconds and launch count of the named kernel since the last
 * pm_ctx_timing_reset (synchronises the stream).  Names: "knn_l2_prep", "knn_l2_mfma_f16",
 * "knn_l2_mfma", "knn_l2_mfma_u8", "knn_l2_mfma_f16s", "knn_l2_refine", "knn_l2_exact", "knn_hamming_expand", "knn_hamming_mfma_i8",
 * "knn_hamming_refine", "knn_hamming512_expand", "knn_hamming512_mfma_i8", "knn_hamming512_refine", "pad_rows_u8", "knn_hamming",
 * "knn_hamming_merge", "filter_gather", "filter_cross_gather", "concat_points",
 * "ransac_fused", "ransac_finish", "ransac_solve", "ransac_score", "ransac_select", "ransac_final", "lmeds_solve", "lmeds_median",
 * "lmeds_final", "fm_count", "flann_search", "ransac_h_fused", "homography_refine", "ransac_a_fused", "affine_refine",
 * "essential_solve", "ransac_e_fused", "recover_pose", "fundamental_refine", "pose_refine", "feat_blur", "feat_decimate",
 * "feat_extrema", "feat_rank", "feat_describe", "feat_compact", "feat_gather", "pose_graph", "pgo_move_points".
 * On a capturing stream no event is recorded, whatever enable says: a call that is captured, and every replay of the
 * graph, adds nothing to pm_ctx_timing_get (time a replay with events of your own around the graph launch). */
int  pm_ctx_timing_enable(pm_ctx* ctx, int enable);
int  pm_ctx_timing_reset(pm_ctx* ctx);
int  pm_ctx_timing_get(pm_ctx* ctx, const char* kernel, double* mean_ms, int* launches);
/* Graph capture of the estimator calls.  These _dev calls keep no per-call state on the host and may be recorded into a
 * HIP graph on a capturing stream, and the graph replayed after the rows and the device-side counts in the recorded
 * buffers have changed: pm_ransac_run_dev, pm_ransac_{homography,affine,essential,pnp,align3d}_run_dev, the six
 * *_refine_dev calls, pm_recover_pose_dev, pm_triangulate_dev, pm_bundle_adjust_dev, pm_gather_pnp_dev,
 * pm_gather_align3d_dev, pm_transform_points3_dev, pm_pose_graph_optimize_dev and pm_pgo_move_points_dev
 * (pm_transform_points_dev belongs to the image family and refuses capture like the rest of it).
 *   Before recording: the *_run_dev calls take workgroup slots, candidate buffers and (E) a normalised copy from the
 *     context's scratch arena, and a context's first such call allocates the arrival words.  Neither can happen on a
 *     capturing stream, so make ONE EAGER CALL of the same or a larger shape (capacity, id range, PM_OPT_RANSAC_WG_IDS)
 *     on this context first.  A call that finds the stream capturing and would have to grow the arena or allocate the
 *     words returns PM_E_UNSUPPORTED, with a message that says so, before it allocates, synchronises or enqueues
 *     anything; the capture stays valid, the outputs are untouched and the context works as before.  The refinements,
 *     pose recovery, triangulation, the gathers and the transform take no scratch and need no such call.
 *   What a recorded graph may outlive: any later call on the context, including one that grows the arena (a larger frame
 *     of pm_stereo_sgm_dev, a larger matcher call, a larger capacity here).  The block the graph's nodes point into is then
 *     retired, not freed; the new block is at least twice as large, so the retired blocks together stay below the live
 *     one.  They are freed by pm_ctx_destroy: destroy the graph first.  Calls recorded in one graph share the arena the
 *     way eager calls do: each *_run_dev carves it from the start, so only stream order (a single chain, one stream)
 *     keeps two of them apart.
 *   Timing: see pm_ctx_timing_enable: nothing is recorded on a capturing stream.
 * pm_ctx_scratch_info: the arena's capacity in bytes and the number of retired blocks (either pointer may be NULL).
 * Reads the context only: no device call, allowed during a capture. */
int  pm_ctx_scratch_info(pm_ctx* ctx, size_t* capacity_bytes, int* retired_blocks);
/* Diagnostics of the MFMA route of pm_bf_knn_l2_f32[_dev]: while enabled, each call records how
 * many queries took the exact re-scan branch of the refinement and whether a non-finite input
 * was seen; pm_ctx_knn_stats returns the values of the last such call (synchronises). */
int  pm_ctx_knn_diag_enable(pm_ctx* ctx, int enable);
int  pm_ctx_knn_stats(pm_ctx* ctx, int* rescans, int* nonfinite);
/* ... and which coarse pass the refinement of the last such call read: 0 = f16 matrix pass on exact integer copies,
 * 1 = f16 matrix pass on rounded copies of general floats, 2 = f32-input matrix pass, 3 = i8 matrix pass on centred
 * u8-valued copies (synchronises). */
int  pm_ctx_knn_route(pm_ctx* ctx, int* route);
/* pm_bf_knn_l2_ratio_dev in its fused form (no record buffer / PM_OPT_FILTER_FUSION = 2) compacts with bounded look-back
 * polls.  *gave_up != 0: a poll of the LAST such call on this context ran out — that call's survivors and count are not to
 * be used (never observed on hardware; the two-launch form has an always-correct fallback instead).  Synchronises. */
int  pm_ctx_filter_fusion_status(pm_ctx* ctx, int* gave_up);
/* Explicit per-context switches for tests and A/B timing (the library reads no environment variables).
 * Every option defaults to 0 = automatic; a value outside an option's range is PM_E_INVALID. */
enum {
    PM_OPT_RANSAC_PATH    = 1,  /* 1: hypothesis-per-lane kernels (solve + score launches), 2: one-launch kernel  */
    PM_OPT_SCORE_OPERANDS = 2,  /* hypothesis-per-lane scorer: 1 LDS-staged points, 2 scalar-operand pair records */
    PM_OPT_HAMMING_ROUTE  = 3,  /* 1: integer-VALU scan, 2: matrix-core route with 64-bit refinement keys          */
    PM_OPT_KNN_F16_WAVES  = 4,  /* f16/i8 coarse kernel: 1 = 8 waves x 32 queries, 2 = 4 waves x 64 queries,
                                   3 (f16 only) = 8 waves x 64 queries in two row groups                         */
    PM_OPT_KNN_STAGING    = 6,  /* f16/i8 coarse kernel, train tiles: 1 = through registers, 2 = LDS-DMA (default)  */
    PM_OPT_KNN_WG_PER_CU  = 7,  /* f16 coarse kernel: train splits sized for 1 (default) or 2 workgroups per CU     */
    PM_OPT_FILTER_FUSION  = 5,  /* pm_bf_knn_l2_ratio_dev: 1 = filter as its own launch, 2 = inside the refinement  */
    PM_OPT_KNN_XCD_TILE   = 8,  /* coarse kernels, workgroup order: 1 = launch order, 2 = one 2-D grid tile per XCD     */
    PM_OPT_KNN_GENERAL_F16 = 9, /* automatic L2 route on general floats: 1 = f32-input matrix pass (enqueued next to the
                                   f16 one), 2 = f16-rounded scaled copies, wider refinement window (default)   */
    PM_OPT_KNN_SEEDED     = 10, /* f16 hint route, row term -||t||^2/2: 1 = a k-chunk of its own (9 chunks, default: faster), 2 =
                                   starts the accumulators from a per-tile LDS array (8 chunks).  1 also sends PM_KNN_HINT_U8
                                   to the f16 pass (the u8 route exists in the seeded form only)                    */
    PM_OPT_KNN_U8_GROUP   = 11, /* u8 route: rows per coarse candidate group, 1 = 4, 2 = 8 (default), 3 = 16                 */
    PM_OPT_KNN_RING       = 12, /* u8 coarse kernel, train tiles: 1 = two LDS buffers (default), 2 = ring of eight with counted
                                   waits and a workgroup barrier per tile, 3 = the ring with split-phase LDS counters
                                   (2, 3: 8-row groups only; measured, not faster: DESIGN.md 2.1); register-operand forms
                                   (8-row groups only): a wave keeps 128 queries as B operands and takes 32-row blocks of
                                   train rows by itself, no tile is shared between waves: 4 = blocks straight from global
                                   memory, 5 = through a private LDS buffer per wave (LDS-DMA), 6 = 5 with one train split
                                   per WAVE (no merge, no barrier; long sweeps only, else form 1 runs)               */
    PM_OPT_KNN_U8_REFINE  = 13, /* u8 route refinement: 1 = canonical f32 kernel (4-row groups only), 2 = integer
                                   re-evaluation on the byte copies, one lane per row (default)                     */
    PM_OPT_KNN_RING_PROLOGUE = 14, /* u8 ring kernel: train tiles requested before the sweep starts, 2 .. 8 (default 2)    */
    PM_OPT_KNN_WIDE       = 15, /* L2 matcher beyond dim % 4 == 0 && dim <= 128 && 16-byte aligned rows: 1 = exact VALU kernel (round 2),
                                   2 = f16 matrix passes on padded copies, up to 256 dimensions (default)             */
    PM_OPT_KNN_PREP_ROWS  = 16, /* u8 route, prep kernel: 1 = 64 rows per workgroup, 2 = 16 rows per workgroup (default), 3 = 32 */
    PM_OPT_RANSAC_FORM    = 17, /* one-launch RANSAC kernel: 1 = correspondences in registers, two teams of four waves (round 2),
                                   2 = correspondences in LDS, one wave per hypothesis, 12 waves (default)           */
    PM_OPT_RANSAC_WG_IDS  = 18, /* one-launch RANSAC kernel: hypothesis ids per workgroup.  0 = automatic (ids spread over ALL
                                   CUs: lowest latency for one run; a pm_batch lane defaults to 32 instead), 1 .. 128 = that
                                   many: fewer, fuller workgroups, so the runs of several streams share the GPU — the fp64
                                   solve costs a wave the same ~21k cycles whether 8 or 64 of its lanes are in use       */
    PM_OPT_HAMMING_REFINE = 19, /* Hamming matrix-core route, refinement: 1 = one wave per query (round 1), 2 = four queries per
                                   wave, one 16-lane row each (default where a query has <= 64 candidate entries); in both
                                   the rare whole-sub-list scans are done by the whole workgroup                       */
    PM_OPT_KNN_SUPERTILE  = 20, /* u8 coarse kernel, two-buffer form, 8-row groups: 128-row tiles per LDS buffer and per
                                   workgroup barrier, 1 = one (default), 2 = two, 3 = four; timed as knn_l2_mfma_u8,
                                   knn_l2_mfma_u8_s2, knn_l2_mfma_u8_s4 (measured, not faster: DESIGN.md 2.1)        */
    PM_OPT_FEAT_CAPACITY  = 21, /* pm_detect_describe[_dev]: candidate (DoG extremum) capacity of a run, 1 .. 2^28; 0 = automatic:
                                   max(65536, 8 * max_kp).  See the overflow rule at pm_detect_describe_dev                */
    PM_OPT_COUNT_         = 22
};
int  pm_ctx_set_option(pm_ctx* ctx, int option, int value);
int  pm_ctx_get_option(pm_ctx* ctx, int option, int* value);
const char* pm_last_error(void);       /* thread-local text of the last PM_E_HIP / PM_E_* */
const char* pm_status_string(int status);
int  pm_version(void);                 /* major*100 + minor */

/* ---- descriptor matching (replaces main.cpp:46 `matcher.match(imageDesc1, imageDesc2, ...)`,
 *      matcher = BruteForceMatcher<L2<float>> of the commented main.cpp:43, generalised to k-NN)
 *
 * q: nq x dim row-major float (imageDesc1), t: nt x dim row-major float (imageDesc2).
 * out: nq*k records, row i at out[i*k .. i*k+k-1], ascending by (distance bits, trainIdx):
 *      smaller distance first, equal distances -> lower trainIdx first (SPEC S3).
 *      If nt < k the tail of each row has trainIdx = -1, distance = +inf.
 * 1 <= k <= PM_MAX_K.  nq == 0 is ok (no output).  nt == 0 gives all -1 rows.
 * `flags`: 0 = automatic.  For dim%4==0 && dim<=128 && k<=2: MFMA coarse pass + canonical
 *          refinement; the coarse pass is the exact f16-MFMA route when the data are integer-valued
 *          (decided on the device, no host round trip: both coarse kernels are enqueued and the one
 *          that does not apply exits at once) and the f32-MFMA route otherwise.  Anything else:
 *          exact VALU kernel.  All routes produce bit-identical output (tests assert it). */
/* Device pointers of the _dev form: rows are read as 16-byte vectors when dim % 4 == 0 and both base pointers are
 * 16-byte aligned (hipMalloc / torch allocations are); otherwise the call takes the exact scalar-load kernel. */
/* Train-set size regimes (nt = train rows; every size nt >= 0 is accepted and every regime returns the same records,
 * bit for bit — tests/test_knn_large_train_gpu.py).  The matrix routes cut the train set into at most 64 splits of whole
 * tiles (128 rows, f32 route 64 rows), so above 131072 rows a split is ceil(tiles / 64) tiles long:
 *   nt <= 131072        splits of at most 2048 rows; the candidate's row-group id takes 9 low mantissa bits.
 *   nt >  131072        the id takes 10 .. 16 bits (11 at 300 001 rows, 13 at 1.2 M, 15 at 7.4 M) and the refinement window
 *                       widens by 2^(bits - 23) (||q||^2 + 2 max ||t||^2): more candidates, more lists scanned exactly (on
 *                       4-dimensional rows at 7.4 M nearly every list).  PM_KNN_HINT_U8 is served by
 *                       the f16 integer route (its integer candidates leave 9 bits for the id), and pm_bf_knn_l2_u8* widen
 *                       the bytes to float on the device and take that route too (scratch: 4 bytes per element).
 *   nt >  7 456 412     (dim <= 128; (nt + 128) * 288 bytes pass 2 GiB) the f16 copies are staged through registers
 *                       instead of LDS-DMA.  (PM_OPT_KNN_SEEDED = 2, an LDS-DMA-only kernel on 256-byte rows, is honoured up
 *                       to 8 388 352 rows and ignored above.)
 *   nt >  16 777 216    more than 16 id bits: the whole call takes the exact VALU kernel (about 1.2 s for 131 queries of
 *                       4 floats at that size, against 0.2 s one row below).
 * Scratch of the matrix routes: 288 bytes per train row (f16 copy, dim <= 128), kept by the context. */
#define PM_MAX_K 16
#define PM_KNN_FORCE_EXACT  1   /* exact VALU kernel only                                           */
#define PM_KNN_FORCE_F32    2   /* f32-MFMA coarse route only (any finite floats)                   */
#define PM_KNN_HINT_INTEGER 4   /* caller states the descriptors are integer-valued with |x| <= 361 */
                                /* (OpenCV SIFT: 0..255): only the exact f16-MFMA coarse route is   */
                                /* launched.  The claim is verified on the device; a wrong hint     */
                                /* costs time (exact re-scan), never correctness.                   */
#define PM_KNN_HINT_U8      8   /* caller states the descriptors are integers in [0, 255] (OpenCV SIFT):  */
                                /* ranked on the i8 matrix cores (x - 128, 4 k-chunks at D = 128, twice   */
                                /* the f16 rate).  Verified on the device like PM_KNN_HINT_INTEGER.        */
#define PM_KNN_HINT_UNIT_NORM 16 /* caller states that every TRAIN row has ||t||^2 <= 1 + 2^-10 (SURF, L2-normalised      */
                                /* descriptors: what main.cpp:37-40 itself produces): general floats, ranked on the      */
                                /* f16 matrix pass with ONE prep launch instead of two (the train scale needs no norm    */
                                /* maximum).  Verified on the device; a wrong hint costs time (exact re-scan).           */
int pm_bf_knn_l2_f32(pm_ctx* ctx, const float* q, int nq, const float* t, int nt,
                     int dim, int k, int flags, pm_match* out);
int pm_bf_knn_l2_f32_dev(pm_ctx* ctx, const float* d_q, int nq, const float* d_t, int nt,
                         int dim, int k, int flags, pm_match* d_out);

/* The same matcher on u8 DESCRIPTOR ROWS (nq x dim / nt x dim bytes, 4-byte aligned device pointers in the _dev forms):
 * what a SIFT extractor holds before it widens to float, a quarter of the bytes on the host link (BASELINE config 5).
 * Output = pm_bf_knn_l2_f32 on the same values converted to float, bit for bit (distances are the canonical f32 ones).
 * dim % 4 == 0, dim <= 128, k <= 4: the u8 route (i8 matrix cores on x - 128, integer refinement); anything else is
 * widened on the device and takes the f32 matcher.  pm_bf_knn_l2_u8_ratio_dev: + ratio test + compaction + gather, as
 * pm_bf_knn_l2_ratio_dev (the record buffer d_knn is required). */
int pm_bf_knn_l2_u8(pm_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, int dim, int k, pm_match* out);
int pm_bf_knn_l2_u8_dev(pm_ctx* ctx, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int dim, int k, pm_match* d_out);
int pm_bf_knn_l2_u8_ratio_dev(pm_ctx* ctx, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int dim, float ratio,
                              const float* d_kp1_xy, const float* d_kp2_xy, pm_match* d_knn, pm_match* d_good,
                              float* d_xy1, float* d_xy2, int32_t* d_n_good);

/* main.cpp:46 + :49-69 (ratio form) + :77-78 + :89-91 in ONE call for batches that stay in HBM: 2-NN, ratio test
 * (d1 < ratio * d2, float multiply, strict), stable compaction in query order and keypoint gather — the outputs of
 * pm_bf_knn_l2_f32_dev(k = 2) followed by pm_filter_ratio_gather_dev, bit for bit.  d_knn (nq x 2 records) may be
 * NULL on the MFMA routes: the filter then rides the refinement launch and no record is written (shapes that take
 * the exact kernel — dim % 4 != 0, dim > 128, unaligned rows — need the buffer).  With d_knn the filter is its own
 * launch, which measured faster, except with PM_KNN_HINT_U8 up to 768 queries, where the fused launch
 * is 1.6-2.9 us shorter and is taken; PM_OPT_FILTER_FUSION pins either form.
 * Graph capture: the matcher and the compaction calls (pm_bf_knn_l2_*, pm_filter_*_gather_dev) pass a per-call epoch
 * as a kernel argument and therefore return PM_E_UNSUPPORTED on a stream that is capturing (a replay would reuse the
 * epoch); enqueue them directly — a replay measured slower than direct launches anyway.
 * Limit: the two-launch form ends in pm_filter_ratio_gather_dev and inherits its limit of 1 048 576 query rows per call
 * (PM_E_UNSUPPORTED above it, after the matcher has run); so do shapes that take the exact kernel.  The fused form on
 * the MFMA routes has no such limit: its per-context count words grow with nq (one stream synchronisation and a
 * reallocation when a call needs more than 4096 tiles of 32 queries, 16 on the u8 route, for the first time). */
int pm_bf_knn_l2_ratio_dev(pm_ctx* ctx, const float* d_q, int nq, const float* d_t, int nt, int dim, int flags,
                           float ratio, const float* d_kp1_xy, const float* d_kp2_xy, pm_match* d_knn,
                           pm_match* d_good, float* d_xy1, float* d_xy2, int32_t* d_n_good);

/* ---- approximate matcher compatible with `FlannBasedMatcher matcher;` (main.cpp:44, the reference's ACTIVE matcher,
 * called at main.cpp:46) — SURVEY.md 8f-4, docs/SPEC.md S17.  cv::flann defaults: 4 randomised kd-trees
 * (KDTreeIndexParams(4)), 32 checks, eps 0, sorted results (SearchParams(32, 0, true)).  The forest is built on the
 * host from the train descriptors (every random draw comes from a counter-based stream keyed by `seed`, not from C
 * rand(): reproducible everywhere), uploaded once, and searched on the GPU (one lane per query, best-bin-first over
 * all trees with one heap).  Output records like pm_bf_knn_l2_f32 (distance = sqrt of the canonical squared L2), rows
 * ascending; with fewer than k examined points the tail has trainIdx = -1.  1 <= k <= 4.
 * Approximate by design: tests report recall against the exact matcher; the exact matcher is also faster at the
 * reference's sizes, so this path exists for behavioural compatibility (pm_cli --matcher flann). */
typedef struct pm_flann_params {
    int32_t  trees;     /* <= 0: 4 */
    int32_t  checks;    /* <= 0: 32 */
    uint64_t seed;
} pm_flann_params;
typedef struct pm_flann_index pm_flann_index;   /* opaque; bound to the context's device */
int pm_flann_build(pm_ctx* ctx, const float* train, int nt, int dim, const pm_flann_params* prm, pm_flann_index** out);
int pm_flann_destroy(pm_flann_index* ix);
int pm_flann_knn_l2_f32(pm_ctx* ctx, pm_flann_index* ix, const float* q, int nq, int k, pm_match* out);
int pm_flann_knn_l2_f32_dev(pm_ctx* ctx, pm_flann_index* ix, const float* d_q, int nq, int k, pm_match* d_out);
/* The forest as built (tests, inspection): *n_nodes records of 16 bytes {int32 child1, child2 (-1: leaf), int32 cut
 * dimension | point id of a leaf, float cut value}; roots[t] = root record of tree t.  nodes may be NULL (size query). */
int pm_flann_export(const pm_flann_index* ix, int32_t* n_nodes, int32_t* roots, void* nodes, int32_t cap_nodes);

/* Binary descriptors (ORB-256 = 32 bytes/row, BRISK / FREAK / BRIEF-64 = 64): Hamming distance, popcount of XOR.
 * `bytes` must be a positive multiple of 4 (other lengths, AKAZE's 61 bytes: pm_pad_rows_u8 below).  Replaces main.cpp:46
 * for BASELINE config C4.  With k <= 2 two lengths run on the matrix cores (+-1 expansion on i8 MFMA + popcount
 * refinement): 32-byte descriptors in 16-byte-aligned device buffers (256 bits, 8 k-chunks), and descriptors of 36 .. 64
 * bytes in any 4-byte-aligned buffers (512 bits, 16 k-chunks: rows are zero-padded to 64 bytes by the expansion launch,
 * which leaves every distance as it is — SPEC S51).  Everything else (k > 2, bytes < 32, bytes > 64, 32-byte rows in
 * unaligned buffers) runs on the integer VALU scan; same output on every route.
 * Train-set size regimes of the matrix-core route (same records in all of them): at most 64 splits of whole 128-row tiles;
 * above 8 388 479 rows ((nt + 128) * 256 bytes pass 2 GiB) the +-1 byte copies are staged through registers instead of
 * LDS-DMA; from 2^23 = 8 388 608 rows on the refinement's keys are 64-bit (below: distance << 23 | row); above
 * 33 554 432 rows a split has more than 2^16 candidate ids and the call takes the VALU scan (about 0.34 s for 67 queries at
 * that size against 11 ms one row below).  Scratch: 256 bytes per train row, kept by the context.
 * The 512-bit route (36 .. 64 bytes) has the same structure with its own limits: scratch 512 bytes per train row (+ 64
 * for the padded packed copy when bytes < 64 or a buffer is not 16-byte aligned); above 4 194 175 rows ((nt + 128) * 512
 * bytes pass 2 GiB) the +-1 copies are staged through registers instead of LDS-DMA; the refinement's keys are
 * distance << 22 | row below 2^22 = 4 194 304 rows (a distance of 512 needs the 10th bit) and 64-bit from there on; above
 * 33 554 432 rows the call takes the VALU scan, as on the 256-bit route.  Tested (tests/test_knn_hamming_wide_gpu.py):
 * 4 194 175, 4 194 176, 4 194 303, 4 194 304 and 4 194 400 rows, i.e. both staging forms and both key widths.  NOT tested:
 * anything larger, in particular the fall-back to the scan above 33 554 432 rows (17 GiB of scratch).
 * Timing names of the 512-bit route: "knn_hamming512_expand", "knn_hamming512_mfma_i8", "knn_hamming512_refine". */
int pm_bf_knn_hamming_u8(pm_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt,
                         int bytes, int k, pm_match* out);
int pm_bf_knn_hamming_u8_dev(pm_ctx* ctx, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt,
                             int bytes, int k, pm_match* d_out);

/* Rows of any byte count for the Hamming matcher: copies n rows of `bytes` bytes into rows of dst_bytes >= bytes bytes
 * and zeroes the tail of each.  Equal zero padding on both sides of a match leaves every Hamming distance unchanged
 * (AKAZE's 61-byte M-LDB rows -> 64).  src may have any alignment; src and dst must not overlap.  PM_E_INVALID: a null
 * pointer with n > 0, bytes < 1, dst_bytes < bytes.  n == 0 is PM_OK.  The _dev form is one launch ("pad_rows_u8"). */
int pm_pad_rows_u8(const uint8_t* src, int n, int bytes, uint8_t* dst, int dst_bytes);
int pm_pad_rows_u8_dev(pm_ctx* ctx, const uint8_t* d_src, int n, int bytes, uint8_t* d_dst, int dst_bytes);

/* ---- strong-match filters (the slot of main.cpp:49-69) -------------------------------------
 * Host-side, O(n).  `out` must hold n (resp. nq) records; survivors keep query order. */

/* Literal main.cpp:49-69: minMatch starts at 1, maxMatch at 0 (main.cpp:49-50); keep i iff
 * (double)distance < minMatch + (maxMatch - minMatch) / 2  (strict, in double, main.cpp:65).
 * min_out/max_out receive the two values the reference prints at main.cpp:58-59. */
int pm_filter_midpoint(const pm_match* m, int n, double* min_out, double* max_out,
                       pm_match* out, int* n_out);
/* Ratio test on k-NN rows (k >= 2): keep row i iff knn[i*k+1].trainIdx >= 0 and
 * knn[i*k].distance < ratio * knn[i*k+1].distance (float multiply, strict).  Emits knn[i*k]. */
int pm_filter_ratio(const pm_match* knn, int nq, int k, float ratio, pm_match* out, int* n_out);
/* Device-resident fusion of pm_filter_ratio + pm_match_indices + pm_gather_points (main.cpp:49-69,
 * :77-78, :89-91) for batches that stay in HBM between the matcher and RANSAC: stable compaction
 * in query order.  d_good: nq records; d_xy1/d_xy2: nq x 2 floats (may be NULL together with the
 * keypoint arrays when only the match list is wanted); *d_n_good: survivor count (device int).
 * Limit: at most 1 048 576 query rows per call (4096 blocks of 256 rows share one set of per-context count words);
 * more returns PM_E_UNSUPPORTED before anything is enqueued and leaves the outputs and the context as they were. */
int pm_filter_ratio_gather_dev(pm_ctx* ctx, const pm_match* d_knn, int nq, int k, float ratio,
                               const float* d_kp1_xy, const float* d_kp2_xy, pm_match* d_good,
                               float* d_xy1, float* d_xy2, int32_t* d_n_good);
/* The reference's own strong-match rule (main.cpp:49-69, what pm_filter_midpoint does on the host)
 * in the same device-resident form: record i of d_m is d_m[i*k] (k = 1 for a 1-NN match list);
 * d_minmax (may be NULL) receives minMatch / maxMatch as two doubles (main.cpp:58-59).
 * Limit: n <= 1 048 576 rows per call, as for pm_filter_ratio_gather_dev (PM_E_UNSUPPORTED above it). */
int pm_filter_midpoint_gather_dev(pm_ctx* ctx, const pm_match* d_m, int n, int k,
                                  const float* d_kp1_xy, const float* d_kp2_xy, pm_match* d_good,
                                  float* d_xy1, float* d_xy2, int32_t* d_n_good, double* d_minmax);
/* ---- cross-check (cv::BFMatcher(norm, crossCheck = true): mutual nearest neighbours) — docs/SPEC.md S41-S42 --------
 * fwd: nq x kf records, the matcher's output for (q, t); rev: nt x kr records, the matcher's output for (t, q), so its
 * trainIdx names a QUERY row.  Row i survives iff j = fwd[i*kf].trainIdx lies in [0, nt), rev[j*kr].trainIdx == i, and
 * with PM_CROSS_RATIO_FWD row i of fwd / with PM_CROSS_RATIO_REV row j of rev also passes the ratio test of
 * pm_filter_ratio (d1 < ratio * d2, second neighbour present).  Survivors keep query order and emit fwd[i*kf]
 * unchanged; their trainIdx are pairwise distinct (a one-to-one matching).  Indices only are compared: ties were
 * settled by the matcher in both directions (lower index first). */
#define PM_CROSS_RATIO_FWD 1    /* + ratio test on the forward row (needs kf >= 2) */
#define PM_CROSS_RATIO_REV 2    /* + ratio test on the reverse row (needs kr >= 2) */
/* Host-side, O(nq).  out holds nq records.  PM_E_INVALID: kf / kr < 1 or too small for cross_flags, unknown flag bits,
 * null arrays.  nq == 0 or nt == 0: no survivor.  ratio is read only with a PM_CROSS_RATIO_* flag. */
int pm_filter_cross(const pm_match* fwd, int nq, int kf, const pm_match* rev, int nt, int kr,
                    int cross_flags, float ratio, pm_match* out, int* n_out);
/* Device-resident form: the rule above + stable compaction in query order + keypoint gather in ONE launch (a third
 * predicate of the pm_filter_ratio_gather_dev kernel; a trainIdx outside [0, nt) is a drop, never an address).  Output
 * contract of pm_filter_ratio_gather_dev: d_good nq records, d_xy1 / d_xy2 nq x 2 floats (NULL together with the
 * keypoint arrays), *d_n_good the survivor count.  d_xy1 row = d_kp1_xy[i], d_xy2 row = d_kp2_xy[j].  Timed as
 * "filter_cross_gather".  Refused on a capturing stream like the other compaction calls.
 * Limit: nq <= 1 048 576 rows per call, as for pm_filter_ratio_gather_dev (PM_E_UNSUPPORTED above it; nt is not
 * limited). */
int pm_filter_cross_gather_dev(pm_ctx* ctx, const pm_match* d_fwd, int nq, int kf, const pm_match* d_rev, int nt, int kr,
                               int cross_flags, float ratio, const float* d_kp1_xy, const float* d_kp2_xy,
                               pm_match* d_good, float* d_xy1, float* d_xy2, int32_t* d_n_good);
/* One-call forms (S42), everything on the context's stream with no host round trip: forward pass pm_bf_knn_*_dev(q, t)
 * with k = 2 if PM_CROSS_RATIO_FWD else 1 into d_fwd, reverse pass pm_bf_knn_*_dev(t, q) with k = 2 if
 * PM_CROSS_RATIO_REV else 1 into d_rev, then pm_filter_cross_gather_dev — the outputs of those three calls, bit for
 * bit.  d_fwd (nq x kf) and d_rev (nt x kr) are caller-owned record buffers and hold the two k-NN lists afterwards.
 * knn_flags (pm_bf_knn_l2_f32_dev) go to both passes, except PM_KNN_HINT_UNIT_NORM, a statement about the train rows
 * only, which the reverse pass does not receive.  The reverse pass is a second full matcher run.  nq == 0 or nt == 0:
 * no survivor, PM_OK.  The survivor arrays feed a pm_points_view {d_xy1, d_xy2, counts = d_n_good} like those of
 * pm_bf_knn_l2_ratio_dev.  Refused on a capturing stream before anything is enqueued. */
int pm_bf_match_cross_l2_f32_dev(pm_ctx* ctx, const float* d_q, int nq, const float* d_t, int nt, int dim, int knn_flags,
                                 int cross_flags, float ratio, const float* d_kp1_xy, const float* d_kp2_xy,
                                 pm_match* d_fwd, pm_match* d_rev, pm_match* d_good, float* d_xy1, float* d_xy2,
                                 int32_t* d_n_good);
int pm_bf_match_cross_l2_u8_dev(pm_ctx* ctx, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int dim,
                                int cross_flags, float ratio, const float* d_kp1_xy, const float* d_kp2_xy,
                                pm_match* d_fwd, pm_match* d_rev, pm_match* d_good, float* d_xy1, float* d_xy2,
                                int32_t* d_n_good);
int pm_bf_match_cross_hamming_u8_dev(pm_ctx* ctx, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int bytes,
                                     int cross_flags, float ratio, const float* d_kp1_xy, const float* d_kp2_xy,
                                     pm_match* d_fwd, pm_match* d_rev, pm_match* d_good, float* d_xy1, float* d_xy2,
                                     int32_t* d_n_good);
/* Host conveniences (upload, run, download; block like pm_bf_knn_l2_f32): out holds up to nq records, *n_out their
 * number. */
int pm_bf_match_cross_l2_f32(pm_ctx* ctx, const float* q, int nq, const float* t, int nt, int dim, int knn_flags,
                             int cross_flags, float ratio, pm_match* out, int* n_out);
int pm_bf_match_cross_l2_u8(pm_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, int dim, int cross_flags,
                            float ratio, pm_match* out, int* n_out);
int pm_bf_match_cross_hamming_u8(pm_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, int bytes,
                                 int cross_flags, float ratio, pm_match* out, int* n_out);

/* ---- guided matching: k-NN restricted by a two-view model (docs/SPEC.md S48-S50) ------------------------------------
 * The step after the first model estimate (COLMAP's guided matching, ORB-SLAM's search along the epipolar line, the
 * `mask` argument of cv::BFMatcher::knnMatch): query row i, keypoint d_kp1_xy[i], is matched against the train rows j
 * whose keypoint d_kp2_xy[j] agrees with the model only — the fp32 inlier test of the RANSAC scorers (S8 / S21) on the
 * pair (kp1[i], kp2[j]) with threshold tau (pixels) — and the nq x nt mask is never built.  One launch, timed as
 * "knn_guided"; the matrix cores are not used.
 *   kind   PM_GUIDE_F_SAMPSON / PM_GUIDE_F_SYM: M is a fundamental matrix, test of PM_ERR_SAMPSON / PM_ERR_SYM_EPIPOLAR;
 *          PM_GUIDE_H: M is a homography taking image 1 to image 2, test of PM_ERR_REPROJ.  An essential matrix is
 *          used as F = K^-T E K^-1; there is no affine gate.
 *   d_M    DEVICE pointer to 9 doubles, row-major, rounded once to float: the d_F of pm_ransac_run_dev /
 *          pm_fundamental_refine_dev or the d_H of pm_ransac_homography_run_dev / pm_homography_refine_dev, on the same
 *          stream with no synchronisation in between.  A model with a non-finite entry or with nine zeros (what the
 *          *_run_dev calls leave behind when they find no model) admits nothing.
 *   d_out  nq x k records, 1 <= k <= 4: the k nearest ADMITTED rows in the order of the plain matchers (distance, then
 *          lower trainIdx); rows with fewer than k admitted train rows end in trainIdx = -1, distance = +inf.
 *          Distances are those of pm_bf_knn_l2_f32 / pm_bf_knn_l2_u8 / pm_bf_knn_hamming_u8, bit for bit (a NaN distance
 *          is reported as the quiet NaN 0x7FC00000).
 *   d_n_admitted  (may be NULL) nq int32: the number of train rows the gate admitted for each query.
 * Keypoint arrays and d_M are 8-byte aligned, float and binary descriptor buffers 4-byte aligned; `bytes` is a multiple
 * of 4.  A descriptor row the gate did not admit is never read.  PM_E_INVALID: null pointers, k outside [1, 4], unknown
 * kind, dim < 1, bytes % 4 != 0.  nq == 0: PM_OK, nothing written.  nt == 0: every row is -1 / +inf, d_n_admitted 0.
 * These calls carry no per-call epoch and may be captured into a graph. */
enum { PM_GUIDE_F_SAMPSON = 0, PM_GUIDE_F_SYM = 1, PM_GUIDE_H = 2 };
int pm_bf_knn_guided_l2_f32_dev(pm_ctx* ctx, const float* d_q, int nq, const float* d_t, int nt, int dim,
                                const float* d_kp1_xy, const float* d_kp2_xy, int kind, const double* d_M, float tau, int k,
                                pm_match* d_out, int32_t* d_n_admitted);
int pm_bf_knn_guided_l2_u8_dev(pm_ctx* ctx, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int dim,
                               const float* d_kp1_xy, const float* d_kp2_xy, int kind, const double* d_M, float tau, int k,
                               pm_match* d_out, int32_t* d_n_admitted);
int pm_bf_knn_guided_hamming_u8_dev(pm_ctx* ctx, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int bytes,
                                    const float* d_kp1_xy, const float* d_kp2_xy, int kind, const double* d_M, float tau,
                                    int k, pm_match* d_out, int32_t* d_n_admitted);
/* One-call guided matching (S50): guided 2-NN into d_knn (nq x 2 records, required), then pm_filter_ratio_gather_dev on
 * it — the outputs of those two calls, bit for bit, with the output contract of pm_bf_knn_l2_ratio_dev: d_good nq
 * records, d_xy1 / d_xy2 nq x 2 floats (NULL together when only the match list is wanted), *d_n_good the survivor
 * count; they feed a pm_points_view {d_xy1, d_xy2, counts = d_n_good}.  A query with a SINGLE admitted train row has no
 * second neighbour and is dropped by the ratio test like any row without one; callers who want such matches take the
 * k = 1 list of pm_bf_knn_guided_*_dev.  The compaction carries a per-call epoch: on a capturing stream these calls
 * return PM_E_UNSUPPORTED before anything is enqueued, and so they do for nq > 1 048 576 (the compaction's limit). */
int pm_bf_match_guided_l2_f32_dev(pm_ctx* ctx, const float* d_q, int nq, const float* d_t, int nt, int dim,
                                  const float* d_kp1_xy, const float* d_kp2_xy, int kind, const double* d_M, float tau,
                                  float ratio, pm_match* d_knn, pm_match* d_good, float* d_xy1, float* d_xy2,
                                  int32_t* d_n_good);
int pm_bf_match_guided_l2_u8_dev(pm_ctx* ctx, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int dim,
                                 const float* d_kp1_xy, const float* d_kp2_xy, int kind, const double* d_M, float tau,
                                 float ratio, pm_match* d_knn, pm_match* d_good, float* d_xy1, float* d_xy2,
                                 int32_t* d_n_good);
int pm_bf_match_guided_hamming_u8_dev(pm_ctx* ctx, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt, int bytes,
                                      const float* d_kp1_xy, const float* d_kp2_xy, int kind, const double* d_M, float tau,
                                      float ratio, pm_match* d_knn, pm_match* d_good, float* d_xy1, float* d_xy2,
                                      int32_t* d_n_good);
/* Host conveniences (upload, run, download; block like pm_bf_knn_l2_f32): everything in host memory, M nine doubles,
 * out nq x k records, n_admitted (may be NULL) nq int32. */
int pm_bf_knn_guided_l2_f32(pm_ctx* ctx, const float* q, int nq, const float* t, int nt, int dim, const float* kp1_xy,
                            const float* kp2_xy, int kind, const double M[9], float tau, int k, pm_match* out,
                            int32_t* n_admitted);
int pm_bf_knn_guided_l2_u8(pm_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, int dim, const float* kp1_xy,
                           const float* kp2_xy, int kind, const double M[9], float tau, int k, pm_match* out,
                           int32_t* n_admitted);
int pm_bf_knn_guided_hamming_u8(pm_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt, int bytes,
                                const float* kp1_xy, const float* kp2_xy, int kind, const double M[9], float tau, int k,
                                pm_match* out, int32_t* n_admitted);

/* Multi-GPU glue: concatenates `parts` padded blocks of `stride` points (d_counts[p] valid in
 * block p), e.g. the all-gathered per-rank survivors of a query-row-sharded matcher, into one
 * contiguous correspondence array in part order; *d_n_total = sum of counts.  A count below 0 is read as 0 and a
 * count above `stride` as `stride`.  1 <= parts <= 65535 and stride >= 1, else PM_E_INVALID. */
int pm_concat_points_dev(pm_ctx* ctx, const float* d_xy1_parts, const float* d_xy2_parts,
                         const int32_t* d_counts, int parts, int stride, float* d_xy1,
                         float* d_xy2, int32_t* d_n_total);

/* ---- match list + gather (main.cpp:71-79, :89-91) ------------------------------------------
 * pm_match_indices: pointIndexes1/2 of main.cpp:77-78.
 * pm_gather_points: KeyPoint::convert(keyPoint, selPoints, pointIndexes) of main.cpp:90-91;
 *   kp_xy is the keypoints' .pt as interleaved (x,y) floats; out_xy[i] = kp_xy[idx[i]].
 *   Returns PM_E_INVALID if an index is outside [0, n_kp). */
int pm_match_indices(const pm_match* m, int n, int32_t* query_idx, int32_t* train_idx);
int pm_gather_points(const float* kp_xy, int n_kp, const int32_t* idx, int n, float* out_xy);
/* Formats the stdout block of main.cpp:73-76 into buf (NUL-terminated, truncated at cap);
 * returns the number of bytes that the full text needs (like snprintf). */
long pm_format_match_list(const pm_match* m, int n, char* buf, size_t cap);

/* ---- robust fundamental matrix (replaces main.cpp:95-98 cv::findFundamentalMat) ------------ */
enum { PM_ERR_SAMPSON = 0, PM_ERR_SYM_EPIPOLAR = 1 };

typedef struct pm_ransac_params {
    int64_t  hyp_begin;     /* hypothesis ids [hyp_begin, hyp_end) are evaluated; ids < 2^32  */
    int64_t  hyp_end;       /* single GPU: 0 .. iters.  Multi-GPU: this rank's shard.          */
    uint64_t seed;          /* counter-based sampler key (SPEC S6): sample(h) depends only on  */
                            /* (seed, h, n), never on the shard or the device                   */
    float    thresh_px;     /* inlier threshold tau in pixels; test is num^2 <= tau^2 * den     */
    int32_t  error_kind;    /* PM_ERR_SAMPSON | PM_ERR_SYM_EPIPOLAR                             */
} pm_ransac_params;

/* xy1/xy2: n x 2 interleaved float pixel coordinates in match order (selPoints1/2 of
 * main.cpp:89-91).  Every hypothesis h in the range: sample 8 correspondences, Hartley-
 * normalised 8-point solve with rank-2 enforcement (fp64), score ALL n correspondences (fp32),
 * count inliers.  Winner: most inliers, ties -> lowest h.
 *   best_key : (inliers << 32) | (0xFFFFFFFF - h); 0 = no valid model in the range.  This is
 *              the value a multi-GPU caller max-reduces (one 8-byte all-reduce).
 *   F        : 3x3 row-major, x2^T F x1 = 0, unit Frobenius norm, F[8] >= 0 (may be NULL)
 *   mask     : n bytes 0/1 (may be NULL);  n_inliers: may be NULL.
 * n < 8 -> PM_E_TOO_FEW.  All-degenerate range -> PM_E_NO_MODEL with F = 0, mask = 0. */
int pm_ransac_fundamental(pm_ctx* ctx, const float* xy1, const float* xy2, int n,
                          const pm_ransac_params* p, double F[9], uint8_t* mask,
                          int* n_inliers, uint64_t* best_key);
/* Device-resident form used by the bench and the multi-GPU path: scores the shard and leaves
 * the shard's best key in *d_best_key (device uint64).  No model is materialised. */
int pm_ransac_score_dev(pm_ctx* ctx, const float* d_xy1, const float* d_xy2, int n,
                        const pm_ransac_params* p, uint64_t* d_best_key);
/* Same, with the correspondence count read on the device: n = min(*d_n, n_max).  Lets a batch
 * flow matcher -> pm_filter_ratio_gather_dev -> RANSAC without a host round trip.  *d_n < 8
 * leaves *d_best_key = 0. */
int pm_ransac_score_devn(pm_ctx* ctx, const float* d_xy1, const float* d_xy2, int n_max,
                         const int32_t* d_n, const pm_ransac_params* p, uint64_t* d_best_key);
/* Whole single-shard run on the device: solve + score [hyp_begin, hyp_end), pick the winner and
 * publish its key, F (9 doubles), mask (n_max bytes, zero beyond n) and inlier count — the
 * device-resident equivalent of pm_ransac_fundamental.  d_n may be NULL (n = n_max). */
int pm_ransac_run_dev(pm_ctx* ctx, const float* d_xy1, const float* d_xy2, int n_max,
                      const int32_t* d_n, const pm_ransac_params* p, uint64_t* d_best_key,
                      double* d_F, uint8_t* d_mask, int32_t* d_n_inliers);
/* Device-resident finalisation: F (9 doubles), mask (n_max bytes, zero beyond n) and inlier
 * count of the hypothesis encoded in *d_key (e.g. the all-reduced winner).  d_n may be NULL
 * (then n = n_max).  A zero key / n < 8 gives F = 0, mask = 0, count 0. */
int pm_ransac_model_from_key_dev(pm_ctx* ctx, const float* d_xy1, const float* d_xy2, int n_max,
                                 const int32_t* d_n, const pm_ransac_params* p,
                                 const uint64_t* d_key, double* d_F, uint8_t* d_mask,
                                 int32_t* d_n_inliers);
/* Re-derives F + mask of ONE hypothesis id (every rank calls this with the reduced winner:
 * no model broadcast is needed).  hyp is the id, not the key. */
int pm_ransac_model_from_hyp(pm_ctx* ctx, const float* xy1, const float* xy2, int n,
                             const pm_ransac_params* p, int64_t hyp, double F[9],
                             uint8_t* mask, int* n_inliers);
/* ---- one-launch and sharded forms over a correspondence VIEW --------------------------------------
 * A view names the correspondences without copying them: `parts` blocks of up to `cap` points, part p
 * starting at xy1 + p*pitch_xy / xy2 + p*pitch_xy (floats) and holding counts[p*pitch_cnt] points
 * (device-side, clamped to [0, cap]; counts == NULL: every part is full).  Correspondence i of the run is
 * the i-th point in part order.  parts = 1 is a plain array, optionally with a device-side count.  This is
 * how the all-gathered survivor blocks of a query-row-sharded matcher feed RANSAC on every
 * rank without a concatenation pass. */
#define PM_MAX_PARTS 64
typedef struct pm_points_view {
    const float*   xy1;
    const float*   xy2;
    const int32_t* counts;
    int32_t parts;
    int32_t cap;
    int64_t pitch_xy;
    int32_t pitch_cnt;
    int32_t reserved;
} pm_points_view;
/* What a shard contributes to the multi-GPU exchange: its best key and the fp64 model behind it.  The
 * global winner is the record with the largest key — an arg-max all-reduce, carried as one 80-byte
 * all-gather (RCCL has no user-defined reduction); no rank re-solves anything. */
typedef struct pm_ransac_record {
    uint64_t key;       /* pm_ransac_key of the shard's winner, 0 if it has no valid model */
    double   F[9];
} pm_ransac_record;
/* Sharded run, ONE launch: sample + solve + score ids [hyp_begin, hyp_end) over the view, write the
 * shard's record to *d_record (device). */
int pm_ransac_shard_parts_dev(pm_ctx* ctx, const pm_points_view* view, const pm_ransac_params* p,
                              pm_ransac_record* d_record);
/* After the exchange: winner among d_records[0..n_records), its F (9 doubles, may be NULL), inlier mask
 * over the view (d_mask[0..mask_len), zero beyond the correspondence count), inlier count and (optional)
 * the correspondence count itself.  Only thresh_px and error_kind of *p are used. */
int pm_ransac_finish_parts_dev(pm_ctx* ctx, const pm_points_view* view, const pm_ransac_params* p,
                               const pm_ransac_record* d_records, int n_records, uint64_t* d_key, double* d_F,
                               uint8_t* d_mask, int mask_len, int32_t* d_n_inliers, int32_t* d_n_total);
/* key helpers */
static inline uint64_t pm_ransac_key(uint32_t inliers, uint32_t hyp) {
    return ((uint64_t)inliers << 32) | (uint64_t)(0xFFFFFFFFu - hyp);
}
static inline uint32_t pm_ransac_key_hyp(uint64_t key)     { return 0xFFFFFFFFu - (uint32_t)key; }
static inline uint32_t pm_ransac_key_inliers(uint64_t key) { return (uint32_t)(key >> 32); }

/* ---- robust homography (cv::findHomography(pts1, pts2, RANSAC, thr): the planar-scene / pure-rotation sibling
 * of the findFundamentalMat call at main.cpp:95-98) — docs/SPEC.md S19-S22.  pm_ransac_params as above, with
 * error_kind = PM_ERR_REPROJ (the only kind accepted here; anything else -> PM_E_INVALID).  Every hypothesis h in
 * [hyp_begin, hyp_end) (non-empty): sample 4 correspondences (S19, a stream of its own), Hartley-normalised 4-point
 * DLT in fp64 (S20), score ALL n correspondences with the fp32 one-way reprojection test
 * ||x2 - H x1||^2 <= thresh_px^2, division-free (S21), count inliers.  Winner: most inliers, ties -> lowest h (S22).
 * A sample is invalid (key 0) when 3 of its 4 points are collinear in either image or the orientations of its
 * triples disagree between the images (OpenCV's sample check: reflections stay valid).  The H here is the winning
 * 4-point solve; pm_homography_refine* (below) refines it on its inliers, pm_ransac_homography_refined does both.
 *   H        : 3x3 row-major, x2 ~ H x1, unit Frobenius norm, H[8] >= 0 (pm_f_scale_f33 gives OpenCV's H[8] = 1)
 *   best_key : pm_ransac_key(inliers, h) of the winner, 0 = no valid model
 * One launch per call (solve + score + winner + mask).  Graph capture: as the RANSAC-F entry points — no per-call
 * epoch argument (the arrival ticket returns to zero in the launch), so the device form records on a capturing
 * stream once an eager call of at least its shape has been made on the context ("Graph capture of the estimator
 * calls" above: otherwise PM_E_UNSUPPORTED, before any side effect); the host forms synchronise and therefore cannot
 * be captured. */
enum { PM_ERR_REPROJ = 2 };
/* Host in, host out (mirrors pm_ransac_fundamental).  mask (n bytes), n_inliers, best_key may be NULL.
 * Statuses: PM_E_INVALID (null params or points, bad range, error_kind != PM_ERR_REPROJ, null ctx),
 * n < 4 -> PM_E_TOO_FEW, all hypotheses invalid -> PM_E_NO_MODEL with H = 0, mask = 0 (*best_key = 0). */
int pm_ransac_homography(pm_ctx* ctx, const float* xy1, const float* xy2, int n, const pm_ransac_params* p,
                         double H[9], uint8_t* mask, int* n_inliers, uint64_t* best_key);
/* Whole run on the device over a correspondence view (a plain array is parts = 1, optionally with a device-side
 * count): the count is read on the device, so it chains after pm_filter_ratio_gather_dev /
 * pm_bf_knn_l2_*_ratio_dev with no host round trip.  Writes *d_best_key, d_H (9 doubles), d_mask[0..mask_len)
 * (zero beyond n) and *d_n_inliers; n < 4 or no valid model leaves key 0, H = 0, mask = 0, count 0.  All four
 * output pointers are required.  PM_E_INVALID for bad arguments, as above. */
int pm_ransac_homography_run_dev(pm_ctx* ctx, const pm_points_view* view, const pm_ransac_params* p,
                                 uint64_t* d_best_key, double* d_H, uint8_t* d_mask, int mask_len,
                                 int32_t* d_n_inliers);
/* H, mask and inlier count of ONE hypothesis id (0 <= hyp < 2^32; p's hypothesis range is ignored): the same
 * launch over [hyp, hyp + 1).  An invalid sample -> PM_E_NO_MODEL with H = 0, mask = 0. */
int pm_ransac_homography_from_hyp(pm_ctx* ctx, const float* xy1, const float* xy2, int n,
                                  const pm_ransac_params* p, int64_t hyp, double H[9], uint8_t* mask,
                                  int* n_inliers);

/* ---- refinement of the robust homography on its inliers (what cv::findHomography runs after its RANSAC loop) —
 * docs/SPEC.md S23-S25.  Over the correspondences with mask[i] != 0: a Hartley-normalised least-squares DLT refit on
 * all of them (S23, fp64, Jacobi eigen-solve), then Levenberg-Marquardt on the forward transfer error
 * sum ||x2 - H x1||^2 with H[8] = 1 fixed (S24, up to max_iters iterations, one pass over the inliers each).  LM starts
 * from the refit or from H_in, whichever has the lower cost (ties -> the refit), and accepts only cost decreases, so
 * cost_out <= cost_in.  The mask is not recomputed.  Output H: x2 ~ H x1, unit Frobenius norm, H[8] >= 0 (S20).
 * max_iters in [0, 100]; 0 = refit only; 10 is OpenCV's default.  status: 0 = refined, 1 = kept H_in (fewer than 4
 * inliers, or no refit and no LM gain; H_out = H_in bit for bit), 2 = H_in is zero (no model; H_out = 0).
 * One launch of one workgroup.  Graph capture: the launch keeps no per-call state, so the device form is not refused on
 * a capturing stream; the host forms synchronise and therefore cannot be captured. */
typedef struct pm_h_refine_info {
    double  cost_in, cost_out;   /* sum of squared forward transfer errors over the inliers, px^2 */
    int32_t n_used, iters, status, reserved;
} pm_h_refine_info;
/* Host in, host out.  mask: n bytes 0/1 (e.g. from pm_ransac_homography); H_out may alias H_in; info may be NULL.
 * Statuses: PM_E_INVALID (null arrays, max_iters out of range, null ctx), n < 4 -> PM_E_TOO_FEW (H_out = H_in),
 * H_in zero -> PM_E_NO_MODEL (status 2). */
int pm_homography_refine(pm_ctx* ctx, const float* xy1, const float* xy2, int n, const uint8_t* mask,
                         const double H_in[9], int max_iters, double H_out[9], pm_h_refine_info* info);
/* Device form over a view (count read on the device, as pm_ransac_homography_run_dev): chains after it with no host
 * round trip.  d_mask covers the view's correspondences in view order; d_H_out may equal d_H_in; d_info may be NULL.
 * Data outcomes (zero H, fewer than 4 inliers) are reported in *d_info only. */
int pm_homography_refine_dev(pm_ctx* ctx, const pm_points_view* view, const uint8_t* d_mask, const double* d_H_in,
                             int max_iters, double* d_H_out, pm_h_refine_info* d_info);
/* Convenience: pm_ransac_homography + refinement, one synchronisation; mask/n_inliers/best_key as the RANSAC call
 * (the RANSAC mask), H refined, info may be NULL.  Statuses as pm_ransac_homography. */
int pm_ransac_homography_refined(pm_ctx* ctx, const float* xy1, const float* xy2, int n, const pm_ransac_params* p,
                                 int max_iters, double H[9], uint8_t* mask, int* n_inliers, uint64_t* best_key,
                                 pm_h_refine_info* info);

/* ---- refinement of the robust fundamental matrix on its inliers (the refit every SfM front end runs after
 * cv::findFundamentalMat, which returns the minimal-sample model) — docs/SPEC.md S43-S45.  Over the correspondences with
 * mask[i] != 0: a Hartley-normalised least-squares 8-point refit on all of them (S44, fp64, Jacobi eigen-solve, rank 2
 * enforced as S7 does), then Levenberg-Marquardt on the sum of squared Sampson distances (px^2) over 7 parameters that
 * cannot leave rank 2 (S45: F = U diag(1, sigma, 0) V^T in the refit's normalised coordinates, Cayley rotation steps on U
 * and V, a step of sigma; up to max_iters iterations, one pass over the inliers each).  LM starts from the refit or from
 * F_in, whichever has the lower cost (ties -> the refit); its result counts only if its cost in pixels is below the
 * start's, so cost_out <= cost_in.  The refit and LM need at least 8 inliers.  The mask is not recomputed.  Output F:
 * x2^T F x1 = 0, unit Frobenius norm, F[8] >= 0 (S10), rank 2 by construction.  max_iters in [0, 100]; 0 = refit only.
 * Info: pm_h_refine_info, costs in px^2; status 0 = refined, 1 = kept F_in (fewer than 8 inliers, or no refit and no LM
 * gain; F_out = F_in bit for bit), 2 = F_in is zero (no model; F_out = 0).  One launch of one workgroup.  Graph capture:
 * the launch keeps no per-call state, so the device form is not refused on a capturing stream; the host forms synchronise
 * and therefore cannot be captured.
 * Host in, host out.  mask: n bytes 0/1 (e.g. from pm_ransac_fundamental); F_out may alias F_in; info may be NULL.
 * Statuses: PM_E_INVALID (null arrays, max_iters out of range, null ctx), n < 8 -> PM_E_TOO_FEW (F_out = F_in),
 * F_in zero -> PM_E_NO_MODEL (status 2). */
int pm_fundamental_refine(pm_ctx* ctx, const float* xy1, const float* xy2, int n, const uint8_t* mask,
                          const double F_in[9], int max_iters, double F_out[9], pm_h_refine_info* info);
/* Device form over a view (count read on the device): chains after pm_ransac_run_dev / pm_ransac_finish_parts_dev with
 * no host round trip.  d_mask covers the view's correspondences in view order; d_F_out may equal d_F_in; d_info may be
 * NULL.  Data outcomes (zero F, fewer than 8 inliers) are reported in *d_info only. */
int pm_fundamental_refine_dev(pm_ctx* ctx, const pm_points_view* view, const uint8_t* d_mask, const double* d_F_in,
                              int max_iters, double* d_F_out, pm_h_refine_info* d_info);
/* Convenience: pm_ransac_fundamental (over a non-empty hypothesis range, by the one-launch kernel) + refinement, one
 * synchronisation; mask/n_inliers/best_key as the RANSAC call (the RANSAC mask), F refined, info may be NULL.  Statuses
 * as pm_ransac_fundamental, plus an empty range or max_iters outside [0, 100] -> PM_E_INVALID. */
int pm_ransac_fundamental_refined(pm_ctx* ctx, const float* xy1, const float* xy2, int n, const pm_ransac_params* p,
                                  int max_iters, double F[9], uint8_t* mask, int* n_inliers, uint64_t* best_key,
                                  pm_h_refine_info* info);

/* ---- robust 2D affine and similarity (cv::estimateAffine2D / cv::estimateAffinePartial2D with RANSAC: the
 * alignment models of document scans, aerial mosaics and video stabilisation, where the perspective part of an H is
 * noise) — docs/SPEC.md S26-S30.  One family, the model chosen by `model`:
 *   PM_AFFINE_FULL     6 DOF, x2 = A [x1 y1 1]^T with A = [a0 a1 a2; a3 a4 a5], 3-point samples (estimateAffine2D);
 *   PM_AFFINE_PARTIAL  4 DOF, A = [a -b tx; b a ty] (rotation, uniform scale, translation), 2-point samples
 *                      (estimateAffinePartial2D).
 * pm_ransac_params as for the homography: error_kind = PM_ERR_REPROJ only, ids [hyp_begin, hyp_end) non-empty.  Every
 * hypothesis h: sample MIN_PTS = 3 (full) or 2 (partial) correspondences on a stream of the model's own (S26), solve
 * the minimal system in fp64 (S27; a full sample is invalid when its 3 points are collinear in either image, a partial
 * one when its 2 points coincide in either image), score ALL n correspondences with ||x2 - A x1||^2 <= thresh_px^2 in
 * fp32 (S28), count inliers.  Winner: most inliers, ties -> lowest h (S29).  A: 6 doubles, 2 x 3 row-major (OpenCV's
 * layout).  pm_affine_refine* then refit A on the inliers by closed-form least squares (S30), pm_estimate_affine does
 * both.  Graph capture: as the homography calls (no per-call state; the host forms synchronise). */
enum { PM_AFFINE_FULL = 0, PM_AFFINE_PARTIAL = 1 };
/* Host in, host out (mirrors pm_ransac_homography).  mask (n bytes), n_inliers, best_key may be NULL.
 * Statuses: PM_E_INVALID (model not PM_AFFINE_*, null params or points, bad range, error_kind != PM_ERR_REPROJ, null
 * ctx), n < MIN_PTS -> PM_E_TOO_FEW, all hypotheses invalid -> PM_E_NO_MODEL with A = 0, mask = 0 (*best_key = 0). */
int pm_ransac_affine(pm_ctx* ctx, int model, const float* xy1, const float* xy2, int n, const pm_ransac_params* p,
                     double A[6], uint8_t* mask, int* n_inliers, uint64_t* best_key);
/* A, mask and inlier count of ONE hypothesis id (0 <= hyp < 2^32; p's hypothesis range is ignored): the same launch
 * over [hyp, hyp + 1).  An invalid sample -> PM_E_NO_MODEL with A = 0, mask = 0. */
int pm_ransac_affine_from_hyp(pm_ctx* ctx, int model, const float* xy1, const float* xy2, int n,
                              const pm_ransac_params* p, int64_t hyp, double A[6], uint8_t* mask, int* n_inliers);
/* Whole run on the device over a correspondence view, as pm_ransac_homography_run_dev: chains after
 * pm_filter_ratio_gather_dev / pm_bf_knn_l2_*_ratio_dev with no host round trip.  Writes *d_best_key, d_A (6
 * doubles), d_mask[0..mask_len) (zero beyond n) and *d_n_inliers; n < MIN_PTS or no valid model leaves key 0, A = 0,
 * mask = 0, count 0.  All four output pointers are required. */
int pm_ransac_affine_run_dev(pm_ctx* ctx, int model, const pm_points_view* view, const pm_ransac_params* p,
                             uint64_t* d_best_key, double* d_A, uint8_t* d_mask, int mask_len, int32_t* d_n_inliers);
/* Least-squares refit of A on the correspondences with mask[i] != 0 (what estimateAffine2D's Levenberg-Marquardt
 * refinement converges to [recalled]: the costs are quadratic, so the minimiser of sum ||x2 - A x1||^2 is closed-form;
 * S30).  Sums in S23's fixed order; the refit is kept only if its cost is not higher than A_in's, so
 * cost_out <= cost_in.  The mask is not recomputed.  Info: pm_h_refine_info with iters = 0; status 0 = refitted,
 * 1 = kept A_in (fewer than MIN_PTS inliers, degenerate normal system or no gain; A_out = A_in bit for bit), 2 = A_in
 * is zero (no model).  Host in, host out; A_out may alias A_in; info may be NULL.
 * Statuses: PM_E_INVALID (bad model, null arrays, null ctx), n < MIN_PTS -> PM_E_TOO_FEW (A_out = A_in),
 * A_in zero -> PM_E_NO_MODEL (status 2).  One launch of one workgroup. */
int pm_affine_refine(pm_ctx* ctx, int model, const float* xy1, const float* xy2, int n, const uint8_t* mask,
                     const double A_in[6], double A_out[6], pm_h_refine_info* info);
/* Device form over a view (count read on the device): chains after pm_ransac_affine_run_dev with no host round trip.
 * d_A_out may equal d_A_in; d_info may be NULL; data outcomes are reported in *d_info only. */
int pm_affine_refine_dev(pm_ctx* ctx, int model, const pm_points_view* view, const uint8_t* d_mask, const double* d_A_in,
                         double* d_A_out, pm_h_refine_info* d_info);
/* Convenience: cv::estimateAffine2D / estimateAffinePartial2D in one call — pm_ransac_affine, then (refine != 0) the
 * refit, one synchronisation.  mask/n_inliers/best_key as the RANSAC call (the RANSAC mask).  info (may be NULL): the
 * refit's; with refine == 0 it is zero but for status (1, or 2 without a model).  Statuses as pm_ransac_affine. */
int pm_estimate_affine(pm_ctx* ctx, int model, const float* xy1, const float* xy2, int n, const pm_ransac_params* p,
                       int refine, double A[6], uint8_t* mask, int* n_inliers, uint64_t* best_key,
                       pm_h_refine_info* info);

/* ---- calibrated relative pose (cv::findEssentialMat with RANSAC + cv::recoverPose: visual odometry, SfM front ends,
 * stereo rigs) — docs/SPEC.md S31-S35.  One pinhole camera shared by both views; no distortion
 * (pixels of a real lens go through pm_undistort_points* first, S81).  K is invalid unless
 * fx, fy > 0, all four values are finite and the normalised threshold thresh_px / ((fx + fy) / 2) is finite and > 0 in
 * fp32.  Correspondences are normalised as xn = (x - cx) / fx, yn = (y - cy) / fy (fp64, rounded to fp32).
 * RANSAC-E: pm_ransac_params with error_kind = PM_ERR_SAMPSON; sample h in [hyp_begin, hyp_end) draws 5
 * correspondences (S32) and the 5-point solve (S33) gives up to 10 candidates, model ids 10h + j; every candidate is
 * scored with the Sampson test on the normalised points (S34).  Winner: most inliers, ties -> lowest id; the key is
 * (inliers << 32) | (0xFFFFFFFF - id), so 10 * hyp_end <= 2^32 (and 10 * (hyp_end - hyp_begin) <= 2^31 - 1).
 * E: 9 doubles row-major, x2n^T E x1n = 0 on normalised coordinates, unit Frobenius norm, its first entry of largest
 * magnitude positive.  Pose (S35): R (9 doubles, row-major) and t (3 doubles, unit norm) with x2 ~ R x1 + t; the pose
 * mask is the input mask AND the cheirality of the chosen candidate (depths in (0, dist) in both cameras; OpenCV's
 * default dist is 50).  Statuses: PM_E_INVALID (bad K, null params / points / outputs, bad range, error_kind,
 * dist not > 0), n < 5 -> PM_E_TOO_FEW, no valid candidate -> PM_E_NO_MODEL with E = 0, mask = 0.  Graph capture: as
 * the homography calls (no per-call state; the host forms synchronise). */
typedef struct pm_camera { double fx, fy, cx, cy; } pm_camera;
/* Host in, host out.  mask (n bytes), n_inliers, best_key may be NULL. */
int pm_ransac_essential(pm_ctx* ctx, const float* xy1, const float* xy2, int n, const pm_camera* K,
                        const pm_ransac_params* p, double E[9], uint8_t* mask, int* n_inliers, uint64_t* best_key);
/* All candidates of ONE sample id (0 <= hyp, 10 * hyp + 10 <= 2^32; p's range is ignored): E[10 * 9] (slot j = the
 * j-th real root of S33, zero when unused), counts[j] = its inlier count (-1: unused slot), *n_models = valid slots.
 * No valid candidate -> PM_E_NO_MODEL. */
int pm_ransac_essential_from_hyp(pm_ctx* ctx, const float* xy1, const float* xy2, int n, const pm_camera* K,
                                 const pm_ransac_params* p, int64_t hyp, double E[90], int32_t counts[10], int* n_models);
/* Whole run on the device over a correspondence view (counts read on the device): chains after
 * pm_filter_ratio_gather_dev / pm_bf_knn_l2_*_ratio_dev with no host round trip.  Writes *d_best_key, d_E (9 doubles),
 * d_mask[0..mask_len) (zero beyond n) and *d_n_inliers; n < 5 or no valid model leaves key 0, E = 0, mask = 0. */
int pm_ransac_essential_run_dev(pm_ctx* ctx, const pm_points_view* view, const pm_camera* K, const pm_ransac_params* p,
                                uint64_t* d_best_key, double* d_E, uint8_t* d_mask, int mask_len, int32_t* d_n_inliers);
/* cv::recoverPose: decompose E, triangulate the correspondences with mask_in[i] != 0 (mask_in NULL: all) against the
 * four candidates, keep the one most points pass.  mask_out (n bytes, may alias mask_in), n_good may be NULL; points4
 * (may be NULL): 4 floats per correspondence, the chosen candidate's homogeneous point (cv::triangulatePoints, n x 4).
 * E that does not decompose (rank < 2, not finite) -> PM_E_NO_MODEL with R = 0, t = 0, mask 0. */
int pm_recover_pose(pm_ctx* ctx, const float* xy1, const float* xy2, int n, const pm_camera* K, const double E[9],
                    const uint8_t* mask_in, double dist, double R[9], double t[3], uint8_t* mask_out, int* n_good,
                    float* points4);
/* Device form over a view: d_mask_in may be NULL, d_points4 may be NULL; d_mask_out holds parts * cap bytes (zero beyond
 * n), d_points4 4 * parts * cap floats (written below n).  One launch of one workgroup; a bad E gives R = 0, t = 0. */
int pm_recover_pose_dev(pm_ctx* ctx, const pm_points_view* view, const pm_camera* K, const double* d_E,
                        const uint8_t* d_mask_in, double dist, double* d_R, double* d_t, uint8_t* d_mask_out,
                        int32_t* d_n_good, float* d_points4);
/* Both in one call, one synchronisation: RANSAC-E, then pose recovery on its inliers.  mask: the pose mask (n bytes,
 * may be NULL); n_inliers: RANSAC's count; n_good: the pose's.  Statuses as pm_ransac_essential. */
int pm_estimate_pose(pm_ctx* ctx, const float* xy1, const float* xy2, int n, const pm_camera* K,
                     const pm_ransac_params* p, double dist, double E[9], double R[9], double t[3], uint8_t* mask,
                     int* n_inliers, int* n_good, uint64_t* best_key);

/* ---- refinement of the relative pose on its inliers — docs/SPEC.md S46-S47.  Over the correspondences with
 * mask[i] != 0 (typically the pose mask of pm_recover_pose*): Levenberg-Marquardt on the sum of squared Sampson distances
 * of E = [t]x R on the S31-normalised points, reported in px^2 by the factor ((fx + fy) / 2)^2, over 5 parameters: a
 * Cayley rotation step on R (no transcendental function) and a step of t in the tangent plane of the unit sphere,
 * renormalised.  Sums in S23's fixed order, S24's Cholesky and damping; it runs only with at least 5 inliers, max_iters > 0
 * and a t_in of finite non-zero length, and accepts only cost decreases, so cost_out <= cost_in.  The mask is not
 * recomputed.  max_iters in [0, 100]; 0 returns the input.  Outputs: R_out, t_out (unit norm when refined) and E_out =
 * [t_out]x R_out in S33's convention (unit Frobenius norm, sign of the largest entry; zero if that E has no finite
 * non-zero norm), so pm_recover_pose* can re-triangulate against the refined pose.  Info: pm_h_refine_info; status 0 =
 * refined, 1 = kept the input (R_out, t_out = R_in, t_in bit for bit), 2 = the input pose is zero (no model, E_out = 0).
 * One launch of one workgroup; the device form keeps no per-call state.  Host in, host out: outputs may alias the inputs;
 * E_out and info may be NULL.  Statuses: PM_E_INVALID (bad K or max_iters, null arrays, null ctx), n < 5 -> PM_E_TOO_FEW
 * (outputs = inputs), zero input pose -> PM_E_NO_MODEL. */
int pm_pose_refine(pm_ctx* ctx, const float* xy1, const float* xy2, int n, const pm_camera* K, const uint8_t* mask,
                   const double R_in[9], const double t_in[3], int max_iters, double R_out[9], double t_out[3],
                   double E_out[9], pm_h_refine_info* info);
/* Device form over a view (count read on the device): chains after pm_recover_pose_dev with no host round trip, when
 * that call's d_R and d_t are the two ends of one array of 12 doubles.  d_Rt_in / d_Rt_out: 12 doubles (R, then t),
 * d_Rt_out may equal d_Rt_in; d_mask covers the view's correspondences in view order; d_E_out (9 doubles) and d_info may
 * be NULL; data outcomes are reported in *d_info only. */
int pm_pose_refine_dev(pm_ctx* ctx, const pm_points_view* view, const pm_camera* K, const uint8_t* d_mask,
                       const double* d_Rt_in, int max_iters, double* d_Rt_out, double* d_E_out, pm_h_refine_info* d_info);
/* pm_estimate_pose, then the refinement of its pose on its pose mask, one synchronisation.  mask / n_inliers / n_good /
 * best_key as pm_estimate_pose; R, t refined; E: the E of the refined pose (E_out above); info (may be NULL) the
 * refinement's.  Statuses as pm_estimate_pose, plus max_iters outside [0, 100] -> PM_E_INVALID. */
int pm_estimate_pose_refined(pm_ctx* ctx, const float* xy1, const float* xy2, int n, const pm_camera* K,
                             const pm_ransac_params* p, double dist, int max_iters, double E[9], double R[9], double t[3],
                             uint8_t* mask, int* n_inliers, int* n_good, uint64_t* best_key, pm_h_refine_info* info);

/* ---- absolute camera pose (cv::solvePnPRansac with SOLVEPNP_P3P: locating a new frame against 3-D points that are
 * already known: the map pm_triangulate* builds from posed views, below) — docs/SPEC.md S36-S39.  Correspondence i is a world point
 * xyz[3i .. 3i+2] and its pixel uv[2i .. 2i+1] (f32).  One pinhole pm_camera K, no distortion (pixels of a real lens
 * go through pm_undistort_points* first, S81); K is invalid unless fx, fy > 0
 * and all four values are finite.  Pose: x_cam = R X + t, pixel ~ K x_cam; R 9 doubles row-major, t 3 doubles.
 * pm_ransac_params with error_kind = PM_ERR_REPROJ and thresh_px finite and > 0 (OpenCV's default reprojectionError is
 * 8); sample h in [hyp_begin, hyp_end) draws 3 correspondences (S37) and the P3P solve (Grunert's quartic, S38) gives up
 * to 4 candidates, model ids 4h + j; every candidate is scored with the squared pixel reprojection error
 * ||uv - proj(R X + t)||^2 <= thresh_px^2, points behind the camera rejected (S39).  OpenCV picks one P3P candidate with a
 * fourth point instead [recalled]; here all are scored.  Winner: most inliers, ties -> lowest id; the key is
 * (inliers << 32) | (0xFFFFFFFF - id), so 4 * hyp_end <= 2^32 (and 4 * (hyp_end - hyp_begin) <= 2^31 - 1).  Statuses:
 * PM_E_INVALID (bad K, threshold, range or error_kind, null params / points / outputs, null ctx), n < 4 -> PM_E_TOO_FEW,
 * no valid candidate -> PM_E_NO_MODEL with R = 0, t = 0, mask = 0.  Graph capture: as the homography calls (no per-call
 * state; the host forms synchronise).  pm_pnp_refine* (below) refines the pose on its inliers, pm_solve_pnp_ransac does
 * both. */
/* Plain arrays of correspondences on the device with an optional device-side count (clamped to [0, cap]; NULL: cap). */
typedef struct pm_pnp_view {
    const float*   xyz;     /* cap x 3 world points */
    const float*   uv;      /* cap x 2 pixels */
    const int32_t* count;
    int32_t cap;
    int32_t reserved;
} pm_pnp_view;
/* Host in, host out (cv::solvePnPRansac without its refinement).  mask (n bytes), n_inliers, best_key may be NULL. */
int pm_ransac_pnp(pm_ctx* ctx, const float* xyz, const float* uv, int n, const pm_camera* K, const pm_ransac_params* p,
                  double R[9], double t[3], uint8_t* mask, int* n_inliers, uint64_t* best_key);
/* All candidates of ONE sample id (0 <= hyp, 4 * hyp + 4 <= 2^32; p's range is ignored): Rt[4 * 12] (slot j = the j-th
 * real root of S38: R then t, zero when unused), counts[j] = its inlier count (-1: unused slot), *n_models = valid slots.
 * No valid candidate -> PM_E_NO_MODEL. */
int pm_ransac_pnp_from_hyp(pm_ctx* ctx, const float* xyz, const float* uv, int n, const pm_camera* K,
                           const pm_ransac_params* p, int64_t hyp, double Rt[48], int32_t counts[4], int* n_models);
/* Whole run on the device over a pm_pnp_view (count read on the device): writes *d_best_key, d_Rt (12 doubles: R, then
 * t), d_mask[0..mask_len) (zero beyond n) and *d_n_inliers; n < 4 or no valid model leaves key 0, Rt = 0, mask = 0.
 * All four output pointers are required. */
int pm_ransac_pnp_run_dev(pm_ctx* ctx, const pm_pnp_view* view, const pm_camera* K, const pm_ransac_params* p,
                          uint64_t* d_best_key, double* d_Rt, uint8_t* d_mask, int mask_len, int32_t* d_n_inliers);
/* ---- refinement of the absolute pose on its inliers (the final solvePnP(..., SOLVEPNP_ITERATIVE) that cv::solvePnPRansac
 * runs on its inliers from the RANSAC pose [recalled]) — docs/SPEC.md S40.  Levenberg-Marquardt on the sum of squared
 * pixel reprojection errors over mask[i] != 0 with 6 parameters (a Cayley rotation step, no transcendental function),
 * sums in S23's fixed order, S24's Cholesky and damping; it runs only with at least 4 inliers and max_iters > 0 and
 * accepts only cost decreases, so cost_out <= cost_in.  The mask is not recomputed.  max_iters in [0, 100] (OpenCV's
 * ITERATIVE solver stops at 20 [recalled]).  Info: pm_h_refine_info, costs in px^2; status 0 = refined, 1 = kept the
 * input (R_out, t_out = R_in, t_in bit for bit), 2 = the input pose is zero (no model).  One launch of one workgroup; the
 * device forms keep no per-call state.  Host in, host out: outputs may alias the inputs; info may be NULL.  Statuses:
 * PM_E_INVALID (bad K or max_iters, null arrays, null ctx), n < 4 -> PM_E_TOO_FEW (outputs = inputs), zero input pose ->
 * PM_E_NO_MODEL. */
int pm_pnp_refine(pm_ctx* ctx, const float* xyz, const float* uv, int n, const pm_camera* K, const uint8_t* mask,
                  const double R_in[9], const double t_in[3], int max_iters, double R_out[9], double t_out[3],
                  pm_h_refine_info* info);
/* Device form over a pm_pnp_view (count read on the device): chains after pm_ransac_pnp_run_dev with no host round trip.
 * d_Rt_in / d_Rt_out: 12 doubles (R, then t), d_Rt_out may equal d_Rt_in; d_info may be NULL; data outcomes are reported
 * in *d_info only. */
int pm_pnp_refine_dev(pm_ctx* ctx, const pm_pnp_view* view, const pm_camera* K, const uint8_t* d_mask, const double* d_Rt_in,
                      int max_iters, double* d_Rt_out, pm_h_refine_info* d_info);
/* cv::solvePnPRansac in one call: pm_ransac_pnp, then the refinement of its winner on its mask, one synchronisation.
 * mask / n_inliers / best_key as the RANSAC call (the RANSAC mask); R, t refined; info (may be NULL) the refinement's.
 * Statuses as pm_ransac_pnp, plus max_iters outside [0, 100] -> PM_E_INVALID. */
int pm_solve_pnp_ransac(pm_ctx* ctx, const float* xyz, const float* uv, int n, const pm_camera* K, const pm_ransac_params* p,
                        int max_iters, double R[9], double t[3], uint8_t* mask, int* n_inliers, uint64_t* best_key,
                        pm_h_refine_info* info);
/* The device chain's gather: the compacted match list of pm_bf_knn_l2_*_ratio_dev / pm_filter_ratio_gather_dev (records
 * d_matches[0 .. n), n = *d_count clamped to [0, cap], d_count NULL: cap) into PnP rows: d_uv[i] = d_kp_xy[queryIdx] (the
 * frame's keypoints), d_xyz[i] = d_obj_xyz[trainIdx] (the map's points).  The count passes through unchanged: the view
 * {d_xyz, d_uv, d_count, cap} feeds pm_ransac_pnp_run_dev.  An index out of range gives a NaN row (never an inlier). */
int pm_gather_pnp_dev(pm_ctx* ctx, const pm_match* d_matches, const int32_t* d_count, int cap, const float* d_kp_xy, int n_kp,
                      const float* d_obj_xyz, int n_obj, float* d_uv, float* d_xyz);

/* ---- 3-D to 3-D alignment (cv::estimateAffine3D's slot for a rigid or similarity model, PCL's
 * SampleConsensusModelRegistration, the Sim(3) step of a loop closer: the transform between two sets of corresponding 3-D
 * rows, such as two outputs of pm_stereo_points_dev or pm_triangulate_dev for the same tracks) — docs/SPEC.md S97-S101.
 * Correspondence i is xyz1[3i .. 3i+2] and xyz2[3i .. 3i+2] (f32); a row with a non-finite value in either array is never
 * an inlier and never used by the refit.  Transform: x2 = s R x1 + t.  A model T is 13 doubles: R (9, row-major, det +1),
 * t (3), s (1, > 0); PM_ALIGN3D_RIGID fixes s = 1 exactly.  pm_ransac_params with error_kind = PM_ERR_REPROJ and thresh_px
 * the distance threshold in the points' own unit, finite and > 0; sample h in [hyp_begin, hyp_end) draws 3
 * correspondences (S97) and the triad solve (S98) gives one model, invalid when two sampled points coincide, the three are
 * collinear or a value is not finite in either frame; every model is scored with |s R x1 + t - x2|^2 <= thresh_px^2 in fp32
 * (S99).  Winner: most inliers, ties -> lowest h; the key is (inliers << 32) | (0xFFFFFFFF - h), so hyp_end <= 2^32 (and
 * hyp_end - hyp_begin <= 2^31 - 1).  Statuses: PM_E_INVALID (model not PM_ALIGN3D_*, bad threshold, range or error_kind,
 * null params / points / outputs, null ctx), n < 3 -> PM_E_TOO_FEW, no valid sample -> PM_E_NO_MODEL with T = 0, mask = 0
 * (*best_key = 0).  Graph capture: as the homography calls (no per-call state; the host forms synchronise). */
enum { PM_ALIGN3D_RIGID = 0, PM_ALIGN3D_SIMILARITY = 1 };
/* Plain arrays of correspondences on the device with an optional device-side count (clamped to [0, cap]; NULL: cap). */
typedef struct pm_xyz_view {
    const float*   xyz1;    /* cap x 3 rows of the first frame */
    const float*   xyz2;    /* cap x 3 rows of the second frame */
    const int32_t* count;
    int32_t cap;
    int32_t reserved;
} pm_xyz_view;
/* Host in, host out.  T is required; mask (n bytes), n_inliers, best_key may be NULL. */
int pm_ransac_align3d(pm_ctx* ctx, int model, const float* xyz1, const float* xyz2, int n, const pm_ransac_params* p,
                      double T[13], uint8_t* mask, int* n_inliers, uint64_t* best_key);
/* T, mask and inlier count of ONE sample id (0 <= hyp < 2^32; p's range is ignored): the same launches over
 * [hyp, hyp + 1).  An invalid sample -> PM_E_NO_MODEL with T = 0, mask = 0. */
int pm_ransac_align3d_from_hyp(pm_ctx* ctx, int model, const float* xyz1, const float* xyz2, int n,
                               const pm_ransac_params* p, int64_t hyp, double T[13], uint8_t* mask, int* n_inliers);
/* Whole run on the device over a pm_xyz_view (count read on the device): writes *d_best_key, d_T (13 doubles),
 * d_mask[0..mask_len) (zero beyond n) and *d_n_inliers; n < 3 or no valid model leaves key 0, T = 0, mask = 0, count 0.
 * All four output pointers are required. */
int pm_ransac_align3d_run_dev(pm_ctx* ctx, int model, const pm_xyz_view* view, const pm_ransac_params* p,
                              uint64_t* d_best_key, double* d_T, uint8_t* d_mask, int mask_len, int32_t* d_n_inliers);
/* Least-squares refit of T on the correspondences with mask[i] != 0 and six finite values (S101): Horn's closed-form
 * absolute orientation, the unit quaternion of the largest eigenvalue of a symmetric 4 x 4 matrix found by cyclic Jacobi
 * with a fixed sweep count; the similarity takes Umeyama's least-squares scale.  Sums in S23's fixed order; the refit is
 * kept only if its cost (the sum of squared distances) is not higher than T_in's, so cost_out <= cost_in.  The mask is not
 * recomputed.  Info: pm_h_refine_info with iters = 0; status 0 = refitted, 1 = kept T_in (fewer than 3 usable inliers, a
 * rotation that is not determined: collinear or coincident inliers, no finite positive scale, or no gain; T_out = T_in
 * bit for bit), 2 = T_in is zero (no model).  Host in, host out; T_out may alias T_in; info may be NULL.
 * Statuses: PM_E_INVALID (bad model, null arrays, null ctx), n < 3 -> PM_E_TOO_FEW (T_out = T_in), T_in zero ->
 * PM_E_NO_MODEL (status 2).  One launch of one workgroup. */
int pm_align3d_refine(pm_ctx* ctx, int model, const float* xyz1, const float* xyz2, int n, const uint8_t* mask,
                      const double T_in[13], double T_out[13], pm_h_refine_info* info);
/* Device form over a pm_xyz_view (count read on the device): chains after pm_ransac_align3d_run_dev with no host round
 * trip.  d_T_out may equal d_T_in; d_info may be NULL; data outcomes are reported in *d_info only. */
int pm_align3d_refine_dev(pm_ctx* ctx, int model, const pm_xyz_view* view, const uint8_t* d_mask, const double* d_T_in,
                          double* d_T_out, pm_h_refine_info* d_info);
/* Both in one call — pm_ransac_align3d, then (refine != 0) the refit, one synchronisation.  mask / n_inliers / best_key as
 * the RANSAC call (the RANSAC mask).  info (may be NULL): the refit's; with refine == 0 it is zero but for status (1, or 2
 * without a model).  Statuses as pm_ransac_align3d. */
int pm_estimate_align3d(pm_ctx* ctx, int model, const float* xyz1, const float* xyz2, int n, const pm_ransac_params* p,
                        int refine, double T[13], uint8_t* mask, int* n_inliers, uint64_t* best_key,
                        pm_h_refine_info* info);
/* Apply a 13-double model to rows: out = (float)(s R x + t), fp64 with one rounding to fp32 (S101); a row with a
 * non-finite input or result is three quiet NaNs, so the NaN rows of pm_stereo_points_dev / pm_triangulate_dev stay NaN.
 * Device form: rows [0, n), n = *d_n clamped to [0, cap] (d_n NULL: cap), rows beyond are not written; d_out may be d_xyz;
 * one launch, no per-call state.  Statuses: PM_E_INVALID (null pointer, null ctx, negative size), size 0 ->
 * PM_E_UNSUPPORTED.  pm_transform_points3: the blocking host form. */
int pm_transform_points3_dev(pm_ctx* ctx, const double* d_T, const float* d_xyz, const int32_t* d_n, int cap, float* d_out);
int pm_transform_points3(pm_ctx* ctx, const double* T, const float* xyz, int n, float* out);
/* The device chain's gather, the twin of pm_gather_pnp_dev: the compacted match list (records d_matches[0 .. n), n =
 * *d_count clamped to [0, cap], d_count NULL: cap) between two maps into rows: d_xyz1[i] = d_tab1[queryIdx], d_xyz2[i] =
 * d_tab2[trainIdx] (tables of n1 and n2 rows of 3 floats).  The count passes through unchanged: the view {d_xyz1, d_xyz2,
 * d_count, cap} feeds pm_ransac_align3d_run_dev.  An index out of range gives a NaN row (never an inlier). */
int pm_gather_align3d_dev(pm_ctx* ctx, const pm_match* d_matches, const int32_t* d_count, int cap, const float* d_tab1, int n1,
                          const float* d_tab2, int n2, float* d_xyz1, float* d_xyz2);

/* ---- triangulation: map points from 2 .. 8 posed views (cv::triangulatePoints, then the step a map builder runs behind
 * it: refine the point on its reprojection error and keep it only if it lies in front of every camera, has enough
 * parallax and reprojects well) — docs/SPEC.md S93-S96.  The structure-only half of bundle adjustment; pm_pnp_refine* is
 * the motion-only half, and a caller can alternate them on one stream (pm_bundle_adjust* below moves both at once).  Point i is seen at pixel uv[v][2i .. 2i+1] (f32)
 * of view v, whose pose is x_cam = R X + t as for PnP; one pinhole pm_camera K for every view, no distortion (pixels of a
 * real lens go through pm_undistort_points* first).  Per point, all fp64: the linear solution of the 2V x 4 DLT system
 * (S35's, generalised; a view that does not observe the point contributes zero rows), Levenberg-Marquardt over (X, Y, Z)
 * on the summed squared pixel error with S24's damping (only cost decreases are accepted, so the refined cost is never
 * above the linear one and an unrefined point is returned bit for bit), then three gates at the final point, the first
 * failure being the status: depth in (0, max_depth) in every observing view, the smallest cosine between the rays of two
 * observing views < max_cos_parallax, every observing view's pixel error <= max_reproj_px.  One launch, one lane per
 * point; the pointer arrays live in the struct because observations and poses lie wherever earlier calls left them (the
 * xy1 / xy2 of a pm_points_view, the output of pm_track_lk_gather_dev, the d_Rt of pm_pnp_refine_dev or
 * pm_pose_refine_dev).  A NULL pose is [I|0] exactly: the first camera of pm_recover_pose_dev. */
#define PM_TRI_MAX_VIEWS 8
#define PM_TRI_USE_INITIAL 1   /* skip the linear stage: start from the rows already in d_xyz (re-refine a map) */

typedef struct pm_tri_views {
    const float*   uv[PM_TRI_MAX_VIEWS];  /* view v: cap x 2 pixels (f32), row i = point i; a row S31 turns into NaN
                                             (NaN, inf, |value| > 2^20) means "not seen in this view" */
    const double*  Rt[PM_TRI_MAX_VIEWS];  /* view v: 12 doubles (R row-major, then t), x_cam = R X + t as S36;
                                             NULL = [I|0] exactly */
    const int32_t* count;                 /* device-side point count, clamped to [0, cap]; NULL: cap */
    int32_t n_views, cap;
} pm_tri_views;

typedef struct pm_tri_params {
    double  max_reproj_px;     /* finite, > 0: largest pixel error allowed in any observing view */
    double  max_cos_parallax;  /* in (-1, 1]: the widest-angle pair of rays must have cos < this; 1 switches the test off */
    double  max_depth;         /* > 0, may be +inf: depth in every observing view must lie in (0, max_depth) */
    int32_t max_iters;         /* [0, 100]; 0 = linear solution only */
    int32_t flags;
} pm_tri_params;

enum { PM_TRI_OK = 0, PM_TRI_FEW_VIEWS = 1, PM_TRI_DEGENERATE = 2, PM_TRI_DEPTH = 3, PM_TRI_PARALLAX = 4, PM_TRI_REPROJ = 5 };

/* Device form.  Outputs, row i for point i, rows at or beyond the count not written: d_xyz cap x 3 f32 world points, NaN
 * unless the status is PM_TRI_OK (pm_gather_pnp_dev and the PnP scorer treat a NaN row as "never an inlier"; nothing is
 * compacted, so a caller's track table, descriptors and map rows keep one index); d_status cap bytes (PM_TRI_*: fewer
 * than two observing views, a point at infinity or a non-finite start, then the gates); d_points4 (may be NULL) the
 * linear stage's homogeneous Q as 4 floats per point, the layout and meaning of cv::triangulatePoints and of
 * pm_recover_pose's points4 — written whatever the status, not written under PM_TRI_USE_INITIAL; d_err2 (may be NULL) the
 * largest squared pixel error over the observing views at the final point, NaN unless PM_TRI_OK; *d_n_good (may be NULL)
 * the number of PM_TRI_OK rows.  Under PM_TRI_USE_INITIAL the start is the f32 row already in d_xyz.  Data outcomes are
 * reported per point only.  PM_E_INVALID: a null context, struct, K, params, d_xyz, d_status or uv[v] of a view below
 * n_views, n_views outside [2, 8], cap < 0, a bad K (S31's rule), a parameter outside the ranges above, an unknown flag.
 * No per-call state: the call may be captured. */
int pm_triangulate_dev(pm_ctx* ctx, const pm_tri_views* views, const pm_camera* K, const pm_tri_params* p,
                       float* d_xyz, uint8_t* d_status, float* d_points4, float* d_err2, int32_t* d_n_good);
/* Host in, host out: uv and Rt are arrays of n_views host pointers (Rt[v] may be NULL), n points; one staged block, one
 * synchronisation.  Under PM_TRI_USE_INITIAL xyz is read as well as written. */
int pm_triangulate(pm_ctx* ctx, const float* const* uv, const double* const* Rt, int n_views, int n, const pm_camera* K,
                   const pm_tri_params* p, float* xyz, uint8_t* status, float* points4, float* err2, int* n_good);

/* ---- local bundle adjustment: free poses and points of 2 .. 8 views refined together (the step a map builder runs after
 * it inserts a keyframe) — docs/SPEC.md S113-S117.  pm_triangulate* moves the points alone and pm_pnp_refine* one pose
 * alone; this call moves both at once: Levenberg-Marquardt on the summed squared pixel error over the used observations,
 * solved through the Schur complement on the 6 F parameters of the F free poses (S40's rotation step on the left and its
 * Cayley update, S95's point Jacobian, S24's damped Cholesky and acceptance rule, S23's summation order).  The views are
 * the pm_tri_views a caller built for pm_triangulate_dev, passed on unchanged: row i of uv[v] is point i, a row S31 turns
 * into NaN means "not seen", Rt[v] == NULL is [I|0] exactly, the device-side count is clamped to [0, cap]; one pinhole K
 * for every view.  fixed_mask holds poses: with one held pose the scale is free and only the damping holds it, with two it
 * is fixed.  The used set is decided once, at the start, so the cost function never changes and the accepted cost only
 * falls: observation (i, v) is used iff row i of d_xyz is finite, the pixel is seen, the depth at the start is in (0, inf)
 * and, with gate_px > 0, the squared pixel error at the start is <= gate_px^2; a point is used iff it has at least two used
 * observations, and its observations count only then.  Points live in fp64 in the workspace for the whole run and are
 * rounded to f32 once at the end, and only when a step was accepted: cost_out is the cost of the fp64 state, and a second
 * call starts from the rounded rows, whose cost_in is therefore not this call's cost_out.  One launch of one workgroup: a
 * latency design for a local window, not for a whole map. */
#define PM_BA_MAX_POINTS 65536

typedef struct pm_ba_params {
    double   gate_px;     /* 0: use every observation; finite > 0: drop observations whose pixel error at the START exceeds it */
    int32_t  max_iters;   /* [0, 100]; 0 = evaluate only (cost_in, the used set), nothing moves */
    uint32_t fixed_mask;  /* bit v set: pose v is held.  At least one view held, at least one free. */
    int32_t  flags, reserved;   /* 0 */
} pm_ba_params;

typedef struct pm_ba_info {
    double  cost_in, cost_out;            /* sum of squared pixel errors over the used observations, fp64 state */
    int32_t n_points, n_obs, iters, accepted, status, reserved;
} pm_ba_info;

/* Bytes of device workspace pm_bundle_adjust_dev needs for these views and this cap: pure host arithmetic (no context, no
 * device), a multiple of 16, never decreasing in either argument; 0 for n_views outside [2, 8] or cap outside
 * [0, PM_BA_MAX_POINTS]. */
size_t pm_bundle_adjust_workspace(int n_views, int cap);
/* Device form.  d_Rt_out: n_views x 12 doubles — a held pose bit for bit (a NULL pose as the exact identity), a free pose
 * refined; d_Rt_out + 12 v may be the very pointer views->Rt[v] (every pose is read before any is written).  d_xyz: cap x 3
 * f32, read and written: the map rows of pm_triangulate_dev, NaN rows included; used points are rewritten, every other row
 * keeps its bytes, rows at or beyond the count are not touched.  d_used (may be NULL): cap bytes, bit v of byte i says
 * observation (i, v) is in the cost.  d_work: work_bytes >= pm_bundle_adjust_workspace(n_views, cap) of device memory the
 * call may scribble on (no alignment asked for).  *d_info: the costs, the used points and observations, iters = trial
 * evaluations, accepted = accepted ones, status 0 = at least one step accepted; 1 = nothing improved (every output equals
 * its input bit for bit; max_iters = 0 ends here); 2 = not enough data (a free view with fewer than 4 used observations,
 * or no used point — cap == 0 and a count of 0 among them: outputs equal inputs, cost_out = cost_in).  Data outcomes are
 * reported there only and the return value stays PM_OK.  PM_E_INVALID: a null context, struct, K, params, d_Rt_out, d_xyz,
 * d_work, d_info or uv[v] of a view below n_views, n_views outside [2, 8], cap < 0, a bad K (S31's rule), max_iters outside
 * [0, 100], gate_px negative or not finite, a fixed_mask holding no view or every view or with a bit at or above n_views,
 * non-zero flags, work_bytes too small.  PM_E_UNSUPPORTED: cap > PM_BA_MAX_POINTS.  In every refusal nothing is written.
 * No per-call state and no allocation: the call may be captured.
 * How many steps it takes grows with the distance of the map from the origin: the pose update turns a camera about the world
 * origin (S40), so far from it a turn and a shift are nearly the same motion and the accepted steps get short.  Measured
 * (tests/backend_cases.py, cost_out over the minimum of a dense solver, 3 and 5 views, status 0 throughout): up to 1e3 units away
 * the default max_iters = 10 reaches the minimum; 3e3 units away 10 steps leave up to 10 times the minimum and 30 reach it;
 * 1e4 units away 10 steps leave about 23 times, 30 steps about 14 times, 100 reach it.  With a geo-referenced or long-trajectory
 * map shift the points and the poses' centres near the origin before the call (X - c, t + R c) and back after it, or raise
 * max_iters.  A window with depths of 1:1000 may end 1e-5 of the cost above the minimum (the damping has fallen away and the
 * block of a far point without parallax no longer factors); a second call continues.  The f32 rows carry half an f32 spacing: 5e-4 units at 1e4. */
int pm_bundle_adjust_dev(pm_ctx* ctx, const pm_tri_views* views, const pm_camera* K, const pm_ba_params* p,
                         double* d_Rt_out, float* d_xyz, uint8_t* d_used, void* d_work, size_t work_bytes, pm_ba_info* d_info);
/* Host in, host out: uv and Rt are arrays of n_views host pointers (Rt[v] may be NULL), n points; xyz is read and written,
 * used may be NULL.  One staged block (the workspace inside it), the device form, one synchronisation. */
int pm_bundle_adjust(pm_ctx* ctx, const float* const* uv, const double* const* Rt, int n_views, int n, const pm_camera* K,
                     const pm_ba_params* p, double* Rt_out, float* xyz, uint8_t* used, pm_ba_info* info);

/* ---- pose-graph optimisation: the last step of a loop closer (ORB-SLAM's OptimizeEssentialGraph, a g2o graph of EdgeSim3 /
 * EdgeSE3, GTSAM's BetweenFactor) — docs/SPEC.md S118-S123.  pm_bowdb_query* proposes a loop, pm_bf_match_guided_* verifies it,
 * pm_ransac_align3d* + pm_align3d_refine* measure the transform between the two maps; this call spreads that loop error over
 * the keyframes, and pm_pgo_move_points* moves the map rows with the keyframes they hang on.  Node i of n_nodes is a pose of 13
 * doubles in pm_ransac_align3d's layout (R row-major, t, s) that takes world points to frame i, x_i = s_i R_i X + t_i;
 * fixed[i] != 0 holds it.  Edge e joins the nodes ab[2e] = a and ab[2e+1] = b (int32) with a measurement Z_e of 13 doubles
 * that takes frame-a coordinates to frame-b coordinates, x_b = s_z R_z x_a + t_z — exactly what pm_align3d_refine_dev leaves
 * in d_T_out when xyz1 are points in frame a and xyz2 the same points in frame b, so that call can write row e of the E x 13
 * array directly — and three square-root weights w[3e .. 3e+2] = (w_r, w_t, w_s) >= 0 of its rotation, translation and scale
 * residuals.  With D = P_b P_a^-1 the residual is (w_r rho, w_t (t_D - t_z), w_s (sigma - 1/sigma)/2): rho the Cayley vector
 * of R_z^T R_D (2 tan(angle/2) about the axis), sigma = s_D / s_z; the cost is the sum of its squares over the used edges.
 * PM_PGO_SIM3 moves 7 parameters per free node; PM_PGO_RIGID moves 6, every s keeps its input bits and the scale residual
 * does not exist.  Levenberg-Marquardt with S24's damping and acceptance (the accepted cost only falls); each step's normal
 * equations are solved by conjugate gradients preconditioned with the nodes' damped diagonal blocks, at most cg_iters
 * iterations or until the preconditioned residual has fallen to cg_tol^2 of its start.  The used set is decided once, at the
 * start: edge e is used iff 0 <= a, b < n_nodes, a != b, every value of Z_e, its weights and both poses is finite, the three
 * scales are > 0, at least one of the two nodes is not fixed, and the rotation residual is away from its singularity at a half
 * turn (1 + tr(R_z^T R_D) > 2^-10).  A free node touched by no used edge is held for the run.  One launch of one workgroup: a
 * latency design (loop closing is rare and runs in the background). */
#define PM_PGO_MAX_NODES 16384
#define PM_PGO_MAX_EDGES 131072
enum { PM_PGO_RIGID = 0, PM_PGO_SIM3 = 1 };

typedef struct pm_pgo_params {
    int32_t model;      /* PM_PGO_RIGID or PM_PGO_SIM3 */
    int32_t max_iters;  /* [0, 100]; 0 = evaluate only (cost_in, the used set), nothing moves */
    int32_t cg_iters;   /* [1, 1000]: conjugate-gradient iterations per step at most */
    int32_t flags;      /* 0 */
    double  cg_tol;     /* finite, in [0, 1): stop a solve when r.z <= cg_tol^2 * (r.z at its start); 0 = run cg_iters */
    int32_t reserved, reserved2;   /* 0 */
} pm_pgo_params;

typedef struct pm_pgo_info {
    double  cost_in, cost_out;   /* sum of squared weighted residuals over the used edges */
    int32_t n_edges_used, n_nodes_free, iters, accepted, cg_total, status;
} pm_pgo_info;

/* Bytes of device workspace pm_pose_graph_optimize_dev needs: pure host arithmetic (no context, no device), a multiple of
 * 16, never decreasing in n_nodes or n_edges; 0 for n_nodes outside [2, PM_PGO_MAX_NODES], n_edges outside
 * [0, PM_PGO_MAX_EDGES] or a model that is not PM_PGO_*.  1 745 bytes per edge and 1 281 per node (SIM3). */
size_t pm_pose_graph_workspace(int n_nodes, int n_edges, int model);
/* Device form.  d_pose_in / d_pose_out: n_nodes x 13 doubles, d_pose_out may be d_pose_in (every pose is read before any is
 * written); d_fixed: n_nodes bytes; d_edge_ab: cap_edges x 2 int32; d_edge_Z: cap_edges x 13 doubles; d_edge_w: cap_edges x 3
 * doubles; the edge count is *d_n_edges clamped to [0, cap_edges] (NULL: cap_edges), rows at or beyond it are neither read nor
 * written.  d_edge_used (may be NULL): one byte per edge below the count, 1 = used.  d_work: work_bytes >=
 * pm_pose_graph_workspace(n_nodes, cap_edges, model) of device memory the call may scribble on (no alignment asked for).
 * *d_info: the costs, the used edges, the free nodes that a used edge touches, iters = trial evaluations, accepted =
 * accepted ones, cg_total = conjugate-gradient iterations over all steps, status 0 = at least one step accepted; 1 = nothing
 * improved (every pose equals its input bit for bit; max_iters = 0 ends here); 2 = not enough data (no used edge, or no fixed
 * node: poses equal inputs, cost_out = cost_in).  Held nodes keep their input bits in every case.  Data outcomes are reported
 * there only and the return value stays PM_OK.  PM_E_INVALID: a null context, params, d_info or array other than d_n_edges
 * and d_edge_used, n_nodes < 2, cap_edges < 0, a model that is not PM_PGO_*, max_iters outside [0, 100], cg_iters outside
 * [1, 1000], cg_tol not finite or outside [0, 1), non-zero flags or reserved, work_bytes too small.  PM_E_UNSUPPORTED: n_nodes >
 * PM_PGO_MAX_NODES or cap_edges > PM_PGO_MAX_EDGES.  In every refusal nothing is written.  No per-call state and no
 * allocation: the call may be captured. */
int pm_pose_graph_optimize_dev(pm_ctx* ctx, const double* d_pose_in, int n_nodes, const uint8_t* d_fixed, const int32_t* d_edge_ab,
                               const double* d_edge_Z, const double* d_edge_w, const int32_t* d_n_edges, int cap_edges,
                               const pm_pgo_params* p, double* d_pose_out, uint8_t* d_edge_used, void* d_work, size_t work_bytes,
                               pm_pgo_info* d_info);
/* Host in, host out over n_edges edges; edge_used may be NULL.  One staged block (the workspace inside it), the device
 * form, one synchronisation. */
int pm_pose_graph_optimize(pm_ctx* ctx, const double* pose_in, int n_nodes, const uint8_t* fixed, const int32_t* edge_ab,
                           const double* edge_Z, const double* edge_w, int n_edges, const pm_pgo_params* p, double* pose_out,
                           uint8_t* edge_used, pm_pgo_info* info);
/* The step a loop closer runs after the graph (S123): map row i, anchored to keyframe k = d_anchor[i], moves with it,
 * X' = P_new,k^-1 (P_old,k X): fp64 with one rounding to f32.  A row with a non-finite input or result, a non-finite pose of
 * its anchor or an anchor outside [0, n_nodes) becomes three quiet NaNs (S101's and pm_gather_pnp_dev's convention).  Rows
 * [0, n), n = *d_n clamped to [0, cap] (d_n NULL: cap); rows beyond are not written; d_out may be d_xyz; one launch, no
 * per-call state.  Statuses: PM_E_INVALID (null pointer, null ctx, negative size), size 0 -> PM_E_UNSUPPORTED.
 * pm_pgo_move_points: the blocking host form. */
int pm_pgo_move_points_dev(pm_ctx* ctx, const double* d_pose_old, const double* d_pose_new, int n_nodes, const int32_t* d_anchor,
                           const float* d_xyz, const int32_t* d_n, int cap, float* d_out);
int pm_pgo_move_points(pm_ctx* ctx, const double* pose_old, const double* pose_new, int n_nodes, const int32_t* anchor,
                       const float* xyz, int n, float* out);

/* ---- 7-point + LMedS: what the reference's call literally selects -----------------
 * cv::findFundamentalMat(..., CV_FM_7POINT) with more than 7 points runs OpenCV 2.4's least-median
 * loop over 7-point minimal solves (main.cpp:95-98) [recalled].  Arithmetic: docs/SPEC.md S13-S15.
 * Hypothesis h in [hyp_begin, hyp_end) samples 7 correspondences and yields up to three models
 * (ids 3h, 3h+1, 3h+2); the model with the smallest median symmetric-epipolar residual wins (ties
 * -> lowest id); inliers are the correspondences within the robust sigma derived from that median.
 * F: row-major, x2^T F x1 = 0, unit Frobenius norm, F[8] >= 0 (pm_f_scale_f33 gives OpenCV's
 * F[8] = 1).  n <= 32768.  pm_lmeds_default_iters: OpenCV's iteration count
 * round(log(1 - confidence) / log(1 - (1 - outlier_ratio)^7)) (300 for 0.99 / 0.45).
 * pm_lmeds_fundamental_dev: n >= 8, device pointers in and out (any output may be NULL),
 * asynchronous on the context's stream.  It cannot report PM_E_NO_MODEL without a host round trip:
 * when no model wins (every sample degenerate, every median +inf) or the range is empty
 * (hyp_begin == hyp_end) it returns PM_OK and leaves F = 0, mask = 0 (all n bytes),
 * n_inliers = 0, best_model = -1 and median = +inf on the device. */
typedef struct pm_lmeds_params {
    int64_t  hyp_begin, hyp_end;
    uint64_t seed;
} pm_lmeds_params;
int pm_lmeds_fundamental(pm_ctx* ctx, const float* xy1, const float* xy2, int n,
                         const pm_lmeds_params* p, double F[9], uint8_t* mask, int* n_inliers,
                         int64_t* best_model, double* median);
int pm_lmeds_fundamental_dev(pm_ctx* ctx, const float* d_xy1, const float* d_xy2, int n,
                             const pm_lmeds_params* p, double* d_F, uint8_t* d_mask,
                             int32_t* d_n_inliers, int64_t* d_best_model, double* d_median);
int pm_lmeds_default_iters(double confidence, double outlier_ratio);
/* The adaptive-iteration RANSAC variant of the same family (OpenCV 2.4 CV_FM_RANSAC [recalled];
 * docs/SPEC.md S16): 7-point models, a correspondence is an inlier when its symmetric-epipolar
 * residual is <= thresh_px^2; hypotheses are visited in id order, a model with more inliers than
 * any before becomes the best and shrinks the iteration budget to
 * log(1 - confidence) / log(1 - (inliers/n)^7) (never above max_iters; OpenCV's defaults: 2000, 0.99,
 * 3 px).  The result equals OpenCV's sequential loop on these models; the device solves and counts
 * ahead in batches.  *iters_run = hypotheses visited. */
typedef struct pm_adaptive_params {
    int64_t  max_iters;
    double   confidence;
    float    thresh_px;
    int32_t  reserved;
    uint64_t seed;
} pm_adaptive_params;
int pm_ransac7_adaptive(pm_ctx* ctx, const float* xy1, const float* xy2, int n,
                        const pm_adaptive_params* p, double F[9], uint8_t* mask, int* n_inliers,
                        int64_t* best_model, int* iters_run);

/* ---- batch of independent image pairs (BASELINE config C5) ----------------------------------
 * One pass of main.cpp:46 -> :49-69 (ratio form) -> :89-91 -> :95-98 per pair, streamed: the batch
 * owns `n_lanes` contexts (stream + scratch + device buffers each); pair j runs on lane
 * j % n_lanes, so H2D of the next pair, the kernels of this one and D2H of the previous one
 * overlap.  Descriptors are f32 rows (L2 matcher, k = 2, `knn_flags` as pm_bf_knn_l2_f32);
 * every pair uses the same ratio and RANSAC parameters.  Host pointers in the jobs should be
 * page-locked (pm_host_register, or any hipHostMalloc'd / torch pinned buffer): pageable memory
 * works but serialises the copies.  Blocking: returns when every result is in `results`
 * (and, when non-NULL, `good`: n_jobs x max_n1 records, first n_good valid per pair; `masks`:
 * n_jobs x max_n1 bytes, inlier flag per surviving match).  results[j].status is PM_OK,
 * PM_E_TOO_FEW (fewer than 8 survivors) or PM_E_NO_MODEL. */
typedef struct pm_pair_job {
    const float* desc1;   /* n1 x dim, image-1 descriptors (query side of main.cpp:46) */
    const float* desc2;   /* n2 x dim */
    const float* kp1_xy;  /* n1 x 2 keypoint pixel coordinates */
    const float* kp2_xy;  /* n2 x 2 */
    int32_t n1, n2;
} pm_pair_job;
typedef struct pm_pair_result {
    double   F[9];
    uint64_t best_key;    /* pm_ransac_key of the winner, 0 if none */
    int32_t  n_good;      /* survivors of the ratio test = correspondences given to RANSAC */
    int32_t  n_inliers;
    int32_t  status;
    int32_t  reserved;
} pm_pair_result;
typedef struct pm_batch pm_batch;   /* opaque */
int pm_batch_create(int device, int n_lanes, int max_n1, int max_n2, int dim, pm_batch** out);
int pm_batch_destroy(pm_batch* b);
int pm_batch_set_option(pm_batch* b, int option, int value);     /* pm_ctx_set_option on every lane's context */
/* Descriptor rows of the jobs: 0 = float32 (default), 1 = uint8 (desc1 / desc2 then point at n x dim BYTES; matched by
 * pm_bf_knn_l2_u8_ratio_dev: same results as the float32 rows of the same values, a quarter of the bytes on the link).
 * One-block jobs: when a job's four arrays lie in ONE host allocation in the order desc1 | desc2 | kp1_xy | kp2_xy
 * (desc2 16-byte, keypoints 8-byte aligned relative to desc1, at most 768 bytes of padding in all), the pair is sent
 * in one copy instead of four — detected per job, nothing to declare. */
int pm_batch_set_desc_type(pm_batch* b, int desc_u8);
/* Host threads that enqueue the pairs of one pm_batch_run call: 0 = automatic (two when the batch has >= 4 lanes: each
 * thread owns half of the lanes and every second job), 1 = the calling thread only, 2.  Results are in job order either way. */
int pm_batch_set_host_threads(pm_batch* b, int n);
int pm_batch_run(pm_batch* b, const pm_pair_job* jobs, int n_jobs, float ratio, int knn_flags,
                 const pm_ransac_params* p, pm_pair_result* results, pm_match* good, uint8_t* masks);
/* Page-lock / release a caller-owned host buffer (hipHostRegister) so the batch copies overlap. */
int pm_host_register(void* ptr, size_t bytes);
int pm_host_unregister(void* ptr);

/* ---- the path over the GPUs of one node (SURVEY.md 8b `pm_ransac_reduce`, 8e) ----------------------------
 * One context per (device, lane), one RCCL communicator set per lane (ncclCommInitAll over xGMI), ONE HOST THREAD PER
 * DEVICE that enqueues that device's launches and collectives; RCCL is bound at run time, so single-GPU users never
 * load it.  `devices`: HIP ordinals (NULL: 0 .. n_dev-1).
 *   pm_mgpu_ransac_fundamental  main.cpp:95-98 with the hypothesis ids cut into n_dev contiguous ranges over
 *       replicated correspondences; the exchange is ONE all-gather of the 80-byte pm_ransac_record per device
 *       (arg-max all-reduce with its payload); every device finishes from the winning record, device 0's answer
 *       is returned.  Same bits as pm_ransac_fundamental for any n_dev (tests assert it).
 *   pm_mgpu_match_ransac        main.cpp:46 -> :49-69 (ratio form) -> :89-91 -> :95-98 (BASELINE config C4): query
 *       rows cut into n_dev contiguous blocks (train set replicated), all-gather #1 of the survivor blocks, RANSAC
 *       as above over the gathered view, all-gather #2 of the records.  desc1/desc2: n x dim float32 rows
 *       (binary == 0, L2, knn_flags as pm_bf_knn_l2_f32) or n x dim bytes (binary != 0, Hamming).  Outputs: `good`
 *       (n1 records, first *n_good valid, query order, queryIdx = row of desc1), F, mask (per good match), counts.
 *       PM_E_TOO_FEW / PM_E_NO_MODEL as pm_ransac_fundamental (good / *n_good are valid either way).  Host inputs go
 *       through ONE pinned staging copy that all devices' copy engines read concurrently.
 * Streamed form (round 3) — what a caller with many image pairs against one train image uses:
 *   pm_mgpu_set_lanes           1 .. 4 lanes per device (stream + communicator + buffers each); pair j runs on lane
 *                               j mod L, so pair j+1's matcher overlaps pair j's two all-gathers.  Default 1.
 *   pm_mgpu_set_train[_dev]     the replicated train side (main.cpp:36-40, image 2) made RESIDENT on every device: uploaded
 *                               once from host memory, or adopted from per-device device pointers the caller keeps alive.
 *   pm_mgpu_submit_dev          one image pair from DEVICE pointers: d_desc1[g] / d_kp1_xy[g] = device g's block of
 *                               rows[g] query rows (blocks in device order = query order; equal blocks, the last possibly
 *                               short, when match records with global queryIdx are wanted).  Returns at once with a ticket.
 *                               A lane holds one pair's results until they are collected: at most `lanes` pairs are in flight.
 *   pm_mgpu_collect             blocks for one ticket (any order): result as pm_pair_result (status
 *                               PM_OK / PM_E_TOO_FEW / PM_E_NO_MODEL), optional match records (sum of rows) and mask.
 *   pm_mgpu_allgather_latency   the collective by itself: microseconds per all-gather of bytes_per_device.
 *   pm_mgpu_batch_run           BASELINE config C5 behind the ABI: pm_batch_run with pair p on device p mod n_dev, one host
 *                               thread per device, results in job order (arguments as pm_batch_create + pm_batch_run). */
typedef struct pm_mgpu pm_mgpu;   /* opaque */
int pm_mgpu_create(int n_dev, const int* devices, pm_mgpu** out);
int pm_mgpu_destroy(pm_mgpu* mg);
int pm_mgpu_size(const pm_mgpu* mg);
pm_ctx* pm_mgpu_ctx(pm_mgpu* mg, int i);        /* device i's lane-0 context (options, timing); owned by mg */
pm_ctx* pm_mgpu_lane_ctx(pm_mgpu* mg, int i, int lane);
int pm_mgpu_ransac_fundamental(pm_mgpu* mg, const float* xy1, const float* xy2, int n, const pm_ransac_params* p,
                               double F[9], uint8_t* mask, int* n_inliers, uint64_t* best_key);
int pm_mgpu_match_ransac(pm_mgpu* mg, const void* desc1, int n1, const void* desc2, int n2, int dim, int binary,
                         const float* kp1_xy, const float* kp2_xy, float ratio, int knn_flags,
                         const pm_ransac_params* p, pm_match* good, int* n_good, double F[9], uint8_t* mask,
                         int* n_inliers, uint64_t* best_key);
int pm_mgpu_set_lanes(pm_mgpu* mg, int n_lanes);
int pm_mgpu_set_train(pm_mgpu* mg, const void* desc2, int n2, int dim, int binary, const float* kp2_xy);
int pm_mgpu_set_train_dev(pm_mgpu* mg, const void* const* d_desc2, int n2, int dim, int binary, const float* const* d_kp2_xy);
int pm_mgpu_submit_dev(pm_mgpu* mg, const void* const* d_desc1, const int32_t* rows, const float* const* d_kp1_xy,
                       float ratio, int knn_flags, const pm_ransac_params* p, int* ticket);
int pm_mgpu_collect(pm_mgpu* mg, int ticket, pm_pair_result* result, pm_match* good, uint8_t* mask);
int pm_mgpu_allgather_latency(pm_mgpu* mg, int bytes_per_device, int reps, double* us_per_collective);
int pm_mgpu_batch_run(pm_mgpu* mg, int n_lanes, int max_n1, int max_n2, int dim, const pm_pair_job* jobs, int n_jobs,
                      float ratio, int knn_flags, const pm_ransac_params* p, pm_pair_result* results, pm_match* good,
                      uint8_t* masks);
int pm_mgpu_batch_set_option(pm_mgpu* mg, int option, int value);   /* pm_ctx_set_option on every context of mg */

/* ---- feature front end (replaces main.cpp:22-26 detect and main.cpp:36-40 compute) — docs/SPEC.md S53-S57 -------------
 * Difference-of-Gaussian keypoints and 128-D gradient descriptors from 8-bit grey pixels, on the device: the HIP port of
 * the host extractor behind `pm_cli --img1 --img2` (Lowe's scheme: 3 scales per octave, sigma0 1.6, contrast and edge
 * tests, dominant orientation, 4x4x8 histogram, normalise -> clip 0.2 -> renormalise -> x512 -> 0..255).  Keypoints, their
 * order and every Gaussian level equal the host extractor's bit for bit; descriptors equal it except where the device's
 * atan2f or fp64 exp differs from the host's in the last bit (rare rows, one element off by one).
 *   d_img      h rows of `stride` >= w bytes, row-major.
 *   max_kp     the strongest max_kp extrema are described: |response| descending, ties in scan order (octave, level,
 *              y, x ascending).  Every output array holds max_kp rows.
 *   contrast, edge_r   the host's defaults are 0.03 and 10.
 *   d_kp_xy    n x 2 float, input-image pixels.        d_desc_u8   n x 128 bytes (feeds pm_bf_knn_l2_u8*_dev; may be NULL).
 *   d_desc_f32 n x 128 u8-valued floats (may be NULL). d_meta      n x 4 float {sigma in input pixels, dominant angle in
 *   radians, |DoG response|, octave} (may be NULL).    d_n         device int32: the number of rows written.
 * Rows keep the selection order; rows whose patch leaves the image or whose descriptor has no energy are dropped.
 * w < 32 or h < 32: PM_OK, *d_n = 0.  More than 100 000 000 pixels: PM_E_UNSUPPORTED.
 * Candidate capacity.  Extrema are appended to a buffer of bounded capacity (PM_OPT_FEAT_CAPACITY; default
 * max(65536, 8 * max_kp), at most 2^28 like the option); the device counter keeps counting past it.  When an image
 * has more extrema than that, the _dev form writes *d_n = -1 and NO rows (never a subset): raise the option and call
 * again.  The blocking form reads the counter, grows the buffer to the need and runs again by itself (it allocates
 * and frees its device copy of the image and its output block on every call); *n_out is written only after every row
 * has arrived.
 * The _dev form enqueues on the context's stream and does not synchronise (the context's feature buffer grows on the
 * first call and when a larger image or capacity comes: one stream synchronisation and a reallocation).  Both forms
 * return PM_E_UNSUPPORTED on a capturing stream before anything is allocated, like the matcher.
 * Timing names: "feat_blur", "feat_decimate", "feat_extrema", "feat_rank", "feat_describe", "feat_compact", "feat_gather". */
int pm_detect_describe_dev(pm_ctx* ctx, const uint8_t* d_img, int w, int h, int stride, int max_kp, float contrast,
                           float edge_r, float* d_kp_xy, uint8_t* d_desc_u8, float* d_desc_f32, float* d_meta, int32_t* d_n);
int pm_detect_describe(pm_ctx* ctx, const uint8_t* img, int w, int h, int stride, int max_kp, float contrast, float edge_r,
                       float* kp_xy, uint8_t* desc_u8, float* desc_f32, float* meta, int32_t* n_out);
/* TEST AND INSPECTION SURFACE — pm_detect_level_get and pm_detect_tables exist so that the scale space and the tables can
 * be pinned separately from the rest (tests/test_features_device_*.py).  They carry NO stability promise: they may change
 * or go with the kernels' internals, and no other entry point depends on them.
 * pm_detect_level_get: Gaussian level `level` (0 .. 5) of octave `octave` as the LAST detect call on this context left it;
 * *w_out x *h_out floats into plane (cap_floats of room; plane may be NULL to ask for the size only).  Synchronises. */
int pm_detect_level_get(pm_ctx* ctx, int octave, int level, float* plane, int cap_floats, int* w_out, int* h_out);
/* The host-computed tables the kernels read (S53, S56; no GPU needed): tap_radius[6] and taps[6 * 25] (row 0: the base blur
 * of octave 0, rows 1 .. 5 the level increments; row i holds 2 * tap_radius[i] + 1 values), ori_weight[3 * 393] (inner level
 * l, index dx^2 + dy^2), ori_radius[3], desc_radius[3], cos_sin[72] (36 cosines, then 36 sines of the bin-centre angles).
 * Any pointer may be NULL. */
int pm_detect_tables(int32_t* tap_radius, double* taps, double* ori_weight, int32_t* ori_radius, int32_t* desc_radius,
                     double* cos_sin);

/* ---- binary descriptors on the same front end — docs/SPEC.md S58-S60 -----------------------------------------------------
 * The keypoints, selection order and dominant orientation of pm_detect_describe*, with a steered BRIEF-style descriptor in
 * place of the gradient histogram: 256 comparisons of pixels of the keypoint's own Gaussian level at integer offsets taken
 * from a table pre-rotated to the 36 orientation bins and scaled to the level (S59).  Bit i is 1 where the first pixel of
 * test i is smaller than the second; byte i >> 3, bit i & 7, least significant first (ORB's convention).
 *   d_desc_bits  n x 32 bytes: feeds pm_bf_knn_hamming_u8*, pm_bf_match_cross_hamming_u8*, pm_bf_knn_guided_hamming_u8*
 *                (cols = 32) where it lies.  Required.
 * Every other argument, the status codes, the w < 32 || h < 32 rule, the capture refusal, the candidate capacity with
 * *d_n = -1 and no rows on overflow, and the blocking form's grow-and-retry are those of pm_detect_describe*.  A row is
 * dropped only where its patch leaves the image (the same border rule: the offsets stay within the descriptor radius);
 * there is no energy rule, so the rows of pm_detect_describe* are a subsequence of these, with equal keypoints and meta.
 * Given the same orientation bin the 32 bytes equal the host extractor's (`pm_cli --descriptor bits`) exactly; the bin can
 * differ only where the device's atan2f differs from the host's in the last bit.  pm_detect_level_get works after these
 * calls too.  Timing names: as above, with "feat_describe_bits" and "feat_gather_bits" in place of "feat_describe" and
 * "feat_gather". */
int pm_detect_describe_bits_dev(pm_ctx* ctx, const uint8_t* d_img, int w, int h, int stride, int max_kp, float contrast,
                                float edge_r, float* d_kp_xy, uint8_t* d_desc_bits, float* d_meta, int32_t* d_n);
int pm_detect_describe_bits(pm_ctx* ctx, const uint8_t* img, int w, int h, int stride, int max_kp, float contrast, float edge_r,
                            float* kp_xy, uint8_t* desc_bits, float* meta, int32_t* n_out);
/* TEST AND INSPECTION SURFACE (no stability promise, no GPU needed): base1024 = the 256 tests (x1, y1, x2, y2) of S58 as
 * int8, row-major; steered110592 = the int8 offsets (dx1, dy1, dx2, dy2) of S59, shape [3 levels][36 bins][256 tests][4].
 * Either pointer may be NULL. */
int pm_detect_bits_table(int8_t* base1024, int8_t* steered110592);

/* ---- sparse optical-flow tracking: pyramidal Lucas-Kanade — docs/SPEC.md S61-S66 ------------------------------------------
 * The frame-to-frame way to correspondences (cv::calcOpticalFlowPyrLK, cv::cuda::SparsePyrLKOpticalFlow): the points of the
 * previous frame are tracked into the next one, with sub-pixel positions, no second detection, no descriptors and no k-NN.
 * Inverse-compositional form on integer samples: every sum is an exact integer sum, so the result is a function of the two
 * images, the points and the parameters alone (bit for bit the plain-C statement tests/lk_ref.c).  OpenCV's results are
 * close, not equal: its oscillation rule is not restated and its sampling differs.
 *
 * pm_pyramid is an image pyramid on the device (S61: level l + 1 is a 5-tap binomial reduction of level l, (w + 1) / 2 by
 * (h + 1) / 2 pixels; it exists while l + 1 <= max_level and both sides are at least 16).  It is an object of its own so that
 * a video loop builds ONE pyramid per frame: frame k's pyramid is the "previous" pyramid of the next call.
 *   pm_pyramid_create   allocates every level (the only allocation of the tracking path).  PM_E_INVALID: null pointers,
 *                       max_level outside [0, 7], w or h < 1.  PM_E_UNSUPPORTED: w or h below 16, more than 100 000 000
 *                       pixels, a capturing stream.
 *   pm_pyramid_build_dev  d_img: h rows of `stride` >= w bytes on the device.  Enqueues on the context's stream: one copy and
 *                       one launch per level above 0; does not synchronise.
 *   pm_pyramid_level_get  TEST AND INSPECTION SURFACE (no stability promise).  Level `level` as the last build left it, *w_out
 *                       x *h_out bytes into plane (cap bytes of room; plane may be NULL to ask for the size only); level = -1
 *                       writes the number of levels to *w_out.  Synchronises.
 * pm_lk_params: every field is checked; anything out of range, unknown flag bits or reserved != 0 is PM_E_INVALID. */
typedef struct pm_pyramid pm_pyramid;            /* opaque; device memory owned by the object */
#define PM_LK_USE_INITIAL 1
typedef struct pm_lk_params {
    int32_t win_radius;   /* 2 .. 15 (window 2r+1; OpenCV's 21x21 is 10) */
    int32_t max_level;    /* 0 .. 7; the top level used is min(max_level, levels of the pyramids - 1) */
    int32_t max_iters;    /* 1 .. 100 (OpenCV: 30) */
    float   eps;          /* finite, >= 0 (OpenCV: 0.01) */
    float   min_eig;      /* finite, >= 0, grey-level^2 units (OpenCV: 1e-4) */
    float   fb_thresh;    /* 0 = no forward-backward check; else finite, > 0, pixels */
    int32_t flags;        /* PM_LK_USE_INITIAL = 1 */
    int32_t reserved;     /* 0 */
} pm_lk_params;
int pm_pyramid_create(pm_ctx* ctx, int w, int h, int max_level, pm_pyramid** out);
int pm_pyramid_destroy(pm_pyramid* pyr);
int pm_pyramid_build_dev(pm_ctx* ctx, pm_pyramid* pyr, const uint8_t* d_img, int stride);
int pm_pyramid_level_get(pm_ctx* ctx, const pm_pyramid* pyr, int level, uint8_t* plane, int cap, int* w_out, int* h_out);
/* Tracking, ONE launch ("lk_track": one wave per point; level loop, iterations and the backward track of the
 * forward-backward check inside it).  Enqueues on the context's stream, allocates nothing, keeps no per-call state.
 *   d_pts     cap x 2 float, pixels of the previous frame.   d_n   device int32 count, clamped to [0, cap]; NULL = cap.  The
 *             -1 that pm_detect_describe*_dev writes on overflow counts as 0, so the call chains after it with no host
 *             round trip.  Rows at or beyond the count are neither read nor written.
 *   d_init    cap x 2 float initial positions in the next frame: required with PM_LK_USE_INITIAL, NULL without it.
 *   d_out     cap x 2 float: the last guess, written for EVERY status.   d_status  cap bytes: 1 tracked, 2 left the image
 *             (non-finite input lands here), 3 flat (eigenvalue or determinant test at level 0), 4 failed the
 *             forward-backward check.  A point is a correspondence iff its status is 1.
 *   d_err     mean absolute grey difference of the last window evaluated at level 0, -1 if none (may be NULL).
 *   d_fb      forward-backward distance in pixels, -1 where no backward track ran (may be NULL).
 * The gather form adds one launch ("lk_compact") that keeps the status-1 points in input order: d_xy1 (the input points),
 * d_xy2 (their positions in the next frame), d_src_idx (row in d_pts; may be NULL) and *d_count.  {d_xy1, d_xy2,
 * counts = d_count, parts = 1, cap} is a pm_points_view for every *_run_dev estimator.  d_out / d_status may be NULL there
 * (the rows then live in the context's scratch arena, which may grow on the first call: one stream synchronisation).
 * PM_E_INVALID: null arguments, parameters out of range, reserved != 0, d_init not matching the flag, pyramids of different
 * shape or level count or of another device, cap < 0.  PM_E_UNSUPPORTED: cap == 0 (n == 0 in the host form), and a
 * capturing stream (refused before anything is allocated or launched, like the matcher and the feature front end).
 * pm_track_lk is the blocking host form: host images and points in, host results out; it builds both pyramids and frees
 * everything it allocated.  Timing names: "lk_pyr_down", "lk_track", "lk_compact". */
int pm_track_lk_dev(pm_ctx* ctx, const pm_pyramid* prev, const pm_pyramid* next, const float* d_pts, const int32_t* d_n, int cap,
                    const float* d_init, const pm_lk_params* p, float* d_out, uint8_t* d_status, float* d_err, float* d_fb);
int pm_track_lk_gather_dev(pm_ctx* ctx, const pm_pyramid* prev, const pm_pyramid* next, const float* d_pts, const int32_t* d_n,
                           int cap, const float* d_init, const pm_lk_params* p, float* d_xy1, float* d_xy2, int32_t* d_src_idx,
                           int32_t* d_count, float* d_out, uint8_t* d_status);
int pm_track_lk(pm_ctx* ctx, const uint8_t* img1, const uint8_t* img2, int w, int h, int stride, const float* pts, int n,
                const float* init, const pm_lk_params* p, float* out, uint8_t* status, float* err, float* fb);

/* ---- corners to start and replenish tracks: minimum-eigenvalue (Shi-Tomasi) detection — docs/SPEC.md S67-S70 ---------------
 * The point source of the tracking route (cv::goodFeaturesToTrack with a mask): the strongest corners of level 0 of a built
 * pm_pyramid that keep a minimum distance from each other and from an existing point set.  No scale space, no descriptors.
 * The score of a pixel is the smaller eigenvalue of the gradient matrix over its (2r+1)^2 block, from exact integer sums, in
 * the unit of pm_lk_params.min_eig: at an integer pixel it is bit for bit the value the tracker tests against min_eig at
 * level 0 for win_radius == block_radius, and the region searched (r+1 <= x <= w-r-3, likewise y) is exactly the set of
 * integer points whose tracking template stays inside level 0.  A corner found with min_eig = m therefore never comes back
 * from pm_track_lk* with status 3 at that radius and min_eig <= m.  Candidates are strict 3 x 3 maxima of the score (S68),
 * ranked by score, ties in scan order (S69), cut at quality * the best score, and taken greedily while no keep point and no
 * corner taken before lies nearer than min_dist (S70).  The result is a function of the image, the keep points and the
 * parameters alone (bit for bit the plain-C statement tests/corner_ref.c).
 *   pm_corners_dev   d_keep: cap_keep x 2 float obstacles at any position (NULL with cap_keep 0); d_n_keep: device int32
 *             count, clamped to [0, cap_keep], NULL = cap_keep.  A non-finite keep point blocks nothing.  Writes at most
 *             max_corners rows of d_xy (x, y as floats, integer valued), d_score (may be NULL) and *d_n, in order of
 *             acceptance.  Enqueues three launches on the context's stream and does not synchronise; scratch comes from the
 *             context's arena, which may grow on the first call or with a larger capacity (one stream synchronisation).
 *   pm_corners_replenish_dev   the video-loop form, in place: n = *d_count clamped to [0, cap]; rows [0, n) of d_pts are the
 *             obstacles; up to min(target, cap) - n corners are appended at rows n .. and *d_count becomes n + m; *d_n_new
 *             (may be NULL) = m; d_score (may be NULL) holds cap floats and is written at the new rows only.  Chains after
 *             pm_track_lk_gather_dev (its d_xy2, d_count) with no host round trip, and gives the rows pm_corners_dev gives
 *             with keep = d_pts[0 .. n).
 *   pm_corners   the blocking host form: builds level 0 only and frees what it allocated (images below 16 pixels a side are
 *             PM_E_UNSUPPORTED, as for pm_pyramid_create).
 * Overflow: when more candidates pass S68 than the capacity, the _dev forms write *d_n = -1 (replenish: *d_n_new = -1, *d_count
 * unchanged) and no rows, never a subset; pm_corners grows the capacity and runs again by itself.  In the replenish form
 * *d_n_new is the ONLY overflow signal: with d_n_new == NULL an overflow cannot be told from "no corner found", so a caller
 * that does not size the capacity for its frames passes the pointer.
 * Cost: the ranking counts smaller keys, so its work grows with the SQUARE of the candidate count (the selection's with
 * candidates x accepted corners).  A few thousand candidates, the case of a real frame with a sensible min_eig, cost tens of
 * microseconds; a large noisy frame with min_eig near 0 can produce millions, and a capacity near its ceiling of 2^24 then
 * admits a launch of ~1e14 key comparisons, minutes on the device.  Keep min_eig above the noise floor and the capacity near
 * the default; pm_corners grows the capacity to the exact need, whatever it is.  Scaling with the candidate count has not
 * been measured.
 * PM_E_INVALID: null required pointers, a parameter out of range, flags or reserved != 0, max_corners, cap, cap_keep, n_keep
 * or target < 0, a pyramid of another device.  PM_E_UNSUPPORTED: max_corners == 0, cap == 0 in the replenish form, and a
 * capturing stream (refused before anything is allocated or launched).  An empty search region gives 0 corners and PM_OK.
 * Timing names: "corner_extrema", "corner_rank", "corner_select". */
typedef struct pm_corner_params {
    int32_t block_radius;  /* 1 .. 15 (OpenCV's blockSize 3 is 1; use the tracker's win_radius to share its eigenvalue) */
    float   min_eig;       /* finite, >= 0: absolute floor, the unit of pm_lk_params.min_eig */
    float   quality;       /* 0 .. 1: relative floor against the strongest candidate (OpenCV's qualityLevel); 0 = off */
    float   min_dist;      /* finite, 0 .. 1e6, pixels */
    int32_t capacity;      /* candidate capacity of a run; 0 = max(65536, 8 * max_corners); else 1 .. 2^24 */
    int32_t flags;         /* 0 */
    int32_t reserved[2];   /* 0 */
} pm_corner_params;
int pm_corners_dev(pm_ctx* ctx, const pm_pyramid* pyr, const pm_corner_params* p, const float* d_keep, const int32_t* d_n_keep,
                   int cap_keep, int max_corners, float* d_xy, float* d_score, int32_t* d_n);
int pm_corners_replenish_dev(pm_ctx* ctx, const pm_pyramid* pyr, const pm_corner_params* p, float* d_pts, int32_t* d_count,
                             int cap, int target, float* d_score, int32_t* d_n_new);
int pm_corners(pm_ctx* ctx, const uint8_t* img, int w, int h, int stride, const pm_corner_params* p, const float* keep, int n_keep,
               int max_corners, float* xy, float* score, int32_t* n_out);

/* ---- describe given points: oriented 256-bit descriptors on a pm_pyramid — docs/SPEC.md S71-S74 ---------------------------
 * The `compute` half of a corner front end (ORB is "corners + steered BRIEF"): 32 bytes per GIVEN point, so that the corners of
 * pm_corners* and the tracked points of pm_track_lk* can be matched by appearance with pm_bf_knn_hamming_u8*,
 * pm_bf_match_cross_hamming_u8* and the guided Hamming matchers (cols = 32), and located against a map through
 * pm_gather_pnp_dev.  Points are level-0 pixels; on level p->level the centre is the nearest pixel of (x, y) * 2^-level (ties to
 * even).  A point is INVALID when a coordinate is not finite or beyond 1e6 in magnitude, or when the 35 x 35 square round the
 * centre leaves the level (17 <= cx <= w_l - 18, likewise cy): its row is 32 zero bytes, valid 0, bin 255.  Otherwise the
 * orientation bin (0 .. 35, the bin centres of S56) comes from the intensity centroid over the disc of radius 15, as an arg-max
 * of int64 dot products (S72; a flat patch gives bin 0), and bit i compares the 5 x 5 box sums at the two points of test i of
 * the S58 pattern steered to that bin (S73, S74; packing as S60).  PM_DESCRIBE_UPRIGHT skips the orientation: the unrotated
 * pattern, bin 36.  Everything is integer arithmetic: the rows are a function of the level, the points and the flags alone
 * (bit for bit the plain-C statement tests/describe_ref.c).
 *   pm_describe_points_dev   n = *d_n clamped to [0, cap], NULL = cap; the -1 that pm_corners_dev / pm_detect_describe*_dev write
 *             on overflow counts as 0.  Rows [0, n) of d_desc (cap x 32 bytes, any alignment), d_valid and d_bin (cap bytes each,
 *             either may be NULL) are written; rows at or beyond n are neither read nor written.  One launch on the context's
 *             stream, no synchronisation — except on a context's FIRST describe call, which uploads the two tables (38 KiB) into
 *             a context-owned buffer with a blocking copy (one synchronisation, as the feature buffer of pm_detect_describe*).
 *   pm_describe_points_gather_dev   adds one launch: the valid rows in input order.  d_xy (cap x 2) receives bit copies of their
 *             input points, d_desc (cap x 32) their rows, d_src_idx (may be NULL) their input row numbers, *d_count their
 *             number.  d_xy must not overlap d_pts.  The aligned rows live in the context's scratch arena, which may grow on
 *             the first call or with a larger cap (one stream synchronisation).  Chains after pm_corners_dev (its d_xy, d_n)
 *             and after pm_track_lk_gather_dev (its d_xy2, d_count); d_desc and *d_count feed the Hamming matchers.
 *   pm_describe_points   the blocking host form: builds the pyramid up to p->level, runs, downloads, and frees what it
 *             allocated (images below 16 pixels a side are PM_E_UNSUPPORTED, as for pm_pyramid_create); valid, bin may be NULL.
 *   pm_describe_points_tables   no GPU needed: cos_sin_q20 = nearbyint(2^20 cos theta_b) for b = 0 .. 35, then the sines;
 *             steered = int8 [37][256][4] (dx1, dy1, dx2, dy2), row 36 being the S58 pattern.  Either may be NULL.
 * PM_E_INVALID: null required pointers, level outside 0 .. 7 or not a level of the pyramid, unknown flag bits, reserved != 0,
 * cap or n < 0, a pyramid of another device.  PM_E_UNSUPPORTED: cap == 0 (n == 0 in the host form), and a capturing stream
 * (refused first, before anything is allocated, synchronised or launched).
 * Timing names: "desc_points", "desc_compact". */
#define PM_DESCRIBE_UPRIGHT 1   /* no orientation: the unrotated pattern, bin 36 */
typedef struct pm_describe_params {
    int32_t level;         /* 0 .. levels of the pyramid - 1 */
    int32_t flags;         /* 0 or PM_DESCRIBE_UPRIGHT */
    int32_t reserved[2];   /* 0 */
} pm_describe_params;
int pm_describe_points_dev(pm_ctx* ctx, const pm_pyramid* pyr, const float* d_pts, const int32_t* d_n, int cap,
                           const pm_describe_params* p, uint8_t* d_desc, uint8_t* d_valid, uint8_t* d_bin);
int pm_describe_points_gather_dev(pm_ctx* ctx, const pm_pyramid* pyr, const float* d_pts, const int32_t* d_n, int cap,
                                  const pm_describe_params* p, float* d_xy, uint8_t* d_desc, int32_t* d_src_idx, int32_t* d_count);
int pm_describe_points(pm_ctx* ctx, const uint8_t* img, int w, int h, int stride, const float* pts, int n,
                       const pm_describe_params* p, uint8_t* desc, uint8_t* valid, uint8_t* bin);
int pm_describe_points_tables(int32_t cos_sin_q20[72], int8_t steered[37 * 256 * 4]);

/* ---- apply a 2-D model: warp an 8-bit image by H or A, transform points — docs/SPEC.md S75-S78 -----------------------------
 * The step after pm_ransac_homography_run_dev / pm_ransac_affine_run_dev and their refinements (cv::warpPerspective,
 * cv::warpAffine and cv::perspectiveTransform after cv::findHomography / cv::estimateAffine2D): the stabilised frame, the
 * mosaic tile, the registered scan, and the tracker's PM_LK_USE_INITIAL guess from the last H, without leaving the stream.
 * M is 9 doubles, row-major; with PM_WARP_AFFINE 6 doubles as d_A lies (2 x 3), lifted with the last row (0, 0, 1).  Output
 * pixel (x, y) samples the source at M (x, y, 1)^T: the d_H of x2 ~ H x1 pulls image 2 into frame 1 as it lies.  With
 * PM_WARP_INVERT the adjugate of M takes its place (cv::warpPerspective's default direction).  Positions are fp64, rounded to
 * 1/32 pixel (ties to even); the sample is the integer bilinear sum of four taps with weights that add to 1024,
 * out = (sum + 512) >> 10: every output byte is a function of the inputs alone (bit for bit the plain-C statement
 * tests/warp_ref.c; OpenCV's bytes are close, not equal).  A tap outside the source contributes border_value, or with
 * PM_WARP_REPLICATE the nearest source pixel; a tap of weight zero is never read.  A pixel is VALID when its position is
 * usable (W != 0, finite, below 2^30 in magnitude) and every tap of non-zero weight lies inside the source, under both border
 * modes; pixels whose position is not usable are border_value.
 *   pm_warp_dev   one launch on the context's stream, nothing allocated, the model read on the device.  d_src: sh rows of
 *             sstride bytes, sw used; d_dst: dh rows of dstride bytes, dw written, the rest untouched; base pointers and strides
 *             of any alignment.  d_valid (may be NULL): dw x dh bytes, stride dw, 1 = valid.  d_info (may be NULL): cleared by
 *             one 8-byte async memset before the launch; n_valid = number of valid pixels; status 1 = M (or, with
 *             PM_WARP_AFFINE, its lift) has a non-finite entry or a determinant that is zero or not finite, 2 = every entry of
 *             M is zero (the "no model" value the estimators leave).  With a status other than 0 the whole output is
 *             border_value, nothing is valid, and the call still returns PM_OK: data outcomes are reported in *d_info only.
 *   pm_warp   the blocking host form: one staged device block, freed before it returns.
 *   pm_transform_points_dev   out = ((float)(X / W), (float)(Y / W)) with (X, Y, W) = M (x, y, 1)^T in fp64; flags:
 *             PM_WARP_INVERT, PM_WARP_AFFINE.  Both coordinates are NaN (which pm_track_lk* turns into status 2) when W == 0,
 *             a quotient is not finite, or the model is one pm_warp_dev reports.  n = *d_n clamped to [0, cap], NULL = cap,
 *             -1 counts as 0; rows at or beyond n are neither read nor written.  d_out may equal d_pts.  One launch.
 *   pm_transform_points   the blocking host form.
 * PM_E_INVALID: null required pointers, unknown flag bits, border_value outside 0 .. 255, reserved != 0, a size below 1, a
 * stride below its width, cap or n < 0, d_src and d_dst ranges that overlap.  PM_E_UNSUPPORTED: more than 100 000 000 pixels
 * on either side, cap == 0 (n == 0 in the host form), and a capturing stream (refused first, before anything is launched).
 * Timing names: "warp_bilinear", "warp_points". */
#define PM_WARP_INVERT    1   /* sample through the adjugate of M */
#define PM_WARP_REPLICATE 2   /* taps outside the source take the nearest source pixel */
#define PM_WARP_AFFINE    4   /* M is 6 doubles (2 x 3) */
typedef struct pm_warp_params {
    int32_t flags;          /* PM_WARP_* */
    int32_t border_value;   /* 0 .. 255 */
    int32_t reserved[2];    /* 0 */
} pm_warp_params;
typedef struct pm_warp_info {
    int32_t status;         /* 0 ok, 1 singular or non-finite, 2 zero model */
    int32_t n_valid;
} pm_warp_info;
int pm_warp_dev(pm_ctx* ctx, const uint8_t* d_src, int sw, int sh, int sstride, const double* d_M, const pm_warp_params* p,
                uint8_t* d_dst, int dw, int dh, int dstride, uint8_t* d_valid, pm_warp_info* d_info);
int pm_warp(pm_ctx* ctx, const uint8_t* src, int sw, int sh, int sstride, const double* M, const pm_warp_params* p,
            uint8_t* dst, int dw, int dh, int dstride, uint8_t* valid, pm_warp_info* info);
int pm_transform_points_dev(pm_ctx* ctx, const double* d_M, int flags, const float* d_pts, const int32_t* d_n, int cap, float* d_out);
int pm_transform_points(pm_ctx* ctx, const double* M, int flags, const float* pts, int n, float* out);

/* ---- lens distortion: undistort points and images, remap through a map — docs/SPEC.md S79-S83 ------------------------------
 * The step in front of the calibrated estimators (cv::undistortPoints before cv::findEssentialMat / cv::solvePnPRansac) and in
 * front of the image front end (cv::undistort, cv::initUndistortRectifyMap + cv::remap), without leaving the stream.  The
 * model is OpenCV's with 5 coefficients (k1, k2, p1, p2, k3): for normalised (x, y), r2 = x^2 + y^2,
 * rad = 1 + ((k3 r2 + k2) r2 + k1) r2, xd = x rad + (2 p1 x y + p2 (r2 + 2 x^2)), yd = y rad + (p1 (r2 + 2 y^2) + 2 p2 x y),
 * pixel = (fx xd + cx, fy yd + cy).  All arithmetic is fp64 without fused operations and without transcendental functions:
 * every output is a function of the inputs alone (bit for bit the plain-C statement tests/undistort_ref.c).
 * K (the camera the lens belongs to), lens, R and K_new (the camera of the ideal pixels) are HOST pointers read at call time:
 * lens == NULL means all coefficients zero, R == NULL identity (the rotation step is then skipped, not multiplied through),
 * K_new == NULL means K.  R is 9 doubles, row-major: the rectifying rotation of cv::undistortPoints /
 * cv::initUndistortRectifyMap.  The image forms use its TRANSPOSE as its inverse; R is checked for finiteness only, not for
 * being a rotation.
 *   pm_distort_points_dev     ideal pixel under K_new -> distorted pixel under K (S80): normalise by K_new, apply R^T and divide
 *             by Z (when R is given), distort, project by K, round to fp32.  Both outputs are NaN when Z <= 0, rad <= 0 or a
 *             value is not finite.
 *   pm_undistort_points_dev   the inverse (S81): exactly `iters` fixed-point rounds as cv::undistortPoints runs them, then a
 *             convergence gate: the point is re-distorted and kept only when its pixel error is at most tol_px (and rad > 0);
 *             then R (Z > 0 required) and K_new.  A rejected point is a NaN pair: the estimators never count one as an inlier and
 *             pm_track_lk* turns it into status 2.
 *             Both: n = *d_n clamped to [0, cap], NULL = cap, -1 counts as 0; rows at or beyond n are neither read nor written;
 *             d_out may equal d_pts.  One launch.  pm_undistort_points / pm_distort_points: the blocking host forms.
 *   pm_undistort_dev   output pixel (u, v) under K_new samples the source at the position pm_distort_points gives it, rounded
 *             to 1/32 pixel (S82); sampling, the valid mask, n_valid and the border modes are pm_warp_dev's (S77), and so are
 *             the buffer rules.  A pixel without a usable position (NaN by S80, or 2^30 / 32 pixels away) is border_value and
 *             not valid.  One launch; d_info->status is always 0 (a bad model is PM_E_INVALID on the host).  pm_undistort: the
 *             blocking host form, one staged block.
 *   pm_undistort_map_dev   the positions alone: dw * dh pairs (qx, qy) of int32, 1/32 pixel units, row-major, stride dw;
 *             (INT32_MIN, INT32_MIN) marks a pixel without a usable position.  d_map must be 8-byte aligned.
 *   pm_remap_dev   S77 at the positions of a map: exactly the bytes of pm_undistort_dev when the map is pm_undistort_map_dev's.
 *             Every int32 pair is legal; the pair (INT32_MIN, INT32_MIN) gives border_value and is not valid.  pm_remap: the
 *             blocking host form.
 * PM_E_INVALID: null required pointers, a flag other than PM_WARP_REPLICATE, border_value outside 0 .. 255, reserved != 0, a
 * size below 1, a stride below its width, cap or n < 0, d_src and d_dst (or d_map and d_dst) ranges that overlap, a d_map that
 * is not 8-byte aligned, K or K_new with a non-finite value or fx, fy not > 0, a non-finite lens coefficient or entry of R,
 * iters outside [1, 50], tol_px not finite or not > 0.  PM_E_UNSUPPORTED: more than 100 000 000 pixels on either side,
 * cap == 0 (n == 0 in the host form), and a capturing stream (refused first, before anything is launched).
 * Timing names: "undistort_bilinear", "undistort_map", "remap_q5", "undistort_points", "distort_points". */
typedef struct pm_lens { double k1, k2, p1, p2, k3; } pm_lens;   /* OpenCV's distCoeffs order (5 coefficients) */
int pm_undistort_points_dev(pm_ctx* ctx, const pm_camera* K, const pm_lens* lens, const double* R, const pm_camera* K_new,
                            int iters, double tol_px, const float* d_pts, const int32_t* d_n, int cap, float* d_out);
int pm_undistort_points(pm_ctx* ctx, const pm_camera* K, const pm_lens* lens, const double* R, const pm_camera* K_new,
                        int iters, double tol_px, const float* pts, int n, float* out);
int pm_distort_points_dev(pm_ctx* ctx, const pm_camera* K, const pm_lens* lens, const double* R, const pm_camera* K_new,
                          const float* d_pts, const int32_t* d_n, int cap, float* d_out);
int pm_distort_points(pm_ctx* ctx, const pm_camera* K, const pm_lens* lens, const double* R, const pm_camera* K_new,
                      const float* pts, int n, float* out);
int pm_undistort_dev(pm_ctx* ctx, const uint8_t* d_src, int sw, int sh, int sstride, const pm_camera* K, const pm_lens* lens,
                     const double* R, const pm_camera* K_new, const pm_warp_params* p,
                     uint8_t* d_dst, int dw, int dh, int dstride, uint8_t* d_valid, pm_warp_info* d_info);
int pm_undistort(pm_ctx* ctx, const uint8_t* src, int sw, int sh, int sstride, const pm_camera* K, const pm_lens* lens,
                 const double* R, const pm_camera* K_new, const pm_warp_params* p,
                 uint8_t* dst, int dw, int dh, int dstride, uint8_t* valid, pm_warp_info* info);
int pm_undistort_map_dev(pm_ctx* ctx, const pm_camera* K, const pm_lens* lens, const double* R, const pm_camera* K_new,
                         int dw, int dh, int32_t* d_map);
int pm_remap_dev(pm_ctx* ctx, const uint8_t* d_src, int sw, int sh, int sstride, const int32_t* d_map, const pm_warp_params* p,
                 uint8_t* d_dst, int dw, int dh, int dstride, uint8_t* d_valid, pm_warp_info* d_info);
int pm_remap(pm_ctx* ctx, const uint8_t* src, int sw, int sh, int sstride, const int32_t* map, const pm_warp_params* p,
             uint8_t* dst, int dw, int dh, int dstride, uint8_t* valid, pm_warp_info* info);

/* ---- dense stereo: rectifying rotations, block matching, depth at points — docs/SPEC.md S84-S88 ------------------------------
 * From a calibrated pair to metric 3-D points for pm_ransac_pnp*, on one stream: pm_stereo_rectify gives the R arguments of
 * pm_undistort* (cv::stereoRectify's R1, R2), pm_undistort_dev rectifies both images, pm_stereo_bm_dev gives a disparity map
 * (cv::StereoBM: sums of absolute differences, winner, uniqueness, sub-pixel, all in integers), pm_stereo_lr_check_dev
 * removes what the right image does not confirm, pm_stereo_points_dev reads the depth at given points
 * (cv::reprojectImageTo3D at those pixels).  Every output is a function of the inputs alone (bit for bit the plain-C
 * statement tests/stereo_ref.c).
 *
 *   pm_stereo_rectify   host only, no launch, fp64 (S84).  R, t: the pose of S35, x2 ~ R x1 + t.  R1, R2: camera frame ->
 *             rectified frame of view 1 and view 2; with one K_new for both views corresponding points share a row and
 *             x_left - x_right = fx_new * baseline / Z.  *left_is_view2 != 0: view 2 is the left image.  PM_E_INVALID: null
 *             pointers, non-finite input.  PM_E_NO_MODEL (outputs zero): no baseline, or an optical axis along it.
 *             PM_E_UNSUPPORTED (outputs zero): a vertical rig, |c_y| > |c_x| for the centre c of camera 2.
 *   pm_stereo_bm_dev   8-bit rectified pair of one size -> int16 disparities in 1/16 pixel, PM_STEREO_INVALID where there is
 *             none (S85).  Disparities min_disp .. min_disp + num_disp - 1, window (2 radius + 1)^2; 1 <= radius <= 10,
 *             1 <= num_disp <= 256, -1024 <= min_disp, min_disp + num_disp - 1 <= 1024, 0 <= uniqueness <= 99 (per cent; 0
 *             rejects nothing).  Only pixels for which every disparity is testable are computed.  PM_STEREO_FROM_RIGHT: the
 *             disparity of the right image's pixels, same sign.  dstride in elements.  One launch; d_info (may be NULL):
 *             status always 0, n_valid = pixels that are not PM_STEREO_INVALID.  pm_stereo_bm: the blocking host form;
 *             lr_max_diff16 >= 0 runs the left pass, the FROM_RIGHT pass and pm_stereo_lr_check_dev in one call (and is
 *             PM_E_INVALID together with PM_STEREO_FROM_RIGHT), below 0 there is no check.
 *   pm_stereo_lr_check_dev   in place on the left map (S86): a valid value v at (x, y) survives when the right map at
 *             (x - floor((v + 8) / 16), y) exists, is valid and differs from v by at most max_diff16.  One launch; n_valid is
 *             the count afterwards.
 *   pm_stereo_points_dev   rows (x, y) in the rectified left image -> rows (X, Y, Z) f32 (S87): the map value v at the
 *             rounded pixel, Z = fx * baseline * 16 / v, with R (host, 9 doubles, or NULL) R^T (X, Y, Z): with R1 the frame of
 *             that camera before rectification.  Three quiet NaNs where a coordinate is not finite, the pixel is outside the
 *             map, v is PM_STEREO_INVALID or v <= 0: S36 makes such rows outliers of pm_ransac_pnp*.  The count protocol of
 *             pm_transform_points_dev.  One launch.  pm_stereo_points: the blocking host form.
 * PM_E_INVALID: null required pointers, a parameter out of range, unknown flag bits, reserved != 0, a size below 1, a stride
 * below the width, max_diff16, cap or n < 0, an output range (the map, the xyz rows, the info record) that overlaps an input range or another
 * output, in the host forms as in the _dev forms, a bad K_rect, baseline not finite
 * or not > 0, a non-finite R.  PM_E_UNSUPPORTED: more than 100 000 000 pixels, cap == 0 (n == 0), and a capturing stream, refused
 * before anything else.  An image too small to hold a computed pixel is not an error: every pixel is PM_STEREO_INVALID.
 * Timing names: "stereo_bm", "stereo_lr_check", "stereo_points". */
#define PM_STEREO_INVALID (-32768)
#define PM_STEREO_FROM_RIGHT 1
typedef struct pm_stereo_params {
    int32_t min_disp, num_disp, radius, uniqueness, flags, reserved[3];
} pm_stereo_params;
typedef struct pm_stereo_info {
    int32_t status;  /* always 0 */
    int32_t n_valid;
} pm_stereo_info;
int pm_stereo_rectify(const double R[9], const double t[3], double R1[9], double R2[9], double* baseline, int* left_is_view2);
int pm_stereo_bm_dev(pm_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right, int w, int h, int lstride, int rstride,
                     const pm_stereo_params* p, int16_t* d_disp, int dstride, pm_stereo_info* d_info);
int pm_stereo_bm(pm_ctx* ctx, const uint8_t* left, const uint8_t* right, int w, int h, int lstride, int rstride,
                 const pm_stereo_params* p, int lr_max_diff16, int16_t* disp, int dstride, pm_stereo_info* info);
int pm_stereo_lr_check_dev(pm_ctx* ctx, int16_t* d_left, const int16_t* d_right, int w, int h, int lstride, int rstride,
                           int max_diff16, pm_stereo_info* d_info);
int pm_stereo_points_dev(pm_ctx* ctx, const int16_t* d_disp, int w, int h, int dstride, const pm_camera* K_rect, double baseline,
                         const double* R, const float* d_pts, const int32_t* d_n, int cap, float* d_xyz);
int pm_stereo_points(pm_ctx* ctx, const int16_t* disp, int w, int h, int dstride, const pm_camera* K_rect, double baseline,
                     const double* R, const float* pts, int n, float* xyz);

/* ---- semi-global stereo matching: census cost, 4 or 8 paths — docs/SPEC.md S89-S92 ------------------------------------------
 * A second matcher for the chain above (cv::StereoSGBM, libSGM): where the block matcher lets every pixel decide alone, the
 * costs of a pixel's disparities are summed along 4 or 8 paths with a penalty p1 for a step of one disparity and p2 for a
 * larger one, so textureless and repetitive regions take the disparity of their surroundings.  All integers: the map is a
 * function of the inputs alone (bit for bit the plain-C statement tests/sgm_ref.c).  The map has pm_stereo_bm's format:
 * pm_stereo_lr_check_dev and pm_stereo_points_dev take it unchanged.
 *
 *   pm_stereo_sgm_dev   8-bit rectified pair of one size -> int16 disparities in 1/16 pixel.  The cost of (x, y, d) is the
 *             number of differing bits of two 9 x 7 census words (S89, S90), 0..62; the path sums of S91 use
 *             0 <= p1 <= p2 <= 1023 and paths = 4 (horizontal, vertical) or 8 (and diagonal); winner, uniqueness and
 *             sub-pixel step are S85's on the sum over the paths (S92).  1 <= num_disp <= 256, -1024 <= min_disp,
 *             min_disp + num_disp - 1 <= 1024, 0 <= uniqueness <= 99, flags 0 or PM_STEREO_FROM_RIGHT, reserved 0.  Computed
 *             pixels: rows 3 .. h - 4 and the columns where every disparity is testable with the window's margin of 4; every
 *             other pixel is PM_STEREO_INVALID.  The workspace (two planes of census words and the u16 sums, computed
 *             pixels x num_disp) comes from the context's arena; nothing returns to the host.  paths + 1 launches.  d_info
 *             (may be NULL): status 0, n_valid.
 *   pm_stereo_sgm   the blocking host form; lr_max_diff16 >= 0 runs the left map, the FROM_RIGHT map and
 *             pm_stereo_lr_check_dev (and is PM_E_INVALID together with PM_STEREO_FROM_RIGHT).
 * PM_E_INVALID and PM_E_UNSUPPORTED as for pm_stereo_bm*; also PM_E_UNSUPPORTED: computed pixels x num_disp above 2^30.
 * Timing names: "sgm_census", "sgm_path", "sgm_path_winner". */
typedef struct pm_sgm_params {
    int32_t min_disp, num_disp, p1, p2, paths, uniqueness, flags, reserved;
} pm_sgm_params;
int pm_stereo_sgm_dev(pm_ctx* ctx, const uint8_t* d_left, const uint8_t* d_right, int w, int h, int lstride, int rstride,
                      const pm_sgm_params* p, int16_t* d_disp, int dstride, pm_stereo_info* d_info);
int pm_stereo_sgm(pm_ctx* ctx, const uint8_t* left, const uint8_t* right, int w, int h, int lstride, int rstride,
                  const pm_sgm_params* p, int lr_max_diff16, int16_t* disp, int dstride, pm_stereo_info* info);

/* ---- visual vocabularies: k-means / k-majority training and bag-of-words encoding — docs/SPEC.md S102-S106 ---------------
 * Which earlier image does this one resemble?  Cluster a training set of descriptor rows into K words (cv::kmeans,
 * cv::BOWKMeansTrainer::cluster; k-majority on binary rows as in DBoW2 / ORB-SLAM), then describe an image by the histogram
 * of its rows' nearest words (cv::BOWImgDescriptorExtractor::compute).  The vocabulary is flat: the quantiser is the
 * brute-force matcher with the K words as its train set, so a label is the trainIdx of pm_bf_knn_l2_u8_dev /
 * pm_bf_knn_hamming_u8_dev with k = 1 (ties: the lowest word), and d_dist is that record's distance, bit for bit.
 * Everything is integer arithmetic: every output is a function of the inputs alone (tests/vocab_ref.c restates it).
 *   kind, bytes   PM_VOCAB_L2_U8: rows of `bytes` u8 values (the 128-byte rows of pm_detect_describe*), squared L2;
 *                 PM_VOCAB_BITS: rows of bytes * 8 bits (the 32-byte rows of pm_detect_describe_bits*), Hamming.
 *   pm_vocab      owns its device memory (words, u32 accumulators, the matcher's records and labels for max_rows rows);
 *                 pm_vocab_create is the only allocation of the path.  Bound to the context's device.
 *   pm_vocab_set / _set_dev / _get   the K x bytes words, row-major; _set and _get synchronise, _set_dev does not.
 *   pm_vocab_init_stride_dev         word i <- row floor(i * n / K) (rows repeat when n < K).  Timing name "vocab_init".
 *   pm_vocab_train[_dev]             `iters` iterations of { assign every row, then per word the rounded mean of its rows'
 *                 bytes (halves up) / the majority of their bits (an even split gives 0); a word without rows keeps its
 *                 bytes }.  d_labels: the n labels of the LAST iteration (those of the returned words iff its n_moved == 0).
 *                 d_info: one pm_vocab_iter per iteration: n_changed = rows whose label differs from the previous iteration
 *                 (n in iteration 0), n_empty = words without rows, n_moved = words whose bytes changed, cost = the exact sum
 *                 of the integer distances (squared L2 / bit count) of the rows to their words before the update.  Both may
 *                 be NULL.  iters == 0 runs nothing and writes nothing.  Timing names "vocab_update", "vocab_finish" and
 *                 the matcher's own.
 *   pm_vocab_assign[_dev]            m = n when d_n is NULL, else *d_n clamped to [0, n] (so the call chains after
 *                 pm_detect_describe[_bits]_dev with n = max_kp, and an overflow count of -1 counts nothing).  d_words[i] /
 *                 d_dist[i] = label / distance for i < m, -1 / NaN for m <= i < n; d_hist[w] = rows i < m with label w,
 *                 exactly K words, overwritten.  Each may be NULL.  Timing name "vocab_hist".
 * The _dev forms enqueue on the context's stream and do not synchronise; row pointers are 4-byte aligned.  The host forms
 * stage their rows and outputs in a device block of their own.
 * PM_E_INVALID: null required pointers, an unknown kind, bytes not a multiple of 4 in [4, 256] (bits: [4, 64]), K outside
 * [1, 262144], max_rows < 1, n outside [1, max_rows], iters outside [0, 1000], a vocabulary of another device.
 * PM_E_UNSUPPORTED: max_rows above 2^24 (a u32 sum could overflow), and a capturing stream, refused before anything is
 * allocated or enqueued (the matcher inside refuses capture). */
#define PM_VOCAB_L2_U8 0
#define PM_VOCAB_BITS  1
typedef struct pm_vocab pm_vocab;   /* opaque */
typedef struct pm_vocab_iter { int32_t n_changed, n_empty, n_moved, reserved; uint64_t cost; } pm_vocab_iter;   /* 24 bytes */
int pm_vocab_create(pm_ctx* ctx, int kind, int bytes, int K, int max_rows, pm_vocab** out);
int pm_vocab_destroy(pm_vocab* v);
int pm_vocab_set(pm_ctx* ctx, pm_vocab* v, const uint8_t* words);
int pm_vocab_set_dev(pm_ctx* ctx, pm_vocab* v, const uint8_t* d_words);
int pm_vocab_get(pm_ctx* ctx, const pm_vocab* v, uint8_t* words);
int pm_vocab_init_stride_dev(pm_ctx* ctx, pm_vocab* v, const uint8_t* d_rows, int n);
int pm_vocab_train_dev(pm_ctx* ctx, pm_vocab* v, const uint8_t* d_rows, int n, int iters, int32_t* d_labels, pm_vocab_iter* d_info);
int pm_vocab_train(pm_ctx* ctx, pm_vocab* v, const uint8_t* rows, int n, int iters, int32_t* labels, pm_vocab_iter* info);
int pm_vocab_assign_dev(pm_ctx* ctx, const pm_vocab* v, const uint8_t* d_rows, int n, const int32_t* d_n, int32_t* d_words,
                        float* d_dist, uint32_t* d_hist);
int pm_vocab_assign(pm_ctx* ctx, const pm_vocab* v, const uint8_t* rows, int n, int32_t* words, float* dist, uint32_t* hist);

/* ---- image database: tf-idf bag-of-words scoring and top-N retrieval — docs/SPEC.md S107-S112 ----------------------------
 * The question the histogram of pm_vocab_assign exists for: which earlier image does this one resemble?  An append-only
 * forward index on the device (per image its (word, tf) entries in ascending word order), per-word weights (1, given, or
 * idf), and a query that scores EVERY image with DBoW2's L1 score of the two L1-normalised tf-idf vectors and selects the
 * best `top` (DBoW2::Database::add / query with L1 scoring; the "score and rank" half of a retrieval system built on
 * cv::BOWImgDescriptorExtractor).  Everything up to the one fp64 division per image is integer arithmetic: every output is
 * a function of the inputs alone (tests/bowdb_ref.c restates it).  There is no inverted file.
 *   pm_bowdb      owns one device block (offsets and norms of max_images images, max_entries entries, df / weight / the
 *                 dense query table of K words, counts, selection scratch); pm_bowdb_create is the only allocation of the
 *                 _dev path.  Bound to the context's device.  Weights start at 1.
 *   pm_bowdb_clear_dev   removes all images, entries and df; keeps the weights (train the idf on a corpus, clear, use).
 *   pm_bowdb_add[_dev]   d_hist: the K u32 counts that pm_vocab_assign_dev writes; T = their sum, nnz = the non-zero ones.
 *                 Accepted iff 1 <= T <= 65535, images < max_images and entries + nnz <= max_entries, decided on the device:
 *                 the entries (w, hist[w]) are appended in ascending w, df[w] += 1 for each, the norm is
 *                 Nd = sum tf * weight[w] under the current weights, and *d_id = the previous image count.  Refused: nothing
 *                 changes and *d_id = -1 (empty or T > 65535) or -2 (full).  d_id may be NULL.  Timing name "bow_add".
 *   pm_bowdb_set_weights / _get_weights   K u32 in [0, 8191]; host calls, both synchronise.
 *   pm_bowdb_idf_dev     weight[w] = floor(256 * log2(N / max(df[w], 1))) for the current image count N, by S109's integer
 *                 algorithm (no transcendental function); N == 0 changes nothing.  After either setter the norm of every
 *                 image is recomputed on the device.  Timing names "bow_idf" and "bow_norms".
 *   pm_bowdb_query[_dev] q_w = hist[w] * weight[w], Nq = sum q_w; for an image d_w = tf * weight[w], Nd its norm;
 *                 S = sum over the image's entries of min(q_w * Nd, d_w * Nq) in u64, score = (double)S / (double)(Nq * Nd),
 *                 0 when Nq or Nd is 0.  A query with T = 0 or T > 65535 scores 0 everywhere.  Candidates: images with
 *                 S > 0 and an id outside [excl_lo, excl_hi) (an empty window when excl_hi <= excl_lo), ordered by score
 *                 descending, then id ascending; the selection is exact and does not depend on arrival order.
 *                 d_ids / d_scores: `top` int32 / double, the first min(top, candidates) of them, then -1 / quiet NaN;
 *                 d_count: that number; d_all: the score of every image 0 .. N-1, excluded ones included.  Each may be
 *                 NULL.  The host form's `all` has room for the image count (pm_bowdb_get).  Timing names "bow_query_vec",
 *                 "bow_score", "bow_top".
 *   pm_bowdb_get  synchronises and copies out the counts and, where the pointer is not NULL, n_images + 1 offsets,
 *                 n_entries words and tfs, n_images norms, K df and K weights (call it once for the counts).
 * The _dev forms enqueue on the context's stream and do not synchronise: add and query chain behind pm_vocab_assign_dev
 * with no host round trip (an overflow count of -1 there gives an all-zero histogram: the image is refused as empty).
 * PM_E_INVALID: null required pointers (ctx, db, histogram, weights), K outside [1, 262144], max_images outside [1, 2^22],
 * max_entries outside [1, 2^28], top outside [1, 256], a weight above 8191, a database of another device.
 * PM_E_UNSUPPORTED: a capturing stream, refused by every call before anything is allocated or enqueued. */
typedef struct pm_bowdb pm_bowdb;   /* opaque */
int pm_bowdb_create(pm_ctx* ctx, int K, int max_images, int max_entries, pm_bowdb** out);
int pm_bowdb_destroy(pm_bowdb* db);
int pm_bowdb_clear_dev(pm_ctx* ctx, pm_bowdb* db);
int pm_bowdb_add_dev(pm_ctx* ctx, pm_bowdb* db, const uint32_t* d_hist, int32_t* d_id);
int pm_bowdb_add(pm_ctx* ctx, pm_bowdb* db, const uint32_t* hist, int32_t* id);
int pm_bowdb_set_weights(pm_ctx* ctx, pm_bowdb* db, const uint32_t* weights);
int pm_bowdb_get_weights(pm_ctx* ctx, const pm_bowdb* db, uint32_t* weights);
int pm_bowdb_idf_dev(pm_ctx* ctx, pm_bowdb* db);
int pm_bowdb_query_dev(pm_ctx* ctx, pm_bowdb* db, const uint32_t* d_hist, int top, int excl_lo, int excl_hi, int32_t* d_ids,
                       double* d_scores, int32_t* d_count, double* d_all);
int pm_bowdb_query(pm_ctx* ctx, pm_bowdb* db, const uint32_t* hist, int top, int excl_lo, int excl_hi, int32_t* ids, double* scores,
                   int32_t* count, double* all);
int pm_bowdb_get(pm_ctx* ctx, const pm_bowdb* db, int32_t* n_images, int32_t* n_entries, uint32_t* offsets, uint32_t* words,
                 uint16_t* tfs, uint32_t* norms, uint32_t* df, uint32_t* weights);

/* ---- residual report (main.cpp:103-123) -----------------------------------------------------
 * r[i] = [xa ya 1] * F * [xb yb 1]^T in fp64.  transposed != 0 reproduces the reference
 * literally ((xa,ya) = image-1 point, (xb,yb) = image-2 point: x1^T F x2, main.cpp:110-117);
 * transposed == 0 evaluates x2^T F x1.  mean_abs = sum|r| / n (main.cpp:120,123).
 * pm_f_scale_f33: rescales F so F[8] == 1 when |F[8]| > DBL_EPSILON (OpenCV's output scale,
 * which the magnitudes printed at main.cpp:119 depend on). */
int pm_epipolar_residuals(const float* xy1, const float* xy2, int n, const double F[9],
                          int transposed, double* r, double* mean_abs);
int pm_f_scale_f33(double F[9]);

/* ---- epipolar lines (main.cpp:127-142) ----------------------------------------
 * cv::computeCorrespondEpilines(pts, which_image, F, lines): l = F*x (which_image==1) or
 * F^T*x (==2), scaled so a^2+b^2 = 1; lines: n x 3 floats.  pm_epiline_endpoints: the two
 * cv::Point arguments of main.cpp:138-140 for an image `cols` wide (float->int truncation). */
int pm_epilines(const float* xy, int n, int which_image, const double F[9], float* lines);
int pm_epiline_endpoints(const float* lines, int n, int cols, int32_t* xyxy);

#ifdef __cplusplus
}
#endif
#endif /* PM_H_ */
