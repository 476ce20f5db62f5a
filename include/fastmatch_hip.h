/*
 * fastmatch_hip.h -- C-ABI of libfastmatch_hip.so: the MI355X (gfx950) drop-in for the
 * arithmetic behind Fast-Match's descriptor-matching hot path.
 *
 * The reference (arnfred/Fast-Match) has no native FFI of its own: its Cython modules
 * call OpenCV's cv2.BFMatcher from Python.  Each entry point below therefore names the
 * reference call site whose arithmetic it replaces (file:line in the reference tree);
 * INTEGRATION.md shows the ctypes binding a maintainer would add at those sites.
 *
 * Conventions: plain C, no exceptions.  Every function returns 0 on success and a
 * negative FM_E* code on failure; fm_last_error() returns the message of the last
 * failure on that context (or the last context-less failure when ctx == NULL).
 * The caller owns every host buffer; the library owns device memory behind the opaque
 * handles.  One fm_ctx per device; calls on one ctx are serialised on its HIP stream
 * (not re-entrant per ctx; distinct ctxs are independent).  All calls are synchronous:
 * host outputs are valid on return.  There is no CPU fallback: without a usable
 * gfx950 device fm_ctx_create fails.
 *
 * Sizes.  Row numbers are 32-bit everywhere (idx outputs are int32, the kernels' keys carry a row in 32 bits): a bank holds
 * at most 2^31 - 257 rows and a train collection at most that many rows in all its images together, padding to 128-row
 * stages included; the creators and the adds refuse more with FM_EUNSUPPORTED.  BYTE offsets into a bank's arrays are
 * 64-bit in every kernel, so a bank or a collection may be as large as device memory allows: rows beyond the 2^31- and
 * 2^32-byte marks of every plane (2^21 / 2^22 rows of a wide bank, 2^22 / 2^23 of a float32-route bank, 2^24 / 2^25 of an
 * integer-route bank, 2^25 / 2^26 binary rows of 64 bytes) are tested bit for bit (tests/test_big_offset_gpu.py; DESIGN.md,
 * "Index widths", lists every access).  Two narrower limits come from kernels that spend one work-item per element and
 * end in FM_EDEVICE (a refused launch), never in a wrong result: a float32-route bank (FM_BANK_F32) is prepared for fewer
 * than 2^25 rows, and a cross-check elects among fewer than 2^30 train rows.  A wide pair (FM_BANK_F32W) whose OUTPUT side has
 * 2^20 rows or more takes the exact kernel whatever "f32_filter" says and counts no filter launch: the first tiles alone
 * would fill the filter's record list (K14 below).
 */
#ifndef FASTMATCH_HIP_H
#define FASTMATCH_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FM_OK            0
#define FM_EINVAL       -1   /* bad argument (null handle, dim mismatch, k unsupported ...)  */
#define FM_EDEVICE      -2   /* HIP runtime error; message carries hipGetErrorString          */
#define FM_ENOMEM       -3   /* device or host allocation failed                              */
#define FM_EUNSUPPORTED -4   /* valid request this build cannot serve (e.g. dim > 128)        */

/* Bank kinds (fm_bank_info) */
#define FM_NO_STREAM ((void*)(intptr_t)-1)   /* "no consumer stream" (NULL is the null stream) */
#define FM_BANK_I8   1       /* uint8 / integer-valued float32 rows: exact int8-MFMA route    */
#define FM_BANK_F32  2       /* general float32 rows: fp32 fma-chain route                    */
#define FM_BANK_BIN  3       /* binary descriptors (fm_bank_create_bin): Hamming distance, K11 */
#define FM_BANK_F32W 4       /* float32 rows of 129 .. 256 values ("wide float banks", K14)    */
#define FM_BANK_BIN2 5       /* binary descriptors of 2-bit cells (fm_bank_create_bin2): NORM_HAMMING2, K11b */

typedef struct fm_ctx  fm_ctx;
typedef struct fm_bank fm_bank;

/* ABI revision of this header.  It changes whenever an existing signature or struct layout does (revision 3, r03:
 * fm_expand_fetch_many gained `slot`, fm_expand_desc gained `metric`; revision 4, r04: additions only; revision 5, r04:
 * fm_expand_desc gained the trailing `lazy`; revision 7, r05: additions -- fm_self_dist_plan, fm_bank_create_f32_cap,
 * fm_bank_append_f32, fm_expand_set_log / _log_counts / _fetch_log -- and fm_expand_run_lazy refuses to resume a run
 * that did not park; revision 8, r06: additions -- fm_knn, the option "f32_bound_every" -- and rounds[i][5] of the
 * per-round log may be -2; revision 9: additions -- fm_radius_match, the option "radius_ws_bytes"; revision 10: additions --
 * FM_BANK_BIN, fm_bank_create_bin; revision 11: additions -- fm_collection_*; revision 12: additions -- FM_DT_*,
 * fm_bank_create_dev, fm_knn_dev, fm_xcheck1_dev, fm_knn2_ratio_dev; still revision 12, additions only --
 * fm_collection_match_accepted_each, fm_collection_match_accepted_each_dev, the option "coll_ws_bytes"; still revision 12,
 * additions only -- fm_collection_add_dev, fm_collection_knn_dev, fm_collection_knn2_ratio_dev; still revision 12, additions
 * only -- fm_collection_radius_match, fm_radius_match_dev, fm_collection_radius_match_dev; still revision 12, additions
 * only -- fm_collection_xcheck1_each, fm_collection_xcheck1_each_dev; still revision 12, additions only -- fm_mutual_ratio,
 * fm_mutual_ratio_dev, fm_collection_mutual_ratio_each, fm_collection_mutual_ratio_each_dev; still revision 12, additions
 * only -- fm_mask_create, fm_mask_create_coll, fm_mask_set_u8, fm_mask_set_dev, fm_mask_set_all, fm_mask_destroy,
 * fm_mask_info, fm_knn_masked, fm_knn_masked_dev, fm_collection_knn_masked, fm_collection_knn_masked_dev, the option
 * "masked_mfma", "mask_pack_words"; still revision 12, additions only -- FM_BANK_F32W: the float creators take
 * 129 <= dim <= 256; still revision 12, additions only -- fm_collection_pairs_mutual_ratio,
 * fm_collection_pairs_mutual_ratio_dev; still revision 12, additions only -- fm_collection_add_wide,
 * fm_collection_add_wide_dev; still revision 12, additions only -- fm_hamming_radius_match, fm_hamming_radius_match_dev,
 * fm_collection_hamming_radius_match, fm_collection_hamming_radius_match_dev; still revision 12, additions only --
 * fm_collection_wide_knn2_each, fm_collection_wide_mutual_ratio_each, fm_collection_wide_mutual_ratio_each_dev; still
 * revision 12, additions only -- fm_hamming_self_dist, fm_hamming_self_dist_batch, fm_hamming_set_selfdist,
 * fm_hamming_match_ratio, fm_hamming_match_accepted, fm_hamming_match_accepted_dev,
 * fm_collection_hamming_match_accepted_each, fm_collection_hamming_match_accepted_each_dev; still revision 12, additions
 * only -- fm_wide_self_dist, fm_wide_self_dist_batch, fm_wide_set_selfdist, fm_wide_match_ratio, fm_wide_match_accepted,
 * fm_wide_match_accepted_dev, fm_collection_wide_match_accepted_each, fm_collection_wide_match_accepted_each_dev; still
 * revision 12, additions only -- fm_wide_radius_match, fm_wide_radius_match_dev, fm_collection_wide_radius_match,
 * fm_collection_wide_radius_match_dev; still revision 12, additions only -- fm_wide_knn_masked, fm_wide_knn_masked_dev; still
 * revision 12, additions only -- fm_collection_wide_knn, fm_collection_wide_knn_dev, fm_collection_wide_knn2_ratio,
 * fm_collection_wide_knn2_ratio_dev, fm_collection_wide_votes; still revision 12, additions only -- fm_radius_match_masked,
 * fm_radius_match_masked_dev, fm_collection_radius_match_masked, fm_collection_radius_match_masked_dev; still revision 12,
 * additions only -- FM_BANK_BIN2, FM_DT_BIN2, fm_bank_create_bin2).  A binding
 * compares fm_abi_version() with the FM_ABI_VERSION it was written against before its first call.              */
#define FM_ABI_VERSION 12
int  fm_abi_version(void);

typedef struct fm_stats {
    double   kernel_ms;      /* HIP-event time of the distance kernels since fm_reset_stats   */
    double   total_ms;       /* HIP-event time of whole calls (all kernels + copies)          */
    int64_t  kernel_launches;/* number of distance-kernel launches in kernel_ms               */
    int64_t  pairs;          /* descriptor pairs evaluated by those launches                  */
    int64_t  calls;          /* API calls accounted in total_ms                               */
} fm_stats;

/* fm_stats plus what later revisions add; struct_bytes = sizeof(fm_stats_ex) of the library that filled it.
 * bytes_moved = ALGORITHMIC bytes of the distance-kernel launches in kernel_ms: every bank row of a launch read
 * once (128 B per integer-route row, 512 B per float32 row, the packed width of a binary row) -- the numerator of an HBM-roofline fraction; the
 * bytes a launch really fetched come from the PMC counters (profiles/).                                       */
typedef struct fm_stats_ex {
    int64_t  struct_bytes;
    double   kernel_ms, total_ms;
    int64_t  kernel_launches, pairs, calls;
    int64_t  bytes_moved;
} fm_stats_ex;

/* ---- context ---------------------------------------------------------------------- */
int  fm_ctx_create(int device_id, fm_ctx** ctx);
int  fm_ctx_destroy(fm_ctx* ctx);
/* Per-context options: batch shape and launch tuning by name.  RESULTS NEVER DEPEND ON THEM (the parity
 * tests run the kernels under several settings); they replace the process-wide FM_* environment
 * variables, which now only seed a new context's defaults.  The reference has no counterpart: cv2 is
 * configured per matcher object (fastmatch.pyx:122, 161 build one per call).
 *   "batch_group"  1..16  fm_match_accepted_batch: most image pairs per distance-kernel launch (8)
 *   "batch_tail"   0..16  ... pairs in the short launch a run of pairs ends with (2; 0 = none: for callers
 *                         that enqueue the next batch before waiting for this one, fm_mark / fm_wait)
 *   "nsplit" "nb" "nw"    K1 grid shape: splits of the reduction range, 16-row blocks per wave (4 | 6 | 8),
 *                         waves per workgroup (4 | 8 | 16); 0 = built-in rule
 *   "nbuf"         0|2|3  K1 / K2 LDS stage buffers (0 = 3; top-2 shapes other than 4 blocks per wave: 2)
 *   "prio" "glds" "coop"  0|1  s_setprio around the MFMA burst / LDS-DMA staging / cross-workgroup bounds
 *   "f32_filter"   0..2   float32 route: 0 = all-pairs kernel only, 1 = fp16 filter for large calls, 2 = always
 *   "f32_nw" "f32_nsplit" "f32_fused" "f32_lpc"   K8 launch shape (0 / -1 = rule)
 *   "f32_bound_every"    K8: re-read the shared bounds every n-th stage once a sweep is 8 stages old (1 .. 64, a power of two; 4)
 *   "async_time_every"    every n-th async call carries kernel-timing events (4; 0 = none)
 *   "k1_order"     0..2   K1: how workgroups map to (output chunk, split of the reduction range): 0 split major,
 *                         1 the workgroups of one XCD own a set of output chunks for all splits, 2 they own a
 *                         contiguous share of the split-major order (the guide's XCD remap); see rowreduce.hip
 *   "bound_every"  1..1024  K1 / K2: workgroups re-read the shared K-th-best bounds at every stage of a sweep's first
 *                         eight and then at every n-th (a power of two; 16).  A stale bound is merely weaker
 *   "self_tri"     0..2   fm_self_dist / fm_self_dist_batch: 1 = the triangular sweep (every distance once) -- float32-route banks (r06)
 *                         from 65536 padded rows on; integer banks from 32768 padded rows
 *                         on and for every run of two or more integer banks in a batch call, whatever their sizes (1),
 *                         0 = always the masked full sweep, 2 = always the triangular one
 *   "tri_stages"   0..    ... 128-row stages per workgroup of its launch B (0 = chosen per bank size: fm_self_dist_plan)
 *   "refill_grid"  1..    fm_bank_refill_u8_async: workgroups of its preparation kernel (128: few, long-lived ones beside
 *                         the distance kernels)
 *   "expand_big"   0|1    K7: re-run pairs whose round exceeds 2048 query rows in the 4096-row variant (1)
 *   "expand_huge"  0|1    K7: ... and those that still do in the variant that takes a radius subset of any size in chunks (1)
 *   "expand_delegate" 0.. K7: a chunked round of at least this many descriptor pairs parks its run; the round's cross-check
 *                         is run by the dense kernels on the whole GPU and the run resumed (1 500 000; 0 = never)
 *   "delegated_rounds" 0  a COUNTER, not a setting: rounds whose cross-check the dense kernels ran (fm_expand_run,
 *                         fm_expand_run_lazy) since it was last set to 0 -- the only value it accepts
 *   "expand_grow"  0..4   K7: how often a run that fills its pending stack / result list / hash table is
 *                         repeated in a run state four times as large (2; r05: counted per array)
 *   "expand_prof"  0|1    K7: per-phase timers of the first pair of a launch on stderr
 *   "fp6_filter"   0|1    accepted-match calls (fm_match_accepted*, integer-route banks of dim 128 with self distances): 1 = the
 *                         sweep runs as an FP6 matrix-core filter below the ratio test's distance cut, with exact int8
 *                         rescoring of what it keeps and K1 as the fallback (1); 0 = K1 always.  Results never differ.
 *   "fp6_cap"      1..2^24  ... records per image pair the filter may keep (2^20, 8 bytes each); a pair that needs more is
 *                         redone by K1 on the device, without a host wait
 *   "fp6_nsplit"   0..2^20  ... slices of the query bank the filter's workgroups sweep (0: chosen per launch from the sizes of
 *                         all its pairs and the device's CU count; a forced "nsplit" governs the filter too unless this is set)
 *   "fp6_records", "fp6_fallbacks"  COUNTERS, get only (waits for the context's stream): records appended and pairs redone
 *                         by K1 in the last filter launch, summed over its pairs
 *   "masked_mfma"  0|1    fm_knn_masked and its siblings on the integer route with k <= 2: 1 = the masked matrix-core sweep
 *                         (1), 0 = the masked vector-ALU lists that serve every other k and route.  Results never differ.
 *   "mask_pack_words" 64..2^26-4  fm_mask_set_u8 / _set_dev / _set_all: mask words one kernel launch covers (2^26 - 4: the
 *                         packing kernel spends 64 work-items per word and a launch holds fewer than 2^32); larger masks take
 *                         several launches of whole query rows, at least one row each
 *   "radius_ws_bytes" 65536..2^31-1  fm_radius_match: device bytes for the candidates of one chunk of query rows (2^30;
 *                         24 bytes per candidate, 28 in the collection forms); a row whose own list needs more runs in a
 *                         chunk of its own
 *   "coll_ws_bytes" 0..2^31-1  fm_collection_match_accepted_each, fm_collection_xcheck1_each: device bytes for the
 *                         per-(image, query row) arrays of one chunk of consecutive images (25 bytes per entry in the
 *                         accepted-match test, 17 in the cross-check, which keeps no ratio; at least one image per
 *                         chunk); 0 = one chunk up to 64 MiB, beyond that a quarter of the free device memory (0).
 *                         fm_collection_mutual_ratio_each: device bytes for the gathered train rows of one chunk of
 *                         consecutive candidates -- 132 bytes per candidate on the integer route, 776 on the float32 route,
 *                         80 per 16 bytes of row width (rounded up) for binary rows; whole 128-row stages, at least one per
 *                         chunk; 0 = 2^30.
 *                         fm_collection_pairs_mutual_ratio: device bytes for the sweep partials, 2-NN lists and per-row arrays
 *                         of one chunk of consecutive pairs (one table-driven launch per chunk on the integer route; at
 *                         least one pair per chunk); 0 = 2^30.  A pair (a, b) of a wide collection counts 20 bytes per row of
 *                         pad128(rows(a)) + pad128(rows(b)) (partials and bounds), 3088 per row of rows(a) + rows(b) (256 records
 *                         of 12 bytes, the 2-NN lists) and 17 per row of a: 12.5 MB for two images of 2000 rows
 * Unknown names and out-of-range values return FM_EINVAL.                                          */
int  fm_ctx_set_option(fm_ctx* ctx, const char* name, int64_t value);
int  fm_ctx_get_option(fm_ctx* ctx, const char* name, int64_t* value);
const char* fm_last_error(const fm_ctx* ctx);
int  fm_sync(fm_ctx* ctx);
int  fm_get_stats(fm_ctx* ctx, fm_stats* out);
/* Writes min(out_bytes, sizeof(fm_stats_ex)) bytes: a caller built against an older, shorter struct stays valid. */
int  fm_get_stats_ex(fm_ctx* ctx, fm_stats_ex* out, int64_t out_bytes);
int  fm_reset_stats(fm_ctx* ctx);
/* Name of the device the context runs on (e.g. "gfx950:..."), written NUL-terminated.  */
int  fm_device_name(fm_ctx* ctx, char* buf, int buflen);
/* Float32 route diagnostics: how many row-reduces went through the fp16 MFMA filter
 * (filter_f16.hip) and how many of those had to be redone by the all-pairs float32 kernel
 * because a candidate list could have been incomplete (results are identical either way). */
int  fm_f32_filter_stats(fm_ctx* ctx, int64_t* launches, int64_t* fallbacks);

/* Page-locked host memory for output buffers (optional): results copied into such a buffer
 * move by direct DMA instead of through the runtime's pageable staging path.             */
int  fm_host_alloc(fm_ctx* ctx, int64_t bytes, void** ptr);
int  fm_host_free(fm_ctx* ctx, void* ptr);

/* ---- descriptor banks --------------------------------------------------------------
 * A bank is a device-resident [n, dim] descriptor matrix plus what the kernels need
 * (bytes XOR 0x80 as int8, row norms).  It replaces the ndarray arguments the reference
 * hands to cv2 at every matcher call: Metric_Cache.original/thumb["descriptors"]
 * (cache.pyx:255-260, 278-284) and the Grid_Cache cell descriptors (cache.pyx:134-137).
 * dim must be <= 128 (SIFT = 128); shorter rows are zero-padded, which leaves every L2
 * distance unchanged.  n may be 0.
 *   fm_bank_create_u8  : rows are uint8 (CV_8U descriptors).
 *   fm_bank_create_f32 : rows are float32 (what cv2 SIFT emits).  If every value is an
 *       integer in [0,255] the bank takes the exact int8 route (kind FM_BANK_I8),
 *       otherwise it stays float32 (kind FM_BANK_F32).
 * A query/train pair must have the same kind and dim (cv2 raises on dtype mismatch).    */
int  fm_bank_create_u8 (fm_ctx* ctx, const uint8_t* rows, int64_t n, int dim, fm_bank** bank);
int  fm_bank_create_f32(fm_ctx* ctx, const float*   rows, int64_t n, int dim, fm_bank** bank);
/* Same, but the bank takes the float32 route even if every value happens to be an integer in
 * 0..255: for banks that must pair with a non-integer bank (e.g. one Grid_Cache cell of a
 * RootSIFT image whose values are all 0 or 1).  Distances are the same numbers either way.  */
int  fm_bank_create_f32_route(fm_ctx* ctx, const float* rows, int64_t n, int dim, fm_bank** bank);
/* ---- K11: binary descriptors, NORM_HAMMING -------------------------------------------------------------------------------
 * cv2.BFMatcher(cv2.NORM_HAMMING[, crossCheck]) on ORB / BRIEF / BRISK / FREAK / AKAZE rows: the reference matches SIFT only but
 * names the detector as an argument (get_features(data, feature_type), matchutil.py:31).  A binary bank holds n packed rows of
 * `bytes` bytes, 1 <= bytes <= 64 (0 or negative: FM_EINVAL; > 64: FM_EUNSUPPORTED); n may be 0; fm_bank_info reports
 * dim = bytes, kind = FM_BANK_BIN.  Contract (cv::batchDistance, dtype CV_32S): h(q, t) = popcount(q XOR t), dist = (float)h, exact.
 *   fm_knn2, fm_knn (1 <= k <= 8; k > 8 FM_EUNSUPPORTED): lists ascend by (h, train index) -- the earlier train row wins a tie;
 *     idx -1 / dist +inf where t has fewer than k rows.
 *   fm_xcheck1: every train row elects its nearest query row (strict <: the lowest query index on ties); each query keeps the
 *     closest electing train row (strict <, ascending train order); a query nobody elects gets -1 / +inf.
 *   fm_knn2_ratio: the classic ratio match as for L2, d0 / d1 < tau in float64, d1 == 0 rejected (frequent: duplicate rows).
 * k = 1, 2 and crossCheck run on the matrix cores: every bit an FP4 value +1 / -1 (padding 0), the dot product of two rows is
 * W - 2 h, exact in the f32 accumulator of v_mfma_scale_f32_16x16x128_f8f6f4 (hamming.hip); k = 3 .. 8: vector ALUs (XOR +
 * popcount).
 *   fm_hamming_radius_match(_dev), fm_collection_hamming_radius_match(_dev): radiusMatch on binary banks -- "Hamming radiusMatch"
 *     below, behind fm_radius_match.
 *   fm_hamming_self_dist(_batch), fm_hamming_set_selfdist, fm_hamming_match_ratio, fm_hamming_match_accepted(_dev),
 *     fm_collection_hamming_match_accepted_each(_dev): Fast-Match's self-distance test on binary banks -- "Hamming Fast-Match"
 *     below, behind fm_hamming_radius_match.
 * Every other entry point that takes a bank refuses a binary one with FM_EUNSUPPORTED before any kernel reads it:
 * fm_radius_match(_dev) (the L2-named radius calls keep refusing: fm_hamming_radius_match is the call), fm_self_dist(_batch),
 * fm_bank_set_selfdist, fm_match_ratio, fm_match_accepted* (the L2-named Fast-Match calls keep refusing too: the fm_hamming_*
 * calls of "Hamming Fast-Match" are the ones that serve binary banks), fm_xcheck1_keys*,
 * fm_xcheck1_batched, fm_bank_refill_u8_async, fm_bank_append_*, fm_expand_create.  A binary bank paired with a non-binary one
 * is FM_EINVAL, even when one of them is empty.  Not built: NORM_HAMMING2, masked Hamming radius queries, the expansion loop
 * (fm_expand_*) and the async / batch / sharded-key forms of the accepted-match test on binary banks, k > 8.  (Masked Hamming
 * radius queries have since come: "Masked radiusMatch" below.)  (NORM_HAMMING2 has since come, for bank pairs:
 * "K11b: NORM_HAMMING2" below.)                                                                                                */
int  fm_bank_create_bin(fm_ctx* ctx, const uint8_t* rows /*[n][bytes]*/, int64_t n, int bytes, fm_bank** bank);
/* ---- K11b: NORM_HAMMING2 ---------------------------------------------------------------------------------------------------
 * cv2.BFMatcher(cv2.NORM_HAMMING2[, crossCheck]): the norm OpenCV prescribes for ORB with WTA_K = 3 or 4, where every
 * descriptor element is a 2-bit value.  fm_bank_create_bin2 follows fm_bank_create_bin's rules word for word (1 <= bytes <= 64;
 * 0 or negative: FM_EINVAL; > 64: FM_EUNSUPPORTED; n may be 0; the errors and their order are the same); fm_bank_info reports
 * dim = bytes, kind = FM_BANK_BIN2.  fm_bank_create_dev with FM_DT_BIN2 makes the same bank from device rows read in place at
 * their pitch.  Contract (cv::normHamming with cellSize = 2): h2(q, t) = the number of 2-bit cells of q XOR t that are non-zero,
 * a cell being bits 2c, 2c + 1 of a byte; dist = (float)h2, exact; P = 4 * bytes cells per row.  Every ordering rule is K11's
 * with h2 for h: lists ascend by (h2, train index), strict compares, the lowest index wins a tie.
 * Served, for a pair of FM_BANK_BIN2 banks of one width, under K11's contracts: fm_knn2, fm_knn (1 <= k <= 8), fm_xcheck1,
 * fm_knn2_ratio, fm_mutual_ratio, fm_knn_dev, fm_xcheck1_dev, fm_knn2_ratio_dev, fm_mutual_ratio_dev and
 * fm_hamming_radius_match(_dev) (the radius against h2; r > P admits every real row).
 * k = 1, 2, crossCheck and the radius sweeps run on the matrix cores (hamming2.hip): a cell (a, b) becomes three FP4 values
 * (s_a, s_b, s_a s_b), s = +1 for a 1 bit and -1 for a 0 bit -- the four vertices of a tetrahedron -- so two equal cells add
 * +3 to the dot product of two rows and two different ones -1, whether they differ in one bit or both: dot = 3 P - 4 h2, every
 * partial sum an integer of magnitude <= 768, exact in the f32 accumulator of v_mfma_scale_f32_16x16x128_f8f6f4 in any order.
 * A row is 12 * bytes FP4 values, ceil(12 * bytes / 128) K steps (a 32-byte ORB row: three).  k = 3 .. 8: vector ALUs, the
 * population count of (x | x >> 1) & 0x55555555 over the packed rows.
 * Refused with FM_EUNSUPPORTED and a message that names NORM_HAMMING2, before any kernel reads the bank: every other entry
 * point that takes a bank, a mask or a collection -- the knn and radius masks (fm_mask_create for such banks included), the
 * Hamming Fast-Match family (fm_hamming_self_dist(_batch), fm_hamming_set_selfdist, fm_hamming_match_*), the fm_collection_*
 * calls (fm_collection_add_dev with FM_DT_BIN2 included), every L2-only call, fm_expand_create, the async and batch forms.  A
 * FM_BANK_BIN2 bank paired with a bank of any other kind is FM_EINVAL, even when one of them is empty -- a NORM_HAMMING bank
 * (FM_BANK_BIN) of the same width included: the two norms never mix.                                                          */
int fm_bank_create_bin2(fm_ctx* ctx, const uint8_t* rows /*[n][bytes]*/, int64_t n, int bytes, fm_bank** bank);
/* ---- K14: wide float banks, 129 .. 256 values per row ---------------------------------------------------------------------
 * The 256-D float descriptors of learned extractors (SuperPoint and its kin).  fm_bank_create_f32, fm_bank_create_f32_route and
 * fm_bank_create_dev with FM_DT_F32 / FM_DT_F16 / FM_DT_BF16 (half and bfloat16 widened exactly, the source read in place at
 * its pitch) make a bank of kind FM_BANK_F32W for every 129 <= dim <= 256, WHATEVER the values: integer-valued rows do not go
 * to the int8 route.  n may be 0 -- the bank is still FM_BANK_F32W -- and fm_bank_info reports the real dim.  dim > 256 is
 * FM_EUNSUPPORTED; so are uint8 rows wider than 128 (fm_bank_create_u8, FM_DT_U8) and the gather / capacity creators.  A host
 * and a device creator given the same values build the same bank bit for bit.
 * Contract: the float32 route's, at the wider row.  dist(q, t) = sqrtf(s), s = fmaf(v_k, v_k, s), v_k = q_k - t_k in float32,
 * k ascending over the real dim; results are bit-identical to that chain.  Lists ascend by (distance bits, train index), the
 * lowest index wins a tie, -1 / +inf where there are fewer than k rows, NaN never beats anything.
 * Served, with the semantics and the argument checks they have on the float32 route: fm_knn2, fm_knn with k = 1, 2, fm_xcheck1,
 * fm_knn2_ratio, fm_mutual_ratio, and fm_knn_dev (k <= 2), fm_xcheck1_dev, fm_knn2_ratio_dev, fm_mutual_ratio_dev.  A wide
 * bank paired with a bank of another kind or another dim is FM_EINVAL, even when one of them is empty.
 * Kernels (wide_f32.hip): an exact all-pairs kernel on the vector ALUs, and an fp16 filter on the matrix cores
 * (v_mfma_f32_16x16x32_f16, ceil(dim / 32) K steps) whose candidates are rescored with the exact chain; the option "f32_filter"
 * chooses as on the float32 route (0 exact kernel only, 1 filter from nq * nt >= 4e6, 2 always; banks with a value that is
 * not finite, or whose scales differ by more than 2^8, take the exact kernel) and never changes a result; "f32_nsplit" sets
 * the filter's splits; fm_f32_filter_stats counts the wide filter's launches and its whole-call fallbacks too.
 * A performance cliff to know: the filter keeps its candidates in one list of 256 records per output row (at least 2^20, at most
 * 2^24 records of 12 bytes: up to 192 MiB of the context's workspace) and has no per-row rescan, so a call in which more
 * candidates than that lie inside the fp16 margin -- one large cluster of exact or near duplicates is enough, e.g. 2100 copies of a
 * row against 600 queries next to it -- is redone as a whole by the exact kernel, 7 to 10 times slower; the results are the same.
 * Every other entry point that takes a bank or a collection refuses a wide bank with FM_EUNSUPPORTED and a message that says
 * "wide", before any kernel reads it.  Not built for wide float banks: fm_knn / fm_knn_dev with k >= 3, fm_radius_match(_dev),
 * fm_self_dist(_batch), fm_bank_set_selfdist, fm_match_ratio, fm_match_accepted*, fm_xcheck1_keys*, fm_xcheck1_batched,
 * fm_knn_masked(_dev), fm_bank_refill_u8_async, fm_bank_append_*, fm_expand_create, and every fm_collection_* call -- a wide
 * query bank, and fm_collection_add_f32 / fm_collection_add_dev with more than 128 values per row.  (Fast-Match's self-distance
 * test on wide banks comes under names of its own, "Wide Fast-Match" below: fm_wide_self_dist(_batch), fm_wide_set_selfdist,
 * fm_wide_match_ratio, fm_wide_match_accepted(_dev), fm_collection_wide_match_accepted_each(_dev); the L2-named calls of this
 * list keep refusing.)  (Radius queries on wide banks come under names of their own as well, "Wide radiusMatch" below:
 * fm_wide_radius_match(_dev), and fm_collection_wide_radius_match(_dev) for a wide collection; fm_radius_match(_dev) keeps
 * refusing.)
 * Wide COLLECTIONS: wide images enter a collection through entry points of their own, fm_collection_add_wide (host float32
 * rows) and fm_collection_add_wide_dev (device rows of FM_DT_F32 / FM_DT_F16 / FM_DT_BF16, widened exactly; source, pitch,
 * alignment, ordering and synchronisation rules are fm_collection_add_dev's).  129 <= dim <= 256; dim <= 128 is FM_EINVAL (such
 * rows go to fm_collection_add_f32), dim > 256 FM_EUNSUPPORTED, another dtype FM_EINVAL.  The first successful wide add fixes
 * the collection's kind, FM_BANK_F32W, and its width, even with n = 0 (as the wide bank creators do); a wide add to a
 * collection on which any other add has succeeded is FM_EINVAL, and so is any other add to a wide collection, and another
 * width; every refusal leaves the collection unchanged; fm_collection_clear resets kind and width.  Any values are accepted:
 * there is no FM_COLLECTION_F32_MAX limit, because the padding rows behind an image are excluded by index, never by value; a
 * value that is not finite switches the fp16 filter off for the collection and changes no result.  Host and device adds of
 * the same values build the same collection bit for bit (half and bfloat16: of their widened float32 values) and may
 * alternate.  The stack keeps ONE fp16 scale, K8's rule on the largest finite magnitude added so far: an add that lifts the
 * maximum out of the scale's range rewrites the fp16 plane and the norm terms of every image on the device from the float32
 * rows (nothing is uploaded again); the scale is never lowered again.
 * Served on a wide collection: fm_collection_info (kind FM_BANK_F32W, the real dim), fm_collection_image_rows,
 * fm_collection_train, fm_collection_clear, fm_collection_destroy, and fm_collection_pairs_mutual_ratio(_dev) with its
 * contract word for word: pair (a, b) equals, row by row and bit for bit, fm_mutual_ratio on banks made by fm_bank_create_f32
 * from the same values; the ordered-pair rule, a == b, repeated pairs, pairs == NULL, the packed output, cap, counts only, the
 * error order and the _dev stream rules are unchanged.  There the slots (one direction of one pair) of a whole chunk of pairs
 * lie side by side in one output-row space and run through table forms of the wide kernels -- ONE filter launch, ONE
 * rescoring launch, ONE guarded exact launch and ONE merge launch per chunk, whatever the number of pairs; a workgroup finds
 * its slot by binary search in a prefix array in device memory -- then the join, scan and compaction of the other kinds.  The
 * option "f32_filter" chooses per CHUNK as it does per call for a bank pair (0: the exact kernel alone; 1: the filter from
 * 2 * sum rows(a) rows(b) >= 4e6 over the chunk's pairs; 2: always) and never changes a result; a slot takes one split when
 * the chunk's slots fill the chip without splits (512 workgroups), else the bank-pair rule for its own size.
 * fm_f32_filter_stats counts one launch per filtered chunk and one fallback per chunk redone.  The cliff above is PER CHUNK
 * here: a chunk shares one list of 256 records per output row (at least 2^20 records), so one pair whose candidates overflow
 * it -- a cluster of duplicates -- sends the whole chunk, not the whole call, to the exact kernel; a smaller "coll_ws_bytes"
 * bounds what one such pair can cost.
 * Not built for wide collections: every other fm_collection_* call -- fm_collection_knn(_dev), fm_collection_knn2_ratio(_dev),
 * fm_collection_knn2_each, fm_collection_votes, fm_collection_knn_masked(_dev), fm_collection_radius_match(_dev),
 * fm_collection_match_accepted_each(_dev), fm_collection_xcheck1_each(_dev), fm_collection_mutual_ratio_each(_dev) -- and
 * fm_mask_create_coll: FM_EUNSUPPORTED with a message that says "wide", straight after the NULL-handle checks.  Also not
 * built: k >= 3, LDS staging of the streamed operand, computing a pair's tiles once for both directions.  (Radius queries
 * against a wide collection come under names of their own, "Wide radiusMatch" below: fm_collection_wide_radius_match(_dev);
 * fm_collection_radius_match(_dev) keeps refusing.)  (The stacked knn forms against a wide collection -- knnMatch over all
 * images, the ratio test on it, votes -- come under names of their own too, "Wide stacked knnMatch" below:
 * fm_collection_wide_knn(_dev), fm_collection_wide_knn2_ratio(_dev), fm_collection_wide_votes; the calls listed keep refusing.)
 * Wide QUERIES: a wide query bank is matched against every image of a wide collection, image by image, by entry points of
 * their own -- the calls listed above keep refusing, and their messages name these: fm_collection_wide_knn2_each,
 * fm_collection_wide_mutual_ratio_each and fm_collection_wide_mutual_ratio_each_dev (the localisation pattern: one query image
 * against the N database images that retrieval returned, mutual nearest neighbour + ratio per image).  Slot i of
 * fm_collection_wide_knn2_each (idx / dist [n_images][nq][2]) equals fm_knn2(q, B_i), and image i of the two mutual calls equals
 * fm_mutual_ratio(q, B_i, tau, symmetric) row by row and bit for bit, B_i being a bank made by fm_bank_create_f32 from the
 * values of image i: qidx is the query row, tidx the row inside image i, dist is d0, ratio the forward ratio (symmetric: the
 * larger of the two), rows ascend in qidx, and every rule of fm_mutual_ratio holds -- tau = +inf, a missing second neighbour,
 * 0 / 0, the lowest index wins a tie, NaN never beats anything.  Images are independent (a descriptor present in two images can
 * match in both); an empty image keeps its slot and accepts nothing (knn2: -1 / +inf).  The mutual calls pack their output by
 * fm_collection_pairs_mutual_ratio's rules with "image" for "pair": offsets[0 .. n_images] always hold the full counts,
 * offsets[n_images] = *n_total, rows are written for the longest prefix of whole images that fits in cap, cap = 0 is counts
 * only (the row arrays may be NULL; the counts are the per-image votes); the _dev form writes 12-byte rows {query row, row
 * inside the image, float32 distance bits}, orders consumer_stream in both directions, waits for the device only when n_total
 * is asked for and is not accounted in fm_stats; the host mutual form waits only for its copy out and adds 2 nq sum rows_i
 * pairs to fm_stats, fm_collection_wide_knn2_each nq sum rows_i.  Errors, in this order: NULL handles or a foreign context
 * (FM_EINVAL); a collection that holds images of another kind (FM_EINVAL, the message names fm_collection_mutual_ratio_each or
 * fm_collection_knn2_each; a collection on which no add has succeeded is valid and gives offsets[0] = 0); a query that is not
 * FM_BANK_F32W or whose width is not the collection's (FM_EINVAL, even for an empty query: the wide creators make an empty bank
 * wide); cap < 0, offsets NULL, a row array NULL with cap > 0 (FM_EINVAL; the _dev form checks that its pointers are device
 * memory); for fm_collection_wide_knn2_each idx or dist NULL with n_images * nq > 0 (FM_EINVAL).  nq = 0, a collection of empty
 * images only and n_images = 0 are valid.  Kernels: the table forms above with ONE OPERAND OUTSIDE THE STACK -- a slot is one
 * direction of one image (forward: the query rows are the output rows, image i the reduced rows; reverse: the other way
 * round) and carries which side is the query bank, the two exact scale factors between the query's fp16 scale (fixed at its
 * creation) and the stack's (read at the call) and the reduced side's largest scaled squared norm; ONE filter launch, ONE
 * rescoring launch, ONE guarded exact launch and ONE merge launch per chunk of consecutive images ("coll_ws_bytes"; per image
 * pad128(nq) + pad128(rows_i) output rows, 256 records of 12 bytes per output row, at least 2^20 records), no host wait between
 * the sweeps.  "f32_filter" chooses per chunk and never changes a result: 0 the exact kernel alone, 1 the filter from
 * 2 nq sum rows_i >= 4e6 over the chunk's images (knn2: nq sum rows_i), 2 always; the exact kernel alone when a value on either
 * side is not finite or the two scale exponents differ by more than 8; fm_f32_filter_stats counts one launch per filtered chunk
 * and one fallback per chunk redone (the cliff above, per chunk); "f32_nsplit" keeps its meaning.  Out of scope here: the
 * stacked forms on a wide collection (knnMatch over all images, knn2_ratio, votes mode 0), xcheck1_each / match_accepted_each
 * for wide collections, k >= 3, masks, radius queries, sharing one resident copy of the query's B operand across the forward
 * slots of a chunk, LDS staging of the streamed operand, computing an image's tiles once for both directions.  (Radius
 * queries of a wide query bank against the STACKED images of a wide collection now come under a name of their own:
 * fm_collection_wide_radius_match(_dev), "Wide radiusMatch" below; the stacked knn forms under theirs, "Wide stacked
 * knnMatch" below.)                                                                                                       */
int  fm_bank_destroy(fm_ctx* ctx, fm_bank* bank);
int  fm_bank_info(const fm_bank* bank, int64_t* n, int* dim, int* kind);
/* Attach per-row self distances (Metric_Cache.*["distances"], float64, cache.pyx:252,273)
 * to a query bank so that fm_match_ratio can run the ratio test on the device.          */
int  fm_bank_set_selfdist(fm_ctx* ctx, fm_bank* bank, const double* selfdist /*[n]*/);

/* A new image into an existing bank (created by fm_bank_create_u8 / an integer-valued fm_bank_create_f32 with at
 * least as many rows): no allocation and no host synchronisation -- the copy from `rows` (page-locked memory,
 * fm_host_alloc, for a copy that really is asynchronous; [n][dim] uint8) and the preparation kernel are enqueued
 * on the context's UPLOAD stream and run beside the kernels of the other streams.  The reference builds a new
 * Metric_Cache / cell array per image (cache.pyx:263-284, 124-138); a pipeline over a stream of images re-uses
 * the device arrays instead.  Rules: (1) work enqueued earlier that reads the bank must be COMPLETE (fm_wait on a
 * ticket taken after it, or fm_sync) -- the refill does not wait for it; (2) fm_upload_fence() before the first
 * call that uses a refilled bank; (3) self distances attached to the bank are stale: fm_self_dist_batch.       */
int  fm_bank_refill_u8_async(fm_ctx* ctx, fm_bank* bank, const uint8_t* rows /*page-locked*/, int64_t n);
/* Makes everything enqueued on the context AFTER this call wait (on the device) for the refills enqueued before. */
int  fm_upload_fence(fm_ctx* ctx);

/* ---- K2: brute-force 2-NN ------------------------------------------------------------
 * Replaces cv2.BFMatcher(cv2.NORM_L2, crossCheck=False).knnMatch(q, t, k=2)
 *   matchutil.py:39-43 (bf_match), called from cache.pyx:250; Classic Matching.ipynb:63.
 * idx[2*i+r], dist[2*i+r] = r-th nearest train row of query row i (ascending float32 distance,
 * lower train index first on ties -- ties of the float32 distance, as in cv::batchDistance: d^2 = n
 * and n + 1 can share a root from 4 197 200 on); idx -1 / dist +inf where t has fewer than 2 rows. */
int  fm_knn2(fm_ctx* ctx, const fm_bank* q, const fm_bank* t,
             int32_t* idx /*[nq*2]*/, float* dist /*[nq*2]*/);

/* knnMatch(q, t, k) for the other k the reference's operator signature admits (matchutil.py:39-43 bf_match(dt1, dt2, k),
 * 46-67 flann_match: `k` is any int; the reference itself calls k = 1 and 2 only).  idx[k*i+r], dist[k*i+r] as in fm_knn2;
 * k = 1, 2: the matrix-core path of fm_knn2; 3 <= k <= 8: an exact vector-ALU kernel (off the hot path: ~20 ms for
 * 100k x 100k uint8 rows); k > 8: FM_EUNSUPPORTED.                                                           */
int  fm_knn(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, int32_t k,
            int32_t* idx /*[nq*k]*/, float* dist /*[nq*k]*/);

/* ---- K10: radiusMatch ---------------------------------------------------------------------------------------------
 * cv2.BFMatcher(cv2.NORM_L2).radiusMatch(q, t, maxDistance) with compactResult = False: every train row closer than a
 * distance, one list per query row (empty lists included).  The reference has no call site; it is the one-to-many form
 * of Fast-Match's acceptance test d(q, t) < tau * selfdist(q), a radius per query row.
 *   r_i = radius[i] (radius != NULL) or radius_all -- float32(maxDistance), what the cv2 binding passes.
 *   Train row j is in row i's list iff dist(i, j) < r_i, a strict float32 compare; dist is the value fm_knn2 returns
 *   (integer route sqrtf((float)d2) of the exact int32 d2, float32 route K5's chain s = fmaf(v, v, s), k ascending,
 *   then sqrtf).  r <= 0 or NaN: an empty list; r = +inf: every train row.  nq = 0 and nt = 0 are valid.
 *   A list ascends by (distance bits, train index): OpenCV sorts by distance with an unstable std::sort, so any order
 *   of ties is OpenCV-legal; this one is deterministic.
 * Output: offsets[0 .. nq] always written (offsets[nq] = *n_total, the number of entries; n_total may be NULL);
 * idx / dist[0 .. offsets[m]) written for the longest prefix of rows m whose whole lists fit in cap (cap = 0: counts
 * only, idx / dist may be NULL).  A caller sizes its arrays with a counts call and repeats it with cap = *n_total.
 * Integer route: v_mfma_i32_16x16x64_i8 sweep against the per-row limit D_i = the largest d2 with sqrtf(d2) < r_i;
 * float32 route: an fp16-MFMA filter within K8's margin, then the exact chain for the candidates (radius.hip).
 * fm_collection_radius_match asks the same of a train collection, fm_radius_match_dev / fm_collection_radius_match_dev take the
 * radii from and leave the lists in device memory: both described below.                                              */
int fm_radius_match(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, const float* radius /*[nq] or NULL*/,
                    float radius_all, int64_t cap, int64_t* offsets /*[nq+1]*/, int32_t* idx, float* dist,
                    int64_t* n_total);
/* ---- Hamming radiusMatch ---------------------------------------------------------------------------------------------
 * cv2.BFMatcher(cv2.NORM_HAMMING).radiusMatch on two binary banks (FM_BANK_BIN, K11): "every database row within 50 bits of
 * this one".  fm_radius_match and its kin keep refusing binary banks; these four calls, with the signatures of the four
 * L2 radius calls, are the ones that serve them.
 *   h(q, t) = popcount(q XOR t) over the banks' `bytes` bytes, W = 8 * bytes, dist = (float)h, exact (K11's contract).
 *   r_i = radius[i] (radius != NULL) or radius_all, float32.  Train row j is in row i's list iff (float)h(i, j) < r_i, a STRICT
 *   float32 compare -- fm_radius_match's rule.  Distances are integers, so an inclusive threshold h <= H is r = H + 0.5f.
 *   r <= 0 or NaN: an empty list; r = +inf, or any r > W: every real row.  A list ascends by (h, train index).
 *   offsets / cap / counts-only / longest-prefix-of-whole-rows / *n_total: fm_radius_match's rules, word for word; nq = 0 and
 *   nt = 0 give all-zero offsets.  No option changes a result; "radius_ws_bytes" keeps its meaning (24 bytes a candidate).
 * One FP4 matrix-core sweep (radius.hip, radius_ham_kernel): K11's operands and K11's double-buffered 128-row loop with a
 * threshold epilogue on the raw dot product W - 2 h -- a hit is dot >= W - 2 H_i, H_i the largest integer below r_i
 * (csrc/ham_radius.h); a count sweep, a scan, a fill sweep that writes (float bits of h << 32 | row) keys, K10's segment sort
 * and compaction.  Padding rows (all-zero FP4 rows: h = W / 2 from everything, inside any r > W / 2) are kept out by INDEX.
 * Errors, in this order: NULL handles (check_pair's checks, as in fm_knn2); a bank that is not FM_BANK_BIN (FM_EINVAL, even when it is empty;
 * fm_radius_match is the L2 call); widths that differ (FM_EINVAL); cap < 0; offsets NULL; idx or dist NULL with cap > 0
 * (FM_EINVAL).  Accounted in fm_stats like fm_radius_match, pairs = nq * nt.
 * fm_collection_hamming_radius_match and the _dev forms: with the collections and the device entry points below.          */
int fm_hamming_radius_match(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, const float* radius /*[nq] or NULL*/,
                            float radius_all, int64_t cap, int64_t* offsets /*[nq+1]*/, int32_t* idx, float* dist,
                            int64_t* n_total);

/* ---- Hamming Fast-Match: the self-distance test on binary banks ----------------------------------------------------------
 * Fast-Match's accepted-match test -- dist(q, t) / selfdist(q) < tau on the cross-checked 1-NN -- for binary descriptors
 * (FM_BANK_BIN, K11).  fm_self_dist(_batch), fm_bank_set_selfdist, fm_match_ratio and fm_match_accepted* keep refusing binary
 * banks; the calls below, with the argument lists of their L2 namesakes, are the ones that serve them.
 *   selfdist[i] = (double) min over j != i of popcount(row_i XOR row_j), exact: the second column of fm_knn2(b, b), the value
 *     only.  +inf for a bank of one row; 0 for a row that has a duplicate.
 *   dist = (float)h(q, t); ratio = (double)dist / selfdist[q] in float64; a row is accepted iff ratio < tau.  So a query row
 *     with a duplicate (selfdist 0) is never accepted -- d / 0 = +inf for d > 0 and 0 / 0 = NaN, neither is < tau -- and in a
 *     bank of one query row (selfdist +inf) the ratio is 0, accepted for every tau > 0.
 *   The cross-check is fm_xcheck1's Hamming contract: strict <, the lowest index wins a tie.
 *   fm_hamming_self_dist: synchronous, as fm_self_dist.  fm_hamming_self_dist_batch: as fm_self_dist_batch -- the values are
 *     attached to every bank on the device; with out NULL (or every out[i] NULL) the call only enqueues; a bank listed twice is
 *     FM_EINVAL.  fm_hamming_set_selfdist attaches the caller's values (fm_bank_set_selfdist's rules).
 *   fm_hamming_match_ratio / fm_hamming_match_accepted / fm_hamming_match_accepted_dev: outputs, compaction order, cap and
 *     n_accepted are those of fm_match_ratio / fm_match_accepted / fm_match_accepted_dev, word for word.
 * One FP4 matrix-core sweep of the bank against itself (hamming.hip, ham_self_kernel): K11's top-1 loop, the diagonal candidate
 * dropped in the one stage per wave that holds it, every other stage K11's unmasked body; one launch covers up to "batch_group"
 * banks of one K-step count through a (bank, chunk, split) table in device memory; a merge kernel takes the minimum over the
 * splits.  Padding rows are kept out by INDEX (an all-zero FP4 row is W / 2 from everything; real neighbours can be farther).
 * The match calls run the cross-check's sweep, election, ratio test and compaction of the L2 calls, without a ratio cut.
 * Errors, in this order: NULL handles (and, for the collection forms, a collection of another context): FM_EINVAL; a bank or a
 * collection that is not binary: FM_EINVAL, the message names the L2 call; widths that differ: FM_EINVAL; a query bank with
 * rows but without self distances: FM_EINVAL ("no self distances"); cap < 0 and NULL outputs as in the L2 forms.  Empty banks
 * and empty collections are valid.  fm_stats counts n * n pairs for a self sweep and nq * nt for a match; fm_bank_info is
 * unchanged.
 * Not built: a triangular sweep (every tile once, for both directions); an accepted-only Hamming sweep seeded with the ratio
 * cut; fm_expand_* on binary banks; the async / batch / sharded-key forms (fm_match_accepted_async, _batch, _dev_async,
 * _dev_batch, fm_xcheck1_keys*) for binary banks; NORM_HAMMING2.  (NORM_HAMMING2 has since come for knnMatch, crossCheck,
 * the ratio tests and radiusMatch on bank pairs -- "K11b: NORM_HAMMING2" above -- and stays out of Fast-Match.)
 * fm_collection_hamming_match_accepted_each(_dev): with the collections below.                                            */
int fm_hamming_self_dist(fm_ctx* ctx, const fm_bank* bank, double* selfdist /*[n]*/);
int fm_hamming_self_dist_batch(fm_ctx* ctx, int32_t n, fm_bank* const* banks, double* const* out /*NULL, or [n] of NULL / [n_i]*/);
int fm_hamming_set_selfdist(fm_ctx* ctx, fm_bank* bank, const double* selfdist /*[n]*/);
int fm_hamming_match_ratio(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, double tau, int32_t* tidx /*[nq]*/,
                           float* dist /*[nq]*/, double* ratio /*[nq] or NULL*/, uint8_t* pass /*[nq] or NULL*/, int64_t* n_pass);
int fm_hamming_match_accepted(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, double tau, int64_t cap,
                              int32_t* qidx, int32_t* tidx, float* dist, double* ratio, int64_t* n_accepted);
int fm_hamming_match_accepted_dev(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, double tau, int64_t cap,
                                  int32_t* d_rows /*device [cap][3]*/, int64_t* d_count /*device*/, int64_t* n_accepted);

/* ---- Wide Fast-Match: the self-distance test on wide float banks ---------------------------------------------------------
 * Fast-Match's accepted-match test -- dist(q, t) / selfdist(q) < tau on the cross-checked 1-NN -- for wide float descriptors
 * (FM_BANK_F32W, 129 .. 256 values per row, K14).  fm_self_dist(_batch), fm_bank_set_selfdist, fm_match_ratio,
 * fm_match_accepted* and fm_collection_match_accepted_each(_dev) keep refusing wide banks; the calls below, with the argument
 * lists of their L2 namesakes, are the ones that serve them.
 *   selfdist[i] = (double) min over j != i of dist(i, j), dist being K14's exact chain -- sqrtf(s), s = fmaf(v_k, v_k, s),
 *     k ascending over the real dim; the comparison is strict <, starting from +inf, so a NaN or +inf distance never becomes the
 *     minimum: fm_self_dist's float32-route definition at the wider row.  +inf for a bank of one row and for a row that holds
 *     a NaN (or an infinite value); 0 for a row that has an exact duplicate.  For banks whose values are all finite it equals
 *     the second column of fm_knn2(b, b), the value only.
 *   The cross-check is fm_xcheck1's wide contract: strict <, the lowest index wins a tie, NaN never beats anything.
 *   ratio = (double)dist / selfdist[q] in float64; a row is accepted iff ratio < tau.  So a query row with a duplicate
 *     (selfdist 0) is never accepted -- d / 0 = +inf for d > 0 and 0 / 0 = NaN, neither is < tau -- and in a bank of one query
 *     row (selfdist +inf) the ratio is 0, accepted for every tau > 0.  There is no ratio cut.
 *   fm_wide_self_dist: synchronous, as fm_self_dist.  fm_wide_self_dist_batch: as fm_self_dist_batch -- the values are attached
 *     to every bank on the device; with out NULL (or every out[i] NULL) the call only enqueues; a bank listed twice is
 *     FM_EINVAL.  It runs one sweep per bank, enqueued back to back: separate banks do not share a stack, so the table forms
 *     of the wide kernels do not apply.  fm_wide_set_selfdist attaches the caller's values (fm_bank_set_selfdist's rules).
 *   fm_wide_match_ratio / fm_wide_match_accepted / fm_wide_match_accepted_dev: outputs, compaction order (ascending query
 *     index), cap and n_accepted / n_pass are those of fm_match_ratio / fm_match_accepted / fm_match_accepted_dev, word for word.
 *   fm_collection_wide_match_accepted_each(_dev), on a wide collection (fm_collection_add_wide): slot i equals, row by row and
 *     bit for bit, fm_wide_match_accepted(q, B_i, tau, cap), B_i being a bank made by fm_bank_create_f32 from image i's values.
 *     The output layouts, cap, d_counts / h_counts, the chunking under "coll_ws_bytes" and the _dev stream rules are
 *     fm_collection_match_accepted_each(_dev)'s; an empty image keeps its slot and accepts nothing.
 * Kernels (wide_f32.hip): a SELF form of K14's fp16 filter, of its rescoring and of its exact kernel -- one sweep of the bank
 * over itself with the diagonal candidate dropped by INDEX, in the one 16-row tile per block of output rows that holds it
 * (a scalar branch sends every other tile to an unmasked copy of the tile's tail), before it can enter the filter's bound: its score is the row's maximum, and in
 * the bound it would shut every real neighbour out.  The filter's margin is unchanged, because the diagonal leaves by index
 * and not by value.  Padding rows stay excluded by index.  "f32_filter" and "f32_nsplit" choose the kernel as for a wide bank
 * pair (n * n in the place of nq * nt) and never change a result; fm_f32_filter_stats counts the self sweeps' filter launches
 * and whole-call fallbacks; the cliff described under K14 holds for a self sweep too (a cluster of more than ~1000 exact
 * duplicates overflows the record list and the exact kernel redoes the sweep).  The match calls run the cross-check's reverse
 * top-1 sweep of a wide pair, then the election, ratio test and compaction of the L2 calls.  The collection forms use the
 * table forms of the wide kernels with an operand outside the stack, top-1 and reverse slots alone (output rows = the rows of
 * image i, reduced rows = q): the non-empty images of a chunk lie side by side in one output-row space and run through ONE
 * filter launch, ONE rescoring launch and ONE guarded exact launch -- a chunk whose images hold more than 2^18 rows together
 * is swept in groups of that size, which bounds the record list at 2^26 records -- then a segmented election (every image
 * row's key scatter-mins into qbest[image][q]), the float64 ratio test against q's self distances and the ordered
 * compaction of fm_collection_match_accepted_each.  "f32_filter" chooses per group as it does per chunk for the match graph
 * (1: the filter from nq * rows >= 4e6), and fm_f32_filter_stats counts one launch per filtered group and one fallback per
 * group redone.
 * Errors, in this order: NULL handles (and, for the collection forms, a collection of another context): FM_EINVAL; a bank or a
 * collection that is not wide (FM_BANK_F32W): FM_EINVAL, the message names the L2 or the Hamming call that serves it; dims
 * that differ: FM_EINVAL; a query bank with rows but without self distances: FM_EINVAL ("no self distances"); cap < 0 and NULL
 * outputs as in the L2 forms.  Empty banks and empty collections are valid.  fm_stats counts n * n pairs for a self sweep and
 * nq * nt for a match.
 * Not built: a triangular sweep (every tile once, for both directions); the async / batch / sharded-key forms
 * (fm_match_accepted_async, _batch, _dev_async, _dev_batch, fm_xcheck1_keys*) for wide banks; fm_expand_* on wide banks; wide
 * radiusMatch, masks, k >= 3; a shared launch for fm_wide_self_dist_batch.  (radiusMatch on wide banks has since come under
 * names of its own: "Wide radiusMatch" below; masks on wide knnMatch and on wide radiusMatch too: "Wide knnMatch masks",
 * "Masked radiusMatch".)                                                                                                  */
int fm_wide_self_dist(fm_ctx* ctx, const fm_bank* bank, double* selfdist /*[n]*/);
int fm_wide_self_dist_batch(fm_ctx* ctx, int32_t n, fm_bank* const* banks, double* const* out /*NULL, or [n] of NULL / [n_i]*/);
int fm_wide_set_selfdist(fm_ctx* ctx, fm_bank* bank, const double* selfdist /*[n]*/);
int fm_wide_match_ratio(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, double tau, int32_t* tidx /*[nq]*/,
                        float* dist /*[nq]*/, double* ratio /*[nq] or NULL*/, uint8_t* pass /*[nq] or NULL*/, int64_t* n_pass);
int fm_wide_match_accepted(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, double tau, int64_t cap,
                           int32_t* qidx, int32_t* tidx, float* dist, double* ratio, int64_t* n_accepted);
int fm_wide_match_accepted_dev(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, double tau, int64_t cap,
                               int32_t* d_rows /*device [cap][3]*/, int64_t* d_count /*device*/, int64_t* n_accepted);

/* ---- Wide radiusMatch: every neighbour closer than a distance, on wide float banks ---------------------------------------
 * cv2.BFMatcher(cv2.NORM_L2).radiusMatch for wide float descriptors (FM_BANK_F32W, 129 .. 256 values per row, K14): for
 * unit-norm learned descriptors "keep every neighbour closer than a fixed distance" (SuperPoint's nn_thresh = 0.7) is the usual
 * acceptance test.  fm_radius_match(_dev) and fm_collection_radius_match(_dev) keep refusing wide banks and wide collections
 * (FM_EUNSUPPORTED, a message that says "wide"); the four calls here, with the argument lists of their L2 namesakes word for
 * word, are the ones that serve them: fm_wide_radius_match, fm_wide_radius_match_dev, fm_collection_wide_radius_match,
 * fm_collection_wide_radius_match_dev (the collection forms are declared with the collections below, the _dev forms' stream
 * rules are described with the device entry points).
 *   fm_radius_match's contract applies word for word, with K14's distance: dist(q, t) = sqrtf(s), s = fmaf(v_k, v_k, s),
 *   v_k = q_k - t_k in float32, k ascending over the real dim.  r_i = radius[i] (radius != NULL) or radius_all.  Train row j is
 *   in row i's list iff dist(i, j) < r_i, a strict float32 compare on the bits fm_knn2 returns for a wide pair.  A NaN or +inf
 *   distance is never listed, not even at r = +inf; r <= 0 or NaN gives an empty list.  A list ascends by (distance bits, train
 *   index) -- against a collection by (distance bits, image, row).  offsets[0 .. nq], cap, counts only (cap = 0), the longest
 *   prefix of whole rows and *n_total are fm_radius_match's rules; nq = 0 and nt = 0 are valid.  No option changes a result;
 *   "radius_ws_bytes" keeps its meaning (24 bytes a candidate, 28 against a collection).
 *   fm_collection_wide_radius_match(q, coll): fm_wide_radius_match(q, T) for T = the rows of a WIDE collection
 *   (fm_collection_add_wide) stacked in image order, every entry reported as (img, idx inside the image) --
 *   fm_collection_radius_match's output rules.  The padding rows behind every image are kept out by INDEX.  The stack's fp16
 *   scale and largest scaled squared norm are read at the call: a later add may rewrite them.
 * Kernels (radius.hip, the wide route of K10): a threshold sweep on the matrix cores -- radius_wide_kernel,
 * v_mfma_f32_16x16x32_f16 on the banks' scaled fp16 planes, ceil(dim / 32) = 5 .. 8 K steps, two blocks of 16 query rows per
 * wave as the B operand, the train rows streamed from memory one 16-row tile ahead -- run twice (count, scan, fill); a
 * candidate is a pair with A = |q'|^2 + |t'|^2 - 2 q'.t' <= (r_i^2 + M)(1 + 2^-20) in the accumulator's units, M = 1.25 * 2^-10
 * (|q'|^2 + max |t'|^2), K14's margin; every candidate is then rescored with the exact chain (radius_wide_rescore_kernel) and
 * kept iff dist < r_i; K10's segment sort and compaction follow unchanged.  When a value on either side is not finite, when
 * the two scale exponents differ by more than 8, or when a bank's largest magnitude lies below 2^-59, every pair is a candidate
 * and the exact chain alone decides: same results.  fm_f32_filter_stats counts one launch per call that ran the fp16 sweep
 * (none for a call on the all-pairs path); there is no fallback to count.
 * Errors, in this order: NULL handles, or for the collection forms a collection of another context (FM_EINVAL); a bank or a
 * collection that is not FM_BANK_F32W (FM_EINVAL, even when it is empty: the wide creators make an empty bank wide; the
 * message names fm_radius_match or fm_hamming_radius_match as the call that serves it; a collection on which no add has
 * succeeded is valid and gives all-zero offsets); dims that differ (FM_EINVAL); cap < 0, offsets NULL, or idx / dist (img, for
 * the collection forms) NULL with cap > 0 (FM_EINVAL); for the _dev forms the device-pointer checks of fm_radius_match_dev.
 * Accounted in fm_stats like fm_radius_match: the host forms add nq * real rows pairs, the _dev forms are not accounted.
 * Not built: masks; compactResult = True; one sweep that counts and fills in a single pass; k >= 3 and the stacked knn forms
 * on a wide collection.  (The stacked knn forms on a wide collection have since come, k = 1, 2: "Wide stacked knnMatch"
 * below; masks on a pair of wide banks have since come: "Masked radiusMatch" below.  A wide collection takes no mask.)     */
int fm_wide_radius_match(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, const float* radius /*[nq] or NULL*/,
                         float radius_all, int64_t cap, int64_t* offsets /*[nq+1]*/, int32_t* idx, float* dist,
                         int64_t* n_total);
int fm_wide_radius_match_dev(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, const float* d_radius /*device [nq] or NULL*/,
                             float radius_all, int64_t cap, int64_t* d_offsets /*device [nq+1]*/, int32_t* d_idx, float* d_dist,
                             int64_t* n_total /*host, or NULL*/, void* consumer_stream /*hipStream_t or FM_NO_STREAM*/);

/* ---- train collections: one query against many images ------------------------------------------------------------------
 * cv2.BFMatcher.add([d1, d2, ...]) / train() / clear() and then match(query) / knnMatch(query, k) against ALL added images,
 * every hit carrying DMatch.imgIdx.  The reference matches image pairs only (matchutil.py:39-43); "which image of my database
 * does this query match" is the other ordinary use of a brute-force matcher.  An fm_collection is an ordered list of train
 * images that live on the device in ONE set of arrays, ready for the sweep kernels: every non-empty image starts on a
 * 128-row stage and ends in proper padding rows (at most 127 rows lost per image; an empty image takes no rows but still
 * takes an image index), so an image is a bank view the top-2 sweep can reduce over, and the whole allocation is one bank
 * for the stacked sweep.  Logical order is (image, row) whatever the physical gaps.
 *   fm_collection_add_u8 / _add_f32: append one image of host rows (rules of fm_bank_create_u8 / _f32; n may be 0).  The
 *     first non-empty image fixes the width.  Rows are uploaded at the add; arrays grow by doubling with device-to-device
 *     copies, so images already resident are never uploaded again.  *img_idx (may be NULL) = the image's index.
 *     A width that does not fit, or a uint8 image after float32 ones (and the reverse), is FM_EINVAL, collection unchanged.
 *     The first non-empty image fixes the kind: uint8 rows and float32 rows whose values are all integers in 0 .. 255 take
 *     the integer route (FM_BANK_I8, fm_bank_create_f32's rule), binary rows FM_BANK_BIN.  The first float32 image with
 *     another value REBUILDS a collection of float32 images on the float32 route (FM_BANK_F32) at that add, on the device,
 *     from the resident int8 rows (nothing is uploaded again); from then on fm_collection_info reports FM_BANK_F32 and a
 *     query must be a float32-route bank (fm_bank_create_f32_route for integer-valued rows).  The fp16 planes of all
 *     images share the power-of-two scale chosen at the rebuild; an image that leaves fp16's range under it (or is not
 *     finite) switches the fp16 filter off for the collection (the all-pairs float32 kernel alone: same results).
 *     VALUE LIMIT of a float32-route collection: its padding rows are masked by value (1e18 in every dimension), which
 *     holds while no finite magnitude exceeds FM_COLLECTION_F32_MAX = 2^57 (~1.44e17; 3 * 2^57 < 1e18).  fm_collection_add_f32
 *     of an image with a larger finite magnitude is FM_EUNSUPPORTED, collection unchanged; so is every match call below
 *     for a query bank that holds one (match image by image with fm_knn / fm_knn2, which have no such limit).  Non-finite
 *     values are not counted (their distances are inf / NaN, never a match); a magnitude of exactly 2^57 is accepted.
 *   fm_collection_add_bin: binary rows of 1 .. 64 bytes (rules of fm_bank_create_bin).
 *   fm_collection_train: makes the device tables (stage -> image, real rows per stage, first row per image) current;
 *     implicit in the first match after an add.
 *   fm_collection_locate: HOST code, no context: (image, row) of logical global rows g (first_row[i] = rows of the images
 *     before i, first_row[n_images] = all rows); -1, or a row outside [0, first_row[n_images]), gives -1 / -1.
 * Matching; q is an ordinary bank of the collection's kind (another kind, or another width: FM_EINVAL):
 *   fm_collection_knn, 1 <= k <= 8 (k > 8: FM_EUNSUPPORTED): fm_knn(q, T, k) for T = the images' rows stacked in image
 *     order, every hit reported as (img, row inside that image).  Lists ascend by (distance as fm_knn2 returns it, img,
 *     row): the earlier image wins a tie, as OpenCV's per-image batchDistance(..., update) with strict insertion does.
 *     -1 / -1 / +inf where the whole collection has fewer than k rows.  k = 1, 2: ONE matrix-core sweep over the whole
 *     allocation (padding rows never beat a real row), the physical row -> (img, row) lookup fused into the merge kernel
 *     (a table per 128-row stage: no search; k = 1 is the first column of the top-2 sweep); k = 3 .. 8: the vector-ALU kernel, then a lookup pass over the nq * k
 *     entries (off the hot path).  The float32-root repair above d^2 = 4 197 200 is included.
 *   fm_collection_knn2_ratio: fm_knn2_ratio over the stacked rows (the classic ratio match against a database).
 *   fm_collection_knn2_each: the 2-NN of every query row inside every image SEPARATELY -- what
 *     `for t in images: knnMatch(q, t, 2)` returns, slot by slot equal to fm_knn2(q, image_i): idx / dist
 *     [n_images][nq][2].  The form retrieval needs: a ratio test against the whole database compares a match with the
 *     second view of the same object and rejects it.  Up to "batch_group" images share one launch of the batched top-2
 *     sweep (a block range and a plan per image, any sizes), one merge launch per sweep launch, no host synchronisation
 *     between launches, one copy out.
 *   fm_collection_votes: number of query rows that pass d0 / d1 < tau (float64, d1 == 0 rejected, as fm_knn2_ratio) per
 *     image; mode 0 = the ratio test of the stacked 2-NN list, counted at the image of the first neighbour; 1 = the
 *     per-image ratio test of fm_collection_knn2_each.  Float32-route and binary collections serve fm_collection_knn2_each
 *     and mode 1 by enqueuing the per-image sweeps (K8 / K5, K11) back to back inside the call: no host synchronisation
 *     between images, one copy out.  Counted on the device (integer atomics: deterministic totals);
 *     only n_images words come back.
 *   fm_collection_match_accepted_each: Fast-Match's accepted-match test (fastmatch.pyx:122-124, 161-165) of q against every
 *     image SEPARATELY: slot i equals, row by row and bit for bit, fm_match_accepted(q, bank(image i), tau, cap) -- every train
 *     row of image i elects its nearest query row (float32 distance, lowest query index on ties), every query row keeps the
 *     closest electing train row of image i (lowest row on ties), kept iff (double)dist / selfdist[q] < tau (NaN and inf
 *     rejected: a query row with self distance 0 is never accepted).  q carries self distances (fm_bank_set_selfdist /
 *     fm_self_dist_batch).  qidx / tidx / dist / ratio are [n_images][cap], rows ascending in query index, tidx = the row
 *     inside image i; n_accepted[i] = the FULL count of image i, rows written = min(count, cap).  Images are independent: a
 *     descriptor present in two images matches in both; an empty image has no rows and keeps its slot.  cap = 0: counts only
 *     (the row arrays may be NULL) -- the self-distance analogue of fm_collection_votes, only n_images words come back.
 *     The test divides by the query row's OWN self distance, so a second view of the same object in the database does not
 *     reject a match the way the stacked d0 / d1 test does.  Integer route: ONE reverse top-1 sweep over the whole
 *     allocation (a train row's election does not depend on its image), a segmented election into (image, query row), one
 *     tail launch for all images; the float32-root repair above d^2 = 4 197 200 is included, per image.  Float32 route: the
 *     per-image sweeps (K8 / K5) enqueued back to back, no host synchronisation between images.  Where the per-(image, query row)
 *     arrays exceed the option "coll_ws_bytes" the images run in chunks of consecutive images, enqueued back to back, one
 *     copy out.  Errors, in this order: NULL handles; a query of another kind or width (FM_EINVAL); a binary collection
 *     (FM_EUNSUPPORTED: fm_collection_hamming_match_accepted_each serves it); a query without self distances (FM_EINVAL);
 *     cap < 0 (FM_EINVAL).  nq = 0 writes zero counts and nothing else; n_images = 0 is valid.
 *   fm_collection_hamming_match_accepted_each(_dev): the two calls above on a BINARY collection and a binary query bank that
 *     carries Hamming self distances ("Hamming Fast-Match" above: fm_hamming_self_dist_batch / fm_hamming_set_selfdist): slot i
 *     equals, row by row and bit for bit, fm_hamming_match_accepted(q, bank(image i), tau, cap).  One reverse FP4 sweep per
 *     chunk of images and the segmented election of fm_collection_xcheck1_each, then the tail of the L2 form.  Errors, in this
 *     order: NULL handles or a collection of another context; a collection (when it has rows) or a query bank that is not
 *     binary (FM_EINVAL: fm_collection_match_accepted_each is the L2 call); widths that differ; a query with rows but without
 *     self distances; cap < 0 and the NULL outputs of the L2 form.
 *   fm_collection_match_accepted_each_dev: the same with the results left on the device: 12-byte rows {query, train row in
 *     the image, float32 distance bits} of image i at d_rows + i * cap * 3, d_counts[i] = min(count, cap) (cap = 0: d_rows
 *     may be NULL).  Enqueued on the context's stream; consumer_stream is ordered against the fills in both directions, as in
 *     fm_match_accepted_dev_batch.  h_counts (host, any memory, or NULL) receives the full counts; asking for them is the
 *     call's one host synchronisation.
 *   fm_collection_xcheck1_each: cv2.BFMatcher(norm, crossCheck=True).match(q, image i) for every image in ONE call -- mutual
 *     nearest neighbours image by image, the matcher of binary (ORB keyframe) and float32 databases, which have no
 *     self-distance test.  Slot i of tidx / dist [n_images][nq] equals, row by row and bit for bit, fm_xcheck1(q, bank(image
 *     i)) on all three collection kinds: every train row of image i elects its nearest query row (lowest query index on
 *     ties), every query row keeps the closest electing row of image i (lowest row on ties), -1 / +inf where none elects it;
 *     the float32-root repair above d^2 = 4 197 200 is included, per image.  An empty image keeps its slot, all -1 / +inf;
 *     images are independent: a descriptor present in two images matches in both.  max_dist: a match is kept iff dist <
 *     max_dist, a strict float32 compare on the reported value -- +inf keeps every match (plain cv2), max_dist <= 0 or NaN
 *     keeps none; a dropped entry reads -1 / +inf.  n_matched[i] (may be NULL) = the query rows kept in image i; with tidx ==
 *     dist == NULL only those n_images words come back: mutual-match votes per image (tidx and dist are given together or
 *     not at all; all three NULL is FM_EINVAL).  Integer route: the front half of fm_collection_match_accepted_each without
 *     the ratio cut -- one reverse top-1 sweep per chunk, the segmented election, the tie list redone exactly.  Binary
 *     collections: ONE reverse K11 sweep per chunk with the stack as the output operand; a padding row (an all-zero FP4 row,
 *     at W / 2 from every query row) leaves a valid key that the election drops by index.  Float32 route: the per-image
 *     sweeps (K8 / K5) enqueued back to back, each with fm_xcheck1's own election into slot i -- no faster than the loop
 *     over fm_xcheck1 but for its per-call costs.  Chunks of consecutive images under the option "coll_ws_bytes" as in
 *     fm_collection_match_accepted_each (17 bytes per (image, query row)).  Errors, in fm_collection_knn's order: NULL
 *     handles; a query of another kind or width (FM_EINVAL; as in fm_collection_radius_match a query bank with no rows is
 *     not held to the kind); a float32-route query with a finite magnitude above FM_COLLECTION_F32_MAX (FM_EUNSUPPORTED);
 *     then the output pointers.  nq = 0 writes zero counts and nothing else; n_images = 0 is valid.
 *   fm_collection_xcheck1_each_dev: the kept matches left on the device, word for word as
 *     fm_collection_match_accepted_each_dev leaves its rows: 12-byte rows {query, train row inside the image, float32
 *     distance bits}, ascending in query index, of image i at d_rows + i * cap * 3; d_counts[i] = min(count, cap) (cap = 0:
 *     d_rows may be NULL; cap < 0: FM_EINVAL); consumer_stream ordered in both directions; h_counts (host, or NULL) receives
 *     the full counts and is the call's one host synchronisation -- on the integer and binary routes the call makes no
 *     other (but for the table upload of the first match after an add).
 *   fm_collection_mutual_ratio_each: fm_mutual_ratio(q, image i, tau, symmetric) for every image in ONE call -- mutual nearest
 *     neighbours that also pass the image's own ratio test, the strong per-image test of binary and float32 databases (which
 *     have no self-distance test).  Slot i of qidx / tidx / dist / ratio [n_images][cap] equals, row by row and bit for bit,
 *     fm_mutual_ratio(q, bank(image i), ...) on all three collection kinds; n_accepted[i] = the FULL count of image i, rows
 *     written = min(count, cap); an empty image keeps its slot with count 0; images are independent: a descriptor present in
 *     two images can match in both.  cap = 0: counts only (the row arrays may be NULL) -- only n_images words come back, the
 *     mutual-ratio votes per image.  The forward lists are fm_collection_knn2_each's; which query rows a train row is nearest
 *     to does not depend on the image it sits in, so the candidates of all images -- (image, query row) entries that passed
 *     the ratio test, each naming its first neighbour by its physical row of the stack -- share ONE restricted reverse sweep,
 *     fm_knn2 of the gathered rows over the query bank (float32-root repair included), in chunks of consecutive candidates
 *     under the option "coll_ws_bytes"; then one join and the per-image ordered compaction.  One host wait between the two
 *     sweeps (the 8-byte candidate count).  Accounted in fm_stats: pairs = nq * real rows + candidates * nq.  Errors, in
 *     fm_collection_xcheck1_each's order: NULL handles; a query of another kind or width (FM_EINVAL; a query bank with no rows
 *     is not held to the kind); a float32-route query with a finite magnitude above FM_COLLECTION_F32_MAX (FM_EUNSUPPORTED);
 *     then the outputs (cap < 0, n_accepted NULL, a row array NULL with cap > 0 and nq > 0: FM_EINVAL).  nq = 0 writes zero
 *     counts and nothing else; n_images = 0 is valid.
 *   fm_collection_mutual_ratio_each_dev: the accepted rows left on the device, word for word as fm_collection_xcheck1_each_dev
 *     leaves its rows: 12-byte rows {query, train row inside the image, float32 distance bits}, ascending in query index, of
 *     image i at d_rows + i * cap * 3; d_counts[i] = min(count, cap) (cap = 0: d_rows may be NULL; cap < 0: FM_EINVAL);
 *     consumer_stream ordered in both directions; h_counts (host, or NULL) receives the full counts.  The call waits once for
 *     the candidate count on every route; asking for h_counts is a second wait.
 *   fm_collection_pairs_mutual_ratio: the images of the collection matched AGAINST EACH OTHER -- the match graph of structure
 *     from motion, panorama stitching and loop closure (COLMAP's exhaustive and sequential matchers,
 *     cv::detail::BestOf2NearestMatcher, a pair list from a retrieval step) -- in ONE call.  pairs: host [n_pairs][2] image
 *     indices; pair p = (a, b) is ORDERED and its rows equal, row by row and bit for bit, fm_mutual_ratio(bank(image a),
 *     bank(image b), tau, symmetric, ...) on integer-route, float32-route and binary collections: qidx = the row inside image
 *     a, tidx = the row inside image b, dist = d0, ratio = the forward ratio (symmetric != 0: the larger of the two), rows
 *     ascending in qidx; the float32-root repair above d^2 = 4 197 200 is included, per pair.  a == b is allowed (it equals
 *     fm_mutual_ratio(v, v)), a pair may appear more than once, (b, a) is another pair than (a, b); empty images keep their
 *     index and accept nothing.  pairs == NULL: every (i, j) with i < j in lexicographic order; n_pairs must then equal
 *     n_images (n_images - 1) / 2 (FM_EINVAL otherwise: it guards the caller's array sizes).  The output is packed, by
 *     fm_radius_match's rules with "pair" for "query row": offsets[0 .. n_pairs] are always written with the FULL counts,
 *     offsets[n_pairs] = *n_total; rows are written for the longest prefix of whole pairs that fits in cap; cap = 0: counts
 *     only (the row arrays may be NULL) -- the edge weights of the match graph.  Both images of a pair are resident bank
 *     views of the stack, so a pair is two full top-2 sweeps (a over b, b over a), a join -- the reverse list of a row's first
 *     neighbour is a plain lookup: no gather, no candidate count, no host wait between the sweeps -- and an ordered
 *     compaction without atomics.  Integer route: the sweeps of a whole chunk of pairs are ONE launch of the batched top-2
 *     kernel whose slot descriptors and prefix array live in device memory (any number of slots; a workgroup finds its slot
 *     by binary search), followed by ONE merge launch; chunks of consecutive pairs under the option "coll_ws_bytes" are
 *     enqueued back to back, a running total on the device keeps the offsets global.  Float32-route and binary collections:
 *     the two per-pair sweeps (K8 / K5, K11) enqueued back to back with no host wait between pairs.  The host form waits
 *     only for its copy out.  Accounted in fm_stats: pairs grow by 2 rows(a) rows(b) per pair.  Errors, in this order: NULL
 *     handles or a foreign context; n_pairs < 0, or pairs NULL with another n_pairs (FM_EINVAL); an image index outside
 *     [0, n_images) (FM_EINVAL, nothing is enqueued); cap < 0, offsets NULL, a row array NULL with cap > 0 (FM_EINVAL).
 *     n_pairs = 0 and an empty collection are valid.
 *   fm_collection_pairs_mutual_ratio_dev: the same into DEVICE memory -- d_offsets [n_pairs + 1], 12-byte rows {row in a, row
 *     in b, float32 distance bits} at d_rows [cap][3] (cap = 0: d_rows may be NULL); consumer_stream ordered in both
 *     directions as in fm_collection_mutual_ratio_each_dev; n_total (host, or NULL): asking for it is the call's only host
 *     wait.  Not accounted in fm_stats.
 *   fm_collection_radius_match: fm_radius_match(q, T, ...) for T = the images' rows stacked in image order -- every database
 *     descriptor within r_i of query row i in ONE matrix-core sweep over the whole allocation (place recognition,
 *     de-duplication, Fast-Match's one-to-many test d(q, t) < tau * selfdist(q)).  Every hit is (img, row inside that image);
 *     membership is the strict float32 compare dist < r_i on the value fm_collection_knn returns for the pair (float32-root
 *     behaviour above d^2 = 4 197 200 included).  The radius rules are fm_radius_match's (r <= 0 or NaN: an empty list; +inf:
 *     every real row; radius[i] overrides radius_all), and so are, word for word, the offsets / cap / counts-only /
 *     longest-prefix-of-whole-rows rules; img is written beside idx and dist.  A list ascends by (distance bits, img, row):
 *     physical order in the stack is logical order, so the sort key (distance bits << 32 | physical row) needs no change.
 *     Empty images keep their index and contribute nothing; an empty collection, nq = 0 and a collection of empty images
 *     only are valid and give all-zero offsets.  The padding rows behind every image are masked by INDEX in the sweep's
 *     epilogue, on both routes (the per-stage real-row table; their values -- norm 2^26, 1e18 per float32 dimension -- would
 *     pass r = +inf), and the physical row -> (img, row) lookup is fused into the compaction.  The option "radius_ws_bytes"
 *     keeps its meaning; a candidate takes 28 bytes here (24 for a pair: + img).  Errors, in fm_collection_knn's order: NULL
 *     handles; a query of another kind or width (FM_EINVAL; as in fm_radius_match a query bank with no rows is not held to
 *     the kind: every creator makes an empty bank an integer-route one); a float32-route query with a finite magnitude above
 *     FM_COLLECTION_F32_MAX (FM_EUNSUPPORTED); a binary collection (FM_EUNSUPPORTED: fm_collection_hamming_radius_match serves it); cap < 0, offsets NULL, or img / idx /
 *     dist NULL with cap > 0 (FM_EINVAL).  Accounted in fm_stats like fm_radius_match, pairs = nq * real rows.
 *   fm_collection_hamming_radius_match: fm_hamming_radius_match(q, T, ...) for T = the stacked rows of a BINARY collection --
 *     "Hamming radiusMatch" above is the contract ((float)h < r_i strict, r <= 0 or NaN nothing, r = +inf or r > W every real
 *     row, no option changes a result), fm_collection_radius_match's the output: img beside idx and dist, a list ascends by
 *     (h, img, row inside the image), the offsets / cap / counts-only / prefix rules word for word; an empty collection, nq = 0
 *     and a collection of empty images give all-zero offsets.  The padding rows behind every image are all-zero FP4 rows at
 *     h = W / 2 and WOULD pass any r > W / 2: they are masked by index with the per-stage real-row table, never by value.  A
 *     candidate takes 28 bytes of "radius_ws_bytes".  Errors: fm_collection_radius_match's handle, kind, width checks (an empty
 *     collection takes any binary query); then a query bank or a collection that is not binary (FM_EINVAL); then cap < 0,
 *     offsets NULL, or img / idx / dist NULL with cap > 0 (FM_EINVAL).  Accounted in fm_stats, pairs = nq * real rows.
 *   fm_collection_add_dev, fm_collection_knn_dev, fm_collection_knn2_ratio_dev, fm_collection_radius_match_dev: images from,
 *     and stacked results into, DEVICE memory -- described with the other device entry points below ("descriptors already on
 *     the GPU").
 * Not built: the STACKED crossCheck on a collection (it has no meaning: OpenCV's batchDistance asserts update == 0 under
 * crossCheck -- recalled; neither cv2 nor its source was at hand; the per-image form is built:
 * fm_collection_xcheck1_each), a single reverse K8 sweep
 * over a float32-route stack (its padding output rows would flood the filter's candidate lists: fm_collection_xcheck1_each
 * and fm_collection_match_accepted_each sweep image by image there), Hamming radiusMatch (for pairs or collections) THROUGH THE
 * L2-NAMED CALLS -- fm_radius_match(_dev) and fm_collection_radius_match(_dev) keep refusing binary data; fm_hamming_radius_match(_dev)
 * and fm_collection_hamming_radius_match(_dev) are the entry points that serve it --, NORM_HAMMING2, radius queries per
 * image separately (an _each form, L2 or Hamming), skipping the second count sweep of the counts-then-fill pattern,
 * masks anywhere but in knnMatch (fm_collection_knn_masked is built; "masks" below lists what is not),
 * the expansion loop on a collection, a batched K8 / K11 (float32 / binary) per-image sweep,
 * binary collections in the self-distance test THROUGH THE L2-NAMED CALLS (fm_collection_hamming_match_accepted_each(_dev)
 * serve them), sharding a collection across GPUs (radius queries included), removing single
 * images, turning an integer-route collection of float32 images into a float32-route one for a
 * non-integer QUERY, and for fm_collection_pairs_mutual_ratio: a sweep that computes a pair's tiles once for both
 * directions (d(i, j) = d(j, i): half the matrix-core work of a pair), sharing sweeps between (a, b) and (b, a) of one
 * pair list (the two pairs run the same two sweeps).  (NORM_HAMMING2 has since come for bank pairs -- "K11b: NORM_HAMMING2"
 * above; a collection still takes no FM_BANK_BIN2 rows and no such query bank: FM_EUNSUPPORTED.)                         */
typedef struct fm_collection fm_collection;
#define FM_COLLECTION_F32_MAX 144115188075855872.0f   /* 2^57: largest finite magnitude of a float32-route collection and its queries */
int  fm_collection_create(fm_ctx* ctx, fm_collection** coll);
int  fm_collection_destroy(fm_ctx* ctx, fm_collection* coll);
int  fm_collection_clear(fm_ctx* ctx, fm_collection* coll);
int  fm_collection_add_u8 (fm_ctx* ctx, fm_collection* coll, const uint8_t* rows, int64_t n, int dim, int32_t* img_idx);
int  fm_collection_add_f32(fm_ctx* ctx, fm_collection* coll, const float* rows, int64_t n, int dim, int32_t* img_idx);
int  fm_collection_add_bin(fm_ctx* ctx, fm_collection* coll, const uint8_t* rows, int64_t n, int bytes, int32_t* img_idx);
/* wide images, 129 <= dim <= 256 ("K14: wide float banks" above, Wide COLLECTIONS) */
int  fm_collection_add_wide(fm_ctx* ctx, fm_collection* coll, const float* rows, int64_t n, int dim, int32_t* img_idx);
int  fm_collection_add_wide_dev(fm_ctx* ctx, fm_collection* coll, const void* d_rows, int dtype /*FM_DT_F32 | F16 | BF16*/, int64_t n, int dim,
                                int64_t row_pitch_bytes, void* producer_stream, int32_t* img_idx);
int  fm_collection_train(fm_ctx* ctx, fm_collection* coll);
int  fm_collection_info(const fm_collection* coll, int32_t* n_images, int64_t* n_rows_total, int* dim, int* kind);
int  fm_collection_image_rows(const fm_collection* coll, int64_t* rows /*[n_images]*/);
int  fm_collection_locate(const int64_t* first_row /*[n_images + 1]*/, int32_t n_images, const int64_t* g /*[m]*/, int64_t m,
                          int32_t* img /*[m]*/, int64_t* local /*[m]*/);
int  fm_collection_knn(fm_ctx* ctx, fm_collection* coll, const fm_bank* q, int32_t k,
                       int32_t* img /*[nq*k]*/, int32_t* idx /*[nq*k]*/, float* dist /*[nq*k]*/);
int  fm_collection_knn2_ratio(fm_ctx* ctx, fm_collection* coll, const fm_bank* q, double tau, int64_t cap,
                              int32_t* qidx, int32_t* img, int32_t* tidx, float* dist, double* ratio, int64_t* n_accepted);
int  fm_collection_knn2_each(fm_ctx* ctx, fm_collection* coll, const fm_bank* q,
                             int32_t* idx /*[n_images][nq][2]*/, float* dist /*[n_images][nq][2]*/);
int  fm_collection_votes(fm_ctx* ctx, fm_collection* coll, const fm_bank* q, double tau, int32_t mode,
                         int64_t* votes /*[n_images]*/);
int  fm_collection_radius_match(fm_ctx* ctx, fm_collection* coll, const fm_bank* q, const float* radius /*host [nq] or NULL*/,
                                float radius_all, int64_t cap, int64_t* offsets /*[nq+1]*/, int32_t* img, int32_t* idx, float* dist,
                                int64_t* n_total);
int  fm_collection_hamming_radius_match(fm_ctx* ctx, fm_collection* coll, const fm_bank* q, const float* radius /*host [nq] or NULL*/,
                                        float radius_all, int64_t cap, int64_t* offsets /*[nq+1]*/, int32_t* img, int32_t* idx,
                                        float* dist, int64_t* n_total);
/* (a wide collection: "Wide radiusMatch" above) */
int  fm_collection_wide_radius_match(fm_ctx* ctx, fm_collection* coll, const fm_bank* q, const float* radius /*host [nq] or NULL*/,
                                     float radius_all, int64_t cap, int64_t* offsets /*[nq+1]*/, int32_t* img, int32_t* idx,
                                     float* dist, int64_t* n_total);
int  fm_collection_match_accepted_each(fm_ctx* ctx, fm_collection* coll, const fm_bank* q, double tau, int64_t cap,
                                       int32_t* qidx, int32_t* tidx, float* dist, double* ratio /* each [n_images][cap] */,
                                       int64_t* n_accepted /*[n_images]: the full count per image*/);
int  fm_collection_match_accepted_each_dev(fm_ctx* ctx, fm_collection* coll, const fm_bank* q, double tau, int64_t cap,
                                           int32_t* d_rows /*device [n_images][cap][3]*/, int64_t* d_counts /*device [n_images]*/,
                                           int64_t* h_counts /*host [n_images] or NULL*/, void* consumer_stream /*hipStream_t or FM_NO_STREAM*/);
int  fm_collection_hamming_match_accepted_each(fm_ctx* ctx, fm_collection* coll, const fm_bank* q, double tau, int64_t cap,
                                               int32_t* qidx, int32_t* tidx, float* dist, double* ratio /* each [n_images][cap] */,
                                               int64_t* n_accepted /*[n_images]: the full count per image*/);
int  fm_collection_hamming_match_accepted_each_dev(fm_ctx* ctx, fm_collection* coll, const fm_bank* q, double tau, int64_t cap,
                                                   int32_t* d_rows /*device [n_images][cap][3]*/, int64_t* d_counts /*device [n_images]*/,
                                                   int64_t* h_counts /*host [n_images] or NULL*/, void* consumer_stream /*hipStream_t or FM_NO_STREAM*/);
/* "Wide Fast-Match" above: the two calls on a wide collection and a wide query bank that carries wide self distances */
int  fm_collection_wide_match_accepted_each(fm_ctx* ctx, fm_collection* coll, const fm_bank* q, double tau, int64_t cap,
                                            int32_t* qidx, int32_t* tidx, float* dist, double* ratio /* each [n_images][cap] */,
                                            int64_t* n_accepted /*[n_images]: the full count per image*/);
int  fm_collection_wide_match_accepted_each_dev(fm_ctx* ctx, fm_collection* coll, const fm_bank* q, double tau, int64_t cap,
                                                int32_t* d_rows /*device [n_images][cap][3]*/, int64_t* d_counts /*device [n_images]*/,
                                                int64_t* h_counts /*host [n_images] or NULL*/, void* consumer_stream /*hipStream_t or FM_NO_STREAM*/);
int  fm_collection_xcheck1_each(fm_ctx* ctx, fm_collection* coll, const fm_bank* q, float max_dist,
                                int32_t* tidx /*[n_images][nq] or NULL*/, float* dist /*[n_images][nq] or NULL*/,
                                int64_t* n_matched /*[n_images] or NULL*/);
int  fm_collection_xcheck1_each_dev(fm_ctx* ctx, fm_collection* coll, const fm_bank* q, float max_dist, int64_t cap,
                                    int32_t* d_rows /*device [n_images][cap][3]*/, int64_t* d_counts /*device [n_images]*/,
                                    int64_t* h_counts /*host [n_images] or NULL*/, void* consumer_stream /*hipStream_t or FM_NO_STREAM*/);
int  fm_collection_mutual_ratio_each(fm_ctx* ctx, fm_collection* coll, const fm_bank* q, double tau, int32_t symmetric, int64_t cap,
                                     int32_t* qidx, int32_t* tidx, float* dist, double* ratio /* each [n_images][cap] */,
                                     int64_t* n_accepted /*[n_images]: the full count per image*/);
int  fm_collection_mutual_ratio_each_dev(fm_ctx* ctx, fm_collection* coll, const fm_bank* q, double tau, int32_t symmetric, int64_t cap,
                                         int32_t* d_rows /*device [n_images][cap][3]*/, int64_t* d_counts /*device [n_images]*/,
                                         int64_t* h_counts /*host [n_images] or NULL*/, void* consumer_stream /*hipStream_t or FM_NO_STREAM*/);
int  fm_collection_pairs_mutual_ratio(fm_ctx* ctx, fm_collection* coll, const int32_t* pairs /*host [n_pairs][2] or NULL*/, int64_t n_pairs,
                                      double tau, int32_t symmetric, int64_t cap, int64_t* offsets /*[n_pairs + 1]*/,
                                      int32_t* qidx, int32_t* tidx, float* dist, double* ratio /* each [cap] */, int64_t* n_total /*or NULL*/);
int  fm_collection_pairs_mutual_ratio_dev(fm_ctx* ctx, fm_collection* coll, const int32_t* pairs /*host [n_pairs][2] or NULL*/, int64_t n_pairs,
                                          double tau, int32_t symmetric, int64_t cap, int64_t* d_offsets /*device [n_pairs + 1]*/,
                                          int32_t* d_rows /*device [cap][3]*/, int64_t* n_total /*host or NULL*/,
                                          void* consumer_stream /*hipStream_t or FM_NO_STREAM*/);
/* a wide query bank against every image of a wide collection ("K14: wide float banks" above, Wide QUERIES) */
int  fm_collection_wide_knn2_each(fm_ctx* ctx, fm_collection* coll, const fm_bank* q, int32_t* idx /*[n_images][nq][2]*/,
                                  float* dist /*[n_images][nq][2]*/);
int  fm_collection_wide_mutual_ratio_each(fm_ctx* ctx, fm_collection* coll, const fm_bank* q, double tau, int32_t symmetric, int64_t cap,
                                          int64_t* offsets /*[n_images + 1]*/, int32_t* qidx, int32_t* tidx, float* dist,
                                          double* ratio /* each [cap] */, int64_t* n_total /*or NULL*/);
int  fm_collection_wide_mutual_ratio_each_dev(fm_ctx* ctx, fm_collection* coll, const fm_bank* q, double tau, int32_t symmetric, int64_t cap,
                                              int64_t* d_offsets /*device [n_images + 1]*/, int32_t* d_rows /*device [cap][3]*/,
                                              int64_t* n_total /*host or NULL*/, void* consumer_stream /*hipStream_t or FM_NO_STREAM*/);

/* ---- descriptors already on the GPU: device sources, device results ---------------------------------------------------------
 * Every creator above takes a HOST array and every dense matcher call ends in host arrays: the shape of the reference, whose
 * descriptors come from OpenCV on the CPU (matchutil.py:31-33 get_features -> sift().detectAndCompute; matched at matchutil.py:39-43,
 * fastmatch.pyx:122-123, 161-162, Classic Matching.ipynb:63).  A pipeline whose extractor runs on the GPU (a PyTorch-ROCm model)
 * holds them as device tensors and wants the matches as device tensors; these four entry points take and leave them there.
 *
 * fm_bank_create_dev: a bank from n rows in DEVICE memory of the context's device (hipPointerGetAttributes: a host pointer or
 *   another device's memory is FM_EINVAL), rows row_pitch_bytes apart (0 = dense; a column slice of a wider tensor is a pitched
 *   matrix; below dim * element size, or not a multiple of the element size: FM_EINVAL).  dtype:
 *     FM_DT_U8   uint8 rows            -> FM_BANK_I8 (fm_bank_create_u8)
 *     FM_DT_F32  float32 rows          -> fm_bank_create_f32's rule: all values integers in 0 .. 255 -> FM_BANK_I8, else FM_BANK_F32;
 *                                         float_route != 0: fm_bank_create_f32_route's (FM_BANK_F32 whatever the values)
 *     FM_DT_F16  IEEE half rows        -> widened to float32 (exact), then as FM_DT_F32
 *     FM_DT_BF16 bfloat16 rows         -> widened to float32 (exact), then as FM_DT_F32
 *     FM_DT_BIN  packed binary rows, dim = bytes (1 .. 64; more: FM_EUNSUPPORTED) -> FM_BANK_BIN (fm_bank_create_bin)
 *   Another dtype is FM_EINVAL, dim > 128 FM_EUNSUPPORTED, n = 0 valid (d_rows is then not looked at).  The preparation kernels
 *   read the caller's memory IN PLACE (typed, pitched forms of the upload kernels; half and bfloat16 widen in registers): no
 *   staging copy, nothing crosses PCIe.  CONTRACT: the bank is the one the host creator named above builds from the same values
 *   (for half / bfloat16: from their float32 values) -- same kind, same device arrays, same fp16 scale, filter and norm terms --
 *   so every entry point returns the same bits for it.
 *   Ordering: the kernels wait (on the device) for the work producer_stream has been given so far -- NULL is the null stream,
 *   FM_NO_STREAM says the rows are complete -- so the caller needs no host synchronisation after producing the rows.  The call
 *   itself synchronises with the context's stream as the host creators do (the route and scale decisions read flag words back),
 *   so on return the bank owns its copy and the source is not read again: the caller may overwrite or free it.
 *
 * fm_knn_dev, fm_xcheck1_dev, fm_knn2_ratio_dev: fm_knn (1 <= k <= 8), fm_xcheck1 and fm_knn2_ratio with the results written to
 *   caller-supplied DEVICE memory -- the same values in the same order, for all three bank kinds, by the same kernels: the
 *   merge / finalize / compaction kernels are handed the caller's pointers (k = 1: one small kernel takes the first column of the
 *   top-2 lists).  fm_knn2_ratio_dev leaves 12-byte rows {query, train, float32 distance bits} and *d_count = min(accepted, cap)
 *   as fm_match_accepted_dev does (the ratio is d_rows' distance over the second distance and is not kept); *n_accepted (host,
 *   may be NULL) = the full number accepted.  Output pointers must be device memory of the context's device (NULL, host memory:
 *   FM_EINVAL; d_rows may be NULL when cap = 0); nq = 0 and nt = 0 are valid (nq = 0 writes *d_count = 0 and nothing else).
 *   Ordering is fm_match_accepted_dev_async's: the kernels that write the caller's arrays first wait for the work consumer_stream
 *   has been given so far (whatever last read these arrays; the sweep in front of them does not wait), and consumer_stream is
 *   made to wait for the writes; NULL is the null stream, FM_NO_STREAM means no such stream (fm_sync, or any synchronous call on
 *   the context, completes the work).  Everything is enqueued on the context's stream behind earlier calls.
 *   Host synchronisation: NONE on the integer and binary routes, except fm_knn2_ratio_dev with n_accepted != NULL (one 8-byte
 *   read).  The float32 route makes no promise: its fp16-filter / all-pairs decision is taken on the device today, but it may
 *   come to need the host, and a workspace that has to grow frees the old one, which waits for the device on every route.
 *   The calls are not accounted in fm_stats.
 *
 * fm_collection_add_dev: fm_collection_add_u8 / _f32 / _bin from rows in DEVICE memory.  The source rules are fm_bank_create_dev's
 *   (device memory of the context's device, pitch, alignment to the element size, n = 0 valid: d_rows is not looked at and the
 *   image still takes an index); dtype FM_DT_U8 behaves as fm_collection_add_u8, FM_DT_F32 as fm_collection_add_f32, FM_DT_F16 /
 *   FM_DT_BF16 are widened exactly to float32 in registers and then follow FM_DT_F32, FM_DT_BIN behaves as fm_collection_add_bin
 *   (dim = bytes).  The collection rules are the host adds', with the same codes: width or kind mixing FM_EINVAL, dim > 128 or
 *   binary rows over 64 bytes FM_EUNSUPPORTED, the first non-empty image fixes width and kind, the first float32 image with a
 *   non-integer value rebuilds the collection on the float32 route, a finite magnitude above FM_COLLECTION_F32_MAX is
 *   FM_EUNSUPPORTED.  Every refusal leaves the collection unchanged.  CONTRACT: the collection is the one the host add of the
 *   same values would have built (half / bfloat16: of their float32 values) -- same device arrays, kind, fp16 scale, filter
 *   and norm terms, padding rows -- so every fm_collection_* call returns the same bits; host and device adds may alternate.
 *   No staging copy: the preparation kernels read the caller's memory in place and write into the collection's arrays at the
 *   image's first physical row.  The largest finite magnitude of a floating-point image, which the host add finds with a loop
 *   over the rows, comes from a reduction kernel over the source (four bytes read back).  Passes over the source: one (uint8,
 *   binary, an integer-valued floating-point image on the integer route), two on the float32 route, three for the image that
 *   causes the rebuild.  Ordering is fm_bank_create_dev's: the kernels wait on the device for what producer_stream has been
 *   given so far, the call synchronises with the context's stream (flag words are read back), and on return the source may be
 *   overwritten or freed.
 * fm_collection_knn_dev, fm_collection_knn2_ratio_dev: fm_collection_knn (1 <= k <= 8) and fm_collection_knn2_ratio with the
 *   results written to caller-supplied DEVICE memory: the same values in the same order on all three collection kinds, the
 *   float32-root repair included, by the same kernels handed the caller's pointers (k = 1: one small kernel takes the first
 *   column).  fm_collection_knn2_ratio_dev leaves 16-byte rows {query, img, row inside the image, float32 distance bits} and
 *   *d_count = min(accepted, cap); *n_accepted (host, may be NULL) = the full number accepted.  Pointer checks, stream ordering
 *   in both directions and host synchronisation are fm_knn_dev's / fm_knn2_ratio_dev's (NULL or host memory: FM_EINVAL; d_rows
 *   may be NULL when cap = 0; nq = 0 writes *d_count = 0 and nothing else; an empty collection writes -1 / -1 / +inf and a zero
 *   count; no host synchronisation on the integer and binary routes except n_accepted != NULL -- and the first match after an
 *   add, which uploads the lookup tables as fm_collection_train does).  Errors in fm_collection_knn's order; k > 8 is
 *   FM_EUNSUPPORTED, k < 1 FM_EINVAL.  Not accounted in fm_stats.
 * fm_radius_match_dev, fm_collection_radius_match_dev: fm_radius_match and fm_collection_radius_match with everything that is
 *   per row or per hit in DEVICE memory: the same values in the same order.  d_radius (device float32 [nq], or NULL for
 *   radius_all) is read in place by the limits kernel -- tau * selfdist computed on the device goes straight in, no staging
 *   copy; d_offsets[0 .. nq] is always written (a device copy of the scan, or a small kernel per chunk on the float32 route);
 *   the compaction writes d_idx / d_dist (and d_img) at each row's final offset, for the longest prefix of rows whose whole
 *   lists fit in cap, and nothing beyond that prefix; *n_total (host, may be NULL) = the number of entries.  d_radius,
 *   d_offsets and the list pointers must be device memory of the context's device (fm_knn_dev's check; a host pointer is
 *   FM_EINVAL); the list pointers may be NULL when cap = 0.  Ordering is fm_knn_dev's in both directions: the first kernel
 *   that reads d_radius or writes a caller array waits on the device for what consumer_stream has been given so far, and
 *   consumer_stream is made to wait for the writes; FM_NO_STREAM means no such stream.
 *   Host synchronisation: the call DOES synchronise -- the counts are read back to plan the chunks and the segment sort (per
 *   chunk on the float32 route), as in the host forms; what it spares is the radii going up and the lists coming down.  The
 *   other errors are the host forms', in their order.  Not accounted in fm_stats.
 * fm_hamming_radius_match_dev, fm_collection_hamming_radius_match_dev: the same device forms of fm_hamming_radius_match and
 *   fm_collection_hamming_radius_match -- d_radius read in place, d_offsets always written, the lists at their final offsets
 *   for the rows that fit in cap; pointer checks (after the host forms' errors), stream ordering, *n_total and the host
 *   synchronisation exactly as in fm_radius_match_dev.  Not accounted in fm_stats.
 * fm_wide_radius_match_dev, fm_collection_wide_radius_match_dev: the same device forms of fm_wide_radius_match and
 *   fm_collection_wide_radius_match ("Wide radiusMatch" above) -- pointer checks (after the host forms' errors), stream
 *   ordering, d_offsets written per chunk, *n_total and the host synchronisation as on fm_radius_match_dev's float32 route.
 *   Not accounted in fm_stats.
 * Not built: device sources for fm_bank_refill_u8_async and fm_bank_append_*; device results for
 *   fm_self_dist (fm_self_dist_batch attaches them on the device already) and for fm_collection_knn2_each / _votes; an
 *   enqueue-only float32 route; tensors on another GPU than the context's (copy them over first).                          */
#define FM_DT_U8   1
#define FM_DT_F32  2
#define FM_DT_F16  3
#define FM_DT_BF16 4
#define FM_DT_BIN  5
#define FM_DT_BIN2 6      /* packed binary rows of 2-bit cells, dim = bytes (1 .. 64) -> FM_BANK_BIN2 (fm_bank_create_bin2); banks only */
int  fm_bank_create_dev(fm_ctx* ctx, const void* d_rows, int dtype, int64_t n, int dim, int64_t row_pitch_bytes /*0 = dense*/,
                        int float_route, void* producer_stream /*hipStream_t, NULL = null stream, or FM_NO_STREAM*/, fm_bank** bank);
int  fm_knn_dev(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, int32_t k, int32_t* d_idx /*device [nq*k]*/,
                float* d_dist /*device [nq*k]*/, void* consumer_stream /*hipStream_t or FM_NO_STREAM*/);
int  fm_xcheck1_dev(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, int32_t* d_tidx /*device [nq]*/, float* d_dist /*device [nq]*/,
                    void* consumer_stream /*hipStream_t or FM_NO_STREAM*/);
int  fm_knn2_ratio_dev(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, double tau, int64_t cap,
                       int32_t* d_rows /*device [cap][3]*/, int64_t* d_count /*device*/, int64_t* n_accepted /*host, or NULL*/,
                       void* consumer_stream /*hipStream_t or FM_NO_STREAM*/);
int  fm_collection_add_dev(fm_ctx* ctx, fm_collection* coll, const void* d_rows, int dtype, int64_t n, int dim,
                           int64_t row_pitch_bytes /*0 = dense*/, void* producer_stream /*hipStream_t, NULL = null stream, or FM_NO_STREAM*/,
                           int32_t* img_idx);
int  fm_collection_knn_dev(fm_ctx* ctx, fm_collection* coll, const fm_bank* q, int32_t k, int32_t* d_img /*device [nq*k]*/,
                           int32_t* d_idx /*device [nq*k]*/, float* d_dist /*device [nq*k]*/, void* consumer_stream /*hipStream_t or FM_NO_STREAM*/);
int  fm_collection_knn2_ratio_dev(fm_ctx* ctx, fm_collection* coll, const fm_bank* q, double tau, int64_t cap,
                                  int32_t* d_rows /*device [cap][4]*/, int64_t* d_count /*device*/, int64_t* n_accepted /*host, or NULL*/,
                                  void* consumer_stream /*hipStream_t or FM_NO_STREAM*/);
int  fm_radius_match_dev(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, const float* d_radius /*device [nq] or NULL*/,
                         float radius_all, int64_t cap, int64_t* d_offsets /*device [nq+1]*/, int32_t* d_idx, float* d_dist,
                         int64_t* n_total /*host, or NULL*/, void* consumer_stream /*hipStream_t or FM_NO_STREAM*/);
int  fm_collection_radius_match_dev(fm_ctx* ctx, fm_collection* coll, const fm_bank* q, const float* d_radius /*device [nq] or NULL*/,
                                    float radius_all, int64_t cap, int64_t* d_offsets /*device [nq+1]*/, int32_t* d_img,
                                    int32_t* d_idx, float* d_dist, int64_t* n_total /*host, or NULL*/,
                                    void* consumer_stream /*hipStream_t or FM_NO_STREAM*/);
int  fm_hamming_radius_match_dev(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, const float* d_radius /*device [nq] or NULL*/,
                                 float radius_all, int64_t cap, int64_t* d_offsets /*device [nq+1]*/, int32_t* d_idx, float* d_dist,
                                 int64_t* n_total /*host, or NULL*/, void* consumer_stream /*hipStream_t or FM_NO_STREAM*/);
int  fm_collection_hamming_radius_match_dev(fm_ctx* ctx, fm_collection* coll, const fm_bank* q, const float* d_radius /*device [nq] or NULL*/,
                                            float radius_all, int64_t cap, int64_t* d_offsets /*device [nq+1]*/, int32_t* d_img,
                                            int32_t* d_idx, float* d_dist, int64_t* n_total /*host, or NULL*/,
                                            void* consumer_stream /*hipStream_t or FM_NO_STREAM*/);
/* (wide banks and wide collections, "Wide radiusMatch" above: fm_wide_radius_match_dev is declared there) */
int  fm_collection_wide_radius_match_dev(fm_ctx* ctx, fm_collection* coll, const fm_bank* q, const float* d_radius /*device [nq] or NULL*/,
                                         float radius_all, int64_t cap, int64_t* d_offsets /*device [nq+1]*/, int32_t* d_img,
                                         int32_t* d_idx, float* d_dist, int64_t* n_total /*host, or NULL*/,
                                         void* consumer_stream /*hipStream_t or FM_NO_STREAM*/);

/* ---- masks: knnMatch(q, t, k, mask) and knnMatch(q, k, masks = [...]) (K13, csrc/masked.hip) --------------------------------
 * cv2's mask argument: a CV_8U [nq][nt] matrix, nonzero = the pair (query row, train row) may be matched; for a train
 * collection one such matrix per added image, an empty entry permitting everything.  (OpenCV's behaviour as RECALLED, not
 * verified -- neither cv2 nor its source was at hand, as for SURVEY.md Appendix A: a masked-out pair is skipped before the
 * distance enters the k-NN insertion, so the result is the unmasked algorithm run over the permitted train rows only.)
 *
 * fm_mask -- a device-resident BIT matrix, [nq][n_pad / 64] 64-bit words, n_pad the padded row count of the train operand:
 *   bit b of word w of row i set = (query row i, train row 64 w + b) is permitted; the bits of rows at or beyond the operand's
 *   real rows are always 0.  (A dense byte mask at 100k x 100k is 10 GB; the bit form is 1.25 GB and is what the kernels read.)
 *   fm_mask_create(ctx, nq, nt, &mask): an all-zero (everything forbidden) mask for a bank pair whose train bank has nt rows.
 *   fm_mask_create_coll(ctx, nq, coll, &mask): an all-zero mask laid out on the collection's PHYSICAL stack: every image
 *     starts on a 128-row stage, so an image's bits are whole words and setting one image never reads or modifies another
 *     image's words; the padding rows behind every image have bit 0, so the masked sweeps need no real-row table.  The mask
 *     remembers the collection, its image count and row total; a later add or clear makes it stale (FM_EINVAL at the match).
 *   fm_mask_set_u8(ctx, mask, img, rows, pitch): the host matrix uint8 [nq][rows of image img], nonzero = permitted, `pitch`
 *     bytes between rows (0 = dense); img = 0 for a pair mask.  Uploaded in chunks of query rows through a bounded workspace
 *     (64 MiB) and packed on the device, one wave per word (64 consecutive bytes of a row, one ballot).  Synchronous.
 *   fm_mask_set_dev(ctx, mask, img, d_rows, pitch, producer_stream): the same from device memory of the context's device, read
 *     in place (a torch.bool tensor is one byte per element); pointer check and producer-stream ordering are
 *     fm_bank_create_dev's, and like it the call returns when the source has been read.
 *   fm_mask_set_all(ctx, mask, img, value): all real rows of one image permitted (value != 0) or forbidden, for every query row.
 *   fm_mask_info: nq, the real train rows, the image count (0 for a pair mask), the bytes of the bit matrix.
 *   Errors: a NULL handle, a mask of another context, an image index outside the mask, a NULL source with nq > 0 and a
 *   non-empty image, a pitch below the row width: FM_EINVAL.  nq = 0, nt = 0 and empty images are valid.
 *
 * fm_knn_masked / fm_knn_masked_dev / fm_collection_knn_masked / fm_collection_knn_masked_dev -- the contract:
 *   row i's list is fm_knn's (fm_collection_knn's) list computed over the PERMITTED train rows of row i only; the distances
 *   are the same bits fm_knn reports for the pair; lists ascend by (float32 distance bits, train index), strictly -- for a
 *   collection by (bits, img, row); where fewer than k rows are permitted the tail is -1 / +inf (img -1 too), a row with no
 *   permitted pair is all -1 / +inf.  1 <= k <= 8 on all three bank kinds.
 *   Errors, in this order: (1) NULL handles (ctx, banks / collection, mask): FM_EINVAL; (2) check_pair's rules as in fm_knn --
 *   width or kind mismatch -- or fm_collection_knn's for the collection forms; (3) k < 1: FM_EINVAL, k > 8: FM_EUNSUPPORTED;
 *   (4) FM_EINVAL with a message that says which: a mask of another context, a mask whose nq differs from the query bank's
 *   rows or whose train rows differ from the train bank's, a pair mask given to a collection form and the reverse, a mask of
 *   another collection, a collection that has changed (add or clear) since fm_mask_create_coll; (5) the output pointers
 *   (NULL with nq > 0: FM_EINVAL; the device forms: fm_knn_dev's pointer checks).
 *   The device forms order themselves against consumer_stream in both directions as fm_knn_dev does and are not accounted in
 *   fm_stats; the host forms are accounted like fm_knn (pairs = nq * real train rows).
 *   Routes: integer route (FM_BANK_I8) with k = 1 or 2: the masked sweep on the MATRIX CORES (v_mfma_i32_16x16x64_i8; one
 *   8-byte mask word per 16 query rows x 64 train rows and lane; a wave skips the MFMAs of a stage, and of a 16 x 16 tile,
 *   in which it has no permitted pair).  Everything else -- k = 3 .. 8 on the integer route, every k on the float32 route
 *   (K5's chain: fm_knn2's bits) and for binary banks -- runs on the VECTOR ALUs, the exact list kernels of fm_knn with one
 *   mask bit tested per candidate; NOT on the matrix cores.  Candidates are ordered by the float32 root inside the kernels,
 *   so no float32-root repair pass exists or is needed.
 * Not built ("masks"): masks on the fp16-filter (K8) and FP4 (K11) matrix-core sweeps (the float32 route and binary banks take
 *   the vector-ALU kernels for every k), masked crossCheck, masked radiusMatch, masked ratio / mutual-ratio / accepted-match
 *   calls, masks in the _each forms.  (Masked radiusMatch has since come, on the matrix cores of all four bank kinds: "Masked
 *   radiusMatch" below.)                                                                                                    */
typedef struct fm_mask fm_mask;
int  fm_mask_create(fm_ctx* ctx, int64_t nq, int64_t nt, fm_mask** mask);
int  fm_mask_create_coll(fm_ctx* ctx, int64_t nq, fm_collection* coll, fm_mask** mask);
int  fm_mask_set_u8(fm_ctx* ctx, fm_mask* mask, int32_t img, const uint8_t* rows /*[nq][image rows]*/, int64_t pitch /*0 = dense*/);
int  fm_mask_set_dev(fm_ctx* ctx, fm_mask* mask, int32_t img, const void* d_rows /*device [nq][image rows] bytes*/, int64_t pitch /*0 = dense*/,
                     void* producer_stream /*hipStream_t, NULL = null stream, or FM_NO_STREAM*/);
int  fm_mask_set_all(fm_ctx* ctx, fm_mask* mask, int32_t img, int32_t value);
int  fm_mask_destroy(fm_ctx* ctx, fm_mask* mask);
int  fm_mask_info(const fm_mask* mask, int64_t* nq, int64_t* nt, int32_t* n_images, int64_t* bytes);
int  fm_knn_masked(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, const fm_mask* mask, int32_t k, int32_t* idx /*[nq*k]*/, float* dist /*[nq*k]*/);
int  fm_knn_masked_dev(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, const fm_mask* mask, int32_t k, int32_t* d_idx /*device [nq*k]*/,
                       float* d_dist /*device [nq*k]*/, void* consumer_stream /*hipStream_t or FM_NO_STREAM*/);
int  fm_collection_knn_masked(fm_ctx* ctx, fm_collection* coll, const fm_bank* q, const fm_mask* mask, int32_t k,
                              int32_t* img /*[nq*k]*/, int32_t* idx /*[nq*k]*/, float* dist /*[nq*k]*/);
int  fm_collection_knn_masked_dev(fm_ctx* ctx, fm_collection* coll, const fm_bank* q, const fm_mask* mask, int32_t k,
                                  int32_t* d_img /*device [nq*k]*/, int32_t* d_idx /*device [nq*k]*/, float* d_dist /*device [nq*k]*/,
                                  void* consumer_stream /*hipStream_t or FM_NO_STREAM*/);

/* ---- Wide knnMatch masks: knnMatch(q, t, k, mask) on wide float banks (K14 under a mask, csrc/wide_masked.hip) ---------------
 * fm_knn_masked(_dev) above keep refusing wide float banks (FM_BANK_F32W, 129 .. 256 values per row: FM_EUNSUPPORTED with a
 * message that says "wide"); these two calls serve them, with fm_knn_masked's and fm_knn_masked_dev's argument lists word for
 * word.  Guided matching of learned descriptors: a window round a predicted position, an epipolar band from a pose prior.
 * The mask is fm_mask_create(ctx, nq, nt, &mask)'s, unchanged: its geometry does not depend on the bank kind (a wide bank's
 * padded row count is pad128(n) like every bank's).
 * Contract: row i's list is the list fm_knn(q, t, k) gives for the wide pair, computed over the PERMITTED train rows of row i
 *   only.  The distances are the same bits -- K14's chain: sqrtf(s), s = fmaf(v_k, v_k, s), k ascending over the real dim.
 *   Order: (float32 distance bits, train index), strictly; the lowest permitted index wins a tie.  -1 / +inf where fewer than k
 *   rows are permitted.  A NaN or +inf distance is never listed.  An all-ones mask reproduces fm_knn bit for bit.  nq = 0,
 *   nt = 0 and an all-zero mask are valid.  k = 1, 2; k >= 3 is FM_EUNSUPPORTED, as fm_knn answers for wide banks; k < 1 is
 *   FM_EINVAL.  No option changes a result.
 * Errors, in this order: (1) NULL handles (ctx, banks, mask): FM_EINVAL; (2) a bank that is not FM_BANK_F32W: FM_EINVAL, even
 *   when it is empty, with a message that names fm_knn_masked as the call that serves it; dims that differ: FM_EINVAL; (3) k;
 *   (4) the mask checks of fm_knn_masked, FM_EINVAL with a message that says which: a mask of another context, a mask whose nq
 *   differs from the query bank's rows or whose train rows differ from the train bank's, a collection's mask; (5) the output
 *   pointers: fm_knn_masked's check for the host form (NULL with nq > 0), fm_knn_dev's pointer checks for the device form.
 * Streams and accounting: the device form orders itself against consumer_stream in both directions as fm_knn_masked_dev does
 *   and is not accounted in fm_stats; the host form is accounted like fm_knn_masked (pairs = nq * real train rows).
 *   fm_f32_filter_stats counts one launch per filtered call and one fallback per call that is redone.
 * Routes ("f32_filter" 0 / 1 / 2 and "f32_nsplit" as for every wide sweep): the masked fp16 filter on the MATRIX CORES
 *   (v_mfma_f32_16x16x32_f16, K14's filter shape) for calls of 4e6 pairs or more ("f32_filter" 2: always) on banks the filter
 *   can take, then K14's exact rescoring of the recorded pairs; a lane reads the 16 mask bits of its output row and a 16-row
 *   tile from one 8-byte word per four tiles, a forbidden pair is dropped by INDEX before it can enter a bound, and a wave
 *   skips the matrix instructions -- and the operand fetch -- of a tile in which it has no permitted pair.  Everything else,
 *   and a call whose record list overflowed (2^20 records at least; the call is redone: the fallback), takes the masked exact
 *   kernel: K14's exact tiling on the vector ALUs with one mask bit tested per candidate.
 * Not built: masks in the wide mutual-ratio, ratio, self-distance, radius and collection calls (fm_mutual_ratio, fm_knn2_ratio,
 *   fm_wide_self_dist, fm_wide_match_*, fm_wide_radius_match, fm_collection_wide_*); k >= 3; a masked K8 filter for 128-D float
 *   banks (fm_knn_masked's float32 route stays on the vector ALUs).                                                        */
int  fm_wide_knn_masked(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, const fm_mask* mask, int32_t k, int32_t* idx /*[nq*k]*/, float* dist /*[nq*k]*/);
int  fm_wide_knn_masked_dev(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, const fm_mask* mask, int32_t k, int32_t* d_idx /*device [nq*k]*/,
                            float* d_dist /*device [nq*k]*/, void* consumer_stream /*hipStream_t or FM_NO_STREAM*/);

/* ---- Masked radiusMatch: radiusMatch(q, t, maxDistance, mask) on all four bank kinds (K10 under a mask, csrc/radius.hip) ------
 * cv2.BFMatcher.radiusMatch takes a mask as knnMatch and match do (recalled, not verified, like the mask rules above).
 * Guided matching: every database row within r of a descriptor AMONG the rows inside a window round a predicted position or
 * inside an epipolar band -- without sweeping, sorting and reading back the forbidden rows first.
 * The existing radius calls (fm_radius_match, fm_hamming_radius_match, fm_wide_radius_match, their _dev and collection forms)
 * keep every refusal they have.  The four calls here are new names and dispatch on the bank kind; each argument list is its
 * unmasked namesake's with `const fm_mask* mask` behind the train operand:
 *   fm_radius_match_masked(_dev): FM_BANK_I8 pairs, float32-route pairs, FM_BANK_BIN pairs (distance and radius rules of
 *     fm_hamming_radius_match) and FM_BANK_F32W pairs (those of fm_wide_radius_match); the mask is fm_mask_create's.
 *   fm_collection_radius_match_masked(_dev): integer, float32 and binary collections; the mask is fm_mask_create_coll's.  A wide
 *     collection is FM_EUNSUPPORTED with a message that says "wide" (fm_mask_create_coll keeps refusing one: no such mask exists).
 * Contract: row i's list is the list the unmasked call returns for the same operands and radii with every entry whose pair
 *   (i, train row) is forbidden removed -- nothing else changes.  The distance bits, the strict float32 compare dist < r and
 *   the order (distance bits, train index) -- a collection: (bits, img, row) -- are the unmasked call's.  r <= 0 or NaN: an
 *   empty list; r = +inf: every permitted real row.  offsets, cap (cap = 0: counts only; the longest prefix of whole rows is
 *   written) and *n_total follow fm_radius_match's rules unchanged.  An all-ones mask reproduces the unmasked call bit for bit,
 *   an all-zero mask gives all-zero offsets.  nq = 0 and nt = 0 are valid.  No option changes a result; "radius_ws_bytes" keeps
 *   its meaning (24 bytes per candidate, 28 against a collection -- of the PERMITTED candidates only).  A train bank that grew by
 *   appends never lists a gap row, whatever the mask says.
 * Errors, in this order: (1) NULL handles (ctx, banks / collection, mask): FM_EINVAL; (2) the pair's rules -- width or kind
 *   mismatch, a binary or wide bank against one that is not: FM_EINVAL -- or fm_collection_radius_match's for the collection
 *   forms (a wide collection or a wide query bank: FM_EUNSUPPORTED; a query bank not of the collection's kind: FM_EINVAL);
 *   (3) the mask checks of fm_knn_masked, FM_EINVAL with a message that says which: a mask of another context, a mask whose nq
 *   differs from the query bank's rows or whose train rows differ from the train bank's, a pair mask given to a collection form
 *   and the reverse, a mask of another collection, a collection that has changed (add or clear) since fm_mask_create_coll;
 *   (4) cap < 0, offsets NULL, idx / dist (img) NULL with cap > 0: FM_EINVAL; the _dev forms: fm_radius_match_dev's
 *   device-pointer checks.  A refused call writes nothing.
 * Streams and accounting: the device forms follow fm_radius_match_dev -- radii read in place, offsets and lists written to the
 *   caller's device arrays, ordered against consumer_stream in both directions, not accounted in fm_stats; the host forms are
 *   accounted like fm_radius_match (pairs = nq * real train rows, whatever the mask permits).
 * Kernels: the four threshold sweeps of K10 in MASKED instantiations (the mask is a compile-time parameter; the unmasked
 *   kernels are the code they were): v_mfma_i32_16x16x64_i8, v_mfma_f32_16x16x32_f16 (128-D and wide) and the FP4
 *   v_mfma_scale_f32_16x16x128_f8f6f4.  Per query row and 64-row stage a lane reads one 8-byte mask word, one stage ahead of its
 *   use, and ANDs its 16 bits into the sweep's hit bits in front of the count and in front of the key writes -- the count pass
 *   and the fill pass read the same words.  A wave whose rows permit nothing in a stage skips the stage's operand reads from LDS
 *   and its MFMAs (per block of 16 query rows too); it still takes part in the stage's load and barriers.  The float32
 *   route's `all` path (every pair a candidate) takes the mask as well; the rescoring kernels only ever see permitted pairs.
 * Not built: masks on a wide collection; masked crossCheck, ratio, mutual-ratio and accepted-match calls; compactResult in the
 *   C ABI (the Python BFMatcher drops the rows itself); a skip of the whole workgroup's stage load, or of the wide sweep's
 *   streamed operand fetch, where every row forbids a stage.                                                                  */
int  fm_radius_match_masked(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, const fm_mask* mask, const float* radius /*[nq] or NULL*/,
                            float radius_all, int64_t cap, int64_t* offsets /*[nq+1]*/, int32_t* idx, float* dist, int64_t* n_total);
int  fm_radius_match_masked_dev(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, const fm_mask* mask,
                                const float* d_radius /*device [nq] or NULL*/, float radius_all, int64_t cap,
                                int64_t* d_offsets /*device [nq+1]*/, int32_t* d_idx, float* d_dist, int64_t* n_total /*host, or NULL*/,
                                void* consumer_stream /*hipStream_t or FM_NO_STREAM*/);
int  fm_collection_radius_match_masked(fm_ctx* ctx, fm_collection* coll, const fm_bank* q, const fm_mask* mask,
                                       const float* radius /*[nq] or NULL*/, float radius_all, int64_t cap, int64_t* offsets /*[nq+1]*/,
                                       int32_t* img, int32_t* idx, float* dist, int64_t* n_total);
int  fm_collection_radius_match_masked_dev(fm_ctx* ctx, fm_collection* coll, const fm_bank* q, const fm_mask* mask,
                                           const float* d_radius /*device [nq] or NULL*/, float radius_all, int64_t cap,
                                           int64_t* d_offsets /*device [nq+1]*/, int32_t* d_img, int32_t* d_idx, float* d_dist,
                                           int64_t* n_total /*host, or NULL*/, void* consumer_stream /*hipStream_t or FM_NO_STREAM*/);

/* ---- Wide stacked knnMatch: a wide query against ALL images of a wide collection at once (K14 over the stack, csrc/wide_stack.hip) --
 * cv2.BFMatcher.add(images) followed by knnMatch(query, k) for wide float descriptors (FM_BANK_F32W, 129 .. 256 values per row):
 * "which image of my database does this query row match", every hit carrying imgIdx -- retrieval with 256-D learned
 * descriptors: 2-NN over the whole database, Lowe's ratio against the whole database, votes per image.
 * fm_collection_knn(_dev), fm_collection_knn2_ratio(_dev) and fm_collection_votes keep refusing a wide collection and a wide
 * query bank exactly as before; the five calls here, with the argument lists of their L2 namesakes word for word, are the
 * ones that serve them: fm_collection_wide_knn, fm_collection_wide_knn_dev, fm_collection_wide_knn2_ratio,
 * fm_collection_wide_knn2_ratio_dev, fm_collection_wide_votes.
 * Contract.  Let T be the real rows of the images concatenated in image order.
 *   fm_collection_wide_knn(q, coll, k) equals fm_knn(q, bank(T), k) bit for bit, every entry reported as (img, row inside the
 *   image).  The distances are K14's chain: sqrtf(s), s = fmaf(v_k, v_k, s), k ascending over the real dim.  Lists ascend
 *   strictly by (distance bits, img, row).  Where the collection has fewer than k real rows the entry is -1 / -1 / +inf; a NaN
 *   or +inf distance is never listed.  k = 1, 2; k >= 3 is FM_EUNSUPPORTED, as fm_knn answers for wide banks; k < 1 is
 *   FM_EINVAL.
 *   fm_collection_wide_knn2_ratio follows fm_collection_knn2_ratio's rules on that list: float64 d0 / d1 < tau, d1 == 0
 *   rejected, ascending query index, cap, the full count in *n_accepted (the _dev form: 16-byte rows {query, image, row inside
 *   the image, float32 distance bits}, *d_count the rows that are there).
 *   fm_collection_wide_votes mode 0 is the same test counted at the first neighbour's image; mode 1 is the per-image ratio
 *   test on the lists behind fm_collection_wide_knn2_each (which stay on the device), counted per image.
 *   Empty images keep their index.  A collection on which no add has succeeded is valid, and so are nq = 0 and a collection of
 *   empty images only.  No option changes a result.  The stack's fp16 scale and largest scaled squared norm are read at the
 *   call: a later add may rewrite them.
 * Routes ("f32_filter" 0 / 1 / 2 and "f32_nsplit" as for every wide sweep): ONE sweep over the whole physical stack.  The
 *   stack has zero-filled padding rows behind EVERY image (each starts on a 128-row stage), which a bank-pair kernel -- it
 *   drops padding by index at a bank's end only -- would take for near neighbours (distance |q|: 1.0 for unit-norm rows, nearer
 *   than almost every real row); so the kernels here read the collection's per-stage table of real rows: a reduced row is real
 *   iff (row & 127) < real_rows[row >> 7], one uniform table read per 16-row tile, and a padding row leaves by INDEX before it
 *   can enter a list, a bound or a record.  The fp16 filter on the MATRIX CORES (v_mfma_f32_16x16x32_f16, K14's filter shape;
 *   a tile without a real row skips its matrix instructions and its operand fetch) for calls of 4e6 real pairs or more
 *   ("f32_filter" 2: always) on operands the filter can take, then K14's exact rescoring of the recorded pairs; everything
 *   else -- "f32_filter" 0, a value on either side that is not finite, scale exponents more than 8 apart -- and a call whose
 *   record list overflowed (256 records per query row, 2^20 at least; the call is redone: the fallback) takes the exact
 *   kernel, K14's tiling on the vector ALUs with the same table test.  fm_f32_filter_stats counts one launch per filtered call
 *   and one fallback per call that is redone.  The merge writes (img, row inside the image, distance); the ratio test, the
 *   compaction and the votes behind it are those of the L2 namesakes.
 * Errors, in this order: (1) NULL handles, or a collection of another context: FM_EINVAL; (2) a query that is not FM_BANK_F32W
 *   (even when it is empty: the wide creators make an empty bank wide), or a non-empty collection that is not wide: FM_EINVAL,
 *   with a message that names the L2-named call that serves it (which serves the binary, Hamming, kind too); (3) widths that
 *   differ: FM_EINVAL; (4) k, or for the votes the mode (FM_EINVAL unless 0 or 1); (5) the output pointers: the host forms check
 *   NULL with nq > 0 (votes: with n_images > 0), the _dev forms use fm_collection_knn_dev's and
 *   fm_collection_knn2_ratio_dev's pointer checks.
 * Streams and accounting: the _dev forms order themselves against consumer_stream in both directions, like their namesakes,
 *   and are not accounted in fm_stats; the host forms add nq * real rows pairs (votes mode 1: nq * real rows as well, image by
 *   image).
 * Not built: k >= 3; masks on a wide collection (fm_mask_create_coll keeps refusing it); fm_collection_wide_xcheck1_each; a
 *   stacked sweep shared by several query banks.                                                                          */
int  fm_collection_wide_knn(fm_ctx* ctx, fm_collection* coll, const fm_bank* q, int32_t k,
                            int32_t* img /*[nq*k]*/, int32_t* idx /*[nq*k]*/, float* dist /*[nq*k]*/);
int  fm_collection_wide_knn_dev(fm_ctx* ctx, fm_collection* coll, const fm_bank* q, int32_t k, int32_t* d_img /*device [nq*k]*/,
                                int32_t* d_idx /*device [nq*k]*/, float* d_dist /*device [nq*k]*/, void* consumer_stream /*hipStream_t or FM_NO_STREAM*/);
int  fm_collection_wide_knn2_ratio(fm_ctx* ctx, fm_collection* coll, const fm_bank* q, double tau, int64_t cap,
                                   int32_t* qidx, int32_t* img, int32_t* tidx, float* dist, double* ratio, int64_t* n_accepted);
int  fm_collection_wide_knn2_ratio_dev(fm_ctx* ctx, fm_collection* coll, const fm_bank* q, double tau, int64_t cap,
                                       int32_t* d_rows /*device [cap][4]*/, int64_t* d_count /*device*/, int64_t* n_accepted /*host, or NULL*/,
                                       void* consumer_stream /*hipStream_t or FM_NO_STREAM*/);
int  fm_collection_wide_votes(fm_ctx* ctx, fm_collection* coll, const fm_bank* q, double tau, int32_t mode,
                              int64_t* votes /*[n_images]*/);

/* Classic Ratio-Match in one call: knnMatch(q, t, k=2) then ratio = m[0].distance /
 * m[1].distance (float64) and ratio < tau  -- Classic Matching.ipynb cell 3 (JSON 59-72), the
 * baseline Fast-Match is compared against (README.md:5-13).  Returns the accepted matches
 * compacted in ascending query index: qidx/tidx/dist (= d1)/ratio[0 .. min(*n_accepted, cap)).
 * A zero second distance (where the notebook's Python division raises) is rejected.       */
int  fm_knn2_ratio(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, double tau, int64_t cap,
                   int32_t* qidx, int32_t* tidx, float* dist, double* ratio, int64_t* n_accepted);

/* Mutual nearest neighbours that also pass the ratio test, in one call: what most pipelines with a GPU extractor run -- hloc's
 * "NN-ratio + mutual", kornia's match_smnn, the cv2 loop knnMatch(k = 2) + ratio + crossCheck.  With K2 = fm_knn2(q, t) and R2 =
 * fm_knn2(t, q) (the two nearest QUERY rows of every train row; both ordered by (float32 distance bits, index), the float32-root
 * repair of the integer route included), query row i with (t0, d0), (t1, d1) = K2[i] is accepted iff
 *   1. forward ratio: t1 >= 0 and (double)d0 / (double)d1 < tau -- fm_knn2_ratio's rule (a missing second neighbour or 0 / 0
 *      is rejected; tau = +inf keeps every row whose ratio is a number);
 *   2. mutual: R2[t0][0] == i -- the nearest query row of t0 is i, the lowest query index winning a tie;
 *   3. symmetric != 0 only, reverse ratio: with (q0', e0), (q1', e1) = R2[t0], q1' >= 0 and (double)e0 / (double)e1 < tau (a
 *      query bank of one row accepts nothing in symmetric mode).
 * The accepted rows come out in ascending query index as qidx, tidx = t0, dist = d0; ratio = the forward ratio, in symmetric
 * mode the larger of the two (ratio < tau either way); *n_accepted = the full count, rows written = min(count, cap); cap = 0:
 * the count only (the row arrays may be NULL).  All three bank kinds; nq = 0 and nt = 0 are valid and accept nothing.  Argument
 * checks are fm_knn2_ratio's, in its order (a binary bank paired with a non-binary one: FM_EINVAL).
 * ONE full sweep, where fm_knn2_ratio + fm_xcheck1 take two: the mutual test is only needed for the train rows that are the
 * first neighbour of a query row that already passed the ratio test.  Those rows are gathered into a workspace bank G (every
 * plane the sweeps read on the output side, padded to whole 128-row stages; duplicates where two query rows share a first
 * neighbour) and R2 is fm_knn2(G, q): a sweep of n_cand x nq pairs.  The candidate count is read back between the two sweeps:
 * the call's host wait.  fm_stats: pairs grows by nq * nt + n_cand * nq.
 * fm_mutual_ratio_dev: the accepted rows in caller DEVICE memory, word for word as fm_knn2_ratio_dev leaves them -- 12-byte rows
 * {query, train, float32 distance bits}, *d_count = min(accepted, cap), *n_accepted (host, may be NULL) the full count; pointer
 * checks and stream ordering are fm_knn2_ratio_dev's.  Host synchronisation: ONE on every route, the 8-byte candidate count
 * (and the one n_accepted != NULL asks for, as in fm_knn2_ratio_dev).  Not accounted in fm_stats.                            */
int  fm_mutual_ratio(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, double tau, int32_t symmetric, int64_t cap,
                     int32_t* qidx, int32_t* tidx, float* dist, double* ratio, int64_t* n_accepted);
int  fm_mutual_ratio_dev(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, double tau, int32_t symmetric, int64_t cap,
                         int32_t* d_rows /*device [cap][3]*/, int64_t* d_count /*device*/, int64_t* n_accepted /*host, or NULL*/,
                         void* consumer_stream /*hipStream_t or FM_NO_STREAM*/);

/* Replaces bf_match(d, d, k=2) + [r[1].distance] (cache.pyx:250-252; exact substitute
 * for the approximate flann_match at cache.pyx:271-273).  selfdist[i] = distance from
 * row i to its 2nd entry of the self 2-NN list, as float64 of the float32 value (+inf for a bank of one row).
 * That entry's distance is min over j != i of d(i, j): row i itself is at 0, always the first entry unless a
 * duplicate with a lower index is, and then i (or another duplicate) is the second at 0 = that minimum; only the
 * VALUE is kept, so its order among ties does not matter.  Computed as such: a top-1 sweep of the bank over
 * itself with the diagonal masked (K1's top-1 kernel, not the top-2 one).  r05: integer banks of >= 32768 rows
 * take the TRIANGULAR sweep (option "self_tri"): d(i, j) = d(j, i), so every 16 x 16 tile above the diagonal is
 * computed once and used for both of its rows' minima (rowreduce.hip, "TRI"); same values, bit for bit.        */
int  fm_self_dist(fm_ctx* ctx, const fm_bank* bank, double* selfdist /*[n]*/);
/* HOST code, no context: the workgroups of that triangular sweep for a bank padded to n_pad rows (a multiple of 128)
 * (the kernel itself holds no table: it derives workgroup i by the same arithmetic, rowreduce.hip tri_entry)
 * -- table[4 i .. 4 i + 3] = (output chunk of 512 rows, first 128-row stage, end stage, 0) of workgroup i, the first
 * *n_diag of them the diagonal blocks (launch A), the rest launch B; stages == 0 lets the library choose the piece
 * length (returned in *stages_used).  Writes min(cap, *n_workgroups) entries.  Every (chunk k, stage >= 4 k) is
 * covered exactly once: tests/test_tri_plan.py.                                                                  */
int  fm_self_dist_plan(int64_t n_pad, int32_t stages, int32_t* table /*[cap][4]*/, int64_t cap, int32_t* n_workgroups,
                       int32_t* n_diag, int32_t* stages_used);
/* The Metric_Cache builds of n images in one call: self distances of every bank, ATTACHED to it on the device
 * (as fm_bank_set_selfdist would, without the trip through the host); consecutive integer-route banks -- of any
 * sizes (r05) -- share the triangular sweep's two launches, up to "batch_group" banks each: a dataset of small
 * images builds its caches 2 - 3.7 x faster this way than bank by bank.  out == NULL (or every out[i] NULL):
 * enqueue only, complete after fm_sync / fm_wait; otherwise out[i] (may be NULL per bank) also receives bank i's
 * values and the call is synchronous.  A bank must not be read by work still in flight (see fm_bank_refill).  */
int  fm_self_dist_batch(fm_ctx* ctx, int32_t n, fm_bank* const* banks, double* const* out /*[n] of [n_i], or NULL*/);

/* ---- X1: cross-checked 1-NN ----------------------------------------------------------
 * Replaces cv2.BFMatcher(cv2.NORM_L2, crossCheck=True).knnMatch(q, t, k=1)
 *   fastmatch.pyx:122-123 (match_thumbs) and fastmatch.pyx:161-162 (match_position).
 * tidx[i] = train index matched to query row i or -1 (empty inner list), dist[i] its
 * float32 distance (+inf when unmatched).  OpenCV semantics: reverse-NN + scatter-min
 * with lowest-index tie-breaks.                                */
int  fm_xcheck1(fm_ctx* ctx, const fm_bank* q, const fm_bank* t,
                int32_t* tidx /*[nq]*/, float* dist /*[nq]*/);

/* X1 up to the election, for a train set sharded over ranks (one process per GPU): keys[q] =
 * (distance key << 32) | (t_offset + train row in this bank) of the closest row of THIS bank
 * that elects q, ~0 if none; distance key = the float32 bits of the distance on both routes
 * (cv::batchDistance takes the square root BEFORE it compares, and two integer d^2 >= 4 197 200
 * can share one float32 root: the order of the roots, not of d^2, is OpenCV's).  The element-wise
 * minimum over the ranks
 * (one all-reduce(min) of nq words) equals the keys of the unsharded fm_xcheck1: same
 * matches, same tie-breaks (cv::BFMatcher cross-check, fastmatch.pyx:122-123, 161-162).   */
int  fm_xcheck1_keys(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, int64_t t_offset, uint64_t* keys);
/* The same with the keys left in caller-supplied DEVICE memory (uint64[nq]): the operand of the
 * all-reduce(min) over the ranks, so the keys of a shard never visit the host.                 */
int  fm_xcheck1_keys_dev(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, int64_t t_offset, uint64_t* d_keys);

/* ---- R1: ratio + threshold -----------------------------------------------------------
 * Replaces  ratios = m.distance / query_dis[m.queryIdx]   (fastmatch.pyx:124, 165)
 *      and  ratios < tau                                   (fastmatch.pyx:50, 75, 82)
 * in float64 on the device.  qrows == NULL means row i uses selfdist[i].
 * ratio and pass may each be NULL.                                                      */
int  fm_ratio_filter(fm_ctx* ctx, const float* dist, const double* selfdist,
                     const int32_t* qrows, int64_t n, double tau,
                     double* ratio /*[n] or NULL*/, uint8_t* pass /*[n] or NULL*/,
                     int64_t* n_pass /*or NULL*/);

/* X1 + R1 fused on the device for banks that stay resident (one match_position /
 * match_thumbs round: fastmatch.pyx:161-165, 122-124).  q must carry self distances
 * (fm_bank_set_selfdist).  Outputs as fm_xcheck1 plus ratio[i] (nan when unmatched)
 * and pass[i] = ratio[i] < tau; *n_pass = number of accepted matches.                   */
int  fm_match_ratio(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, double tau,
                    int32_t* tidx /*[nq]*/, float* dist /*[nq]*/,
                    double* ratio /*[nq] or NULL*/, uint8_t* pass /*[nq] or NULL*/,
                    int64_t* n_pass /*or NULL*/);

/* As fm_match_ratio, but returns only the accepted matches (ratio < tau), compacted on the
 * device in ascending query index: qidx/tidx/dist/ratio[0 .. min(*n_accepted, cap)).
 * *n_accepted is the total number accepted (may exceed cap; the rest is dropped).        */
int  fm_match_accepted(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, double tau, int64_t cap,
                       int32_t* qidx, int32_t* tidx, float* dist, double* ratio,
                       int64_t* n_accepted);

/* As fm_match_accepted, but the call only ENQUEUES the work on the context's stream and returns:
 * the results are valid after the next fm_sync(ctx) (or any synchronous call on the context).
 * Every output -- qidx, tidx, dist, ratio and *n_accepted -- must be page-locked host memory
 * (fm_host_alloc), which the compaction kernel writes directly; banks must be integer valued.
 * A stream of image pairs then runs back to back on the GPU with no host round
 * trip between pairs (the reference maps its matcher over pairs sequentially, turntable.py:59):
 * the K1 launches follow each other on the context's stream while each pair's small kernels
 * (election, ratio test, compaction) run on a second stream beside the next pair's K1.          */
int  fm_match_accepted_async(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, double tau, int64_t cap,
                             int32_t* qidx, int32_t* tidx, float* dist, double* ratio,
                             int64_t* n_accepted /*page-locked*/);

/* Completion points for the enqueue-only calls.  fm_mark remembers everything enqueued on the context
 * so far and returns a ticket; fm_wait(ticket) blocks until that work is complete, while work enqueued
 * after the mark keeps running -- the results of batch i can be consumed while batch i + 1 computes
 * (double-buffered outputs).  fm_sync waits for everything.  Tickets are valid for the next 8 marks.  */
int  fm_mark(fm_ctx* ctx, int64_t* ticket);
int  fm_wait(fm_ctx* ctx, int64_t ticket);

/* n independent image pairs in one call, enqueued like n fm_match_accepted_async calls (same output
 * rules: every qidx[i] / tidx[i] / dist[i] / ratio[i] / n_accepted[i] page-locked, results valid after
 * fm_sync).  Consecutive pairs go through the distance kernel TOGETHER, up to eight pairs per launch (option
 * "batch_group": up to sixteen) -- r05: of ANY sizes (a dataset's images all differ; before, only pairs of equal padded sizes
 * shared a launch and the others cost 7 % more per descriptor pair), small ones included (a pair whose train bank has fewer than
 * 32768 rows is planned with 4-wave workgroups when it runs alone; inside a batch it is planned again in the batched kernel's
 * 8-wave shape, the other pairs fill the chip): inside one launch the
 * workgroups of the next pair fill the CUs the previous pair leaves, where separate launches drain the chip and pay a launch gap (~4 % of
 * a 100k x 100k pair).  The reference maps its matcher over the pairs of a dataset one after the
 * other (turntable.py:59); this is that loop as one call.  Pairs that cannot be grouped (an empty bank, a query
 * bank without self distances, an option that forces another kernel shape) are enqueued one by one; pairs on the float32 route, which has no enqueue-only form,
 * run synchronously in their place (their outputs are complete when the call returns, the pairs around
 * them stay asynchronous).  Every pair is validated before anything is enqueued.  A run of pairs ends with
 * a short launch (2 pairs) because only the LAST launch's small kernels are exposed to a caller that
 * synchronises after the call; a caller that enqueues the next batch first (fm_mark / fm_wait) sets the
 * options batch_tail = 0 and batch_group = 16 (fm_ctx_set_option) for one launch per run.              */
int  fm_match_accepted_batch(fm_ctx* ctx, int32_t n, const fm_bank* const* q, const fm_bank* const* t, double tau,
                             int64_t cap, int32_t* const* qidx, int32_t* const* tidx, float* const* dist,
                             double* const* ratio, int64_t* const* n_accepted /*page-locked words*/);

/* fm_match_accepted_batch with the results left on the device, as fm_match_accepted_dev_async leaves
 * them: pair i's rows at d_rows + i * cap * 3 (int32 [n][cap][3]), its count at d_counts[i] (and in the
 * page-locked word h_counts[i] if h_counts is not NULL).  One contiguous block per call, so the caller
 * ships a whole step with ONE all-gather of n * cap rows.  consumer_stream as in
 * fm_match_accepted_dev_async: ordered against the fills in both directions.                     */
int  fm_match_accepted_dev_batch(fm_ctx* ctx, int32_t n, const fm_bank* const* q, const fm_bank* const* t, double tau,
                                 int64_t cap, int32_t* d_rows /*device [n][cap][3]*/, int64_t* d_counts /*device [n]*/,
                                 int64_t* h_counts /*page-locked [n] or NULL*/, void* consumer_stream /*hipStream_t or FM_NO_STREAM*/);

/* As fm_match_accepted, but the accepted matches stay on the device: d_rows[i] = {query index,
 * train index, float32 distance bits} (12-byte rows, ascending query index, at most cap of
 * them) and *d_count = the number of rows written = min(accepted, cap), both in caller-supplied DEVICE
 * memory (n_accepted / h_count on the host receive the full number of accepted matches) -- the send
 * buffer of the multi-GPU result gather (fm_gather_matches / an RCCL all-gather), so nothing
 * bounces through the host.  The reference has no counterpart (single process); the rows are
 * the (queryIdx, trainIdx, distance) of the DMatch list fastmatch.pyx:161-165 consumes.
 * Synchronous: the buffers are complete on return.  n_accepted (host) may be NULL.          */
int  fm_match_accepted_dev(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, double tau, int64_t cap,
                           int32_t* d_rows /*device [cap][3]*/, int64_t* d_count /*device*/,
                           int64_t* n_accepted /*host, or NULL*/);

/* fm_match_accepted_dev without the synchronisation: the call enqueues and returns.  The match
 * kernel (K1) goes to the context's stream, the small kernels behind it (election, ratio test,
 * compaction into d_rows / d_count) to a second stream, where they overlap the NEXT pair's K1.
 * consumer_stream is the stream that will read d_rows / d_count -- the stream the caller's all-gather
 * is enqueued on; NULL is the null stream (PyTorch's default stream), FM_NO_STREAM means none: the compaction first waits for the work that
 * stream has been given so far (the collective that last read these buffers), and the stream is
 * made to wait for the compaction, so the caller needs no host synchronisation between pairs.
 * h_count: page-locked host word (fm_host_alloc) that also receives the count, or NULL.
 * Integer-valued banks only.  fm_gather_matches called next follows the same ordering.         */
int  fm_match_accepted_dev_async(fm_ctx* ctx, const fm_bank* q, const fm_bank* t, double tau, int64_t cap,
                                 int32_t* d_rows /*device [cap][3]*/, int64_t* d_count /*device*/,
                                 int64_t* h_count /*page-locked or NULL*/, void* consumer_stream /*hipStream_t or FM_NO_STREAM*/);

/* ---- K4: many match_position rounds in one launch ------------------------------------
 * Round b matches the query rows  q_rows[q_off[b] .. q_off[b+1])  of bank q (the radius
 * subset Metric_Cache.get returns, cache.pyx:173-188, in its order) against the train
 * rows [t_off[b], t_off[b+1]) of bank t (cells of a Grid_Cache packed back to back).
 * Output is per query slot i in [0, q_off[B]):  tidx[i] = train row index LOCAL to the
 * round's cell (-1 = none), dist[i], and ratio[i] = dist / selfdist[q_rows[i]] when q
 * carries self distances (else nan).  Semantics per round are exactly fm_xcheck1 on the
 * gathered sub-matrices.  Both routes: integer-valued banks run the int8 round; float32 banks
 * the float32 round (fp16 MFMA filter + exact float32 chain, bit-identical to fm_xcheck1); a
 * float32 round that cannot be completed on the device reports tidx = -2 for all its slots
 * (redo it with fm_xcheck1 on gathered banks).  At most 4096 query rows per round.        */
int  fm_xcheck1_batched(fm_ctx* ctx, const fm_bank* q, const int32_t* q_rows,
                        const int64_t* q_off /*[B+1]*/, const fm_bank* t,
                        const int64_t* t_off /*[B+1]*/, int64_t n_rounds,
                        int32_t* tidx, float* dist, double* ratio /*or NULL*/);

/* ---- K7: device-resident expansion loop ------------------------------------------------
 * Replaces the whole of do_iter + get_neighbors + match_position (fastmatch.pyx:56-103,
 * 145-169) for an image pair whose features are all known up front: the query bank with its
 * keypoint positions and position index (Metric_Cache.original, cache.pyx:278-284) and
 * every Grid_Cache cell's descriptors packed back to back (cache.pyx:124-138).  One
 * persistent workgroup per pair replays the reference's depth-first order exactly; many
 * pairs run concurrently in one launch.  Results come back in discovery order.  The two banks
 * must be of one kind: integer valued (int8 round) or float32 (float32 round).            */
typedef struct fm_expand fm_expand;

typedef struct fm_expand_desc {
    const fm_bank* query;          /* query bank carrying self distances                    */
    const double*  query_pos;      /* [nq][2] keypoint positions (x, y)                     */
    double         index_bucket;   /* uniform-grid position index over query_pos:           */
    double         index_x0, index_y0;   /*   bucket size and origin                         */
    int32_t        index_nbx, index_nby; /*   buckets along x / y                            */
    const int32_t* index_order;    /* [nq] keypoints sorted by bucket (by*nbx + bx)         */
    const int32_t* index_start;    /* [nbx*nby + 1] first entry of each bucket in order[]   */
    const fm_bank* target;         /* all cells' descriptors, cell after cell               */
    const int64_t* cell_off;       /* [cols*rows + 1] row range of cell id = col*rows + row */
    const double*  target_pos;     /* [nt][2] full-image keypoint positions (offset applied)*/
    int32_t        width, height;  /* target image size                                     */
    int32_t        cell_w, cell_h; /* Grid_Cache cell size                                  */
    int32_t        rows, cols;     /* Grid_Cache.rows (cells along x), .cols (along y)      */
    int32_t        margin, radius;
    int64_t        match_cap;      /* first capacity of the result list (0 = 4 * nq) and    */
    int64_t        stack_cap;      /* of the pending stack (0 = default); fm_expand_run     */
                                   /* repeats a run that fills one in a state 4x as large   */
    int32_t        metric;         /* radius query metric: the reference builds its BallTree with
                                    * options["metric"] (cache.pyx:160, 276): FM_METRIC_*    */
    int32_t        lazy;           /* non-zero: LAZY TARGET -- the reference's own mode (cache.pyx:102-106, 124-138: a cell's
                                    * features are computed when the loop first reaches it).  `target` is a bank made with
                                    * fm_bank_create_u8_cap (possibly empty), cell_off / target_pos are ignored; cells are
                                    * added with fm_bank_append_u8 + fm_expand_set_cell and the pair is driven with
                                    * fm_expand_run_lazy.  Integer-route banks, or (r05) float32-route banks:
                                    * target from fm_bank_create_f32_cap, cells added with fm_bank_append_f32.          */
} fm_expand_desc;

#define FM_METRIC_EUCLIDEAN 0      /* "minkowski" (p = 2), "euclidean": dx^2 + dy^2 <= r^2     */
#define FM_METRIC_MANHATTAN 1      /* |dx| + |dy| <= r                                          */
#define FM_METRIC_CHEBYSHEV 2      /* max(|dx|, |dy|) <= r                                      */

#define FM_EXPAND_OK            0
#define FM_EXPAND_STACK_FULL    1
#define FM_EXPAND_SUBSET_FULL   2  /* a radius subset the device could not take.  Integer-route pairs that exceed the first
                                      * kernel's 2048 rows are re-run by fm_expand_run in a 4096-row kernel and then in one that
                                      * takes a subset of ANY size in chunks (options expand_big / expand_huge; float32 pairs go from
                                      * 2048 straight to the chunked kernel; r05: pairs under the float32-root guard and subsets with
                                      * thousands of keypoints at one distance too, and a round may ACCEPT any number); what is left:
                                      * a subset beyond 640 x 2048 rows, or expand_big / expand_huge switched off */
#define FM_EXPAND_OUT_OF_BOUNDS 3  /* a target position outside the image (cache.pyx:56-57) */
#define FM_EXPAND_MATCH_FULL    4  /* 1, 4, 5: reported only when the run state could not grow any further */
#define FM_EXPAND_TABLE_FULL    5
#define FM_EXPAND_LIST_FULL     6  /* float32 round: more candidates inside the fp16 margin than fit  */
#define FM_EXPAND_NEED_CELL     7  /* lazy target: the loop reached a cell that has not been added yet (fm_expand_run_lazy) */
#define FM_EXPAND_LOG_FULL      9  /* the per-round log's arrays filled and could not grow any further (fm_expand_set_log);
                                      * (8 is internal: a round parked for the dense kernels, settled inside the call) */

/* LIFETIME: the pair BORROWS desc->query and desc->target -- device arrays and, for delegated rounds and lazy
 * targets, the banks' host-side descriptors -- so both banks must outlive the fm_expand, and a bank that an fm_expand names
 * must not be refilled (fm_bank_refill_u8_async) while it exists: row counts, cell offsets and the float32-root guard were
 * fixed when the pair was created.  (The Python binding keeps references; a C client keeps the order destroy(pair), then banks.) */
int  fm_expand_create(fm_ctx* ctx, const fm_expand_desc* desc, fm_expand** out);
int  fm_expand_destroy(fm_ctx* ctx, fm_expand* ex);
/* Run n expansions in one launch, one workgroup each.  Run i = (pairs[i], seeds[i], tau[i]): seeds[i] =
 * [n_seeds[i]][2][2] float64 (query_pos, target_pos) in visiting order (fastmatch.pyx:50), tau[i] the
 * ratio threshold.  A pair may appear SEVERAL times -- the reference is driven as pairs x thresholds
 * (turntable.py:59-60: { tau : f(tau) for tau in thresholds } per pair) and the runs of one pair are
 * independent of each other: each gets a run state of its own (pending stack, seen / found tables,
 * result list; created on first use, kept), the k-th appearance of a pair in a launch uses its run
 * slot k.  Per run outputs: number of matches, rounds, descriptor pairs evaluated, and a FM_EXPAND_*
 * status (non-zero = the device gave up; the caller falls back to the host loop).                */
int  fm_expand_run(fm_ctx* ctx, int32_t n, fm_expand* const* pairs, const double* const* seeds,
                   const int64_t* n_seeds, const double* tau, int64_t* n_matches,
                   int64_t* n_rounds, int64_t* n_pairs, int32_t* status);
/* ---- lazy targets: the device loop with cells computed on demand (r04) ---------------------------------------------
 * fastmatch.pyx:154 -> cache.pyx:102-106, 124-138: a grid cell's features are computed (SIFT on the cell's crop) the first
 * time the expansion reaches it, so most cells of a large image are never computed.  With a lazy pair the loop still runs on
 * the device: a round that needs a missing cell parks the loop's state and ends the launch with FM_EXPAND_NEED_CELL; the host
 * computes that cell, appends its descriptors to the target bank, registers it and resumes.
 *   fm_bank_create_u8_cap : a bank with room for `capacity` rows (n of them now, possibly 0).
 *   fm_bank_append_u8     : n more rows at the next multiple of 32 rows (*first_row); FM_EINVAL when the capacity is used up.
 *                           The rows skipped in between ("gap rows") are padding rows INSIDE the bank, below its row count;
 *                           row indices everywhere are the bank's physical rows, gaps included.  A grown bank is meant for
 *                           fm_expand (cells name their own row ranges), and every dense call takes one too:
 *                             as the TRAIN side a gap row is never a neighbour, an elected row or a list entry -- fm_knn2,
 *                             fm_knn (every k), fm_xcheck1(_keys), fm_match_ratio / fm_match_accepted*, fm_knn2_ratio,
 *                             fm_mutual_ratio, fm_radius_match, fm_knn_masked (whatever the mask says about a gap row: an
 *                             fm_mask is made from row counts and cannot know the bank's gaps, the call forbids them),
 *                             fm_self_dist, their _dev forms; the results are those of a fresh bank of the real rows with the
 *                             indices mapped to physical rows, and no entry point refuses a grown bank for its gaps;
 *                             as the QUERY side a gap position is an output row like any other: its slot holds a valid index
 *                             or -1 and is otherwise unspecified (list forms may list it); the real rows' results are
 *                             unaffected, in both directions of a cross-check.
 *                           Wide, binary and collection banks take no appends, as before.
 *   fm_expand_set_cell    : cell (= col * rows + row) := rows [first_row, first_row + n_rows) with their full-image positions;
 *                           n_rows = 0 for a cell without features.
 *   fm_expand_run_lazy    : one run in slot 0, from the start (resume = 0) or from where the last launch parked (resume != 0:
 *                           FM_EINVAL unless that launch ended with FM_EXPAND_NEED_CELL; its seeds are re-used, `seeds` is ignored).
 *                           status 0: done (fm_expand_fetch); FM_EXPAND_NEED_CELL: *need_cell; else the device gave up.
 *                           (Rounds of >= "expand_delegate" descriptor pairs are cross-checked by the dense kernels inside the call.) */
int  fm_bank_create_u8_cap(fm_ctx* ctx, const uint8_t* rows, int64_t n, int dim, int64_t capacity, fm_bank** bank);
int  fm_bank_append_u8(fm_ctx* ctx, fm_bank* bank, const uint8_t* rows, int64_t n, int64_t* first_row);
/* r05, the same for descriptors that are NOT integer valued (RootSIFT-style float32 on a pixel target): an empty float32-route
 * bank with room for `capacity` rows whose fp16 planes use the power-of-two scale of `scale_like` (the query bank the target
 * will be matched against: a growing bank cannot derive a scale from rows it has not seen), and n more rows at the next
 * multiple of 32.  fm_bank_append_f32 returns FM_EUNSUPPORTED -- bank unchanged -- for a value that is not finite or that
 * leaves fp16's range under that scale (more than ~4 x the largest magnitude of scale_like).                              */
int  fm_bank_create_f32_cap(fm_ctx* ctx, int dim, int64_t capacity, const fm_bank* scale_like, fm_bank** bank);
int  fm_bank_append_f32(fm_ctx* ctx, fm_bank* bank, const float* rows, int64_t n, int64_t* first_row);
int  fm_expand_set_cell(fm_ctx* ctx, fm_expand* ex, int32_t cell, int64_t first_row, int64_t n_rows, const double* pos /*[n_rows][2]*/);
int  fm_expand_run_lazy(fm_ctx* ctx, fm_expand* ex, const double* seeds, int64_t n_seeds, double tau, int32_t resume,
                        int64_t* n_matches, int64_t* n_rounds, int64_t* n_pairs, int32_t* status, int32_t* need_cell);

/* ---- pre-extracted targets: all cells of a Grid_Cache at once (r04) -------------------------------------------------
 * The device loop's target bank holds "every cell's descriptors, cell after cell" (fm_expand_desc.target / cell_off /
 * target_pos).  For a target given as pre-extracted features (keypoint positions + descriptors instead of pixels) a
 * cell's features are the keypoints inside the crop Grid_Cache hands its caching function (cache.pyx:128-131: x from
 * row * cell_w - margin, clipped at 0, over cell_w + 2 * margin; same along y) -- a keypoint lands in up to four cells.
 *   fm_grid_pack_cells       : HOST code, no context: cell_off[rows * cols + 1] (cell id = col * rows + row) and *n_rows
 *                              always; when `capacity` >= *n_rows also src_row[n_rows] (the keypoint of every packed row,
 *                              ascending inside a cell) and target_pos[n_rows][2] (crop-local position + the offset
 *                              match_position adds, fastmatch.pyx:157-158).  A caller whose capacity was too small
 *                              reads *n_rows and calls again.
 *   fm_bank_create_u8_gather /
 *   fm_bank_create_f32_gather: a bank whose row i is rows[src_row[i]] -- the n_src descriptors cross PCIe once and are
 *                              gathered by the upload kernel.  FM_EINVAL for an entry outside [0, n_src).  float_route
 *                              as fm_bank_create_f32_route (non-zero: keep the float32 route even if integer valued).  */
int  fm_grid_pack_cells(const double* positions /*[n][2]*/, int64_t n, int32_t width, int32_t height, int32_t cell_w, int32_t cell_h,
                        int32_t rows, int32_t cols, int32_t margin, int64_t capacity, int64_t* cell_off, int64_t* n_rows,
                        int32_t* src_row, double* target_pos);
int  fm_bank_create_u8_gather(fm_ctx* ctx, const uint8_t* rows, int64_t n_src, int dim, const int32_t* src_row, int64_t n, fm_bank** bank);
int  fm_bank_create_f32_gather(fm_ctx* ctx, const float* rows, int64_t n_src, int dim, int float_route, const int32_t* src_row,
                               int64_t n, fm_bank** bank);

/* Memory of the run states: fm_expand_info reports the bytes ONE run state of the pair takes (pending stack, seen /
 * found tables, result arrays: ~210 MB for a 300k-keypoint pair) and how many exist; fm_expand_trim frees the states
 * from slot `keep` (>= 1) on; fm_mem_info is hipMemGetInfo of the context's device.  fm_expand_run creates a state for
 * every run of a launch and keeps it, so a caller that puts pairs x thresholds into one launch (turntable.py:59-60)
 * sizes its launches with these (fastmatch.run_device_loops does) instead of meeting FM_ENOMEM.                    */
int  fm_expand_info(const fm_expand* ex, int64_t* state_bytes, int32_t* n_slots);
int  fm_expand_trim(fm_ctx* ctx, fm_expand* ex, int32_t keep);
int  fm_mem_info(fm_ctx* ctx, int64_t* free_bytes, int64_t* total_bytes);
/* Copy the first n results of the last run in slot 0 of `ex`: query row index, positions [n][2][2]
 * (query x,y then target x,y) and ratio -- the tuples do_iter appends (fastmatch.pyx:86). */
int  fm_expand_fetch(fm_ctx* ctx, const fm_expand* ex, int64_t n, int32_t* index,
                     double* positions, double* ratio);
/* fm_expand_fetch for several runs of one fm_expand_run with a single synchronisation: n[i] results of
 * run slot slot[i] of ex[i] into index[i] / positions[i] / ratio[i] (any of the three arrays of
 * pointers, or single entries, may be NULL).  slot == NULL: slots by appearance, as fm_expand_run
 * assigns them (the k-th entry naming a pair reads its slot k).                                    */
int  fm_expand_fetch_many(fm_ctx* ctx, int32_t n_ex, const fm_expand* const* ex, const int32_t* slot, const int64_t* n,
                          int32_t* const* index, double* const* positions, double* const* ratio);

/* ---- the per-round log on the device (r05) ------------------------------------------------------------------------------
 * options["log"] of fastmatch.match (fastmatch.pyx:46, 79-80): do_iter appends log_round(...) (fastmatch.pyx:172-180) once per
 * processed round -- query_pos, target_pos, Grid_Cache.last, result_pos[ratios < tau], radius, ratios[ratios < tau], margin.
 * With fm_expand_set_log(enable != 0) the runs of the pair (fm_expand_run and fm_expand_run_lazy) record, per processed round
 * in order, rounds[i][0..3] = the popped (query_pos, target_pos) as float64 bit patterns, rounds[i][4] = the cell the round
 * fetched (col * rows + row: Grid_Cache.last is the crop of the most recently COMPUTED cell, cache.pyx:102-106, which the
 * caller derives from the order in which cells first appear), rounds[i][5] = its accepted matches (-1: the cell has no
 * features, -2: no pair passed the cross-check, an empty radius subset included -- in both cases match_position's arrays come
 * from an empty list and have shape (0,), not (0, 2, 2): fastmatch.pyx:155-156, 162-167); and, for every accepted
 * match in the round's order BEFORE the result dedup (fastmatch.pyx:82-86 dedups the matches, not the log), its query row, its
 * row of the (packed / growing) target bank and its float64 ratio.  fm_expand_log_counts gives the sizes of the last run in
 * `slot`, fm_expand_fetch_log copies them (any pointer may be NULL).  The arrays grow fourfold up to 12 times (when
 * there is no memory for larger ones the old ones stand); a run that still overflows ends with FM_EXPAND_LOG_FULL.  enable > 1: on, with `enable` records and
 * `enable` accepted matches as the arrays' FIRST capacity (the defaults: 4 x the grid's cells, 4 x the query's keypoints).  */
int  fm_expand_set_log(fm_ctx* ctx, fm_expand* ex, int32_t enable);
int  fm_expand_log_counts(fm_ctx* ctx, const fm_expand* ex, int32_t slot, int64_t* n_rounds, int64_t* n_entries);
int  fm_expand_fetch_log(fm_ctx* ctx, const fm_expand* ex, int32_t slot, int64_t n_rounds, int64_t n_entries,
                         int64_t* rounds /*[n_rounds][6]*/, int32_t* query_row /*[n_entries]*/, int32_t* target_row /*[n_entries]*/,
                         double* ratio /*[n_entries]*/);

/* ---- result gather across the GPUs of a node (RCCL over xGMI) --------------------------------
 * Independent image pairs are sharded over ranks (one process per GPU, pair i -> rank i mod N);
 * matching needs no communication and the per-pair match lists come back with ONE exchange: an
 * all-gather of every rank's accepted rows and their counts.  The reference is single process
 * (turntable.py:59 maps the matcher over its pairs sequentially); this is the data-parallel axis
 * it implies.  RCCL is bound at run time (dlopen), so a process that never gathers needs none.
 *   fm_comm_unique_id : rank 0 draws the 128-byte id; the launcher hands it to every rank.
 *   fm_comm_init      : collective; binds the context's device and stream to the communicator.
 *   fm_gather_matches : d_rows / d_count as fm_match_accepted_dev leaves them (device memory);
 *                       d_all_rows [nranks][cap][3] int32, d_all_counts [nranks] int64 (device).
 *                       Runs on the context's stream behind the matching kernels; wait != 0
 *                       synchronises before returning, wait == 0 returns at once (fm_sync later).  */
int  fm_comm_unique_id(void* id128);
int  fm_comm_init(fm_ctx* ctx, int nranks, int rank, const void* id128);
int  fm_comm_destroy(fm_ctx* ctx);
int  fm_gather_matches(fm_ctx* ctx, const int32_t* d_rows, const int64_t* d_count, int64_t cap,
                       int32_t* d_all_rows, int64_t* d_all_counts, int wait);
/* Counts first, then only *rows_per_rank = min(cap, max over the ranks of their counts) rows per rank:
 * d_all_rows is laid out [nranks][*rows_per_rank][3].  Ships what is there instead of the padded capacity
 * (xGMI traffic / 3 on the bench's workload) for one host synchronisation between the two collectives;
 * returns when both are done.                                                                          */
int  fm_gather_matches_counted(fm_ctx* ctx, const int32_t* d_rows, const int64_t* d_count, int64_t cap,
                               int32_t* d_all_rows, int64_t* d_all_counts, int64_t* rows_per_rank);

#ifdef __cplusplus
}
#endif
#endif /* FASTMATCH_HIP_H */
