/* gaml_hip_debug.h -- test, tuning and tracing entry points of the DEVELOPMENT build, libgaml_hip_dev.so
 * (gaml_amd/csrc/Makefile: the same sources compiled with -DGAML_HIP_DEV).
 *
 * NOT part of the drop-in boundary (include/gaml_hip.h), and not in the product: libgaml_hip.so exports none of these
 * symbols, carries none of the A/B switches and tuning knobs they set (every knob is compiled in at its default), no
 * kernel instantiation with in-kernel time stamps and no crash hook. These entry points expose intermediate state to
 * the parity tests (tests/) and the tuning tools (tools/); a caller that only wants ProbCalculator::CalcProb never
 * includes this file.
 */
#ifndef GAML_HIP_DEBUG_H_
#define GAML_HIP_DEBUG_H_

#include "gaml_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- PacBio SAM ingestion, piece by piece ------------------------------------------------------ */
/* host-only introspection (no device needed): how one SAM line is parsed
 * ({flags,len,posstart,posend,sstart,send,slen,tstart,tend,edit_dist}) and which DP cells it gets
 * (rows row0.., one column interval per row). Returns the number of rows, <0 on a malformed line. */
/* the banded DP of one SAM line against an explicit target string ("path + '\n' + reverse
 * complement") and read, on the GPU: what AligmentProbability (graph.cc:2175-2297) returns, as a
 * log.  Returns the number of DP rows (<0: error); when band_lo/band_hi hold at least that many
 * entries they receive the column interval per row that the kernel derived from the CIGAR. */
int gaml_hip_debug_sam_logprob(gaml_hip_ctx* ctx, const char* target, int32_t target_len, const char* read, int32_t read_len,
                               const char* sam_line, int64_t sam_len, double mismatch_prob, double* logprob_out,
                               int32_t* band_lo, int32_t* band_hi, int32_t band_cap);
/* host-only: what the DP kernel is given for one SAM line: {n_ops, row_f, col_f, bl, el, max_width}
 * and the run-length CIGAR ((length << 2) | code, 0 = M, 1 = I, 2 = D). Returns n_ops, <0 on a malformed line. */
int gaml_hip_debug_sam_shape(const char* sam_line, int64_t len, int32_t total_len, int32_t* out6, uint32_t* ops, int32_t cap);
int32_t gaml_hip_debug_sam_band(const char* sam_line, int64_t len, int32_t total_len, int32_t* fields10, int32_t* row0,
                                int32_t* lo, int32_t* hi, int32_t cap);

/* ---- host-side half of an evaluation ----------------------------------------------------------- */
/* Host-side half of an evaluation WITHOUT touching the device (works on a host-only context):
 * window registration + alignment of missing windows + window-occurrence lists for `paths`,
 * exactly what gaml_hip_calc_* does before it launches. For tests of the host logic. */
int gaml_hip_debug_prepare(gaml_hip_ctx* ctx, const int32_t* paths, const int64_t* path_offs, int32_t n_paths);
/* occurrence list of the last prepare/evaluation: 5 ints per entry {window id, shift, min_pos,
 * path, rank}; returns the number of entries. */
int64_t gaml_hip_debug_occurrences(gaml_hip_ctx* ctx, int readset, int mate, int32_t* out5, int64_t cap);
/* what the occurrence TABLES of the last prepare/evaluation hold (the host image that the device copy mirrors), as the
 * same 5 ints per entry, path = position of the path in the set, rank = path-local; min_pos as stored (clamped at
 * -32768 in the 8-byte entries). Sorted by (path, rank). For tests of the incremental table maintenance: must describe
 * the same occurrences as gaml_hip_debug_occurrences. info3 (may be NULL): {1 if the last planning was incremental,
 * incremental calls so far, whole-set calls so far}. */
int64_t gaml_hip_debug_table_occurrences(gaml_hip_ctx* ctx, int readset, int mate, int32_t* out5, int64_t cap, int64_t* info3);
/* The coverage bitmap layout of the path set of the last prepare/evaluation of paired set `readset` (penalty_constant > 0): slot_base[slot]
 * = first bit of the region of the path whose table entries carry that slot (what the scoring kernels mark through; 0 for
 * slots not in use), and in the order of the paths in the set path_base[n_paths + 1] (monotone, multiples of 32; a path
 * keeps its length + 64 bits rounded up to words), start_off[n_paths + 1] / starts[] (the contig start coordinates of
 * path k: starts[start_off[k] .. start_off[k + 1]), what the sweep reads) and slots[n_paths]. counts4 (may be NULL) =
 * {slots, paths, contig starts, bits in all}; path_base / start_off need room for cap_paths + 1 entries. Returns the
 * number of paths, -1 when the set has no penalty or nothing was prepared. Works on a host-only context. */
int32_t gaml_hip_debug_cov_layout(gaml_hip_ctx* ctx, int readset, int32_t* slot_base, int32_t cap_slots, int32_t* path_base, int32_t* start_off,
                                  int32_t* slots, int32_t cap_paths, int32_t* starts, int32_t cap_starts, int32_t* counts4);
/* The same of region g of the last pass of a gap profile that took the device route (gaml_hip_gap_profile with
 * gaml_hip_set_gap_penalty_device on): what gap_tables_kernel derived for the g-th length of that pass, copied back from the
 * arena; counts4[3] is the total the host sized that length's bitmap and sweep with. Arguments and format as above. Returns
 * -1 when the set has no penalty, no such pass ran, the pass had no region g, or the context has no device. Call it before
 * the next evaluation re-uses the arena slot. */
int32_t gaml_hip_debug_gap_cov_layout(gaml_hip_ctx* ctx, int readset, int g, int32_t* slot_base, int32_t cap_slots, int32_t* path_base,
                                      int32_t* start_off, int32_t* slots, int32_t cap_paths, int32_t* starts, int32_t cap_starts, int32_t* counts4);
/* Region g of the last pass of a gap profile that took the mixed device route (gaml_hip_set_gap_mixed_device on), of single-end
 * set `readset`: what gap_single_tables_kernel derived for the g-th length of that pass, copied back from the set's arena and
 * listed like gaml_hip_debug_occurrences: 5 ints per entry {window id, shift, min_pos, path, rank}, by rank. Returns the number
 * of entries, -1 when no such pass ran, the pass had no region g, or the context has no device. Call it before the next
 * evaluation re-uses the arena. */
int64_t gaml_hip_debug_gap_single_table(gaml_hip_ctx* ctx, int readset, int g, int32_t* out5, int64_t cap);
/* Column g (0..7) of the count table [sub-walk][8] that gap_pacbio_counts_kernel built for the last such pass of PacBio set
 * `readset`: out[w] = occurrences of cached sub-walk w in the path set with the pass's g-th length; columns behind the pass's
 * lengths hold 0. Returns the number of sub-walks, -1 when no such pass ran or the context has no device. */
int64_t gaml_hip_debug_gap_pacbio_counts(gaml_hip_ctx* ctx, int readset, int g, int32_t* out, int64_t cap);
/* The split enumeration of that route for `path` (one path, entry gap_pos a gap) with `len` in the gap: what the lengths
 * share + the growths that reach the gap, put together in the reference's order as {sub-walk id, begin} pairs (hits_out: 2
 * ints per hit, at most cap hits written), *misses_out (may be NULL) the lookups that found nothing. Returns the number of
 * hits; -1 on bad arguments, -2 when the result differs from the whole enumeration of the path (gaml_hip_last_error). Works
 * on a host-only context. */
int64_t gaml_hip_debug_pacbio_gap_enum(gaml_hip_ctx* ctx, int readset, const int32_t* path, int32_t path_len, int32_t gap_pos, int32_t len,
                                       int32_t* hits_out, int64_t cap, int64_t* misses_out);
/* node ids of a cached window (by id); returns its length, -1 if the id is unknown */
int32_t gaml_hip_debug_window_walk(gaml_hip_ctx* ctx, int readset, int mate, int32_t window_id, int32_t* out, int32_t cap);
/* ---- tuning ------------------------------------------------------------------------------------- */
/* The development build's A/B switches and tuning knobs: the one list of them. Every knob is 0 by default, and the release
 * library is compiled with every one at 0. A number never moves and is never re-used (probes load libraries built from
 * older trees and address them by number): a new knob takes the next number, before GAML_HIP_KNOB_COUNT. */
enum gaml_hip_knob {
  GAML_HIP_KNOB_GRID_CAP_COMPACT = 0,       /* n > 0: most blocks of the compact class (default: from the device's CU count) */
  GAML_HIP_KNOB_SCORE_LDS_BYTES = 1,        /* n: dynamic LDS bytes on the single-set scoring launch (occupancy experiments) */
  GAML_HIP_KNOB_FINISH_MODE = 2,            /* retired, setting it has no effect (it chose the last-block finish route of the paired scoring kernels, which is removed) */
  GAML_HIP_KNOB_TIMELINE = 3,               /* 8: in-kernel time stamps (gaml_hip_debug_timeline); any non-zero value keeps batches off the multi-set kernel */
  GAML_HIP_KNOB_NO_MEMO = 4,                /* 1: no floor/log memo of pair terms */
  GAML_HIP_KNOB_ALIGNER_ROUTE = 5,          /* gaml_hip_aligner_route: which route the window aligner is held to (default: its own choice per batch) */
  GAML_HIP_KNOB_DELTA_POLICY = 6,           /* gaml_hip_delta_policy: delta lists off, or no rebuild after a quiet spell */
  GAML_HIP_KNOB_NO_SPIN = 7,                /* 1: blocking calls wait with hipStreamSynchronize, no spinning on the pinned partials */
  GAML_HIP_KNOB_UPLOAD_ROUTE = 8,           /* gaml_hip_upload_route: pinned staging slots instead of host stores through the BAR */
  GAML_HIP_KNOB_ALIGNER_TIMED = 9,          /* 1: device syncs between the aligner's stages, for stage times */
  GAML_HIP_KNOB_GRID_CAP_CLASS1 = 10,       /* n > 0: most blocks of the <= 2-record class (default: a third of the compact class's) */
  GAML_HIP_KNOB_BATCH_ROUTE = 11,           /* gaml_hip_batch_route: how gaml_hip_calc_prob_batch scores its path sets (default: one pass, tables from patches) */
  GAML_HIP_KNOB_PLAN_WHOLE_SET = 12,        /* 1: every path set planned from scratch, no incremental planning */
  GAML_HIP_KNOB_NO_RESIDENT_TABLES = 13,    /* 1: whole per-call tables through the ring, no resident device copy */
  GAML_HIP_KNOB_REBUILD_ON_CALLER = 14,     /* 1: every table build on the calling stream, none beside the evaluations */
  GAML_HIP_KNOB_NO_RETIRE = 15,             /* 1: rebuilds never retire unused windows */
  GAML_HIP_KNOB_KEEP_DOMINATED = 16,        /* 1: record tables keep the junction records that never survive the overwrite rule (from the next table build; same values) */
  GAML_HIP_KNOB_NO_OCC_DEVICE = 17,         /* 1: whole-set calls build their occurrence tables on the host (no device route, occ_device.hip.h) */
  GAML_HIP_KNOB_GAP_FALLBACK = 18,          /* 1: gaml_hip_gap_profile and the gap-length search take their fallback route */
  GAML_HIP_KNOB_NO_STATIC_INDEX = 19,       /* 1: no static memo indices, every compact-class pair resolved per call (from the next table build; same values) */
  GAML_HIP_KNOB_GRID_CAP_COMPACT_REST = 20, /* n > 0: most blocks of the compact class's second part */
  GAML_HIP_KNOB_NO_COV_INSTANCE = 21,       /* 1: a set with a coverage penalty scores its compact class in the general form (three table loads per pair, no streamed values) */
  GAML_HIP_KNOB_DELTA_ONE_BLOCK = 22,       /* 1: delta maintenance by one-block launches only (default: multi-block above 3,000 records) */
  GAML_HIP_KNOB_ALIGNER_FIRST_CAP = 23,     /* n > 0: the aligner's general route starts with room for n spans and n candidates (its retry loop grows both; same records) */
  GAML_HIP_KNOB_DELTA_SPILL_CAP = 24,       /* n > 0: the delta store's spill area holds n long lists, 16 n records per mate (read when the store is reserved: set it before the first evaluation) */
  GAML_HIP_KNOB_TAKE_OVER_AFTER = 25,       /* n > 0: a build beside the evaluations takes over n evaluations after its start (default 96) */
  GAML_HIP_KNOB_REBUILD_DIVISOR = 26,       /* n > 1: tables are rebuilt when the delta lists pass pairs / n, at least 256 (default: pairs / 8, at least 4,096) */
  /* the block counts of the scoring launches: a cap can only LOWER a grid (0: the built-in rule, n > 0: min(that rule, n)) -- the
   * partial buffers are sized from the built-in maxima. With the three GRID_CAP knobs above they let a test of a few thousand pairs
   * run every class's stride loop for several rounds (tests/test_gpu_grid_split.py). */
  GAML_HIP_KNOB_GRID_CAP_CLASS2 = 27,       /* n > 0: most blocks of the 3-4-record class */
  GAML_HIP_KNOB_GRID_CAP_DELTA = 28,        /* n > 0: most blocks of the delta pairs */
  GAML_HIP_KNOB_GRID_CAP_OVERFLOW = 29,     /* n > 0: most wave-per-pair blocks */
  GAML_HIP_KNOB_GRID_CAP_SETS = 30,         /* n > 0: most blocks of every launch sized by grid_for: the single-end and PacBio scorers, their multi-set forms, the coverage sweeps */
  GAML_HIP_KNOB_PACBIO_SWEEP_CAP = 31,      /* n > 0: a contig goes to the block-per-contig sweep of a penalised PacBio set's chunk with up to min(n, 2048) intervals, larger ones through the general chain (default: 2048) */
  GAML_HIP_KNOB_COUNT = 32
};
/* the values of the knobs that choose between routes (0 = the default, in every one) */
enum gaml_hip_aligner_route {
  GAML_HIP_ALIGNER_HOST = 1,         /* the host aligner */
  GAML_HIP_ALIGNER_HOST_SORT = 2,    /* the hits of large batches sorted on the host */
  GAML_HIP_ALIGNER_GENERAL = 3,      /* always the general route, no small-batch pipeline */
  GAML_HIP_ALIGNER_PER_MATE = 4,     /* one small-batch pipeline per mate */
  GAML_HIP_ALIGNER_INPUT_BLOCK = 5,  /* window strings always through the input block, never the kernel arguments */
  GAML_HIP_ALIGNER_HOST_FILING = 6   /* hits filed on the host */
};
enum gaml_hip_delta_policy {
  GAML_HIP_DELTA_NO_LISTS = 1,         /* no delta lists: every newly activated window rebuilds the tables, on the calling stream */
  GAML_HIP_DELTA_NO_QUIET_REBUILD = 2  /* no rebuild after 64 calls without an activation */
};
enum gaml_hip_upload_route {
  GAML_HIP_UPLOAD_MEMCPY = 1,      /* pinned staging slot + hipMemcpyAsync */
  GAML_HIP_UPLOAD_COPY_KERNEL = 2  /* pinned staging slot + copy kernel */
};
enum gaml_hip_batch_route {
  GAML_HIP_BATCH_SEQUENTIAL = 1,   /* one launch per path set */
  GAML_HIP_BATCH_FULL_TABLES = 2,  /* one pass, whole tables per set */
  GAML_HIP_BATCH_NO_CAPTURE = 3    /* one pass, every set resolves every pair (no capture of unchanged pairs) */
};
/* `knob` is a gaml_hip_knob (an int in the signature: a probe may address a library built from an older tree by number);
 * GAML_HIP_EINVAL outside 0 .. GAML_HIP_KNOB_COUNT - 1. A multi-device context passes the value on to every shard.
 * Environment (development build): GAML_DL_STAMPS=1 prints the delta kernel's stage times. */
int gaml_hip_debug_set_knob(gaml_hip_ctx* ctx, int knob, int value);
/* Ablation 8 (GAML_HIP_KNOB_TIMELINE = 8) of the last evaluation of paired read set rs: 8 wall-clock stamps (10 ns units) per wave,
 * [kernel entry, tables in LDS, records in, occurrences in, memo in, stores issued, block reduced, class]. Returns the
 * number of waves copied. Tuning aid (tools/kernel_timeline.py). */
int gaml_hip_debug_timeline(gaml_hip_ctx* ctx, int rs, unsigned long long* out, int64_t cap_waves);

/* Environment (read once): GAML_HIP_TRACE_HOST=1 -- host-side phase times of slow calls, table builds and rebuilds on
 * stderr; GAML_HIP_TRACE_ALIGNER=1 -- aligner stage times with gaml_hip_aligner_stats; GAML_HIP_BACKTRACE=1 -- a
 * backtrace on stderr when the process aborts or faults (also after the HIP runtime reports a GPU memory fault). */
/* host-only (works without a device): the record tables of the windows that are active now, built with and without the
 * rule "a junction record that the first node's own record always overwrites stays out" (GAML_HIP_KNOB_KEEP_DOMINATED), compared pair by
 * pair. out6 = {records left out mate 1, mate 2, compact-class pairs with / without the rule, records checked,
 * violations}; GAML_HIP_ESTATE if a record was left out that the rule does not cover. */
int gaml_hip_debug_fold_check(gaml_hip_ctx* ctx, int readset, int64_t* out6);
/* The library's own stable radix sort (gaml_amd/csrc/radix_sort.hip.h: the aligner's hit ordering, graph.cc:841, 895-897, and
   the PacBio coverage sweep, graph.cc:3198-3250) on caller data: keys[n] and, unless null, vals[n] are sorted in place on
   bits [begin_bit, end_bit); run_max (or null) receives the inclusive running maximum of the sorted payload (of the sorted
   keys without one). */
int gaml_hip_debug_radix_sort(gaml_hip_ctx* ctx, uint64_t* keys, uint64_t* vals, int64_t n, int begin_bit, int end_bit, uint64_t* run_max);
/* host-only: the static memo indices of the compact class (both records of a pair in windows with the same node walk:
 * orientation rule, insert distance and memo index do not depend on the path set) recomputed from the window cache.
 * out8 = {pairs with an index, other compact-class pairs, violations, then why those others have none: a mate without
 * record, records in different windows, orientation rule, distance outside the insert-size table, edit count or length
 * code outside the memo}; GAML_HIP_ESTATE on a violation. */
int gaml_hip_debug_static_check(gaml_hip_ctx* ctx, int readset, int64_t* out8);
/* The device table build (gaml_amd/csrc/table_build.hip.h: the read-major join the reference does per call through hash maps,
 * graph.cc:535-598) against the host restatement build_pair_tables on the windows that are active now: a fresh build into
 * scratch buffers, every array compared entry by entry. out8 = {pairs, compact class, its static part, <= 2 records, <= 4,
 * more, entries compared, mismatches}; GAML_HIP_ESTATE when they differ. */
int gaml_hip_debug_tables_check(gaml_hip_ctx* ctx, int readset, int64_t* out8);
/* per-block partial sums / floored counts of the last blocking evaluation of paired set `readset` (path set `set` of a
 * batch launch, 0 for a single call), in block order; layout8 = {blocks of the compact class's static part, of the
 * compact class, up to the <= 2-record class, up to the <= 4-record class, lane-per-pair blocks, all scoring blocks,
 * 0, partials}. Returns the number of partials. For bit-equality hunts between routes. */
int32_t gaml_hip_debug_block_partials(gaml_hip_ctx* ctx, int readset, int32_t set, double* sums, int32_t* zeros, int32_t cap, int32_t* layout8);

/* Occurrence tables of whole-set calls built on the device (gaml_amd/csrc/occ_device.hip.h), paired set `readset`:
 * out6 = {calls whose tables the device built, calls whose tables the host built, device-route calls evaluated again on
 * the host route because two paths share a window, pool compactions, pool entries in use (both mates), memo combinations
 * known to share windows}. */
int gaml_hip_debug_occ_route(gaml_hip_ctx* ctx, int readset, int64_t* out6);
/* When the last call took the device route: its device tables copied back and compared entry by entry with the host image
 * built for the same set. out4 = {entries compared, entries present, mismatches, mates whose host image needs lists};
 * GAML_HIP_ESTATE when they differ. All zeros when the last call did not take the route. */
int gaml_hip_debug_occ_check(gaml_hip_ctx* ctx, int readset, int64_t* out4);

/* Which of its rarely taken routes the window aligner took so far (gaml_amd/csrc/aligner_launch.hip.h): out4 = {attempts of the
 * general route repeated because the spans or candidates did not fit its buffers, paired small batches handed to the per-mate
 * route because the candidates did not fit the fixed buffers, ... because the device filing refused them (more than 2,048
 * candidates, pool full), batches flushed to the host aligner after the sixth attempt}. */
int gaml_hip_debug_aligner_routes(gaml_hip_ctx* ctx, int64_t* out4);

/* The resident read-major table of single-end set `readset` against the host's build_read_major over the window cache as
 * it stands, entry by entry, whichever route built it (gaml_hip_set_single_device): waits for the library's stream, copies
 * first[] / extra[] back, changes no state. out4 = {entries compared (reads + further records), mismatching first[]
 * entries, mismatching extra[] entries, sizes that differ}. A host-only context reports the sizes and zeros. GAML_HIP_ESTATE
 * when windows were activated since the last scoring call (the table is older than the cache). */
int gaml_hip_debug_single_table_check(gaml_hip_ctx* ctx, int readset, int64_t* out4);

/* bad_bases of paired set `readset` for every path set of the last gaml_hip_calc_prob_batch, in the batch's order, whichever
 * route its chunks took (0 for a set without coverage penalty). Returns the number of path sets; at most `cap` are written.
 * A batch over penalised sets: GAML_HIP_KNOB_BATCH_ROUTE at 0 takes the one-pass routes (tables from patches, else whole; the
 * capture of unchanged pairs is always off for such a launch, so NO_CAPTURE equals 0 there), FULL_TABLES whole tables per set,
 * SEQUENTIAL one call per path set. */
int32_t gaml_hip_debug_batch_bad_bases(gaml_hip_ctx* ctx, int readset, int64_t* out, int32_t cap);
/* The same of PacBio set `readset` (0 for a set without coverage penalty): filled by the one-pass routes
 * (gaml_hip_set_pacbio_penalty_onepass) and by the sequential path alike, so a test can hold route against route.
 * GAML_HIP_EINVAL for a handle that is not a PacBio set. */
int32_t gaml_hip_debug_pacbio_batch_bad_bases(gaml_hip_ctx* ctx, int readset, int64_t* out, int32_t cap);

/* The LIVE record tables plus the live delta lists (gaml_amd/csrc/delta_dev.hip.h) of paired set `readset` against the host
 * restatement build_pair_tables, read by read, over the windows the tables and their lists took in. Inspects and changes
 * nothing: starts no rebuild, finishes none, prepares no tables (gaml_hip_debug_tables_check does all three); while a rebuild
 * runs beside the evaluations it covers the live tables and lists only. For every pair on the lists: its list (fixed stride
 * or spill range) record for record, the head words (L1 | L2 << 16, the two list lengths), the unused stride entries, its
 * slot and the tables' mark; for every other pair: the tables' own list is complete; the numbering 0 .. n-1, the spill
 * ranges in use (below the area's top, disjoint), the device counters against their pinned copy, the records left out.
 * out12 = {pairs on the lists, of those from the compact class's static part, its other part, the <= 2-record class, <= 4,
 * more, pairs at the fixed stride with lists of up to 2 records, of 3 to 4, long lists, entries compared, mismatches, records
 * of later windows left out}; GAML_HIP_ESTATE on a mismatch (GAML_HIP_TRACE_HOST=1 prints the first sixteen). */
int gaml_hip_debug_delta_check(gaml_hip_ctx* ctx, int readset, int64_t* out12);
/* Which launches the delta maintenance of paired set `readset` chose so far: out10 = {one-block launches with 1, 2, 4, 8
 * records per thread, multi-block launches, of those with the window list in device memory, windows cut across launches,
 * records and windows of the last maintenance call, the smallest block of a one-record-per-thread launch (0: none)}. */
int gaml_hip_debug_delta_routes(gaml_hip_ctx* ctx, int readset, int64_t* out10);
/* The live lists' numbering: reads[d] = the read of the pair with delta index d, spill[d] = its spill index (-1: fixed
 * stride). Returns the number of pairs on the lists; at most `cap` are written. */
int32_t gaml_hip_debug_delta_numbering(gaml_hip_ctx* ctx, int readset, int32_t* reads, int32_t* spill, int32_t cap);

#ifdef __cplusplus
}
#endif
#endif /* GAML_HIP_DEBUG_H_ */
