// ctx.hip.h -- the library context: device / pinned buffers, per-read-set device state, gaml_hip_ctx.
// Shared by gaml_hip.hip (the C ABI, launches) and multi.hip (several device shards in one process, RCCL).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include "resource.hip.h"
#include "radix_sort.hip.h"

#include <algorithm>
#include <atomic>
#include <fcntl.h>
#include <sys/mman.h>
#include <unistd.h>
#include <chrono>
#include <climits>
#include <limits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <immintrin.h>
#include <memory>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "aligner.hip.h"
#include "aligner_small.hip.h"
#include "aligner_file.hip.h"
#include "host_model.h"
#include "kernels.hip.h"
#include "paired_multi.hip.h"
#include "set_kernels.hip.h"
#include "table_build.hip.h"
#include "single_tables.hip.h"
#include "delta_dev.hip.h"
#include "pacbio_dp.hip.h"
#include "pacbio_sweep.hip.h"
#include "internal.h"


// A/B switches and tuning knobs (gaml_hip_debug_set_knob) exist in development builds (-DGAML_HIP_DEV) only; the release
// library is compiled with every one of them at its default, 0. KNOB(c, NO_MEMO) reads GAML_HIP_KNOB_NO_MEMO of enum
// gaml_hip_knob (include/gaml_hip_debug.h: the one list of them).
#ifdef GAML_HIP_DEV
#define KNOB(c, i) ((c)->knobs[GAML_HIP_KNOB_##i])
#else
#define KNOB(c, i) 0
#endif
// ... and so do the aligner's route counters (gaml_hip_debug_aligner_routes): 0 general-route retries, 1 / 2 paired small batches
// handed to the per-mate route because the candidates did not fit / because the device filing refused them, 3 batches flushed
// to the host aligner after the sixth attempt
#ifdef GAML_HIP_DEV
#define ALN_ROUTE(c, i) ((c)->aln_routes[i]++)
#else
#define ALN_ROUTE(c, i) ((void)0)
#endif

namespace gaml {
namespace detail {

inline double now_us() {
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// development aid (development build, GAML_HIP_PROBE=1): a 4-byte fill + stream synchronise at a few places of an evaluation; reports
// how long the device took to answer -- how the 12-25 ms stall after the cold alignment batch was found (AlignScratch::stage)
inline void gpu_probe(hipStream_t st, void* p4, const char* label) {
#ifdef GAML_HIP_DEV
  static const bool on = getenv("GAML_HIP_PROBE") != nullptr;
  if (!on || !p4) return;
  const double t0 = now_us();
  (void)hipMemsetAsync(p4, 0, 4, st);
  (void)hipStreamSynchronize(st);
  const double dt = now_us() - t0;
  fprintf(stderr, "probe %-28s %8.2f ms%s\n", label, dt * 1e-3, dt > 1000.0 ? "   <-- stall" : "");
#else
  (void)st; (void)p4; (void)label;
#endif
}

struct Reducer {  // per read set: partials + ticket + 2-double result
  DevBuf part_sum, part_zero, ticket, out;
  hipError_t init() {
    hipError_t e;
    if ((e = part_sum.reserve((4 * kMaxBlocks + kOvfMaxBlocks) * sizeof(double))) != hipSuccess) return e;
    if ((e = part_zero.reserve((4 * kMaxBlocks + kOvfMaxBlocks) * sizeof(int))) != hipSuccess) return e;
    if ((e = ticket.reserve(kTicketWords * sizeof(unsigned))) != hipSuccess) return e;
    if ((e = out.reserve(4 * sizeof(double))) != hipSuccess) return e;
    if ((e = hipMemset(ticket.p, 0, kTicketWords * sizeof(unsigned))) != hipSuccess) return e;
    if ((e = hipMemset(out.p, 0, 4 * sizeof(double))) != hipSuccess) return e;
    return hipDeviceSynchronize();  // the scoring stream is non-blocking: make the zeroes land first
  }
};

struct AlignDev {  // device copies the GPU aligner needs: reads (1 byte per base) + the max-hash index
  DevBuf reads, read_off, bucket_hash, bucket_top, bucket_off, bucket_reads;  // bucket_top: first bucket per upper half of the key (aln_find_bucket)
  DevBuf htab;     // key -> bucket, open addressing (AlnHashSlot, 2^hbits slots; hbits = 0: none)
  int hbits = 0;
  bool uploaded = false;
};
struct AlignScratch {  // per context, grown on demand
  DevBuf wstr, wins, blk, spans, cands, hits, counters;
  DevBuf sort_keys, sort_idx, sort_tmp, hits_sorted, file_tmp;  // large batches: hits ordered (and filed) on the device
  // What a large batch sends and receives travels through pinned memory of the library's own. (Copies straight from / to the
  // job's vectors made the runtime register those pages with the device -- and FREEING such a buffer afterwards makes the
  // driver evict the process's queues: the first dispatch after the cold batch started 12-25 ms late, the device idle.)
  PinBuf stage;
};

// small batches (aln_small_*): one set of buffers per mate, so that the two mates' pipelines run side by side. Input
// block written by the host (device memory behind the BAR, or its pinned twin), counters + hits published in mapped
// pinned memory behind a sequence word.
struct AlignSmall {
  DevBuf spans, cands, hits, counters, wcopy;
  HostBlock in;     // [windows][code-buffer offsets][window strings] of a batch
  PinBuf out_host;
  AlnStrArgs str_args;  // a small batch's window strings as they travel in the launches' argument segments
  unsigned long long out_seq = 0;
  double seen_us = 0;   // host clock when the last batch's sequence word was seen (timing builds)
  Event probe_ev[4];  // timing probes of the development build (GAML_ALN_WAIT)
};
// one batch of pending windows of one mate: strings built once, possibly already in flight on the device
struct AlnJob {
  bool prepared = false, enqueued = false;
  std::string wstr;
  std::vector<AlnWindow> wins;
  std::vector<int32_t> blk;  // blk[w] = first block of window w in span_maxima_kernel's grid; blk[n] = the grid size
  unsigned long long seq = 0;
  void* stream = nullptr;  // where the small-batch pipeline was enqueued
};

struct MateDev {
  DevBuf first, extra, pows;  // pows = mismatch_pow | match_pow (first / extra: the read-major tables of a single-end set)
  AlignDev aln;
  uint64_t uploaded_generation = ~0ull;
  size_t pow_n = 0;
  // paired sets: the alignment-window cache's records ON THE DEVICE, window-major (a window's records contiguous, ordered by
  // (position, read)): int4 {window id, position, edit | orient << 8, read}. Window::dfirst points into it. Filled by the
  // aligner's filing kernels, or mirrored from the host pool for windows the host filed (host aligner, caller-supplied records)
  DevBuf pool;
  int64_t pool_n = 0;         // records in use
  size_t filed_done = 0;      // ShortMate::filed[0 .. filed_done) are on the device
  DevBuf lens;                // read lengths
};

// the device side of one build of the record tables: everything a rebuild replaces as a whole (table_build.hip.h)
struct TableDev {
  DevBuf rec8[2], first[2], extra[2], inl[2], len_code, len12, static_idx, static_val;
  DevBuf slot_of_read, read_of_slot, dirty_of_slot;  // read -> slot, slot -> read, slot -> index on the delta lists (-1: none)
  DevBuf cnt;              // the build's device counters (kTb*)
  bool built = false;
  // what the host knows of it once the build is through
  int64_t class_count[4] = {0, 0, 0, 0}, n0a = 0, extras[2] = {0, 0}, dropped[2] = {0, 0};
  bool keep_dominated = false;   // KEEP_DOMINATED when it was built
#ifdef GAML_HIP_DEV
  std::vector<int32_t> held[2];  // per mate: the windows whose records the tables and their delta lists took in, in that order (gaml_hip_debug_delta_check)
  size_t held_built[2] = {0, 0}; // ... of which the first so many came with the build, the rest through the delta lists
#endif
  std::vector<int32_t> read_of_slot_host;  // fetched on demand (gaml_hip_read_probs)
  bool ros_valid = false;
};

// scratch of a table build (one build at a time per set)
struct BuildScratch {
  DevBuf k_in, k_out, k_tmp, v_in, v_tmp, hist, v_sorted[2], rstart[2], rend[2], one[2], cl, sidx, more[2], start[2], tiles, wins[2], peer0;
  PinBuf h_wins[2], h_peer, h_cnt;
};

// A rebuild of the record tables beside the evaluations: the build is a chain of kernels on a stream of its own over the
// device pool (a few hundred microseconds at 833 k pairs); evaluations go on over the old tables + delta lists, and the new
// tables take over a FIXED number of evaluations later (equal inputs must give equal outputs run to run, and a rebuild
// changes the order of the final sum). What was activated in between is applied to the new tables' (empty) delta lists by
// the same kernel that maintains the live ones.
// what the slices of one build share (paired_build_enqueue)
struct BuildPlan { int64_t A[2] = {0, 0}; int n_act[2] = {0, 0}; unsigned tiles = 0, none1 = 0, none2 = 0; int ins_n = 0, units = 1; bool empty = true; };

struct TableRebuild {
  bool active = false;
  bool retired = false;        // a rebuild beside the evaluations was decided and the unused windows have left: the next evaluation starts the build
  int next_slice = 0;          // slices of the build's launch chain enqueued so far
  int64_t start_eval = 0;      // the set's evaluation count when the rebuild was decided
  TableDev tab;                // the spare set of buffers: being built, or idle
  Stream stream;
  Event done, mark;
  std::vector<std::pair<int32_t, int32_t>> after;  // (mate, window) activated since the build started: not in the new tables
};

// what the host keeps of the live tables (the tables themselves exist on the device only)
using EventPair = std::pair<Event, Event>;  // around a scoring launch (gaml_hip_set_event_timing)

struct PairInfo {
  int64_t class_count[4] = {0, 0, 0, 0};  // 0: compact; 1: <= 2 records; 2: <= 4; 3: more
  int64_t n0a = 0;                        // static part of the compact class
  std::vector<uint32_t> len_combo;        // distinct L1 | L2 << 16 values (<= 256), in order of first appearance: fixed per read set
  int64_t dropped_records[2] = {0, 0};
};

// the advice move of a paired set (advice.hip.h): the index over this shard's pairs and the buffers of a query
struct AdviceDev {
  bool built = false;
  int32_t threshold = 0;
  int64_t n_ent = 0, queries = 0;
  std::vector<int64_t> h_offs;          // host-only contexts: the index on the host
  std::vector<int32_t> h_ent;
  DevBuf offs, ent;                     // the index, resident: CSR over the pairs, entries node << 1 | orient1
  DevBuf scratch;                       // build: sort keys / payloads, flags, places, scan tiles
  DevBuf first, last, cnt, at, tiles;   // query: per-pair keys (stamped with the call's serial), counts, places
  DevBuf in, mask, out;                 // query: steps | path | reach, exclusion + reach bits, the list
  PinBuf h_in, h_out;
  uint32_t serial = 0;
  std::vector<AdviceStep> steps;        // the last query's walk ...
  std::vector<int32_t> list;            // ... and its candidates
};

struct PairedSet {
  gaml_paired_cfg cfg;
  ShortMate mate[2];
  PairInfo pt;
  MateDev dev[2];                     // (pows, aligner index, record pool, generation)
  TableDev tab;                       // the live record tables
  TableRebuild rebuild;
  BuildScratch scratch;
  BuildPlan build_plan;
  int64_t async_rebuilds = 0, retired_windows = 0, eval_count = 0;
  // per set, fixed: length-combination code per pair, the per-combination tables, the memo of pair terms
  DevBuf lcode, len_combo_dev, combo_tabs, memo;
  int memo_codes = 0;
  bool statics_uploaded = false, kernels_warm = false, prereserved = false;
  // Delta store (device): pairs whose record lists gained records of windows activated after the tables were built. Their
  // complete lists sit at a fixed stride (4 records per mate; longer ones in the spill area); maintained by
  // delta_apply_kernel, read by the scoring launch. The host knows upper bounds (and the exact counts once a blocking call
  // has returned: h_dstate, written by the kernels).
  DevBuf dl_slot, dl_spill, dl_rec[2], sp_rng[2], sp_rec[2], sp_slot, dstate;
  DevBuf dl_bins, dl_bin_count, dl_blk_tot, dl_wlist, dl_stamps;   // multi-block maintenance launches (delta_dev.hip.h)
  PinBuf h_dstate;
  size_t delta_cap = 0, cap_spill = 0, cap_sprec = 0;
  int64_t nd_est = 0, ns_est = 0;     // delta pairs (upper bound) / long lists (last exact count) as the host knows them
  bool spill_may_grow = false;        // activations since the counts were last read back
  int dl_seq = 0;                     // sequence number of the last maintenance launch (h_dstate[kDsSeq] == dl_seq: the counts are current)
  int64_t full_rebuilds = 0, delta_updates = 0;
  // which launches paired_delta_apply chose so far (gaml_hip_debug_delta_routes): one-block <1>, <2>, <4>, <8>, multi-block,
  // multi-block with the window list in device memory, windows cut across launches, records / windows of the last apply,
  // the smallest <1> block used (0: none yet)
  int64_t dl_routes[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  int quiet_calls = 0;       // evaluations since the last window activation
  int64_t delta_left_out = 0, delta_left_out_base = 0;  // records of later windows that never reached the delta lists (always overwritten); the device counts them per list generation
  bool compact_requested = false;  // gaml_hip_compact_tables: fold the delta lists into the tables at the next evaluation
  PinBuf h_timeline; int timeline_waves = 0;  // ablation 8 (tools/kernel_timeline.py)
  PinBuf h_part_sum, h_part_zero;     // per-block partials written straight to pinned host memory (blocking calls): [set][block]
  size_t host_part_stride = 0;        // entries per set
  int last_total_blocks = 0, last_sets = 1;
  int last_blocks[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // partials written per path set of the last launch(es)
  bool last_host_partials = false;
  DevBuf probs, tabs, cov_bits, bad;
  // gaml_hip_calc_prob_batch over a set with a coverage penalty: per launch [kMaxSets 64-bit counters | the bitmaps of its path
  // sets], the launches of a chunk one behind the other (cov_multi_used: a launch never shares a bitmap with one in flight);
  // store_bad_multi_kernel hands the counters over to h_bad[set's number in the chunk]
  DevBuf cov_multi;
  size_t cov_multi_used = 0;
  PinBuf h_bad;
  std::vector<int64_t> batch_bad;     // bad_bases per path set of the last gaml_hip_calc_prob_batch, or per length of the last gap profile on the device route (gaml_hip_debug_batch_bad_bases)
  // where the last device gap pass of a penalised set left its regions' coverage layouts (gaml_hip_debug_gap_cov_layout)
  struct GapCov { int slot = -1, n = 0; size_t stride = 0, sb_off = 0, pb_off = 0, so_off = 0, st_off = 0; int n_sb = 0, n_pb = 0, n_st = 0; int32_t total_bits[8] = {0}; } gap_cov;
  Arena arena;                        // per-call tables (occurrence images, thresholds, coverage layout): ring, whole tables per call
  // Blocking calls on a large-BAR device keep ONE resident copy of the tables and patch it in place (the kernel
  // of the previous call is done when the call returns): a call that shares most paths with the previous one writes
  // a few dozen 12-byte entries through the BAR instead of the whole image. Capacities leave room to grow.
  struct Persist {
    HostBlock blk;                     // (always fine-grained memory: the route exists on a large-BAR device only; blk.cap: bytes of the layout)
    size_t cap_w[2] = {0, 0}, cap_lo[2] = {0, 0}, cap_m[2] = {0, 0};  // table entries / list bounds / list entries per mate
    size_t off_tfloor = 0, off_occ[2] = {0, 0}, off_lo[2] = {0, 0}, off_m[2] = {0, 0};
    size_t cap_cov = 0, off_cov = 0;   // coverage layout of the call (penalty_constant > 0): int32 entries / where they start; written whole per call
    bool valid = false;                // the copy mirrors the host images as of their last take_changed()
    size_t last_bytes = 0;             // table entries + coverage layout the last update wrote (gaml_hip_last_phases()[6])
  } persist;
  // Whole-set blocking calls on the resident route build the occurrence tables on the device (occ_device.hip.h): every
  // memo's prepacked entries (PathMemo::pre) stay in a pool in device memory, a call sends one descriptor per path and
  // occ_scatter_kernel writes the entries into one of two tables per mate (used in alternation; the other one is cleared
  // in the same launch). The host images are not built for such a call: they go stale until a consumer rebuilds them.
  struct OccDev {
    DevBuf pool[2];                    // OccPre ranges, one per memo and mate, bump-allocated; compacted when full
    size_t pool_cap[2] = {0, 0}, pool_used[2] = {0, 0};
    uint32_t pool_gen = 1;             // a memo's range is valid while PathMemo::dev_gen equals this
    PinBuf stage;                      // uploads of new ranges: staged here, copied in stream order
    DevBuf tab[2][2], list[2][2];      // [mate][table]: 12-byte entries (all ones: absent) / window ids the table last received
    DevBuf stamp[2];                   // per window: serial of the last call that wrote it (duplicates between paths)
    size_t cap_w = 0, cap_list = 0;
    int32_t list_n[2][2] = {{0, 0}, {0, 0}};
    uint32_t serial = 0;               // device-route calls so far: the call with serial n writes table n & 1
    PinBuf dup;                        // set by the kernel when a window occurs in two paths of the set
    bool taken = false;                // the current call takes the device route
    bool check_dup = false;            // the last launch took it: the blocking call reads the duplicate flag
    bool image_stale = false;          // the host images do not hold the current set
    std::vector<std::vector<uint64_t>> shared;  // memo combinations (id << 32 | serial per path) known to share windows
    size_t shared_next = 0;
    std::vector<uint64_t> key;         // this call's combination
    int64_t dev_calls = 0, host_calls = 0, fallbacks = 0, compactions = 0;
  } occdev;
  int64_t batches_patched = 0, batches_full = 0;  // gaml_hip_calc_prob_batch chunks whose per-set tables were built on the device from patches / written whole
  size_t batch_slack = 0;             // extra bytes per path set region of a batch (grows when a set's tables did not fit)
  PairedPlanner planner;
  OccImage image[2];                 // persistent host images of the occurrence tables, patched per call
  std::vector<Occ> scratch_occ[2];   // debug dumps only
  Reducer red;
  Staging stage_pool;                // host-filed windows on their way into the device pool
  std::vector<double> ins_tab, floor_tab, logfloor_tab, covthr_tab;
  bool floor_positive = true;  // every floor exp(c + k s) > 0 (else "probability 0 is floored" does not hold: no memo / shortcut paths)
  bool tabs_uploaded = false;
  int64_t last_bad_bases = 0;
  AdviceDev adv;
};

// a single-end set's side of gaml_hip_calc_prob_batch (single_batch.hip.h)
struct SgMulti {
  DevBuf part_sum, part_zero, ticket;  // per set and block; a ticket of its own (single_score_multi_kernel)
  PinBuf out;       // {sum, floored, 0, reads} per set, written by the last block
  int64_t launches = 0;
};

// a single-end set's side of the device route (gaml_hip_set_single_device; single_tables.hip.h, single_device.hip.h): the
// host pool's mirror is MateDev::pool / pool_n, the table lands in MateDev::first / extra like the host-built one
struct SingleTabDev {
  DevBuf hdr, k_in, k_out, k_tmp, v_in, v_out, v_tmp, hist, flag, before, tiles, zero;  // zero: [0] stays 0 (tb_scan_*'s "entries left out"), [1] the heads of the last build
  uint64_t built_generation = ~0ull;  // ShortMate::active_generation the DEVICE route built the resident table at (~0: the host route's table, or none)
  int64_t built_records = 0;          // records of that build
  int64_t aligned_windows = 0, builds = 0, mirrored = 0, host_builds = 0;  // gaml_hip_single_device_stats
};

struct SingleSet {
  gaml_single_cfg cfg;
  ShortMate mate;
  ReadMajor rm;
  MateDev dev;
  DevBuf lens, probs, tabs, occ_arena;
  std::vector<Occ> last_occ;
  Reducer red;
  std::vector<double> floor_tab, logfloor_tab;
  bool tabs_uploaded = false;
  Staging stage;
  SgMulti multi;
  int64_t table_bytes = 0;  // occurrence tables staged by the last call or chunk (gaml_hip_single_stats)
  SingleTabDev td;
  // where the last mixed device gap pass left its regions in occ_arena (gap_mixed.hip.h; gaml_hip_debug_gap_single_table)
  struct GapTab { int n = 0; size_t region0 = 0, stride = 0, off_direct = 0, off_lo = 0, off_m = 0; int n_direct = 0, n_lo = 0, n_multi = 0; } gap_tab;
};

struct DpDev {  // device buffers of the PacBio banded DP
  DevBuf path, jobs, ops, scratch, out, dbg;
};

// coverage sweep of a PacBio set with a penalty (pacbio_sweep.hip.h)
struct PbSweepDev {
  // follows the record cache: per sub-walk the intervals {position, position_end} of its records that clear GetMinReadProb
  DevBuf iv_off, iv;
  std::vector<int32_t> iv_off_host;
  uint64_t generation = ~0ull;
  // per evaluation: contig lengths | node intervals | occurrences, staged as one block; then the evaluation's interval
  // list: node intervals first, the records' after them (this rank's; all ranks' after the exchange)
  DevBuf in, all;
  DevBuf key_begin, key_end, pos, key_begin_s, key_end_s, pos_s, end_max, tmp, bad;
  Staging stage;
};

// what a path contributes to a PacBio evaluation (pacbio_enumerate): its cached sub-walks in the order the reference
// meets them (graph.cc:2438-2454), each with the path coordinate it starts at, and the lookups that found nothing
struct PbHit { int32_t walk, begin; };
// `bad`: the path's bad_bases (CalcScoreForPacbio's sum is over the paths of the call, each swept on its own), -1 until a
// chunk of the one-pass routes has swept it; holds as long as the memo entry does
struct PbEnum { std::vector<PbHit> hits; int64_t misses = 0; int32_t len = 0; int64_t bad = -1; };

// a PacBio set's side of gaml_hip_calc_prob_batch (pacbio_batch.hip.h)
struct PbMulti {
  std::unordered_map<Walk, PbEnum, WalkHasher> memo;  // by normalised path; holds for one state of the record cache
  uint64_t memo_generation = ~0ull;
  DevBuf count;     // [sub-walk][kMaxSets] occurrence counts of the chunk's path sets
  DevBuf part_sum, part_zero, ticket;  // per set and block; a ticket of its own (pacbio_score_multi_kernel)
  PinBuf out;       // {sum, floored, 0, reads} per set, written by the last block
  int64_t launches = 0;
  // a set with a penalty (gaml_hip_set_pacbio_penalty_onepass): the chunk's paths without a memoised value, one contig each
  DevBuf sweep_in;  // headers | node intervals | occurrences of the contigs pacbio_path_sweep_kernel takes, staged as one block
  DevBuf bad;       // per swept contig: the block-per-contig kernel's first, the general chain's behind them
  PinBuf bad_host;  // ... handed over behind the sweeps (pacbio_store_bad_kernel)
  int64_t penalty_stats[4] = {0, 0, 0, 0};  // gaml_hip_pacbio_penalty_stats
};

struct PacbioSet {
  gaml_single_cfg cfg;
  int64_t n_global = 0, lo = 0, hi = 0;
  std::vector<int32_t> lens;  // shard
  double log_match = 0, log_mismatch = 0;
  std::unordered_map<Walk, int32_t, WalkHasher> walk_id;
  std::vector<std::vector<gaml_pacbio_aligment>> recs;  // per sub-walk, local read ids
  uint64_t generation = 0, uploaded_generation = ~0ull;
  int32_t max_len = 0;
  int64_t misses = 0;
  DevBuf d_lens, rec_off, rec_walk, rec_logp, walk_count, logprobs;
  Reducer red;
  int64_t last_bad_bases = 0;
  std::vector<int64_t> batch_bad;  // bad_bases per path set of the last gaml_hip_calc_prob_batch, whichever route (gaml_hip_debug_pacbio_batch_bad_bases)
  Staging stage;
  PbSweepDev sweep;
  PbMulti multi;
  // a gap profile on the mixed device route (gap_mixed.hip.h): per sub-walk its occurrences in what the lengths share, resident
  // for the profile's passes; the record cache it was counted against; the columns of the last pass (gaml_hip_debug_gap_pacbio_counts)
  DevBuf gap_core;
  uint64_t gap_core_generation = ~0ull;
  int gap_cols = 0;
  // cache-miss side (SAM ingestion): bases of this shard's reads and the name -> global id map
  bool have_reads = false;
  std::string bases;
  std::vector<int64_t> base_off;  // local read i = bases[base_off[i], base_off[i+1])
  std::unordered_map<std::string, int32_t> name_id;
  DevBuf d_bases;
  DpDev dp;
  bool bases_uploaded = false;
  double dp_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

struct PairedPrep {
  int64_t assembled_records = 0;  // records the reference would touch in GetPositionsOnlyPath
  // coverage bitmap layout (penalty_constant > 0). The scoring kernels mark through slot_base[path slot of the table entry];
  // the sweep walks the paths in set order: path_base[k] (monotone: it finds a word's path by binary search), the contig
  // starts of path k at starts[start_off[k] .. start_off[k + 1]). slot_base[slots[k]] == path_base[k].
  std::vector<int32_t> slot_base, path_base, start_off, starts;
  int32_t total_bits = 0, n_paths = 0;
  bool general = false;           // some window occurs several times in this path set: the GEN instantiation of the scoring kernels
};

struct SetRef { int kind, idx; };

// GAML_HIP_GAP_PENALTY=device: what a new context's gap_penalty_device starts as (read when the context is made)
inline bool gap_penalty_env() { const char* e = getenv("GAML_HIP_GAP_PENALTY"); return e && strcmp(e, "device") == 0; }
// GAML_HIP_GAP_MIXED=device: what a new context's gap_mixed_device starts as (read when the context is made)
inline bool gap_mixed_env() { const char* e = getenv("GAML_HIP_GAP_MIXED"); return e && strcmp(e, "device") == 0; }
// GAML_HIP_SINGLE_BATCH=onepass: what a new context's single_onepass starts as (read when the context is made)
inline bool single_onepass_env() { const char* e = getenv("GAML_HIP_SINGLE_BATCH"); return e && strcmp(e, "onepass") == 0; }
// GAML_HIP_PACBIO_PENALTY_BATCH=onepass: what a new context's pacbio_penalty_onepass starts as (read when the context is made)
inline bool pacbio_penalty_onepass_env() { const char* e = getenv("GAML_HIP_PACBIO_PENALTY_BATCH"); return e && strcmp(e, "onepass") == 0; }
// GAML_HIP_SINGLE_DEVICE=1: what a new context's single_device starts as (read when the context is made)
inline bool single_device_env() { const char* e = getenv("GAML_HIP_SINGLE_DEVICE"); return e && strcmp(e, "1") == 0; }

}  // namespace detail
}  // namespace gaml

using namespace gaml;          // (this header is private to the library's two HIP translation units)
using namespace gaml::detail;

struct gaml_hip_ctx {
  // (first, so that they go last: everything below that was used on them is destroyed while they exist)
  Stream stream;
  Stream aux_stream;  // the overflow kernel runs beside the main kernel
  gaml::MultiState* multi = nullptr;  // several device shards behind this context (gaml_hip_create_multi): every call is forwarded
  gaml::CommState* comm = nullptr;    // RCCL communicator of a sharded context (gaml_hip_comm_init_rank / the shards of a multi context)
  int device = -1;
  DevBuf warm_buf; bool general_warm = false;  // warm_general_kernels (gaml_hip.hip)
  AlnJob aln_job[2];  // the two mates' pending alignment batches (align_pending_pair): buffers kept from call to call
  GraphStore g;
  bool have_graph = false;
  std::vector<std::unique_ptr<SingleSet>> singles;
  std::vector<std::unique_ptr<PairedSet>> paireds;
  std::vector<std::unique_ptr<PacbioSet>> pacbios;
  std::vector<SetRef> handles;  // creation order -> (kind, index)
  int32_t rank = 0, world = 1;
  bool multi_shard = false;  // one of the shards of a multi-device context (gaml_hip_create_multi)
  AlignScratch aln_scratch;
  AlignSmall aln_small[2];
  int64_t aln_windows = 0, aln_candidates = 0;  // GPU aligner statistics
  double aln_us = 0;
  double aln_stage_us[5] = {0, 0, 0, 0, 0};  // window strings + upload, spans + candidates, extension, D2H of hits, sort + finalize
  int64_t aln_batches = 0;
  int64_t aln_routes[4] = {0, 0, 0, 0};  // ALN_ROUTE: development builds only
  int knobs[GAML_HIP_KNOB_COUNT] = {0};  // tuning experiments and A/B switches (gaml_hip_debug.h), development builds only: read through KNOB()
  bool direct_write = false;  // large-BAR device: the host writes per-call tables straight into device memory (Arena)
  int32_t peers = 1;  // contexts (incl. this one) that hold reads of the same read sets: >1 => window maxima must be exchanged
  std::string err;
  // timing
  bool event_timing = false;
  int event_every = 1;    // time every k-th scoring launch (attached events cost ~4 us of host time per launch)
  int64_t event_tick = 0;
  std::vector<EventPair> ev_pool;  // one pair per scoring launch of a call
  std::vector<uint64_t> ev_call;  // ... and the evaluation (eval_serial) it belongs to
  uint64_t eval_serial = 0;
  size_t ev_used = 0;
  double t_host_us = 0, t_dev_wall_us = 0, t_kernel_us = 0;
  int64_t stat_launches = 0;
  double stat_device_us = 0, stat_algo_bytes = 0;
  DevBuf packed;  // 4 doubles per read set
  PinBuf packed_host;
  // gaml_hip_shm_exchange_*: the ranks of one node add up their (host-resident) partials through a POSIX shared-memory block
  char* shm_base = nullptr; size_t shm_bytes = 0; int shm_rank = 0, shm_world = 0, shm_cap = 0; unsigned long long shm_step = 0; std::string shm_name;
  PinBuf fetch_host;            // gaml_hip_fetch_async / _wait: [sequence word | 63 x pad | doubles]
  unsigned long long fetch_seq = 0;
  hipStream_t fetch_stream = nullptr;  // where the last fetch went: the caller's stream or this context's, not owned
  DevBuf batch_dev;  // gaml_hip_calc_prob_batch: 4 doubles per read set and path set
  PinBuf batch_host;
  // gaml_hip_gap_profile / gaml_hip_fix_gap_length (gap_profile.hip.h): {profile calls, lengths scored on the device route, on the
  // fallback, device passes}, and the path set with the base length in its gap (kept from call to call)
  int64_t gap_stats[4] = {0, 0, 0, 0};
  bool gap_penalty_device = gap_penalty_env();  // penalised paired sets may take the gap profile's device route (gaml_hip_set_gap_penalty_device)
  bool gap_mixed_device = gap_mixed_env();  // contexts with single-end sets and / or PacBio sets without a penalty may take the gap profile's device route (gaml_hip_set_gap_mixed_device)
  bool single_onepass = single_onepass_env();  // single-end sets go along on the batch's one-pass routes (gaml_hip_set_single_onepass)
  bool pacbio_penalty_onepass = pacbio_penalty_onepass_env();  // PacBio sets with a penalty go along on the batch's one-pass routes (gaml_hip_set_pacbio_penalty_onepass)
  bool single_device = single_device_env();  // single-end sets: windows aligned in device batches, read-major tables built by kernels (gaml_hip_set_single_device)
  AlnJob single_job;  // a single-end set's pending alignment batch (prepare_single_host): buffers kept from call to call, like aln_job
  std::vector<int32_t> gap_flat;
  std::vector<int64_t> gap_offs;
  // evaluation in progress (between eval_begin and eval_finish)
  bool pending_open = false;
  std::vector<Walk> pending_paths;
  bool pending_paths_valid = false;  // contexts of paired sets only never materialise the vectors
  int32_t pending_total_len = 0;
  std::vector<std::unique_ptr<PairedPrep>> pending_prep;  // per paired set
  double pending_host_us = 0;
  double prof[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // phase stamps of the last blocking call (us): see gaml_hip_debug_profile
  bool used_default_stream = false;  // an *_async entry point was handed NULL (the legacy default stream) since the last gaml_hip_sync
  // sharded evaluations: two status words the finisher kernel of a scoring launch writes with the partials, so that the exchange needs no
  // dispatch of its own for them (multi.hip: ctx_set_status / ctx_status_done)
  double* status_dst = nullptr; double status_a = 0, status_b = 0; bool status_done = false;
  bool host_results = false;  // blocking call: kernels write their results into pinned host memory, no D2H copy
  bool occ_route = false;     // gaml_hip_calc_partials: whole-set calls may build their occurrence tables on the device (occ_device.hip.h)
  // sharded evaluation with a coverage penalty: sweeps wait for the other ranks' coverage maps
  bool defer_cov = false;
  struct PendingCov { int paired_idx; CovArgs args; double* out4; };
  std::vector<PendingCov> pending_cov;
  // same for a PacBio set: the alignment intervals of the other ranks' reads are missing (device lists: PbSweepDev::all)
  struct PendingPacbio {
    int pacbio_idx;
    double* out4;
    int32_t n_paths;
    int64_t n_node, n_own;  // node intervals (every rank has them); this rank's record intervals behind them
  };
  std::vector<PendingPacbio> pending_pb;
};
