/* gaml_hip.h -- C ABI of libgaml_hip.so: the MI355X (gfx950) implementation of GAML's
 * assembly-likelihood hot path.
 *
 * This is the drop-in boundary.  GAML has no plugin/FFI layer; the path sits behind the
 * header-only class ProbCalculator (reference prob_calculator.h:37-124) whose CalcProb()
 * calls the three per-read-set scorers of graph.cc.  A maintainer replaces
 * prob_calculator.h by include/gaml_hip_prob_calculator.h; that
 * header forwards to the functions below.  Plain C types only, caller-owned input
 * buffers (copied during the call), library-owned host and device state, integer status
 * returns (0 = ok, <0 = error, text via gaml_hip_last_error).  No exceptions cross.
 *
 * Every entry point cites the reference interface it replaces (file:line under the
 * reference tree).  All citations: graph.cc / graph.h / gaml.cc / prob_calculator.h.
 */
#ifndef GAML_HIP_H_
#define GAML_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gaml_hip_ctx gaml_hip_ctx; /* opaque: graph + read sets + device state */

/* Aligment record, 4 x int32 = 16 B (reference graph.h:211-231). */
typedef struct gaml_aligment {
  int32_t position;    /* 1-based start inside the window's node string (graph.cc:890) */
  int32_t edit_dist;
  int32_t read_id;
  int32_t orientation; /* 0 forward, 1 reverse complement */
} gaml_aligment;

/* PacbioAligment record (reference graph.h:516-535): 3 x int32 + logdouble (f64 log). */
typedef struct gaml_pacbio_aligment {
  int32_t position;
  int32_t position_end;
  int32_t read_id;
  int32_t pad_;
  double logprob;
} gaml_pacbio_aligment;

/* SingleReadConfig (prob_calculator.h:7-18) + the read set's error model (gaml.cc:812-813). */
typedef struct gaml_single_cfg {
  double penalty_constant;
  double step;              /* penalty_step for single / pacbio (gaml.cc:818) */
  double min_prob_per_base;
  double min_prob_start;
  double weight;
  double mismatch_prob;     /* match_prob = 1 - 4*mismatch_prob */
} gaml_single_cfg;

/* PairedReadConfig (prob_calculator.h:20-35). step = insert_mean - penalty_step (gaml.cc:860). */
typedef struct gaml_paired_cfg {
  double penalty_constant;
  double step;
  double insert_mean;
  double insert_std;
  double min_prob_per_base;
  double min_prob_start;
  double weight;
  double mismatch_prob;
} gaml_paired_cfg;

/* ---- life cycle ------------------------------------------------------------------- */
/* device >= 0: HIP device ordinal (required for scoring). device = -1: host-only context:
 * graph / read sets / window alignment / occurrence tables work, every scoring call fails
 * with GAML_HIP_ENODEVICE (there is no CPU scoring path in this library). */
int gaml_hip_create(gaml_hip_ctx** out, int device);
void gaml_hip_destroy(gaml_hip_ctx* ctx);
const char* gaml_hip_last_error(const gaml_hip_ctx* ctx);
const char* gaml_hip_version(void);

#define GAML_HIP_OK 0
#define GAML_HIP_EINVAL (-1)
#define GAML_HIP_ENODEVICE (-2)
#define GAML_HIP_EHIP (-3)
#define GAML_HIP_ESTATE (-4)

/* ---- several GPUs -------------------------------------------------------------------
 * The reference's caller is ONE process holding ONE ProbCalculator (gaml.cc:1010, prob_calculator.h:37-124);
 * nothing in the reference is parallel (the sharding is new design). Two ways to more than one GPU:
 *
 * (1) gaml_hip_create_multi: one context that owns n_devices shards, one per listed HIP device (a device may be
 *     listed more than once, or be -1 for a host-only shard: rehearsals and tests). Reads are split by contiguous
 *     id range (shard i of n keeps [N*i/n, N*(i+1)/n)), graph / paths / window registration are replicated, each
 *     shard is driven by its own host thread. Every entry point of this header then works on the whole set:
 *     gaml_hip_calc_prob returns the value over all reads. Per evaluation the shards exchange ONE sum of 4 f64 per
 *     read set -- by an RCCL all-reduce over xGMI on the shards' streams (one communicator per shard,
 *     ncclCommInitAll; the default when every shard has its own GPU) or, as the measured alternative, by adding the
 *     shards' pinned-host partials in rank order on the calling thread (gaml_hip_set_exchange). The cold-path
 *     maximum of new windows' record positions and, with penalty_constant > 0, the union of the coverage maps /
 *     PacBio alignment intervals are merged in the library too (device lists). Environment: GAML_HIP_EXCHANGE=host|rccl picks the
 *     initial exchange ("rccl": creation fails when RCCL cannot be used).
 * (2) one process per GPU (torch.distributed.run, MPI): every process creates a plain context, calls
 *     gaml_hip_set_shard(rank, world) (or gaml_hip_set_presharded) and then gaml_hip_comm_init_rank with an id
 *     that rank 0 made with gaml_hip_comm_unique_id and sent to the others by any means (128 bytes). From then on
 *     gaml_hip_calc_prob / gaml_hip_calc_prob_batch are collective calls -- same paths on every rank, same value
 *     back on every rank -- with the same in-library RCCL exchanges as (1). */
int gaml_hip_create_multi(gaml_hip_ctx** out, const int32_t* devices, int32_t n_devices);
/* What the ProbCalculator adapters call: environment GAML_HIP_DEVICES unset -> gaml_hip_create(out, 0); "all" -> every
 * visible HIP device; "0,1,2,3" -> those (one entry: a plain context; several: gaml_hip_create_multi). */
int gaml_hip_create_from_env(gaml_hip_ctx** out);
int gaml_hip_num_shards(const gaml_hip_ctx* ctx);  /* 1 for a plain context */
#define GAML_HIP_EXCHANGE_HOST 0
#define GAML_HIP_EXCHANGE_RCCL 1            /* ncclAllGather of the ranks' partials, summed in RANK ORDER by every rank: the same
                                             * doubles in the same order on every rank and in every run (default) */
#define GAML_HIP_EXCHANGE_RCCL_ALLREDUCE 2  /* ncclAllReduce(sum): the order of the additions is RCCL's choice */
int gaml_hip_set_exchange(gaml_hip_ctx* ctx, int32_t mode);  /* multi-device contexts only; RCCL needs distinct devices */
int gaml_hip_get_exchange(const gaml_hip_ctx* ctx);
#define GAML_HIP_COMM_ID_BYTES 128
int gaml_hip_comm_unique_id(void* id_out /* GAML_HIP_COMM_ID_BYTES */);
int gaml_hip_comm_init_rank(gaml_hip_ctx* ctx, const void* id /* GAML_HIP_COMM_ID_BYTES */, int32_t rank, int32_t world);

/* ---- inputs ----------------------------------------------------------------------- */
/* Graph node sequences, what Graph::nodes[i]->s holds after LoadGraph (graph.cc:52-106):
 * n_nodes = 2 * velvet nodes, twin of i is i^1. bases = concatenation, offs[n_nodes+1]. */
int gaml_hip_set_graph(gaml_hip_ctx* ctx, int32_t n_nodes, const char* bases, const int64_t* offs);
/* Same, parsed from a Velvet LastGraph file by the library (graph.cc:52-106). */
int gaml_hip_load_graph(gaml_hip_ctx* ctx, const char* lastgraph_file);

/* Read sets. Returns the read-set handle (>= 0). Reads = concatenated bases + offs[n+1];
 * what ReadSet::PreprocessReads + PrepareReadIndex leave in a ReadSet (graph.cc:1366-1415).
 * Order of creation within a kind = order of ProbCalculator's constructor vectors. */
int gaml_hip_add_single(gaml_hip_ctx* ctx, const gaml_single_cfg* cfg, int32_t n_reads,
                        const char* bases, const int64_t* offs);
int gaml_hip_add_paired(gaml_hip_ctx* ctx, const gaml_paired_cfg* cfg, int32_t n_pairs,
                        const char* bases1, const int64_t* offs1, const char* bases2, const int64_t* offs2);
/* PacBio: only read lengths are needed by the scoring side (graph.cc:3062-3088, graph.h:478-481). */
int gaml_hip_add_pacbio(gaml_hip_ctx* ctx, const gaml_single_cfg* cfg, int32_t n_reads, const int32_t* read_lens);
/* FASTQ-file variants (read ids by first appearance of the name, graph.h:410-420). */
int gaml_hip_add_single_fastq(gaml_hip_ctx* ctx, const gaml_single_cfg* cfg, const char* fastq);
int gaml_hip_add_paired_fastq(gaml_hip_ctx* ctx, const gaml_paired_cfg* cfg, const char* fastq1, const char* fastq2);
int gaml_hip_add_pacbio_fastq(gaml_hip_ctx* ctx, const gaml_single_cfg* cfg, const char* fastq);

/* Read sharding for multi-GPU runs (new design): this context keeps and
 * scores only reads [n*rank/world, n*(rank+1)/world) of every read set. Call before adding
 * read sets. Partial results are combined with gaml_hip_combine_partials. */
int gaml_hip_set_shard(gaml_hip_ctx* ctx, int32_t rank, int32_t world);
/* Alternative: the caller already hands each process only its own reads (world processes in
 * all). Nothing is partitioned; the context only knows that window maxima must be exchanged
 * with the other processes (gaml_hip_eval_* below). */
int gaml_hip_set_presharded(gaml_hip_ctx* ctx, int32_t world);

/* Alignment records computed outside the library (the reference's external-aligner branch
 * graph.cc:924-1033 produces exactly these per sub-walk; BLASR output for PacBio,
 * graph.cc:2776-2782). mate = 0/1 for paired sets, 0 otherwise. read_id is global. */
int gaml_hip_put_window_records(gaml_hip_ctx* ctx, int readset, int mate, const int32_t* subpath, int32_t subpath_len,
                                const gaml_aligment* recs, int64_t n);
int gaml_hip_put_pacbio_records(gaml_hip_ctx* ctx, int readset, const int32_t* subpath, int32_t subpath_len,
                                const gaml_pacbio_aligment* recs, int64_t n);

/* ---- PacBio cache-miss side: BLASR's SAM output -> cached alignment records -------------------
 * The reference, on a path with an uncached sub-walk, writes the path to a file, runs BLASR and
 * turns every SAM line into a cached record (PacbioReadSet::GetReadProbabilitiesSlow
 * graph.cc:2650-2795): ParseAligment (:2945-3021), the banded sum-over-alignments probability
 * AligmentProbability (:2175-2297, on the GPU here) and the filing rule (:2760-2782).  Running
 * BLASR stays with the caller; these three entry points are the rest.
 *
 * gaml_hip_add_pacbio_reads: like gaml_hip_add_pacbio but keeps the read bases (read_seq_,
 *   PacbioReadSet::PreprocessReads graph.cc:1416-1439) and the read names (GetReadId graph.h:410-420);
 *   `names` = n names, each followed by '\n'.  Reads may not hold '\n' or '-'.
 * gaml_hip_pacbio_missing: the index ranges [begin, end] of `path` the reference would hand to
 *   BLASR (merged ranges of uncached sub-walks, GetReadProbabilities graph.cc:2438-2478); writes
 *   up to `cap` pairs to ranges_out and returns the number of ranges.
 * gaml_hip_pacbio_ingest_sam: `path` is the sub-path that was aligned (as given to BLASR:
 *   path string + separator + reverse complement), `sam` the SAM text ('@' lines are skipped).
 *   Every sub-walk of the path that was not cached before gets a cache entry; a record is filed
 *   under the sub-walk it spans exactly as the reference does.  Unknown read names and lines
 *   with fewer than 10 columns are errors (the reference asserts / reads out of range). */
int gaml_hip_add_pacbio_reads(gaml_hip_ctx* ctx, const gaml_single_cfg* cfg, int32_t n_reads, const char* bases,
                              const int64_t* offsets, const char* names);
int32_t gaml_hip_pacbio_missing(gaml_hip_ctx* ctx, int readset, const int32_t* path, int32_t path_len, int32_t* ranges_out,
                                int32_t cap);
int gaml_hip_pacbio_ingest_sam(gaml_hip_ctx* ctx, int readset, const int32_t* path, int32_t path_len, const char* sam,
                               int64_t sam_len, int64_t* filed_out);
/* cached records of one sub-walk (global read ids); -1 when the sub-walk is not cached */
int64_t gaml_hip_pacbio_records(gaml_hip_ctx* ctx, int readset, const int32_t* subpath, int32_t subpath_len,
                                gaml_pacbio_aligment* out, int64_t cap);
/* last ingest: {SAM records, DP jobs, DP rows, DP cells, kernel ms (HIP events), host parse+prepare ms,
 * upload+kernel+download ms, scratch bytes} */
int gaml_hip_pacbio_dp_stats(gaml_hip_ctx* ctx, int readset, double* out8);
/* ---- the hot path ------------------------------------------------------------------ */
/* ProbCalculator::CalcProb(paths, zeros, total_len) (prob_calculator.h:63-109):
 * paths = flattened node ids (>= 0) / gaps (< 0), path_offs[n_paths+1].
 * zeros_out: 2 ints per read set (low-probability reads, reads) in the reference's order:
 * single sets, then paired, then pacbio, each in creation order. May be NULL.
 * The value is a pure function of (paths, alignment-window cache): every call rescoring all
 * reads from scratch on the GPU (= the reference evaluated with a fresh ScoringState). */
int gaml_hip_calc_prob(gaml_hip_ctx* ctx, const int32_t* paths, const int64_t* path_offs, int32_t n_paths,
                       double* prob_out, int32_t* zeros_out, int32_t* total_len_out);

/* Sharded form: per read set 4 doubles {sum of log-probabilities over this shard's reads,
 * floored reads, bad_bases (valid on every rank), reads in shard}. After an all-reduce(sum)
 * of elements 0, 1 and 3 (element 2 is replicated: take any rank's), gaml_hip_combine_partials
 * gives CalcProb's value. n_sets = gaml_hip_num_readsets. */
int gaml_hip_calc_partials(gaml_hip_ctx* ctx, const int32_t* paths, const int64_t* path_offs, int32_t n_paths,
                           double* partials_out /* 4 * n_sets */, int32_t* total_len_out);
int gaml_hip_combine_partials(gaml_hip_ctx* ctx, const double* partials /* 4 * n_sets, reduced */,
                              int32_t total_len, double* prob_out, int32_t* zeros_out);

/* Two-phase form, REQUIRED for sharded contexts whenever new windows get aligned (cold path):
 * the reference drops an alignment whose path position is more than 5 below the largest position
 * seen at earlier nodes of the contig (graph.cc:577) -- a maximum over ALL reads, so shards must
 * exchange the largest record position of every newly aligned window once.
 *   gaml_hip_eval_begin          registration + alignment + window placement; *pending_out = number
 *                                of windows whose maxima need exchanging (always 0 when world == 1,
 *                                and 0 in a sharded run once the window cache is warm)
 *   gaml_hip_eval_pending_maxpos the local maxima, in an order that is identical on every rank
 *   (caller: all-reduce(max) over ranks)
 *   gaml_hip_eval_apply_maxpos   install the reduced maxima
 *   gaml_hip_eval_finish[_async] thresholds, device tables, kernels; partials as gaml_hip_calc_partials */
int gaml_hip_eval_begin(gaml_hip_ctx* ctx, const int32_t* paths, const int64_t* path_offs, int32_t n_paths,
                        int64_t* pending_out, int32_t* total_len_out);
int64_t gaml_hip_eval_pending_maxpos(gaml_hip_ctx* ctx, int32_t* out, int64_t cap);
int gaml_hip_eval_apply_maxpos(gaml_hip_ctx* ctx, const int32_t* reduced, int64_t n);
int gaml_hip_eval_finish(gaml_hip_ctx* ctx, double* partials_out /* 4 * n_sets */);
int gaml_hip_eval_finish_async(gaml_hip_ctx* ctx, void* d_partials, void* hip_stream);
/* wait for everything enqueued on the library's private stream */
int gaml_hip_sync(gaml_hip_ctx* ctx);

/* Single-node exchange of the partials through POSIX shared memory (new; the reference is one process). After a
 * BLOCKING evaluation (gaml_hip_eval_finish / gaml_hip_calc_partials) a rank's partials are host values; the ranks of
 * one node add them up here in ~1 us instead of sending them back through the device for an RCCL all-reduce of 32
 * bytes (~30 us of dependent dispatches). Every rank opens the same `name` (e.g. "/gaml_<port>") with its rank and
 * the world size -- rank 0 FIRST (it replaces whatever block of that name exists), the others after a barrier of the
 * caller's; _allreduce_sum is collective, sums in rank order (identical bits on every rank) and waits at most
 * 30 s for the others. Not for read sets with penalty_constant > 0 on a sharded context (those need the coverage
 * exchange of gaml_hip_eval_score_async). _close(unlink_name = 1) on one rank removes the name. */
int gaml_hip_shm_exchange_open(gaml_hip_ctx* ctx, const char* name, int32_t rank, int32_t world, int32_t cap_doubles);
int gaml_hip_shm_allreduce_sum(gaml_hip_ctx* ctx, double* inout, int32_t n_doubles);
int gaml_hip_shm_exchange_close(gaml_hip_ctx* ctx, int32_t unlink_name);

/* Device values -> host at the end of a stream-ordered sequence (after the all-reduce of the partials, say) without a
 * D2H copy command and without the runtime's completion wake-up: _async enqueues a one-block kernel on `hip_stream`
 * (NULL: the library's stream) that writes n_doubles values from d_src and then a sequence word into mapped pinned
 * memory; _wait polls that word (bounded; then hipStreamSynchronize) and copies the values out. One fetch in flight per
 * context. Nothing in the reference corresponds to it (single process, host arithmetic). */
int gaml_hip_fetch_async(gaml_hip_ctx* ctx, const void* d_src, int32_t n_doubles, void* hip_stream);
int gaml_hip_fetch_wait(gaml_hip_ctx* ctx, double* out, int32_t n_doubles);

/* Maintenance hint.  Windows aligned after the device record tables of a paired set were built are
 * scored from delta lists (slightly slower per pair); the library folds them into the tables by
 * itself when they grow past 1/8 of the pairs or after 64 evaluations without a new window.  This
 * call asks for the fold at the next evaluation -- e.g. after a warm-up phase, before a long run of
 * re-scoring.  Results do not change (only the order of the final sum, i.e. last bits). */
int gaml_hip_compact_tables(gaml_hip_ctx* ctx);

/* Sharded evaluation with a coverage penalty (penalty_constant > 0 on a paired set; SURVEY 8e "the one
 * non-separable piece").  bad_bases (graph.cc:1893-1919) is a function of the union of every rank's
 * well-aligned pair positions, so the sweep has to wait for the other ranks' coverage maps:
 *   n = gaml_hip_eval_score_async(ctx, d_partials, stream)   instead of gaml_hip_eval_finish_async:
 *       scoring kernels of all read sets; returns how many coverage maps await the exchange (0: done);
 *   for i < n:
 *     gaml_hip_eval_coverage_export_async(ctx, i, dst, cap, &bytes, stream)   copy this rank's map (one bit
 *         per path base, same size on every rank) into caller memory, e.g. a torch tensor (dst NULL: size only);
 *     all-gather the maps (RCCL);
 *     gaml_hip_eval_coverage_finish_async(ctx, i, maps, n_maps, contribute, stream)   OR the n_maps gathered
 *         maps into this rank's, run the sweep, store bad_bases into the partials: the value where
 *         `contribute` is non-zero (exactly one rank, e.g. rank 0), 0 elsewhere, so that the
 *         all-reduce(sum) of the partials counts it once.
 * Single-end sets need no exchange (their bad_bases is identically 0 in the reference, graph.cc:1701-1733).
 * PacBio sets with a penalty (graph.cc:3198-3250: sweep over the alignment intervals of ALL reads): after
 * gaml_hip_eval_score_async, for i < gaml_hip_eval_pacbio_pending(ctx):
 *     n = gaml_hip_eval_pacbio_intervals(ctx, i)   how many alignment intervals this rank's reads contribute
 *         (known on the host, no synchronisation);
 *     gaml_hip_eval_pacbio_export_async(ctx, i, dst, cap, stream)   copy them -- 16 bytes each: int32 {contig,
 *         begin, end, 0} in path coordinates -- into caller DEVICE memory with room for `cap` intervals;
 *     all-gather them (counts differ per rank: gather the counts first); then
 *     gaml_hip_eval_pacbio_finish_async(ctx, i, intervals, n_intervals, contribute, stream)   `intervals`: the
 *         n_intervals gathered intervals of all ranks (this rank's among them) in device memory; sorts them
 *         together with the contigs' node intervals, runs the sweep on the device and stores bad_bases into the
 *         partials like the paired form. No interval ever visits the host.
 * `stream` everywhere here: the stream the caller orders its own copies and collectives on. NULL is the legacy default
 * stream (what torch.cuda.current_stream().cuda_stream is on torch's default stream) and is used as such -- the
 * library's work is ordered against the caller's other work on it like on any other handle. */
int32_t gaml_hip_eval_score_async(gaml_hip_ctx* ctx, void* d_partials, void* stream);
int gaml_hip_eval_coverage_export_async(gaml_hip_ctx* ctx, int32_t i, void* dst, int64_t cap, int64_t* bytes_out, void* stream);
int gaml_hip_eval_coverage_finish_async(gaml_hip_ctx* ctx, int32_t i, const void* maps, int32_t n_maps, int32_t contribute,
                                        void* stream);
int32_t gaml_hip_eval_pacbio_pending(gaml_hip_ctx* ctx);
int64_t gaml_hip_eval_pacbio_intervals(gaml_hip_ctx* ctx, int32_t i);
int gaml_hip_eval_pacbio_export_async(gaml_hip_ctx* ctx, int32_t i, void* dst, int64_t cap, void* stream);
int gaml_hip_eval_pacbio_finish_async(gaml_hip_ctx* ctx, int32_t i, const void* intervals, int64_t n_intervals, int32_t contribute,
                                      void* stream);

/* Device-resident form for callers that already own a HIP stream (e.g. torch): enqueue the
 * whole evaluation on `stream` and leave the 4*n_sets partials in device memory at
 * d_partials (f64). No host synchronisation. `hip_stream`: the stream the caller orders its own work
 * on; NULL is the legacy default stream (gaml_hip_sync waits for it as well as for the library's own). */
int gaml_hip_calc_partials_async(gaml_hip_ctx* ctx, const int32_t* paths, const int64_t* path_offs, int32_t n_paths,
                                 void* d_partials, void* hip_stream, int32_t* total_len_out);

/* Batched speculative scoring.  The move generators evaluate several near-identical
 * path sets and keep the best (moves.cc:107-113 LocalChange2, 694-800 FixGapLength, 1156-1305
 * FixRepForNode2): n_sets independent CalcProb calls whose results are only compared afterwards.
 * This entry point takes them in one call: the evaluations are enqueued back to back on the
 * library's stream, the host prepares set i+1 while the device scores set i, and there is ONE
 * synchronisation and ONE device->host copy for the whole batch.  Results (and the window cache
 * afterwards) are those of n_sets gaml_hip_calc_prob calls in the same order.
 * A context of paired sets and / or PacBio sets without coverage penalty (BASELINE config 4: paired + PacBio) scores up
 * to 8 path sets per pass over the records instead: per chunk one launch per paired set over its records and one per
 * PacBio set over its cached alignments (occurrence counts of all sets of the chunk side by side per sub-walk), one wait.
 * Same values bit for bit, same gaml_hip_read_probs / gaml_hip_bad_bases / gaml_hip_pacbio_stats afterwards. A PacBio set
 * with a coverage penalty keeps the whole context on the path described above, unless the context's switch is on
 * (gaml_hip_set_pacbio_penalty_onepass, off by default): then such a set goes along too, its chunk sweeping every path it
 * has no bad_bases for yet once, one contig per block (gaml_hip_pacbio_penalty_stats counts). A single-end set keeps the
 * context on that path as well, unless the context's switch is on (gaml_hip_set_single_onepass, off by default): then a single-end set goes along as well, one launch
 * per set and chunk over its read-major records with the occurrence tables of all sets of the chunk side by side
 * (gaml_hip_single_stats counts the chunks). Same values bit for bit with the switch on or off.
 *   paths / path_offs : all paths of all sets, concatenated (path k = paths[path_offs[k] .. path_offs[k+1]))
 *   set_offs[n_sets+1]: set i = paths set_offs[i] .. set_offs[i+1]-1
 *   probs_out[n_sets]; zeros_out[n_sets * 2 * num_readsets] and total_lens_out[n_sets] may be NULL.
 * Not for sharded contexts (GAML_HIP_ESTATE): there the batch is a loop over the gaml_hip_eval_*
 * protocol with one all-reduce over all sets' partials (gaml_amd/dist.py: ShardedScorer.calc_prob_batch). */
int gaml_hip_calc_prob_batch(gaml_hip_ctx* ctx, int32_t n_sets, const int32_t* paths, const int64_t* path_offs,
                             const int32_t* set_offs, double* probs_out, int32_t* zeros_out, int32_t* total_lens_out);
/* gaml_hip_set_single_onepass / gaml_hip_get_single_onepass: may single-end sets go along on the one-pass routes of
 * gaml_hip_calc_prob_batch (1) or does a single-end set keep its context on the sequential path (0, the default). Per
 * context, any kind of context: in-process multi-device and rank-per-process contexts only keep the flag (their batches
 * go other ways). A new context starts with 1 when the environment holds GAML_HIP_SINGLE_BATCH=onepass. Same values
 * either way; the gap-length search of such a context runs on its fallback, whose batches follow the switch. */
int gaml_hip_set_single_onepass(gaml_hip_ctx* ctx, int32_t on);
int gaml_hip_get_single_onepass(const gaml_hip_ctx* ctx);
/* gaml_hip_set_pacbio_penalty_onepass / gaml_hip_get_pacbio_penalty_onepass: may PacBio sets with a coverage penalty go along
 * on the one-pass routes of gaml_hip_calc_prob_batch (1) or does such a set keep its context on the sequential path (0, the
 * default). Per context, any kind of context: host-only, in-process multi-device and rank-per-process contexts only keep the
 * flag (their batches go other ways). A new context starts with 1 when the environment holds
 * GAML_HIP_PACBIO_PENALTY_BATCH=onepass. Same values bit for bit either way, same gaml_hip_read_probs / gaml_hip_bad_bases /
 * gaml_hip_pacbio_stats afterwards; the gap-length search of such a context runs on its fallback, whose batches follow the
 * switch. With it on, bad_bases of a path set is the sum of its paths' values (CalcScoreForPacbio sweeps every path on its
 * own): a chunk sweeps each distinct path it has no value for once and keeps the value with the path's memo entry until
 * the record cache changes.
 * gaml_hip_pacbio_penalty_stats: cumulative out4 = {chunks this set scored with its penalty on the one-pass routes, contigs
 * swept one per block, contigs swept through the general chain (more intervals than a block takes), distinct paths of a
 * chunk whose value the memo had}. GAML_HIP_EINVAL for a handle that is not a PacBio set; zeros on a host-only context;
 * a multi-device context reports its first shard. */
int gaml_hip_set_pacbio_penalty_onepass(gaml_hip_ctx* ctx, int32_t on);
int gaml_hip_get_pacbio_penalty_onepass(const gaml_hip_ctx* ctx);
int gaml_hip_pacbio_penalty_stats(gaml_hip_ctx* ctx, int readset, int64_t* out4);
/* gaml_hip_set_single_device / gaml_hip_get_single_device: are the windows of single-end sets aligned on the device, one
 * batch per path set that brings new ones, and their read-major record tables built there by kernels from a mirror of the
 * host's record pool (1), or does the host align window by window and build and upload the whole table whenever a window
 * joins (0, the default). Per context, settable at any time, effective from the next evaluation; the table is rebuilt on
 * the other route after a flip. Served on plain single-device contexts: host-only, in-process multi-device and
 * rank-per-process contexts only keep the flag and stay on the host route. A new context starts with 1 when the
 * environment holds GAML_HIP_SINGLE_DEVICE=1. Same records, same tables, same values bit for bit either way. */
int gaml_hip_set_single_device(gaml_hip_ctx* ctx, int32_t on);
int gaml_hip_get_single_device(const gaml_hip_ctx* ctx);


/* ---- the advice move of a paired set (ExtendPathsAdv moves.cc:933-998) -------------------------------------------
 * gaml_hip_advice_build: ReadSet::BuildAdviceIndex (graph.cc:323-342) on mate 2 -- registers (and aligns) the one-node
 *   window of every node longer than `threshold` and inverts their records into a per-pair list of nodes. Runs once per
 *   read set: a later call with another threshold does nothing. Paired sets only (else GAML_HIP_EINVAL).
 * gaml_hip_advice_index: that index; pair r's entries are entries[offs[r] .. offs[r+1]), each node << 1 | orient1
 *   (orient1: the pair's first record in the node's window has orientation 1, i.e. the node is in GetAdviceIndex1),
 *   nodes ascending. offs: n_pairs + 1; writes at most `cap` entries, returns their total (GAML_HIP_ESTATE: not built).
 * gaml_hip_advice_candidates: `cands` of moves.cc:956-986 for a path the caller has already reversed if it wanted to:
 *   registers the mate-1 windows GetSubpathsFromPath names (rs1.GetPositions graph.cc:651-712), keeps the pairs whose
 *   first slot has orientation 0, and lists their GetAdviceIndex1 nodes that pass `flags` -- ONLY_OUT: skip nodes of the
 *   path and their twins; ALLOW_GAPS: keep every node, else only those in `reach` (the keys of reach_limit_[path.back()]).
 *   Pairs ascending, duplicates kept: the list equals the reference's element for element. Writes at most `cap` entries,
 *   returns the count. The retry with ALLOW_GAPS on an empty list (moves.cc:975-987) is the caller's.
 * Single-device, in-process multi-device and host-only contexts; rank-per-process contexts get GAML_HIP_ESTATE. */
#define GAML_HIP_ADVICE_ONLY_OUT 1
#define GAML_HIP_ADVICE_ALLOW_GAPS 2
int gaml_hip_advice_build(gaml_hip_ctx* ctx, int readset, int32_t threshold);
int64_t gaml_hip_advice_index(gaml_hip_ctx* ctx, int readset, int64_t* offs /* n_pairs + 1 */, int32_t* entries, int64_t cap);
int64_t gaml_hip_advice_candidates(gaml_hip_ctx* ctx, int readset, const int32_t* path, int32_t path_len, const int32_t* reach,
                                   int32_t n_reach, int32_t flags, int32_t* out, int64_t cap);

/* ---- the gap-length search (FixGapLength moves.cc:694-800) ----------------------------------------------------------
 * gaml_hip_gap_profile: probs_out[k] is what gaml_hip_calc_prob returns for `paths` with entry `gap_pos` of path `path_id`
 *   (a gap: negative) set to -lens[k]; zeros_out (n_lens * 2 * num_readsets) and total_lens_out (n_lens) may be NULL.
 *   A gap's length changes where the windows behind it sit and 2T, nothing else: a context of paired sets without
 *   coverage penalty on a large-BAR device plans the set once, with lens[0], derives every other length's tables from
 *   the resident ones on the device and scores up to 8 lengths per pass over the records. Every other context (other
 *   kinds of read sets, a penalty, no memo, several devices, rank-per-process -- there the call is collective) runs the
 *   lengths through gaml_hip_calc_prob_batch / gaml_hip_calc_prob: same values. A set with a coverage penalty takes the
 *   device route too once gaml_hip_set_gap_penalty_device says so (every length's coverage layout is then derived on the
 *   device beside its tables; a length whose bitmap would not fit int32 bits sends the call to the fallback).
 *   GAML_HIP_EINVAL: path_id or gap_pos
 *   out of range, an entry that is not a gap, a length < 1, n_lens < 0, a total length beyond int32. n_lens == 0 does
 *   nothing. Afterwards the library's tables describe the set with lens[0].
 * gaml_hip_fix_gap_length: FixGapLength(paths, path_id, gap_pos, prob_calc, prev_len) -- *len_out is the length the
 *   reference leaves in paths[path_id][gap_pos] (the caller stores -*len_out there). The trace is the reference's sequence
 *   of CalcProb evaluations as (length, value), in its order: at most trace_cap are written, *n_trace_out (may be NULL)
 *   is their number. The values come from gap profiles of up to 8 lengths chosen before they are needed (the first
 *   probes with the doubling bounds, a ternary step with both possible next steps), so the search costs a few passes,
 *   not one blocking call per evaluation; where the profile takes its fallback nothing is computed ahead.
 *   GAML_HIP_EINVAL also when the search reaches a length whose total would not fit int32.
 * gaml_hip_gap_stats: cumulative {profile calls (the search's included), lengths scored on the device route, lengths
 *   scored on the fallback, device passes}.
 * gaml_hip_set_gap_penalty_device / gaml_hip_get_gap_penalty_device: may paired sets with a coverage penalty take the
 *   device route (1) or not (0, the default). Per context, any kind of context: one the device route never serves only
 *   keeps the flag. A new context starts with 1 when the environment holds GAML_HIP_GAP_PENALTY=device. Same values on
 *   both routes.
 * gaml_hip_set_gap_mixed_device / gaml_hip_get_gap_mixed_device: may a context that holds single-end sets and / or PacBio
 *   sets without a coverage penalty -- beside paired sets or on their own -- take the device route (1) or not (0, the
 *   default). With 1 a profile builds ONE single-end occurrence table on the host (the set with lens[0]) and derives every
 *   other length's on the device, enumerates the edited path's PacBio sub-walks once and per length only those that contain
 *   the gap entry, and scores up to 8 lengths per pass with the batch's multi-set kernels; it does not depend on
 *   gaml_hip_set_single_onepass. What takes which route with the switch on: paired, single-end and unpenalised PacBio sets
 *   the device route; a PacBio set with penalty_constant > 0 (whatever gaml_hip_set_pacbio_penalty_onepass says), a
 *   penalised paired set without gaml_hip_set_gap_penalty_device, several devices, rank-per-process and host-only contexts
 *   the fallback. Per context, any kind of context: one the device route never serves only keeps the flag. A new context
 *   starts with 1 when the environment holds GAML_HIP_GAP_MIXED=device. Same values on both routes; a PacBio set's `misses`
 *   (gaml_hip_pacbio_stats) count every length a pass scored, those scored ahead of the search included. */
int gaml_hip_gap_profile(gaml_hip_ctx* ctx, const int32_t* paths, const int64_t* path_offs, int32_t n_paths,
                         int32_t path_id, int32_t gap_pos, const int32_t* lens, int32_t n_lens,
                         double* probs_out, int32_t* zeros_out /* n_lens * 2 * num_readsets, may be NULL */,
                         int32_t* total_lens_out /* may be NULL */);
int gaml_hip_fix_gap_length(gaml_hip_ctx* ctx, const int32_t* paths, const int64_t* path_offs, int32_t n_paths,
                            int32_t path_id, int32_t gap_pos, int32_t* len_out,
                            int32_t* trace_lens, double* trace_probs, int32_t trace_cap, int32_t* n_trace_out);
int gaml_hip_gap_stats(gaml_hip_ctx* ctx, int64_t* out4);
int gaml_hip_set_gap_penalty_device(gaml_hip_ctx* ctx, int32_t on);
int gaml_hip_get_gap_penalty_device(const gaml_hip_ctx* ctx);
int gaml_hip_set_gap_mixed_device(gaml_hip_ctx* ctx, int32_t on);
int gaml_hip_get_gap_mixed_device(const gaml_hip_ctx* ctx);

/* ---- introspection (tests, bench, logging) ----------------------------------------- */
int gaml_hip_num_readsets(const gaml_hip_ctx* ctx);
int gaml_hip_readset_kind(const gaml_hip_ctx* ctx, int readset);   /* 0 single, 1 paired, 2 pacbio */
int64_t gaml_hip_readset_reads(const gaml_hip_ctx* ctx, int readset); /* global read (pair) count */
int32_t gaml_hip_num_nodes(const gaml_hip_ctx* ctx);
int32_t gaml_hip_node_len(const gaml_hip_ctx* ctx, int32_t node);
/* per-read values of the last evaluation of a read set: probs (linear; log for pacbio),
 * n = reads in this shard. ScoringState::probs (graph.h:612-619) for paired sets. */
int gaml_hip_read_probs(gaml_hip_ctx* ctx, int readset, double* out, int64_t n);
/* bad_bases of the last evaluation (graph.cc:1893-1919 / 1701-1733 / 3226-3250). */
int gaml_hip_bad_bases(gaml_hip_ctx* ctx, int readset, int64_t* out);
/* alignment-window cache (aligment_cache_, graph.h:427): number of windows, and the sorted
 * records of one window (returns count, -1 if the window is not cached). */
int64_t gaml_hip_window_count(const gaml_hip_ctx* ctx, int readset, int mate);
int64_t gaml_hip_window_records(gaml_hip_ctx* ctx, int readset, int mate, const int32_t* subpath, int32_t subpath_len,
                                gaml_aligment* out, int64_t cap);
/* force alignment of one window with the library's own aligner (AlignSubpathInternal graph.cc:839-899) */
int64_t gaml_hip_align_window(gaml_hip_ctx* ctx, int readset, int mate, const int32_t* subpath, int32_t subpath_len);
/* GPU window aligner (cold path): windows aligned on the device so far, seed candidates extended, wall time.
 * The device aligns the windows of a paired set's mate whose reads have at most 510 bases and whose indexed read
 * length is at least 16; every other mate, single-end sets and host-only contexts are served by the library's host
 * aligner with identical records, and do not count here -- counters that stay at zero mean the host aligner ran. A
 * single-end set whose reads fit the same bounds counts here as well when its context's switch is on
 * (gaml_hip_set_single_device): its windows then go to the device in batches.
 * (Development builds: GAML_HIP_KNOB_ALIGNER_ROUTE = GAML_HIP_ALIGNER_HOST, gaml_hip_debug.h, forces the host aligner.) */
int gaml_hip_aligner_stats(gaml_hip_ctx* ctx, int64_t* windows, int64_t* candidates, double* microseconds);
/* the same time by stage, host clock, cumulative: out6 = {window strings + upload, spans + candidates (small batches: the
 * whole device pipeline up to the published headers), extension, hits to the host, ordering + filing on the host, batches} */
int gaml_hip_aligner_stages(gaml_hip_ctx* ctx, double* out6);
/* ---- monitoring (what bench.py prints beside its numbers; all cheap, host-side) --------------------------------- */
/* pairs per record-count class of a paired set's device tables {<= 1 record per mate, <= 2, <= 4, more} */
int gaml_hip_pair_classes(gaml_hip_ctx* ctx, int readset, int64_t* out4);
/* device record tables of a paired set (built and maintained by kernels: the records never leave the device): {table
 * builds, delta updates, pairs currently on the delta lists, builds that ran BESIDE the evaluations on a stream of their
 * own and took over a fixed number of evaluations later (of the table builds), gaml_hip_calc_prob_batch chunks whose per-set tables were built on
 * the device from patches, chunks whose tables were written whole, records of mate 1 / mate 2 that the current tables
 * leave out because another record of the same read always overwrites them, such records of windows that joined later
 * and therefore never reached the delta lists (since creation), pairs of the compact class whose pair term came with
 * the tables (both records in one window, or a mate without alignment)} */
int gaml_hip_table_stats(gaml_hip_ctx* ctx, int readset, int64_t* out10);
/* record cache of a PacBio set: {cached sub-walks, cached records (this shard's reads), sub-walk lookups of the evaluations
 * so far that found nothing cached (cumulative; the reference would run BLASR there), gaml_hip_calc_prob_batch chunks the
 * set scored in one multi-set launch}. Host-only contexts too; GAML_HIP_EINVAL for a handle that is not a PacBio set. A
 * multi-device context reports its first shard, like gaml_hip_table_stats. A gap profile on the mixed device route
 * (gaml_hip_set_gap_mixed_device) counts a pass as one such launch, and the lookups of every length a pass scored --
 * those scored ahead of the search included, which the fallback never scores. */
int gaml_hip_pacbio_stats(gaml_hip_ctx* ctx, int readset, int64_t* out4);
/* a single-end set: {windows registered, records in the read-major table (those of the windows some scored path set has
 * named; this shard's reads), bytes of occurrence tables staged by the last call or chunk, gaml_hip_calc_prob_batch chunks
 * the set scored in one multi-set launch}. Host-only contexts too; GAML_HIP_EINVAL for a handle that is not a single-end
 * set. A multi-device context reports its first shard, like gaml_hip_pacbio_stats. */
int gaml_hip_single_stats(gaml_hip_ctx* ctx, int readset, int64_t* out4);
/* the device route of a single-end set (gaml_hip_set_single_device): {windows of this set aligned by the device aligner,
 * read-major tables built on the device, records copied into the device's mirror of the record pool, tables built on the
 * host (the route of a context whose switch is off)}, all cumulative. Host-only contexts too (the first three stay 0);
 * GAML_HIP_EINVAL for a handle that is not a single-end set. A multi-device context reports its first shard. */
int gaml_hip_single_device_stats(gaml_hip_ctx* ctx, int readset, int64_t* out4);
/* host-side phase times of the last blocking paired evaluation, microseconds: [0] pass 1 (planner; includes [2]),
 * [1] thresholds + occurrence tables, [2] alignment of newly registered windows (inside pass 1), [3] per-call tables
 * written, [4] record tables / delta lists brought up to date, [5] kernel launches, [6] bytes of per-call tables
 * written (a call whose tables the device built: memo entries uploaded + thresholds; a set with a coverage penalty: plus
 * its coverage bitmap layout, which is written whole per call), [7] wait for the device */
int gaml_hip_last_phases(gaml_hip_ctx* ctx, double* out8);
/* timing of the last scoring call, microseconds: [0] host preparation (window registration,
 * alignment of new windows, occurrence tables), [1] H2D + kernels + D2H wall, [2] device time
 * of the scoring kernels measured with HIP events on the library's stream (0 if events off). */
int gaml_hip_last_timing(const gaml_hip_ctx* ctx, double* out3);
/* HIP event timing of the dominant kernel (default off): on = 1 times every scoring launch, on = k > 1
 * every k-th. The two events are attached to the dispatch itself (hipExtLaunchKernelGGL), so they hold the
 * kernel's own begin / end stamps -- what rocprofv3's kernel trace reports -- at ~4 us of extra host time per
 * timed launch; sampling keeps that out of a throughput measurement. gaml_hip_kernel_stats then describes the
 * timed launches (count, summed device time, summed algorithmic bytes). */
int gaml_hip_set_event_timing(gaml_hip_ctx* ctx, int on);
/* cumulative kernel statistics since the last reset: launches, total device microseconds
 * (HIP events), algorithmic bytes streamed (SURVEY.md 8d accounting). */
int gaml_hip_kernel_stats(gaml_hip_ctx* ctx, int reset, int64_t* launches, double* device_us, double* algo_bytes);

#ifdef __cplusplus
}
#endif
#endif /* GAML_HIP_H_ */
