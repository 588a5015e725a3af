// single_batch.hip.h -- the single-end side of gaml_hip_calc_prob_batch's one-pass routes (paired_batch.hip.h), taken only
// where the context says so (gaml_hip_set_single_onepass): per chunk of up to kMaxSets path sets and per single-end set the
// sets' occurrence tables side by side in one arena, one upload, one dispatch of single_score_multi_kernel
// (one translation unit with gaml_hip.hip, which includes this file behind single_launch.hip.h)
//
//   SgChunk               a chunk's single-end launches: nothing reaches the sets' bookkeeping until the chunk stands
//   single_chunk_launch   register + align every set's windows in order, then build every set's table over the FINAL window
//                         count, stage them into one slot, launch
//   single_chunk_collect  after the route's wait: the partials into their slots, the chunk counted
#pragma once

std::vector<int> slots_of_kind(const gaml_hip_ctx* c, int kind);  // pacbio_batch.hip.h

// A route may give its chunk up after this launch (patched -> full tables -> sequential): the route that takes over scores
// the sets again (registering a window twice is a lookup), and overwrites the per-read values. The device is waited for
// first: the staging slot and the arena are reused without an event inside a blocking call.
struct SgChunk {
  gaml_hip_ctx* c;
  bool launched = false, collected = false;
  std::vector<int64_t> table_bytes;  // per single-end set: what the chunk staged (gaml_hip_single_stats), held back like the count
  explicit SgChunk(gaml_hip_ctx* ctx) : c(ctx) {}
  ~SgChunk() { if (launched && !collected) (void)hipStreamSynchronize(c->stream); }
  SgChunk(const SgChunk&) = delete;
};

// Depends on the paths alone, so it goes out before the host plans the paired sets: the kernel runs under that planning.
// Paths eval_begin would refuse launch nothing (eval_begin reports them when the route gets there).
int single_chunk_launch(gaml_hip_ctx* c, SgChunk& ch, int n, const int32_t* paths, const int64_t* offs, const int32_t* set_offs) {
  if (c->singles.empty() || !c->have_graph || n <= 0 || n > kMaxSets) return 0;
  for (int32_t p = set_offs[0]; p < set_offs[n]; p++) {
    if (offs[p + 1] < offs[p]) return 0;
    for (int64_t q = offs[p]; q < offs[p + 1]; q++) if (paths[q] >= c->g.n()) return 0;
  }
  hipStream_t st = c->stream;
  std::vector<std::vector<Walk>> sets((size_t)n);
  for (int k = 0; k < n; k++)
    for (int32_t p = set_offs[k]; p < set_offs[k + 1]; p++) sets[(size_t)k].emplace_back(paths + offs[p], paths + offs[p + 1]);
  ch.table_bytes.assign(c->singles.size(), 0);
  for (size_t j = 0; j < c->singles.size(); j++) {
    SingleSet& s = *c->singles[j];
    SgMulti& M = s.multi;
    if (int e = single_init_dev(c, s)) return e;
    // every set's windows first, in the order sequential calls would register and align them: a window a later set adds
    // must read as absent in the earlier sets' tables, so the tables are built over the final window count
    std::vector<Occ> occs[kMaxSets];
    int32_t tl[kMaxSets];
    for (int k = 0; k < n; k++) if (int e = prepare_single_host(c, s, sets[(size_t)k], occs[k], &tl[k])) return e;  // (s.last_occ: the last set's)
    OccTable occ[kMaxSets];
    OccLayout lay[kMaxSets];
    size_t at = 0;
    for (int k = 0; k < n; k++) {
      build_occ_table(s.mate.wins.size(), occs[k], occ[k]);
      lay[k] = layout_occ(occ[k], at);  // (every offset of a layout is 16-byte aligned)
      at = lay[k].end;
    }
    if (int e = single_sync_records(c, s, st)) return e;
    void* host = nullptr;
    const int slot = stage_acquire(c, s.stage, at, &host);
    if (slot < 0) return slot;
    for (int k = 0; k < n; k++) pack_occ(occ[k], lay[k], (char*)host);
    if (at > s.occ_arena.cap) { HIP_TRY(c, hipStreamSynchronize(st)); HIP_TRY(c, s.occ_arena.reserve(at)); }
    if (int e = stage_upload(c, s.stage, slot, s.occ_arena.p, at, st)) return e;
    if (int e = stage_release(c, s.stage, slot, st)) return e;
    ch.table_bytes[j] = (int64_t)at;
    if (!M.ticket.p) {
      HIP_TRY(c, M.part_sum.reserve((size_t)kMaxSets * kMaxBlocks * sizeof(double)));
      HIP_TRY(c, M.part_zero.reserve((size_t)kMaxSets * kMaxBlocks * sizeof(int)));
      HIP_TRY(c, M.out.reserve((size_t)kMaxSets * 4 * sizeof(double)));
      HIP_TRY(c, M.ticket.reserve(kTicketWords * sizeof(unsigned)));
      HIP_TRY(c, hipMemset(M.ticket.p, 0, kTicketWords * sizeof(unsigned)));
      HIP_TRY(c, hipDeviceSynchronize());  // the scoring stream is non-blocking: make the zeroes land first
    }
    ch.launched = true;
    const int64_t n_reads = s.mate.n_local();
    if (n_reads == 0) { memset(M.out.p, 0, (size_t)kMaxSets * 4 * sizeof(double)); continue; }  // (what launch_single leaves: four zeroes)
    SingleMultiArgs a;
    const MateView v0 = view_of(s.dev, (const char*)s.occ_arena.p, lay[0]);
    a.first = v0.first; a.extra = v0.extra; a.mism_pow = v0.mism_pow; a.match_pow = v0.match_pow;
    a.lens = s.lens.as<int>();
    a.floor_tab = s.tabs.as<double>();
    a.logfloor_tab = s.tabs.as<double>() + s.mate.max_len + 1;
    a.n = (int)n_reads; a.n_sets = n;
    for (int k = 0; k < kMaxSets; k++) {  // (the slots behind n_sets repeat the last set's: never read)
      const MateView v = view_of(s.dev, (const char*)s.occ_arena.p, lay[std::min(k, n - 1)]);
      a.occ[k] = v.occ; a.multi_off[k] = v.multi_off; a.multi[k] = v.multi;
      const int32_t t = tl[std::min(k, n - 1)];
      a.two_T[k] = (double)(2 * (t == 0 ? 1 : t));
    }
    a.probs = s.probs.as<double>();
    const int grid = GRID_FOR(c, n_reads);  // single_score_kernel's grid
    a.part_sum = M.part_sum.as<double>(); a.part_zero = M.part_zero.as<int>(); a.part_stride = grid;
    a.ticket = M.ticket.as<unsigned>();
    a.out = (double*)M.out.dev;
    a.n_reads = (double)n_reads;
    EventPair* ev = nullptr;
    if (c->event_timing && (c->event_tick++ % c->event_every) == 0) { if (int e = take_events(c, &ev)) return e; }
    hipExtLaunchKernelGGL(single_score_multi_kernel, dim3((unsigned)grid), dim3(kBlock), 0, st, ev ? ev->first : nullptr, ev ? ev->second : nullptr, 0, a);
    HIP_TRY(c, hipGetLastError());
    if (!c->event_timing || ev) {
      // the records once (16 per record), the sets' tables, and per read its length (4) + the last set's value (8)
      c->stat_algo_bytes += 16.0 * (double)s.rm.total_records + (double)at + 12.0 * (double)n_reads;
      c->stat_launches++;
    }
  }
  return 0;
}

// after the route's wait: partials_out[(k * read sets + slot) * 4 ..] = {sum, floored, 0, reads} of path set k
int single_chunk_collect(gaml_hip_ctx* c, SgChunk& ch, int n, double* partials_out) {
  if (c->singles.empty()) return 0;
  if (!ch.launched) return fail(c, GAML_HIP_ESTATE, "batch: the chunk's single-end launch is missing");
  const size_t ns = c->handles.size();
  const std::vector<int> slot = slots_of_kind(c, 0);
  for (size_t j = 0; j < c->singles.size(); j++) {
    SingleSet& s = *c->singles[j];
    const double* res = (const double*)s.multi.out.p;
    for (int k = 0; k < n; k++) memcpy(partials_out + ((size_t)k * ns + (size_t)slot[j]) * 4, res + 4 * k, 4 * sizeof(double));
    s.table_bytes = ch.table_bytes[j];
    s.multi.launches++;
  }
  ch.collected = true;
  return 0;
}
