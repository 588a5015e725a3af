// pacbio_batch.hip.h -- the PacBio side of gaml_hip_calc_prob_batch's one-pass routes (paired_batch.hip.h): per chunk of up
// to kMaxSets path sets and per PacBio set one table of occurrence counts, one upload, one dispatch of
// pacbio_score_multi_kernel
// (one translation unit with gaml_hip.hip, which includes this file behind pacbio_launch.hip.h)
//
//   slots_of_kind         where combine() expects the partials of the sets of one kind (scoring_order)
//   PbChunk               a chunk's PacBio launches: what they would add to the bookkeeping, held back until the chunk stands
//   pacbio_chunk_launch   enumerate every path once (memo by path), build [sub-walk][kMaxSets], stage, launch
//   pacbio_chunk_collect  after the route's wait: the partials into their slots, the bookkeeping of n sequential calls
#pragma once

// handle index (c->paireds / c->pacbios) -> slot of the set's four partials in one path set's results
std::vector<int> slots_of_kind(const gaml_hip_ctx* c, int kind) {
  std::vector<int> slot(kind == 1 ? c->paireds.size() : kind == 2 ? c->pacbios.size() : c->singles.size(), 0);
  auto order = scoring_order(c);
  for (size_t k = 0; k < order.size(); k++) if (order[k].kind == kind) slot[(size_t)order[k].idx] = (int)k;
  return slot;
}

// A route may give its chunk up after the PacBio launch: the route that takes over scores the sets again, so nothing of
// this launch may have reached the set's bookkeeping by then (misses would count twice). The per-read values the kernel
// wrote are overwritten by the launch that takes over; the device is waited for first (the staging slot and the count
// table are reused without an event inside a blocking call).
struct PbChunk {
  gaml_hip_ctx* c;
  bool launched = false, collected = false;
  std::vector<int64_t> misses;  // per PacBio set: lookups that missed, over all sets of the chunk
  explicit PbChunk(gaml_hip_ctx* ctx) : c(ctx) {}
  ~PbChunk() { if (launched && !collected) (void)hipStreamSynchronize(c->stream); }
  PbChunk(const PbChunk&) = delete;
};

// Depends on the paths alone, so it goes out before the host plans the paired sets: the kernel runs under that planning.
// Paths eval_begin would refuse launch nothing (eval_begin reports them when the route gets there).
int pacbio_chunk_launch(gaml_hip_ctx* c, PbChunk& ch, int n, const int32_t* paths, const int64_t* offs, const int32_t* set_offs) {
  if (c->pacbios.empty() || !c->have_graph || n <= 0 || n > kMaxSets) return 0;
  for (int32_t p = set_offs[0]; p < set_offs[n]; p++) {
    if (offs[p + 1] < offs[p]) return 0;
    for (int64_t q = offs[p]; q < offs[p + 1]; q++) if (paths[q] >= c->g.n()) return 0;
  }
  hipStream_t st = c->stream;
  ch.misses.assign(c->pacbios.size(), 0);
  Walk path;
  for (size_t j = 0; j < c->pacbios.size(); j++) {
    PacbioSet& s = *c->pacbios[j];
    PbMulti& M = s.multi;
    const int64_t n_reads = s.hi - s.lo;
    if (int e = pacbio_init_dev(c, s)) return e;
    // candidates share all but one or two paths, with each other and with the chunks before: a path is enumerated once
    // per state of the record cache
    if (M.memo_generation != s.generation || M.memo.size() > 8192) { M.memo.clear(); M.memo_generation = s.generation; }
    const size_t n_walks = s.recs.size();
    const size_t bytes = align16(std::max<size_t>(1, n_walks) * kMaxSets * sizeof(int32_t));
    void* host = nullptr;
    const int slot = stage_acquire(c, s.stage, bytes, &host);
    if (slot < 0) return slot;
    int32_t* table = (int32_t*)host;
    memset(table, 0, bytes);
    for (int k = 0; k < n; k++)
      for (int32_t p = set_offs[k]; p < set_offs[k + 1]; p++) {
        path.assign(paths + offs[p], paths + offs[p + 1]);
        for (auto& x : path) if (x >= 0) x = c->g.norm[x];  // NormalizePath graph.h:268-273
        auto it = M.memo.find(path);
        if (it == M.memo.end()) {
          it = M.memo.emplace(path, PbEnum()).first;
          pacbio_enumerate(c, s, path, it->second);
        }
        ch.misses[j] += it->second.misses;
        for (const PbHit& h : it->second.hits) table[(size_t)h.walk * kMaxSets + k]++;
      }
    if (int e = pacbio_sync_records(c, s, st)) return e;
    if (!M.ticket.p) {
      HIP_TRY(c, M.part_sum.reserve((size_t)kMaxSets * kMaxBlocks * sizeof(double)));
      HIP_TRY(c, M.part_zero.reserve((size_t)kMaxSets * kMaxBlocks * sizeof(int)));
      HIP_TRY(c, M.out.reserve((size_t)kMaxSets * 4 * sizeof(double)));
      HIP_TRY(c, M.ticket.reserve(kTicketWords * sizeof(unsigned)));
      HIP_TRY(c, hipMemset(M.ticket.p, 0, kTicketWords * sizeof(unsigned)));
      HIP_TRY(c, hipDeviceSynchronize());  // the scoring stream is non-blocking: make the zeroes land first
    }
    if (bytes > M.count.cap) { HIP_TRY(c, hipStreamSynchronize(st)); HIP_TRY(c, M.count.reserve(bytes)); }
    if (int e = stage_upload(c, s.stage, slot, M.count.p, bytes, st)) return e;
    if (int e = stage_release(c, s.stage, slot, st)) return e;
    ch.launched = true;
    if (n_reads == 0) { memset(M.out.p, 0, (size_t)kMaxSets * 4 * sizeof(double)); continue; }  // (what launch_pacbio leaves: four zeroes)
    PacbioMultiArgs a;
    a.rec_off = s.rec_off.as<int>(); a.rec_walk = s.rec_walk.as<int>(); a.rec_logp = s.rec_logp.as<double>();
    a.counts = M.count.as<int>(); a.lens = s.d_lens.as<int>();
    a.floor_a = std::log(std::exp(s.cfg.min_prob_start));     // logdouble(exp(c)) graph.cc:3075
    a.floor_b = std::log(std::exp(s.cfg.min_prob_per_base));  // logdouble(exp(k))
    a.n = (int)n_reads; a.n_sets = n;
    a.logprobs = s.logprobs.as<double>();
    const int grid = GRID_FOR(c, n_reads * 64);  // one wave per read: pacbio_score_kernel's grid
    a.part_sum = M.part_sum.as<double>(); a.part_zero = M.part_zero.as<int>(); a.part_stride = grid;
    a.ticket = M.ticket.as<unsigned>();
    a.out = (double*)M.out.dev;
    a.n_reads = (double)n_reads;
    EventPair* ev = nullptr;
    if (c->event_timing && (c->event_tick++ % c->event_every) == 0) { if (int e = take_events(c, &ev)) return e; }
    hipExtLaunchKernelGGL(pacbio_score_multi_kernel, dim3((unsigned)grid), dim3(kBlock), 0, st, ev ? ev->first : nullptr, ev ? ev->second : nullptr, 0, a);
    HIP_TRY(c, hipGetLastError());
    if (!c->event_timing || ev) {
      int64_t nrec = 0;
      for (auto& v : s.recs) nrec += (int64_t)v.size();
      c->stat_algo_bytes += (12.0 + 4.0 * kMaxSets) * (double)nrec + (4.0 + 8.0 * n) * (double)n_reads;
      c->stat_launches++;
    }
  }
  return 0;
}

// after the route's wait: partials_out[(k * read sets + slot) * 4 ..] = {sum, floored, 0, reads} of path set k; the sets'
// bookkeeping as n sequential calls leave it (misses of every set, no bad bases, the per-read values of the last set)
int pacbio_chunk_collect(gaml_hip_ctx* c, PbChunk& ch, int n, double* partials_out) {
  if (c->pacbios.empty()) return 0;
  if (!ch.launched) return fail(c, GAML_HIP_ESTATE, "batch: the chunk's PacBio launch is missing");
  const size_t ns = c->handles.size();
  const std::vector<int> slot = slots_of_kind(c, 2);
  for (size_t j = 0; j < c->pacbios.size(); j++) {
    PacbioSet& s = *c->pacbios[j];
    const double* res = (const double*)s.multi.out.p;
    for (int k = 0; k < n; k++) memcpy(partials_out + ((size_t)k * ns + (size_t)slot[j]) * 4, res + 4 * k, 4 * sizeof(double));
    s.misses += ch.misses[j];
    s.last_bad_bases = 0;
    s.multi.launches++;
  }
  ch.collected = true;
  return 0;
}
