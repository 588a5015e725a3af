// pacbio_batch.hip.h -- the PacBio side of gaml_hip_calc_prob_batch's one-pass routes (paired_batch.hip.h): per chunk of up
// to kMaxSets path sets and per PacBio set one table of occurrence counts, one upload, one dispatch of
// pacbio_score_multi_kernel
// (one translation unit with gaml_hip.hip, which includes this file behind pacbio_launch.hip.h)
//
//   slots_of_kind         where combine() expects the partials of the sets of one kind (scoring_order)
//   PbChunk               a chunk's PacBio launches: what they would add to the bookkeeping, held back until the chunk stands
//   pacbio_chunk_launch   enumerate every path once (memo by path), build [sub-walk][kMaxSets], stage, launch
//   pacbio_chunk_sweep    a set with a coverage penalty (gaml_hip_set_pacbio_penalty_onepass): the chunk's paths that have no
//                         memoised bad_bases yet, one contig each, swept behind the scoring kernel
//   pacbio_chunk_collect  after the route's wait: the partials into their slots, the bookkeeping of n sequential calls
//
// A set with a penalty: CalcScoreForPacbio's bad_bases (graph.cc:3183-3251) is an integer sum over the paths of the call, and
// a path's events depend on the normalised path and the record cache alone -- what PbMulti::memo is keyed by. So PbEnum
// carries the path's value once a chunk has swept it, a chunk sweeps its distinct paths without one (one or two in an
// annealing run) and a set's bad_bases is the sum over its paths as listed. Contigs of up to kPbSweepCap intervals go one
// per block through pacbio_path_sweep_kernel, larger ones together through the chain of single calls (pacbio_sweep_run,
// adding per contig); both write one result array, pacbio_store_bad_kernel hands it to the host.
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
struct PbChunkSweep {  // a penalised set's side of the chunk: nothing of it reaches the memo or the counters before collect
  std::vector<PbEnum*> swept;  // the chunk's distinct paths without a value, in the order of the result array
  std::vector<std::vector<const PbEnum*>> set_paths;  // per path set its paths as listed (one listed three times counts three times)
  int64_t n_block = 0, n_chain = 0, n_memo = 0;  // contigs to the block-per-contig kernel / the general chain; distinct paths whose value the memo had
};
struct PbChunk {
  gaml_hip_ctx* c;
  bool launched = false, collected = false;
  std::vector<int64_t> misses;  // per PacBio set: lookups that missed, over all sets of the chunk
  std::vector<PbChunkSweep> sweep;  // per PacBio set (empty lists for one without a penalty)
  explicit PbChunk(gaml_hip_ctx* ctx) : c(ctx) {}
  ~PbChunk() { if (launched && !collected) (void)hipStreamSynchronize(c->stream); }
  PbChunk(const PbChunk&) = delete;
};

// The sweeps of a penalised set's chunk: `todo` are its distinct paths without a memoised value (memo entries: the key is the
// normalised path). Enqueued on `st`, nothing waits; the values land in PbMulti::bad_host in the order of sw.swept.
int pacbio_chunk_sweep(gaml_hip_ctx* c, PacbioSet& s, PbChunkSweep& sw, const std::vector<std::pair<const Walk*, PbEnum*>>& todo, hipStream_t st) {
  typedef unsigned long long u64;
  PbMulti& M = s.multi;
  if (todo.empty()) return 0;
  if (int e = pacbio_sweep_sync(c, s, st)) return e;
  const std::vector<int32_t>& iv_off = s.sweep.iv_off_host;
  const int64_t cap = GRID_CAPPED(c, PACBIO_SWEEP_CAP, kPbSweepCap);  // (the development build's knob only lowers it)
  // block-per-contig: headers | node intervals {begin, end} | occurrences; the general chain: pacbio_sweep_prepare's lists
  std::vector<PbPathHdr> hdr;
  std::vector<int32_t> node;
  std::vector<PbPathOcc> occ;
  std::vector<int32_t> chain_tl, chain_node;
  std::vector<PbOcc> chain_occ;
  std::vector<PbEnum*> chain_paths;
  std::vector<int32_t> nd;
  for (const auto& t : todo) {
    const Walk& path = *t.first;
    const PbEnum& en = *t.second;
    nd.clear();
    nd.push_back(-1000); nd.push_back(2000);  // the events (-1000, 1), (2000, -3000) of graph.cc:3198-3199
    int32_t pp = 0;
    for (int32_t x : path) {
      if (x >= 0) { const int32_t cl = c->g.len(x); if (cl > 0) { nd.push_back(pp); nd.push_back(pp + cl); } pp += cl; }  // graph.cc:3202-3210
      else pp += -x;
    }
    const int64_t n_node = (int64_t)nd.size() / 2;
    int64_t n_iv = n_node;
    for (const PbHit& h : en.hits) n_iv += iv_off[h.walk + 1] - iv_off[h.walk];
    if (n_iv <= cap) {
      PbPathHdr h;
      h.tl = en.len; h.node_off = (int32_t)(node.size() / 2); h.n_node = (int32_t)n_node; h.occ_off = (int32_t)occ.size(); h.n_occ = (int32_t)en.hits.size();
      h.n_iv = (int32_t)n_iv; h.out = (int32_t)hdr.size(); h.pad = 0;
      node.insert(node.end(), nd.begin(), nd.end());
      int32_t at = (int32_t)n_node;
      for (const PbHit& hit : en.hits) { occ.push_back(PbPathOcc{hit.walk, hit.begin, at, 0}); at += iv_off[hit.walk + 1] - iv_off[hit.walk]; }
      hdr.push_back(h);
      sw.swept.push_back(t.second);
    } else {
      const int32_t no = (int32_t)chain_tl.size();
      chain_tl.push_back(en.len);
      for (size_t q = 0; q < nd.size(); q += 2) { chain_node.push_back(no); chain_node.push_back(nd[q]); chain_node.push_back(nd[q + 1]); chain_node.push_back(0); }
      for (const PbHit& hit : en.hits) chain_occ.push_back(PbOcc{hit.walk, hit.begin, no, 0});
      chain_paths.push_back(t.second);
    }
  }
  sw.n_block = (int64_t)hdr.size();
  sw.n_chain = (int64_t)chain_paths.size();
  sw.swept.insert(sw.swept.end(), chain_paths.begin(), chain_paths.end());
  const size_t total = sw.swept.size();
  HIP_TRY(c, M.bad.reserve(total * sizeof(u64), st));
  if (total * sizeof(u64) > M.bad_host.cap) { HIP_TRY(c, hipStreamSynchronize(st)); HIP_TRY(c, M.bad_host.reserve(total * sizeof(u64))); }
  HIP_TRY(c, hipMemsetAsync(M.bad.p, 0, total * sizeof(u64), st));
  if (!hdr.empty()) {
    const size_t hdr_bytes = hdr.size() * sizeof(PbPathHdr), node_bytes = align16(node.size() * sizeof(int32_t)), occ_bytes = occ.size() * sizeof(PbPathOcc);
    const size_t bytes = hdr_bytes + node_bytes + occ_bytes;  // (whole 16-byte units: the copy kernel moves int4s)
    void* host = nullptr;
    const int slot = stage_acquire(c, s.stage, bytes, &host);
    if (slot < 0) return slot;
    memcpy(host, hdr.data(), hdr_bytes);
    memcpy((char*)host + hdr_bytes, node.data(), node.size() * sizeof(int32_t));
    if (occ_bytes) memcpy((char*)host + hdr_bytes + node_bytes, occ.data(), occ_bytes);
    HIP_TRY(c, M.sweep_in.reserve(bytes, st));
    if (int e = stage_upload(c, s.stage, slot, M.sweep_in.p, bytes, st)) return e;
    if (int e = stage_release(c, s.stage, slot, st)) return e;
    PbPathSweepArgs a;
    a.hdr = (const PbPathHdr*)M.sweep_in.p;
    a.node = (const int2*)((const char*)M.sweep_in.p + hdr_bytes); a.n_node_all = (int)(node.size() / 2);
    a.occ = (const PbPathOcc*)((const char*)M.sweep_in.p + hdr_bytes + node_bytes); a.n_occ_all = (int)occ.size();
    a.iv_off = s.sweep.iv_off.as<int>(); a.n_walks = (int)iv_off.size() - 1;
    a.iv = s.sweep.iv.as<int2>(); a.n_iv_all = iv_off.back();
    a.step = s.cfg.step;
    a.bad = M.bad.as<u64>(); a.n_bad = (int)total;
    hipLaunchKernelGGL(pacbio_path_sweep_kernel, dim3((unsigned)hdr.size()), dim3(256), 0, st, a);
    HIP_TRY(c, hipGetLastError());
  }
  if (!chain_paths.empty()) {
    int64_t n_own = 0;
    if (int e = pacbio_sweep_prepare(c, s, chain_tl, chain_node, chain_occ, st, &n_own)) return e;
    if (int e = pacbio_sweep_run(c, s, (int64_t)chain_node.size() / 4 + n_own, (int32_t)chain_tl.size(), st, nullptr, 1.0, M.bad.as<u64>() + hdr.size())) return e;
  }
  hipLaunchKernelGGL(pacbio_store_bad_kernel, dim3(1), dim3(256), 0, st, M.bad.as<u64>(), (u64*)M.bad_host.dev, (int)total);
  HIP_TRY(c, hipGetLastError());
  return 0;
}

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
  ch.sweep.clear();
  ch.sweep.resize(c->pacbios.size());
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
    const bool cov = s.cfg.penalty_constant > 0;  // (here only with the context's switch on: batch_fast_capable)
    PbChunkSweep& sw = ch.sweep[j];
    std::vector<std::pair<const Walk*, PbEnum*>> todo;  // distinct by memo entry: a path in several sets, or twice in one, is swept once
    std::unordered_set<const PbEnum*> seen;
    if (cov) sw.set_paths.resize((size_t)n);
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
        if (cov) {
          sw.set_paths[(size_t)k].push_back(&it->second);
          if (seen.insert(&it->second).second) {
            if (it->second.bad < 0) todo.emplace_back(&it->first, &it->second);
            else sw.n_memo++;
          }
        }
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
    if (n_reads == 0) {  // (what launch_pacbio leaves: four zeroes; the sweep does not depend on the reads)
      memset(M.out.p, 0, (size_t)kMaxSets * 4 * sizeof(double));
      if (cov) { if (int e = pacbio_chunk_sweep(c, s, sw, todo, st)) return e; }
      continue;
    }
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
    if (cov) { if (int e = pacbio_chunk_sweep(c, s, sw, todo, st)) return e; }
  }
  return 0;
}

// after the route's wait: partials_out[(k * read sets + slot) * 4 ..] = {sum, floored, 0, reads} of path set k; the sets'
// bookkeeping as n sequential calls leave it (misses of every set, the last set's bad bases, the per-read values of the last
// set). A penalised set: the swept values into the memo, set k's bad_bases = the sum over its paths; its counters move here.
int pacbio_chunk_collect(gaml_hip_ctx* c, PbChunk& ch, int n, double* partials_out) {
  if (c->pacbios.empty()) return 0;
  if (!ch.launched) return fail(c, GAML_HIP_ESTATE, "batch: the chunk's PacBio launch is missing");
  const size_t ns = c->handles.size();
  const std::vector<int> slot = slots_of_kind(c, 2);
  for (size_t j = 0; j < c->pacbios.size(); j++) {
    PacbioSet& s = *c->pacbios[j];
    const double* res = (const double*)s.multi.out.p;
    for (int k = 0; k < n; k++) memcpy(partials_out + ((size_t)k * ns + (size_t)slot[j]) * 4, res + 4 * k, 4 * sizeof(double));
    PbChunkSweep& sw = ch.sweep[j];
    const bool cov = !sw.set_paths.empty();
    if (cov) {
      const unsigned long long* got = (const unsigned long long*)s.multi.bad_host.p;
      for (size_t q = 0; q < sw.swept.size(); q++)
        if (got[q] > (unsigned long long)INT64_MAX) return fail(c, GAML_HIP_ESTATE, "batch: the PacBio coverage sweep refused a contig's lists");
      for (size_t q = 0; q < sw.swept.size(); q++) sw.swept[q]->bad = (int64_t)got[q];
    }
    s.misses += ch.misses[j];
    s.last_bad_bases = 0;
    for (int k = 0; k < n; k++) {
      int64_t bad = 0;
      if (cov) {
        for (const PbEnum* e : sw.set_paths[(size_t)k]) bad += e->bad;
        partials_out[((size_t)k * ns + (size_t)slot[j]) * 4 + 2] = (double)bad;  // (what store_bad_bases_kernel leaves a single call)
      }
      s.batch_bad.push_back(bad);
      s.last_bad_bases = bad;
    }
    if (cov) {
      s.multi.penalty_stats[0]++;
      s.multi.penalty_stats[1] += sw.n_block;
      s.multi.penalty_stats[2] += sw.n_chain;
      s.multi.penalty_stats[3] += sw.n_memo;
    }
    s.multi.launches++;
  }
  ch.collected = true;
  return 0;
}
