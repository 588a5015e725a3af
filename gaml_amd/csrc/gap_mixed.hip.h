// gap_mixed.hip.h -- the gap profile's device route (gap_profile.hip.h) for the read sets that are not paired: single-end sets
// and PacBio sets without a coverage penalty, where the context asks for it (gaml_hip_set_gap_mixed_device /
// GAML_HIP_GAP_MIXED=device, off by default).
// (one translation unit with gaml_hip.hip, which includes this file through gap_profile.hip.h)
//
// A single-end set: windows never span a gap (split_contigs), so every length registers and aligns the same windows and the
// choice between a direct entry and a list (build_occ_table) is the same; an occurrence's shift is stv + tl with tl running
// over ALL paths of the set, so a gap longer by d moves the shift of every occurrence whose visiting rank lies behind the
// gap -- the later paths' included -- and nothing else. The host builds ONE table (the base length's) per profile; region g
// of the set's arena is derived from it on the device.
// A PacBio set: gaps do not split a path there, a sub-walk's cache key holds the gap entry -len. Only sub-walks that contain
// the gap entry can differ between two lengths (their keys, and the growth cut-off on that length's coordinates); every other
// sub-walk is the same key at every length (those that start behind the gap begin d later, which only a coverage sweep would
// read: a penalised PacBio set keeps the context on the fallback). The edited path is enumerated ONCE per profile into a
// core, per length only the growths that reach the gap; the count table of a pass is core + patches, built on the device.
//
//   gap_single_tables_kernel   region g := the base table, shift + (lens[g] - base) in every entry of rank >= first_rank
//   gap_pacbio_counts_kernel   counts[w][k] := core[w] for the pass's columns, 0 behind them; then the pass's patches
//   pacbio_enumerate_gap_core / _len   the split enumeration; their sum is pacbio_enumerate's of the path with that length
//   GapMixed                   a profile's plan for these sets and what a pass holds back until it stands (SgChunk, PbChunk)
//   gap_mixed_plan / _launch / _collect   once per profile; per pass before the paired sets' work; per pass after the wait
#pragma once

namespace gaml {

struct GapSingleTabArgs {
  const char* base;      // the table of the set with the base length in the gap (layout_occ)
  char* regions;         // set g at regions + g * stride, laid out like the base table
  size_t stride;
  size_t off_direct, off_lo, bytes_lo, off_m;  // from `base` / from a region's start; all 16-byte aligned
  int n_direct, n_multi; // OccQuads: one per window / list entries
  int first_rank;        // visiting rank of the first occurrence behind the gap
  int n_sets;
  int delta[kMaxSets];   // set g: its gap length minus the base length
};

// grid (sets of this pass, parts of the table): one 16-byte load and store per OccQuad {shift, min_pos, path, rank}. A direct
// entry with path == -1 says "does not occur", one with rank < 0 points at a list (never >= first_rank, which is >= 0).
__global__ __launch_bounds__(256) void gap_single_tables_kernel(GapSingleTabArgs a) {
  const int g = (int)blockIdx.x;
  if (g >= a.n_sets) return;
  const int delta = a.delta[g];
  char* region = a.regions + (size_t)g * a.stride;
  const size_t first = (size_t)blockIdx.y * blockDim.x + threadIdx.x, step = (size_t)gridDim.y * blockDim.x;
  const int4* src = (const int4*)(a.base + a.off_direct);
  int4* dst = (int4*)(region + a.off_direct);
  for (size_t w = first; w < (size_t)a.n_direct; w += step) {
    int4 e = src[w];
    if (e.z >= 0 && e.w >= a.first_rank) e.x += delta;
    dst[w] = e;
  }
  const int4* src_m = (const int4*)(a.base + a.off_m);
  int4* dst_m = (int4*)(region + a.off_m);
  for (size_t q = first; q < (size_t)a.n_multi; q += step) {
    int4 e = src_m[q];
    if (e.w >= a.first_rank) e.x += delta;
    dst_m[q] = e;
  }
  if (blockIdx.y == 0) block_copy_words(region + a.off_lo, a.base + a.off_lo, a.bytes_lo);
}

struct GapPbPatch { int32_t walk, column, count, pad; };  // counts[walk][column] += count
struct GapPbCountArgs {
  const int* core;       // per sub-walk: its occurrences in what the lengths share
  int* counts;           // [sub-walk][kMaxSets]
  int n_walks, n_sets;
  const GapPbPatch* patches;
  int n_patches;
};

// One pass over the sub-walks, two 16-byte stores each. A patch is added by the block that wrote its row, behind a barrier:
// the row's stores have left the block's waves by then (__syncthreads waits for them), and no other block touches the row.
__global__ __launch_bounds__(256) void gap_pacbio_counts_kernel(GapPbCountArgs a) {
  const int bd = (int)blockDim.x;
  for (int w = (int)blockIdx.x * bd + (int)threadIdx.x; w < a.n_walks; w += (int)gridDim.x * bd) {
    const int c = a.core[w], n = a.n_sets;
    int4* row = (int4*)(a.counts + (size_t)w * kMaxSets);
    row[0] = make_int4(n > 0 ? c : 0, n > 1 ? c : 0, n > 2 ? c : 0, n > 3 ? c : 0);
    row[1] = make_int4(n > 4 ? c : 0, n > 5 ? c : 0, n > 6 ? c : 0, n > 7 ? c : 0);
  }
  __syncthreads();
  for (int t = (int)threadIdx.x; t < a.n_patches; t += bd) {
    const GapPbPatch p = a.patches[t];
    if (p.walk < 0 || p.walk >= a.n_walks || p.column < 0 || p.column >= a.n_sets) continue;
    if ((p.walk / bd) % (int)gridDim.x != (int)blockIdx.x) continue;
    atomicAdd(a.counts + (size_t)p.walk * kMaxSets + p.column, p.count);
  }
}
static_assert(kMaxSets == 8, "gap_pacbio_counts_kernel writes a row as two int4");

}  // namespace gaml

namespace {

// What the lengths of one gap share of a (normalised) path's enumeration: every lookup of a sub-walk that does not contain
// the gap entry, per start in the reference's order (hits of start i: hits[start_off[i] .. start_off[i + 1])), and the starts
// whose growth gets to the gap entry -- the start at the entry itself included.
struct PbGapCore {
  Walk path;                       // with the base length in the gap
  int32_t gap_pos = 0, base_len = 0;
  std::vector<int32_t> begins, ends;  // the base length's coordinates
  std::vector<PbHit> hits;
  std::vector<uint8_t> moves;      // per hit: it starts behind the gap, its begin moves with the length
  std::vector<int32_t> start_off;
  std::vector<int32_t> reach;
  int64_t misses = 0;
};
struct PbGapLen { std::vector<std::pair<int32_t, PbHit>> hits; int64_t misses = 0; };  // (start, hit), starts ascending

void pacbio_enumerate_gap_core(const gaml_hip_ctx* c, const PacbioSet& s, const Walk& path, int32_t gap_pos, PbGapCore& out) {
  const int32_t m = (int32_t)path.size();
  out.path = path; out.gap_pos = gap_pos; out.base_len = -path[(size_t)gap_pos];
  out.begins.assign((size_t)m, 0); out.ends.assign((size_t)m, 0);
  out.hits.clear(); out.moves.clear(); out.reach.clear(); out.misses = 0;
  out.start_off.assign((size_t)m + 1, 0);
  int32_t len = 0;
  for (int32_t i = 0; i < m; i++) {
    out.begins[i] = len;
    len += path[i] < 0 ? -path[i] : c->g.len(path[i]);
    out.ends[i] = len;
  }
  Walk sub;
  for (int32_t i = 0; i < m; i++) {
    out.start_off[i] = (int32_t)out.hits.size();
    if (i == gap_pos) { out.reach.push_back(i); continue; }  // every sub-walk from here holds the entry
    sub.clear();
    bool reached = false;
    for (int32_t j = i; j < m; j++) {
      if (i < gap_pos && j == gap_pos) { reached = true; break; }
      sub.push_back(path[j]);
      auto it = s.walk_id.find(sub);
      if (it == s.walk_id.end()) out.misses++;
      else { out.hits.push_back(PbHit{it->second, out.begins[i]}); out.moves.push_back(i > gap_pos ? 1 : 0); }
      if (out.ends[j] - out.ends[i] > s.max_len) break;  // (both ends on the same side of the gap: no length in it)
    }
    if (reached) out.reach.push_back(i);
  }
  out.start_off[m] = (int32_t)out.hits.size();
}

// the growths that reach the gap, with `len` in it: the reference's cut-off on that length's coordinates (a start in front
// of the gap sees the span grow by len - base_len, the start at the entry sees both ends move alike)
void pacbio_enumerate_gap_len(const PacbioSet& s, const PbGapCore& core, int32_t len, PbGapLen& out) {
  out.hits.clear(); out.misses = 0;
  const int32_t m = (int32_t)core.path.size(), gp = core.gap_pos, d = len - core.base_len;
  Walk sub;
  for (int32_t i : core.reach) {
    sub.assign(core.path.begin() + i, core.path.begin() + gp);
    for (int32_t j = gp; j < m; j++) {
      sub.push_back(j == gp ? -len : core.path[j]);
      auto it = s.walk_id.find(sub);
      if (it == s.walk_id.end()) out.misses++;
      else out.hits.emplace_back(i, PbHit{it->second, core.begins[i]});
      if ((int64_t)(core.ends[j] - core.ends[i]) + (i < gp ? d : 0) > (int64_t)s.max_len) break;
    }
  }
}

// core + one length's part as pacbio_enumerate lists them
void pacbio_gap_assemble(const PbGapCore& core, const PbGapLen& part, int32_t len, PbEnum& out) {
  out.hits.clear();
  const int32_t m = (int32_t)core.path.size(), d = len - core.base_len;
  size_t at = 0;
  for (int32_t i = 0; i < m; i++) {
    for (int32_t q = core.start_off[i]; q < core.start_off[i + 1]; q++) out.hits.push_back(PbHit{core.hits[q].walk, core.hits[q].begin + (core.moves[q] ? d : 0)});
    for (; at < part.hits.size() && part.hits[at].first == i; at++) out.hits.push_back(part.hits[at].second);
  }
  out.misses = core.misses + part.misses;
  out.len = (m ? core.ends[m - 1] : 0) + d;
  out.bad = -1;
}

// development build: the split enumeration against the whole one, on every call
int pacbio_gap_check(gaml_hip_ctx* c, const PacbioSet& s, const PbGapCore& core, const PbGapLen& part, int32_t len) {
  PbEnum got, want;
  pacbio_gap_assemble(core, part, len, got);
  Walk whole = core.path;
  whole[(size_t)core.gap_pos] = -len;
  pacbio_enumerate(c, s, whole, want);
  bool same = got.misses == want.misses && got.len == want.len && got.hits.size() == want.hits.size();
  for (size_t q = 0; same && q < got.hits.size(); q++) same = got.hits[q].walk == want.hits[q].walk && got.hits[q].begin == want.hits[q].begin;
  if (!same) return fail(c, GAML_HIP_ESTATE, "gap profile: the split PacBio enumeration differs from the whole one");
  return 0;
}

struct GapMixed {
  gaml_hip_ctx* c;
  int32_t base_len = 0;
  bool in_flight = false;  // a pass is launched and not collected: nothing of it has reached the sets' bookkeeping
  // (occ_len: the gap length SingleSet::last_occ stands at)
  struct Sg { int32_t tl0 = 0, occ_len = 0; int first_rank = 0; OccLayout lay; int n_direct = 0, n_multi = 0; size_t bytes_lo = 0; int64_t table_bytes = 0; };
  struct Pb { PbGapCore core; int64_t shared_misses = 0, pass_misses = 0; size_t n_walks = 0; };
  std::vector<Sg> sg;
  std::vector<Pb> pb;
  explicit GapMixed(gaml_hip_ctx* ctx) : c(ctx) {}
  ~GapMixed() { if (in_flight) (void)hipStreamSynchronize(c->stream); }
  GapMixed(const GapMixed&) = delete;
  bool any() const { return !sg.empty() || !pb.empty(); }
};

constexpr size_t kGapSingleArenaMax = (size_t)1 << 30;  // base table + regions of one single-end set

// Once per profile, after eval_begin (c->pending_paths: the path set with the base length). Returns 1 when a set cannot go
// this way (nothing has reached a set's bookkeeping: the fallback takes the profile), < 0 on an error.
int gap_mixed_plan(gaml_hip_ctx* c, GapMixed& mx, int32_t path_id, int32_t gap_pos, int32_t base_len, int chunk, hipStream_t st) {
  mx.base_len = base_len;
  if (c->singles.empty() && c->pacbios.empty()) return 0;
  if (!c->pending_paths_valid || (size_t)path_id >= c->pending_paths.size()) return fail(c, GAML_HIP_ESTATE, "gap profile: the path set is not at hand");
  const std::vector<Walk>& paths = c->pending_paths;
  // where the first occurrence behind the gap starts, in a single-end set's coordinates (stv + tl: prepare_single_host)
  int64_t behind = (int64_t)path_id * 1000000 + base_len;
  for (int32_t p = 0; p < path_id; p++) behind += walk_length(c->g, paths[(size_t)p]);
  for (int32_t q = 0; q < gap_pos; q++) { const int32_t x = paths[(size_t)path_id][(size_t)q]; behind += x < 0 ? -(int64_t)x : c->g.len(x); }
  mx.sg.resize(c->singles.size());
  for (size_t j = 0; j < c->singles.size(); j++) {
    SingleSet& s = *c->singles[j];
    GapMixed::Sg& r = mx.sg[j];
    if (int e = single_init_dev(c, s)) return e;
    std::vector<Occ> occs;
    if (int e = prepare_single_host(c, s, paths, occs, &r.tl0)) return e;
    r.first_rank = 0; r.occ_len = base_len;
    for (const Occ& o : occs) if ((int64_t)o.shift < behind) r.first_rank++;  // (shifts ascend in visiting order)
    OccTable occ;
    build_occ_table(s.mate.wins.size(), occs, occ);
    r.lay = layout_occ(occ, 0);
    r.n_direct = (int)occ.direct.size(); r.n_multi = (int)occ.multi.size(); r.bytes_lo = occ.multi_off.size() * sizeof(int32_t);
    const size_t total = r.lay.end * ((size_t)chunk + 1);
    if (total > kGapSingleArenaMax) return 1;  // (the regions would outgrow what one set's arena may take)
    if (int e = single_sync_records(c, s, st)) return e;
    void* host = nullptr;
    const int slot = stage_acquire(c, s.stage, r.lay.end, &host);
    if (slot < 0) return slot;
    pack_occ(occ, r.lay, (char*)host);
    if (total > s.occ_arena.cap) { HIP_TRY(c, hipStreamSynchronize(st)); HIP_TRY(c, s.occ_arena.reserve(total)); }
    if (int e = stage_upload(c, s.stage, slot, s.occ_arena.p, r.lay.end, st)) return e;
    if (int e = stage_release(c, s.stage, slot, st)) return e;
    r.table_bytes = (int64_t)r.lay.end;
    SgMulti& M = s.multi;
    if (!M.ticket.p) {
      HIP_TRY(c, M.part_sum.reserve((size_t)kMaxSets * kMaxBlocks * sizeof(double)));
      HIP_TRY(c, M.part_zero.reserve((size_t)kMaxSets * kMaxBlocks * sizeof(int)));
      HIP_TRY(c, M.out.reserve((size_t)kMaxSets * 4 * sizeof(double)));
      HIP_TRY(c, M.ticket.reserve(kTicketWords * sizeof(unsigned)));
      HIP_TRY(c, hipMemset(M.ticket.p, 0, kTicketWords * sizeof(unsigned)));
      HIP_TRY(c, hipDeviceSynchronize());  // the scoring stream is non-blocking: make the zeroes land first
    }
  }
  mx.pb.resize(c->pacbios.size());
  Walk path;
  for (size_t j = 0; j < c->pacbios.size(); j++) {
    PacbioSet& s = *c->pacbios[j];
    PbMulti& M = s.multi;
    GapMixed::Pb& r = mx.pb[j];
    if (int e = pacbio_init_dev(c, s)) return e;
    if (M.memo_generation != s.generation || M.memo.size() > 8192) { M.memo.clear(); M.memo_generation = s.generation; }
    r.n_walks = s.recs.size();
    const size_t bytes = align16(std::max<size_t>(1, r.n_walks) * sizeof(int32_t));
    void* host = nullptr;
    const int slot = stage_acquire(c, s.stage, bytes, &host);
    if (slot < 0) return slot;
    int32_t* core = (int32_t*)host;
    memset(core, 0, bytes);
    r.shared_misses = 0;
    for (size_t p = 0; p < paths.size(); p++) {
      path = paths[p];
      for (auto& x : path) if (x >= 0) x = c->g.norm[x];  // NormalizePath graph.h:268-273
      if ((int32_t)p == path_id) {
        pacbio_enumerate_gap_core(c, s, path, gap_pos, r.core);
        r.shared_misses += r.core.misses;
        for (const PbHit& h : r.core.hits) core[h.walk]++;
        continue;
      }
      auto it = M.memo.find(path);  // the other paths: as a batch's chunk finds them
      if (it == M.memo.end()) {
        it = M.memo.emplace(path, PbEnum()).first;
        pacbio_enumerate(c, s, path, it->second);
      }
      r.shared_misses += it->second.misses;
      for (const PbHit& h : it->second.hits) core[h.walk]++;
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
    // the resident column follows the record cache and the path set: written once per profile
    const size_t count_bytes = align16(std::max<size_t>(1, r.n_walks) * kMaxSets * sizeof(int32_t));
    if (bytes > s.gap_core.cap || count_bytes > M.count.cap) {
      HIP_TRY(c, hipStreamSynchronize(st));
      HIP_TRY(c, s.gap_core.reserve(bytes));
      HIP_TRY(c, M.count.reserve(count_bytes));
    }
    if (int e = stage_upload(c, s.stage, slot, s.gap_core.p, bytes, st)) return e;
    if (int e = stage_release(c, s.stage, slot, st)) return e;
    s.gap_core_generation = s.generation;
  }
  return 0;
}

// Per pass of n lengths, before the paired sets' work of the pass: the PacBio sets' launches, then the single-end sets', as
// a batch's chunk orders them. Nothing reaches the sets' bookkeeping before gap_mixed_collect.
int gap_mixed_launch(gaml_hip_ctx* c, GapMixed& mx, const int32_t* lens, int n, hipStream_t st) {
  if (!mx.any()) return 0;
  for (size_t j = 0; j < c->pacbios.size(); j++) {
    PacbioSet& s = *c->pacbios[j];
    PbMulti& M = s.multi;
    GapMixed::Pb& r = mx.pb[j];
    const int64_t n_reads = s.hi - s.lo;
    // this pass's patches: the sub-walks that contain the gap entry, per length; equal (sub-walk, column) pairs folded
    std::vector<GapPbPatch> patches;
    PbGapLen part;
    r.pass_misses = 0;
    for (int k = 0; k < n; k++) {
      pacbio_enumerate_gap_len(s, r.core, lens[k], part);
#ifdef GAML_HIP_DEV
      if (int e = pacbio_gap_check(c, s, r.core, part, lens[k])) return e;
#endif
      r.pass_misses += r.shared_misses + part.misses;
      const size_t first = patches.size();
      for (const auto& h : part.hits) {
        size_t q = first;
        while (q < patches.size() && patches[q].walk != h.second.walk) q++;
        if (q < patches.size()) patches[q].count++;
        else patches.push_back(GapPbPatch{h.second.walk, k, 1, 0});
      }
    }
    const GapPbPatch* dev_patches = nullptr;
    if (!patches.empty()) {
      void* host = nullptr;
      const int slot = stage_acquire(c, s.stage, patches.size() * sizeof(GapPbPatch), &host);
      if (slot < 0) return slot;
      memcpy(host, patches.data(), patches.size() * sizeof(GapPbPatch));
      dev_patches = (const GapPbPatch*)s.stage.slot[slot].dev;  // (few entries: the kernel reads the pinned slot itself, like stage_copy_kernel)
      if (int e = stage_release(c, s.stage, slot, st)) return e;
    }
    mx.in_flight = true;
    GapPbCountArgs ca;
    ca.core = s.gap_core.as<int>(); ca.counts = M.count.as<int>();
    ca.n_walks = (int)r.n_walks; ca.n_sets = n;
    ca.patches = dev_patches; ca.n_patches = (int)patches.size();
    const unsigned cgrid = (unsigned)std::max<size_t>(1, std::min<size_t>(256, (r.n_walks + 255) / 256));
    hipLaunchKernelGGL(gap_pacbio_counts_kernel, dim3(cgrid), dim3(256), 0, st, ca);
    HIP_TRY(c, hipGetLastError());
    s.gap_cols = n;
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
  for (size_t j = 0; j < c->singles.size(); j++) {
    SingleSet& s = *c->singles[j];
    SgMulti& M = s.multi;
    GapMixed::Sg& r = mx.sg[j];
    const size_t stride = r.lay.end;
    GapSingleTabArgs ta;
    memset(&ta, 0, sizeof(ta));
    ta.base = (const char*)s.occ_arena.p; ta.regions = (char*)s.occ_arena.p + stride; ta.stride = stride;
    ta.off_direct = r.lay.direct; ta.off_lo = r.lay.multi_off; ta.bytes_lo = r.bytes_lo; ta.off_m = r.lay.multi;
    ta.n_direct = r.n_direct; ta.n_multi = r.n_multi; ta.first_rank = r.first_rank; ta.n_sets = n;
    for (int k = 0; k < n; k++) ta.delta[k] = lens[k] - mx.base_len;
    // a block per 2048 entries of the larger list and per length; one block per length is the floor
    const size_t most = (size_t)std::max(r.n_direct, r.n_multi);
    const unsigned parts = (unsigned)std::max<size_t>(1, std::min<size_t>(64, (most + 2047) / 2048));
    mx.in_flight = true;
    hipLaunchKernelGGL(gap_single_tables_kernel, dim3((unsigned)n, parts), dim3(256), 0, st, ta);
    HIP_TRY(c, hipGetLastError());
    s.gap_tab = SingleSet::GapTab{n, stride, stride, r.lay.direct, r.lay.multi_off, r.lay.multi, r.n_direct, (int)(r.bytes_lo / sizeof(int32_t)), r.n_multi};
    const int64_t n_reads = s.mate.n_local();
    if (n_reads == 0) { memset(M.out.p, 0, (size_t)kMaxSets * 4 * sizeof(double)); continue; }  // (what launch_single leaves: four zeroes)
    SingleMultiArgs a;
    OccLayout reg = r.lay;
    const MateView v0 = view_of(s.dev, (const char*)s.occ_arena.p, reg);
    a.first = v0.first; a.extra = v0.extra; a.mism_pow = v0.mism_pow; a.match_pow = v0.match_pow;
    a.lens = s.lens.as<int>();
    a.floor_tab = s.tabs.as<double>();
    a.logfloor_tab = s.tabs.as<double>() + s.mate.max_len + 1;
    a.n = (int)n_reads; a.n_sets = n;
    for (int k = 0; k < kMaxSets; k++) {  // (the slots behind n_sets repeat the last set's: never read)
      const int g = std::min(k, n - 1);
      const MateView v = view_of(s.dev, (const char*)s.occ_arena.p + stride * (size_t)(g + 1), reg);
      a.occ[k] = v.occ; a.multi_off[k] = v.multi_off; a.multi[k] = v.multi;
      const int64_t t = (int64_t)r.tl0 + (lens[g] - mx.base_len);
      a.two_T[k] = (double)(2 * std::max<int64_t>(1, t));
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
      c->stat_algo_bytes += 16.0 * (double)s.rm.total_records + (double)(stride * (size_t)n) + 12.0 * (double)n_reads;
      c->stat_launches++;
    }
  }
  return 0;
}

// after the pass's wait: partials_out[(k * read sets + slot) * 4 ..] = {sum, floored, 0, reads} of length k, and the sets'
// bookkeeping as n sequential calls leave it (pacbio_chunk_collect, single_chunk_collect); last_len: the pass's last length
void gap_mixed_collect(gaml_hip_ctx* c, GapMixed& mx, int n, int32_t last_len, double* partials_out) {
  if (!mx.any()) return;
  const size_t ns = c->handles.size();
  const std::vector<int> pslot = slots_of_kind(c, 2), sslot = slots_of_kind(c, 0);
  for (size_t j = 0; j < c->pacbios.size(); j++) {
    PacbioSet& s = *c->pacbios[j];
    const double* res = (const double*)s.multi.out.p;
    for (int k = 0; k < n; k++) memcpy(partials_out + ((size_t)k * ns + (size_t)pslot[j]) * 4, res + 4 * k, 4 * sizeof(double));
    s.misses += mx.pb[j].pass_misses;  // (of every length scored, those scored ahead of the search included)
    s.last_bad_bases = 0;
    s.multi.launches++;
  }
  for (size_t j = 0; j < c->singles.size(); j++) {
    SingleSet& s = *c->singles[j];
    const double* res = (const double*)s.multi.out.p;
    for (int k = 0; k < n; k++) memcpy(partials_out + ((size_t)k * ns + (size_t)sslot[j]) * 4, res + 4 * k, 4 * sizeof(double));
    s.table_bytes = mx.sg[j].table_bytes;
    s.multi.launches++;
    // the occurrence list a call with the pass's last length leaves (prepare_single_host left the base length's)
    const int32_t d = last_len - mx.sg[j].occ_len;
    if (d != 0) for (Occ& o : s.last_occ) if (o.rank >= mx.sg[j].first_rank) o.shift += d;
    mx.sg[j].occ_len = last_len;
  }
  mx.in_flight = false;
}

}  // namespace

#ifdef GAML_HIP_DEV
extern "C" {

int64_t gaml_hip_debug_gap_single_table(gaml_hip_ctx* c, int rs, int g, int32_t* out5, int64_t cap) {
  if (!c || c->multi || rs < 0 || rs >= (int)c->handles.size() || c->handles[rs].kind != 0 || c->device < 0) return -1;
  SingleSet& s = *c->singles[c->handles[rs].idx];
  const SingleSet::GapTab& G = s.gap_tab;
  if (g < 0 || g >= G.n || !s.occ_arena.p) return -1;  // no mixed device pass yet, or the pass had no region g
  if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return -1;
  const char* region = (const char*)s.occ_arena.p + G.region0 + (size_t)g * G.stride;
  std::vector<OccQuad> direct((size_t)std::max(1, G.n_direct)), multi((size_t)std::max(1, G.n_multi));
  std::vector<int32_t> lo((size_t)std::max(1, G.n_lo));
  if (G.n_direct && hipMemcpy(direct.data(), region + G.off_direct, (size_t)G.n_direct * sizeof(OccQuad), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (G.n_lo && hipMemcpy(lo.data(), region + G.off_lo, (size_t)G.n_lo * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (G.n_multi && hipMemcpy(multi.data(), region + G.off_m, (size_t)G.n_multi * sizeof(OccQuad), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  std::vector<Occ> v;
  for (int32_t w = 0; w < G.n_direct; w++) {
    const OccQuad& e = direct[(size_t)w];
    if (e.path < 0) continue;
    if (e.rank >= 0) { v.push_back(Occ{w, e.shift, e.min_pos, e.path, e.rank}); continue; }
    const int32_t list = -e.rank - 1;
    if (list + 1 >= G.n_lo) return -1;
    for (int32_t q = lo[(size_t)list]; q < lo[(size_t)list + 1] && q < G.n_multi; q++) v.push_back(Occ{w, multi[(size_t)q].shift, multi[(size_t)q].min_pos, multi[(size_t)q].path, multi[(size_t)q].rank});
  }
  std::sort(v.begin(), v.end(), [](const Occ& a, const Occ& b) { return a.rank < b.rank; });
  for (int64_t i = 0; i < (int64_t)v.size() && i < cap; i++) {
    const Occ& o = v[(size_t)i];
    out5[5 * i] = o.wid; out5[5 * i + 1] = o.shift; out5[5 * i + 2] = o.min_pos; out5[5 * i + 3] = o.path; out5[5 * i + 4] = o.rank;
  }
  return (int64_t)v.size();
}

int64_t gaml_hip_debug_gap_pacbio_counts(gaml_hip_ctx* c, int rs, int g, int32_t* out, int64_t cap) {
  if (!c || c->multi || rs < 0 || rs >= (int)c->handles.size() || c->handles[rs].kind != 2 || c->device < 0) return -1;
  PacbioSet& s = *c->pacbios[c->handles[rs].idx];
  if (s.gap_cols <= 0 || g < 0 || g >= kMaxSets || !s.multi.count.p) return -1;  // no mixed device pass yet
  if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return -1;
  const size_t n_walks = s.recs.size();
  std::vector<int32_t> table(std::max<size_t>(1, n_walks) * kMaxSets);
  if (n_walks && hipMemcpy(table.data(), s.multi.count.p, n_walks * kMaxSets * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  for (int64_t w = 0; w < (int64_t)n_walks && w < cap; w++) out[w] = table[(size_t)w * kMaxSets + (size_t)g];
  return (int64_t)n_walks;
}

int64_t gaml_hip_debug_pacbio_gap_enum(gaml_hip_ctx* c, int rs, const int32_t* path, int32_t path_len, int32_t gap_pos, int32_t len,
                                        int32_t* hits_out, int64_t cap, int64_t* misses_out) {
  if (!c || c->multi || rs < 0 || rs >= (int)c->handles.size() || c->handles[rs].kind != 2 || !c->have_graph) return -1;
  if (!path || path_len <= 0 || gap_pos < 0 || gap_pos >= path_len || path[gap_pos] >= 0 || len < 1) return -1;
  for (int32_t q = 0; q < path_len; q++) if (path[q] >= c->g.n()) return -1;
  const PacbioSet& s = *c->pacbios[c->handles[rs].idx];
  Walk p(path, path + path_len);
  for (auto& x : p) if (x >= 0) x = c->g.norm[x];
  PbGapCore core;
  PbGapLen part;
  PbEnum en;
  pacbio_enumerate_gap_core(c, s, p, gap_pos, core);
  pacbio_enumerate_gap_len(s, core, len, part);
  if (pacbio_gap_check(c, s, core, part, len)) return -2;  // (gaml_hip_last_error says so)
  pacbio_gap_assemble(core, part, len, en);
  for (int64_t i = 0; i < (int64_t)en.hits.size() && i < cap; i++) { hits_out[2 * i] = en.hits[(size_t)i].walk; hits_out[2 * i + 1] = en.hits[(size_t)i].begin; }
  if (misses_out) *misses_out = en.misses;
  return (int64_t)en.hits.size();
}

}  // extern "C"
#endif
